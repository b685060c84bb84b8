// Device-side transform body shared by the FFT kernels (kern_fft.hip) and the long
// overlap-save FIR (kern_fir_ols_long.hip): the complex helpers and the Stockham
// autosort passes on an LDS-resident power-of-two transform.
#pragma once
#include <hip/hip_runtime.h>

namespace sdsp {

template <typename T> struct c2 { T re, im; };
template <typename T> __device__ __forceinline__ c2<T> ca(c2<T> a, c2<T> b) { return {a.re + b.re, a.im + b.im}; }
template <typename T> __device__ __forceinline__ c2<T> cs(c2<T> a, c2<T> b) { return {a.re - b.re, a.im - b.im}; }
template <typename T> __device__ __forceinline__ c2<T> cm(c2<T> a, c2<T> b) {
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
template <typename T, bool INV> __device__ __forceinline__ c2<T> twl(const c2<T>* __restrict__ tw, int m) {
    c2<T> w = tw[m];
    if constexpr (INV) w.im = -w.im;
    return w;
}
template <typename T, bool INV> __device__ __forceinline__ c2<T> rot(c2<T> a) {  // *(-j) fwd, *(+j) inv
    if constexpr (INV) return {-a.im, a.re};
    else return {a.im, -a.re};
}

// Stockham passes on an LDS transform `a` (natural order in), result in `a` or
// `b` (returned).  `lane` in [0, nthr), nthr threads cooperate on this transform.
template <typename T, bool INV>
__device__ c2<T>* stockham(c2<T>* a, c2<T>* b, int N, int logN, const c2<T>* __restrict__ tw, int lane, int nthr) {
    int Ns = 1;
    if (logN & 1) {  // one radix-2 pass
        for (int j = lane; j < N / 2; j += nthr) {
            const c2<T> v0 = a[j], v1 = a[j + N / 2];
            // Ns = 1: no twiddle
            b[2 * j] = ca(v0, v1);
            b[2 * j + 1] = cs(v0, v1);
        }
        __syncthreads();
        c2<T>* t = a; a = b; b = t;
        Ns = 2;
    }
    for (; Ns < N; Ns *= 4) {
        for (int j = lane; j < N / 4; j += nthr) {
            const int k = j % Ns;
            const int stride = N / (Ns * 4);  // twiddle index step
            c2<T> v0 = a[j], v1 = a[j + N / 4], v2 = a[j + N / 2], v3 = a[j + 3 * (N / 4)];
            if (Ns > 1) {
                v1 = cm(v1, twl<T, INV>(tw, (1 * k * stride) & (N - 1)));
                v2 = cm(v2, twl<T, INV>(tw, (2 * k * stride) & (N - 1)));
                v3 = cm(v3, twl<T, INV>(tw, (3 * k * stride) & (N - 1)));
            }
            const c2<T> s02 = ca(v0, v2), d02 = cs(v0, v2), s13 = ca(v1, v3), d13 = rot<T, INV>(cs(v1, v3));
            const int o = (j / Ns) * Ns * 4 + k;
            b[o] = ca(s02, s13);
            b[o + Ns] = ca(d02, d13);
            b[o + 2 * Ns] = cs(s02, s13);
            b[o + 3 * Ns] = cs(d02, d13);
        }
        __syncthreads();
        c2<T>* t = a; a = b; b = t;
    }
    return a;
}

}  // namespace sdsp

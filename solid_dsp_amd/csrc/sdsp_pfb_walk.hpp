// The three polyphase-filterbank / interpolator kernels and their selection rule, shared by
// kern_pfb.hip and the up-converter's kern_duc.hip: kernel templates with a store hook as their
// last template parameter, instantiated by the unit that launches them.
//
// Every finished dot product passes through a store hook on its way out: hook.at(acc, o) with o
// the output's index within its channel (as u32, wrapping).  StoreIdentity returns it as it is
// (kern_pfb.hip: its generated code is that of the kernels before the hook existed);
// StoreNcoMix multiplies it by the oscillator's phasor at theta0 + o dtheta.  hook.stage() runs
// once per workgroup, by every thread, before a workgroup barrier that precedes the first at().
#pragma once
#include "sdsp_device.hpp"
#include "sdsp_kernels.hpp"
#include "sdsp_nco_dev.hpp"

namespace sdsp {

struct StoreIdentity {
    static constexpr bool kIdentity = true;
    struct Args {};  // what the launch passes; the kernel builds its hook from it
    __device__ __forceinline__ explicit StoreIdentity(Args) {}
    __device__ __forceinline__ void stage() const {}
    // the barrier after stage() in a walk that has none of its own
    __device__ __forceinline__ void barrier() const {}
    template <typename I> __device__ __forceinline__ I at(I v, uint32_t) const { return v; }
};

// NCO mix on store: v * phasor(theta0 + o dtheta), the phase formed as nco_one does (u32, wrapping)
template <typename T> struct StoreNcoMix {
    struct Args {
        const double* table;  // the handle's f64 sine table
        uint32_t theta0, dtheta;
        bool down;
    };
    static constexpr bool kIdentity = false;
    T* lut;  // LDS, 1024 entries
    const double* table;
    uint32_t theta0, dtheta;
    bool down;
    // one table per workgroup: the constructor is inlined into the kernel, once
    __device__ __forceinline__ explicit StoreNcoMix(Args a)
        : table(a.table), theta0(a.theta0), dtheta(a.dtheta), down(a.down) {
        __shared__ T lut_lds[1024];
        lut = lut_lds;
    }
    __device__ __forceinline__ void stage() const {
        for (int i = threadIdx.x; i < 1024; i += blockDim.x) lut[i] = (T)table[i];
    }
    __device__ __forceinline__ void barrier() const { __syncthreads(); }
    __device__ __forceinline__ cpx<T> at(cpx<T> v, uint32_t o) const {
        return nco_mix_at(lut, v, theta0 + o * dtheta, down);
    }
};

template <typename I>
__device__ inline I pfb_ext(const I* __restrict__ x, const I* __restrict__ hist, long long j, int H) {
    if (j >= 0) return x[j];
    const long long h = (long long)H + j;
    return h >= 0 ? hist[h] : zero_v<I>();
}

// One lane per output, the fallback for very long branches.
template <typename C, typename I, bool EXACT, typename Hook>
__global__ void __launch_bounds__(256)
pfb_kernel(const I* __restrict__ x, const I* __restrict__ hist, const C* __restrict__ cb, I* __restrict__ y,
           long long n, int K, int M, int H, typename Hook::Args ha) {
    const Hook hook(ha);
    const int ch = blockIdx.y;
    x += (long long)ch * n;
    hist += (long long)ch * H;
    const long long total = n * M;
    y += (long long)ch * total;
    hook.stage();
    hook.barrier();
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += stride) {
        const long long j = o / M;
        const int p = (int)(o - j * M);
        const C* c = cb + (long long)p * K;
        I acc = zero_v<I>();
        for (int i = 0; i < K; ++i) acc = mac<EXACT>(acc, c[i], pfb_ext(x, hist, j - i, H));
        y[o] = hook.at(acc, (uint32_t)o);
    }
}

// Staged form for every other shape: a 256-lane workgroup owns T consecutive
// inputs of one channel (T M ~ 4096 outputs); the T + K - 1 samples they need
// and (when they fit) the M K branch coefficients are staged once in LDS with
// coalesced loads, then the lanes walk the tile's outputs in order (stores
// contiguous across the workgroup), each the reference dot product
// sum_{i<K} cb[p][i] x[j-i] in the reference order -- where pfb_kernel above
// re-reads K samples and K coefficients from global memory per output and
// divides 64-bit indices.
constexpr int kPfbStageBytes = 48 * 1024;

template <typename C, typename I, bool EXACT, bool CB_LDS, typename Hook>
__global__ void __launch_bounds__(256)
pfb_stage_kernel(const I* __restrict__ x, const I* __restrict__ hist, const C* __restrict__ cb, I* __restrict__ y,
                 long long n, int K, int M, int H, int T, typename Hook::Args ha) {
    const Hook hook(ha);
    extern __shared__ __attribute__((aligned(16))) unsigned char pfb_lds[];
    I* xs = reinterpret_cast<I*>(pfb_lds);  // xs[s] = x[j0 - K + 1 + s]
    const int ch = blockIdx.y;
    x += (long long)ch * n;
    hist += (long long)ch * H;
    y += (long long)ch * n * M;
    const long long j0 = (long long)blockIdx.x * T;
    const int nt = n - j0 < T ? (int)(n - j0) : T;
    const int ns = nt + K - 1;
    const C* cbs = cb;
    if constexpr (CB_LDS) {
        C* c = reinterpret_cast<C*>(pfb_lds + ((size_t)(T + K - 1) * sizeof(I) + 15) / 16 * 16);
        for (int i = threadIdx.x; i < M * K; i += 256) c[i] = cb[i];
        cbs = c;
    }
    const long long base = j0 - K + 1;
    if (base >= 0) {
        for (int i = threadIdx.x; i < ns; i += 256) xs[i] = x[base + i];
    } else {
        for (int i = threadIdx.x; i < ns; i += 256) xs[i] = pfb_ext(x, hist, base + i, H);
    }
    hook.stage();
    __syncthreads();
    const unsigned um = (unsigned)M, total = (unsigned)nt * um;
    I* yt = y + j0 * M;
    const uint32_t o0 = (uint32_t)j0 * um;  // the tile's first output, mod 2^32
    for (unsigned o = threadIdx.x; o < total; o += 256) {
        const unsigned j = o / um, p = o - j * um;
        const C* c = cbs + (size_t)p * K;
        const I* w = xs + j + K - 1;  // w[-i] = x[j0 + j - i]
        I acc = zero_v<I>();
        for (int i = 0; i < K; ++i) acc = mac<EXACT>(acc, c[i], w[-i]);
        // (the identity is spelt out: through at() the c64 instances named their two zeroed
        // accumulator registers the other way round)
        if constexpr (Hook::kIdentity) yt[o] = acc;
        else yt[o] = hook.at(acc, o0 + o);
    }
}

// Tiled form for M = 2^m (8 <= M <= 512) and K in {4, 8, 16}: the interpolator
// shape (InterpolatingFIRFilter::execute_block, one input in, M outputs out).
// A 256-lane workgroup owns T = 16 * 512 / M consecutive inputs of one channel
// (XCD-ordered: each XCD streams one contiguous stretch of the output).  Lane
// (g, q) -- q = 0 .. M/2-1 a pair of branches (2q, 2q + 1), g = 0 .. 512/M - 1
// a run of R = 16 inputs -- keeps its 2K branch coefficients and the R + K - 1
// samples its run needs in registers (staged once through LDS, read as
// wave-broadcasts) and writes its 2R outputs as 16-byte stores: for one input
// the M/2 lanes of a run cover M contiguous outputs.  Every output is the
// reference dot product sum_{i<K} cb[p][i] x[j-i] in the reference order.
constexpr int kInterpR = 16;

template <typename I> struct alignas(2 * sizeof(I)) Pair {
    I a, b;
};

template <typename C, typename I, bool EXACT, int K, typename Hook>
__global__ void __launch_bounds__(256)
interp_tile_kernel(const I* __restrict__ x, const I* __restrict__ hist, const C* __restrict__ cb,
                   I* __restrict__ y, long long n, int M, int H, long long q8, typename Hook::Args ha) {
    const Hook hook(ha);
    constexpr int R = kInterpR;
    __shared__ I xs[1024 + 16];  // T + K - 1 <= 16 * 64 + 15 samples (M >= 8)
    const int ch = blockIdx.y;
    const int xc = blockIdx.x & 7;
    const long long tile = (long long)xc * q8 + (blockIdx.x >> 3);
    const int P = M >> 1, G = 256 / P, T = G * R;
    const long long j0 = tile * T;
    if (j0 >= n) return;  // uniform
    x += (long long)ch * n;
    hist += (long long)ch * H;
    y += (long long)ch * n * M;
    const int t = threadIdx.x;
    // stage x[j0 - K + 1, j0 + T) (zero past n, history before 0)
    for (int i = t; i < T + K - 1; i += 256) {
        const long long j = j0 - (K - 1) + i;
        xs[i] = j < n ? pfb_ext(x, hist, j, H) : zero_v<I>();
    }
    const int g = t / P, q = t - g * P;
    C c0[K], c1[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        c0[i] = cb[(long long)(2 * q) * K + i];
        c1[i] = cb[(long long)(2 * q + 1) * K + i];
    }
    hook.stage();
    __syncthreads();
    I w[R + K - 1];  // w[m] = x[jg - K + 1 + m], jg = j0 + g R
#pragma unroll
    for (int m = 0; m < R + K - 1; ++m) w[m] = xs[g * R + m];
    const long long jg = j0 + (long long)g * R;
    I* yo = y + jg * M + 2 * q;
    const uint32_t og = (uint32_t)jg * (uint32_t)M + 2u * (uint32_t)q;  // yo's output index, mod 2^32
#pragma unroll
    for (int r = 0; r < R; ++r) {
        I a0 = zero_v<I>(), a1 = zero_v<I>();
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const I s = w[r + K - 1 - i];  // x[jg + r - i]
            a0 = mac<EXACT>(a0, c0[i], s);
            a1 = mac<EXACT>(a1, c1[i], s);
        }
        if (jg + r < n) {
            const uint32_t o = og + (uint32_t)r * (uint32_t)M;
            store_nt(reinterpret_cast<Pair<I>*>(yo + (long long)r * M), Pair<I>{hook.at(a0, o), hook.at(a1, o + 1)});
        }
    }
}

template <typename I>
bool interp_tile_applies(const PfbArgs& a) {
    return a.M >= 8 && a.M <= 512 && (a.M & (a.M - 1)) == 0 && (a.K == 4 || a.K == 8 || a.K == 16) &&
           a.H == a.K && ((uintptr_t)a.y % (2 * sizeof(I))) == 0;
}

// The kernel-selection rule of launch_pfb, for the kernels instantiated with `Hook`.
template <typename C, typename I, typename Hook>
hipError_t pfb_route(const PfbArgs& a, typename Hook::Args ha, hipStream_t s) {
    if (interp_tile_applies<I>(a)) {
        const int P = a.M / 2, T = (256 / P) * kInterpR;
        const long long tiles = ((long long)a.n + T - 1) / T;
        const long long q8 = (tiles + 7) / 8;
        if (8 * q8 > 0x7fffffffLL) return hipErrorInvalidValue;
        const dim3 grid((unsigned)(8 * q8), (unsigned)a.channels);
#define SDSP_INTERP(EX, KK)                                                                                      \
    hipLaunchKernelGGL((interp_tile_kernel<C, I, EX, KK, Hook>), grid, dim3(256), 0, s, (const I*)a.x,           \
                       (const I*)a.hist, (const C*)a.cb, (I*)a.y, (long long)a.n, a.M, a.H, q8, ha)
#define SDSP_INTERP_K(KK)                                                                                        \
    if (a.K == KK) {                                                                                             \
        if (a.exact) SDSP_INTERP(true, KK); else SDSP_INTERP(false, KK);                                         \
        return hipGetLastError();                                                                                \
    }
        SDSP_INTERP_K(4)
        SDSP_INTERP_K(8)
        SDSP_INTERP_K(16)
#undef SDSP_INTERP_K
#undef SDSP_INTERP
        return hipErrorInvalidValue;
    }
#ifndef SDSP_PFB_LAB  // lab builds keep the per-output kernel for A/B (tools/lab.mk)
    {
        const int T = a.M >= 4096 ? 1 : 4096 / a.M;
        const size_t xb = ((size_t)(T + a.K - 1) * sizeof(I) + 15) / 16 * 16, cbb = (size_t)a.M * a.K * sizeof(C);
        if (xb <= kPfbStageBytes && (unsigned long long)T * a.M < (1ULL << 31)) {
            const bool cb_lds = xb + cbb <= kPfbStageBytes;
            const size_t lds = xb + (cb_lds ? cbb : 0);
            dim3 g((unsigned)((a.n + T - 1) / T), (unsigned)a.channels);
#define SDSP_PFB_STAGE(EX, CBL)                                                                                  \
    hipLaunchKernelGGL((pfb_stage_kernel<C, I, EX, CBL, Hook>), g, dim3(256), lds, s, (const I*)a.x,             \
                       (const I*)a.hist, (const C*)a.cb, (I*)a.y, (long long)a.n, a.K, a.M, a.H, T, ha)
            if (a.exact) {
                if (cb_lds) SDSP_PFB_STAGE(true, true); else SDSP_PFB_STAGE(true, false);
            } else {
                if (cb_lds) SDSP_PFB_STAGE(false, true); else SDSP_PFB_STAGE(false, false);
            }
#undef SDSP_PFB_STAGE
            return hipGetLastError();
        }
    }
#endif
    const long long total = (long long)a.n * a.M;
    long long blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    dim3 grid((unsigned)blocks, (unsigned)a.channels);
    if (a.exact)
        hipLaunchKernelGGL((pfb_kernel<C, I, true, Hook>), grid, dim3(256), 0, s, (const I*)a.x, (const I*)a.hist,
                           (const C*)a.cb, (I*)a.y, (long long)a.n, a.K, a.M, a.H, ha);
    else
        hipLaunchKernelGGL((pfb_kernel<C, I, false, Hook>), grid, dim3(256), 0, s, (const I*)a.x, (const I*)a.hist,
                           (const C*)a.cb, (I*)a.y, (long long)a.n, a.K, a.M, a.H, ha);
    return hipGetLastError();
}

}  // namespace sdsp

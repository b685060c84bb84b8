// Overlap-save FIR for long filters (3841 < L - 1 <= 2^20) on 32-bit complex samples (gfx950).
//
// One segment transform of N = N1 N2 points per V = N - (L-1) outputs, N1 = 2^floor(log2 N / 2),
// in three passes over a scratch `tmp` of [segments][N1][N2] c32 samples (a plain four-step
// forward, product, four-step inverse would take five passes, a gather and a scatter).  With
// n = n2 + N2 n1 the segment input index, k = k1 + N1 k2 the spectrum index, m = m2 + N2 m1 the
// segment output index and w[i] = ext(s V - (L-1) + i) the window of segment s:
//
//   P1  A[k1][n2] = W_N^(n2 k1) sum_n1 w[n2 + N2 n1] W_N1^(n1 k1)           -> tmp[s][k1][n2]
//       (the window gather is this pass's load)
//   P2  per row (s, k1), in place: FFT over n2 (X[k1 + N1 k2]), times the filter spectrum
//       G[k1][k2], inverse FFT over k2, times W_N^(-k1 m2)                  -> tmp[s][k1][m2]
//       (the inverse is split the mirrored way, so its first pass runs on the row the
//       forward's second pass leaves in LDS)
//   P3  y_seg[m2 + N2 m1] = sum_k1 tmp[s][k1][m2] W_N1^(-k1 m1), stored to
//       y[s V + m - (L-1)] where m >= L-1 and the position is inside the block.
//
// P1 and P3 take C adjacent columns per workgroup, so their global accesses are runs of C
// consecutive samples.  The inter-pass twiddles W_N^(+-a b) come from f64 sincospi of the exact
// phase, as in fft_pass_kernel (kern_fft.hip); the N1- and N2-point transforms are the LDS
// Stockham passes of sdsp_fft_dev.hpp with f64-computed tables.  The spectrum G holds
// scale / N (ols_tables.cpp ols_long_spectrum).  Channels are folded into the segment index.
#include "sdsp_device.hpp"
#include "sdsp_fft_dev.hpp"
#include "sdsp_kernels.hpp"

namespace sdsp {

namespace {

using cf = c2<float>;

struct LongGeom {
    int logN, l1, l2;
    int lc;    // log2 of the columns per workgroup (P1, P3)
    int nthr;  // threads per transform
    int pad;   // P1, P3: elements of padding after the two N1-point buffers of a column
    int Lm1;
    long long n, V, nseg;  // samples per channel, outputs per segment, segments per channel
};

// the stream extended by the history (last L-1 inputs, oldest first) and by zeros past the
// block (ext_load of kern_fir_direct.hip)
__device__ __forceinline__ cf ext(const cf* __restrict__ x, const cf* __restrict__ hist, long long j, long long n,
                                  int Lm1) {
    if (j >= 0) return j < n ? x[j] : cf{0.0f, 0.0f};
    const long long h = (long long)Lm1 + j;
    return h >= 0 ? hist[h] : cf{0.0f, 0.0f};
}

// W_N^(m) forward, W_N^(-m) inverse, m already reduced mod N
template <bool INV> __device__ __forceinline__ cf wn(int m, int logN) {
    double sn, cs;
    sincospi((INV ? 2.0 : -2.0) * (double)m / (double)(1 << logN), &sn, &cs);
    return cf{(float)cs, (float)sn};
}

// P1: grid (N2 / C, segments of the round), block C * nthr
__global__ void __launch_bounds__(1024)
ols_long_p1_kernel(const cf* __restrict__ x, const cf* __restrict__ hist, cf* __restrict__ tmp,
                   const cf* __restrict__ tw1, LongGeom g, long long seg0) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    cf* buf = reinterpret_cast<cf*>(lds_raw);
    const int N1 = 1 << g.l1, N2 = 1 << g.l2, C = 1 << g.lc, Nm = (1 << g.logN) - 1;
    const int tid = threadIdx.x, nth = blockDim.x, tot = C * N1, cst = 2 * N1 + g.pad;
    const int c0 = blockIdx.x * C;
    const long long gs = seg0 + blockIdx.y, ch = gs / g.nseg, sidx = gs - ch * g.nseg;
    x += ch * g.n;
    hist += ch * g.Lm1;
    const long long base = sidx * g.V - g.Lm1 + c0;  // stream position of window sample c0
    for (int e = tid; e < tot; e += nth) {
        const int c = e & (C - 1), n1 = e >> g.lc;
        buf[c * cst + n1] = ext(x, hist, base + c + (long long)N2 * n1, g.n, g.Lm1);
    }
    __syncthreads();
    cf* a = buf + (tid / g.nthr) * cst;
    cf* r = stockham<float, false>(a, a + N1, N1, g.l1, tw1, tid % g.nthr, g.nthr);
    const int roff = (int)(r - a);  // 0 or N1, the same for every column
    cf* out = tmp + (size_t)blockIdx.y * ((size_t)Nm + 1) + c0;
    for (int e = tid; e < tot; e += nth) {
        const int c = e & (C - 1), k1 = e >> g.lc;
        out[(size_t)k1 * N2 + c] = cm(buf[c * cst + roff + k1], wn<false>(((c0 + c) * k1) & Nm, g.logN));
    }
}

// P2: grid (N1 / R, segments of the round), block R * nthr; R rows per workgroup
__global__ void __launch_bounds__(1024)
ols_long_p2_kernel(cf* __restrict__ tmp, const cf* __restrict__ G, const cf* __restrict__ tw2, LongGeom g) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    cf* buf = reinterpret_cast<cf*>(lds_raw);
    const int N2 = 1 << g.l2, Nm = (1 << g.logN) - 1;
    const int sub = threadIdx.x / g.nthr, lane = threadIdx.x % g.nthr;
    const int k1 = blockIdx.x * (blockDim.x / g.nthr) + sub;
    cf* row = tmp + (size_t)blockIdx.y * ((size_t)Nm + 1) + (size_t)k1 * N2;
    const cf* Gr = G + (size_t)k1 * N2;
    cf* a = buf + (size_t)sub * 2 * N2;
    for (int i = lane; i < N2; i += g.nthr) a[i] = row[i];
    __syncthreads();
    cf* r = stockham<float, false>(a, a + N2, N2, g.l2, tw2, lane, g.nthr);  // r[k2] = X[k1 + N1 k2]
    cf* o = r == a ? a + N2 : a;
    for (int i = lane; i < N2; i += g.nthr) r[i] = cm(r[i], Gr[i]);
    __syncthreads();
    const cf* q = stockham<float, true>(r, o, N2, g.l2, tw2, lane, g.nthr);
    for (int i = lane; i < N2; i += g.nthr) row[i] = cm(q[i], wn<true>((k1 * i) & Nm, g.logN));
}

// P3: grid (N2 / C, segments of the round), block C * nthr
__global__ void __launch_bounds__(1024)
ols_long_p3_kernel(const cf* __restrict__ tmp, cf* __restrict__ y, const cf* __restrict__ tw1, LongGeom g,
                   long long seg0) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    cf* buf = reinterpret_cast<cf*>(lds_raw);
    const int N1 = 1 << g.l1, N2 = 1 << g.l2, C = 1 << g.lc, Nm = (1 << g.logN) - 1;
    const int tid = threadIdx.x, nth = blockDim.x, tot = C * N1, cst = 2 * N1 + g.pad;
    const int c0 = blockIdx.x * C;
    const long long gs = seg0 + blockIdx.y, ch = gs / g.nseg, sidx = gs - ch * g.nseg;
    y += ch * g.n;
    const cf* in = tmp + (size_t)blockIdx.y * ((size_t)Nm + 1) + c0;
    for (int e = tid; e < tot; e += nth) {
        const int c = e & (C - 1), k1 = e >> g.lc;
        buf[c * cst + k1] = in[(size_t)k1 * N2 + c];
    }
    __syncthreads();
    cf* a = buf + (tid / g.nthr) * cst;
    cf* r = stockham<float, true>(a, a + N1, N1, g.l1, tw1, tid % g.nthr, g.nthr);
    const int roff = (int)(r - a);
    const long long o0 = sidx * g.V - g.Lm1 + c0;  // block position of segment output m = c0
    for (int e = tid; e < tot; e += nth) {
        const int c = e & (C - 1), m1 = e >> g.lc;
        const long long m = c0 + c + (long long)N2 * m1, pos = o0 + c + (long long)N2 * m1;
        if (m >= g.Lm1 && pos < g.n) y[pos] = buf[c * cst + roff + m1];
    }
}

}  // namespace

size_t ols_long_segments(size_t n, int log2n, int Lm1) {
    const size_t V = ((size_t)1 << log2n) - (size_t)Lm1;
    return (n + V - 1) / V;
}

hipError_t launch_fir_ols_long(const OlsLongPlan& p, const void* x, const void* hist, void* y, void* tmp, size_t n,
                               size_t channels, size_t segs_per_round, hipStream_t s) {
    if (n == 0 || channels == 0) return hipSuccess;
    LongGeom g{};
    g.logN = p.log2n;
    g.l1 = p.log2n / 2;
    g.l2 = p.log2n - g.l1;
    const int N1 = 1 << g.l1, N2 = 1 << g.l2;
    // columns per workgroup, two N1-point LDS buffers each, in at most 128 KB; one element of
    // padding per column where it fits, so that lanes on consecutive columns hit different banks
    const int C = N1 <= 256 ? 16 : N1 <= 1024 ? 8 : 4;
    g.lc = __builtin_ctz(C);
    g.pad = (size_t)C * (2 * N1 + 1) * sizeof(cf) <= 128 * 1024 ? 1 : 0;
    g.Lm1 = p.Lm1;
    g.n = (long long)n;
    g.V = ((long long)1 << p.log2n) - p.Lm1;
    g.nseg = (long long)ols_long_segments(n, p.log2n, p.Lm1);
    const long long total = g.nseg * (long long)channels;
    if (segs_per_round < 1) segs_per_round = 1;
    // P1 / P3: N1 / 4 threads per column, at most 1024 per workgroup
    int nthr13 = N1 / 4;
    while (nthr13 * C > 1024) nthr13 /= 2;
    const size_t lds13 = (size_t)C * (2 * N1 + g.pad) * sizeof(cf);
    // P2: N2 / 4 threads per row, R rows in 512 threads at most
    const int nthr2 = N2 / 4;
    int R = 2048 / N2 < 8 ? 2048 / N2 : 8;
    if (R < 1) R = 1;
    const size_t lds2 = (size_t)R * 2 * N2 * sizeof(cf);
    for (long long seg0 = 0; seg0 < total; seg0 += (long long)segs_per_round) {
        const unsigned S = (unsigned)(total - seg0 < (long long)segs_per_round ? total - seg0 : segs_per_round);
        g.nthr = nthr13;
        hipLaunchKernelGGL(ols_long_p1_kernel, dim3(N2 / C, S), dim3(C * nthr13), lds13, s, (const cf*)x,
                           (const cf*)hist, (cf*)tmp, (const cf*)p.d_tw1, g, seg0);
        g.nthr = nthr2;
        hipLaunchKernelGGL(ols_long_p2_kernel, dim3(N1 / R, S), dim3(R * nthr2), lds2, s, (cf*)tmp,
                           (const cf*)p.d_G, (const cf*)p.d_tw2, g);
        g.nthr = nthr13;
        hipLaunchKernelGGL(ols_long_p3_kernel, dim3(N2 / C, S), dim3(C * nthr13), lds13, s, (const cf*)tmp, (cf*)y,
                           (const cf*)p.d_tw1, g, seg0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sdsp

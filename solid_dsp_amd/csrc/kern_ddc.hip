// Digital down-converter (gfx950): the NCO's mix-down on the load path of the decimating FIR.
//
// A DDC handle is by definition the composition, sample for sample,
//     v = nco.mix_down(x[i]); nco.step(); decimator.push/execute(v)
// (src/nco/mod.rs:94-172 into src/filter/fir/decim.rs:115-118, 221-228).  The oscillator is a pure
// function of the sample's index in the call, theta_0 + i * dtheta mod 2^32, so the mixed stream is
// never written: each kernel here multiplies a sample by its phasor between the load and the
// sample's first use.  Stream traffic is the decimator's own, 8 + 8/M bytes per c32 input; the
// only addition is the f32 / f64 copy of the 1024-entry sine table each workgroup stages in LDS
// (4 / 8 KB).  The delay line holds mixed samples, so samples that come from the history are not
// mixed again.
//
// Shared or copied: the polyphase walk (sdsp_decim_walk.hpp) is shared with kern_decim.hip, which
// instantiates it with the identity hook (its generated code unchanged); here the hook is
// LoadNcoMix.  The reference-order walk below is a copy of kern_fir_direct.hip's decimator
// kernels with the hook added: routing the existing kernels through a shared body changed their
// instruction schedule, so they keep their own text.
//   * FMA, L = K*M with K in {2,4,8,16} and an M-sample row of 32..256 bytes, M >= 8: the
//     column-parallel polyphase walk (poly_group), with its wave-uniform interior / edge split, XCD
//     order, nontemporal 16-byte interior loads and `seg`.  The table is staged after the first
//     loads are issued, so no workgroup leaves before that barrier: a lane group past the last
//     output walks zero outputs instead of returning.
//   * EXACT, and FMA shapes outside the above: the reference-order walk (decim_direct_body, or
//     decim_global_body for tiles beyond LDS).  The mix is nco_one's product (num-complex
//     roundings, this unit is built with -ffp-contract=off) and the sum the literal left-to-right
//     one, so EXACT is bit-identical to the NCO handle followed by the EXACT decimator.
//   * ddc_hist_kernel: the next history, the last L-1 samples of (old history ++ mixed block).
//
// The direction is a run-time flag (mix_up differs by one conjugate, a sign flip of the sine).
#include "sdsp_decim_walk.hpp"
#include "sdsp_device.hpp"
#include "sdsp_kernels.hpp"
#include "sdsp_nco_dev.hpp"

namespace sdsp {

namespace {

// ---------------------------------------------------------------- reference-order walk
// A copy of decim_direct_kernel / decim_global_kernel (and their tile rule) of kern_fir_direct.hip
// with the load hook added.  A change to either copy belongs in both.
constexpr int kDirectThreads = 256;
constexpr int kStageU = 16;  // staging loads in flight per lane (32 or 40 measured slower)

// extended stream: history (last L-1 samples, oldest first) then x
template <typename I>
__device__ inline I ext_load(const I* __restrict__ x, const I* __restrict__ hist, long long j, long long n, int Lm1) {
    if (j >= 0) return j < n ? x[j] : zero_v<I>();
    long long h = (long long)Lm1 + j;
    return h >= 0 ? hist[h] : zero_v<I>();
}

// Decimating FIR: output m sits at block-relative input index j_m = j0 + m*M
// (DecimatingFIRFilter::push advances the phase, emission when it wraps to 0,
// src/filter/fir/decim.rs:115-118,221-228).
//   y[m] = (sum_{i<L} cr[i] * ext(j_m - i)) * scale
// Tap i = k*M + p.  LDS row rho holds the M samples ext(j_{m0} + (rho-K+1)*M - p),
// p = 0..M-1, so lane u reads row u-k+K-1 left to right for tap group k — the
// reference order — and lanes hit rows 16 bytes apart in bank space.
template <typename C, typename I, bool EXACT, typename Hook>
__device__ __forceinline__ void decim_direct_body(const I* __restrict__ x, const I* __restrict__ hist,
                                                  const C* __restrict__ cr, C scale, I* __restrict__ y, long long n,
                                                  long long nout, int L, int M, long long j0, int T,
                                                  const Hook& hook) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int ch = blockIdx.y;
    x += (long long)ch * n;
    y += (long long)ch * nout;
    hist += (long long)ch * (L - 1);
    const int K = (L + M - 1) / M;
    const int rowBytes = M * (int)sizeof(I) + 16;
    const int rows = T + K - 1;
    const long long m0 = (long long)blockIdx.x * T;
    const long long jm0 = j0 + m0 * M;
    const int tid = threadIdx.x;
    hook.stage();

    // stage: interior tiles read the contiguous inputs x[base + f] with kStageU loads in
    // flight per lane (f -> row f / M, slot M-1 - f % M); edge tiles go through ext_load
    const long long base = jm0 - (long long)(K - 1) * M - (M - 1);
    const int total = rows * M;
    if (base >= 0 && base + total <= n) {
        for (int f0 = 0; f0 < total; f0 += kStageU * (int)blockDim.x) {
            I v[kStageU];
#pragma unroll
            for (int u = 0; u < kStageU; ++u) {
                const int f = f0 + u * (int)blockDim.x + tid;
                if (f < total) v[u] = x[base + f];
            }
#pragma unroll
            for (int u = 0; u < kStageU; ++u) {
                const int f = f0 + u * (int)blockDim.x + tid;
                if (f < total) {
                    const int rho = f / M, q = f - rho * M;
                    *reinterpret_cast<I*>(lds + rho * rowBytes + (M - 1 - q) * (int)sizeof(I)) =
                        hook.template at<false>(v[u], base, f);
                }
            }
        }
    } else {
        for (int f = tid; f < total; f += blockDim.x) {
            const int rho = f / M, p = f - rho * M;
            const long long j = jm0 + (long long)(rho - K + 1) * M - p;
            *reinterpret_cast<I*>(lds + rho * rowBytes + p * (int)sizeof(I)) =
                hook.template at<true>(ext_load(x, hist, j, n, L - 1), j, 0);
        }
    }
    __syncthreads();
    const long long m = m0 + tid;
    if (tid >= T || m >= nout) return;
    I acc = zero_v<I>();
    for (int k = 0; k < K; ++k) {
        const I* row = reinterpret_cast<const I*>(lds + (tid - k + K - 1) * rowBytes);
        const C* ck = cr + k * M;
        const int pe = min(M, L - k * M);
        // unrolled so that a run of LDS reads is in flight before the (ordered) sums
        // consume it; the summation order is unchanged
        if (pe == M) {
#pragma unroll 16
            for (int p = 0; p < M; ++p) acc = mac<EXACT>(acc, ck[p], row[p]);
        } else {
#pragma unroll 16
            for (int p = 0; p < pe; ++p) acc = mac<EXACT>(acc, ck[p], row[p]);
        }
    }
    y[m] = mul_(acc, scale);
}

// Same arithmetic with no LDS tile (very large M*L tiles).
template <typename C, typename I, bool EXACT, typename Hook>
__device__ __forceinline__ void decim_global_body(const I* __restrict__ x, const I* __restrict__ hist,
                                                  const C* __restrict__ cr, C scale, I* __restrict__ y, long long n,
                                                  long long nout, int L, int M, long long j0, const Hook& hook) {
    const int ch = blockIdx.y;
    x += (long long)ch * n;
    y += (long long)ch * nout;
    hist += (long long)ch * (L - 1);
    hook.stage();
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nout) return;
    const long long jm = j0 + m * M;
    I acc = zero_v<I>();
    for (int i = 0; i < L; ++i)
        acc = mac<EXACT>(acc, cr[i], hook.template at<true>(ext_load(x, hist, jm - i, n, L - 1), jm - i, 0));
    y[m] = mul_(acc, scale);
}

// outputs (= lanes) per workgroup of decim_direct_body: the largest multiple of 64 whose LDS rows
// fit in 40 KB, so that several workgroups per CU overlap their staging and sums; *lds receives
// the tile's bytes (above `cap`: the caller takes decim_global_body)
inline int decim_direct_tile(int L, int M, size_t sample_bytes, size_t cap, size_t* lds) {
    const int K = (L + M - 1) / M;
    const size_t rowBytes = (size_t)M * sample_bytes + 16;
    int T = kDirectThreads;
    while (T > 64 && (size_t)(T + K - 1) * rowBytes > 40 * 1024) T -= 64;
    if ((size_t)(T + K - 1) * rowBytes > cap) T = 64;
    *lds = (size_t)(T + K - 1) * rowBytes;
    return T;
}

// ---------------------------------------------------------------- kernels
template <typename C, typename T, int M, int K, int V>
__global__ void __launch_bounds__(kPolyThreads)
ddc_poly_kernel(const cpx<T>* __restrict__ x, const cpx<T>* __restrict__ hist, const C* __restrict__ cr, C scale,
                cpx<T>* __restrict__ y, long long n, long long nout, long long j0, long long seg,
                const double* __restrict__ table, uint32_t theta0, uint32_t dtheta, bool down) {
    using I = cpx<T>;
    using Geo = PolyGeom<I, M, K, V>;
    constexpr int G = Geo::G, CH = Geo::CH, MV = Geo::MV;
    constexpr int L = K * M;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ T lut[1024];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane / MV, q = lane % MV;
    const int ch = blockIdx.y;
    x += (long long)ch * n;
    y += (long long)ch * nout;
    hist += (long long)ch * (L - 1);

    const long long wave_id = (long long)xcd_order(blockIdx.x, gridDim.x) * kPolyWaves + wave;  // XCD-ordered
    const long long gid = wave_id * G + g;
    // a group past the last output walks no outputs (its one warm-up step reads zeros through the
    // bounds-checked edge path) and still meets the workgroup's barrier in hook.stage()
    const long long m_begin = gid * seg < nout ? gid * seg : nout;
    const long long m_end = m_begin + seg < nout ? m_begin + seg : nout;

    C tap[K][V];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int e = 0; e < V; ++e) tap[k][e] = cr[k * M + (M - 1 - (q * V + e))];

    const LoadNcoMix<T> hook{lut, table, theta0, dtheta, down};
    char* tile = lds + (wave * G + g) * CH * Geo::RB;
    // wave-uniform interior test over all groups of this wave (rows warm-up .. last chunk); a wave
    // with a group past the last output fails it: j0 + nout*M >= n
    const long long first_j = j0 - (M - 1) + (wave_id * G * seg - K) * M;
    const long long last_row = (wave_id * G + G - 1) * seg + (seg + CH - 1) / CH * CH - 1;
    const long long last_j = j0 + last_row * M;
    if (first_j >= 0 && last_j < n)
        poly_group<C, I, M, K, V, true>(x, hist, tap, scale, y, tile, n, L - 1, j0, m_begin, m_end, q, hook);
    else
        poly_group<C, I, M, K, V, false>(x, hist, tap, scale, y, tile, n, L - 1, j0, m_begin, m_end, q, hook);
}

template <typename C, typename T, bool EXACT>
__global__ void __launch_bounds__(kDirectThreads)
ddc_direct_kernel(const cpx<T>* __restrict__ x, const cpx<T>* __restrict__ hist, const C* __restrict__ cr, C scale,
                  cpx<T>* __restrict__ y, long long n, long long nout, int L, int M, long long j0, int Tl,
                  const double* __restrict__ table, uint32_t theta0, uint32_t dtheta, bool down) {
    __shared__ T lut[1024];
    decim_direct_body<C, cpx<T>, EXACT>(x, hist, cr, scale, y, n, nout, L, M, j0, Tl,
                                        LoadNcoMix<T>{lut, table, theta0, dtheta, down});
}

template <typename C, typename T, bool EXACT>
__global__ void __launch_bounds__(kDirectThreads)
ddc_global_kernel(const cpx<T>* __restrict__ x, const cpx<T>* __restrict__ hist, const C* __restrict__ cr, C scale,
                  cpx<T>* __restrict__ y, long long n, long long nout, int L, int M, long long j0,
                  const double* __restrict__ table, uint32_t theta0, uint32_t dtheta, bool down) {
    __shared__ T lut[1024];
    decim_global_body<C, cpx<T>, EXACT>(x, hist, cr, scale, y, n, nout, L, M, j0,
                                        LoadNcoMix<T>{lut, table, theta0, dtheta, down});
}

// new_hist[k] = ext(n - (L-1) + k), k in [0, L-1): samples of the call mixed, old entries shifted
template <typename T>
__global__ void __launch_bounds__(256)
ddc_hist_kernel(const cpx<T>* __restrict__ x, const cpx<T>* __restrict__ old_hist, cpx<T>* __restrict__ new_hist,
                long long n, int Lm1, const double* __restrict__ table, uint32_t theta0, uint32_t dtheta,
                bool down) {
    __shared__ T lut[1024];
    const LoadNcoMix<T> hook{lut, table, theta0, dtheta, down};
    hook.stage();
    const int ch = blockIdx.y;
    x += (long long)ch * n;
    old_hist += (long long)ch * Lm1;
    new_hist += (long long)ch * Lm1;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < Lm1; k += gridDim.x * blockDim.x) {
        const long long j = n - Lm1 + k;
        new_hist[k] = j >= 0 ? hook.template at<false>(x[j], j, 0) : old_hist[Lm1 + j];
    }
}

template <typename C, typename T, int M, int K, int V>
hipError_t launch_ddc_poly_t(const DdcArgs& d, hipStream_t s) {
    using I = cpx<T>;
    using Geo = PolyGeom<I, M, K, V>;
    const FirArgs& a = d.fir;
    const long long nout = (long long)a.nout;
    const long long seg = poly_seg(a.seg, nout, Geo::CH);
    const long long groups = (nout + seg - 1) / seg;
    const long long waves = (groups + Geo::G - 1) / Geo::G;
    dim3 grid((unsigned)((waves + kPolyWaves - 1) / kPolyWaves), (unsigned)a.channels);
    const size_t lds = (size_t)kPolyWaves * Geo::LDS_WAVE;
    const C scale = *reinterpret_cast<const C*>(a.scale);
    hipLaunchKernelGGL((ddc_poly_kernel<C, T, M, K, V>), grid, dim3(kPolyThreads), lds, s, (const I*)a.x,
                       (const I*)a.hist, (const C*)a.taps_rev, scale, (I*)a.y, (long long)a.n, nout,
                       (long long)a.j0, seg, d.table, d.theta0, d.dtheta, d.down);
    return hipGetLastError();
}

template <typename C, typename T, int M, int K>
hipError_t ddc_poly_by_v(const DdcArgs& d, hipStream_t s) {
    constexpr int VW = 16 / (int)sizeof(cpx<T>);
    // complex taps at K = 16: with two columns per lane the 64 tap registers, the two 16-row
    // vectors and the mix do not fit 512 registers (232-264 bytes of scratch per lane, where the
    // decimator's kernel has none), so these shapes take one sample per lane, which fits
    constexpr bool kTwoColumns = VW > 1 && !(is_cpx<C>::value && K == 16);
    if constexpr (kTwoColumns) {
        // 16-byte rows: every row start j0 - (M-1) + rho*M a multiple of VW, and 16-byte
        // aligned channel bases
        const FirArgs& a = d.fir;
        const bool aligned = (a.j0 + 1) % VW == 0 && (a.channels == 1 || a.n % VW == 0) &&
                             reinterpret_cast<uintptr_t>(a.x) % 16 == 0;
        if (aligned) return launch_ddc_poly_t<C, T, M, K, VW>(d, s);
    }
    return launch_ddc_poly_t<C, T, M, K, 1>(d, s);
}

template <typename C, typename T, int M>
bool ddc_poly_by_k(const DdcArgs& d, hipStream_t s, hipError_t* err) {
    switch (d.fir.L / M) {
        case 2: *err = ddc_poly_by_v<C, T, M, 2>(d, s); return true;
        case 4: *err = ddc_poly_by_v<C, T, M, 4>(d, s); return true;
        case 8: *err = ddc_poly_by_v<C, T, M, 8>(d, s); return true;
        case 16: *err = ddc_poly_by_v<C, T, M, 16>(d, s); return true;
    }
    return false;
}

// the decimator's own shape rule (kern_decim.hip): an M-sample row of 32..256 bytes
template <typename C, typename T>
bool ddc_poly_by_m(const DdcArgs& d, hipStream_t s, hipError_t* err) {
    constexpr int sz = (int)sizeof(cpx<T>);
    switch (d.fir.M) {
        case 8: if constexpr (8 * sz <= 256) return ddc_poly_by_k<C, T, 8>(d, s, err); break;
        case 16: if constexpr (16 * sz <= 256) return ddc_poly_by_k<C, T, 16>(d, s, err); break;
        case 32: if constexpr (32 * sz <= 256) return ddc_poly_by_k<C, T, 32>(d, s, err); break;
    }
    return false;
}

template <typename C, typename T>
hipError_t launch_ddc_t(const DdcArgs& d, hipStream_t s) {
    using I = cpx<T>;
    const FirArgs& a = d.fir;
    hipError_t err;
    if (!a.exact && a.M >= 8 && a.L % a.M == 0 && ddc_poly_by_m<C, T>(d, s, &err)) return err;
    const C scale = *reinterpret_cast<const C*>(a.scale);
    size_t lds = 0;
    // the sine table's static LDS comes on top of the tile
    const size_t cap = 64 * 1024 - 1024 * sizeof(T);
    const int Tl = decim_direct_tile(a.L, a.M, sizeof(I), cap, &lds);
#define SDSP_DDC_ARGS (const I*)a.x, (const I*)a.hist, (const C*)a.taps_rev, scale, (I*)a.y, (long long)a.n, \
                      (long long)a.nout, a.L, a.M, (long long)a.j0
    if (lds <= cap) {
        dim3 grid((unsigned)((a.nout + Tl - 1) / Tl), (unsigned)a.channels);
        if (a.exact)
            hipLaunchKernelGGL((ddc_direct_kernel<C, T, true>), grid, dim3(Tl), lds, s, SDSP_DDC_ARGS, Tl, d.table,
                               d.theta0, d.dtheta, d.down);
        else
            hipLaunchKernelGGL((ddc_direct_kernel<C, T, false>), grid, dim3(Tl), lds, s, SDSP_DDC_ARGS, Tl, d.table,
                               d.theta0, d.dtheta, d.down);
    } else {
        dim3 grid((unsigned)((a.nout + kDirectThreads - 1) / kDirectThreads), (unsigned)a.channels);
        if (a.exact)
            hipLaunchKernelGGL((ddc_global_kernel<C, T, true>), grid, dim3(kDirectThreads), 0, s, SDSP_DDC_ARGS,
                               d.table, d.theta0, d.dtheta, d.down);
        else
            hipLaunchKernelGGL((ddc_global_kernel<C, T, false>), grid, dim3(kDirectThreads), 0, s, SDSP_DDC_ARGS,
                               d.table, d.theta0, d.dtheta, d.down);
    }
#undef SDSP_DDC_ARGS
    return hipGetLastError();
}

template <typename T>
hipError_t launch_ddc_hist_t(const DdcArgs& d, const void* new_hist, hipStream_t s) {
    const FirArgs& a = d.fir;
    const int Lm1 = a.L - 1;
    if (Lm1 <= 0) return hipSuccess;
    dim3 grid((unsigned)((Lm1 + 255) / 256), (unsigned)a.channels);
    hipLaunchKernelGGL((ddc_hist_kernel<T>), grid, dim3(256), 0, s, (const cpx<T>*)a.x, (const cpx<T>*)a.hist,
                       (cpx<T>*)new_hist, (long long)a.n, Lm1, d.table, d.theta0, d.dtheta, d.down);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ddc(int dtype, const DdcArgs& d, hipStream_t s) {
    if (d.fir.nout == 0) return hipSuccess;
    switch (dtype) {
        case 1: return launch_ddc_t<float, float>(d, s);
        case 2: return launch_ddc_t<c32, float>(d, s);
        case 4: return launch_ddc_t<double, double>(d, s);
        case 5: return launch_ddc_t<c64, double>(d, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_ddc_hist(int dtype, const DdcArgs& d, void* new_hist, hipStream_t s) {
    if (d.fir.n == 0) return hipSuccess;
    switch (dtype) {
        case 1: case 2: return launch_ddc_hist_t<float>(d, new_hist, s);
        case 4: case 5: return launch_ddc_hist_t<double>(d, new_hist, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace sdsp

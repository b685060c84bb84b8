// Arbitrary-rate resampler (gfx950): a linear interpolation between two neighbouring samples of the
// interpolating FIR's stream, chosen per output by a Q32.32 time accumulator; the interpolated
// stream is never written.
//
// With z the EXACT interpolator's stream over the handle's whole history (kern_pfb.hip, M = P),
//     z[j P + p] = sum_{i<K} cb[p][i] x[j - i],
// output k of a call with time register t and step `step` (both Q32.32 input samples) is
//     T = t + k step;   j = T >> 32;   f = T & (2^32 - 1)
//     v = f P;          b = v >> 32;   mu = (R)(v & (2^32 - 1)) 2^-32
//     out[k] = a + mu (c - a),   c = z[j P + b],   a = z[j P + b - 1]
// so c is branch b on the window ending at x[j]; a is branch b - 1 on the same window for b >= 1 and
// branch P - 1 on the window ending at x[j - 1] for b = 0 (it reaches x[j - K]: the oldest sample of
// the handle's window when j = 0).  Every output follows from k alone: no lane walks the accumulator.
// Both sums run in the interpolator's order from a zero accumulator, mac<true> for EXACT and
// mac<false> for FMA; the last line is three rounded operations for EXACT (this file is built
// with -ffp-contract=off) and one fma(mu, c - a, a) for FMA.
//
//   arb_stage_kernel  a workgroup owns `tile` consecutive outputs; their input span (K + 1 samples
//                     more than the inputs they sit on) and, when both fit, the branch table sit in
//                     LDS; a lane reads its K + 1 window samples once and feeds both sums from them
//   arb_kernel        one lane per output from global memory, 64-bit indices: steps of K inputs or
//                     more, where a span would mostly be samples no output reads, and spans too wide
//
// Branch rows in LDS have an odd stride of K | 1 elements, as the rational resampler's: the branch
// walk b_k = floor(frac(T_k) P) visits rows at an irregular stride, and an odd row stride puts two
// lanes on one bank only when their rows are congruent mod 64 (32 for 4-byte reads), where a stride
// of K = 2^m elements would fold all P rows onto 64 / K bank groups.
#include "sdsp_device.hpp"
#include "sdsp_kernels.hpp"
#include "sdsp_pfb_walk.hpp"

namespace sdsp {

namespace {

// a + mu (c - a) on re and im separately; mu is real
template <bool EXACT> __device__ inline float arb_lerp(float a, float c, float mu) {
    if constexpr (EXACT) return a + mu * (c - a);
    else return __builtin_fmaf(mu, c - a, a);
}
template <bool EXACT> __device__ inline double arb_lerp(double a, double c, double mu) {
    if constexpr (EXACT) return a + mu * (c - a);
    else return __builtin_fma(mu, c - a, a);
}
template <bool EXACT, typename T> __device__ inline cpx<T> arb_lerp(cpx<T> a, cpx<T> c, T mu) {
    return {arb_lerp<EXACT>(a.re, c.re, mu), arb_lerp<EXACT>(a.im, c.im, mu)};
}

// f P -> branch b and mu: (R)m is the round-to-nearest conversion (m >= 2^32 - 128 gives 1.0f in f32)
template <typename R> __device__ inline R arb_branch(uint32_t f, uint32_t P, uint32_t* b) {
    const uint64_t v = (uint64_t)f * P;  // P < 2^31
    *b = (uint32_t)(v >> 32);
    return (R)(uint32_t)v * (R)2.3283064365386962890625e-10;  // 2^-32, exact
}

template <typename C, typename I, bool EXACT>
__global__ void __launch_bounds__(256)
arb_kernel(const I* __restrict__ x, const I* __restrict__ hist, const C* __restrict__ cb, I* __restrict__ y,
           long long n, long long n_out, int K, int P, int H, uint64_t step, uint64_t t) {
    using R = typename real_of<I>::type;
    const int ch = blockIdx.y;
    x += (long long)ch * n;
    hist += (long long)ch * H;
    y += (long long)ch * n_out;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n_out; k += stride) {
        const uint64_t T = t + (uint64_t)k * step;  // < n 2^32 <= 2^63 (sdsp_arb_count)
        const long long j = (long long)(T >> 32);
        uint32_t b;
        const R mu = arb_branch<R>((uint32_t)T, (uint32_t)P, &b);
        const bool early = b == 0;  // a's window ends at x[j - 1]
        const C* cc = cb + (long long)b * K;
        const C* ca = cb + (long long)(early ? P - 1 : (int)b - 1) * K;
        I accc = zero_v<I>(), acca = zero_v<I>();
        I sp = pfb_ext(x, hist, j, H);
        for (int i = 0; i < K; ++i) {
            const I sn = pfb_ext(x, hist, j - i - 1, H);  // down to x[j - K] >= x[-K] = hist[0]
            accc = mac<EXACT>(accc, cc[i], sp);
            acca = mac<EXACT>(acca, ca[i], early ? sn : sp);
            sp = sn;
        }
        y[k] = arb_lerp<EXACT>(acca, accc, mu);
    }
}

// xs[s] = x[j0 - K + s] for the tile's first input j0 = T0 >> 32; output o of the tile sits on input
// j0 + jr, jr = (f0 + o step) >> 32, and reads xs[jr .. jr + K].  The last one reads up to
// s = ((f0 + (nt - 1) step) >> 32) + K < S (arb_plan sizes S for f0 = 2^32 - 1), and j0 + jr < n
// because every T < n 2^32.
template <typename C, typename I, bool EXACT, bool CB_LDS>
__global__ void __launch_bounds__(256)
arb_stage_kernel(const I* __restrict__ x, const I* __restrict__ hist, const C* __restrict__ cb, I* __restrict__ y,
                 long long n, long long n_out, int K, int P, int H, uint64_t step, uint64_t t, int tile, int S) {
    using R = typename real_of<I>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char arb_lds[];
    I* xs = reinterpret_cast<I*>(arb_lds);
    const int ch = blockIdx.y;
    x += (long long)ch * n;
    hist += (long long)ch * H;
    y += (long long)ch * n_out;
    const long long k0 = (long long)blockIdx.x * tile;
    const int nt = n_out - k0 < tile ? (int)(n_out - k0) : tile;
    const uint64_t T0 = t + (uint64_t)k0 * step;  // the one 64-bit multiply
    const long long j0 = (long long)(T0 >> 32);
    const uint64_t f0 = T0 & 0xffffffffULL;
    const int ns = (int)((f0 + (uint64_t)(nt - 1) * step) >> 32) + K + 1;  // tile step < 2^60; ns <= S
    const C* cbs = cb;
    int cs = K;
    if constexpr (CB_LDS) {
        C* cl = reinterpret_cast<C*>(arb_lds + ((size_t)S * sizeof(I) + 15) / 16 * 16);
        cs = K | 1;
        for (int i = threadIdx.x; i < P * K; i += 256) {
            const int row = i / K;
            cl[row * cs + (i - row * K)] = cb[i];
        }
        cbs = cl;
    }
    const long long base = j0 - K;
    if (base >= 0) {
        for (int i = threadIdx.x; i < ns; i += 256) xs[i] = x[base + i];
    } else {
        for (int i = threadIdx.x; i < ns; i += 256) xs[i] = pfb_ext(x, hist, base + i, H);
    }
    __syncthreads();
    I* yt = y + k0;
    for (unsigned o = threadIdx.x; o < (unsigned)nt; o += 256) {
        const uint64_t To = f0 + (uint64_t)o * step;
        uint32_t b;
        const R mu = arb_branch<R>((uint32_t)To, (uint32_t)P, &b);
        const bool early = b == 0;
        const C* cc = cbs + (size_t)b * cs;
        const C* ca = cbs + (size_t)(early ? P - 1 : (int)b - 1) * cs;
        const I* w = xs + (To >> 32) + K;  // w[-i] = x[j - i], i <= K
        I accc = zero_v<I>(), acca = zero_v<I>();
        I sp = w[0];
        for (int i = 0; i < K; ++i) {
            const I sn = w[-i - 1];
            accc = mac<EXACT>(accc, cc[i], sp);
            acca = mac<EXACT>(acca, ca[i], early ? sn : sp);
            sp = sn;
        }
        yt[o] = arb_lerp<EXACT>(acca, accc, mu);
    }
}

template <typename C, typename I>
hipError_t launch_arb_t(const ArbArgs& a, const ArbPlan& p, hipStream_t s) {
    const long long n = (long long)a.n, n_out = (long long)a.n_out;
    const long long tiles = (n_out + (long long)p.tile - 1) / (long long)p.tile;
    if (tiles > 0x7fffffffLL || a.channels > 65535) return hipErrorInvalidValue;
    const I* x = (const I*)a.x;
    const I* hist = (const I*)a.hist;
    const C* cb = (const C*)a.cb;
    I* y = (I*)a.y;
    if (p.kernel == kArbStaged) {
        const dim3 g((unsigned)tiles, (unsigned)a.channels);
#define SDSP_ARB_STAGE(EX, CBL)                                                                                    \
    hipLaunchKernelGGL((arb_stage_kernel<C, I, EX, CBL>), g, dim3(256), p.lds, s, x, hist, cb, y, n, n_out, a.K, a.P, \
                       a.H, a.step, a.t, (int)p.tile, p.S)
        if (a.exact) {
            if (p.cb_lds) SDSP_ARB_STAGE(true, true); else SDSP_ARB_STAGE(true, false);
        } else {
            if (p.cb_lds) SDSP_ARB_STAGE(false, true); else SDSP_ARB_STAGE(false, false);
        }
#undef SDSP_ARB_STAGE
        return hipGetLastError();
    }
    const dim3 g((unsigned)(tiles > 65536 ? 65536 : tiles), (unsigned)a.channels);
    if (a.exact)
        hipLaunchKernelGGL((arb_kernel<C, I, true>), g, dim3(256), 0, s, x, hist, cb, y, n, n_out, a.K, a.P, a.H,
                           a.step, a.t);
    else
        hipLaunchKernelGGL((arb_kernel<C, I, false>), g, dim3(256), 0, s, x, hist, cb, y, n, n_out, a.K, a.P, a.H,
                           a.step, a.t);
    return hipGetLastError();
}

}  // namespace

// The selection rule.  The staged kernel serves every shape that advances by fewer than K inputs per
// output and whose span fits with a tile of 256 outputs or more; everything else runs one lane per
// output.
ArbPlan arb_plan(int dtype, int P, uint64_t step, int K, int forced) {
    static const size_t sbytes[6] = {4, 8, 8, 8, 16, 16}, cbytes[6] = {4, 4, 8, 8, 8, 16};
    const size_t sb = sbytes[dtype], cbz = cbytes[dtype];
    const bool dense = (step >> 32) < (uint64_t)K;  // else most of a span is samples no output reads

    ArbPlan st{};
    bool stage_ok = false;
    if (dense) {
        int tile = 4096;
        size_t xb = 0;
        uint64_t S = 0;
        for (; tile >= 256; tile >>= 1) {
            S = ((0xffffffffULL + (uint64_t)(tile - 1) * step) >> 32) + (uint64_t)K + 1;  // step < K 2^32
            xb = ((size_t)S * sb + 15) / 16 * 16;
            if (xb <= (size_t)kPfbStageBytes) break;
        }
        if (tile >= 256) {
            stage_ok = true;
            const size_t cbb = (size_t)P * (size_t)(K | 1) * cbz;
            st.kernel = kArbStaged;
            st.tile = (size_t)tile;
            st.S = (int)S;
            st.cb_lds = xb + cbb <= (size_t)kPfbStageBytes;
            st.lds = xb + (st.cb_lds ? cbb : 0);
        }
    }

    ArbPlan po{};
    po.kernel = kArbPerOutput;
    po.tile = 256;

    if (forced == kArbStaged && stage_ok) return st;
    if (forced == kArbPerOutput) return po;
    return stage_ok ? st : po;
}

hipError_t launch_arb(int dtype, const ArbArgs& a, hipStream_t s) {
    if (a.n_out == 0) return hipSuccess;
    if (dtype < 0 || dtype > 5) return hipErrorInvalidValue;
    const ArbPlan p = arb_plan(dtype, a.P, a.step, a.K, a.kernel);
    switch (dtype) {
        case 0: return launch_arb_t<float, float>(a, p, s);
        case 1: return launch_arb_t<float, c32>(a, p, s);
        case 2: return launch_arb_t<c32, c32>(a, p, s);
        case 3: return launch_arb_t<double, double>(a, p, s);
        case 4: return launch_arb_t<double, c64>(a, p, s);
        case 5: return launch_arb_t<c64, c64>(a, p, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace sdsp

// Rational resampler (gfx950): the interpolating FIR's stream taken every D-th sample, with only the
// kept dot products computed.
//
// With z the EXACT interpolator's output for a call of n inputs (kern_pfb.hip),
//     z[u] = sum_{i<K} cb[p][i] x[j - i],   j = u / M,  p = u mod M,
// a call with phase counter c writes out[k] = z[u_k], u_k = (k + 1) D - 1 - c, k < n_out =
// floor((c + n M) / D): the reference decimator's convention (it emits on counts D - 1, 2D - 1, ...)
// applied to the interpolated stream.  The sum runs in that order from a zero accumulator in all
// three kernels, mac<true> for EXACT (bit-identical to the interpolator), mac<false> for FMA.
//
//   resamp_stage_kernel   a workgroup owns T consecutive outputs; their input span and (when both
//                         fit) the branch table sit in LDS; lanes walk the outputs in order
//   resamp_kernel         one lane per output from global memory, 64-bit indices: shapes whose
//                         span would mostly be samples no output reads (D > M K), or too wide
//   resamp_branch_kernel  K in {4, 8, 16}: a lane keeps one branch's coefficients in registers for
//                         the whole tile and advances by a whole number of inputs per output
//
// Branch rows in LDS have an odd stride of K | 1 elements: the stride-D walk over p then puts two
// lanes on one bank only when their branches are congruent mod 64 (32 for 4-byte reads), where a
// stride of K = 2^m elements would fold all M rows onto 64 / K bank groups.
#include "sdsp_device.hpp"
#include "sdsp_kernels.hpp"
#include "sdsp_pfb_walk.hpp"

namespace sdsp {

namespace {

template <typename C, typename I, bool EXACT>
__global__ void __launch_bounds__(256)
resamp_kernel(const I* __restrict__ x, const I* __restrict__ hist, const C* __restrict__ cb, I* __restrict__ y,
              long long n, long long n_out, int K, int M, int H, long long D, long long c) {
    const int ch = blockIdx.y;
    x += (long long)ch * n;
    hist += (long long)ch * H;
    y += (long long)ch * n_out;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n_out; k += stride) {
        const long long u = (k + 1) * D - 1 - c;  // < n M < 2^63 (sdsp_resamp_count)
        const long long j = u / M;
        const int p = (int)(u - j * M);
        const C* cp = cb + (long long)p * K;
        I acc = zero_v<I>();
        for (int i = 0; i < K; ++i) acc = mac<EXACT>(acc, cp[i], pfb_ext(x, hist, j - i, H));
        y[k] = acc;
    }
}

// xs[s] = x[j0 - K + 1 + s] for the tile's first input j0; the last output of the tile reads up to
// s = (r0 + (nt - 1) D) / M + K - 1 < S = ceil(T D / M) + K (resamp_plan), and j0 + that < n because
// every u_k < n M.
template <typename C, typename I, bool EXACT, bool CB_LDS>
__global__ void __launch_bounds__(256)
resamp_stage_kernel(const I* __restrict__ x, const I* __restrict__ hist, const C* __restrict__ cb,
                    I* __restrict__ y, long long n, long long n_out, int K, int M, int H, int D, long long c, int T,
                    int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char resamp_lds[];
    I* xs = reinterpret_cast<I*>(resamp_lds);
    const int ch = blockIdx.y;
    x += (long long)ch * n;
    hist += (long long)ch * H;
    y += (long long)ch * n_out;
    const long long k0 = (long long)blockIdx.x * T;
    const int nt = n_out - k0 < T ? (int)(n_out - k0) : T;
    const long long u0 = (k0 + 1) * (long long)D - 1 - c;
    const long long j0 = u0 / M;
    const unsigned um = (unsigned)M, ud = (unsigned)D, r0 = (unsigned)(u0 - j0 * M);
    const int ns = (int)((r0 + (unsigned)(nt - 1) * ud) / um) + K;  // M + T D < 2^31 (resamp_plan)
    const C* cbs = cb;
    int cs = K;
    if constexpr (CB_LDS) {
        C* cl = reinterpret_cast<C*>(resamp_lds + ((size_t)S * sizeof(I) + 15) / 16 * 16);
        cs = K | 1;
        for (int i = threadIdx.x; i < M * K; i += 256) {
            const int row = i / K;
            cl[row * cs + (i - row * K)] = cb[i];
        }
        cbs = cl;
    }
    const long long base = j0 - K + 1;
    if (base >= 0) {
        for (int i = threadIdx.x; i < ns; i += 256) xs[i] = x[base + i];
    } else {
        for (int i = threadIdx.x; i < ns; i += 256) xs[i] = pfb_ext(x, hist, base + i, H);
    }
    __syncthreads();
    I* yt = y + k0;
    for (unsigned o = threadIdx.x; o < (unsigned)nt; o += 256) {
        const unsigned v = r0 + o * ud;
        const unsigned j = v / um, p = v - j * um;
        const C* cp = cbs + (size_t)p * cs;
        const I* w = xs + j + K - 1;  // w[-i] = x[j0 + j - i]
        I acc = zero_v<I>();
        for (int i = 0; i < K; ++i) acc = mac<EXACT>(acc, cp[i], w[-i]);
        yt[o] = acc;
    }
}

// A = Pd floor(256 / Pd) lanes, Pd = M / gcd(M, D): lane l takes outputs k0 + l + r A, r < R.  Since
// A D = step M with step = (A / Pd)(D / g), its branch p = (r0 + l D) mod M never changes and its
// input index advances by `step` per output.  xs[s] = x[j0 - K + 1 + s], s < S =
// (M - 1 + (A - 1) D) / M + (R - 1) step + K, zero past the call's last input.
template <typename C, typename I, bool EXACT, int K>
__global__ void __launch_bounds__(256)
resamp_branch_kernel(const I* __restrict__ x, const I* __restrict__ hist, const C* __restrict__ cb,
                     I* __restrict__ y, long long n, long long n_out, int M, int H, int D, long long c, int A, int R,
                     int step, int S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char resamp_lds[];
    I* xs = reinterpret_cast<I*>(resamp_lds);
    const int ch = blockIdx.y;
    x += (long long)ch * n;
    hist += (long long)ch * H;
    y += (long long)ch * n_out;
    const int t = threadIdx.x;
    const long long k0 = (long long)blockIdx.x * (A * R);
    const long long u0 = (k0 + 1) * (long long)D - 1 - c;
    const long long j0 = u0 / M;
    const unsigned r0 = (unsigned)(u0 - j0 * M);
    for (int i = t; i < S; i += A) {
        const long long j = j0 - (K - 1) + i;
        xs[i] = j < n ? pfb_ext(x, hist, j, H) : zero_v<I>();
    }
    const unsigned v = r0 + (unsigned)t * (unsigned)D;  // M + 256 D < 2^31 (resamp_plan)
    const unsigned jl = v / (unsigned)M, p = v - jl * (unsigned)M;
    C cr[K];
#pragma unroll
    for (int i = 0; i < K; ++i) cr[i] = cb[(long long)p * K + i];
    __syncthreads();
    const I* w = xs + jl + K - 1;  // w[-i] = x[j0 + jl - i]
    for (int r = 0; r < R; ++r) {
        const long long k = k0 + t + (long long)r * A;
        if (k >= n_out) break;
        I acc = zero_v<I>();
#pragma unroll
        for (int i = 0; i < K; ++i) acc = mac<EXACT>(acc, cr[i], w[-i]);
        y[k] = acc;
        w += step;
    }
}

size_t gcd_sz(size_t a, size_t b) {
    while (b) {
        const size_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

template <typename C, typename I>
hipError_t launch_resamp_t(const ResampArgs& a, const ResampPlan& p, hipStream_t s) {
    const long long n = (long long)a.n, n_out = (long long)a.n_out;
    const long long tiles = (n_out + (long long)p.tile - 1) / (long long)p.tile;
    if (tiles > 0x7fffffffLL || a.channels > 65535) return hipErrorInvalidValue;
    const I* x = (const I*)a.x;
    const I* hist = (const I*)a.hist;
    const C* cb = (const C*)a.cb;
    I* y = (I*)a.y;
    if (p.kernel == kResampStaged) {
        const dim3 g((unsigned)tiles, (unsigned)a.channels);
#define SDSP_RESAMP_STAGE(EX, CBL)                                                                               \
    hipLaunchKernelGGL((resamp_stage_kernel<C, I, EX, CBL>), g, dim3(256), p.lds, s, x, hist, cb, y, n, n_out, a.K, \
                       a.M, a.H, (int)a.D, (long long)a.c, p.T, p.S)
        if (a.exact) {
            if (p.cb_lds) SDSP_RESAMP_STAGE(true, true); else SDSP_RESAMP_STAGE(true, false);
        } else {
            if (p.cb_lds) SDSP_RESAMP_STAGE(false, true); else SDSP_RESAMP_STAGE(false, false);
        }
#undef SDSP_RESAMP_STAGE
        return hipGetLastError();
    }
    if (p.kernel == kResampBranch) {
        const dim3 g((unsigned)tiles, (unsigned)a.channels);
#define SDSP_RESAMP_BRANCH(EX, KK)                                                                                \
    hipLaunchKernelGGL((resamp_branch_kernel<C, I, EX, KK>), g, dim3((unsigned)p.A), p.lds, s, x, hist, cb, y, n, \
                       n_out, a.M, a.H, (int)a.D, (long long)a.c, p.A, p.R, p.step, p.S)
#define SDSP_RESAMP_BRANCH_K(KK)                                                                                  \
    if (a.K == KK) {                                                                                              \
        if (a.exact) SDSP_RESAMP_BRANCH(true, KK); else SDSP_RESAMP_BRANCH(false, KK);                            \
        return hipGetLastError();                                                                                 \
    }
        SDSP_RESAMP_BRANCH_K(4)
        SDSP_RESAMP_BRANCH_K(8)
        SDSP_RESAMP_BRANCH_K(16)
#undef SDSP_RESAMP_BRANCH_K
#undef SDSP_RESAMP_BRANCH
        return hipErrorInvalidValue;
    }
    const dim3 g((unsigned)(tiles > 65536 ? 65536 : tiles), (unsigned)a.channels);
    if (a.exact)
        hipLaunchKernelGGL((resamp_kernel<C, I, true>), g, dim3(256), 0, s, x, hist, cb, y, n, n_out, a.K, a.M, a.H,
                           (long long)a.D, (long long)a.c);
    else
        hipLaunchKernelGGL((resamp_kernel<C, I, false>), g, dim3(256), 0, s, x, hist, cb, y, n, n_out, a.K, a.M, a.H,
                           (long long)a.D, (long long)a.c);
    return hipGetLastError();
}

}  // namespace

// The selection rule.  The staged kernel serves every shape whose span fits with T >= 256 and
// D <= M K; everything else runs one lane per output.  The branch-stationary kernel is never the
// automatic choice (DESIGN section 4 has the measurement); `forced` selects it where it applies.
ResampPlan resamp_plan(int dtype, int M, size_t D, int K, int forced) {
    static const size_t sbytes[6] = {4, 8, 8, 8, 16, 16}, cbytes[6] = {4, 4, 8, 8, 8, 16};
    const size_t sb = sbytes[dtype], cbz = cbytes[dtype];
    const unsigned long long um = (unsigned long long)M, ud = (unsigned long long)D, lim = 1ULL << 31;
    const bool dense = ud <= um * (unsigned long long)K;  // else most of a span is samples no output reads

    ResampPlan st{};
    bool stage_ok = false;
    if (dense) {
        int T = 4096;
        size_t xb = 0;
        unsigned long long S = 0;
        for (; T >= 256; T >>= 1) {
            S = ((unsigned long long)T * ud + um - 1) / um + (unsigned long long)K;
            xb = ((size_t)S * sb + 15) / 16 * 16;
            if (xb <= (size_t)kPfbStageBytes) break;
        }
        if (T >= 256 && um + (unsigned long long)T * ud < lim) {
            stage_ok = true;
            const size_t cbb = (size_t)M * (size_t)(K | 1) * cbz;
            st.kernel = kResampStaged;
            st.tile = (size_t)T;
            st.T = T;
            st.S = (int)S;
            st.cb_lds = xb + cbb <= (size_t)kPfbStageBytes;
            st.lds = xb + (st.cb_lds ? cbb : 0);
        }
    }

    ResampPlan br{};
    bool branch_ok = false;
    const size_t g = gcd_sz((size_t)M, D), Pd = (size_t)M / g;
    if (dense && (K == 4 || K == 8 || K == 16) && Pd <= 256 && um + 256 * ud < lim) {
        const unsigned long long A = Pd * (256 / Pd), step1 = (A / Pd) * (ud / g);
        for (int R = 16; R >= 1; R >>= 1) {
            const unsigned long long S = (um - 1 + (A - 1) * ud) / um + (unsigned long long)(R - 1) * step1 +
                                         (unsigned long long)K;
            if (S * sb <= (unsigned long long)kPfbStageBytes) {
                branch_ok = true;
                br.kernel = kResampBranch;
                br.tile = (size_t)(A * R);
                br.A = (int)A;
                br.R = R;
                br.step = (int)step1;
                br.S = (int)S;
                br.lds = ((size_t)S * sb + 15) / 16 * 16;
                break;
            }
        }
    }

    ResampPlan po{};
    po.kernel = kResampPerOutput;
    po.tile = 256;

    if (forced == kResampStaged && stage_ok) return st;
    if (forced == kResampBranch && branch_ok) return br;
    if (forced == kResampPerOutput) return po;
    return stage_ok ? st : po;
}

hipError_t launch_resamp(int dtype, const ResampArgs& a, hipStream_t s) {
    if (a.n_out == 0) return hipSuccess;
    if (dtype < 0 || dtype > 5) return hipErrorInvalidValue;
    const ResampPlan p = resamp_plan(dtype, a.M, a.D, a.K, a.kernel);
    switch (dtype) {
        case 0: return launch_resamp_t<float, float>(a, p, s);
        case 1: return launch_resamp_t<float, c32>(a, p, s);
        case 2: return launch_resamp_t<c32, c32>(a, p, s);
        case 3: return launch_resamp_t<double, double>(a, p, s);
        case 4: return launch_resamp_t<double, c64>(a, p, s);
        case 5: return launch_resamp_t<c64, c64>(a, p, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace sdsp

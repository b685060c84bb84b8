// Spectrometer: the oversampled channeliser's frames squared and integrated in registers (gfx950).
//
// Per stream, Y[m] is frame m of kern_oschan.hip (the same branch sums, rotation and transform: the
// same bits), p[m][k] = Y.re Y.re + Y.im Y.im (two rounded products, one rounded sum), and spectrum j
// integrates frames jA .. jA + A - 1 in sub-blocks of 32 frames counted from frame jA, the last one
// shorter when 32 does not divide A:
//   s_b[k] = ((0 + p[jA + 32 b][k]) + p[jA + 32 b + 1][k]) + ..       sequential
//   P_j[k] = (((0 + s_0) + s_1) + ..) * scale                         sequential, one rounded multiply
// One definition of the arithmetic: both main kernels, every sub-blocks-per-workgroup value and every
// call split give the same bits.
//
// A call of `frames` frames starts `filled` frames into the open integration (0 <= filled < A).  Its
// sub-blocks are numbered sb = 0 .. nsb - 1 from the one frame 0 falls into (spec_cut): that one
// continues the carried sum `sub` when filled mod 32 > 0 and is shorter by as many frames; the last one
// is open when the call ends inside it and goes to the new `sub`.  Every closed sub-block goes to the
// partials scratch [streams][nsb][M].  The cut points come from filled, A and the frame index: they
// restart at every integration start.
//
//   spec_frame_kernel  grid (run of R sub-blocks, stream).  kern_oschan.hip's per-frame body looped
//                      over the run's frames: branch sums from global memory, 2 M samples of LDS.
//   spec_slide_kernel  the same grid.  kern_oschan.hip's ring of K M + D samples in LDS, advanced D
//                      per frame, the next frame's samples requested a frame ahead.
//   spec_fold_kernel   one lane per (stream, integration the call touches, bin): the carried `tot`
//                      or 0, plus the integration's closed sub-blocks in order; a finished integration
//                      is scaled and stored, the trailing open one becomes the new `tot`.
// The lane that stores r[q] in kern_oschan.hip, q = tid + j nthr, owns bin q here: acc[NPT] stays in
// registers across the frames of a sub-block.  sub and tot are ping-pong buffers (another workgroup
// may still read the old one).
#include "sdsp_chan_dev.hpp"
#include "sdsp_device.hpp"
#include "sdsp_fft_dev.hpp"
#include "sdsp_kernels.hpp"

namespace sdsp {

namespace {

constexpr size_t kSpecLdsAuto = 40 * 1024;  // automatic choice: the sliding kernel up to this footprint
#ifndef SDSP_SPEC_SUB  // (tools/lab/spec_cut31.hip sets 31: the numerically wrong library of profiles/r21/LAB.md)
#define SDSP_SPEC_SUB 32
#endif
constexpr int kSpecSub = SDSP_SPEC_SUB;     // frames of a whole sub-block

// frames [f0, f1) of the call that its sub-block sb holds, and whether the call closes it
struct SpecCut {
    long long f0, f1;
    bool closed;
};

__host__ __device__ inline SpecCut spec_cut(long long sb, int filled, int A, long long frames) {
    const int nsa = (A + kSpecSub - 1) / kSpecSub;  // sub-blocks of an integration
    const long long g = filled / kSpecSub + sb;     // counted from the open integration's first
    const long long j = g / nsa, b = g % nsa;
    const long long g0 = j * A + b * kSpecSub;      // in frames since the open integration's start
    const long long g1 = g0 + kSpecSub < (j + 1) * A ? g0 + kSpecSub : (j + 1) * A;
    SpecCut c;
    c.f0 = g0 > filled ? g0 - filled : 0;
    c.f1 = g1 - filled < frames ? g1 - filled : frames;
    c.closed = g1 - filled <= frames;
    return c;
}

// The epilogue both main kernels share: the lane's bins of frame f join acc; at the end of sub-block
// `sb` the sums go to the partials (closed) or to the new `sub` (open), and the next sub-block starts
// from zero.
template <typename T, int NPT>
struct SpecLane {
    T acc[NPT];
    long long sb;
    SpecCut cut;

    __device__ __forceinline__ void open(long long first_sb, const T* __restrict__ sub_in, int filled, int A,
                                         long long frames, int M, int tid, int nthr) {
        sb = first_sb;
        cut = spec_cut(sb, filled, A, frames);
        const bool carried = sb == 0 && filled % kSpecSub > 0;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int q = tid + j * nthr;
            acc[j] = carried && q < M ? sub_in[q] : T(0);
        }
    }
    __device__ __forceinline__ void add(const c2<T>* r, long long f, T* __restrict__ part, T* __restrict__ sub_out,
                                        int filled, int A, long long frames, int M, int tid, int nthr) {
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int q = tid + j * nthr;
            if (q < M) {
                const c2<T> v = r[q];
                const T p = v.re * v.re + v.im * v.im;
                acc[j] = acc[j] + p;
            }
        }
        if (f + 1 < cut.f1) return;
        T* dst = cut.closed ? part + sb * M : sub_out;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int q = tid + j * nthr;
            if (q < M) dst[q] = acc[j];
            acc[j] = T(0);
        }
        cut = spec_cut(++sb, filled, A, frames);
    }
};

}  // namespace

// R sub-blocks per workgroup; nsb sub-blocks in the call
template <typename T, int NPT>
__global__ void __launch_bounds__(256)
spec_frame_kernel(const c2<T>* __restrict__ x, const c2<T>* __restrict__ hist, const T* __restrict__ cbt,
                  const c2<T>* __restrict__ tw, const T* __restrict__ sub_in, T* __restrict__ sub_out,
                  T* __restrict__ part, int M, int logM, int K, int D, int c, long long n, long long frames, int A,
                  int filled, long long nsb, int R) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    c2<T>* a = reinterpret_cast<c2<T>*>(lds_raw);
    c2<T>* b = a + M;
    const int s = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
    const long long H = (long long)K * M - D;
    x += (long long)s * n;
    hist += (long long)s * H;
    part += (long long)s * nsb * M;
    sub_in += (long long)s * M;
    sub_out += (long long)s * M;
    const long long sb0 = (long long)blockIdx.x * R, sb1 = sb0 + R < nsb ? sb0 + R : nsb;
    const long long f1 = spec_cut(sb1 - 1, filled, A, frames).f1;
    SpecLane<T, NPT> lane;
    lane.open(sb0, sub_in, filled, A, frames, M, tid, nthr);
    for (long long f = lane.cut.f0; f < f1; ++f) {
        const int sh = oschan_shift(c, f, D, M);
        const long long e = (f + 1) * D - 1;  // the frame's newest sample
        for (int p = tid; p < M; p += nthr) {
            c2<T> acc = {T(0), T(0)};
            for (int i = 0; i < K; ++i)
                chan_mac(acc, cbt[(long long)i * M + p], oschan_sample(x, hist, e - p - (long long)i * M, H));
            a[(p - sh) & (M - 1)] = acc;
        }
        __syncthreads();
        const c2<T>* r = stockham<T, false>(a, b, M, logM, tw, tid, nthr);  // ends on a barrier
        lane.add(r, f, part, sub_out, filled, A, frames, M, tid, nthr);
        __syncthreads();  // r is read before the next frame's sums overwrite a
    }
}

// kern_oschan.hip's oschan_slide_kernel (its LDS layout, ring arithmetic, KC and TWL are described
// there) over the frames of a run of sub-blocks, with SpecLane in place of the store.
template <typename T, int NPT, int KC, bool TWL>
__global__ void __launch_bounds__(256)
spec_slide_kernel(const c2<T>* __restrict__ x, const c2<T>* __restrict__ hist, const T* __restrict__ cbt,
                  const c2<T>* __restrict__ tw, const T* __restrict__ sub_in, T* __restrict__ sub_out,
                  T* __restrict__ part, int M, int logM, int K, int D, int c, long long n, long long frames, int A,
                  int filled, long long nsb, int R) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    c2<T>* ring = reinterpret_cast<c2<T>*>(lds_raw);
    const int s = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
    if constexpr (KC > 0) K = KC;
    const int win = K * M, cap = win + D;
    const long long H = (long long)win - D;
    c2<T>* a = ring + cap;
    c2<T>* b = a + M;
    x += (long long)s * n;
    hist += (long long)s * H;
    part += (long long)s * nsb * M;
    sub_in += (long long)s * M;
    sub_out += (long long)s * M;
    const long long sb0 = (long long)blockIdx.x * R, sb1 = sb0 + R < nsb ? sb0 + R : nsb;
    const long long f1 = spec_cut(sb1 - 1, filled, A, frames).f1;  // the run emits frames [f0, f1)
    SpecLane<T, NPT> lane;
    lane.open(sb0, sub_in, filled, A, frames, M, tid, nthr);
    const long long f0 = lane.cut.f0;
    const c2<T>* twp = tw;
    if constexpr (TWL) {  // (visible to every lane after the first frame's barrier below)
        c2<T>* t = b + M;
        for (int q = tid; q < M; q += nthr) t[q] = tw[q];
        twp = t;
    }
    T cf[KC > 0 ? KC : 1][NPT];
    if constexpr (KC > 0) {
#pragma unroll
        for (int i = 0; i < KC; ++i)
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const int p = tid + j * nthr;
                cf[i][j] = p < M ? cbt[(long long)i * M + p] : T(0);
            }
    }
    // the H samples before the run's first new one, ring[0 .. H)
    const long long j0 = f0 * D;
    for (int q = tid; q < (int)H; q += nthr) ring[q] = oschan_sample(x, hist, j0 - H + q, H);
    c2<T> nx[NPT];  // the frame's D new samples, requested one frame ahead
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int r = tid + j * nthr;
        nx[j] = r < D ? x[j0 + r] : c2<T>{T(0), T(0)};
    }
    int wpos = (int)H;  // where the frame's new samples go; < cap
    for (long long f = f0; f < f1; ++f) {
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int r = tid + j * nthr;
            if (r < D) {
                int q = wpos + r;
                if (q >= cap) q -= cap;
                ring[q] = nx[j];
            }
        }
        int e = wpos + D - 1;  // the newest sample
        if (e >= cap) e -= cap;
        wpos = e + 1 == cap ? 0 : e + 1;
        __syncthreads();  // (and every lane has read the frame before's r)
        if (f + 1 < f1) {
            const c2<T>* src = x + (f + 1) * D;
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const int r = tid + j * nthr;
                if (r < D) nx[j] = src[r];
            }
        }
        const int sh = oschan_shift(c, f, D, M);
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int p = tid + j * nthr;
            if (p < M) {
                int q = e - p;
                if (q < 0) q += cap;
                c2<T> acc = {T(0), T(0)};
                if constexpr (KC > 0) {
#pragma unroll
                    for (int i = 0; i < KC; ++i) {
                        chan_mac(acc, cf[i][j], ring[q]);
                        q -= M;
                        if (q < 0) q += cap;
                    }
                } else {
                    for (int i = 0; i < K; ++i) {
                        chan_mac(acc, cbt[(long long)i * M + p], ring[q]);
                        q -= M;
                        if (q < 0) q += cap;
                    }
                }
                a[(p - sh) & (M - 1)] = acc;
            }
        }
        __syncthreads();
        const c2<T>* r = stockham<T, false>(a, b, M, logM, twp, tid, nthr);  // ends on a barrier
        lane.add(r, f, part, sub_out, filled, A, frames, M, tid, nthr);
    }
}

// nint integrations touched by the call, the first `spectra` of them finished by it.  Integration 0 is
// the one open at the call's start: its sub-blocks before filled / 32 are in tot_in.  The call's
// sub-block numbering (spec_cut) puts sub-block b of integration ji at ji nsa + b - filled / 32.
template <typename T>
__global__ void __launch_bounds__(256)
spec_fold_kernel(const T* __restrict__ part, const T* __restrict__ tot_in, T* __restrict__ tot_out,
                 T* __restrict__ out, int M, int logM, int A, int filled, long long frames, long long nsb,
                 long long nint, long long spectra, T scale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nint * M) return;
    const int s = blockIdx.y, k = (int)(i & (M - 1));
    const long long ji = i >> logM;
    const int nsa = (A + kSpecSub - 1) / kSpecSub, first = filled / kSpecSub;
    const bool done = ji < spectra;
    const int lo = ji == 0 ? first : 0;
    const int hi = done ? nsa : (int)((filled + frames - ji * A) / kSpecSub);
    T t = ji == 0 && first > 0 ? tot_in[(long long)s * M + k] : T(0);
    const T* p = part + ((long long)s * nsb + ji * nsa - first) * M + k;
    int b = lo;
    for (; b + 8 <= hi; b += 8) {  // eight loads in flight ahead of the dependent adds
        T v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(long long)(b + u) * M];
#pragma unroll
        for (int u = 0; u < 8; ++u) t = t + v[u];
    }
    for (; b < hi; ++b) t = t + p[(long long)b * M];
    if (done) out[((long long)s * spectra + ji) * M + k] = t * scale;
    else tot_out[(long long)s * M + k] = t;
}

size_t spec_subblocks(size_t filled, size_t A, size_t frames) {
    if (frames == 0) return 0;
    const size_t nsa = (A + kSpecSub - 1) / kSpecSub, g = filled + frames - 1;
    return (g / A) * nsa + (g % A) / kSpecSub - filled / kSpecSub + 1;
}

// Which kernel a handle runs and its sub-blocks per workgroup on a long block: a function of the
// shape and the two knobs alone (sdsp_spec_info).
//   kernel: a sliding request runs the sliding kernel where its ring (K M + D samples) and the
//           Stockham pair (2 M) fit kChanLdsCap, else the per-frame kernel.  Automatic is the sliding
//           kernel where ring, pair and table take at most kSpecLdsAuto, but for K = 1 at M = 256.
//           oschan_plan's bound is 16 KiB; measured here at complex f32, 2^27 samples, K = 1 and 8
//           (profiles/r21/LAB.md), at one sub-block per workgroup: the sliding
//           kernel takes 0.70 to 0.90 of the per-frame kernel's time up to 12 KiB, 0.94 at 23 KiB
//           (M = 256, K = 8; 0.91 at two sub-blocks), 0.96 to 0.98 at 40 KiB (M = 1024, K = 1, D = M),
//           1.01 to 1.03 at 36 KiB (M = 1024, K = 1, D = M/2, ranges overlapping) and 1.27 to 1.47 at
//           92 and 96 KiB (1.16 to 1.34 at its best count); at M = 256, K = 1, D = M/2 (9 KiB) it takes
//           1.02 to 1.03, ranges apart, hence the exception.  Other K, complex f64: the same bound,
//           reasoned, not measured.
//   sub-blocks: the knob when set.  Automatic on the sliding kernel: the smallest count whose frames
//           (min(A, 32) each) reach 4 ceil((K M - D) / D), four times the run's fill, at least 1;
//           1 on the per-frame kernel, which has no fill.  Measured on the same shapes: 2, 4 and 8
//           sub-blocks of 32 frames cost the per-frame kernel 0 to 17, 3 to 30 and 9 to 98 % over one;
//           on the sliding kernel up to 40 KiB two cost -1 to 6 % and eight 6 to 38 %, except at
//           M = 256, K = 8 (fill 15 frames), where two take 0.96 to 0.97 of one, ranges apart: the
//           starting rule (twice the fill) chose one there.
SpecPlan spec_plan(bool f64, int M, int K, int D, int A, int kernel, int subblocks) {
    const size_t sample = f64 ? 16 : 8;
    const size_t base = ((size_t)K * M + (size_t)D + 2 * (size_t)M) * sample;
    const bool fits = base <= kChanLdsCap;
    const bool pays = base + (size_t)M * sample <= kSpecLdsAuto && !(K == 1 && M == 256);
    SpecPlan p;
    p.kernel = (kernel == kSpecSlide && fits) || (kernel == 0 && pays) ? kSpecSlide : kSpecPerFrame;
    if (subblocks > 0) p.subblocks = (size_t)subblocks;
    else if (p.kernel == kSpecPerFrame) p.subblocks = 1;
    else {
        const size_t fill = ((size_t)K * M - 1) / D;  // ceil((K M - D) / D): the fill, in frames
        const size_t per = A < kSpecSub ? A : kSpecSub;
        p.subblocks = 4 * fill > per ? (4 * fill + per - 1) / per : 1;
    }
    return p;
}

template <typename T, int NPT>
hipError_t launch_spec_n(const SpecArgs& a, const SpecPlan& p, size_t nsb, int thr, hipStream_t s) {
    const c2<T>* x = (const c2<T>*)a.x;
    const c2<T>* hist = (const c2<T>*)a.hist;
    const bool slide = p.kernel == kSpecSlide;
    // an automatic run never drops below the fill's own length: the fill then doubles the reads at most
    const size_t per = (size_t)(a.A < kSpecSub ? a.A : kSpecSub), fill = ((size_t)a.K * a.M - 1) / a.D;
    const size_t least = slide && fill > per ? (fill + per - 1) / per : 1;
    const size_t R = chunk_frames(p.subblocks, a.subblocks > 0, nsb, a.streams, least);
    dim3 grid((unsigned)((nsb + R - 1) / R), (unsigned)a.streams);
    if (!slide) {
        hipLaunchKernelGGL((spec_frame_kernel<T, NPT>), grid, dim3(thr), 2 * (size_t)a.M * sizeof(c2<T>), s, x, hist,
                           (const T*)a.cbt, (const c2<T>*)a.tw, (const T*)a.sub_in, (T*)a.sub_out, (T*)a.part, a.M,
                           a.logM, a.K, a.D, a.phase, (long long)a.n, (long long)a.frames, a.A, a.filled,
                           (long long)nsb, (int)R);
        return hipGetLastError();
    }
    const size_t base = ((size_t)a.K * a.M + a.D + 2 * (size_t)a.M) * sizeof(c2<T>);
    const size_t table = (size_t)a.M * sizeof(c2<T>);
    const bool twl = base + table <= kChanLdsAll;
    chan_dispatch_k(a.K, [&](auto k) {
        // (K NPT > 40 fits no precision's 128 KiB: those depths get no register instance of their own)
        constexpr int KC = decltype(k)::value * NPT <= 40 ? decltype(k)::value : 0;
        const auto kernel = twl ? spec_slide_kernel<T, NPT, KC, true> : spec_slide_kernel<T, NPT, KC, false>;
        hipLaunchKernelGGL(kernel, grid, dim3(thr), twl ? base + table : base, s, x, hist, (const T*)a.cbt,
                           (const c2<T>*)a.tw, (const T*)a.sub_in, (T*)a.sub_out, (T*)a.part, a.M, a.logM, a.K, a.D,
                           a.phase, (long long)a.n, (long long)a.frames, a.A, a.filled, (long long)nsb, (int)R);
    });
    return hipGetLastError();
}

template <typename T>
hipError_t launch_spec_t(const SpecArgs& a, const SpecPlan& p, hipStream_t s) {
    const size_t nsb = spec_subblocks(a.filled, a.A, a.frames);
    const int thr = chan_threads(a.M);  // NPT bins per lane cover the frame
    hipError_t e = chan_dispatch_npt(a.M, thr, [&](auto npt) {
        return launch_spec_n<T, decltype(npt)::value>(a, p, nsb, thr, s);
    });
    if (e != hipSuccess) return e;
    const size_t total = (size_t)a.filled + a.frames;
    const size_t spectra = total / a.A, nint = (total + a.A - 1) / a.A;
    dim3 grid((unsigned)((nint * a.M + 255) / 256), (unsigned)a.streams);
    hipLaunchKernelGGL((spec_fold_kernel<T>), grid, dim3(256), 0, s, (const T*)a.part, (const T*)a.tot_in,
                       (T*)a.tot_out, (T*)a.out, a.M, a.logM, a.A, a.filled, (long long)a.frames, (long long)nsb,
                       (long long)nint, (long long)spectra, (T)a.scale);
    return hipGetLastError();
}

hipError_t launch_spec(bool f64, const SpecArgs& a, hipStream_t s) {
    if (a.frames == 0) return hipSuccess;
    const SpecPlan p = spec_plan(f64, a.M, a.K, a.D, a.A, a.kernel, a.subblocks);
    return f64 ? launch_spec_t<double>(a, p, s) : launch_spec_t<float>(a, p, s);
}

}  // namespace sdsp

// Oversampled analysis channeliser: M channels, one frame every D <= M samples (gfx950).
//
// Per stream, with cbt[i][p] = h[p + (K-1-i) M] (the analysis channeliser's branch table, [K][M]),
// x[<0] = 0 and m the frame index since create / reset / set_streams,
//   v_p[m] = sum_{i<K} cbt[i][p] * x[(m+1) D - 1 - p - i M]      p = 0 .. M-1
//   w_q[m] = v_{(q + (m+1) D) mod M}[m]                           (an index rotation, no arithmetic)
//   Y[m]   = FORWARD_FFT_M(w[m])                                  (unnormalised)
// D = M is sdsp_chan (the rotation is 0).  For every D channel k is a plain down-converter,
//   Y[m][k] = (g * (x[n] e^{+j 2 pi k (n+1) / M}))[(m+1) D - 1],  g[p + i M] = h[p + (K-1-i) M]:
// a mix, a filter and a decimation by D with a phase-continuous oscillator.  The rotation buys that;
// without it the output is a sliding STFT whose channel k turns by e^{-j 2 pi k (m+1) D / M} from
// frame to frame.  It is an index rotation, not a twiddle multiply, which would cost a rounding.
//
// One definition of the arithmetic, no algorithm switch: the branch sum starts from a zero
// accumulator and runs i = 0, 1, .., K-1, each step acc + c * v with a rounded multiply and a
// rounded add (-ffp-contract=off, as chan_kernel); the transform is stockham<T, false> on the
// make_twiddles(M) table.  So both kernels below give the same bits at every frames-per-workgroup
// value and every call split, and at D = M the bits of chan_kernel.
//
// A call sees frames f = 0 .. frames-1 of its own block; c = (frames before the call * D) mod M
// carries the rotation across calls: sh = (c + (f+1) D) mod M, formed in 64 bits, and v_p lands at
// index (p - sh) mod M of the transform's input.  Sample j of the call is x[j], or hist[H + j] for
// j < 0, H = K M - D (the lowest index a frame reads is (f+1) D - K M >= -H).
//
//   oschan_frame_kernel  grid (frame, stream).  Branch sums from global memory, 2 M samples of LDS:
//                        fits every shape; the fallback and the cross-check.
//   oschan_slide_kernel  grid (chunk of F frames, stream).  A ring of K M + D samples of the stream
//                        stays in LDS and advances by D samples per frame: one HBM read per input
//                        sample, (K M - D) / (F D) extra for the chunk's fill.
#include "sdsp_chan_dev.hpp"
#include "sdsp_device.hpp"
#include "sdsp_fft_dev.hpp"
#include "sdsp_kernels.hpp"

namespace sdsp {

namespace {

constexpr size_t kOschanLdsAuto = 16 * 1024;  // automatic choice: the sliding kernel up to this footprint

}  // namespace

template <typename T>
__global__ void __launch_bounds__(256)
oschan_frame_kernel(const c2<T>* __restrict__ x, const c2<T>* __restrict__ hist, const T* __restrict__ cbt,
                    c2<T>* __restrict__ y, const c2<T>* __restrict__ tw, int M, int logM, int K, int D, int c,
                    long long n, long long frames) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    c2<T>* a = reinterpret_cast<c2<T>*>(lds_raw);
    c2<T>* b = a + M;
    const long long f = blockIdx.x;
    const int s = blockIdx.y;
    const long long H = (long long)K * M - D;
    x += (long long)s * n;
    hist += (long long)s * H;
    y += ((long long)s * frames + f) * M;
    const int sh = oschan_shift(c, f, D, M);
    const long long e = (f + 1) * D - 1;  // the frame's newest sample
    for (int p = threadIdx.x; p < M; p += blockDim.x) {
        c2<T> acc = {T(0), T(0)};
        for (int i = 0; i < K; ++i)
            chan_mac(acc, cbt[(long long)i * M + p], oschan_sample(x, hist, e - p - (long long)i * M, H));
        a[(p - sh) & (M - 1)] = acc;
    }
    __syncthreads();
    const c2<T>* r = stockham<T, false>(a, b, M, logM, tw, threadIdx.x, blockDim.x);
    for (int q = threadIdx.x; q < M; q += blockDim.x) y[q] = r[q];
}

// LDS: ring[cap = K M + D], then the Stockham pair a, b [M each], then (TWL) the twiddle table [M].
// Before frame f's sums the ring holds samples (f+1) D - K M .. (f+1) D - 1 of the call, the newest
// at index e; lane p reads ring[(e - p - i M) mod cap], consecutive lanes walking downwards, 8 bytes
// each for complex f32 (ds_read_b64, no bank conflict).  cap is no power of two: every index wraps by
// one conditional add or subtract (a step is at most M <= cap).  The D samples of frame f+1 are
// requested into registers before frame f's sums and transform and written behind the window after
// them; the D spare slots keep that write off the samples frame f reads.
//
// KC = K for K = 1 .. 8, 0 for any other K.  A lane's branches p never change, so with KC > 0 its
// K NPT coefficients are read once per workgroup and stay in registers (at most 40 values: the ring
// and the pair fit 128 KiB); with KC = 0 every frame re-reads them through the cache.
//
// TWL: the twiddle table sits in LDS behind the pair.  A twiddle read from global memory inside a
// pass would queue behind the next frame's request, which is in flight across the transform (vmcnt
// counts loads in issue order).
template <typename T, int NPT, int KC, bool TWL>
__global__ void __launch_bounds__(256)
oschan_slide_kernel(const c2<T>* __restrict__ x, const c2<T>* __restrict__ hist, const T* __restrict__ cbt,
                    c2<T>* __restrict__ y, const c2<T>* __restrict__ tw, int M, int logM, int K, int D, int c,
                    long long n, long long frames, int F) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    c2<T>* ring = reinterpret_cast<c2<T>*>(lds_raw);
    const int s = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
    const long long f0 = (long long)blockIdx.x * F;  // the chunk emits frames [f0, f1)
    const long long f1 = f0 + F < frames ? f0 + F : frames;
    if constexpr (KC > 0) K = KC;
    const int win = K * M, cap = win + D;
    const long long H = (long long)win - D;
    c2<T>* a = ring + cap;
    c2<T>* b = a + M;
    x += (long long)s * n;
    hist += (long long)s * H;
    y += (long long)s * frames * M;
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
    // the H samples before the chunk's first new one, ring[0 .. H)
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
        __syncthreads();
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
        c2<T>* out = y + f * M;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int q = tid + j * nthr;
            if (q < M) out[q] = r[q];
        }
        // the next frame's ring write touches neither a nor b; its barrier stands before the sums
        // that overwrite a, and r is read above
    }
}

// Which kernel a handle runs and the sliding kernel's frames per workgroup on a long block: a
// function of the shape and the two knobs alone (sdsp_oschan_info).
//   kernel: a sliding request runs the sliding kernel where its ring (K M + D samples) and the
//           Stockham pair (2 M) fit kChanLdsCap, else the per-frame kernel.  Automatic is the
//           sliding kernel where ring, pair and table take at most kOschanLdsAuto, ten workgroups to
//           a CU.  Measured at K = 8, D = M/2, complex f32: the sliding kernel
//           takes 0.72 and 0.80 of the per-frame kernel's time at M = 64 and 128 (6 and 12 KiB), the
//           same time at M = 256 (24 KiB), 1.09 and 1.37 times at M = 512 and 1024 (47 and 94 KiB,
//           three and one workgroup to a CU).  Other K: the same bound, reasoned, not measured.
//   frames: the knob when set.  Automatic: max(32, 2 ceil((K M - D) / D)).  Measured at M = 64 and
//           128, K = 8: 16 to 64 frames are level, 128 cost 4 to 9 %, 512 cost 25 to 40 %; 8 frames,
//           whose fill re-reads twice the input, cost 3 to 14 %: the fill comes from L2, so it only
//           has to stay below the chunk's own reads.
OschanPlan oschan_plan(bool f64, int M, int K, int D, int kernel, int frames_per_block) {
    const size_t sample = f64 ? 16 : 8;
    const size_t base = ((size_t)K * M + (size_t)D + 2 * (size_t)M) * sample;
    const bool fits = base <= kChanLdsCap, pays = base + (size_t)M * sample <= kOschanLdsAuto;
    OschanPlan p;
    p.kernel = (kernel == kOschanSlide && fits) || (kernel == 0 && pays) ? kOschanSlide : kOschanPerFrame;
    if (p.kernel == kOschanPerFrame) p.frames_per_block = 1;
    else if (frames_per_block > 0) p.frames_per_block = (size_t)frames_per_block;
    else {
        const size_t fill = ((size_t)K * M - 1) / D;  // ceil((K M - D) / D): the fill, in frames
        p.frames_per_block = 2 * fill > 32 ? 2 * fill : 32;
    }
    return p;
}

template <typename T, int NPT>
hipError_t launch_oschan_n(const OschanArgs& a, const OschanPlan& p, int thr, hipStream_t s) {
    const c2<T>* x = (const c2<T>*)a.x;
    const c2<T>* hist = (const c2<T>*)a.hist;
    if (p.kernel == kOschanPerFrame) {
        dim3 grid((unsigned)a.frames, (unsigned)a.streams);
        hipLaunchKernelGGL((oschan_frame_kernel<T>), grid, dim3(thr), 2 * (size_t)a.M * sizeof(c2<T>), s, x, hist,
                           (const T*)a.cbt, (c2<T>*)a.y, (const c2<T>*)a.tw, a.M, a.logM, a.K, a.D, a.phase,
                           (long long)a.n, (long long)a.frames);
        return hipGetLastError();
    }
    // never below the fill's own length in frames, ceil((K M - D) / D): the fill then doubles the
    // reads at most.  (Reasoned, not measured.)
    const size_t F = chunk_frames(p.frames_per_block, a.frames_per_block > 0, a.frames, a.streams,
                                  ((size_t)a.K * a.M - 1) / a.D);
    dim3 grid((unsigned)((a.frames + F - 1) / F), (unsigned)a.streams);
    const size_t base = ((size_t)a.K * a.M + a.D + 2 * (size_t)a.M) * sizeof(c2<T>);
    const size_t table = (size_t)a.M * sizeof(c2<T>);
    const bool twl = base + table <= kChanLdsAll;
    chan_dispatch_k(a.K, [&](auto k) {
        // (K NPT > 40 fits no precision's 128 KiB: those depths get no register instance of their own)
        constexpr int KC = decltype(k)::value * NPT <= 40 ? decltype(k)::value : 0;
        const auto kernel = twl ? oschan_slide_kernel<T, NPT, KC, true> : oschan_slide_kernel<T, NPT, KC, false>;
        hipLaunchKernelGGL(kernel, grid, dim3(thr), twl ? base + table : base, s, x, hist, (const T*)a.cbt,
                           (c2<T>*)a.y, (const c2<T>*)a.tw, a.M, a.logM, a.K, a.D, a.phase, (long long)a.n,
                           (long long)a.frames, (int)F);
    });
    return hipGetLastError();
}

template <typename T>
hipError_t launch_oschan_t(const OschanArgs& a, const OschanPlan& p, hipStream_t s) {
    const int thr = chan_threads(a.M);  // NPT branches per lane cover the frame
    return chan_dispatch_npt(a.M, thr,
                             [&](auto npt) { return launch_oschan_n<T, decltype(npt)::value>(a, p, thr, s); });
}

hipError_t launch_oschan(bool f64, const OschanArgs& a, hipStream_t s) {
    if (a.frames == 0) return hipSuccess;
    const OschanPlan p = oschan_plan(f64, a.M, a.K, a.D, a.kernel, a.frames_per_block);
    return f64 ? launch_oschan_t<double>(a, p, s) : launch_oschan_t<float>(a, p, s);
}

}  // namespace sdsp

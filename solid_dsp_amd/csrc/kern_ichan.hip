// Synthesis channeliser: the inverse FFT fused into the polyphase bank (gfx950).
//
// The counterpart of the PFB + FFT channeliser (kern_fft.hip): M baseband channels in, one
// wideband stream out.  Per stream, with cb[r][i] = g[r + (K-1-i) M] (the analysis channeliser's
// own branch table) and frames before the handle's first equal to zero,
//   u[m]       = REVERSE_FFT_M(X[m])                 (e^{+j 2 pi k q / M}, unnormalised)
//   y[m M + r] = sum_{i<K} cb[r][i] * u[m-i][M-1-r]  r = 0 .. M-1
// One definition of the arithmetic, no algorithm switch: the transform is stockham<T, true> on
// the make_twiddles(M) table (what sdsp_fft REVERSE runs up to 4096 points), the branch sum
// starts from a zero accumulator and runs i = 0, 1, .., K-1 (newest frame first), and each of its
// steps is acc + c * v with a rounded multiply and a rounded add (-ffp-contract=off).  So the two
// kernels below are bit-identical to each other and to the same sums done on the output of an
// FFT handle.
//
// The coefficients arrive as cbt[i][r] = cb[r][i] ([K][M]): lane r reads cbt[i][r], consecutive
// lanes consecutive addresses.  Lane `tid` owns outputs r = tid + j * blockDim.x, j < NPT; it reads
// u[M-1-r]: consecutive lanes walk one LDS row downwards, 8 bytes each for complex f32, which
// ds_read_b64 serves without a bank conflict (32 lanes on 64 distinct banks).
//
//   ichan_frame_kernel  grid (frame, stream).  K transforms per frame, 2 M samples of LDS: fits
//                       every shape; the fallback and the cross-check.
//   ichan_ring_kernel   grid (chunk of F frames, stream).  The K most recent transformed frames
//                       stay in LDS: one HBM read, one transform and K multiply-adds per output
//                       sample, (K-1)/F extra reads for the chunk's warm-up.
#include "sdsp_chan_dev.hpp"
#include "sdsp_device.hpp"
#include "sdsp_fft_dev.hpp"
#include "sdsp_kernels.hpp"

namespace sdsp {

namespace {

// frame f of one stream: from the block, or from the history ([(K-1) M], oldest first) when f < 0
template <typename T>
__device__ __forceinline__ const c2<T>* ichan_src(const c2<T>* x, const c2<T>* hist, long long f, int M, int K) {
    return f >= 0 ? x + f * M : hist + ((long long)(K - 1) + f) * M;
}

// the lane's samples r = tid + j nthr of one frame, into registers
template <typename T, int NPT>
__device__ __forceinline__ void ichan_request(c2<T> (&nx)[NPT], const c2<T>* __restrict__ src, int M, int tid,
                                              int nthr) {
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int r = tid + j * nthr;
        nx[j] = r < M ? src[r] : c2<T>{T(0), T(0)};
    }
}

// acc[j] += c[r] * u[M-1-r] for the lane's outputs r = tid + j nthr
template <typename T, int NPT>
__device__ __forceinline__ void ichan_branch_step(c2<T> (&acc)[NPT], const T* __restrict__ c, const c2<T>* u, int M,
                                                  int tid, int nthr) {
    u = static_cast<const c2<T>*>(__builtin_assume_aligned(u, 2 * sizeof(T)));
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int r = tid + j * nthr;
        if (r < M) chan_mac(acc[j], c[r], u[M - 1 - r]);
    }
}

}  // namespace

template <typename T, int NPT>
__global__ void __launch_bounds__(256)
ichan_frame_kernel(const c2<T>* __restrict__ x, const c2<T>* __restrict__ hist, const T* __restrict__ cbt,
                   c2<T>* __restrict__ y, const c2<T>* __restrict__ tw, int M, int logM, int K, long long n) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    c2<T>* a = reinterpret_cast<c2<T>*>(lds_raw);
    c2<T>* b = a + M;
    const long long m = blockIdx.x;
    const int s = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
    x += (long long)s * n;
    hist += (long long)s * (K - 1) * M;
    y += (long long)s * n + m * M;
    c2<T> acc[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) acc[j] = {T(0), T(0)};
    for (int i = 0; i < K; ++i) {
        const c2<T>* src = ichan_src(x, hist, m - i, M, K);
        for (int e = tid; e < M; e += nthr) a[e] = src[e];
        __syncthreads();
        const c2<T>* u = stockham<T, true>(a, b, M, logM, tw, tid, nthr);  // (ends on a barrier)
        ichan_branch_step<T, NPT>(acc, cbt + (long long)i * M, u, M, tid, nthr);
        __syncthreads();  // u is a or b: the next frame's load and first pass overwrite both
    }
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int r = tid + j * nthr;
        if (r < M) y[r] = acc[j];
    }
}

// LDS: a ring of K+1 slots of M samples.  Before frame f is transformed, frame f-i (i = 1 .. K-1)
// sits in slot (q - i) mod (K+1), and slots q and q+1 are free: the Stockham ping-pong pair.  The
// frame is loaded into whichever of the two makes the result land in slot q (q when the number of
// passes is even, q+1 when it is odd).  Frame f-(K-1) retires after this frame's sums, so the free
// pair of the next frame is {q+1, q+2} and q moves on by one: no slot is ever copied.
//
// KC = K for K = 1 .. 8 (the depths the streaming analysis kernel has too), 0 for any other K.  A
// lane's outputs r never change, so with KC > 0 its K NPT coefficients are read once per workgroup
// and stay in registers (at most 64 values: K M <= 16384 samples and M / 256 outputs per lane);
// with KC = 0 every frame re-reads them through the cache.  The sums are the same either way.
//
// TWL: the twiddle table sits in LDS behind the ring (M more samples; every shape but the ones whose
// ring alone is within M samples of the 160 KiB).  A twiddle read from global memory inside a pass
// would queue behind the next frame's request, which is in flight across the transform: vmcnt
// counts loads in issue order, so the first pass would wait for HBM.  With the table in LDS (and
// KC > 0) the transform and the sums issue no vector-memory load at all.
template <typename T, int NPT, int KC, bool TWL>
__global__ void __launch_bounds__(256)
ichan_ring_kernel(const c2<T>* __restrict__ x, const c2<T>* __restrict__ hist, const T* __restrict__ cbt,
                  c2<T>* __restrict__ y, const c2<T>* __restrict__ tw, int M, int logM, int K, long long n,
                  long long frames, int F) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    c2<T>* ring = reinterpret_cast<c2<T>*>(lds_raw);
    const int s = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
    const long long m0 = (long long)blockIdx.x * F;  // the chunk emits frames [m0, m1)
    const long long m1 = m0 + F < frames ? m0 + F : frames;
    x += (long long)s * n;
    hist += (long long)s * (K - 1) * M;
    y += (long long)s * n;
    const bool odd = ((logM & 1) + (logM >> 1)) & 1;  // Stockham passes: one radix-2 when logM is odd, then radix-4
    if constexpr (KC > 0) K = KC;
    const c2<T>* twp = tw;
    if constexpr (TWL) {  // (visible to every lane after the first frame's barrier below)
        c2<T>* t = ring + (size_t)(K + 1) * M;
        for (int e = tid; e < M; e += nthr) t[e] = tw[e];
        twp = t;
    }
    T cf[KC > 0 ? KC : 1][NPT];
    if constexpr (KC > 0) {
#pragma unroll
        for (int i = 0; i < KC; ++i)
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const int r = tid + j * nthr;
                cf[i][j] = r < M ? cbt[(long long)i * M + r] : T(0);
            }
    }
    c2<T> nx[NPT];  // the next frame, requested one frame ahead
    long long f = m0 - (K - 1);  // K-1 warm-up frames: transformed, nothing emitted
    ichan_request<T, NPT>(nx, ichan_src(x, hist, f, M, K), M, tid, nthr);
    int q = 0;
    for (; f < m1; ++f) {
        const int q1 = q == K ? 0 : q + 1;
        c2<T>* a = ring + (size_t)(odd ? q1 : q) * M;
        c2<T>* b = ring + (size_t)(odd ? q : q1) * M;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int r = tid + j * nthr;
            if (r < M) a[r] = nx[j];
        }
        __syncthreads();
        if (f + 1 < m1) ichan_request<T, NPT>(nx, ichan_src(x, hist, f + 1, M, K), M, tid, nthr);
        stockham<T, true>(a, b, M, logM, twp, tid, nthr);  // lands in slot q, ends on a barrier
        if (f >= m0) {
            c2<T> acc[NPT];
#pragma unroll
            for (int j = 0; j < NPT; ++j) acc[j] = {T(0), T(0)};
            int sl = q;
            if constexpr (KC > 0) {
#pragma unroll
                for (int i = 0; i < KC; ++i) {
                    const c2<T>* u = static_cast<const c2<T>*>(
                        __builtin_assume_aligned(ring + (size_t)sl * M, 2 * sizeof(T)));
#pragma unroll
                    for (int j = 0; j < NPT; ++j) {
                        const int r = tid + j * nthr;
                        if (r < M) chan_mac(acc[j], cf[i][j], u[M - 1 - r]);
                    }
                    sl = sl == 0 ? KC : sl - 1;
                }
            } else {
                for (int i = 0; i < K; ++i) {
                    ichan_branch_step<T, NPT>(acc, cbt + (long long)i * M, ring + (size_t)sl * M, M, tid, nthr);
                    sl = sl == 0 ? K : sl - 1;
                }
            }
            c2<T>* out = y + f * M;
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const int r = tid + j * nthr;
                if (r < M) out[r] = acc[j];
            }
        }
        __syncthreads();  // the oldest slot, read above, is one of the next frame's free pair
        q = q1;
    }
}

// Which kernel a handle runs and the ring kernel's frames per workgroup on a long block: a
// function of the shape and the two knobs alone (sdsp_ichan_info).
//   kernel: the ring kernel where its K+1 slots fit kChanLdsCap, unless the per-frame kernel is
//           asked for; a ring request that does not fit runs the per-frame kernel.
//   frames: the knob when set.  Automatic: max(128, 8 (K-1)).  The warm-up then re-reads at most an
//           eighth of the input, 7/128 of it at K = 8, and a block of 2^17 frames is 1024
//           workgroups, four for each of the 256 CUs.  Measured at 2^27 samples, K = 8 (DESIGN.md
//           section 4): 128 and 256 frames are level at M = 1024, 64 and 128 at M = 64; 32 frames
//           cost 5 to 8 %, 8 frames 47 to 54 %, and 512 frames (256 workgroups at M = 1024) 42 to 60 %.
IchanPlan ichan_plan(bool f64, int M, int K, int kernel, int frames_per_block) {
    const size_t sample = f64 ? 16 : 8;
    const bool fits = ((size_t)K + 1) * (size_t)M * sample <= kChanLdsCap;
    IchanPlan p;
    p.kernel = kernel != kIchanPerFrame && fits ? kIchanRing : kIchanPerFrame;
    if (p.kernel == kIchanPerFrame) p.frames_per_block = 1;
    else if (frames_per_block > 0) p.frames_per_block = (size_t)frames_per_block;
    else p.frames_per_block = (size_t)(8 * (K - 1) > 128 ? 8 * (K - 1) : 128);
    return p;
}

template <typename T, int NPT>
hipError_t launch_ichan_n(const IchanArgs& a, const IchanPlan& p, int thr, hipStream_t s) {
    const c2<T>* x = (const c2<T>*)a.x;
    const c2<T>* hist = (const c2<T>*)a.hist;
    if (p.kernel == kIchanPerFrame) {
        dim3 grid((unsigned)a.frames, (unsigned)a.streams);
        hipLaunchKernelGGL((ichan_frame_kernel<T, NPT>), grid, dim3(thr), 2 * (size_t)a.M * sizeof(c2<T>), s, x, hist,
                           (const T*)a.cbt, (c2<T>*)a.y, (const c2<T>*)a.tw, a.M, a.logM, a.K, (long long)a.n);
        return hipGetLastError();
    }
    // never below K frames: the warm-up then doubles the reads at most (the per-frame kernel reads and
    // transforms K times)
    const size_t F = chunk_frames(p.frames_per_block, a.frames_per_block > 0, a.frames, a.streams, (size_t)a.K);
    dim3 grid((unsigned)((a.frames + F - 1) / F), (unsigned)a.streams);
    const size_t ring = ((size_t)a.K + 1) * a.M * sizeof(c2<T>), table = (size_t)a.M * sizeof(c2<T>);
    const bool twl = ring + table <= kChanLdsAll;  // (all but M = 4096, K = 1 in complex f64)
    chan_dispatch_k(a.K, [&](auto kc) {
        constexpr int KC = decltype(kc)::value;
        const auto kernel = twl ? ichan_ring_kernel<T, NPT, KC, true> : ichan_ring_kernel<T, NPT, KC, false>;
        hipLaunchKernelGGL(kernel, grid, dim3(thr), twl ? ring + table : ring, s, x, hist, (const T*)a.cbt,
                           (c2<T>*)a.y, (const c2<T>*)a.tw, a.M, a.logM, a.K, (long long)a.n, (long long)a.frames,
                           (int)F);
    });
    return hipGetLastError();
}

template <typename T>
hipError_t launch_ichan_t(const IchanArgs& a, const IchanPlan& p, hipStream_t s) {
    const int thr = chan_threads(a.M);  // NPT outputs per lane cover the frame
    return chan_dispatch_npt(a.M, thr, [&](auto npt) { return launch_ichan_n<T, decltype(npt)::value>(a, p, thr, s); });
}

hipError_t launch_ichan(bool f64, const IchanArgs& a, hipStream_t s) {
    if (a.frames == 0) return hipSuccess;
    const IchanPlan p = ichan_plan(f64, a.M, a.K, a.kernel, a.frames_per_block);
    return f64 ? launch_ichan_t<double>(a, p, s) : launch_ichan_t<float>(a, p, s);
}

}  // namespace sdsp

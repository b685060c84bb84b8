// C-ABI runtime for FFT (src/fft/mod.rs:175-215), the PFB + FFT channeliser
// (build-defined), its synthesis counterpart (sdsp_ichan), its oversampled form
// (sdsp_oschan), the spectrometer on that form (sdsp_spec) and batched DotProduct::execute
// (src/dot_product/mod.rs:153-171).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "sdsp.h"
#include "sdsp_host.hpp"
#include "sdsp_kernels.hpp"

using namespace sdsp;

namespace {

bool is_pow2(size_t n) { return n && !(n & (n - 1)); }
int ilog2(size_t n) {
    int l = 0;
    while ((size_t)1 << l < n) ++l;
    return l;
}

// e^{-j 2 pi m / N}, computed in f64, stored as c32 or c64
int make_twiddles(DevBuf& buf, size_t N, bool f64) {
    std::vector<double> w(2 * N);
    for (size_t m = 0; m < N; ++m) {
        const double a = -2.0 * M_PI * (double)m / (double)N;
        w[2 * m] = std::cos(a);
        w[2 * m + 1] = std::sin(a);
    }
    if (f64) {
        SDSP_TRY(buf.ensure(w.size() * 8), "alloc twiddles");
        SDSP_TRY(hipMemcpy(buf.p, w.data(), w.size() * 8, hipMemcpyHostToDevice), "copy twiddles");
    } else {
        std::vector<float> f(w.begin(), w.end());
        SDSP_TRY(buf.ensure(f.size() * 4), "alloc twiddles");
        SDSP_TRY(hipMemcpy(buf.p, f.data(), f.size() * 4, hipMemcpyHostToDevice), "copy twiddles");
    }
    return SDSP_OK;
}

// power-of-two transform: Stockham in LDS (N <= 4096) or the four-step
// decomposition N = N1 N2 (two strided passes, inter-pass twiddle) above
struct Pow2Plan {
    size_t N = 0;
    int group = 4, wave1024 = 16;  // pass kernel knobs (SDSP_TUNE_FFT_GROUP / SDSP_TUNE_FFT_WAVE1024)
    int logN = 0, l1 = 0, l2 = 0;
    DevBuf tw, tw1, tw2, twx;
    bool four_step() const { return N > 4096; }
    int build(size_t n, bool f64) {
        N = n;
        logN = ilog2(n);
        if (!four_step()) return make_twiddles(tw, N, f64);
        l1 = logN / 2;
        l2 = logN - l1;
        int st = make_twiddles(tw1, (size_t)1 << l1, f64);
        if (st) return st;
        st = make_twiddles(tw2, (size_t)1 << l2, f64);
        if (st || f64 || l1 != 10 || l2 != 10) return st;
        // 2^20 = 1024 x 1024, complex f32: the wave-FFT passes take the inter-pass
        // twiddle W_N^m as Th[m >> 10] * Tl[m & 1023] (each from f64)
        std::vector<float> t(4 * 1024);
        for (int j = 0; j < 1024; ++j) {
            const double a = -2.0 * M_PI * (double)j / (double)N, b = -2.0 * M_PI * (double)j * 1024.0 / (double)N;
            t[2 * j] = (float)std::cos(a);
            t[2 * j + 1] = (float)std::sin(a);
            t[2048 + 2 * j] = (float)std::cos(b);
            t[2048 + 2 * j + 1] = (float)std::sin(b);
        }
        SDSP_TRY(twx.ensure(t.size() * 4), "alloc twiddles");
        SDSP_TRY(hipMemcpy(twx.p, t.data(), t.size() * 4, hipMemcpyHostToDevice), "copy twiddles");
        return SDSP_OK;
    }
    // in -> out (may alias); tmp: batch * N samples when four_step()
    hipError_t run(bool f64, const void* in, void* out, void* tmp, size_t batch, bool inverse, hipStream_t s) const {
        if (!four_step()) {
            FftArgs a{in, out, tw.p, (int)N, logN, true, inverse, batch};
            return launch_fft(f64, a, s);
        }
        const long long n = (long long)N, N1 = 1LL << l1, N2 = 1LL << l2;
        // pass 1: columns n2 (length N1, stride N2) -> tmp[k1][n2] * W_N^(n2 k1)
        FftPass p1{in, tmp, tw1.p, (int)N1, l1, (long long)batch * N2, N2, n, 1, N2, 1, N2, n, inverse, twx.p,
                   group, wave1024};
        hipError_t e = launch_fft_pass(f64, p1, s);
        if (e != hipSuccess) return e;
        // pass 2: rows k1 (length N2) -> out[k1 + N1 k2]
        FftPass p2{tmp, out, tw2.p, (int)N2, l2, (long long)batch * N1, N1, n, N2, 1, 1, N1, 0, inverse, nullptr,
                   group, wave1024};
        return launch_fft_pass(f64, p2, s);
    }
};

int upload(DevBuf& buf, const std::vector<double>& v, bool f64) {
    if (f64) {
        SDSP_TRY(buf.ensure(v.size() * 8), "alloc");
        SDSP_TRY(hipMemcpy(buf.p, v.data(), v.size() * 8, hipMemcpyHostToDevice), "upload");
    } else {
        std::vector<float> f(v.begin(), v.end());
        SDSP_TRY(buf.ensure(f.size() * 4), "alloc");
        SDSP_TRY(hipMemcpy(buf.p, f.data(), f.size() * 4, hipMemcpyHostToDevice), "upload");
    }
    return SDSP_OK;
}

constexpr size_t kDirectMax = 512;  // non-power-of-two sizes up to this run the direct DFT

}  // namespace

// (records no fence: calls on different streams share the scratch buffers unordered)
struct sdsp_fft : HandleCore {
    size_t N = 0;
    int direction = 0;  // 0 FORWARD, 1 REVERSE
    bool f64 = true;
    int kind = 0;       // 0 direct DFT, 1 power of two, 2 Bluestein
    DevBuf tw;
    Pow2Plan p2;        // kind 1: the transform; kind 2: the length-M convolution transform
    size_t M = 0;       // Bluestein convolution length (power of two >= 2N - 1)
    DevBuf chirp, spec; // Bluestein: w[N] of the direction, B[M] = FFT_M(conj chirp) / M
    DevBuf work, tmp;   // device scratch, grown with the batch
};

constexpr size_t kSpecMaxIntegration = 32768;  // 1024 sub-blocks of 32 frames

// The strings of a channeliser family that differ from its siblings'
struct ChanText {
    const char *dtype, *block, *overlap;  // refusals: create's dtype, a block's length, an in-place block
    const char *create, *launch;          // what a device error names
};

// What the three channeliser handles share: an M-point power-of-two transform and a K-deep
// polyphase bank over frames `step` samples apart (M for sdsp_chan and sdsp_ichan, D <= M for
// sdsp_oschan).  A block of n samples per stream is n / step frames and frames * M outputs; the
// history keeps the K M - step samples before the block, which is (K-1) M at step = M.
struct ChanCore : HandleCore {
    const ChanText* text = nullptr;
    int dtype = SDSP_RC32;
    size_t M = 0, K = 0, step = 0, streams = 1;
    DevBuf table, tw;  // the branch coefficients in the family's layout; make_twiddles(M)
    PingPong hist;     // [streams][K M - step] input samples, oldest first
    size_t phase = 0;  // (samples so far) mod M: stays 0 at step = M
    int kernel = 0;    // SDSP_TUNE_*CHAN_KERNEL
    int fpb = 0;       // SDSP_TUNE_*CHAN_FRAMES_PER_BLOCK

    // create's argument checks in their one order, then the device (`integration`: sdsp_spec's A, 1 elsewhere)
    static int check(const ChanText& t, int dtype, const void* taps, size_t len, size_t M, size_t step, int device,
                     size_t integration = 1) {
        if (dtype != SDSP_RC32 && dtype != SDSP_RC64) { set_error(t.dtype); return SDSP_E_UNSUPPORTED; }
        if (!taps && len > 0) { set_error("taps pointer is null"); return SDSP_E_INVALID_ARGUMENT; }
        if (M == 0) { set_error("FIR Filter Error NotEnoughFilters"); return SDSP_E_NOT_ENOUGH_FILTERS; }
        if (len == 0) { set_error("FIR Filter Error CoefficientsLengthZero"); return SDSP_E_COEFFICIENTS_LENGTH_ZERO; }
        if (!is_pow2(M) || M < 4 || M > 4096) {
            set_error("channel count must be a power of two in [4, 4096]");
            return SDSP_E_UNSUPPORTED;
        }
        if (step == 0 || step > M) {  // (sdsp_oschan's D; M itself for the other two)
            set_error("decimation (the frame stride) must be in [1, channels]");
            return SDSP_E_UNSUPPORTED;
        }
        if (integration == 0 || integration > kSpecMaxIntegration) {
            set_error("integration must be in [1, 32768] frames (sum finished spectra for more)");
            return SDSP_E_UNSUPPORTED;
        }
        if (len < M) { set_error("fewer taps than channels"); return SDSP_E_INVALID_ARGUMENT; }
        return check_device(device, nullptr);
    }
    // Checked arguments -> a handle with one stream of zero history.  Row i of the table is the taps'
    // block K-1-i, cbt[i][p] = h[p + (K-1-i) M] ([K][M]); `by_branch` stores its transpose,
    // cb[p][i] ([M][K], pfb.rs:33-40).  Taps beyond K M are ignored.
    int init(const ChanText& t, int dt, const void* taps, size_t len, size_t channels, size_t stride, bool by_branch,
             int dev) {
        text = &t;
        dtype = dt;
        M = channels;
        K = len / M;
        step = stride;
        const size_t cbytes = coef_bytes(dtype);
        const unsigned char* src = (const unsigned char*)taps;
        std::vector<unsigned char> tab(K * M * cbytes);
        for (size_t i = 0; i < K; ++i)
            for (size_t p = 0; p < M; ++p)
                std::memcpy(&tab[(by_branch ? p * K + i : i * M + p) * cbytes], src + (p + (K - 1 - i) * M) * cbytes,
                            cbytes);
        hipError_t e = open(dev);
        if (e == hipSuccess) e = table.ensure(tab.size());
        if (e == hipSuccess) e = hipMemcpy(table.p, tab.data(), tab.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return device_status(e, t.create);
        const int st = make_twiddles(tw, M, dtype == SDSP_RC64);
        return st ? st : set_streams(1);
    }
    // also the reset: zero history in both halves, phase 0, nothing queued
    int set_streams(size_t count) {
        if (count == 0) return SDSP_E_INVALID_ARGUMENT;
        DeviceGuard g(device);
        SDSP_TRY(fence.wait(), "wait for queued work");  // a queued block may still read the history
        streams = count;
        SDSP_TRY(hist.reset(streams * (K * M - step) * sample_bytes(dtype), stream), "zero history");
        phase = 0;
        return quiesce();
    }
    int synchronize() const {
        DeviceGuard g(device);
        return quiesce();
    }
    // One device block of n samples per stream on the caller's stream (or the handle's):
    // launch(d_in, n, frames, d_out, stream) -> hipError_t queues the family's kernel, which reads
    // hist.front() and `phase`; then the history moves on by the n inputs.
    template <typename Launch>
    int block_device(const void* d_in, size_t n, void* d_out, size_t* frames, void* user_stream, Launch launch) {
        if (n % step) { set_error(text->block); return SDSP_E_INVALID_ARGUMENT; }
        const size_t fr = n / step;
        if (frames) *frames = fr;
        if (fr == 0) return SDSP_OK;
        const size_t sb = streams * sample_bytes(dtype);
        if (ranges_overlap(d_in, n * sb, d_out, fr * M * sb)) {
            set_error(text->overlap);
            return SDSP_E_INVALID_ARGUMENT;
        }
        DeviceGuard g(device);
        hipStream_t s = pick(user_stream, stream);
        SDSP_TRY(fence.order_before(s), "order after queued work");  // the history this launch reads
        SDSP_TRY(launch(d_in, n, fr, d_out, s), text->launch);
        SDSP_TRY(launch_hist_update(dtype, d_in, hist.front(), hist.back(), n, (int)(K * M - step), streams, s),
                 "history update");
        hist.flip();
        phase = (phase + n) % M;
        SDSP_TRY(fence.record(s), "record fence");
        return SDSP_OK;
    }
    // The host-slice twin: [streams][n] in and [streams][frames][M] out through the staging buffers
    template <typename Launch> int block_host(const void* in, size_t n, void* out, size_t* frames, Launch launch) {
        DeviceGuard g(device);
        if (n % step) { set_error(text->block); return SDSP_E_INVALID_ARGUMENT; }
        const size_t fr = n / step, sb = streams * sample_bytes(dtype);
        if (frames) *frames = fr;
        if (n == 0) return SDSP_OK;
        return staged(in, n * sb, out, fr * M * sb, [&](const void* d_in, void* d_out, hipStream_t s) {
            return block_device(d_in, n, d_out, nullptr, s, launch);
        });
    }
};

// *_create: null `out`, the checks, then a handle of type H on `device`
template <typename H>
int chan_create(H** out, const ChanText& t, int dtype, const void* taps, size_t len, size_t M, size_t step,
                bool by_branch, int device, size_t integration = 1) {
    if (!out) return SDSP_E_INVALID_ARGUMENT;
    *out = nullptr;
    int st = ChanCore::check(t, dtype, taps, len, M, step, device, integration);
    if (st) return st;
    DeviceGuard g(device);
    H* h = new H();
    st = h->init(t, dtype, taps, len, M, step, by_branch, device);
    if (st) { destroy_handle(h); return st; }
    *out = h;
    return SDSP_OK;
}

struct sdsp_chan : ChanCore {
    int fast = 5;     // streaming M = 1024 kernel variant (SDSP_TUNE_CHAN_STREAMING): 8-frame rounds
    bool xcd = true;  // XCD-contiguous chunk order (SDSP_TUNE_CHAN_XCD_ORDER)
    auto launcher() {
        return [this](const void* d_in, size_t n, size_t fr, void* d_out, hipStream_t s) {
            ChanArgs a{d_in, hist.front(), table.p, d_out, tw.p, (int)M, ilog2(M), (int)K, n, fr, streams};
            a.fast = fast;
            a.frames_per_block = fpb;
            a.xcd_order = xcd;
            return launch_chan(dtype == SDSP_RC64, a, s);
        };
    }
};

struct sdsp_ichan : ChanCore {  // (the history holds untransformed input frames)
    auto launcher() {
        return [this](const void* d_in, size_t n, size_t fr, void* d_out, hipStream_t s) {
            const IchanArgs a{d_in, hist.front(), table.p, d_out, tw.p, (int)M, ilog2(M), (int)K,
                              n, fr, streams, kernel, fpb};
            return launch_ichan(dtype == SDSP_RC64, a, s);
        };
    }
};

struct sdsp_oschan : ChanCore {
    auto launcher() {
        return [this](const void* d_in, size_t n, size_t fr, void* d_out, hipStream_t s) {
            const OschanArgs a{d_in, hist.front(), table.p, d_out, tw.p, (int)M, ilog2(M), (int)K,
                               (int)step, (int)phase, n, fr, streams, kernel, fpb};
            return launch_oschan(dtype == SDSP_RC64, a, s);
        };
    }
};

// The oversampled channeliser's frames squared and integrated A at a time.  On top of ChanCore's
// history and phase: the open sub-block's sum, the open integration's closed sub-blocks and the
// frames in the open integration, all zero after create, reset and set_streams; the scale survives.
struct sdsp_spec : ChanCore {
    size_t A = 1, filled = 0;
    double scale = 1.0;  // rounded to the real type
    int subblocks = 0;   // SDSP_TUNE_SPEC_SUBBLOCKS
    PingPong sub, tot;   // [streams][M] reals each
    DevBuf part;         // the call's closed sub-blocks, grown on demand

    size_t real_bytes() const { return sample_bytes(dtype) / 2; }
    int set_streams(size_t count) {
        const int st = ChanCore::set_streams(count);
        if (st) return st;
        DeviceGuard g(device);
        SDSP_TRY(sub.reset(streams * M * real_bytes(), stream), "zero sums");
        SDSP_TRY(tot.reset(streams * M * real_bytes(), stream), "zero sums");
        filled = 0;
        return quiesce();
    }
    // One device block: ChanCore::block_device's order of steps, with spectra M reals per stream out
    int block_device(const void* d_in, size_t n, void* d_out, size_t* spectra, void* user_stream) {
        if (n % step) { set_error(text->block); return SDSP_E_INVALID_ARGUMENT; }
        const size_t fr = n / step, sp = (filled + fr) / A;
        if (spectra) *spectra = sp;
        if (fr == 0) return SDSP_OK;
        if (!d_in || (sp && !d_out)) { set_error("block pointer is null"); return SDSP_E_INVALID_ARGUMENT; }
        if (ranges_overlap(d_in, n * streams * sample_bytes(dtype), d_out, sp * M * streams * real_bytes())) {
            set_error(text->overlap);
            return SDSP_E_INVALID_ARGUMENT;
        }
        DeviceGuard g(device);
        hipStream_t s = pick(user_stream, stream);
        // (a larger scratch frees the old one, which waits for the device)
        SDSP_TRY(part.ensure(streams * spec_subblocks(filled, A, fr) * M * real_bytes()), "spectrometer scratch");
        SDSP_TRY(fence.order_before(s), "order after queued work");
        const SpecArgs a{d_in, hist.front(), table.p, tw.p, sub.front(), sub.back(), tot.front(), tot.back(),
                         part.p, d_out, (int)M, ilog2(M), (int)K, (int)step, (int)phase, (int)A, (int)filled,
                         scale, n, fr, streams, kernel, subblocks};
        SDSP_TRY(launch_spec(dtype == SDSP_RC64, a, s), text->launch);
        SDSP_TRY(launch_hist_update(dtype, d_in, hist.front(), hist.back(), n, (int)(K * M - step), streams, s),
                 "history update");
        hist.flip();
        sub.flip();
        tot.flip();
        phase = (phase + n) % M;
        filled = (filled + fr) % A;
        SDSP_TRY(fence.record(s), "record fence");
        return SDSP_OK;
    }
    int block_host(const void* in, size_t n, void* out, size_t* spectra) {
        DeviceGuard g(device);
        if (n % step) { set_error(text->block); return SDSP_E_INVALID_ARGUMENT; }
        const size_t sp = (filled + n / step) / A;
        if (spectra) *spectra = sp;
        if (n == 0) return SDSP_OK;
        return staged(in, n * streams * sample_bytes(dtype), out, sp * M * streams * real_bytes(),
                      [&](const void* d_in, void* d_out, hipStream_t s) {
                          return block_device(d_in, n, d_out, nullptr, s);
                      });
    }
};

constexpr ChanText kChanText{"channeliser takes real taps and complex samples (SDSP_RC32 / SDSP_RC64)",
                             "channeliser blocks must be a whole number of M-sample frames",
                             "input and output blocks overlap (in-place channelising is not supported)",
                             "chan create", "channeliser"};
constexpr ChanText kIchanText{"synthesis channeliser takes real taps and complex samples (SDSP_RC32 / SDSP_RC64)",
                              "synthesis channeliser blocks must be a whole number of M-sample frames",
                              "input and output blocks overlap (in-place synthesis is not supported)",
                              "ichan create", "synthesis channeliser"};
constexpr ChanText kOschanText{
    "oversampled channeliser takes real taps and complex samples (SDSP_RC32 / SDSP_RC64)",
    "oversampled channeliser blocks must be a whole number of D-sample frame strides",
    "input and output blocks overlap (in-place channelising is not supported)",
    "oschan create", "oversampled channeliser"};

constexpr ChanText kSpecText{
    "spectrometer takes real taps and complex samples (SDSP_RC32 / SDSP_RC64)",
    "spectrometer blocks must be a whole number of D-sample frame strides",
    "input and output blocks overlap",
    "spec create", "spectrometer"};

extern "C" {

// FFT::new(nfft, direction, flags)   src/fft/mod.rs:175-186
int sdsp_fft_create(sdsp_fft** out, size_t nfft, int direction, int precision, int device) {
    if (!out) return SDSP_E_INVALID_ARGUMENT;
    *out = nullptr;
    if (nfft == 0 || nfft > (1u << 24)) {  // the reference panics on a zero-length plan
        set_error("FFT size must be in [1, 2^24]");
        return SDSP_E_INVALID_ARGUMENT;
    }
    // Bluestein convolves at M = the power of two >= 2 nfft - 1: above 2^23 that is 2^25, whose
    // four-step passes would be longer than the 4096 points fft_pass_kernel holds in LDS
    if (!is_pow2(nfft) && nfft > (1u << 23)) {
        set_error("FFT sizes above 2^23 must be powers of two (the chirp-z convolution is at most 2^24 points)");
        return SDSP_E_INVALID_ARGUMENT;
    }
    if (direction != 0 && direction != 1) return SDSP_E_INVALID_ARGUMENT;
    int st = check_device(device, nullptr);
    if (st) return st;
    DeviceGuard g(device);
    sdsp_fft* h = new sdsp_fft();
    h->N = nfft;
    h->direction = direction;
    h->f64 = precision != 0;
    hipError_t e = h->open(device);
    if (e != hipSuccess) { delete h; return device_status(e, "stream"); }
    if (is_pow2(nfft)) {
        h->kind = 1;
        st = h->p2.build(nfft, h->f64);
    } else if (nfft <= kDirectMax) {
        h->kind = 0;
        st = make_twiddles(h->tw, nfft, h->f64);
    } else {
        // Bluestein: X[k] = w[k] sum_n (x[n] w[n]) conj(w[k - n]),  w[n] = e^{-/+ j pi n^2 / N}
        h->kind = 2;
        size_t M = 1;
        while (M < 2 * nfft - 1) M <<= 1;
        h->M = M;
        const double sgn = direction == 1 ? 1.0 : -1.0;
        std::vector<double> w(2 * nfft), bb(2 * M, 0.0);
        for (size_t n = 0; n < nfft; ++n) {
            const unsigned long long q = (unsigned long long)((unsigned __int128)n * n % (2 * (unsigned __int128)nfft));
            const double ang = sgn * M_PI * (double)q / (double)nfft;
            w[2 * n] = std::cos(ang);
            w[2 * n + 1] = std::sin(ang);
            bb[2 * n] = w[2 * n];  // conj(w)
            bb[2 * n + 1] = -w[2 * n + 1];
            if (n) {
                bb[2 * (M - n)] = w[2 * n];
                bb[2 * (M - n) + 1] = -w[2 * n + 1];
            }
        }
        host_fft_pow2(bb, M);
        for (auto& v : bb) v /= (double)M;
        st = upload(h->chirp, w, h->f64);
        if (!st) st = upload(h->spec, bb, h->f64);
        if (!st) st = h->p2.build(M, h->f64);
    }
    if (st) { sdsp_fft_destroy(h); return st; }
    *out = h;
    return SDSP_OK;
}

void sdsp_fft_destroy(sdsp_fft* h) { destroy_handle(h); }

size_t sdsp_fft_len(const sdsp_fft* h) { return h ? h->N : 0; }

int sdsp_fft_set_tuning(sdsp_fft* h, int key, int value) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (key == SDSP_TUNE_FFT_GROUP && value >= 1 && value <= 64) h->p2.group = value;
    else if (key == SDSP_TUNE_FFT_WAVE1024 && (value == 0 || value == 1 || value == 8 || value == 16))
        h->p2.wave1024 = value;
    else return SDSP_E_INVALID_ARGUMENT;
    return SDSP_OK;
}

int sdsp_fft_execute_device(sdsp_fft* h, const void* d_in, void* d_out, size_t batch, void* stream) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (batch == 0) return SDSP_OK;
    DeviceGuard g(h->device);
    hipStream_t s = pick(stream, h->stream);
    const size_t cb = h->f64 ? 16 : 8;
    const bool inv = h->direction == 1;
    if (h->kind == 0) {
        if (d_in == d_out) {  // the direct DFT reads every input per output: work from a copy
            SDSP_TRY(h->work.ensure(batch * h->N * cb), "dft scratch");
            SDSP_TRY(hipMemcpyAsync(h->work.p, d_in, batch * h->N * cb, hipMemcpyDeviceToDevice, s), "dft copy");
            d_in = h->work.p;
        }
        FftArgs a{d_in, d_out, h->tw.p, (int)h->N, ilog2(h->N), false, inv, batch};
        SDSP_TRY(launch_fft(h->f64, a, s), "fft");
    } else if (h->kind == 1) {
        if (h->p2.four_step()) SDSP_TRY(h->tmp.ensure(batch * h->N * cb), "fft scratch");
        SDSP_TRY(h->p2.run(h->f64, d_in, d_out, h->tmp.p, batch, inv, s), "fft");
    } else {
        const long long N = (long long)h->N, M = (long long)h->M;
        SDSP_TRY(h->work.ensure(batch * h->M * cb), "bluestein scratch");
        if (h->p2.four_step()) SDSP_TRY(h->tmp.ensure(batch * h->M * cb), "bluestein scratch");
        SDSP_TRY(launch_bluestein(h->f64, 0, d_in, h->work.p, h->chirp.p, N, M, (long long)batch, s), "bluestein in");
        SDSP_TRY(h->p2.run(h->f64, h->work.p, h->work.p, h->tmp.p, batch, false, s), "bluestein fft");
        SDSP_TRY(launch_bluestein(h->f64, 1, nullptr, h->work.p, h->spec.p, N, M, (long long)batch, s), "bluestein mul");
        SDSP_TRY(h->p2.run(h->f64, h->work.p, h->work.p, h->tmp.p, batch, true, s), "bluestein ifft");
        SDSP_TRY(launch_bluestein(h->f64, 2, h->work.p, d_out, h->chirp.p, N, M, (long long)batch, s), "bluestein out");
    }
    return SDSP_OK;
}

// plan kind (0 direct DFT, 1 power of two in LDS, 2 Bluestein, 3 four-step power of two)
int sdsp_fft_method(const sdsp_fft* h) {
    if (!h) return -1;
    if (h->kind == 1 && h->p2.four_step()) return 3;
    return h->kind;
}

// FFT::execute(&[Complex]) -> Vec<Complex> over `batch` contiguous transforms   src/fft/mod.rs:188-215
int sdsp_fft_execute(sdsp_fft* h, const void* in, void* out, size_t batch) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (batch == 0) return SDSP_OK;
    DeviceGuard g(h->device);
    const size_t bytes = h->N * batch * (h->f64 ? 16 : 8);
    return h->staged(in, bytes, out, bytes, [&](const void* d_in, void* d_out, hipStream_t s) {
        return sdsp_fft_execute_device(h, d_in, d_out, batch, s);
    });
}

// ---- channeliser -----------------------------------------------------------
int sdsp_chan_create(sdsp_chan** out, int dtype, const void* taps, size_t len, size_t M, int device) {
    return chan_create(out, kChanText, dtype, taps, len, M, M, true, device);
}

void sdsp_chan_destroy(sdsp_chan* h) { destroy_handle(h); }

int sdsp_chan_set_streams(sdsp_chan* h, size_t streams) {
    return h ? h->set_streams(streams) : SDSP_E_INVALID_ARGUMENT;
}

int sdsp_chan_set_tuning(sdsp_chan* h, int key, int value) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (key == SDSP_TUNE_CHAN_STREAMING && value >= 0 && value <= 6) h->fast = value;
    else if (key == SDSP_TUNE_CHAN_FRAMES_PER_BLOCK && value >= 0) h->fpb = value;
    else if (key == SDSP_TUNE_CHAN_XCD_ORDER) h->xcd = value != 0;
    else return SDSP_E_INVALID_ARGUMENT;
    return SDSP_OK;
}

int sdsp_chan_reset(sdsp_chan* h) { return h ? h->set_streams(h->streams) : SDSP_E_INVALID_ARGUMENT; }

int sdsp_chan_execute_block_device(sdsp_chan* h, const void* d_in, size_t n, void* d_out, size_t* frames,
                                   void* stream) {
    return h ? h->block_device(d_in, n, d_out, frames, stream, h->launcher()) : SDSP_E_INVALID_ARGUMENT;
}

int sdsp_chan_execute_block(sdsp_chan* h, const void* in, size_t n, void* out, size_t* frames) {
    return h ? h->block_host(in, n, out, frames, h->launcher()) : SDSP_E_INVALID_ARGUMENT;
}

int sdsp_chan_synchronize(sdsp_chan* h) { return h ? h->synchronize() : SDSP_E_INVALID_ARGUMENT; }

// ---- synthesis channeliser ---------------------------------------------------
int sdsp_ichan_create(sdsp_ichan** out, int dtype, const void* taps, size_t len, size_t M, int device) {
    return chan_create(out, kIchanText, dtype, taps, len, M, M, false, device);
}

void sdsp_ichan_destroy(sdsp_ichan* h) { destroy_handle(h); }

int sdsp_ichan_set_streams(sdsp_ichan* h, size_t streams) {
    return h ? h->set_streams(streams) : SDSP_E_INVALID_ARGUMENT;
}

int sdsp_ichan_set_tuning(sdsp_ichan* h, int key, int value) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (key == SDSP_TUNE_ICHAN_KERNEL && value >= 0 && value <= 2) h->kernel = value;
    else if (key == SDSP_TUNE_ICHAN_FRAMES_PER_BLOCK && value >= 0) h->fpb = value;
    else return SDSP_E_INVALID_ARGUMENT;
    return SDSP_OK;
}

int sdsp_ichan_reset(sdsp_ichan* h) { return h ? h->set_streams(h->streams) : SDSP_E_INVALID_ARGUMENT; }

size_t sdsp_ichan_channels(const sdsp_ichan* h) { return h ? h->M : 0; }
size_t sdsp_ichan_subfilter_len(const sdsp_ichan* h) { return h ? h->K : 0; }

int sdsp_ichan_info(const sdsp_ichan* h, int* kernel, size_t* frames_per_block) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    const IchanPlan p = ichan_plan(h->dtype == SDSP_RC64, (int)h->M, (int)h->K, h->kernel, h->fpb);
    if (kernel) *kernel = p.kernel;
    if (frames_per_block) *frames_per_block = p.frames_per_block;
    return SDSP_OK;
}

int sdsp_ichan_execute_block_device(sdsp_ichan* h, const void* d_in, size_t n, void* d_out, size_t* frames,
                                    void* stream) {
    return h ? h->block_device(d_in, n, d_out, frames, stream, h->launcher()) : SDSP_E_INVALID_ARGUMENT;
}

int sdsp_ichan_execute_block(sdsp_ichan* h, const void* in, size_t n, void* out, size_t* frames) {
    return h ? h->block_host(in, n, out, frames, h->launcher()) : SDSP_E_INVALID_ARGUMENT;
}

int sdsp_ichan_synchronize(sdsp_ichan* h) { return h ? h->synchronize() : SDSP_E_INVALID_ARGUMENT; }

// ---- oversampled analysis channeliser ----------------------------------------
int sdsp_oschan_create(sdsp_oschan** out, int dtype, const void* taps, size_t len, size_t M, size_t D, int device) {
    return chan_create(out, kOschanText, dtype, taps, len, M, D, false, device);
}

void sdsp_oschan_destroy(sdsp_oschan* h) { destroy_handle(h); }

int sdsp_oschan_set_streams(sdsp_oschan* h, size_t streams) {
    return h ? h->set_streams(streams) : SDSP_E_INVALID_ARGUMENT;
}

int sdsp_oschan_set_tuning(sdsp_oschan* h, int key, int value) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (key == SDSP_TUNE_OSCHAN_KERNEL && value >= 0 && value <= 2) h->kernel = value;
    else if (key == SDSP_TUNE_OSCHAN_FRAMES_PER_BLOCK && value >= 0) h->fpb = value;
    else return SDSP_E_INVALID_ARGUMENT;
    return SDSP_OK;
}

int sdsp_oschan_reset(sdsp_oschan* h) { return h ? h->set_streams(h->streams) : SDSP_E_INVALID_ARGUMENT; }

size_t sdsp_oschan_channels(const sdsp_oschan* h) { return h ? h->M : 0; }
size_t sdsp_oschan_decimation(const sdsp_oschan* h) { return h ? h->step : 0; }
size_t sdsp_oschan_subfilter_len(const sdsp_oschan* h) { return h ? h->K : 0; }
size_t sdsp_oschan_phase(const sdsp_oschan* h) { return h ? h->phase : 0; }

int sdsp_oschan_info(const sdsp_oschan* h, int* kernel, size_t* frames_per_block) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    const OschanPlan p = oschan_plan(h->dtype == SDSP_RC64, (int)h->M, (int)h->K, (int)h->step, h->kernel, h->fpb);
    if (kernel) *kernel = p.kernel;
    if (frames_per_block) *frames_per_block = p.frames_per_block;
    return SDSP_OK;
}

int sdsp_oschan_execute_block_device(sdsp_oschan* h, const void* d_in, size_t n, void* d_out, size_t* frames,
                                     void* stream) {
    return h ? h->block_device(d_in, n, d_out, frames, stream, h->launcher()) : SDSP_E_INVALID_ARGUMENT;
}

int sdsp_oschan_execute_block(sdsp_oschan* h, const void* in, size_t n, void* out, size_t* frames) {
    return h ? h->block_host(in, n, out, frames, h->launcher()) : SDSP_E_INVALID_ARGUMENT;
}

int sdsp_oschan_synchronize(sdsp_oschan* h) { return h ? h->synchronize() : SDSP_E_INVALID_ARGUMENT; }

// ---- spectrometer --------------------------------------------------------------
int sdsp_spec_create(sdsp_spec** out, int dtype, const void* taps, size_t len, size_t M, size_t D, size_t A,
                     int device) {
    int st = chan_create(out, kSpecText, dtype, taps, len, M, D, false, device, A);
    if (st) return st;
    (*out)->A = A;
    st = (*out)->set_streams(1);  // the sums, which ChanCore::init knows nothing of
    if (st) { destroy_handle(*out); *out = nullptr; }
    return st;
}

void sdsp_spec_destroy(sdsp_spec* h) { destroy_handle(h); }

int sdsp_spec_set_streams(sdsp_spec* h, size_t streams) {
    return h ? h->set_streams(streams) : SDSP_E_INVALID_ARGUMENT;
}

int sdsp_spec_set_tuning(sdsp_spec* h, int key, int value) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (key == SDSP_TUNE_SPEC_KERNEL && value >= 0 && value <= 2) h->kernel = value;
    else if (key == SDSP_TUNE_SPEC_SUBBLOCKS && value >= 0) h->subblocks = value;
    else return SDSP_E_INVALID_ARGUMENT;
    return SDSP_OK;
}

int sdsp_spec_reset(sdsp_spec* h) { return h ? h->set_streams(h->streams) : SDSP_E_INVALID_ARGUMENT; }

int sdsp_spec_set_scale(sdsp_spec* h, double scale) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->scale = h->dtype == SDSP_RC64 ? scale : (double)(float)scale;  // read at each launch
    return SDSP_OK;
}

size_t sdsp_spec_channels(const sdsp_spec* h) { return h ? h->M : 0; }
size_t sdsp_spec_decimation(const sdsp_spec* h) { return h ? h->step : 0; }
size_t sdsp_spec_subfilter_len(const sdsp_spec* h) { return h ? h->K : 0; }
size_t sdsp_spec_integration(const sdsp_spec* h) { return h ? h->A : 0; }
size_t sdsp_spec_phase(const sdsp_spec* h) { return h ? h->phase : 0; }
size_t sdsp_spec_filled(const sdsp_spec* h) { return h ? h->filled : 0; }

int sdsp_spec_info(const sdsp_spec* h, int* kernel, size_t* subblocks_per_workgroup) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    const SpecPlan p = spec_plan(h->dtype == SDSP_RC64, (int)h->M, (int)h->K, (int)h->step, (int)h->A, h->kernel,
                                 h->subblocks);
    if (kernel) *kernel = p.kernel;
    if (subblocks_per_workgroup) *subblocks_per_workgroup = p.subblocks;
    return SDSP_OK;
}

int sdsp_spec_count(size_t decimation, size_t integration, size_t filled, size_t n, size_t* spectra,
                    size_t* next_filled) {
    if (decimation == 0 || integration == 0 || integration > kSpecMaxIntegration || filled >= integration ||
        n % decimation)
        return SDSP_E_INVALID_ARGUMENT;
    const size_t total = filled + n / decimation;
    if (spectra) *spectra = total / integration;
    if (next_filled) *next_filled = total % integration;
    return SDSP_OK;
}

int sdsp_spec_execute_block_device(sdsp_spec* h, const void* d_in, size_t n, void* d_out, size_t* spectra,
                                   void* stream) {
    return h ? h->block_device(d_in, n, d_out, spectra, stream) : SDSP_E_INVALID_ARGUMENT;
}

int sdsp_spec_execute_block(sdsp_spec* h, const void* in, size_t n, void* out, size_t* spectra) {
    return h ? h->block_host(in, n, out, spectra) : SDSP_E_INVALID_ARGUMENT;
}

int sdsp_spec_synchronize(sdsp_spec* h) { return h ? h->synchronize() : SDSP_E_INVALID_ARGUMENT; }

// ---- DotProduct ---------------------------------------------------------------
// batch vectors of n samples (stride samples apart), coefficients as given to
// DotProduct::new(&coefs, direction) (0 FORWARD, 1 REVERSE), device buffers.
int sdsp_dot_execute_batched_device(int dtype, const void* coefs, size_t len, int direction, const void* d_samples,
                                    size_t n, size_t stride, size_t batch, void* d_out, void* stream) {
    if (dtype < 0 || dtype > 5 || direction < 0 || direction > 1) return SDSP_E_INVALID_ARGUMENT;
    if (batch == 0) return SDSP_OK;
    int dev = 0;
    SDSP_TRY(hipGetDevice(&dev), "device");
    int st = check_device(dev, nullptr);
    if (st) return st;
    const size_t cb = coef_bytes(dtype);
    std::vector<unsigned char> c((const unsigned char*)coefs, (const unsigned char*)coefs + len * cb);
    if (direction == 1)
        for (size_t i = 0; i < len / 2; ++i)
            std::swap_ranges(&c[i * cb], &c[i * cb] + cb, &c[(len - 1 - i) * cb]);
    DevBuf d_c;
    SDSP_TRY(d_c.ensure(c.size()), "alloc coefs");
    hipStream_t s = (hipStream_t)stream;
    SDSP_TRY(hipMemcpyAsync(d_c.p, c.data(), c.size(), hipMemcpyHostToDevice, s), "copy coefs");
    DotArgs a{d_c.p, (int)std::min(n, len), d_samples, stride, batch, d_out};
    SDSP_TRY(launch_dot(dtype, a, s), "dot");
    SDSP_TRY(hipStreamSynchronize(s), "sync");  // d_c is released on return
    return SDSP_OK;
}

// single DotProduct::execute over host buffers (out = one sample)
int sdsp_dot_execute(int dtype, const void* coefs, size_t len, int direction, const void* samples, size_t n,
                     void* out) {
    if (dtype < 0 || dtype > 5) return SDSP_E_INVALID_ARGUMENT;
    int dev = 0;
    SDSP_TRY(hipGetDevice(&dev), "device");
    int st = check_device(dev, nullptr);
    if (st) return st;
    const size_t sb = sample_bytes(dtype);
    DevBuf s, o;
    SDSP_TRY(s.ensure(std::max<size_t>(n, 1) * sb), "alloc");
    SDSP_TRY(o.ensure(sb), "alloc");
    if (n) SDSP_TRY(hipMemcpy(s.p, samples, n * sb, hipMemcpyHostToDevice), "H2D");
    st = sdsp_dot_execute_batched_device(dtype, coefs, len, direction, s.p, n, n, 1, o.p, nullptr);
    if (st) return st;
    SDSP_TRY(hipMemcpy(out, o.p, sb, hipMemcpyDeviceToHost), "D2H");
    return SDSP_OK;
}

}  // extern "C"

// C-ABI runtime of libsdsp.so: handles, HBM-resident delay lines, streams,
// kernel selection.  Every exported function cites the reference method it
// replaces in include/sdsp.h.
//
// There is deliberately no CPU execution path: if no gfx950 device is usable
// the create calls fail with SDSP_E_NO_DEVICE and nothing runs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ols_tables.hpp"
#include "sdsp.h"
#include "sdsp_host.hpp"
#include "sdsp_kernels.hpp"

namespace sdsp {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

// Process-wide starting algorithm of new FIR-type and IIR handles: SDSP_ALGO_EXACT unless
// sdsp_set_default_algo or the SDSP_DEFAULT_ALGO environment variable ("auto" / "exact" / "fma",
// or 0 / 1 / 2; read once, at the first handle or query) says otherwise -- so a deployment can move
// an unchanged reference-API caller onto the fast paths without a per-handle set_algo call.
static std::atomic<int> g_default_algo{-1};  // -1: not yet read from the environment
static int parse_algo_env(const char* e) {
    if (!e) return SDSP_ALGO_EXACT;
    std::string v(e);
    for (auto& ch : v) ch = (char)std::tolower((unsigned char)ch);
    if (v == "auto" || v == "0") return SDSP_ALGO_AUTO;
    if (v == "fma" || v == "2") return SDSP_ALGO_FMA;
    return SDSP_ALGO_EXACT;  // "exact", "1", anything else
}
int default_algo() {
    int v = g_default_algo.load();
    if (v >= 0) return v;
    int expect = -1;
    g_default_algo.compare_exchange_strong(expect, parse_algo_env(std::getenv("SDSP_DEFAULT_ALGO")));
    return g_default_algo.load();
}
int device_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return SDSP_OK;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? SDSP_E_OUT_OF_MEMORY : SDSP_E_DEVICE;
}

int check_device(int device, int* cus) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        set_error("no HIP device visible (libsdsp has no CPU execution path)");
        return SDSP_E_NO_DEVICE;
    }
    if (device < 0 || device >= count) {
        set_error("device index out of range");
        return SDSP_E_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
        set_error("hipGetDeviceProperties failed");
        return SDSP_E_NO_DEVICE;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(std::string("libsdsp is built for gfx950; device is ") + prop.gcnArchName);
        return SDSP_E_NO_DEVICE;
    }
    if (cus) *cus = prop.multiProcessorCount;
    return SDSP_OK;
}

// ---- FirCore (sdsp_host.hpp): the decimating FIR state of sdsp_fir and sdsp_ddc ----
hipError_t FirCore::init(int dt, const void* h, size_t len, const void* sc, size_t decimation, int dev) {
    dtype = dt;
    algo = default_algo();
    L = len;
    M = decimation;
    const size_t cb = coef_bytes(dt);
    taps.assign((const unsigned char*)h, (const unsigned char*)h + len * cb);
    scale.assign((const unsigned char*)sc, (const unsigned char*)sc + cb);
    std::vector<unsigned char> rev(len * cb);
    for (size_t i = 0; i < len; ++i) std::memcpy(&rev[i * cb], &taps[(len - 1 - i) * cb], cb);
    hipError_t e = open(dev);
    if (e == hipSuccess) e = d_taps_rev.ensure(rev.size());
    if (e == hipSuccess) e = hipMemcpy(d_taps_rev.p, rev.data(), rev.size(), hipMemcpyHostToDevice);
    return e;
}

int FirCore::zero_state() {
    SDSP_TRY(fence.wait(), "wait for queued work");
    SDSP_TRY(hist.reset(hist_bytes(), stream), "zero history");
    ci = 0;
    return quiesce();
}

int FirCore::read_hist(void* host) const {
    if (int st = quiesce()) return st;
    if (hist_bytes() && host) SDSP_TRY(hipMemcpy(host, hist.front(), hist_bytes(), hipMemcpyDeviceToHost), "get state");
    return SDSP_OK;
}

int FirCore::write_hist(const void* host) {
    if (int st = quiesce()) return st;
    if (hist_bytes() && host) SDSP_TRY(hipMemcpy(hist.front(), host, hist_bytes(), hipMemcpyHostToDevice), "set state");
    return SDSP_OK;
}

int FirCore::copy_state_to(FirCore* c) const {
    c->algo = algo;
    c->decim_seg = decim_seg;
    if (channels != 1) {
        c->channels = channels;
        if (int st = c->zero_state()) return st;
    }
    if (int st = quiesce()) return st;
    if (hist_bytes())
        SDSP_TRY(hipMemcpy(c->hist.front(), hist.front(), hist_bytes(), hipMemcpyDeviceToDevice), "clone state");
    c->ci = ci;
    return SDSP_OK;
}

}  // namespace sdsp

using namespace sdsp;

// ===========================================================================
// FIR / decimating FIR
// ===========================================================================
struct sdsp_fir;

// The overlap-save side of a FIR handle: which plan applies, the device tables (contents:
// ols_tables.cpp), the long path's scratch, the two launch plans, the knobs, and whether the
// tables match the handle's taps, scale and transform size.  Defined below sdsp_fir.
struct FirOls {
    bool ok = false;     // false: the next run builds the tables first
    OlsPlan plan{};      // 4096-point kernels; plan.kernel is SDSP_TUNE_OLS_KERNEL (build leaves it alone)
    OlsLongPlan lplan{};  // three-pass path of kern_fir_ols_long.hip (L - 1 > 3840, c32 samples)
    int long_log2n = 0;  // SDSP_TUNE_OLS_LONG_LOG2N (0 = automatic)
    int long_segs = 0;   // SDSP_TUNE_OLS_LONG_SEGS (0 = automatic)
    DevBuf H, tw1, tw2, pkt, ostab, hhalf;
    DevBuf lG, ltw, ltmp;  // spectrum [N1][N2], tables [N1 | N2], scratch [segments][N]

    static bool is_real(const sdsp_fir* h);   // real f32 samples and taps: kern_fir_ols_real.hip
    static bool is_short(const sdsp_fir* h);  // the 4096-point one-workgroup segment kernels
    static bool is_long(const sdsp_fir* h);   // longer taps on c32 samples: the three-pass transform
    static bool applicable(const sdsp_fir* h) { return is_short(h) || is_long(h); }
    int log2n(const sdsp_fir* h) const;       // of the long path's transform size
    void info(const sdsp_fir* h, size_t* nfft, size_t* valid) const;
    void invalidate() { ok = false; }
    int build(sdsp_fir* h);
    // one block on stream s (builds first when the tables are stale); *hist_done as launch_fir_ols
    int run(sdsp_fir* h, const void* d_in, const void* hist, void* d_out, size_t n, hipStream_t s, bool* hist_done);
    void copy_knobs_from(const FirOls& o) {  // a clone builds its own tables on its first run
        plan.kernel = o.plan.kernel;
        long_log2n = o.long_log2n;
        long_segs = o.long_segs;
    }
};

// (taps, delay line, phase and algorithm: FirCore, sdsp_host.hpp)
struct sdsp_fir : FirCore {
    int cus = 256;
    mutable unsigned long long device_ops = 0;  // sdsp_fir_device_ops
    HostMapped step_out;  // per-sample execute on the device: output at [0, 16), completion flag at [16, 20)
    unsigned step_seq = 0;
    // host delay line for per-sample calls and small host blocks (runtime_host_step below):
    // hbuf holds 2(L-1) samples, the window (oldest first) is hbuf[hpos, hpos + L-1)
    std::vector<unsigned char> hbuf;
    size_t hpos = 0;
    bool host_valid = false;  // hbuf holds the current window (single-channel handles only)
    bool dev_stale = false;   // the host consumed samples after hist.front() was last written
    int host_step = 1;        // SDSP_TUNE_HOST_STEP
    size_t host_macs = 1u << 16;  // host blocks: n * L up to this many multiply-adds
    FirOls ols;                   // overlap-save plan
};

bool FirOls::is_real(const sdsp_fir* h) { return h->dtype == SDSP_RR32; }
bool FirOls::is_short(const sdsp_fir* h) {
    return (h->dtype == SDSP_RR32 || h->dtype == SDSP_RC32 || h->dtype == SDSP_CC32) && h->M == 1 && h->L >= 2 &&
           h->L - 1 <= 256 * 15;
}
bool FirOls::is_long(const sdsp_fir* h) {
    return (h->dtype == SDSP_RC32 || h->dtype == SDSP_CC32) && h->M == 1 && h->L - 1 > 256 * 15 &&
           h->L - 1 <= kOlsLongMaxLm1;
}

// the tuned value, else the smallest power of two >= 4 (L-1) and >= 2^14 (at least three
// quarters of every transform is output)
int FirOls::log2n(const sdsp_fir* h) const {
    if (long_log2n) return long_log2n;
    int lg = 14;
    while (((size_t)1 << lg) < 4 * (h->L - 1)) ++lg;
    return lg;
}

void FirOls::info(const sdsp_fir* h, size_t* nfft, size_t* valid) const {
    *nfft = *valid = 0;
    if (is_short(h)) {
        *nfft = kOlsN;
        *valid = kOlsN - 256 * ((h->L - 1 + 255) / 256);
    } else if (is_long(h)) {
        *nfft = (size_t)1 << log2n(h);
        *valid = *nfft - (h->L - 1);
    }
}

// one table into its device buffer, queued on s: `v` must live until s is synchronised
static int upload(DevBuf& b, const std::vector<float>& v, hipStream_t s, const char* what) {
    SDSP_TRY(b.ensure(v.size() * 4), std::string("alloc ").append(what).c_str());
    SDSP_TRY(hipMemcpyAsync(b.p, v.data(), v.size() * 4, hipMemcpyHostToDevice, s),
             std::string("copy ").append(what).c_str());
    return SDSP_OK;
}

// tables of g[i] = scale * h[L-1-i] on the device (ols_tables.cpp), and the plan that points at them
int FirOls::build(sdsp_fir* h) {
    SDSP_TRY(h->fence.wait(), "wait for queued work");
    const unsigned char *taps = h->taps.data(), *scale = h->scale.data();
    hipStream_t s = h->stream;
    int st = SDSP_OK;
    if (is_long(h)) {
        const int lg = log2n(h);
        const std::vector<float> G = ols_long_spectrum(taps, scale, h->dtype, h->L, lg), tw = ols_long_twiddles(lg);
        if ((st = upload(lG, G, s, "long spectrum")) || (st = upload(ltw, tw, s, "long tables"))) return st;
        SDSP_TRY(hipStreamSynchronize(s), "sync");
        const size_t N1 = (size_t)1 << (lg / 2);
        lplan = OlsLongPlan{lG.p, ltw.p, (const float*)ltw.p + 2 * N1, lg, (int)(h->L - 1)};
        ok = true;
        return SDSP_OK;
    }
    const std::vector<cd> G = ols_spectrum(taps, scale, h->dtype, h->L);
    const std::vector<float> Hs = ols_rows_H(G), t1 = ols_rows_tw(256, 4096), t2 = ols_rows_tw(16, 256);
    const std::vector<float> pk = ols_pack_pkt(Hs, t1, t2), os = ols_os_bases();
    // real f32 samples: the packed-pair kernel reads pkt and ostab only (H, tw1, tw2 stay null)
    const bool real = is_real(h), real_taps = ols_real_taps(h->dtype, scale);
    const std::vector<float> hh = real_taps ? ols_half_table(G) : std::vector<float>();
    if (!real && ((st = upload(H, Hs, s, "H")) || (st = upload(tw1, t1, s, "tw1")) || (st = upload(tw2, t2, s, "tw2"))))
        return st;
    if ((st = upload(pkt, pk, s, "packed tables")) || (st = upload(ostab, os, s, "one-shot tables"))) return st;
    if (real_taps && (st = upload(hhalf, hh, s, "half spectrum"))) return st;
    SDSP_TRY(hipStreamSynchronize(s), "sync");
    plan.d_H = H.p;
    plan.d_tw1 = tw1.p;
    plan.d_tw2 = tw2.p;
    plan.d_pkt = pkt.p;
    plan.d_ostab = ostab.p;
    plan.d_hhalf = real_taps ? hhalf.p : nullptr;
    plan.sample_bytes = real ? 4 : 8;
    plan.halo_rows = (int)((h->L - 1 + 255) / 256);
    ok = true;
    return SDSP_OK;
}

int FirOls::run(sdsp_fir* h, const void* d_in, const void* hist, void* d_out, size_t n, hipStream_t s,
                bool* hist_done) {
    if (!ok)
        if (int st = build(h)) return st;
    if (!is_long(h)) {
        SDSP_TRY(launch_fir_ols(plan, d_in, hist, h->hist.back(), d_out, n, (int)h->L, h->channels, h->cus, s,
                                hist_done),
                 "fir ols");
        return SDSP_OK;
    }
    const int lg = lplan.log2n;
    const size_t total = h->channels * ols_long_segments(n, lg, (int)h->L - 1);
    // segments per round: the tuned value, else what 256 MiB of scratch hold
    const size_t fit = std::max<size_t>(1, ((size_t)256 << 20) / ((size_t)8 << lg));
    const size_t round = std::min(total, long_segs ? (size_t)long_segs : fit);
    SDSP_TRY(ltmp.ensure(round * ((size_t)8 << lg)), "alloc long scratch");
    SDSP_TRY(launch_fir_ols_long(lplan, d_in, hist, d_out, ltmp.p, n, h->channels, round, s), "fir ols long");
    return SDSP_OK;
}

namespace {

int fir_alloc_state(sdsp_fir* h) {
    if (int st = h->zero_state()) return st;
    const size_t lm1 = h->L - 1, sb = sample_bytes(h->dtype);
    h->hbuf.assign(2 * lm1 * sb, 0);  // the zeroed window, both copies
    h->hpos = 0;
    h->host_valid = h->channels == 1;
    h->dev_stale = false;
    return SDSP_OK;
}

// AUTO moves a long-filter c32 block to the three-pass path from this many samples
// (profiles/r10/LAB.md: the A/B against the reference-order kernel at L = 3842)
constexpr size_t kOlsLongAutoMin = (size_t)1 << 16;

int fir_resolve_algo(const sdsp_fir* h, size_t n) {
    if (h->algo == SDSP_ALGO_FFT) return FirOls::applicable(h) ? SDSP_ALGO_FFT : SDSP_ALGO_EXACT;
    if (h->algo != SDSP_ALGO_AUTO) return h->algo;
    // AUTO: overlap-save for long 32-bit complex blocks, reference-order direct form otherwise
    // (real f32 streams take overlap-save only when asked: AUTO keeps their bits)
    if (FirOls::is_short(h) && !FirOls::is_real(h) && n >= (size_t)(1 << 16)) return SDSP_ALGO_FFT;
    if (FirOls::is_long(h) && n >= kOlsLongAutoMin) return SDSP_ALGO_FFT;
    return SDSP_ALGO_EXACT;
}

int fir_create_common(sdsp_fir** out, int dtype, const void* taps, size_t len, const void* scale, size_t M,
                      int device) {
    *out = nullptr;
    if (dtype < 0 || dtype > 5) {
        set_error("bad dtype");
        return SDSP_E_INVALID_ARGUMENT;
    }
    if (len == 0) {
        set_error("FIR Filter Error CoefficientsLengthZero");
        return SDSP_E_COEFFICIENTS_LENGTH_ZERO;
    }
    if (M < 1) {
        set_error("FIR Filter Error DecimationLessThanOne");
        return SDSP_E_DECIMATION_LESS_THAN_ONE;
    }
    if (len > (1u << 30)) {
        set_error("tap count too large");
        return SDSP_E_INVALID_ARGUMENT;
    }
    int cus = 256;
    int st = check_device(device, &cus);
    if (st) return st;
    DeviceGuard g(device);
    sdsp_fir* h = new sdsp_fir();
    h->cus = cus;
    st = device_status(h->init(dtype, taps, len, scale, M, device), "fir create");
    if (!st) st = fir_alloc_state(h);
    if (st) {
        sdsp_fir_destroy(h);
        return st;
    }
    *out = h;
    return SDSP_OK;
}

// ---------------------------------------------------------------------------
// Host step: Filter::execute(sample), DecimatingFIRFilter::push and small host
// blocks run on the host against the handle's own delay line, in
// the reference's arithmetic (fir/mod.rs:209-212, decim.rs:115-118, 221-228:
// acc = 0; acc += cr[i] x[n-i] for i = 0..L-1; y = acc * scale; num-complex
// products, no contraction -- this TU is built with -ffp-contract=off).  It is
// the product's own small-work path, not a fallback: creating a handle still
// requires the gfx950 device, and every block above the threshold runs on it.
// Coherence: the state is the last L-1 inputs, so it moves between host and
// device only when the side that runs next does not hold it -- one D2H of L-1
// samples before the first host step after device work (host_pull), one H2D
// before the first device call after host steps (host_flush).
template <typename T> struct hcx {
    T re, im;
};
template <typename T> inline T hmul(T a, T b) { return a * b; }
template <typename T> inline hcx<T> hmul(T a, hcx<T> b) { return {a * b.re, a * b.im}; }
template <typename T> inline hcx<T> hmul(hcx<T> a, T b) { return {a.re * b, a.im * b}; }
template <typename T> inline hcx<T> hmul(hcx<T> a, hcx<T> b) {
    return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
template <typename T> inline T hadd(T a, T b) { return a + b; }
template <typename T> inline hcx<T> hadd(hcx<T> a, hcx<T> b) { return {a.re + b.re, a.im + b.im}; }
// fused forms: fmac_ of sdsp_device.hpp (the device FMA kernels), one rounding per fma
inline float hfma(float acc, float c, float x) { return std::fma(c, x, acc); }
inline double hfma(double acc, double c, double x) { return std::fma(c, x, acc); }
template <typename T> inline hcx<T> hfma(hcx<T> acc, T c, hcx<T> x) { return {hfma(acc.re, c, x.re), hfma(acc.im, c, x.im)}; }
template <typename T> inline hcx<T> hfma(hcx<T> acc, hcx<T> c, hcx<T> x) {
    return {hfma(hfma(acc.re, c.re, x.re), -c.im, x.im), hfma(hfma(acc.im, c.re, x.im), c.im, x.re)};
}
template <typename T> inline T hzero() { return T{}; }

template <typename C, typename I>
void host_step_t(sdsp_fir* h, const unsigned char* sample, unsigned char* out, bool emit, bool fused) {
    const size_t L = h->L, lm1 = L - 1;
    I x;
    std::memcpy(&x, sample, sizeof(I));
    I* b = reinterpret_cast<I*>(h->hbuf.data());
    if (emit) {
        const I* w = b + h->hpos;  // window oldest first: x[n - i] = w[lm1 - i]
        const C* taps = reinterpret_cast<const C*>(h->taps.data());  // cr[i] = h[L-1-i]
        I acc = hzero<I>();
        if (fused) {
            acc = hfma(acc, taps[L - 1], x);
            for (size_t i = 1; i < L; ++i) acc = hfma(acc, taps[L - 1 - i], w[lm1 - i]);
        } else {
            acc = hadd(acc, hmul(taps[L - 1], x));
            for (size_t i = 1; i < L; ++i) acc = hadd(acc, hmul(taps[L - 1 - i], w[lm1 - i]));
        }
        C sc;
        std::memcpy(&sc, h->scale.data(), sizeof(C));
        const I y = hmul(acc, sc);
        std::memcpy(out, &y, sizeof(I));
    }
    if (lm1) {  // Window::push (src/window/mod.rs:36-41) on the doubled buffer
        b[h->hpos] = x;
        b[h->hpos + lm1] = x;
        h->hpos = h->hpos + 1 == lm1 ? 0 : h->hpos + 1;
    }
}

void host_step(sdsp_fir* h, const unsigned char* sample, unsigned char* out, bool emit) {
    const bool fused = h->algo == SDSP_ALGO_FMA;
    switch (h->dtype) {
        case SDSP_RR32: return host_step_t<float, float>(h, sample, out, emit, fused);
        case SDSP_RC32: return host_step_t<float, hcx<float>>(h, sample, out, emit, fused);
        case SDSP_CC32: return host_step_t<hcx<float>, hcx<float>>(h, sample, out, emit, fused);
        case SDSP_RR64: return host_step_t<double, double>(h, sample, out, emit, fused);
        case SDSP_RC64: return host_step_t<double, hcx<double>>(h, sample, out, emit, fused);
        case SDSP_CC64: return host_step_t<hcx<double>, hcx<double>>(h, sample, out, emit, fused);
    }
}

// the host window := the device history (after device work)
int host_pull(sdsp_fir* h) {
    if (h->host_valid) return SDSP_OK;
    SDSP_TRY(h->fence.wait(), "wait for queued work");
    SDSP_TRY(hipStreamSynchronize(h->stream), "sync");
    const size_t lm1 = h->L - 1, sb = sample_bytes(h->dtype);
    h->hbuf.resize(2 * lm1 * sb);
    ++h->device_ops;
    if (lm1) {
        SDSP_TRY(hipMemcpy(h->hbuf.data(), h->hist.front(), lm1 * sb, hipMemcpyDeviceToHost), "pull history");
        std::memcpy(h->hbuf.data() + lm1 * sb, h->hbuf.data(), lm1 * sb);
    }
    h->hpos = 0;
    h->host_valid = true;
    return SDSP_OK;
}

// the device history := the host window (before device work after host steps).  No
// kernel can be reading hist here: host steps start only after host_pull's
// synchronisation, a synchronising host call, or a state reset.
int host_flush(const sdsp_fir* hc) {
    sdsp_fir* h = const_cast<sdsp_fir*>(hc);
    if (!h->dev_stale) return SDSP_OK;
    ++h->device_ops;
    const size_t lm1 = h->L - 1, sb = sample_bytes(h->dtype);
    if (lm1)
        SDSP_TRY(hipMemcpy(h->hist.front(), h->hbuf.data() + h->hpos * sb, lm1 * sb, hipMemcpyHostToDevice),
                 "flush history");
    h->dev_stale = false;
    return SDSP_OK;
}

// keep a valid host window current across a device block whose input the host holds
void host_feed(sdsp_fir* h, const unsigned char* in, size_t n) {
    const size_t lm1 = h->L - 1, sb = sample_bytes(h->dtype);
    if (!h->host_valid || !lm1 || !n) return;
    if (n >= lm1) {
        std::memcpy(h->hbuf.data(), in + (n - lm1) * sb, lm1 * sb);
        std::memcpy(h->hbuf.data() + lm1 * sb, in + (n - lm1) * sb, lm1 * sb);
        h->hpos = 0;
        return;
    }
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(h->hbuf.data() + h->hpos * sb, in + i * sb, sb);
        std::memcpy(h->hbuf.data() + (h->hpos + lm1) * sb, in + i * sb, sb);
        h->hpos = h->hpos + 1 == lm1 ? 0 : h->hpos + 1;
    }
}

bool host_eligible(const sdsp_fir* h, size_t n) {
    return h->host_step && h->channels == 1 && h->algo != SDSP_ALGO_FFT && n * h->L <= h->host_macs;
}

// n inputs through the host step; outputs (when `out`) where the phase emits (decim.rs:221-228)
int host_run(sdsp_fir* h, const unsigned char* in, size_t n, unsigned char* out, size_t* n_out) {
    int st = host_pull(h);
    if (st) return st;
    const size_t sb = sample_bytes(h->dtype);
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool emit = out && (h->M == 1 || (h->M - 1 - h->ci) % h->M == 0);
        host_step(h, in + i * sb, emit ? out + k * sb : nullptr, emit);
        h->ci = (h->ci + 1) % h->M;
        k += emit;
    }
    if (n) h->dev_stale = true;
    if (n_out) *n_out = k;
    return SDSP_OK;
}

// one input through the single-launch device step kernel (kern_fir_step.hip,
// SDSP_TUNE_HOST_STEP = 0): the delay line shifts on the device, the output (when
// the phase emits and `want` is set) lands in host-mapped memory
int fir_step_device(sdsp_fir* h, const void* sample, void* out, size_t* n_out, bool want) {
    SDSP_TRY(h->fence.wait(), "wait for queued work");
    ++h->device_ops;
    int st = host_flush(h);
    if (st) return st;
    if (!h->step_out.host) {
        SDSP_TRY(h->step_out.ensure(32), "alloc mapped output");
        std::memset(h->step_out.host, 0, 32);  // pinned memory is not zeroed: no stale flag value
    }
    const bool emit = want && (h->M == 1 || (h->M - 1 - h->ci) % h->M == 0);  // decim.rs:221-231
    unsigned* flag_h = reinterpret_cast<unsigned*>((char*)h->step_out.host + 16);
    unsigned seq = ++h->step_seq;
    if (seq == 0) seq = h->step_seq = 1;  // the flag's initial 0 never matches
    FirStepArgs a{sample, h->hist.front(), h->hist.back(), h->d_taps_rev.p, h->scale.data(),
                  h->step_out.dev, reinterpret_cast<unsigned*>((char*)h->step_out.dev + 16), seq, (int)h->L - 1,
                  (int)h->L, emit, h->algo != SDSP_ALGO_FMA};
    SDSP_TRY(launch_fir_step(h->dtype, a, h->stream), "fir step");
    h->hist.flip();
    h->ci = (h->ci + 1) % h->M;
    h->host_valid = false;
    // the flag is released after the whole workgroup's delay-line stores; the fence orders any
    // later launch on a caller stream after the kernel itself
    SDSP_TRY(h->fence.record(h->stream), "record fence");
    SDSP_TRY(wait_host_flag(flag_h, seq, h->stream), "fir step wait");
    if (emit && out) std::memcpy(out, h->step_out.host, sample_bytes(h->dtype));
    if (n_out) *n_out = emit ? 1 : 0;
    return SDSP_OK;
}

int fir_step(sdsp_fir* h, const void* sample, void* out, size_t* n_out, bool want) {
    if (!h || !sample || h->channels != 1) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    if (!h->host_step) return fir_step_device(h, sample, out, n_out, want);
    size_t k = 0;
    int st = host_run(h, (const unsigned char*)sample, 1, want ? (unsigned char*)out : nullptr, &k);
    if (n_out) *n_out = k;
    return st;
}
}  // namespace

extern "C" {

const char* sdsp_last_error(void) { return g_last_error.c_str(); }
const char* sdsp_version(void) { return "sdsp 0.1.0 (gfx950)"; }
size_t sdsp_sample_size(int dtype) { return sample_bytes(dtype); }
size_t sdsp_coef_size(int dtype) { return coef_bytes(dtype); }

int sdsp_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    int n = 0;
    for (int d = 0; d < count; ++d) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, d) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++n;
    }
    return n;
}

int sdsp_fir_create(sdsp_fir** out, int dtype, const void* taps, size_t len, const void* scale, int device) {
    return fir_create_common(out, dtype, taps, len, scale, 1, device);
}

int sdsp_decim_create(sdsp_fir** out, int dtype, const void* taps, size_t len, const void* scale,
                      size_t decimation, int device) {
    return fir_create_common(out, dtype, taps, len, scale, decimation, device);
}

void sdsp_fir_destroy(sdsp_fir* h) { destroy_handle(h); }

int sdsp_fir_set_channels(sdsp_fir* h, size_t channels) {
    if (!h || channels == 0) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    h->channels = channels;
    return fir_alloc_state(h);
}

int sdsp_fir_set_algo(sdsp_fir* h, int algo) {
    if (!h || algo < 0 || algo > 3) return SDSP_E_INVALID_ARGUMENT;
    if (algo == SDSP_ALGO_FFT && !FirOls::applicable(h)) {
        set_error("overlap-save needs no decimation and 32-bit samples: complex with L-1 <= 2^20, or real with real "
                  "taps and L-1 <= 3840");
        return SDSP_E_UNSUPPORTED;
    }
    h->algo = algo;
    return SDSP_OK;
}

int sdsp_fir_get_algo(const sdsp_fir* h) { return h ? h->algo : -1; }

int sdsp_set_default_algo(int algo) {
    if (algo != SDSP_ALGO_AUTO && algo != SDSP_ALGO_EXACT && algo != SDSP_ALGO_FMA) {
        set_error("default algorithm: SDSP_ALGO_AUTO, SDSP_ALGO_EXACT or SDSP_ALGO_FMA");
        return SDSP_E_INVALID_ARGUMENT;
    }
    sdsp::g_default_algo.store(algo);
    return SDSP_OK;
}

int sdsp_get_default_algo(void) { return sdsp::default_algo(); }

int sdsp_fir_set_tuning(sdsp_fir* h, int key, int value) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    switch (key) {
        case SDSP_TUNE_OLS_KERNEL:  // every value computes the full output (performance only)
            if (value < kOlsOneShot || value > kOlsOneShotWide) return SDSP_E_INVALID_ARGUMENT;
            h->ols.plan.kernel = value;
            return SDSP_OK;
        case SDSP_TUNE_OLS_LONG_LOG2N:  // 0, or log2 N with 2^13 <= N <= 2^22 and N >= 2 (L-1) (long scope only)
            if (value != 0 && !(FirOls::is_long(h) && value >= kOlsLongMinLog2N && value <= kOlsLongMaxLog2N &&
                                ((size_t)1 << value) >= 2 * (h->L - 1))) {
                set_error("long overlap-save transform size: 0, or log2 N in [13, 22] with N >= 2 (L-1) on a handle "
                          "with 3840 < L-1 <= 2^20 and 32-bit complex samples");
                return SDSP_E_INVALID_ARGUMENT;
            }
            if (value != h->ols.long_log2n) {  // the plan is rebuilt on the next run
                DeviceGuard g(h->device);
                SDSP_TRY(h->fence.wait(), "wait for queued work");
                h->ols.long_log2n = value;
                if (FirOls::is_long(h)) h->ols.invalidate();
            }
            return SDSP_OK;
        case SDSP_TUNE_OLS_LONG_SEGS:
            if (value < 0 || value > 4096) return SDSP_E_INVALID_ARGUMENT;
            h->ols.long_segs = value;
            return SDSP_OK;
        case SDSP_TUNE_DECIM_SEG:
            if (value < 0) return SDSP_E_INVALID_ARGUMENT;
            h->decim_seg = value;
            return SDSP_OK;
        case SDSP_TUNE_HOST_STEP:
            if (value < 0 || value > 1) return SDSP_E_INVALID_ARGUMENT;
            if (!value) {  // the device kernels take over: they need the newest window
                DeviceGuard g(h->device);
                int st = host_flush(h);
                if (st) return st;
            }
            h->host_step = value;
            return SDSP_OK;
        case SDSP_TUNE_HOST_BLOCK_MACS:
            if (value < 0) return SDSP_E_INVALID_ARGUMENT;
            h->host_macs = (size_t)value;
            return SDSP_OK;
        default:
            set_error("unknown or retired tuning key");
            return SDSP_E_INVALID_ARGUMENT;
    }
}

int sdsp_fir_clone(const sdsp_fir* h, sdsp_fir** out) {
    if (!h || !out) return SDSP_E_INVALID_ARGUMENT;
    int st = fir_create_common(out, h->dtype, h->taps.data(), h->L, h->scale.data(), h->M, h->device);
    if (st) return st;
    sdsp_fir* c = *out;
    DeviceGuard g(h->device);
    c->ols.copy_knobs_from(h->ols);
    c->host_step = h->host_step;
    c->host_macs = h->host_macs;
    // the device history has to be the newest state before it is copied; the clone reads its own
    // host window back when it needs one
    st = h->quiesce();
    if (!st) st = host_flush(h);
    if (!st) st = h->copy_state_to(c);
    c->host_valid = false;
    if (st) {  // a failure leaves the caller no handle to destroy
        sdsp_fir_destroy(c);
        *out = nullptr;
    }
    return st;
}

int sdsp_fir_set_scale(sdsp_fir* h, const void* scale) {
    if (!h || !scale) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    SDSP_TRY(h->fence.wait(), "wait for queued work");  // the next run rebuilds tables a queued kernel may read
    std::memcpy(h->scale.data(), scale, h->scale.size());
    h->ols.invalidate();
    return SDSP_OK;
}
int sdsp_fir_get_scale(const sdsp_fir* h, void* scale) {
    if (!h || !scale) return SDSP_E_INVALID_ARGUMENT;
    std::memcpy(scale, h->scale.data(), h->scale.size());
    return SDSP_OK;
}
int sdsp_fir_ols_info(const sdsp_fir* h, size_t* nfft, size_t* valid) {
    if (!h || !nfft || !valid) return SDSP_E_INVALID_ARGUMENT;
    h->ols.info(h, nfft, valid);
    return SDSP_OK;
}
size_t sdsp_fir_len(const sdsp_fir* h) { return h ? h->L : 0; }
size_t sdsp_fir_decimation(const sdsp_fir* h) { return h ? h->M : 0; }

int sdsp_fir_coefficients(const sdsp_fir* h, void* out) {
    if (!h || !out) return SDSP_E_INVALID_ARGUMENT;
    const size_t cb = coef_bytes(h->dtype);
    unsigned char* o = (unsigned char*)out;
    for (size_t i = 0; i < h->L; ++i) std::memcpy(o + i * cb, &h->taps[(h->L - 1 - i) * cb], cb);
    return SDSP_OK;
}

size_t sdsp_fir_output_count(const sdsp_fir* h, size_t n) { return h ? h->output_count(n) : 0; }

int sdsp_fir_execute_block_device(sdsp_fir* h, const void* d_in, size_t n, void* d_out, size_t* n_out,
                                  void* stream) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    hipStream_t s = pick(stream, h->stream);
    const size_t nout = sdsp_fir_output_count(h, n);
    if (n_out) *n_out = nout;
    if (n == 0) return SDSP_OK;
    const size_t sb = sample_bytes(h->dtype);
    if (ranges_overlap(d_in, h->channels * n * sb, d_out, h->channels * nout * sb)) {
        set_error("input and output blocks overlap (in-place filtering is not supported)");
        return SDSP_E_INVALID_ARGUMENT;
    }
    int hst = host_flush(h);
    if (hst) return hst;
    ++h->device_ops;
    h->host_valid = false;  // the input is device-resident: the host window is re-read when needed
    // work queued on another stream (the fence) reads or writes the history this launch uses
    SDSP_TRY(h->fence.order_before(s), "order after queued work");
    const void* hist = h->hist.front();
    bool hist_done = false;  // the overlap-save launch wrote the next history itself
    if (h->M == 1) {
        const int algo = fir_resolve_algo(h, n);
        if (algo == SDSP_ALGO_FFT) {
            if (int st = h->ols.run(h, d_in, hist, d_out, n, s, &hist_done)) return st;
        } else {
            FirArgs a{d_in, hist, h->d_taps_rev.p, h->scale.data(), d_out, n, n, h->channels, (int)h->L, 1, 0,
                      algo != SDSP_ALGO_FMA};
            SDSP_TRY(launch_fir_direct(h->dtype, a, s), "fir direct");
        }
    } else {
        FirArgs a{d_in, hist, h->d_taps_rev.p, h->scale.data(), d_out, n, nout, h->channels, (int)h->L, (int)h->M,
                  h->j0(), h->decim_algo(n) != SDSP_ALGO_FMA};
        a.seg = h->decim_seg;
        SDSP_TRY(launch_decim_direct(h->dtype, a, s), "decim direct");
        h->ci = (h->ci + n) % h->M;
    }
    if (!hist_done)
        SDSP_TRY(launch_hist_update(h->dtype, d_in, hist, h->hist.back(), n, (int)h->L - 1, h->channels, s),
                 "history update");
    h->hist.flip();
    SDSP_TRY(h->fence.record(s), "record fence");
    return SDSP_OK;
}

int sdsp_fir_execute_block(sdsp_fir* h, const void* in, size_t n, void* out, size_t* n_out) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    SDSP_TRY(h->fence.wait(), "wait for queued work");
    const size_t sb = sample_bytes(h->dtype);
    const size_t nout = sdsp_fir_output_count(h, n);
    if (n_out) *n_out = nout;
    if (n == 0) return SDSP_OK;
    if (host_eligible(h, n)) return host_run(h, (const unsigned char*)in, n, (unsigned char*)out, nullptr);
    const bool keep = h->host_valid;
    int st = h->staged(in, h->channels * n * sb, out, h->channels * nout * sb,
                       [&](const void* d_in, void* d_out, hipStream_t s) {
                           return sdsp_fir_execute_block_device(h, d_in, n, d_out, nullptr, s);
                       });
    if (st) return st;
    h->host_valid = keep;  // the host holds the input: move its window on without a read-back
    host_feed(h, (const unsigned char*)in, n);
    return SDSP_OK;
}

int sdsp_fir_execute(sdsp_fir* h, const void* sample, void* out, size_t* n_out) {
    if (!out) return SDSP_E_INVALID_ARGUMENT;
    return fir_step(h, sample, out, n_out, true);
}

int sdsp_decim_write(sdsp_fir* h, const void* samples, size_t n) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (n == 0) return SDSP_OK;
    DeviceGuard g(h->device);
    SDSP_TRY(h->fence.wait(), "wait for queued work");
    if (host_eligible(h, n)) return host_run(h, (const unsigned char*)samples, n, nullptr, nullptr);
    int hst = host_flush(h);
    if (hst) return hst;
    const size_t sb = sample_bytes(h->dtype);
    ++h->device_ops;
    SDSP_TRY(h->stage_in.ensure(h->channels * n * sb), "stage in");
    SDSP_TRY(hipMemcpyAsync(h->stage_in.p, samples, h->channels * n * sb, hipMemcpyHostToDevice, h->stream), "H2D");
    SDSP_TRY(launch_hist_update(h->dtype, h->stage_in.p, h->hist.front(), h->hist.back(), n,
                                (int)h->L - 1, h->channels, h->stream),
             "history update");
    h->hist.flip();
    h->ci = (h->ci + n) % h->M;
    SDSP_TRY(hipStreamSynchronize(h->stream), "sync");
    host_feed(h, (const unsigned char*)samples, n);
    return SDSP_OK;
}

int sdsp_decim_push(sdsp_fir* h, const void* sample) {
    if (h && h->channels != 1) return sdsp_decim_write(h, sample, 1);  // one sample per channel
    return fir_step(h, sample, nullptr, nullptr, false);
}

int sdsp_fir_reset(sdsp_fir* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    return fir_alloc_state(h);
}

size_t sdsp_fir_state_len(const sdsp_fir* h) { return h ? h->state_len() : 0; }

int sdsp_fir_get_state(const sdsp_fir* h, void* hist, size_t* phase) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    if (h->dev_stale) {  // the host window is the newer one
        if (int st = h->quiesce()) return st;
        if (h->hist_bytes() && hist)
            std::memcpy(hist, h->hbuf.data() + h->hpos * sample_bytes(h->dtype), h->hist_bytes());
    } else if (int st = h->read_hist(hist)) {
        return st;
    }
    if (phase) *phase = h->ci;
    return SDSP_OK;
}

int sdsp_fir_set_state(sdsp_fir* h, const void* hist, size_t phase) {
    if (!h || phase >= h->M) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    if (int st = h->write_hist(hist)) return st;
    h->ci = phase;
    h->dev_stale = false;
    h->host_valid = false;  // re-read on the next host step
    return SDSP_OK;
}

int sdsp_fir_frequency_response(const sdsp_fir* h, double f, double* re_im) {
    if (!h || !re_im) return SDSP_E_INVALID_ARGUMENT;
    // coefficients() returns the REVERSED stored taps (fir/mod.rs:173-176, used at :263-273)
    std::vector<cd> c(h->L);
    for (size_t i = 0; i < h->L; ++i) c[i] = coef_at(h->taps.data(), h->dtype, h->L - 1 - i);
    const bool real = !coef_is_complex(h->dtype);
    cd o = poly_response(c, real, f);
    cd s = coef_at(h->scale.data(), h->dtype, 0);
    cd r = real ? cmul(s.re, o) : cmul(s, o);
    re_im[0] = r.re;
    re_im[1] = r.im;
    return SDSP_OK;
}

int sdsp_fir_group_delay(const sdsp_fir* h, double f, double* delay) {
    if (!h || !delay) return SDSP_E_INVALID_ARGUMENT;
    std::vector<cd> c(h->L);
    for (size_t i = 0; i < h->L; ++i) c[i] = coef_at(h->taps.data(), h->dtype, h->L - 1 - i);
    double d = 0.0;
    if (fir_group_delay(c, !coef_is_complex(h->dtype), f, &d)) d = 0.0;  // errors map to 0.0 (:293-303)
    *delay = d;
    return SDSP_OK;
}

unsigned long long sdsp_fir_device_ops(const sdsp_fir* h) { return h ? h->device_ops : 0; }

int sdsp_fir_synchronize(sdsp_fir* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    return h->quiesce();
}

}  // extern "C"

// ===========================================================================
// Polyphase filterbank / interpolating FIR
// ===========================================================================
// (struct sdsp_pfb: sdsp_host.hpp, shared with the up-converter's runtime_duc.cpp)
namespace {

int pfb_alloc_state(sdsp_pfb* h) {
    SDSP_TRY(h->fence.wait(), "wait for queued work");
    SDSP_TRY(h->hist.reset(h->channels * h->K * sample_bytes(h->dtype), h->stream), "zero window");
    return h->quiesce();
}

int pfb_create_common(sdsp_pfb** out, int dtype, const unsigned char* taps, size_t len, size_t M,
                      const unsigned char* scale, bool interp, int device) {
    *out = nullptr;
    const size_t cbytes = coef_bytes(dtype);
    const size_t K = len / M;
    if (K == 0) {  // the reference panics in Window::new(0) (src/window/mod.rs:18)
        set_error("fewer taps than filters: sub-filter length 0");
        return SDSP_E_INVALID_ARGUMENT;
    }
    int st = check_device(device, nullptr);
    if (st) return st;
    DeviceGuard g(device);
    sdsp_pfb* h = new sdsp_pfb();
    h->dtype = dtype;
    h->algo = default_algo() == SDSP_ALGO_FMA ? SDSP_ALGO_FMA : SDSP_ALGO_EXACT;  // (EXACT / FMA only)
    h->M = M;
    h->K = K;
    h->interp = interp;
    h->scale.assign(scale, scale + cbytes);
    h->cb.resize(M * K * cbytes);
    // rev_sub_coefs[K - index - 1] = coefficients[filter + index * filters]  (pfb.rs:33-40)
    for (size_t p = 0; p < M; ++p)
        for (size_t idx = 0; idx < K; ++idx)
            std::memcpy(&h->cb[(p * K + (K - idx - 1)) * cbytes], taps + (p + idx * M) * cbytes, cbytes);
    hipError_t e = h->open(device);
    if (e == hipSuccess) e = h->d_cb.ensure(h->cb.size());
    if (e == hipSuccess) e = hipMemcpy(h->d_cb.p, h->cb.data(), h->cb.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        st = device_status(e, "pfb create");
        sdsp_pfb_destroy(h);
        return st;
    }
    st = pfb_alloc_state(h);
    if (st) {
        sdsp_pfb_destroy(h);
        return st;
    }
    *out = h;
    return SDSP_OK;
}

}  // namespace

extern "C" {

int sdsp_pfb_create(sdsp_pfb** out, int dtype, const void* taps, size_t len, size_t filters, const void* scale,
                    int device) {
    if (!out) return SDSP_E_INVALID_ARGUMENT;
    *out = nullptr;
    if (dtype < 0 || dtype > 5) return SDSP_E_INVALID_ARGUMENT;
    if (filters == 0) {  // pfb.rs:25-26
        set_error("FIR Filter Error NotEnoughFilters");
        return SDSP_E_NOT_ENOUGH_FILTERS;
    }
    if (len == 0) {  // pfb.rs:27-28
        set_error("FIR Filter Error CoefficientsLengthZero");
        return SDSP_E_COEFFICIENTS_LENGTH_ZERO;
    }
    return pfb_create_common(out, dtype, (const unsigned char*)taps, len, filters, (const unsigned char*)scale,
                             false, device);
}

int sdsp_interp_create(sdsp_pfb** out, int dtype, const void* taps, size_t len, size_t M, int device) {
    if (!out) return SDSP_E_INVALID_ARGUMENT;
    *out = nullptr;
    if (dtype < 0 || dtype > 5) return SDSP_E_INVALID_ARGUMENT;
    if (len == 0) {  // interp.rs:28-29
        set_error("FIR Filter Error CoefficientsLengthZero");
        return SDSP_E_COEFFICIENTS_LENGTH_ZERO;
    }
    if (M < 1) {  // interp.rs:30-31
        set_error("FIR Filter Error InterpolationLessThanOne");
        return SDSP_E_INTERPOLATION_LESS_THAN_ONE;
    }
    // sub-filter length computed in f32 (interp.rs:35-40), taps zero-padded to K*M (:43-46)
    const float q = (float)len / (float)M;
    const size_t K = (q == std::floor(q)) ? (size_t)q : (size_t)std::ceil(q);
    const size_t cbytes = coef_bytes(dtype);
    std::vector<unsigned char> eff(K * M * cbytes, 0);
    std::memcpy(eff.data(), taps, std::min(len, K * M) * cbytes);
    std::vector<unsigned char> one(cbytes, 0);
    if (coef_is_f32(dtype)) { float v = 1.0f; std::memcpy(one.data(), &v, 4); }
    else { double v = 1.0; std::memcpy(one.data(), &v, 8); }
    return pfb_create_common(out, dtype, eff.data(), K * M, M, one.data(), true, device);
}

void sdsp_pfb_destroy(sdsp_pfb* h) { destroy_handle(h); }

int sdsp_pfb_clone(const sdsp_pfb* h, sdsp_pfb** out) {
    if (!h || !out) return SDSP_E_INVALID_ARGUMENT;
    int st = check_device(h->device, nullptr);
    if (st) return st;
    DeviceGuard g(h->device);
    sdsp_pfb* c = new sdsp_pfb();
    c->dtype = h->dtype; c->M = h->M; c->K = h->K; c->channels = h->channels;
    c->interp = h->interp; c->cb = h->cb; c->scale = h->scale; c->algo = h->algo;
    hipError_t e = c->open(h->device);
    if (e == hipSuccess) e = c->d_cb.ensure(c->cb.size());
    if (e == hipSuccess) e = hipMemcpy(c->d_cb.p, c->cb.data(), c->cb.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { st = device_status(e, "pfb clone"); sdsp_pfb_destroy(c); return st; }
    st = pfb_alloc_state(c);
    if (st) { sdsp_pfb_destroy(c); return st; }
    const size_t hb = h->channels * h->K * sample_bytes(h->dtype);
    st = h->quiesce();
    if (!st) st = device_status(hipMemcpy(c->hist.front(), h->hist.front(), hb, hipMemcpyDeviceToDevice), "pfb clone state");
    if (st) { sdsp_pfb_destroy(c); return st; }
    *out = c;
    return SDSP_OK;
}

size_t sdsp_pfb_len(const sdsp_pfb* h) { return h ? h->M : 0; }
size_t sdsp_pfb_subfilter_len(const sdsp_pfb* h) { return h ? h->K : 0; }
int sdsp_pfb_set_scale(sdsp_pfb* h, const void* scale) {
    if (!h || !scale) return SDSP_E_INVALID_ARGUMENT;
    std::memcpy(h->scale.data(), scale, h->scale.size());
    return SDSP_OK;
}
int sdsp_pfb_get_scale(const sdsp_pfb* h, void* scale) {
    if (!h || !scale) return SDSP_E_INVALID_ARGUMENT;
    std::memcpy(scale, h->scale.data(), h->scale.size());
    return SDSP_OK;
}
int sdsp_pfb_coefficients(const sdsp_pfb* h, void* out) {
    if (!h || !out) return SDSP_E_INVALID_ARGUMENT;
    std::memcpy(out, h->cb.data(), h->cb.size());
    return SDSP_OK;
}

int sdsp_pfb_set_algo(sdsp_pfb* h, int algo) {
    if (!h || (algo != SDSP_ALGO_EXACT && algo != SDSP_ALGO_FMA)) return SDSP_E_INVALID_ARGUMENT;
    h->algo = algo;
    return SDSP_OK;
}

int sdsp_pfb_set_channels(sdsp_pfb* h, size_t channels) {
    if (!h || channels == 0) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    h->channels = channels;
    return pfb_alloc_state(h);
}

int sdsp_pfb_execute_block_device(sdsp_pfb* h, const void* d_in, size_t n, void* d_out, void* stream) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (n == 0) return SDSP_OK;
    const PfbArgs a{d_in, h->hist.front(), h->d_cb.p, d_out, n, h->channels, (int)h->K, (int)h->M, (int)h->K,
                    h->algo != SDSP_ALGO_FMA};
    return h->block_device(d_in, n, d_out, n * h->M, stream, "pfb",
                           [&](hipStream_t s) { return launch_pfb(h->dtype, a, s); });
}

int sdsp_pfb_execute_block(sdsp_pfb* h, const void* in, size_t n, void* out) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (n == 0) return SDSP_OK;
    return h->block_host(in, n, out, n * h->M, [&](const void* d_in, void* d_out, hipStream_t s) {
        return sdsp_pfb_execute_block_device(h, d_in, n, d_out, s);
    });
}

int sdsp_pfb_push(sdsp_pfb* h, const void* sample) {
    if (!h || h->channels != 1) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    SDSP_TRY(h->fence.wait(), "wait for queued work");
    const size_t sb = sample_bytes(h->dtype);
    SDSP_TRY(h->stage_in.ensure(sb), "stage in");
    SDSP_TRY(hipMemcpyAsync(h->stage_in.p, sample, sb, hipMemcpyHostToDevice, h->stream), "H2D");
    SDSP_TRY(launch_hist_update(h->dtype, h->stage_in.p, h->hist.front(), h->hist.back(), 1,
                                (int)h->K, 1, h->stream),
             "window push");
    h->hist.flip();
    SDSP_TRY(hipStreamSynchronize(h->stream), "sync");
    return SDSP_OK;
}

int sdsp_pfb_execute(sdsp_pfb* h, size_t index, void* out) {
    if (!h || h->channels != 1 || index >= h->M) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    SDSP_TRY(h->fence.wait(), "wait for queued work");
    const size_t sb = sample_bytes(h->dtype);
    SDSP_TRY(h->stage_out.ensure(h->M * sb), "stage out");
    // all branches on the current window: x = newest sample, history = the K-1 before it
    const unsigned char* win = (const unsigned char*)h->hist.front();
    PfbArgs a{win + (h->K - 1) * sb, win, h->d_cb.p, h->stage_out.p, 1, 1, (int)h->K, (int)h->M,
              (int)h->K - 1, h->algo != SDSP_ALGO_FMA};
    SDSP_TRY(launch_pfb(h->dtype, a, h->stream), "pfb execute");
    SDSP_TRY(hipMemcpyAsync(out, (unsigned char*)h->stage_out.p + index * sb, sb, hipMemcpyDeviceToHost, h->stream),
             "D2H");
    SDSP_TRY(hipStreamSynchronize(h->stream), "sync");
    return SDSP_OK;
}

int sdsp_pfb_reset(sdsp_pfb* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    return pfb_alloc_state(h);
}

// InterpolatingFIRFilter::frequency_response / group_delay over the flattened
// branch coefficients (interp.rs:113-137); PolyPhaseFilterBank has no Filter impl.
int sdsp_pfb_frequency_response(const sdsp_pfb* h, double f, double* re_im) {
    if (!h || !re_im) return SDSP_E_INVALID_ARGUMENT;
    std::vector<cd> c(h->M * h->K);
    for (size_t i = 0; i < c.size(); ++i) c[i] = coef_at(h->cb.data(), h->dtype, i);
    const bool real = !coef_is_complex(h->dtype);
    cd o = poly_response(c, real, f);
    cd s = coef_at(h->scale.data(), h->dtype, 0);
    cd r = real ? cmul(s.re, o) : cmul(s, o);
    re_im[0] = r.re;
    re_im[1] = r.im;
    return SDSP_OK;
}

int sdsp_pfb_group_delay(const sdsp_pfb* h, double f, double* delay) {
    if (!h || !delay) return SDSP_E_INVALID_ARGUMENT;
    std::vector<cd> c(h->M * h->K);
    for (size_t i = 0; i < c.size(); ++i) c[i] = coef_at(h->cb.data(), h->dtype, i);
    double d = 0.0;
    if (fir_group_delay(c, !coef_is_complex(h->dtype), f, &d)) d = 0.0;
    *delay = d;
    return SDSP_OK;
}

int sdsp_pfb_synchronize(sdsp_pfb* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    return h->quiesce();
}

// ===========================================================================
// utilities
// ===========================================================================
int sdsp_bandwidth_copy_device(const void* d_src, void* d_dst, size_t bytes, void* stream) {
    int dev = 0;
    SDSP_TRY(hipGetDevice(&dev), "get device");
    hipDeviceProp_t p;
    SDSP_TRY(hipGetDeviceProperties(&p, dev), "props");
    SDSP_TRY(launch_bw_copy(d_src, d_dst, bytes, p.multiProcessorCount, (hipStream_t)stream), "bw copy");
    return SDSP_OK;
}

int sdsp_synth_f32_device(void* d_out, uint64_t seed, uint64_t channel, uint64_t start, size_t count,
                          void* stream) {
    SDSP_TRY(launch_synth_f32((float*)d_out, seed, channel, start, count, (hipStream_t)stream), "synth");
    return SDSP_OK;
}

}  // extern "C"

// C-ABI runtime of the digital down-converter (include/sdsp.h, sdsp_ddc_*): a decimating FIR
// whose input passes through the NCO's mix-down on the kernels' load path (kern_ddc.hip).  The
// handle owns what the two reference objects own: the decimator's reversed taps, delay line
// (ping-pong, mixed samples) and phase, and the oscillator's u32 phase and frequency registers
// (host state, as in sdsp_nco) with its sine table on the device.  A block object: no per-sample
// push and no host-step path.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "sdsp.h"
#include "sdsp_host.hpp"
#include "sdsp_kernels.hpp"

using namespace sdsp;

struct sdsp_ddc : HandleCore {
    int dtype = SDSP_RC32;
    size_t L = 0, M = 1, channels = 1;
    std::vector<unsigned char> taps;   // original order (clone)
    std::vector<unsigned char> scale;  // one Coef
    DevBuf d_taps_rev;                 // cr[i] = h[L-1-i]
    PingPong hist;                     // [channels][L-1] mixed samples, oldest first
    size_t ci = 0;                     // DecimatingFIRFilter::current_item
    int algo = SDSP_ALGO_EXACT;
    int decim_seg = 0;                 // SDSP_TUNE_DECIM_SEG
    uint32_t theta = 0, delta_theta = 0;  // NCO registers (src/nco/mod.rs:27-34)
    bool down = true;
    DevBuf d_table;                    // 1024-entry f64 sine table
};

namespace {

int ddc_alloc_state(sdsp_ddc* h) {
    SDSP_TRY(h->fence.wait(), "wait for queued work");
    SDSP_TRY(h->hist.reset(h->channels * (h->L - 1) * sample_bytes(h->dtype), h->stream), "zero history");
    h->ci = 0;
    return h->quiesce();
}

// AUTO: the fused multiply-add kernels for long 32-bit blocks (n inputs), as the decimator
int ddc_resolve_algo(const sdsp_ddc* h, size_t n) {
    if (h->algo != SDSP_ALGO_AUTO) return h->algo;
    return h->dtype <= SDSP_CC32 && n >= (size_t)(1 << 16) ? SDSP_ALGO_FMA : SDSP_ALGO_EXACT;
}

size_t hist_bytes(const sdsp_ddc* h) { return h->channels * (h->L - 1) * sample_bytes(h->dtype); }

}  // namespace

extern "C" {

int sdsp_ddc_create(sdsp_ddc** out, int dtype, const void* taps, size_t len, const void* scale, size_t decimation,
                    int device) {
    if (!out) return SDSP_E_INVALID_ARGUMENT;
    *out = nullptr;
    if (dtype != SDSP_RC32 && dtype != SDSP_CC32 && dtype != SDSP_RC64 && dtype != SDSP_CC64) {
        set_error("a down-converter takes complex samples: SDSP_RC32, SDSP_CC32, SDSP_RC64 or SDSP_CC64");
        return SDSP_E_INVALID_ARGUMENT;
    }
    if (!taps || !scale || len == 0 || len > (1u << 30)) {
        set_error("down-converter taps: 1 .. 2^30 coefficients and a scale");
        return SDSP_E_INVALID_ARGUMENT;
    }
    if (decimation < 1 || decimation > (1u << 30)) {
        set_error("down-converter decimation must be >= 1");
        return SDSP_E_INVALID_ARGUMENT;
    }
    int st = check_device(device, nullptr);
    if (st) return st;
    DeviceGuard g(device);
    sdsp_ddc* h = new sdsp_ddc();
    h->dtype = dtype;
    h->algo = default_algo();
    h->L = len;
    h->M = decimation;
    const size_t cb = coef_bytes(dtype);
    h->taps.assign((const unsigned char*)taps, (const unsigned char*)taps + len * cb);
    h->scale.assign((const unsigned char*)scale, (const unsigned char*)scale + cb);
    std::vector<unsigned char> rev(len * cb);
    for (size_t i = 0; i < len; ++i) std::memcpy(&rev[i * cb], &h->taps[(len - 1 - i) * cb], cb);
    double table[1024];
    nco_sine_table(table);
    hipError_t e = h->open(device);
    if (e == hipSuccess) e = h->d_taps_rev.ensure(rev.size());
    if (e == hipSuccess) e = hipMemcpy(h->d_taps_rev.p, rev.data(), rev.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h->d_table.ensure(sizeof(table));
    if (e == hipSuccess) e = hipMemcpy(h->d_table.p, table, sizeof(table), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        st = device_status(e, "ddc create");
        sdsp_ddc_destroy(h);
        return st;
    }
    st = ddc_alloc_state(h);
    if (st) {
        sdsp_ddc_destroy(h);
        return st;
    }
    *out = h;
    return SDSP_OK;
}

void sdsp_ddc_destroy(sdsp_ddc* h) { destroy_handle(h); }

int sdsp_ddc_clone(const sdsp_ddc* h, sdsp_ddc** out) {
    if (!h || !out) return SDSP_E_INVALID_ARGUMENT;
    int st = sdsp_ddc_create(out, h->dtype, h->taps.data(), h->L, h->scale.data(), h->M, h->device);
    if (st) return st;
    sdsp_ddc* c = *out;
    DeviceGuard g(h->device);
    c->algo = h->algo;
    c->decim_seg = h->decim_seg;
    c->down = h->down;
    c->theta = h->theta;
    c->delta_theta = h->delta_theta;
    // a failure from here on leaves the caller no handle to destroy
    auto fail = [&](int code) {
        sdsp_ddc_destroy(c);
        *out = nullptr;
        return code;
    };
    if (h->channels != 1 && (st = sdsp_ddc_set_channels(c, h->channels))) return fail(st);
    if ((st = h->quiesce())) return fail(st);
    const size_t hb = hist_bytes(h);
    if (hb) {
        const hipError_t e = hipMemcpy(c->hist.front(), h->hist.front(), hb, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) return fail(device_status(e, "clone state"));
    }
    c->ci = h->ci;
    return SDSP_OK;
}

int sdsp_ddc_reset(sdsp_ddc* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    h->theta = 0;  // NCO::reset  src/nco/mod.rs:53-56
    h->delta_theta = 0;
    return ddc_alloc_state(h);
}

int sdsp_ddc_set_channels(sdsp_ddc* h, size_t channels) {
    if (!h || channels == 0) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    h->channels = channels;
    return ddc_alloc_state(h);
}

int sdsp_ddc_set_algo(sdsp_ddc* h, int algo) {
    if (!h || algo < 0 || algo > 3) return SDSP_E_INVALID_ARGUMENT;
    if (algo == SDSP_ALGO_FFT) {
        set_error("overlap-save does not apply to a decimating handle");
        return SDSP_E_UNSUPPORTED;
    }
    h->algo = algo;
    return SDSP_OK;
}

int sdsp_ddc_get_algo(const sdsp_ddc* h) { return h ? h->algo : -1; }

int sdsp_ddc_set_direction(sdsp_ddc* h, int up) {
    if (!h || (up != 0 && up != 1)) return SDSP_E_INVALID_ARGUMENT;
    h->down = up == 0;
    return SDSP_OK;
}

// The oscillator's registers are host state read at each launch: a setter between two calls takes
// effect at the next call's first sample (src/nco/mod.rs:59-86; u32 adds wrap as in release builds)
int sdsp_ddc_set_frequency(sdsp_ddc* h, double delta_theta) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->delta_theta = nco_constrain(delta_theta);
    return SDSP_OK;
}
int sdsp_ddc_adjust_frequency(sdsp_ddc* h, double dt) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->delta_theta += nco_constrain(dt);
    return SDSP_OK;
}
int sdsp_ddc_set_phase(sdsp_ddc* h, double phi) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->theta = nco_constrain(phi);
    return SDSP_OK;
}
int sdsp_ddc_adjust_phase(sdsp_ddc* h, double delta_phi) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->theta += nco_constrain(delta_phi);
    return SDSP_OK;
}
int sdsp_ddc_get_nco_state(const sdsp_ddc* h, uint32_t* theta, uint32_t* delta_theta) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (theta) *theta = h->theta;
    if (delta_theta) *delta_theta = h->delta_theta;
    return SDSP_OK;
}
int sdsp_ddc_set_nco_state(sdsp_ddc* h, uint32_t theta, uint32_t delta_theta) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->theta = theta;
    h->delta_theta = delta_theta;
    return SDSP_OK;
}

size_t sdsp_ddc_output_count(const sdsp_ddc* h, size_t n) {
    if (!h) return 0;
    if (h->M == 1) return n;
    const size_t j0 = (h->M - 1 - h->ci) % h->M;  // first input index whose push wraps the phase to 0
    return j0 < n ? (n - 1 - j0) / h->M + 1 : 0;
}

int sdsp_ddc_execute_block_device(sdsp_ddc* h, const void* d_in, size_t n, void* d_out, size_t* n_out,
                                  void* stream) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    hipStream_t s = pick(stream, h->stream);
    const size_t nout = sdsp_ddc_output_count(h, n);
    if (n_out) *n_out = nout;
    if (n == 0) return SDSP_OK;
    if (!d_in || (nout && !d_out)) return SDSP_E_INVALID_ARGUMENT;
    const size_t sb = sample_bytes(h->dtype);
    if (ranges_overlap(d_in, h->channels * n * sb, d_out, h->channels * nout * sb)) {
        set_error("input and output blocks overlap (in-place filtering is not supported)");
        return SDSP_E_INVALID_ARGUMENT;
    }
    // work queued on another stream (the fence) reads or writes the history this launch uses
    SDSP_TRY(h->fence.order_before(s), "order after queued work");
    const void* hist = h->hist.front();
    const size_t j0 = (h->M - 1 - h->ci) % h->M;
    const bool exact = ddc_resolve_algo(h, n) != SDSP_ALGO_FMA;
    DdcArgs a{FirArgs{d_in, hist, h->d_taps_rev.p, h->scale.data(), d_out, n, nout, h->channels, (int)h->L,
                      (int)h->M, j0, exact},
              (const double*)h->d_table.p, h->theta, h->delta_theta, h->down};
    a.fir.seg = h->decim_seg;
    SDSP_TRY(launch_ddc(h->dtype, a, s), "ddc");
    SDSP_TRY(launch_ddc_hist(h->dtype, a, h->hist.back(), s), "ddc history update");
    h->hist.flip();
    h->ci = (h->ci + n) % h->M;
    h->theta += (uint32_t)((uint64_t)n * h->delta_theta);  // n steps, wrapping
    SDSP_TRY(h->fence.record(s), "record fence");
    return SDSP_OK;
}

int sdsp_ddc_execute_block(sdsp_ddc* h, const void* in, size_t n, void* out, size_t* n_out) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    SDSP_TRY(h->fence.wait(), "wait for queued work");
    const size_t sb = sample_bytes(h->dtype);
    const size_t nout = sdsp_ddc_output_count(h, n);
    if (n_out) *n_out = nout;
    if (n == 0) return SDSP_OK;
    if (!in || (nout && !out)) return SDSP_E_INVALID_ARGUMENT;
    return h->staged(in, h->channels * n * sb, out, h->channels * nout * sb,
                     [&](const void* d_in, void* d_out, hipStream_t s) {
                         return sdsp_ddc_execute_block_device(h, d_in, n, d_out, nullptr, s);
                     });
}

size_t sdsp_ddc_state_len(const sdsp_ddc* h) { return h ? h->channels * (h->L - 1) : 0; }

int sdsp_ddc_get_state(const sdsp_ddc* h, void* hist, size_t* phase) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    const size_t hb = hist_bytes(h);
    if (int st = h->quiesce()) return st;
    if (hb && hist) SDSP_TRY(hipMemcpy(hist, h->hist.front(), hb, hipMemcpyDeviceToHost), "get state");
    if (phase) *phase = h->ci;
    return SDSP_OK;
}

int sdsp_ddc_set_state(sdsp_ddc* h, const void* hist, size_t phase) {
    if (!h || phase >= h->M) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    const size_t hb = hist_bytes(h);
    if (int st = h->quiesce()) return st;
    if (hb && hist) SDSP_TRY(hipMemcpy(h->hist.front(), hist, hb, hipMemcpyHostToDevice), "set state");
    h->ci = phase;
    return SDSP_OK;
}

int sdsp_ddc_set_tuning(sdsp_ddc* h, int key, int value) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (key != SDSP_TUNE_DECIM_SEG || value < 0) {
        set_error("down-converter tuning: SDSP_TUNE_DECIM_SEG >= 0");
        return SDSP_E_INVALID_ARGUMENT;
    }
    h->decim_seg = value;
    return SDSP_OK;
}

int sdsp_ddc_synchronize(sdsp_ddc* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    return h->quiesce();
}

}  // extern "C"

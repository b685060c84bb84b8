// C-ABI runtime of the digital down-converter (include/sdsp.h, sdsp_ddc_*): a decimating FIR
// whose input passes through the NCO's mix-down on the kernels' load path (kern_ddc.hip).  The
// handle is what the two reference objects are: the decimator's state (FirCore, sdsp_host.hpp:
// reversed taps, ping-pong delay line of mixed samples, phase, algorithm) shared with sdsp_fir,
// and the oscillator (Oscillator, host registers as in sdsp_nco) with its sine table on the
// device and the mixing direction.  A block object: no per-sample push and no host-step path.
#include <hip/hip_runtime.h>

#include "sdsp.h"
#include "sdsp_host.hpp"
#include "sdsp_kernels.hpp"

using namespace sdsp;

struct sdsp_ddc : FirCore {
    Oscillator osc;
    bool down = true;
    DevBuf d_table;  // 1024-entry f64 sine table
};

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
    hipError_t e = h->init(dtype, taps, len, scale, decimation, device);
    if (e == hipSuccess) e = nco_upload_sine_table(h->d_table);
    st = device_status(e, "ddc create");
    if (!st) st = h->zero_state();
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
    c->down = h->down;
    c->osc = h->osc;
    st = h->copy_state_to(c);
    if (st) {  // a failure leaves the caller no handle to destroy
        sdsp_ddc_destroy(c);
        *out = nullptr;
    }
    return st;
}

int sdsp_ddc_reset(sdsp_ddc* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    h->osc.reset();
    return h->zero_state();
}

int sdsp_ddc_set_channels(sdsp_ddc* h, size_t channels) {
    if (!h || channels == 0) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    h->channels = channels;
    return h->zero_state();
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

// the oscillator's setters (Oscillator, sdsp_host.hpp): in effect from the next call's first sample
int sdsp_ddc_set_frequency(sdsp_ddc* h, double delta_theta) {
    return h ? h->osc.set_frequency(delta_theta) : SDSP_E_INVALID_ARGUMENT;
}
int sdsp_ddc_adjust_frequency(sdsp_ddc* h, double dt) {
    return h ? h->osc.adjust_frequency(dt) : SDSP_E_INVALID_ARGUMENT;
}
int sdsp_ddc_set_phase(sdsp_ddc* h, double phi) {
    return h ? h->osc.set_phase(phi) : SDSP_E_INVALID_ARGUMENT;
}
int sdsp_ddc_adjust_phase(sdsp_ddc* h, double delta_phi) {
    return h ? h->osc.adjust_phase(delta_phi) : SDSP_E_INVALID_ARGUMENT;
}
int sdsp_ddc_get_nco_state(const sdsp_ddc* h, uint32_t* theta, uint32_t* delta_theta) {
    return h ? h->osc.get(theta, delta_theta) : SDSP_E_INVALID_ARGUMENT;
}
int sdsp_ddc_set_nco_state(sdsp_ddc* h, uint32_t theta, uint32_t delta_theta) {
    return h ? h->osc.set(theta, delta_theta) : SDSP_E_INVALID_ARGUMENT;
}

size_t sdsp_ddc_output_count(const sdsp_ddc* h, size_t n) { return h ? h->output_count(n) : 0; }

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
    DdcArgs a{FirArgs{d_in, h->hist.front(), h->d_taps_rev.p, h->scale.data(), d_out, n, nout, h->channels,
                      (int)h->L, (int)h->M, h->j0(), h->decim_algo(n) != SDSP_ALGO_FMA},
              (const double*)h->d_table.p, h->osc.theta, h->osc.delta_theta, h->down};
    a.fir.seg = h->decim_seg;
    SDSP_TRY(launch_ddc(h->dtype, a, s), "ddc");
    SDSP_TRY(launch_ddc_hist(h->dtype, a, h->hist.back(), s), "ddc history update");
    h->hist.flip();
    h->ci = (h->ci + n) % h->M;
    h->osc.advance(n);
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

size_t sdsp_ddc_state_len(const sdsp_ddc* h) { return h ? h->state_len() : 0; }

int sdsp_ddc_get_state(const sdsp_ddc* h, void* hist, size_t* phase) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    if (int st = h->read_hist(hist)) return st;
    if (phase) *phase = h->ci;
    return SDSP_OK;
}

int sdsp_ddc_set_state(sdsp_ddc* h, const void* hist, size_t phase) {
    if (!h || phase >= h->M) return SDSP_E_INVALID_ARGUMENT;
    DeviceGuard g(h->device);
    if (int st = h->write_hist(hist)) return st;
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

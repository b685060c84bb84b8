// C-ABI runtime of the digital up-converter (include/sdsp.h, sdsp_duc_*): an interpolating FIR
// whose outputs pass through the NCO's mix-up on the kernels' store path (kern_duc.hip).  The
// handle is what the two reference objects are: an interpolator handle made by sdsp_interp_create
// (taps, branch layout, window of unmixed inputs, algorithm, the block path sdsp_pfb::block_device
// and the HandleCore every call here runs on: device, stream, fence, staging), and the oscillator
// (Oscillator, host registers as in sdsp_nco and sdsp_ddc) with its sine table on the device and
// the mixing direction.  A block object: no per-sample push and no per-branch execute.
#include <hip/hip_runtime.h>

#include "sdsp.h"
#include "sdsp_host.hpp"
#include "sdsp_kernels.hpp"

using namespace sdsp;

struct sdsp_duc {
    sdsp_pfb* f = nullptr;  // the interpolator
    Oscillator osc;
    bool down = false;
    DevBuf d_table;  // 1024-entry f64 sine table
};

namespace {

// the oscillator half of create and clone: *out owns `f` afterwards, or `f` is destroyed
int duc_wrap(sdsp_pfb* f, sdsp_duc** out) {
    DeviceGuard g(f->device);
    sdsp_duc* h = new sdsp_duc();
    h->f = f;
    if (const int st = device_status(nco_upload_sine_table(h->d_table), "duc create")) {
        sdsp_duc_destroy(h);
        return st;
    }
    *out = h;
    return SDSP_OK;
}

}  // namespace

extern "C" {

int sdsp_duc_create(sdsp_duc** out, int dtype, const void* taps, size_t len, size_t interpolation, int device) {
    if (!out) return SDSP_E_INVALID_ARGUMENT;
    *out = nullptr;
    if (dtype != SDSP_RC32 && dtype != SDSP_CC32 && dtype != SDSP_RC64 && dtype != SDSP_CC64) {
        set_error("an up-converter takes complex samples: SDSP_RC32, SDSP_CC32, SDSP_RC64 or SDSP_CC64");
        return SDSP_E_INVALID_ARGUMENT;
    }
    if (len && !taps) {
        set_error("up-converter taps: a null pointer");
        return SDSP_E_INVALID_ARGUMENT;
    }
    // len = 0, interpolation = 0, then the device: the interpolator's own checks, codes and layout
    sdsp_pfb* f = nullptr;
    if (int st = sdsp_interp_create(&f, dtype, taps, len, interpolation, device)) return st;
    return duc_wrap(f, out);
}

void sdsp_duc_destroy(sdsp_duc* h) {
    if (!h) return;
    {
        // work queued on a caller's stream may still read the table
        DeviceGuard g(h->f->device);
        (void)h->f->quiesce();
        h->d_table.release();
    }
    sdsp_pfb_destroy(h->f);
    delete h;
}

int sdsp_duc_clone(const sdsp_duc* h, sdsp_duc** out) {
    if (!h || !out) return SDSP_E_INVALID_ARGUMENT;
    *out = nullptr;
    sdsp_pfb* f = nullptr;
    if (int st = sdsp_pfb_clone(h->f, &f)) return st;  // taps, algorithm, channels, window
    if (int st = duc_wrap(f, out)) return st;
    (*out)->down = h->down;
    (*out)->osc = h->osc;
    return SDSP_OK;
}

int sdsp_duc_reset(sdsp_duc* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->osc.reset();
    return sdsp_pfb_reset(h->f);
}

int sdsp_duc_set_channels(sdsp_duc* h, size_t channels) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    return sdsp_pfb_set_channels(h->f, channels);
}

int sdsp_duc_set_algo(sdsp_duc* h, int algo) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    return sdsp_pfb_set_algo(h->f, algo);
}

int sdsp_duc_get_algo(const sdsp_duc* h) { return h ? h->f->algo : -1; }

int sdsp_duc_set_direction(sdsp_duc* h, int down) {
    if (!h || (down != 0 && down != 1)) return SDSP_E_INVALID_ARGUMENT;
    h->down = down == 1;
    return SDSP_OK;
}

// the oscillator's setters (Oscillator, sdsp_host.hpp): in effect from the next call's first output
int sdsp_duc_set_frequency(sdsp_duc* h, double delta_theta) {
    return h ? h->osc.set_frequency(delta_theta) : SDSP_E_INVALID_ARGUMENT;
}
int sdsp_duc_adjust_frequency(sdsp_duc* h, double dt) {
    return h ? h->osc.adjust_frequency(dt) : SDSP_E_INVALID_ARGUMENT;
}
int sdsp_duc_set_phase(sdsp_duc* h, double phi) {
    return h ? h->osc.set_phase(phi) : SDSP_E_INVALID_ARGUMENT;
}
int sdsp_duc_adjust_phase(sdsp_duc* h, double delta_phi) {
    return h ? h->osc.adjust_phase(delta_phi) : SDSP_E_INVALID_ARGUMENT;
}
int sdsp_duc_get_nco_state(const sdsp_duc* h, uint32_t* theta, uint32_t* delta_theta) {
    return h ? h->osc.get(theta, delta_theta) : SDSP_E_INVALID_ARGUMENT;
}
int sdsp_duc_set_nco_state(sdsp_duc* h, uint32_t theta, uint32_t delta_theta) {
    return h ? h->osc.set(theta, delta_theta) : SDSP_E_INVALID_ARGUMENT;
}

size_t sdsp_duc_interpolation(const sdsp_duc* h) { return h ? h->f->M : 0; }
size_t sdsp_duc_subfilter_len(const sdsp_duc* h) { return h ? h->f->K : 0; }

// the interpolator's block path with launch_duc as the kernel, then the oscillator's n * M steps
int sdsp_duc_execute_block_device(sdsp_duc* h, const void* d_in, size_t n, void* d_out, void* stream) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (n == 0) return SDSP_OK;
    sdsp_pfb* f = h->f;
    const DucArgs a{PfbArgs{d_in, f->hist.front(), f->d_cb.p, d_out, n, f->channels, (int)f->K, (int)f->M, (int)f->K,
                            f->algo != SDSP_ALGO_FMA},
                    (const double*)h->d_table.p, h->osc.theta, h->osc.delta_theta, h->down};
    if (int st = f->block_device(d_in, n, d_out, n * f->M, stream, "duc",
                                 [&](hipStream_t s) { return launch_duc(f->dtype, a, s); }))
        return st;
    h->osc.advance((uint64_t)n * f->M);
    return SDSP_OK;
}

int sdsp_duc_execute_block(sdsp_duc* h, const void* in, size_t n, void* out) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (n == 0) return SDSP_OK;
    return h->f->block_host(in, n, out, n * h->f->M, [&](const void* d_in, void* d_out, hipStream_t s) {
        return sdsp_duc_execute_block_device(h, d_in, n, d_out, s);
    });
}

int sdsp_duc_synchronize(sdsp_duc* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    return sdsp_pfb_synchronize(h->f);
}

}  // extern "C"

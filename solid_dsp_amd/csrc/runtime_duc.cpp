// C-ABI runtime of the digital up-converter (include/sdsp.h, sdsp_duc_*): an interpolating FIR
// whose outputs pass through the NCO's mix-up on the kernels' store path (kern_duc.hip).  The
// handle is what the two reference objects are: an interpolator handle made by sdsp_interp_create
// (taps, branch layout, window of unmixed inputs, algorithm, and the HandleCore every call here
// runs on: device, stream, fence, staging), and the oscillator's u32 phase and frequency registers
// (host state, as in sdsp_nco and sdsp_ddc) with its sine table on the device.  A block object: no
// per-sample push and no per-branch execute.
#include <hip/hip_runtime.h>

#include "sdsp.h"
#include "sdsp_host.hpp"
#include "sdsp_kernels.hpp"

using namespace sdsp;

struct sdsp_duc {
    sdsp_pfb* f = nullptr;                // the interpolator
    uint32_t theta = 0, delta_theta = 0;  // NCO registers (src/nco/mod.rs:27-34)
    bool down = false;
    DevBuf d_table;                       // 1024-entry f64 sine table
};

namespace {

// the oscillator half of create and clone: *out owns `f` afterwards, or `f` is destroyed
int duc_wrap(sdsp_pfb* f, sdsp_duc** out) {
    DeviceGuard g(f->device);
    sdsp_duc* h = new sdsp_duc();
    h->f = f;
    double table[1024];
    nco_sine_table(table);
    hipError_t e = h->d_table.ensure(sizeof(table));
    if (e == hipSuccess) e = hipMemcpy(h->d_table.p, table, sizeof(table), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        const int st = device_status(e, "duc create");
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
    (*out)->theta = h->theta;
    (*out)->delta_theta = h->delta_theta;
    return SDSP_OK;
}

int sdsp_duc_reset(sdsp_duc* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->theta = 0;  // NCO::reset  src/nco/mod.rs:53-56
    h->delta_theta = 0;
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

// The oscillator's registers are host state read at each launch: a setter between two calls takes
// effect at the next call's first output (src/nco/mod.rs:59-86; u32 adds wrap as in release builds)
int sdsp_duc_set_frequency(sdsp_duc* h, double delta_theta) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->delta_theta = nco_constrain(delta_theta);
    return SDSP_OK;
}
int sdsp_duc_adjust_frequency(sdsp_duc* h, double dt) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->delta_theta += nco_constrain(dt);
    return SDSP_OK;
}
int sdsp_duc_set_phase(sdsp_duc* h, double phi) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->theta = nco_constrain(phi);
    return SDSP_OK;
}
int sdsp_duc_adjust_phase(sdsp_duc* h, double delta_phi) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->theta += nco_constrain(delta_phi);
    return SDSP_OK;
}
int sdsp_duc_get_nco_state(const sdsp_duc* h, uint32_t* theta, uint32_t* delta_theta) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (theta) *theta = h->theta;
    if (delta_theta) *delta_theta = h->delta_theta;
    return SDSP_OK;
}
int sdsp_duc_set_nco_state(sdsp_duc* h, uint32_t theta, uint32_t delta_theta) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->theta = theta;
    h->delta_theta = delta_theta;
    return SDSP_OK;
}

size_t sdsp_duc_interpolation(const sdsp_duc* h) { return h ? h->f->M : 0; }
size_t sdsp_duc_subfilter_len(const sdsp_duc* h) { return h ? h->f->K : 0; }

// sdsp_pfb_execute_block_device with launch_duc in launch_pfb's place and the oscillator's advance
int sdsp_duc_execute_block_device(sdsp_duc* h, const void* d_in, size_t n, void* d_out, void* stream) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (n == 0) return SDSP_OK;
    sdsp_pfb* f = h->f;
    DeviceGuard g(f->device);
    hipStream_t s = pick(stream, f->stream);
    const size_t sb = sample_bytes(f->dtype);
    if (ranges_overlap(d_in, f->channels * n * sb, d_out, f->channels * n * f->M * sb)) {
        set_error("input and output blocks overlap (in-place filtering is not supported)");
        return SDSP_E_INVALID_ARGUMENT;
    }
    // work queued on another stream (the fence) reads or writes the window this launch uses
    SDSP_TRY(f->fence.order_before(s), "order after queued work");
    const DucArgs a{PfbArgs{d_in, f->hist.front(), f->d_cb.p, d_out, n, f->channels, (int)f->K, (int)f->M, (int)f->K,
                            f->algo != SDSP_ALGO_FMA},
                    (const double*)h->d_table.p, h->theta, h->delta_theta, h->down};
    SDSP_TRY(launch_duc(f->dtype, a, s), "duc");
    SDSP_TRY(launch_hist_update(f->dtype, d_in, f->hist.front(), f->hist.back(), n, (int)f->K, f->channels, s),
             "window update");
    f->hist.flip();
    h->theta += (uint32_t)((uint64_t)n * f->M) * h->delta_theta;  // n*M steps, wrapping
    SDSP_TRY(f->fence.record(s), "record fence");
    return SDSP_OK;
}

int sdsp_duc_execute_block(sdsp_duc* h, const void* in, size_t n, void* out) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (n == 0) return SDSP_OK;
    sdsp_pfb* f = h->f;
    DeviceGuard g(f->device);
    const size_t bytes = f->channels * n * sample_bytes(f->dtype);
    return f->staged(in, bytes, out, bytes * f->M, [&](const void* d_in, void* d_out, hipStream_t s) {
        return sdsp_duc_execute_block_device(h, d_in, n, d_out, s);
    });
}

int sdsp_duc_synchronize(sdsp_duc* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    return sdsp_pfb_synchronize(h->f);
}

}  // extern "C"

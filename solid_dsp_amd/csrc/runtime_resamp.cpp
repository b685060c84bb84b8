// C-ABI runtime of the rational resampler (include/sdsp.h, sdsp_resamp_*): an interpolating FIR
// whose output is taken every D-th sample, with only the kept dot products computed
// (kern_resamp.hip).  The handle owns an interpolator handle made by sdsp_interp_create, as the
// up-converter does (taps, K, zero padding, branch layout, window, algorithm, the block path
// sdsp_pfb::block_device and the HandleCore every call here runs on), and adds the decimation D,
// the phase counter c (host state, the reference decimator's counter applied to the interpolated
// stream) and the kernel knob.  A block object: no per-sample entry point, no scale, no window
// get / set.
#include <hip/hip_runtime.h>

#include "sdsp.h"
#include "sdsp_host.hpp"
#include "sdsp_kernels.hpp"

using namespace sdsp;

struct sdsp_resamp {
    sdsp_pfb* f = nullptr;  // the interpolator
    size_t D = 1, c = 0;    // decimation; interpolated samples since the last one kept, < D
    int kernel = 0;         // SDSP_TUNE_RESAMP_KERNEL
};

extern "C" {

int sdsp_resamp_count(size_t interpolation, size_t decimation, size_t phase, size_t n, size_t* n_out,
                      size_t* next_phase) {
    if (interpolation == 0 || decimation == 0 || phase >= decimation) return SDSP_E_INVALID_ARGUMENT;
    const unsigned __int128 t = (unsigned __int128)phase + (unsigned __int128)n * interpolation;
    if (t >> 63) return SDSP_E_INVALID_ARGUMENT;  // c + n M has to fit 63 bits
    const unsigned long long v = (unsigned long long)t;
    if (n_out) *n_out = (size_t)(v / decimation);
    if (next_phase) *next_phase = (size_t)(v % decimation);
    return SDSP_OK;
}

int sdsp_resamp_create(sdsp_resamp** out, int dtype, const void* taps, size_t len, size_t interpolation,
                       size_t decimation, int device) {
    if (!out) return SDSP_E_INVALID_ARGUMENT;
    *out = nullptr;
    if (dtype < 0 || dtype > 5) {
        set_error("resampler dtype: not one of the six (Coef, In) pairs");
        return SDSP_E_INVALID_ARGUMENT;
    }
    if (len && !taps) {
        set_error("resampler taps: a null pointer");
        return SDSP_E_INVALID_ARGUMENT;
    }
    if (decimation == 0) {
        set_error("FIR Filter Error DecimationLessThanOne");
        return SDSP_E_DECIMATION_LESS_THAN_ONE;
    }
    if (decimation > 0x7fffffffULL) {
        set_error("resampler decimation: larger than 2^31 - 1");
        return SDSP_E_INVALID_ARGUMENT;
    }
    // len = 0, interpolation = 0, then the device: the interpolator's own checks, codes and layout
    sdsp_pfb* f = nullptr;
    if (int st = sdsp_interp_create(&f, dtype, taps, len, interpolation, device)) return st;
    sdsp_resamp* h = new sdsp_resamp();
    h->f = f;
    h->D = decimation;
    *out = h;
    return SDSP_OK;
}

void sdsp_resamp_destroy(sdsp_resamp* h) {
    if (!h) return;
    sdsp_pfb_destroy(h->f);  // waits for queued work first
    delete h;
}

int sdsp_resamp_clone(const sdsp_resamp* h, sdsp_resamp** out) {
    if (!h || !out) return SDSP_E_INVALID_ARGUMENT;
    *out = nullptr;
    sdsp_pfb* f = nullptr;
    if (int st = sdsp_pfb_clone(h->f, &f)) return st;  // taps, algorithm, channels, window
    sdsp_resamp* c = new sdsp_resamp(*h);
    c->f = f;
    *out = c;
    return SDSP_OK;
}

int sdsp_resamp_reset(sdsp_resamp* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->c = 0;
    return sdsp_pfb_reset(h->f);
}

int sdsp_resamp_set_channels(sdsp_resamp* h, size_t channels) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (int st = sdsp_pfb_set_channels(h->f, channels)) return st;
    h->c = 0;
    return SDSP_OK;
}

int sdsp_resamp_set_algo(sdsp_resamp* h, int algo) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    return sdsp_pfb_set_algo(h->f, algo);
}

int sdsp_resamp_get_algo(const sdsp_resamp* h) { return h ? h->f->algo : -1; }

int sdsp_resamp_set_tuning(sdsp_resamp* h, int key, int value) {
    if (!h || key != SDSP_TUNE_RESAMP_KERNEL || value < 0 || value > 3) return SDSP_E_INVALID_ARGUMENT;
    h->kernel = value;
    return SDSP_OK;
}

size_t sdsp_resamp_interpolation(const sdsp_resamp* h) { return h ? h->f->M : 0; }
size_t sdsp_resamp_decimation(const sdsp_resamp* h) { return h ? h->D : 0; }
size_t sdsp_resamp_subfilter_len(const sdsp_resamp* h) { return h ? h->f->K : 0; }

int sdsp_resamp_get_phase(const sdsp_resamp* h, size_t* phase) {
    if (!h || !phase) return SDSP_E_INVALID_ARGUMENT;
    *phase = h->c;
    return SDSP_OK;
}

int sdsp_resamp_set_phase(sdsp_resamp* h, size_t phase) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (phase >= h->D) {
        set_error("resampler phase: not below the decimation");
        return SDSP_E_INVALID_ARGUMENT;
    }
    h->c = phase;
    return SDSP_OK;
}

size_t sdsp_resamp_output_count(const sdsp_resamp* h, size_t n) {
    size_t n_out = 0;
    if (!h || sdsp_resamp_count(h->f->M, h->D, h->c, n, &n_out, nullptr)) return 0;
    return n_out;
}

int sdsp_resamp_info(const sdsp_resamp* h, int* kernel, size_t* tile) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    const ResampPlan p = resamp_plan(h->f->dtype, (int)h->f->M, h->D, (int)h->f->K, h->kernel);
    if (kernel) *kernel = p.kernel;
    if (tile) *tile = p.tile;
    return SDSP_OK;
}

int sdsp_resamp_execute_block_device(sdsp_resamp* h, const void* d_in, size_t n, void* d_out, size_t* n_out,
                                     void* stream) {
    if (n_out) *n_out = 0;
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (n == 0) return SDSP_OK;
    sdsp_pfb* f = h->f;
    size_t no = 0, next = 0;
    if (sdsp_resamp_count(f->M, h->D, h->c, n, &no, &next)) {
        set_error("resampler block: n * interpolation does not fit 63 bits");
        return SDSP_E_INVALID_ARGUMENT;
    }
    const ResampArgs a{d_in, f->hist.front(), f->d_cb.p, d_out, n, no, f->channels, (int)f->K, (int)f->M, (int)f->K,
                       h->D, h->c, f->algo != SDSP_ALGO_FMA, h->kernel};
    if (int st = f->block_device(d_in, n, d_out, no, stream, "resamp",  // (launches nothing when no == 0)
                                 [&](hipStream_t s) { return launch_resamp(f->dtype, a, s); }))
        return st;
    h->c = next;
    if (n_out) *n_out = no;
    return SDSP_OK;
}

int sdsp_resamp_execute_block(sdsp_resamp* h, const void* in, size_t n, void* out, size_t* n_out) {
    if (n_out) *n_out = 0;
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (n == 0) return SDSP_OK;
    return h->f->block_host(in, n, out, sdsp_resamp_output_count(h, n),
                            [&](const void* d_in, void* d_out, hipStream_t s) {
                                return sdsp_resamp_execute_block_device(h, d_in, n, d_out, n_out, s);
                            });
}

int sdsp_resamp_synchronize(sdsp_resamp* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    return sdsp_pfb_synchronize(h->f);
}

}  // extern "C"

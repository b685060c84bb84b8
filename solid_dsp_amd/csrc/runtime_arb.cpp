// C-ABI runtime of the arbitrary-rate resampler (include/sdsp.h, sdsp_arb_*): an interpolating FIR
// with P branches whose stream is read at a Q32.32 time accumulator, each output a linear
// interpolation between two neighbouring interpolated samples (kern_arb.hip).  The handle owns an
// interpolator handle made by sdsp_interp_create, as the rational resampler does (taps, K, zero
// padding, branch layout, window, algorithm, the block path sdsp_pfb::block_device and the
// HandleCore every call here runs on), and adds the step, the time of the next output (host state,
// shared by all channels) and the kernel knob.  Every call runs on sdsp_arb_count, a host-only
// function.  A block object: no per-sample entry point, no scale, no window get / set.
#include <hip/hip_runtime.h>

#include <cmath>

#include "sdsp.h"
#include "sdsp_host.hpp"
#include "sdsp_kernels.hpp"

using namespace sdsp;

struct sdsp_arb {
    sdsp_pfb* f = nullptr;  // the interpolator
    uint64_t step = 0;      // input samples per output, Q32.32
    uint64_t t = 0;         // time of the next output from the next call's first input, Q32.32, < 2^63
    int kernel = 0;         // SDSP_TUNE_ARB_KERNEL
};

namespace {

constexpr uint64_t kStepMin = 1ULL << 16, kStepMax = 1ULL << 48;
bool step_ok(uint64_t step) { return step >= kStepMin && step <= kStepMax; }

}  // namespace

extern "C" {

int sdsp_arb_count(uint64_t step, uint64_t t, size_t n, size_t* n_out, uint64_t* next_t) {
    if (!step_ok(step) || (t >> 63) || n >= (1ULL << 31)) return SDSP_E_INVALID_ARGUMENT;
    const uint64_t end = (uint64_t)n << 32;  // < 2^63
    uint64_t no = 0, next = 0;
    if (t >= end) {
        next = t - end;
    } else {
        const uint64_t d = end - t;  // d + step - 1 < 2^63 + 2^48
        no = (d + step - 1) / step;
        next = no * step - d;  // < step
    }
    if (n_out) *n_out = (size_t)no;
    if (next_t) *next_t = next;
    return SDSP_OK;
}

int sdsp_arb_step_from_rate(double rate, uint64_t* step) {
    if (!step || !std::isfinite(rate) || !(rate > 0.0)) return SDSP_E_INVALID_ARGUMENT;
    const double v = std::floor(std::ldexp(1.0 / rate, 32) + 0.5);
    if (!(v >= (double)kStepMin && v <= (double)kStepMax)) return SDSP_E_INVALID_ARGUMENT;  // (not finite too)
    *step = (uint64_t)v;
    return SDSP_OK;
}

int sdsp_arb_create(sdsp_arb** out, int dtype, const void* taps, size_t len, size_t filters, uint64_t step,
                    int device) {
    if (!out) return SDSP_E_INVALID_ARGUMENT;
    *out = nullptr;
    if (dtype < 0 || dtype > 5) {
        set_error("arbitrary-rate resampler dtype: not one of the six (Coef, In) pairs");
        return SDSP_E_INVALID_ARGUMENT;
    }
    if (len && !taps) {
        set_error("arbitrary-rate resampler taps: a null pointer");
        return SDSP_E_INVALID_ARGUMENT;
    }
    if (!step_ok(step)) {
        set_error("arbitrary-rate resampler step: outside 2^16 .. 2^48");
        return SDSP_E_INVALID_ARGUMENT;
    }
    if (filters > 0x7fffffffULL) {
        set_error("arbitrary-rate resampler filters: larger than 2^31 - 1");
        return SDSP_E_INVALID_ARGUMENT;
    }
    // len = 0, filters = 0, then the device: the interpolator's own checks, codes and layout
    sdsp_pfb* f = nullptr;
    if (int st = sdsp_interp_create(&f, dtype, taps, len, filters, device)) return st;
    sdsp_arb* h = new sdsp_arb();
    h->f = f;
    h->step = step;
    *out = h;
    return SDSP_OK;
}

void sdsp_arb_destroy(sdsp_arb* h) {
    if (!h) return;
    sdsp_pfb_destroy(h->f);  // waits for queued work first
    delete h;
}

int sdsp_arb_clone(const sdsp_arb* h, sdsp_arb** out) {
    if (!h || !out) return SDSP_E_INVALID_ARGUMENT;
    *out = nullptr;
    sdsp_pfb* f = nullptr;
    if (int st = sdsp_pfb_clone(h->f, &f)) return st;  // taps, algorithm, channels, window
    sdsp_arb* c = new sdsp_arb(*h);
    c->f = f;
    *out = c;
    return SDSP_OK;
}

int sdsp_arb_reset(sdsp_arb* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    h->t = 0;
    return sdsp_pfb_reset(h->f);
}

int sdsp_arb_set_channels(sdsp_arb* h, size_t channels) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (int st = sdsp_pfb_set_channels(h->f, channels)) return st;
    h->t = 0;
    return SDSP_OK;
}

int sdsp_arb_set_algo(sdsp_arb* h, int algo) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    return sdsp_pfb_set_algo(h->f, algo);
}

int sdsp_arb_get_algo(const sdsp_arb* h) { return h ? h->f->algo : -1; }

int sdsp_arb_set_tuning(sdsp_arb* h, int key, int value) {
    if (!h || key != SDSP_TUNE_ARB_KERNEL || value < 0 || value > 2) return SDSP_E_INVALID_ARGUMENT;
    h->kernel = value;
    return SDSP_OK;
}

size_t sdsp_arb_filters(const sdsp_arb* h) { return h ? h->f->M : 0; }
size_t sdsp_arb_subfilter_len(const sdsp_arb* h) { return h ? h->f->K : 0; }

int sdsp_arb_get_step(const sdsp_arb* h, uint64_t* step) {
    if (!h || !step) return SDSP_E_INVALID_ARGUMENT;
    *step = h->step;
    return SDSP_OK;
}

int sdsp_arb_set_step(sdsp_arb* h, uint64_t step) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (!step_ok(step)) {
        set_error("arbitrary-rate resampler step: outside 2^16 .. 2^48");
        return SDSP_E_INVALID_ARGUMENT;
    }
    h->step = step;
    return SDSP_OK;
}

int sdsp_arb_get_time(const sdsp_arb* h, uint64_t* t) {
    if (!h || !t) return SDSP_E_INVALID_ARGUMENT;
    *t = h->t;
    return SDSP_OK;
}

int sdsp_arb_set_time(sdsp_arb* h, uint64_t t) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (t >> 63) {
        set_error("arbitrary-rate resampler time: not below 2^63");
        return SDSP_E_INVALID_ARGUMENT;
    }
    h->t = t;
    return SDSP_OK;
}

size_t sdsp_arb_output_count(const sdsp_arb* h, size_t n) {
    size_t n_out = 0;
    if (!h || sdsp_arb_count(h->step, h->t, n, &n_out, nullptr)) return 0;
    return n_out;
}

int sdsp_arb_info(const sdsp_arb* h, int* kernel, size_t* tile) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    const ArbPlan p = arb_plan(h->f->dtype, (int)h->f->M, h->step, (int)h->f->K, h->kernel);
    if (kernel) *kernel = p.kernel;
    if (tile) *tile = p.tile;
    return SDSP_OK;
}

int sdsp_arb_execute_block_device(sdsp_arb* h, const void* d_in, size_t n, void* d_out, size_t* n_out,
                                  void* stream) {
    if (n_out) *n_out = 0;
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (n == 0) return SDSP_OK;
    sdsp_pfb* f = h->f;
    size_t no = 0;
    uint64_t next = 0;
    if (sdsp_arb_count(h->step, h->t, n, &no, &next)) {
        set_error("arbitrary-rate resampler block: n is not below 2^31");
        return SDSP_E_INVALID_ARGUMENT;
    }
    const ArbArgs a{d_in, f->hist.front(), f->d_cb.p, d_out, n, no, f->channels, (int)f->K, (int)f->M, (int)f->K,
                    h->step, h->t, f->algo != SDSP_ALGO_FMA, h->kernel};
    if (int st = f->block_device(d_in, n, d_out, no, stream, "arb",  // (launches nothing when no == 0)
                                 [&](hipStream_t s) { return launch_arb(f->dtype, a, s); }))
        return st;
    h->t = next;
    if (n_out) *n_out = no;
    return SDSP_OK;
}

int sdsp_arb_execute_block(sdsp_arb* h, const void* in, size_t n, void* out, size_t* n_out) {
    if (n_out) *n_out = 0;
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    if (n == 0) return SDSP_OK;
    if (n >= (1ULL << 31)) {
        set_error("arbitrary-rate resampler block: n is not below 2^31");
        return SDSP_E_INVALID_ARGUMENT;
    }
    return h->f->block_host(in, n, out, sdsp_arb_output_count(h, n),
                            [&](const void* d_in, void* d_out, hipStream_t s) {
                                return sdsp_arb_execute_block_device(h, d_in, n, d_out, n_out, s);
                            });
}

int sdsp_arb_synchronize(sdsp_arb* h) {
    if (!h) return SDSP_E_INVALID_ARGUMENT;
    return sdsp_pfb_synchronize(h->f);
}

}  // extern "C"

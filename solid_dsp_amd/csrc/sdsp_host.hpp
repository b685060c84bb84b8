// Internal host-side helpers shared by the runtime units (runtime*.cpp) and design.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "sdsp.h"
#include "sdsp_kernels.hpp"

namespace sdsp {

struct cd { double re, im; };

cd cmul(cd a, cd b);
cd cmul(double a, cd b);
cd cadd(cd a, cd b);
cd cdiv(cd a, cd b);
cd from_polar(double r, double t);
cd poly_response(const std::vector<cd>& c, bool real, double f);
int fir_group_delay(const std::vector<cd>& h, bool real, double f, double* out);
int iir_group_delay(const std::vector<double>& b, const std::vector<double>& a, double f, double* out);

// in-place radix-2 FFT of M (a power of two) interleaved complex f64 values, forward sign
// (design.cpp)
void host_fft_pow2(std::vector<double>& a, size_t M);

void set_error(const std::string& msg);
// the algorithm new FIR-type and IIR handles start on (sdsp_set_default_algo; SDSP_DEFAULT_ALGO)
int default_algo();
int device_status(hipError_t e, const char* what);
#define SDSP_TRY(expr, what)                                        \
    do {                                                            \
        hipError_t _e = (expr);                                     \
        if (_e != hipSuccess) return sdsp::device_status(_e, what); \
    } while (0)

// the NCO's phase arithmetic (runtime_rx.cpp): constrain() of an angle to the u32 phase register,
// and the 1024-entry f64 sine table of NCO::new
uint32_t nco_constrain(double theta);
void nco_sine_table(double* table);

// [a, a + na) and [b, b + nb) overlap (byte ranges)
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!na || !nb) return false;
    const auto pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + nb && pb < pa + na;
}

// SDSP_OK when `device` is a usable gfx950 device, SDSP_E_NO_DEVICE otherwise; *cus (when given)
// receives its compute-unit count
int check_device(int device, int* cus);

// makes `d` the calling thread's device for a scope and puts the caller's back
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int d) {
        (void)hipGetDevice(&prev);
        if (prev != d) (void)hipSetDevice(d);
    }
    ~DeviceGuard() {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
    }
};

// the stream a call runs on: the caller's, or the handle's own when none is given
inline hipStream_t pick(void* user, hipStream_t own) { return user ? (hipStream_t)user : own; }

// dtype traits (sdsp_dtype)
inline size_t sample_bytes(int dt) {
    static const size_t b[6] = {4, 8, 8, 8, 16, 16};
    return (dt >= 0 && dt < 6) ? b[dt] : 0;
}
inline size_t coef_bytes(int dt) {
    static const size_t b[6] = {4, 4, 8, 8, 8, 16};
    return (dt >= 0 && dt < 6) ? b[dt] : 0;
}
inline bool coef_is_complex(int dt) { return dt == 2 || dt == 5; }
inline bool coef_is_f32(int dt) { return dt <= 2; }

// widen one stored coefficient to complex<f64>
inline cd coef_at(const unsigned char* p, int dt, size_t i) {
    switch (dt) {
        case 0: case 1: { float v; std::memcpy(&v, p + 4 * i, 4); return {(double)v, 0.0}; }
        case 2: { float v[2]; std::memcpy(v, p + 8 * i, 8); return {(double)v[0], (double)v[1]}; }
        case 3: case 4: { double v; std::memcpy(&v, p + 8 * i, 8); return {v, 0.0}; }
        case 5: { double v[2]; std::memcpy(v, p + 16 * i, 16); return {v[0], v[1]}; }
    }
    return {0.0, 0.0};
}

// pinned host memory mapped into the device address space (coherent): a kernel
// writes it directly, the host reads it after the stream synchronises
struct HostMapped {
    void* host = nullptr;
    void* dev = nullptr;
    HostMapped() = default;
    HostMapped(const HostMapped&) = delete;
    HostMapped& operator=(const HostMapped&) = delete;
    ~HostMapped() {
        if (host) (void)hipHostFree(host);
    }
    hipError_t ensure(size_t bytes) {
        if (host) return hipSuccess;
        hipError_t e = hipHostMalloc(&host, bytes, hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) {
            host = nullptr;
            return e;
        }
        return hipHostGetDevicePointer(&dev, host, 0);
    }
};

// Wait until a kernel has released *flag == seq into host-mapped memory: a short
// spin (the step kernels finish within microseconds of the launch), then the
// stream's own synchronisation, which also surfaces launch errors.
inline hipError_t wait_host_flag(const unsigned* flag, unsigned seq, hipStream_t s) {
    for (int i = 0; i < (1 << 22); ++i) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return hipSuccess;
        __builtin_ia32_pause();
    }
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq ? hipSuccess : hipErrorUnknown;
}

// owned device allocation
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t ensure(size_t b) {
        if (b <= bytes && p) return hipSuccess;
        release();
        if (b == 0) b = 16;
        hipError_t e = hipMalloc(&p, b);
        if (e == hipSuccess) bytes = b;
        else p = nullptr;
        return e;
    }
};

// Completion marker of the last work a handle queued, on whichever stream it went
// (a caller's stream or the handle's own).  *_execute_block_device may run on any
// stream: each launch is first ordered after the marker (order_before) and then
// records a new one (record), so a call on a caller stream s1, a call on the handle
// stream and another call on s1 run in that order.  Host-side operations (the
// host-slice entry points, reset and the other state reallocations, set_state /
// get_state, clone, table rebuilds after set_scale, *_synchronize and destroy) first
// wait for the marker (HandleCore::quiesce, HandleCore::staged), so a kernel still
// reading the delay line or the tables is never raced by a host copy on the handle's
// own stream, or by a free.  The fir, pfb, iir, chan, acorr and agc handles record
// it; the fft and nco handles do not (the boundary).
//
// The markers rotate through kRing events: a stream never re-records the event it
// has just waited on (a stream waiting on an event that it then re-records every
// call crashed the host side in round 3), and an event is only
// recorded again kRing records later.
struct StreamFence {
    static constexpr int kRing = 4;
    hipEvent_t ev[kRing] = {};
    int cur = 0;                   // ev[cur] is the pending marker
    hipStream_t stream = nullptr;  // where the pending marker was recorded
    bool pending = false;
    StreamFence() = default;
    StreamFence(const StreamFence&) = delete;
    StreamFence& operator=(const StreamFence&) = delete;
    ~StreamFence() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    // A marker on the legacy default stream is recorded through its null handle: an event
    // recorded on the special handle hipStreamLegacy makes every later hipStreamWaitEvent on
    // it crash inside the runtime (SIGSEGV, any waiting stream), while one recorded on the null
    // stream is waited for normally (tools/fence_probe.hip, profiles/r05/fence_probe.log: the
    // round-4 AutoCorrelator crash, a block on torch's default stream followed by get_energy)
    hipError_t record(hipStream_t s) {
        const int nxt = (cur + 1) % kRing;
        if (!ev[nxt]) {
            hipError_t e = hipEventCreateWithFlags(&ev[nxt], hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        hipError_t e = hipEventRecord(ev[nxt], legacy(s) ? nullptr : s);
        if (e != hipSuccess) return e;
        cur = nxt;
        pending = true;
        stream = s;
        return hipSuccess;
    }
    // order work about to be queued on `s` after the pending marker (nothing to do on the
    // marker's own stream: stream order; the null handle and hipStreamLegacy are the same
    // stream).  Device-side waits from any stream, the legacy one included (record() keeps the
    // marker off the hipStreamLegacy handle)
    hipError_t order_before(hipStream_t s) {
        if (!pending || s == stream || (legacy(s) && legacy(stream))) return hipSuccess;
        return hipStreamWaitEvent(s, ev[cur], 0);
    }
    static bool legacy(hipStream_t s) { return s == nullptr || s == hipStreamLegacy; }
    // the marker stays pending until a synchronize has succeeded (a failed wait must
    // not let later host operations skip it)
    hipError_t wait() {
        if (!pending) return hipSuccess;
        const hipError_t e = hipEventSynchronize(ev[cur]);
        if (e == hipSuccess) pending = false;
        return e;
    }
};

// Delay-line state that a kernel reads from one buffer and writes to the other: front() is the
// current state, back() the one the next launch writes, flip() after that launch
struct PingPong {
    DevBuf buf[2];
    int cur = 0;
    void* front() const { return buf[cur].p; }
    void* back() const { return buf[cur ^ 1].p; }
    void flip() { cur ^= 1; }
    // both halves hold `bytes` zeroed bytes (queued on `s`), front() is the first
    hipError_t reset(size_t bytes, hipStream_t s) {
        for (DevBuf& b : buf) {
            hipError_t e = b.ensure(bytes);
            if (e == hipSuccess && bytes) e = hipMemsetAsync(b.p, 0, bytes, s);
            if (e != hipSuccess) return e;
        }
        cur = 0;
        return hipSuccess;
    }
};

// What every handle of the C ABI owns besides its own tables and state: its device, a
// non-blocking stream, the fence of the last block it queued and the staging buffers of its
// host-slice entry points.  Every handle struct derives from it.
struct HandleCore {
    int device = 0;
    hipStream_t stream = nullptr;
    mutable StreamFence fence;
    DevBuf stage_in, stage_out;

    hipError_t open(int dev) {
        device = dev;
        return hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    }
    // nothing the handle queued is running any more, on a caller's stream or its own: the body of
    // every *_synchronize, and what state reads, writes, reallocations and destroy wait for first
    int quiesce() const {
        SDSP_TRY(fence.wait(), "wait for queued work");
        SDSP_TRY(hipStreamSynchronize(stream), "sync");
        return SDSP_OK;
    }
    // A host-slice entry point: in -> stage_in, run(d_in, d_out, stream) -> status, stage_out -> out
    // (when out_bytes and run returned 0), synchronised.  The fence wait comes first for every
    // handle: the call is synchronous and run() orders itself after the fence anyway, so waiting
    // here changes nothing observable and keeps the staging copies out of a queued block's way.
    template <typename Run> int staged(const void* in, size_t in_bytes, void* out, size_t out_bytes, Run run) {
        SDSP_TRY(fence.wait(), "wait for queued work");
        SDSP_TRY(stage_in.ensure(in_bytes), "stage in");
        SDSP_TRY(stage_out.ensure(out_bytes), "stage out");
        SDSP_TRY(hipMemcpyAsync(stage_in.p, in, in_bytes, hipMemcpyHostToDevice, stream), "H2D");
        const int st = run(stage_in.p, stage_out.p, stream);
        if (st) return st;
        if (out_bytes) SDSP_TRY(hipMemcpyAsync(out, stage_out.p, out_bytes, hipMemcpyDeviceToHost, stream), "D2H");
        SDSP_TRY(hipStreamSynchronize(stream), "sync");
        return SDSP_OK;
    }
};

// The body of every *_destroy.  The order matters: the waits come before any free, because work
// queued on a caller stream may still read the tables and the history; and the handle is deleted
// inside the guard's scope, so every DevBuf member frees under the handle's device.
template <typename H> void destroy_handle(H* h) {
    if (!h) return;
    DeviceGuard g(h->device);
    if (h->stream) {  // (no stream: create failed before anything was queued)
        (void)h->quiesce();
        (void)hipStreamDestroy(h->stream);
    }
    delete h;
}

// The oscillator of the NCO, the down-converter and the up-converter: the two u32 registers of
// struct NCO (src/nco/mod.rs:27-34) as host state, read at each launch, so a setter between two
// calls takes effect at the next call's first sample (:53-86; u32 adds wrap as in release builds)
// The setters return SDSP_OK: the exported functions forward to them.
struct Oscillator {
    uint32_t theta = 0, delta_theta = 0;
    void reset() { theta = delta_theta = 0; }
    int set_frequency(double dtheta) { return set(theta, nco_constrain(dtheta)); }
    int adjust_frequency(double dt) { return set(theta, delta_theta + nco_constrain(dt)); }
    int set_phase(double phi) { return set(nco_constrain(phi), delta_theta); }
    int adjust_phase(double dphi) { return set(theta + nco_constrain(dphi), delta_theta); }
    // `steps` calls of NCO::step (:94-96); the product wraps mod 2^32 as the single adds would
    void advance(uint64_t steps) { theta += (uint32_t)(steps * delta_theta); }
    int get(uint32_t* t, uint32_t* dt) const {
        if (t) *t = theta;
        if (dt) *dt = delta_theta;
        return SDSP_OK;
    }
    int set(uint32_t t, uint32_t dt) {
        theta = t;
        delta_theta = dt;
        return SDSP_OK;
    }
};

// nco_sine_table() into `d` on the current device (runtime_rx.cpp)
hipError_t nco_upload_sine_table(DevBuf& d);

// What a decimating FIR is on the device, whoever feeds it: taps, delay line, decimation phase
// and the kernel choice.  sdsp_fir (runtime.cpp) adds the host step and overlap-save around it,
// sdsp_ddc (runtime_ddc.cpp) the oscillator; the members below (runtime.cpp) serve both alike.
struct FirCore : HandleCore {
    int dtype = 0;
    size_t L = 0, M = 1, channels = 1;
    std::vector<unsigned char> taps;   // original order (host copy for coefficients / design queries / clone)
    std::vector<unsigned char> scale;  // one Coef
    DevBuf d_taps_rev;                 // cr[i] = h[L-1-i]  (DotProduct REVERSE, dot_product/mod.rs:73-81)
    PingPong hist;                     // [channels][L-1] oldest first
    size_t ci = 0;                     // DecimatingFIRFilter::current_item (decim.rs:7)
    int algo = SDSP_ALGO_EXACT;        // reference-order kernel unless the caller opts in (sdsp.h)
    int decim_seg = 0;                 // outputs per lane group of the polyphase decimator (0 = auto)

    size_t state_len() const { return channels * (L - 1); }
    size_t hist_bytes() const { return state_len() * sample_bytes(dtype); }
    size_t j0() const { return (M - 1 - ci) % M; }  // first input index whose push wraps the phase to 0
    size_t output_count(size_t n) const {
        if (M == 1) return n;
        return j0() < n ? (n - 1 - j0()) / M + 1 : 0;
    }
    // AUTO on a decimating handle: the fused multiply-add kernels for long 32-bit blocks (n inputs)
    int decim_algo(size_t n) const {
        if (algo != SDSP_ALGO_AUTO) return algo;
        return dtype <= SDSP_CC32 && n >= (size_t)(1 << 16) ? SDSP_ALGO_FMA : SDSP_ALGO_EXACT;
    }
    // validated arguments -> taps and scale stored, the process default algorithm, the stream open
    // and the reversed taps on `device` (the current one); the state is not yet allocated
    hipError_t init(int dtype, const void* taps, size_t len, const void* scale, size_t M, int device);
    int zero_state();  // [channels][L-1] zeros in both halves, phase 0, nothing queued
    // the device halves of get_state / set_state: after quiesce(), the delay line to / from `host`
    // (nothing when it is null)
    int read_hist(void* host) const;
    int write_hist(const void* host);
    // `c`, freshly created from this handle's taps: algorithm, knob, channels, delay line and phase
    int copy_state_to(FirCore* c) const;
};

}  // namespace sdsp

// Polyphase filterbank / interpolating FIR handle (runtime.cpp).  Defined here because the
// up-converter (runtime_duc.cpp) and the resampler (runtime_resamp.cpp) are an interpolator handle
// plus their own registers, and launch their own kernels on its coefficients and window.
struct sdsp_pfb : sdsp::HandleCore {
    int dtype = 0;
    size_t M = 0, K = 0, channels = 1;
    bool interp = false;
    std::vector<unsigned char> cb;     // [M][K] branch coefficients, stored order
    std::vector<unsigned char> scale;  // kept, never applied (pfb.rs:85-90)
    sdsp::DevBuf d_cb;
    sdsp::PingPong hist;  // [channels][K] : the Window(K), oldest first
    int algo = SDSP_ALGO_EXACT;

    // One device block of n inputs and n_out outputs per channel on the caller's stream (or the
    // handle's): launch(stream) -> hipError_t queues the kernel that reads d_in and hist.front(),
    // then the window moves on by the n inputs.  `what` names the launch in an error.
    template <typename Launch>
    int block_device(const void* d_in, size_t n, void* d_out, size_t n_out, void* user_stream, const char* what,
                     Launch launch) {
        sdsp::DeviceGuard g(device);
        hipStream_t s = sdsp::pick(user_stream, stream);
        const size_t sb = sdsp::sample_bytes(dtype);
        if (sdsp::ranges_overlap(d_in, channels * n * sb, d_out, channels * n_out * sb)) {
            sdsp::set_error("input and output blocks overlap (in-place filtering is not supported)");
            return SDSP_E_INVALID_ARGUMENT;
        }
        // work queued on another stream (the fence) reads or writes the window this launch uses
        SDSP_TRY(fence.order_before(s), "order after queued work");
        SDSP_TRY(launch(s), what);
        SDSP_TRY(sdsp::launch_hist_update(dtype, d_in, hist.front(), hist.back(), n, (int)K, channels, s),
                 "window update");
        hist.flip();
        SDSP_TRY(fence.record(s), "record fence");
        return SDSP_OK;
    }
    // The host-slice twin: [channels][n] in and [channels][n_out] out through the staging buffers,
    // run(d_in, d_out, stream) being the device entry point
    template <typename Run> int block_host(const void* in, size_t n, void* out, size_t n_out, Run run) {
        sdsp::DeviceGuard g(device);
        const size_t sb = channels * sdsp::sample_bytes(dtype);
        return staged(in, n * sb, out, n_out * sb, run);
    }
};

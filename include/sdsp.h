/*
 * sdsp.h — C ABI of the MI355X-native streaming filter engine (libsdsp.so).
 *
 * Drop-in boundary for juliantos/solid-dsp's hot path.  Every entry point
 * replaces one method of the reference's Rust API; the reference item it
 * replaces is cited (paths relative to the reference checkout).  A Rust shim
 * crate keeps `solid::filter::*` / `solid::dot_product::*` and forwards to
 * these symbols (INTEGRATION.md shows the bindings).
 *
 * Conventions (mirroring the reference):
 *  - Construction copies taps into the handle (DotProduct::new, alloc_zeroed,
 *    src/dot_product/mod.rs:57-87) and can fail with the reference's error
 *    enums (FIRErrorCode src/filter/fir/mod.rs:40-45, IIRErrorCode
 *    src/filter/iir/mod.rs:41-49, SecondOrderErrorCode src/filter/iir/sos.rs:19-21),
 *    returned as sdsp_status codes.  Execution cannot fail except for device
 *    errors (>= SDSP_E_DEVICE); sdsp_last_error() gives the message.
 *  - Complex samples/taps are interleaved {re, im}, the #[repr(C)] layout of
 *    num::Complex<T>.
 *  - A handle is bound to one device and owns: the tap copy, the delay-line
 *    state (the reference's `Window`, src/window/mod.rs:9-77) resident in HBM,
 *    one hipStream_t and device staging buffers.  A handle is not thread safe
 *    (the reference types are !Send); distinct handles may run concurrently.
 *  - `*_execute_block` takes HOST slices (like `&[In] -> Vec<Out>`) and is
 *    PCIe-bound; `*_execute_block_device` takes device pointers (HBM resident)
 *    and a hipStream_t and is asynchronous.  NULL = the handle's own stream;
 *    the legacy null stream is passed as hipStreamLegacy ((void*)1).  Calls on
 *    one handle must be stream-ordered (the delay line is updated in HBM at
 *    the end of every call).
 *  - No CPU fallback: with no usable gfx950 device every create call returns
 *    SDSP_E_NO_DEVICE.
 *  - Streaming calls do not filter in place: an input block that overlaps its
 *    output block is rejected with SDSP_E_INVALID_ARGUMENT (the kernels read
 *    each input window, and the delay-line update reads the block's tail, after
 *    other workgroups have started writing outputs).
 *  - Host-side state calls (reset, get/set_state, clone, set_scale) first wait
 *    for the work an earlier *_execute_block_device queued on a caller stream.
 */
#ifndef SDSP_H
#define SDSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDSP_API __attribute__((visibility("default")))

/* (Coef, In) pairs.  Out = Coef * In (num-complex Mul). */
typedef enum {
    SDSP_RR32 = 0, /* f32  taps, f32  samples                                  */
    SDSP_RC32 = 1, /* f32  taps, c32  samples ("crcf")                         */
    SDSP_CC32 = 2, /* c32  taps, c32  samples ("cccf")                         */
    SDSP_RR64 = 3, /* f64  taps, f64  samples (the reference Filter path)      */
    SDSP_RC64 = 4, /* f64  taps, c64  samples (FIRFilter<f64, Complex<f64>>)   */
    SDSP_CC64 = 5  /* c64  taps, c64  samples                                  */
} sdsp_dtype;

/* Kernel selection for FIR-type and IIR handles.  A new handle uses SDSP_ALGO_EXACT:
 * by default every result is bit-identical to the reference algorithm at the handle's
 * precision, whatever the block size.  The fast kernels are opt-in. */
typedef enum {
    SDSP_ALGO_AUTO = 0,  /* FFT overlap-save for 32-bit complex blocks >= 65536 samples (taps up to
                            2^20 + 1, no decimation), else EXACT */
    SDSP_ALGO_EXACT = 1, /* direct form in the reference summation order, no FMA contraction:
                            bit-identical to the reference algorithm at the handle's precision */
    SDSP_ALGO_FMA = 2,   /* direct form, same order, fused multiply-add                      */
    SDSP_ALGO_FFT = 3    /* overlap-save fast convolution, no decimation.  Up to 3841 taps: N = 4096 in
                            LDS, 32-bit complex samples, and real f32 samples with real f32 taps (two
                            real segments per transform).  3842 to 2^20 + 1 taps, 32-bit complex
                            samples: one N-point transform per segment in three passes, N the power
                            of two >= 4 (len - 1) and >= 2^14 (sdsp_fir_ols_info) */
} sdsp_algo;

typedef enum {
    SDSP_OK = 0,
    /* FIRErrorCode (src/filter/fir/mod.rs:40-45) */
    SDSP_E_COEFFICIENTS_LENGTH_ZERO = 1,
    SDSP_E_DECIMATION_LESS_THAN_ONE = 2,
    SDSP_E_INTERPOLATION_LESS_THAN_ONE = 3,
    SDSP_E_NOT_ENOUGH_FILTERS = 4,
    /* IIRErrorCode (src/filter/iir/mod.rs:41-49) */
    SDSP_E_NUMERATOR_LENGTH_ZERO = 10,
    SDSP_E_DENOMINATOR_LENGTH_ZERO = 11,
    SDSP_E_SOS_SIZE_ZERO = 12,
    SDSP_E_SOS_SIZE_MISMATCH = 13,
    SDSP_E_SOS_SIZE_NOT_MULTIPLE_OF_3 = 14,
    SDSP_E_IIR_DECIMATION_LESS_THAN_ONE = 15,
    SDSP_E_IIR_INTERPOLATION_LESS_THAN_ONE = 16,
    /* SecondOrderErrorCode (src/filter/iir/sos.rs:19-21) */
    SDSP_E_SOS_COEFFICIENTS_NOT_IN_RANGE = 20,
    /* NCOErrorCode (src/nco/mod.rs:7-10) */
    SDSP_E_NCO_BANDWIDTH_OUT_OF_RANGE = 30,
    /* AGCErrorCode (src/auto_gain_control/mod.rs:49-56) */
    SDSP_E_AGC_BANDWIDTH_OUT_OF_RANGE = 40,
    SDSP_E_AGC_SIGNAL_LEVEL_OUT_OF_RANGE = 41,
    SDSP_E_AGC_GAIN_BELOW_THRESHOLD = 42,
    SDSP_E_AGC_SCALE_BELOW_THRESHOLD = 43,
    SDSP_E_AGC_SAMPLES_TOO_LOW = 44,
    /* argument errors the reference reports by panicking */
    SDSP_E_INVALID_ARGUMENT = 90,
    SDSP_E_UNSUPPORTED = 91,
    /* device errors */
    SDSP_E_DEVICE = 100,
    SDSP_E_NO_DEVICE = 101,
    SDSP_E_OUT_OF_MEMORY = 102
} sdsp_status;

SDSP_API const char* sdsp_last_error(void);
SDSP_API const char* sdsp_version(void);
/* number of visible gfx950 devices (0 when none) */
SDSP_API int sdsp_device_count(void);
/* bytes of one sample / one tap of a dtype */
SDSP_API size_t sdsp_sample_size(int dtype);
SDSP_API size_t sdsp_coef_size(int dtype);

/* ------------------------------------------------------------------------
 * FIR and decimating FIR  (FIRFilter src/filter/fir/mod.rs:58-304,
 *                          DecimatingFIRFilter src/filter/fir/decim.rs:5-281)
 * A FIR handle is a DecimatingFIRFilter with decimation 1.  `channels`
 * independent delay lines share the taps; device/host buffers are
 * channel-major: sample i of channel c at [c * n + i].
 * ------------------------------------------------------------------------ */
typedef struct sdsp_fir sdsp_fir;

/* FIRFilter::new(&[Coef], scale)                    src/filter/fir/mod.rs:79-88 */
SDSP_API int sdsp_fir_create(sdsp_fir** out, int dtype, const void* taps, size_t len,
                             const void* scale, int device);
/* DecimatingFIRFilter::new(&[Coef], scale, M)       src/filter/fir/decim.rs:27-42 */
SDSP_API int sdsp_decim_create(sdsp_fir** out, int dtype, const void* taps, size_t len,
                               const void* scale, size_t decimation, int device);
/* channel count (default 1); resets the delay lines */
SDSP_API int sdsp_fir_set_channels(sdsp_fir* h, size_t channels);
/* SDSP_ALGO_FFT on a handle it does not cover (64-bit dtypes, decimators, real f32 samples with
 * more than 3841 taps, more than 2^20 + 1 taps) fails with SDSP_E_UNSUPPORTED; every block of a
 * handle set to it takes the overlap-save path, whatever its length */
SDSP_API int sdsp_fir_set_algo(sdsp_fir* h, int algo);
SDSP_API int sdsp_fir_get_algo(const sdsp_fir* h); /* resolved algorithm */
/* Process-wide starting algorithm of handles created afterwards (sdsp_fir_create,
 * sdsp_decim_create, the sdsp_iir_* / sdsp_sos_create family; PFB / interpolator handles take FMA
 * when it is FMA, else EXACT): SDSP_ALGO_EXACT (the default: every result bit-identical to the
 * reference), SDSP_ALGO_AUTO (blocks of >= 65536 32-bit complex samples on the overlap-save FIR,
 * >= 65536 32-bit inputs on the FMA decimator, IIR blocks of >= 8192 samples on the scans where
 * the cascade admits one; everything shorter on the reference order) or SDSP_ALGO_FMA.  Read from
 * the environment variable SDSP_DEFAULT_ALGO ("auto" / "exact" / "fma") at the first handle or
 * query unless set here first.  Not part of the reference API: it lets a deployment move an
 * unchanged caller of that API onto the fast paths.  Existing handles keep their algorithm. */
SDSP_API int sdsp_set_default_algo(int algo);
SDSP_API int sdsp_get_default_algo(void);
/* kernel-variant knobs: performance only, every accepted value computes the complete output
 * (retired keys of earlier builds are rejected with SDSP_E_INVALID_ARGUMENT). */
typedef enum {
    SDSP_TUNE_DECIM_SEG = 6,     /* FMA decimator: outputs per lane group (0 = automatic) */
    SDSP_TUNE_IIR_WAVE_SCAN = 7, /* IIR scan kernel: 0 = block scan, 1 = wave scan with 256-byte chunks (default
                                    for complex and f64 samples), 2 = 128-byte chunks (default for real f32),
                                    3/4 = paired 128/64-byte chunks (real f32), 5 = 256-byte chunks rerun
                                    instead of corrected, 6 = 128-byte chunks without the register prefetch */
    SDSP_TUNE_CHAN_STREAMING = 8, /* channeliser: streaming M=1024 kernel where it applies: 3 = 1024-thread
                                     workgroups, sixteen frames per round, the next round's samples
                                     requested before this round's stores; 1 = the same without; 2 / 4 =
                                     512-thread workgroups without / with that prefetch; 5 (default) / 6 =
                                     as 3 with eight / four frames per round (waves 0..7 / 0..3 transform);
                                     0 = per-frame kernel */
    SDSP_TUNE_CHAN_FRAMES_PER_BLOCK = 9, /* streaming channeliser: frames per workgroup (0 = automatic, 64..256) */
    SDSP_TUNE_OLS_KERNEL = 14,   /* overlap-save segments (16-byte aligned rows): 0 (default) one-shot
                                    XCD-ordered kernels: the interior segments in one launch (one halo row
                                    compiled in when L <= 257), the boundary segments and the next history
                                    in a second,
                                    1 persistent packed kernel for the interior segments (L <= 1025),
                                    2 scalar kernel, 3 the one-shot kernel with 16-byte lanes.
                                    Real f32 handles: 0 (default, and every value but 3) 4-byte lanes,
                                    3 8-byte lanes (8-byte aligned rows, else as 0) */
    SDSP_TUNE_CHAN_XCD_ORDER = 15, /* streaming channeliser: 1 (default) = each XCD walks a contiguous
                                     eighth of the frame chunks, 0 = launch order */
    SDSP_TUNE_HOST_STEP = 16,     /* FIR / decimator: 1 (default) = execute(sample), push and host blocks with
                                     n * len <= SDSP_TUNE_HOST_BLOCK_MACS run on the host against the
                                     handle's delay line (single-channel handles, not the FFT algorithm;
                                     reference arithmetic, bit-identical to the EXACT/FMA kernels);
                                     0 = every call launches device work (one-sample step kernel) */
    SDSP_TUNE_HOST_BLOCK_MACS = 17, /* host-block threshold in multiply-adds (default 65536) */
    SDSP_TUNE_FFT_GROUP = 18,      /* four-step passes on the generic pass kernel: at most this many
                                      transforms per workgroup (1..64, default 4) */
    SDSP_TUNE_FFT_WAVE1024 = 19,   /* four-step passes of 1024 points (c32): 16 (default) pipelined persistent
                                      wave-FFT kernel, 1 / 8 one-shot with 16 / 8 transforms per workgroup,
                                      0 the generic pass kernel */
    SDSP_TUNE_ACORR_KERNEL = 20,   /* AutoCorrelator: 0 (default) pipelined kernel on interior tiles (delay
                                      and window <= 128), one-shot kernel elsewhere; 1 the one-shot kernel
                                      everywhere, delayed input staged in LDS (delay <= 256); 2 the one-shot
                                      kernel with two loads per product */
    SDSP_TUNE_AGC_KERNEL = 21,     /* AGC bank: 0 (default) pipelined kernel for calls < 2^22 samples per
                                      channel, 1 the plain per-sample kernel */
    SDSP_TUNE_OLS_LONG_LOG2N = 22, /* overlap-save with more than 3841 taps: log2 of the segment transform
                                      size N, 13..22 with N >= 2 (len - 1); 0 (default) = the smallest
                                      power of two >= 4 (len - 1) and >= 2^14.  Other handles accept 0 only */
    SDSP_TUNE_OLS_LONG_SEGS = 23,  /* the same path: segments per round of its three passes, 1..4096;
                                      0 (default) = what 256 MiB of scratch hold */
    SDSP_TUNE_RESAMP_KERNEL = 24,  /* rational resampler: 0 (default) automatic, 1 staged kernel, 2 one lane
                                      per output, 3 branch-stationary lanes; a value whose kernel does not
                                      apply to the handle's shape runs the automatic choice (sdsp_resamp_info) */
    SDSP_TUNE_ICHAN_KERNEL = 25,   /* synthesis channeliser: 0 (default) automatic, 1 per-frame kernel, 2 ring
                                      kernel (transformed frames kept in LDS); a value whose kernel does not
                                      fit the handle's shape runs the automatic choice (sdsp_ichan_info) */
    SDSP_TUNE_ICHAN_FRAMES_PER_BLOCK = 26, /* synthesis channeliser, ring kernel: frames per workgroup, any
                                      value >= 1 (below K-1 too); 0 (default) = automatic */
    SDSP_TUNE_OSCHAN_KERNEL = 27,  /* oversampled channeliser: 0 (default) automatic, 1 per-frame kernel, 2
                                      sliding kernel (the stream's window kept in LDS); a value whose kernel
                                      does not fit the handle's shape runs the automatic choice
                                      (sdsp_oschan_info) */
    SDSP_TUNE_OSCHAN_FRAMES_PER_BLOCK = 28, /* oversampled channeliser, sliding kernel: frames per workgroup,
                                      any value >= 1; 0 (default) = automatic */
    SDSP_TUNE_ARB_KERNEL = 29,     /* arbitrary-rate resampler: 0 (default) automatic, 1 staged kernel, 2 one
                                      lane per output; a value whose kernel does not apply to the handle's
                                      shape and step runs the automatic choice (sdsp_arb_info) */
    SDSP_TUNE_ACORR_SLOTS = 30,    /* AutoCorrelator, pipelined kernel: at most this many persistent waves
                                      per channel (1..65536, rounded up to whole eights, one per XCD);
                                      0 (default) = what the device holds resident.  Same results: fewer
                                      waves walk more tiles each */
    SDSP_TUNE_SPEC_KERNEL = 31,    /* spectrometer: 0 (default) automatic, 1 per-frame kernel, 2 sliding
                                      kernel (the stream's window kept in LDS); a value whose kernel does
                                      not fit the handle's shape runs the automatic choice (sdsp_spec_info) */
    SDSP_TUNE_SPEC_SUBBLOCKS = 32  /* spectrometer: sub-blocks (of up to 32 frames) per workgroup, any
                                      value >= 1; 0 (default) = automatic */
} sdsp_tune_key;
SDSP_API int sdsp_fir_set_tuning(sdsp_fir* h, int key, int value);
SDSP_API void sdsp_fir_destroy(sdsp_fir* h);        /* Drop */
/* Clone (derive(Clone), fir/mod.rs:58): same taps and a snapshot of the delay line */
SDSP_API int sdsp_fir_clone(const sdsp_fir* h, sdsp_fir** out);
/* set_scale / get_scale                              fir/mod.rs:103-124, decim.rs:57-78 */
SDSP_API int sdsp_fir_set_scale(sdsp_fir* h, const void* scale);
SDSP_API int sdsp_fir_get_scale(const sdsp_fir* h, void* scale);
/* segment transform size and outputs per segment that SDSP_ALGO_FFT would use on this handle
 * (no reference counterpart): 4096 and 4096 - 256 ceil((len - 1) / 256) up to 3841 taps, N and
 * N - (len - 1) above (SDSP_TUNE_OLS_LONG_LOG2N), both 0 where overlap-save does not apply */
SDSP_API int sdsp_fir_ols_info(const sdsp_fir* h, size_t* nfft, size_t* valid);
/* len (fir/mod.rs:139-142), get_decimation (decim.rs:92-95) */
SDSP_API size_t sdsp_fir_len(const sdsp_fir* h);
SDSP_API size_t sdsp_fir_decimation(const sdsp_fir* h);
/* coefficients(): the stored (REVERSED) taps, as DotProduct::coefficents (fir/mod.rs:173-176) */
SDSP_API int sdsp_fir_coefficients(const sdsp_fir* h, void* out_len_taps);
/* number of outputs a block of n inputs produces from the current phase */
SDSP_API size_t sdsp_fir_output_count(const sdsp_fir* h, size_t n);
/* Filter::execute(sample) -> Vec<Out> (0 or 1 outputs)  fir/mod.rs:209-212, decim.rs:221-228
 * (single channel handles only) *n_out = 0/1 */
SDSP_API int sdsp_fir_execute(sdsp_fir* h, const void* sample, void* out, size_t* n_out);
/* Filter::execute_block(&[In]) -> Vec<Out>          fir/mod.rs:235-241, decim.rs:250-256
 * in: channels*n host samples; out: channels*output_count(n) host samples */
SDSP_API int sdsp_fir_execute_block(sdsp_fir* h, const void* in, size_t n, void* out, size_t* n_out);
/* device-resident variant (asynchronous on `stream`; NULL = handle stream) */
SDSP_API int sdsp_fir_execute_block_device(sdsp_fir* h, const void* d_in, size_t n, void* d_out,
                                           size_t* n_out, void* stream);
/* DecimatingFIRFilter::push / write (advance phase, no output)  decim.rs:115-118, 136-139 */
SDSP_API int sdsp_decim_push(sdsp_fir* h, const void* sample);
SDSP_API int sdsp_decim_write(sdsp_fir* h, const void* samples, size_t n);
/* reset: zero the delay lines and the phase (Window::reset, src/window/mod.rs:54-56) */
SDSP_API int sdsp_fir_reset(sdsp_fir* h);
/* delay-line state: the last len-1 inputs per channel, oldest first (+ the phase) */
SDSP_API size_t sdsp_fir_state_len(const sdsp_fir* h);
SDSP_API int sdsp_fir_get_state(const sdsp_fir* h, void* hist, size_t* phase);
SDSP_API int sdsp_fir_set_state(sdsp_fir* h, const void* hist, size_t phase);
/* Filter::frequency_response / group_delay (host f64)   fir/mod.rs:263-303 */
SDSP_API int sdsp_fir_frequency_response(const sdsp_fir* h, double f, double* re_im);
SDSP_API int sdsp_fir_group_delay(const sdsp_fir* h, double f, double* delay);
SDSP_API int sdsp_fir_synchronize(sdsp_fir* h);
/* diagnostic (no reference counterpart): how many calls on this handle queued device work or moved
   its delay line between host and device (kernel launches, async copies, history pulls / flushes);
   per-sample calls on the host step leave it unchanged */
SDSP_API unsigned long long sdsp_fir_device_ops(const sdsp_fir* h);

/* ------------------------------------------------------------------------
 * Polyphase filterbank and interpolating FIR
 *  (PolyPhaseFilterBank src/filter/fir/pfb.rs:3-91,
 *   InterpolatingFIRFilter src/filter/fir/interp.rs:6-138)
 * ------------------------------------------------------------------------ */
typedef struct sdsp_pfb sdsp_pfb;

/* PolyPhaseFilterBank::new(&[Coef], filters, scale)  pfb.rs:24-49 */
SDSP_API int sdsp_pfb_create(sdsp_pfb** out, int dtype, const void* taps, size_t len, size_t filters,
                             const void* scale, int device);
/* InterpolatingFIRFilter::new(&[Coef], M)            interp.rs:27-54 */
SDSP_API int sdsp_interp_create(sdsp_pfb** out, int dtype, const void* taps, size_t len,
                                size_t interpolation, int device);
SDSP_API void sdsp_pfb_destroy(sdsp_pfb* h);
SDSP_API int sdsp_pfb_clone(const sdsp_pfb* h, sdsp_pfb** out);
SDSP_API size_t sdsp_pfb_len(const sdsp_pfb* h);          /* number of filters M */
SDSP_API size_t sdsp_pfb_subfilter_len(const sdsp_pfb* h); /* K */
SDSP_API int sdsp_pfb_set_scale(sdsp_pfb* h, const void* scale);
SDSP_API int sdsp_pfb_get_scale(const sdsp_pfb* h, void* scale);
/* coefficents(): M x K branch coefficients (stored order) */
SDSP_API int sdsp_pfb_coefficients(const sdsp_pfb* h, void* out_mk);
/* push(sample)  pfb.rs:81-83 */
SDSP_API int sdsp_pfb_push(sdsp_pfb* h, const void* sample);
/* execute(index) on the current window  pfb.rs:85-90 */
SDSP_API int sdsp_pfb_execute(sdsp_pfb* h, size_t index, void* out);
/* reset  pfb.rs:77-79 */
SDSP_API int sdsp_pfb_reset(sdsp_pfb* h);
/* dot-product order: SDSP_ALGO_EXACT (default, the reference's sequential sum,
 * bit-identical) or SDSP_ALGO_FMA (fused multiply-add, same order) */
SDSP_API int sdsp_pfb_set_algo(sdsp_pfb* h, int algo);
/* independent channels in one handle: blocks are channel-major [channels][n]
 * in, [channels][n*M] out; resets every channel's window */
SDSP_API int sdsp_pfb_set_channels(sdsp_pfb* h, size_t channels);
/* for each input: push, then all M branch outputs -> out[n*M]
 * (InterpolatingFIRFilter::execute_block  interp.rs:102-111).  The _device form
 * rejects overlapping input and output blocks (SDSP_E_INVALID_ARGUMENT). */
SDSP_API int sdsp_pfb_execute_block(sdsp_pfb* h, const void* in, size_t n, void* out);
SDSP_API int sdsp_pfb_execute_block_device(sdsp_pfb* h, const void* d_in, size_t n, void* d_out, void* stream);
SDSP_API int sdsp_pfb_frequency_response(const sdsp_pfb* h, double f, double* re_im);
SDSP_API int sdsp_pfb_group_delay(const sdsp_pfb* h, double f, double* delay);
SDSP_API int sdsp_pfb_synchronize(sdsp_pfb* h);

/* ------------------------------------------------------------------------
 * IIR family  (IIRFilter src/filter/iir/mod.rs:62-414, SecondOrderFilter
 *  src/filter/iir/sos.rs:34-231, DecimatingIIRFilter src/filter/iir/decim.rs:5-280,
 *  InterpolatingIIRFilter src/filter/iir/interp.rs:6-268).
 * dtype: SDSP_RR32, SDSP_RC32, SDSP_RR64, SDSP_RC64 (real coefficients, like
 * the reference's Conj + Real bound).  type: 0 = Normal, 1 = SecondOrder.
 * algo: SDSP_ALGO_EXACT = reference-order serial recurrence (one lane per
 * channel, bit-identical); SDSP_ALGO_FMA = block-parallel scan (stable SOS
 * cascades); SDSP_ALGO_AUTO = scan for long blocks when the cascade admits it.
 * ------------------------------------------------------------------------ */
typedef struct sdsp_iir sdsp_iir;

/* IIRFilter::new(&ff, &fb, IIRFilterType)            mod.rs:92-164 */
SDSP_API int sdsp_iir_create(sdsp_iir** out, int dtype, const void* ff, size_t nff, const void* fb, size_t nfb,
                             int type, int device);
/* DecimatingIIRFilter::new(&ff, &fb, type, M)         decim.rs:11-30 */
SDSP_API int sdsp_iir_decim_create(sdsp_iir** out, int dtype, const void* ff, size_t nff, const void* fb,
                                   size_t nfb, int type, size_t decimation, int device);
/* InterpolatingIIRFilter::new(&ff, &fb, type, M)      interp.rs:12-31 */
SDSP_API int sdsp_iir_interp_create(sdsp_iir** out, int dtype, const void* ff, size_t nff, const void* fb,
                                    size_t nfb, int type, size_t interpolation, int device);
/* SecondOrderFilter::new(&ff, &fb) (f64)              sos.rs:55-75 */
SDSP_API int sdsp_sos_create(sdsp_iir** out, const double* ff, size_t nff, const double* fb, size_t nfb,
                             int device);
SDSP_API void sdsp_iir_destroy(sdsp_iir* h);
SDSP_API int sdsp_iir_clone(const sdsp_iir* h, sdsp_iir** out);
SDSP_API int sdsp_iir_set_channels(sdsp_iir* h, size_t channels);
SDSP_API int sdsp_iir_set_algo(sdsp_iir* h, int algo);
/* kernel-variant knob (SDSP_TUNE_IIR_WAVE_SCAN; performance only) */
SDSP_API int sdsp_iir_set_tuning(sdsp_iir* h, int key, int value);
/* scan plan of section group g: warm-up chunks (0 = scan not admissible) and chunk length */
SDSP_API int sdsp_iir_scan_info(const sdsp_iir* h, int group, int* warmup_chunks, int* chunk);
/* the wave scan a cascade group gets when the scan is requested: 0 none (serial recurrence),
 * 1 warm-up chunks (decaying state response), 2 exact inter-wave carries (non-decaying but
 * well conditioned: aggregate pass + carry scan + output pass); -1 bad handle/group */
SDSP_API int sdsp_iir_wscan_mode(const sdsp_iir* h, int group);
SDSP_API size_t sdsp_iir_output_count(const sdsp_iir* h, size_t n);
/* Filter::execute / execute_block                     mod.rs:270-316, decim.rs:203-225, interp.rs:197-214 */
SDSP_API int sdsp_iir_execute(sdsp_iir* h, const void* sample, void* out, size_t* n_out);
SDSP_API int sdsp_iir_execute_block(sdsp_iir* h, const void* in, size_t n, void* out, size_t* n_out);
SDSP_API int sdsp_iir_execute_block_device(sdsp_iir* h, const void* d_in, size_t n, void* d_out, size_t* n_out,
                                           void* stream);
SDSP_API int sdsp_iir_reset(sdsp_iir* h);
/* state: SOS (w1, w2) per section per channel; Normal the last cap-1 w values, newest first */
SDSP_API size_t sdsp_iir_state_len(const sdsp_iir* h);
SDSP_API int sdsp_iir_get_state(const sdsp_iir* h, void* state, size_t* phase);
SDSP_API int sdsp_iir_set_state(sdsp_iir* h, const void* state, size_t phase);
/* numerator_coefs() / denominator_coefs() as stored (mod.rs:123-127,156-157); which: 0 num, 1 den */
SDSP_API size_t sdsp_iir_num_coefs(const sdsp_iir* h, int which);
SDSP_API int sdsp_iir_coefficients(const sdsp_iir* h, double* num, double* den);
/* SecondOrderFilter numerator_coefs (a[1..]/a0) and denominator_coefs (b/a0) of one section */
SDSP_API int sdsp_sos_section_coefs(const sdsp_iir* h, int section, double* num2, double* den3);
/* Filter::frequency_response / group_delay (host f64)  mod.rs:336-413 */
SDSP_API int sdsp_iir_frequency_response(const sdsp_iir* h, double f, double* re_im);
SDSP_API int sdsp_iir_group_delay(const sdsp_iir* h, double f, double* delay);
SDSP_API int sdsp_iir_synchronize(sdsp_iir* h);

/* ------------------------------------------------------------------------
 * FFT  (FFT::new / FFT::execute, src/fft/mod.rs:175-215).  direction: 0 FORWARD,
 * 1 REVERSE (unnormalised, like the reference).  precision: 0 = complex f32,
 * 1 = complex f64.  Sizes 1 .. 2^23 and the power of two 2^24;
 * any other size fails with SDSP_E_INVALID_ARGUMENT: a size that is no power of
 * two convolves at the power of two >= 2 nfft - 1, at most 2^24.  Power-of-two sizes up to 4096 run a radix-4 Stockham FFT in LDS, larger
 * powers of two a four-step FFT (two strided LDS passes, f64 inter-pass twiddles);
 * other sizes up to 512 a direct DFT, larger ones Bluestein's chirp-z transform
 * over a power-of-two convolution (where the reference plans Rader / mixed radix,
 * src/fft/mod.rs:123-170; the results agree within the transforms' rounding).
 * ------------------------------------------------------------------------ */
typedef struct sdsp_fft sdsp_fft;
SDSP_API int sdsp_fft_create(sdsp_fft** out, size_t nfft, int direction, int precision, int device);
SDSP_API void sdsp_fft_destroy(sdsp_fft* h);
SDSP_API size_t sdsp_fft_len(const sdsp_fft* h);
/* device plan: 0 direct DFT, 1 power of two in LDS, 2 Bluestein, 3 four-step power of two */
SDSP_API int sdsp_fft_method(const sdsp_fft* h);
/* kernel-variant knobs: SDSP_TUNE_FFT_GROUP, SDSP_TUNE_FFT_WAVE1024 (performance only) */
SDSP_API int sdsp_fft_set_tuning(sdsp_fft* h, int key, int value);
/* `batch` contiguous transforms of nfft complex samples */
SDSP_API int sdsp_fft_execute(sdsp_fft* h, const void* in, void* out, size_t batch);
SDSP_API int sdsp_fft_execute_device(sdsp_fft* h, const void* d_in, void* d_out, size_t batch, void* stream);

/* ------------------------------------------------------------------------
 * PFB + FFT channeliser (build-defined composition of PolyPhaseFilterBank's
 * coefficient layout, src/filter/fir/pfb.rs:24-49, and FFT FORWARD; SURVEY
 * Appendix A.6).  M channels (power of two, 4..4096), K = len / M taps per
 * branch, branch p fed by input phase M-1-p.  dtype SDSP_RC32 or SDSP_RC64.
 * Blocks are whole frames: n (per stream) a multiple of M; out[s][frame][M].
 * sdsp_chan_create refuses, in this order and before any device work: a null
 * `out`, another dtype (SDSP_E_UNSUPPORTED), a null `taps` with len > 0
 * (SDSP_E_INVALID_ARGUMENT), channels = 0, len = 0, a channel count that is no
 * power of two in 4..4096 (SDSP_E_UNSUPPORTED), len < channels; then a missing
 * device.  sdsp_ichan_create, sdsp_oschan_create and sdsp_spec_create check in the same order.
 * ------------------------------------------------------------------------ */
typedef struct sdsp_chan sdsp_chan;
SDSP_API int sdsp_chan_create(sdsp_chan** out, int dtype, const void* taps, size_t len, size_t channels,
                              int device);
SDSP_API void sdsp_chan_destroy(sdsp_chan* h);
SDSP_API int sdsp_chan_set_streams(sdsp_chan* h, size_t streams);
/* kernel-variant knobs: SDSP_TUNE_CHAN_STREAMING, SDSP_TUNE_CHAN_FRAMES_PER_BLOCK,
 * SDSP_TUNE_CHAN_XCD_ORDER (performance only) */
SDSP_API int sdsp_chan_set_tuning(sdsp_chan* h, int key, int value);
SDSP_API int sdsp_chan_reset(sdsp_chan* h);
SDSP_API int sdsp_chan_execute_block(sdsp_chan* h, const void* in, size_t n, void* out, size_t* frames);
SDSP_API int sdsp_chan_execute_block_device(sdsp_chan* h, const void* d_in, size_t n, void* d_out,
                                            size_t* frames, void* stream);
SDSP_API int sdsp_chan_synchronize(sdsp_chan* h);

/* ------------------------------------------------------------------------
 * Synthesis ("inverse") channeliser: the counterpart of sdsp_chan, M baseband
 * channels back into one wideband stream (build-defined; the inverse FFT fused
 * into the polyphase bank).  Taps g are real, len >= M, K = len / M (later taps
 * are ignored, as in sdsp_chan_create); cb[r][i] = g[r + (K-1-i) M] is the
 * analysis channeliser's own branch table.  M a power of two, 4..4096; dtype
 * SDSP_RC32 or SDSP_RC64.  Per stream the input is whole frames X[m][0..M) in the
 * layout sdsp_chan_execute_block writes, [streams][frames][M] (n = frames * M
 * samples per stream), the output n time samples, [streams][n]:
 *
 *     u[m]       = REVERSE_FFT_M(X[m])                 (e^{+j 2 pi k q / M}, unnormalised)
 *     y[m M + r] = sum_{i<K} cb[r][i] * u[m-i][M-1-r]  r = 0 .. M-1
 *
 * Frames before the handle's first are zero.  Fed by an sdsp_chan built from
 * taps h (branch depth K_h), a handle built from g (depth K_g) gives, in exact
 * arithmetic,
 *
 *     y[m M + r] = M sum_{i<K_g} sum_{j<K_h} g[r + (K_g-1-i) M] h[(M-1-r) + (K_h-1-j) M] x[(m-i-j) M + r]
 *
 * (K = 1 and all-ones taps on both sides: y = M x).  One definition of the
 * arithmetic: the transform is the one sdsp_fft REVERSE runs up to 4096 points,
 * the branch sum starts from zero and runs i = 0 .. K-1, each step acc + c * v
 * with a rounded multiply and a rounded add; every kernel gives the same bits.
 * State: the last K-1 input frames per stream, zero after create, reset and
 * set_streams.  Blocks as sdsp_chan_execute_block[_device]: n a multiple of M,
 * n = 0 a no-op, no overlap of input and output.
 * ------------------------------------------------------------------------ */
typedef struct sdsp_ichan sdsp_ichan;
SDSP_API int sdsp_ichan_create(sdsp_ichan** out, int dtype, const void* taps, size_t len, size_t channels,
                               int device);
SDSP_API void sdsp_ichan_destroy(sdsp_ichan* h);
SDSP_API int sdsp_ichan_set_streams(sdsp_ichan* h, size_t streams);
/* kernel-variant knobs: SDSP_TUNE_ICHAN_KERNEL, SDSP_TUNE_ICHAN_FRAMES_PER_BLOCK (performance only) */
SDSP_API int sdsp_ichan_set_tuning(sdsp_ichan* h, int key, int value);
SDSP_API int sdsp_ichan_reset(sdsp_ichan* h);
SDSP_API size_t sdsp_ichan_channels(const sdsp_ichan* h);      /* M */
SDSP_API size_t sdsp_ichan_subfilter_len(const sdsp_ichan* h); /* K */
SDSP_API int sdsp_ichan_execute_block(sdsp_ichan* h, const void* in, size_t n, void* out, size_t* frames);
SDSP_API int sdsp_ichan_execute_block_device(sdsp_ichan* h, const void* d_in, size_t n, void* d_out,
                                             size_t* frames, void* stream);
/* what the next call runs: *kernel = 1 per-frame, 2 ring; *frames_per_block = the ring kernel's frames
 * per workgroup on a long block (an automatic value shrinks on blocks too short to fill the device
 * at it), 1 on the per-frame kernel.  Either pointer may be null */
SDSP_API int sdsp_ichan_info(const sdsp_ichan* h, int* kernel, size_t* frames_per_block);
SDSP_API int sdsp_ichan_synchronize(sdsp_ichan* h);

/* ------------------------------------------------------------------------
 * Oversampled analysis channeliser: M channels, one frame every D <= M samples
 * (build-defined; sdsp_chan is the critically sampled case D = M).  Taps h are
 * real, len >= M, K = len / M (later taps are ignored, as in sdsp_chan_create);
 * cb[p][i] = h[p + (K-1-i) M] is the channeliser's own branch table.  M a power
 * of two, 4..4096; 1 <= decimation D <= M; dtype SDSP_RC32 or SDSP_RC64.  Per
 * stream, with x[<0] = 0 and m the frame index since create / reset /
 * set_streams (64-bit, carried across calls):
 *
 *     v_p[m] = sum_{i<K} cb[p][i] * x[(m+1) D - 1 - p - i M]      p = 0 .. M-1
 *     w_q[m] = v_{(q + (m+1) D) mod M}[m]                  (an index rotation, no arithmetic)
 *     Y[m]   = FORWARD_FFT_M(w[m])                         (unnormalised)
 *
 * - D = M is sdsp_chan: the rotation is 0 and the index is (m-i) M + (M-1-p).
 * - Every channel is a plain down-converter: with g[p + i M] = h[p + (K-1-i) M],
 *       Y[m][k] = (g * (x[n] e^{+j 2 pi k (n+1) / M}))[(m+1) D - 1],
 *   a mix, a filter and a decimation by D with a phase-continuous oscillator.
 *   The rotation buys this: without it the output is a sliding STFT whose
 *   channel k turns by e^{-j 2 pi k (m+1) D / M} from frame to frame.
 * - It is an index rotation, not a multiply by a twiddle (which would change
 *   the bits and cost a rounding).
 *
 * One definition of the arithmetic: the branch sum starts from zero and runs
 * i = 0 .. K-1, each step acc + c * v with a rounded multiply and a rounded add;
 * the transform is the one sdsp_fft FORWARD runs up to 4096 points; every
 * kernel, at every frames-per-workgroup value and every call split, gives the
 * same bits.  Blocks: n (per stream) a multiple of D gives frames = n / D
 * frames, out[s][frame][M] (n M / D samples per stream); n = 0 is a no-op;
 * input and output may not overlap.  State: the last K M - D input samples per
 * stream and the frame counter (sdsp_oschan_phase); both zero after create,
 * reset and set_streams; a refused call changes neither.
 * ------------------------------------------------------------------------ */
typedef struct sdsp_oschan sdsp_oschan;
SDSP_API int sdsp_oschan_create(sdsp_oschan** out, int dtype, const void* taps, size_t len, size_t channels,
                                size_t decimation, int device);
SDSP_API void sdsp_oschan_destroy(sdsp_oschan* h);
SDSP_API int sdsp_oschan_set_streams(sdsp_oschan* h, size_t streams);
/* kernel-variant knobs: SDSP_TUNE_OSCHAN_KERNEL, SDSP_TUNE_OSCHAN_FRAMES_PER_BLOCK (performance only) */
SDSP_API int sdsp_oschan_set_tuning(sdsp_oschan* h, int key, int value);
SDSP_API int sdsp_oschan_reset(sdsp_oschan* h);
SDSP_API size_t sdsp_oschan_channels(const sdsp_oschan* h);      /* M */
SDSP_API size_t sdsp_oschan_decimation(const sdsp_oschan* h);    /* D */
SDSP_API size_t sdsp_oschan_subfilter_len(const sdsp_oschan* h); /* K */
SDSP_API size_t sdsp_oschan_phase(const sdsp_oschan* h);         /* (frames so far * D) mod M; 0 for a null handle */
SDSP_API int sdsp_oschan_execute_block(sdsp_oschan* h, const void* in, size_t n, void* out, size_t* frames);
SDSP_API int sdsp_oschan_execute_block_device(sdsp_oschan* h, const void* d_in, size_t n, void* d_out,
                                              size_t* frames, void* stream);
/* what the next call runs: *kernel = 1 per-frame, 2 sliding; *frames_per_block = the sliding kernel's
 * frames per workgroup on a long block (an automatic value shrinks on blocks too short to fill the
 * device at it), 1 on the per-frame kernel.  Either pointer may be null */
SDSP_API int sdsp_oschan_info(const sdsp_oschan* h, int* kernel, size_t* frames_per_block);
SDSP_API int sdsp_oschan_synchronize(sdsp_oschan* h);

/* ------------------------------------------------------------------------
 * Spectrometer: integrated power spectra of the oversampled channeliser's
 * frames, |Y|^2 summed inside the kernel (build-defined).  K = 1 with the taps
 * a window is Welch's method at hop D; K > 1 is the polyphase spectrometer.
 * Taps, channels M, decimation D and dtype as sdsp_oschan_create, checked in
 * the same order; after the decimation check and before "fewer taps than
 * channels", integration A must lie in 1..32768 (SDSP_E_UNSUPPORTED): longer
 * integrations are the caller's sum of finished spectra, M values per 32768
 * frames.  T is the dtype's real type.  Per stream, with m the frame index
 * since create / reset / set_streams:
 *
 *     Y[m]    = frame m of sdsp_oschan with the same taps, M and D: the same
 *               bits, index rotation and carried frame phase included
 *     p[m][k] = Y.re * Y.re + Y.im * Y.im        (two rounded products, one rounded sum)
 *
 * Spectrum j integrates frames jA .. jA + A - 1 in sub-blocks of 32 frames
 * counted from frame jA, the last one shorter when 32 does not divide A:
 *
 *     s_b[k] = ((0 + p[jA + 32 b][k]) + p[jA + 32 b + 1][k]) + ..      sequential, rounded in T
 *     P_j[k] = (((0 + s_0) + s_1) + ..) * scale      sequential over at most 1024 sub-blocks,
 *                                                    then one rounded multiply
 *
 * scale is a real T, 1 after create; sdsp_spec_set_scale rounds its argument
 * to T, applies to spectra completed afterwards and survives reset.  One
 * definition of the arithmetic: every kernel, every sub-blocks-per-workgroup
 * value and every call split gives the same bits.
 *
 * Blocks: n (per stream) a multiple of D gives frames = n / D; the call emits
 * spectra = (filled + frames) / A whole spectra, filled being the frames in the
 * open integration (0 <= filled < A, sdsp_spec_filled), as out[s][spectrum][M]
 * in T.  n = 0 is a no-op; a call that emits nothing may pass a null output;
 * input and output may not overlap; a refused call changes no state.  State
 * per stream: sdsp_oschan's K M - D sample history and frame phase, the open
 * sub-block's running sum, the running sum of the open integration's closed
 * sub-blocks, and filled; all zero after create, reset and set_streams.
 * ------------------------------------------------------------------------ */
typedef struct sdsp_spec sdsp_spec;
SDSP_API int sdsp_spec_create(sdsp_spec** out, int dtype, const void* taps, size_t len, size_t channels,
                              size_t decimation, size_t integration, int device);
SDSP_API void sdsp_spec_destroy(sdsp_spec* h);
SDSP_API int sdsp_spec_set_streams(sdsp_spec* h, size_t streams);
/* kernel-variant knobs: SDSP_TUNE_SPEC_KERNEL, SDSP_TUNE_SPEC_SUBBLOCKS (performance only) */
SDSP_API int sdsp_spec_set_tuning(sdsp_spec* h, int key, int value);
SDSP_API int sdsp_spec_reset(sdsp_spec* h);
SDSP_API int sdsp_spec_set_scale(sdsp_spec* h, double scale);
SDSP_API size_t sdsp_spec_channels(const sdsp_spec* h);      /* M */
SDSP_API size_t sdsp_spec_decimation(const sdsp_spec* h);    /* D */
SDSP_API size_t sdsp_spec_subfilter_len(const sdsp_spec* h); /* K */
SDSP_API size_t sdsp_spec_integration(const sdsp_spec* h);   /* A */
SDSP_API size_t sdsp_spec_phase(const sdsp_spec* h);         /* (frames so far * D) mod M, as sdsp_oschan_phase */
SDSP_API size_t sdsp_spec_filled(const sdsp_spec* h);        /* frames in the open integration; 0 for a null handle */
/* host [streams][n] in, [streams][spectra][M] reals out through the staging buffers; *spectra (may be
 * null) receives the count */
SDSP_API int sdsp_spec_execute_block(sdsp_spec* h, const void* in, size_t n, void* out, size_t* spectra);
SDSP_API int sdsp_spec_execute_block_device(sdsp_spec* h, const void* d_in, size_t n, void* d_out, size_t* spectra,
                                            void* stream);
/* what the next call runs: *kernel = 1 per-frame, 2 sliding; *subblocks_per_workgroup on a long block
 * (an automatic value shrinks on blocks too short to fill the device at it).  Either pointer may be null */
SDSP_API int sdsp_spec_info(const sdsp_spec* h, int* kernel, size_t* subblocks_per_workgroup);
SDSP_API int sdsp_spec_synchronize(sdsp_spec* h);
/* The block arithmetic without a handle or a device: a block of n samples per stream that starts
 * `filled` frames into an integration emits *spectra spectra and leaves *next_filled frames (either
 * pointer may be null).  SDSP_E_INVALID_ARGUMENT for decimation = 0, integration outside 1..32768,
 * filled >= integration or n no multiple of decimation */
SDSP_API int sdsp_spec_count(size_t decimation, size_t integration, size_t filled, size_t n, size_t* spectra,
                             size_t* next_filled);

/* ------------------------------------------------------------------------
 * DotProduct (src/dot_product/mod.rs:37-171): DotProduct::new(&coefs, direction)
 * + Execute::execute(&samples), reference order (bit-identical).  direction:
 * 0 FORWARD, 1 REVERSE.  The batched form runs `batch` sample vectors of n
 * samples spaced `stride` samples apart (device pointers, current device).
 * ------------------------------------------------------------------------ */
SDSP_API int sdsp_dot_execute(int dtype, const void* coefs, size_t len, int direction, const void* samples,
                              size_t n, void* out);
SDSP_API int sdsp_dot_execute_batched_device(int dtype, const void* coefs, size_t len, int direction,
                                             const void* d_samples, size_t n, size_t stride, size_t batch,
                                             void* d_out, void* stream);

/* ------------------------------------------------------------------------
 * AutoCorrelator (src/filter/auto_correlator/mod.rs:26-214), SURVEY §8f row 3.
 * precision: 0 = Complex<f32>, 1 = Complex<f64> (the reference's push() needs
 * C = f64, :99-102; the f32 handle runs the same operations at f32).  After each
 * push the output is sum_{j < window} x[n-j] * conj(x[n-j-delay]) over the delayed
 * Window's unfilled tail (terms with j + delay >= window are zero), newest first,
 * from zero — bit-identical to the reference order.  `channels` independent
 * correlators, channel-major buffers.  Energy: sum of |x|^2 over the last
 * window_size inputs (f64; the reference's running sum agrees to rounding).
 * ------------------------------------------------------------------------ */
typedef struct sdsp_acorr sdsp_acorr;
/* AutoCorrelator::<C>::new(window_size, delay)        :51-62 */
SDSP_API int sdsp_acorr_create(sdsp_acorr** out, size_t window_size, size_t delay, int precision, int device);
SDSP_API void sdsp_acorr_destroy(sdsp_acorr* h);
SDSP_API int sdsp_acorr_set_channels(sdsp_acorr* h, size_t channels);
/* kernel-variant knobs: SDSP_TUNE_ACORR_KERNEL, SDSP_TUNE_ACORR_SLOTS (performance only) */
SDSP_API int sdsp_acorr_set_tuning(sdsp_acorr* h, int key, int value);
SDSP_API size_t sdsp_acorr_window_size(const sdsp_acorr* h);
SDSP_API size_t sdsp_acorr_delay(const sdsp_acorr* h);
/* reset  :76-85 */
SDSP_API int sdsp_acorr_reset(sdsp_acorr* h);
/* push (one sample, single channel)  :99-111;  write (push only)  :128-137 */
SDSP_API int sdsp_acorr_push(sdsp_acorr* h, const void* sample);
SDSP_API int sdsp_acorr_write(sdsp_acorr* h, const void* samples, size_t n);
SDSP_API int sdsp_acorr_write_device(sdsp_acorr* h, const void* d_samples, size_t n, void* stream);
/* execute() on the current windows (no push), one value per channel  :156-163 */
SDSP_API int sdsp_acorr_execute(sdsp_acorr* h, void* out);
/* execute_block: push then execute per sample  :181-191 */
SDSP_API int sdsp_acorr_execute_block(sdsp_acorr* h, const void* in, size_t n, void* out);
SDSP_API int sdsp_acorr_execute_block_device(sdsp_acorr* h, const void* d_in, size_t n, void* d_out, void* stream);
/* get_energy, one f64 per channel  :212-214 */
SDSP_API int sdsp_acorr_get_energy(sdsp_acorr* h, double* energy);
SDSP_API int sdsp_acorr_synchronize(sdsp_acorr* h);

/* ------------------------------------------------------------------------
 * NCO (src/nco/mod.rs:27-187), SURVEY §8f row 4.  Phase and frequency are u32
 * registers on the host (as in the reference); sample blocks are mixed on the
 * device with the reference's 1024-entry f64 sine table and index rule.
 * mix_block: out[i] = mix_up(x[i]) (down = 0) or mix_down(x[i]) (down = 1), then
 * step() — the loop mix_up_block / mix_down_block spell out (:153-172; the
 * reference's versions index an empty Vec and panic for any non-empty input).
 * precision 0 = Complex<f32> samples (f32 table and product), 1 = Complex<f64>
 * (bit-identical to the reference).
 * ------------------------------------------------------------------------ */
typedef struct sdsp_nco sdsp_nco;
SDSP_API int sdsp_nco_create(sdsp_nco** out, int device);                     /* NCO::new  :36-50 */
SDSP_API void sdsp_nco_destroy(sdsp_nco* h);
SDSP_API int sdsp_nco_reset(sdsp_nco* h);                                     /* :53-56 */
SDSP_API uint32_t sdsp_nco_constrain(double theta);                           /* constrain :175-187 */
SDSP_API int sdsp_nco_set_frequency(sdsp_nco* h, double delta_theta);         /* :59-61 */
SDSP_API int sdsp_nco_adjust_frequency(sdsp_nco* h, double dt);               /* :64-66 */
SDSP_API double sdsp_nco_get_frequency(const sdsp_nco* h);                    /* :69-76 */
SDSP_API int sdsp_nco_set_phase(sdsp_nco* h, double phi);                     /* :79-81 */
SDSP_API int sdsp_nco_adjust_phase(sdsp_nco* h, double delta_phi);            /* :84-86 */
SDSP_API double sdsp_nco_get_phase(const sdsp_nco* h);                        /* :89-91 */
SDSP_API int sdsp_nco_step(sdsp_nco* h);                                      /* :94-96 */
SDSP_API int sdsp_nco_sincos(const sdsp_nco* h, double* sin_cos);             /* :104-117 (sin, cos) */
SDSP_API int sdsp_nco_set_internal_pll_bandwidth(sdsp_nco* h, double bw);     /* :124-132 */
SDSP_API int sdsp_nco_pll_step(sdsp_nco* h, double delta_phi);                /* :135-138 */
SDSP_API int sdsp_nco_get_state(const sdsp_nco* h, uint32_t* theta, uint32_t* delta_theta);
SDSP_API int sdsp_nco_set_state(sdsp_nco* h, uint32_t theta, uint32_t delta_theta);
SDSP_API int sdsp_nco_mix_block(sdsp_nco* h, int down, int precision, const void* in, size_t n, void* out);
SDSP_API int sdsp_nco_mix_block_device(sdsp_nco* h, int down, int precision, const void* d_in, size_t n,
                                       void* d_out, void* stream);
SDSP_API int sdsp_nco_synchronize(sdsp_nco* h);

/* ------------------------------------------------------------------------
 * Digital down-converter: NCO mix-down fused into the decimating FIR.  A
 * build-defined composition of two reference objects (as the channeliser is):
 * a handle with taps, scale, decimation M and an oscillator (theta, delta_theta)
 * is, sample for sample,
 *     v = nco.mix_down(x[i]); nco.step(); decimator.push/execute(v)
 * i.e. sdsp_nco_mix_block(down) followed by sdsp_fir_execute_block on a
 * sdsp_decim_create handle, without the mixed stream's round trip through
 * memory.  The delay line holds mixed samples (the last len - 1, oldest first,
 * the decimator's layout); after a block of n samples theta += n * delta_theta
 * (wrapping) and the decimator phase advances as sdsp_fir_* does.  Channels are
 * channel-major and share the oscillator, the sample index counted within the
 * channel.  dtype: the complex-sample pairs SDSP_RC32, SDSP_CC32, SDSP_RC64,
 * SDSP_CC64; len >= 1 and decimation >= 1 as sdsp_decim_create (a real dtype,
 * len = 0 or decimation = 0 fails with SDSP_E_INVALID_ARGUMENT).  Algorithms: SDSP_ALGO_EXACT (bit-identical to the
 * two-handle composition on their EXACT paths), SDSP_ALGO_FMA, SDSP_ALGO_AUTO
 * (FMA from 65536 32-bit inputs per call, as the decimator); SDSP_ALGO_FFT fails
 * with SDSP_E_UNSUPPORTED.  New handles start on the process default
 * (sdsp_set_default_algo).  Block entry points only: stream ordering, staging,
 * the refusal of overlapping blocks and the error strings follow
 * sdsp_fir_execute_block[_device].
 * ------------------------------------------------------------------------ */
typedef struct sdsp_ddc sdsp_ddc;
SDSP_API int sdsp_ddc_create(sdsp_ddc** out, int dtype, const void* taps, size_t len, const void* scale,
                             size_t decimation, int device);
SDSP_API void sdsp_ddc_destroy(sdsp_ddc* h);
/* same taps, knobs, delay line, decimator phase and oscillator state */
SDSP_API int sdsp_ddc_clone(const sdsp_ddc* h, sdsp_ddc** out);
/* zeroed delay line, decimator phase 0, theta = delta_theta = 0 (NCO::reset) */
SDSP_API int sdsp_ddc_reset(sdsp_ddc* h);
SDSP_API int sdsp_ddc_set_channels(sdsp_ddc* h, size_t channels); /* resets the delay lines */
SDSP_API int sdsp_ddc_set_algo(sdsp_ddc* h, int algo);
SDSP_API int sdsp_ddc_get_algo(const sdsp_ddc* h);
SDSP_API int sdsp_ddc_set_direction(sdsp_ddc* h, int up); /* 0 = mix_down (default), 1 = mix_up */
SDSP_API int sdsp_ddc_set_frequency(sdsp_ddc* h, double delta_theta);   /* NCO :59-61 */
SDSP_API int sdsp_ddc_adjust_frequency(sdsp_ddc* h, double dt);         /* NCO :64-66 */
SDSP_API int sdsp_ddc_set_phase(sdsp_ddc* h, double phi);               /* NCO :79-81 */
SDSP_API int sdsp_ddc_adjust_phase(sdsp_ddc* h, double delta_phi);      /* NCO :84-86 */
SDSP_API int sdsp_ddc_get_nco_state(const sdsp_ddc* h, uint32_t* theta, uint32_t* delta_theta);
SDSP_API int sdsp_ddc_set_nco_state(sdsp_ddc* h, uint32_t theta, uint32_t delta_theta);
SDSP_API size_t sdsp_ddc_output_count(const sdsp_ddc* h, size_t n);
SDSP_API int sdsp_ddc_execute_block(sdsp_ddc* h, const void* in, size_t n, void* out, size_t* n_out);
SDSP_API int sdsp_ddc_execute_block_device(sdsp_ddc* h, const void* d_in, size_t n, void* d_out, size_t* n_out,
                                           void* stream);
/* delay line ([channels][len-1] mixed samples, oldest first) and decimator phase, as sdsp_fir_* */
SDSP_API size_t sdsp_ddc_state_len(const sdsp_ddc* h);
SDSP_API int sdsp_ddc_get_state(const sdsp_ddc* h, void* hist, size_t* phase);
SDSP_API int sdsp_ddc_set_state(sdsp_ddc* h, const void* hist, size_t phase);
/* kernel-variant knob: SDSP_TUNE_DECIM_SEG (performance only) */
SDSP_API int sdsp_ddc_set_tuning(sdsp_ddc* h, int key, int value);
SDSP_API int sdsp_ddc_synchronize(sdsp_ddc* h);

/* ------------------------------------------------------------------------
 * Digital up-converter: NCO mix-up fused into the interpolating FIR.  A
 * build-defined composition of two reference objects (as the down-converter
 * and the channeliser are): a handle with taps, interpolation M and an
 * oscillator (theta, delta_theta) is, sample for sample,
 *     y = interpolator.execute(x[j])                  (M outputs, interp.rs:93-111)
 *     for p in 0..M: out[j*M + p] = nco.mix_up(y[p]); nco.step()
 * i.e. sdsp_pfb_execute_block on a sdsp_interp_create handle followed by
 * sdsp_nco_mix_block(down = 0), without the interpolated stream's round trip
 * through memory.
 *   dtype: the complex-sample pairs SDSP_RC32, SDSP_CC32, SDSP_RC64, SDSP_CC64;
 *     a real dtype or one out of range fails with SDSP_E_INVALID_ARGUMENT.
 *   len = 0 and interpolation = 0 fail with the interpolator's own codes,
 *     SDSP_E_COEFFICIENTS_LENGTH_ZERO and SDSP_E_INTERPOLATION_LESS_THAN_ONE,
 *     before the device is looked at.
 *   Sub-filter length K (computed in f32), zero padding of the taps and the
 *     branch layout are sdsp_interp_create's.  There is no scale: the
 *     interpolator has none.
 *   Oscillator: theta and delta_theta are u32 host registers read at launch, as
 *     in sdsp_ddc.  Output o = j*M + p of a channel is mixed with the phasor at
 *     theta + (u32)o * delta_theta; after a block of n inputs
 *     theta += (u32)(n*M) * delta_theta, wrapping.  Channels are channel-major
 *     and share the oscillator, the output index counted within the channel.
 *   Direction: mix_up by default; sdsp_duc_set_direction(h, 1) selects mix_down.
 *   Precision: 32-bit pairs use the f32 sine table and product, 64-bit pairs
 *     the f64 ones (sdsp_nco_mix_block's precision 0 / 1).
 *   Window: the last K unmixed inputs per channel, oldest first.
 *   Algorithms: SDSP_ALGO_EXACT (bit-identical to the two-handle composition on
 *     its EXACT path) and SDSP_ALGO_FMA; anything else fails with
 *     SDSP_E_INVALID_ARGUMENT, as sdsp_pfb_set_algo.  New handles follow the
 *     process default as interpolators do: FMA when it is FMA, else EXACT.
 *   Block entry points only: stream ordering, host staging, the refusal of
 *     overlapping blocks, n = 0 and the error strings follow
 *     sdsp_pfb_execute_block[_device].  The output holds n * M samples per channel.
 * ------------------------------------------------------------------------ */
typedef struct sdsp_duc sdsp_duc;
SDSP_API int sdsp_duc_create(sdsp_duc** out, int dtype, const void* taps, size_t len, size_t interpolation,
                             int device);
SDSP_API void sdsp_duc_destroy(sdsp_duc* h);
/* same taps, algorithm, direction, window and oscillator state */
SDSP_API int sdsp_duc_clone(const sdsp_duc* h, sdsp_duc** out);
/* zeroed window, theta = delta_theta = 0 (NCO::reset) */
SDSP_API int sdsp_duc_reset(sdsp_duc* h);
SDSP_API int sdsp_duc_set_channels(sdsp_duc* h, size_t channels); /* resets the windows */
SDSP_API int sdsp_duc_set_algo(sdsp_duc* h, int algo);
SDSP_API int sdsp_duc_get_algo(const sdsp_duc* h);
SDSP_API int sdsp_duc_set_direction(sdsp_duc* h, int down); /* 0 = mix_up (default), 1 = mix_down */
SDSP_API int sdsp_duc_set_frequency(sdsp_duc* h, double delta_theta);   /* NCO :59-61 */
SDSP_API int sdsp_duc_adjust_frequency(sdsp_duc* h, double dt);         /* NCO :64-66 */
SDSP_API int sdsp_duc_set_phase(sdsp_duc* h, double phi);               /* NCO :79-81 */
SDSP_API int sdsp_duc_adjust_phase(sdsp_duc* h, double delta_phi);      /* NCO :84-86 */
SDSP_API int sdsp_duc_get_nco_state(const sdsp_duc* h, uint32_t* theta, uint32_t* delta_theta);
SDSP_API int sdsp_duc_set_nco_state(sdsp_duc* h, uint32_t theta, uint32_t delta_theta);
SDSP_API size_t sdsp_duc_interpolation(const sdsp_duc* h);
SDSP_API size_t sdsp_duc_subfilter_len(const sdsp_duc* h);
SDSP_API int sdsp_duc_execute_block(sdsp_duc* h, const void* in, size_t n, void* out);
SDSP_API int sdsp_duc_execute_block_device(sdsp_duc* h, const void* d_in, size_t n, void* d_out, void* stream);
SDSP_API int sdsp_duc_synchronize(sdsp_duc* h);

/* ------------------------------------------------------------------------
 * Rational resampler: an M/D polyphase FIR that computes only the outputs it
 * keeps.  A build-defined composition of reference objects (as the channeliser
 * and the two converters are): a handle has taps, interpolation M >= 1,
 * decimation D >= 1, a window of the last K inputs per channel and a phase
 * counter c in [0, D), the number of interpolated samples since the last one
 * kept (0 after create and reset).  With z what sdsp_pfb_execute_block on a
 * sdsp_interp_create handle with the same taps, M and window writes for a call
 * of n inputs per channel (n * M samples), a call writes
 *     out[k] = z[u_k],  u_k = (k + 1) * D - 1 - c,  k = 0 .. n_out - 1
 *     n_out  = floor((c + n * M) / D),  then  c <- (c + n * M) mod D
 * which is the reference decimator's convention (it emits on counts D - 1,
 * 2D - 1, ...; decim.rs) applied to the interpolated stream.  With
 * j = u_k / M and p = u_k mod M,
 *     out[k] = sum_{i<K} cb[p][i] * x[j - i]
 * summed in that order from a zero accumulator, x[j - i] taken from the window
 * for j - i < 0: the interpolator's own expression, for 1 / D of its outputs.
 *   dtype: any of the six pairs.  Check order of create: dtype out of range and
 *     null taps with len > 0 (SDSP_E_INVALID_ARGUMENT), decimation = 0
 *     (SDSP_E_DECIMATION_LESS_THAN_ONE), decimation > 2^31 - 1
 *     (SDSP_E_INVALID_ARGUMENT), then the interpolator's own checks
 *     (SDSP_E_COEFFICIENTS_LENGTH_ZERO, SDSP_E_INTERPOLATION_LESS_THAN_ONE, the
 *     device).  *out is null after every failure.
 *   Sub-filter length K (computed in f32), zero padding of the taps and the
 *     branch layout are sdsp_interp_create's.  There is no scale.
 *   Channels are channel-major and share c: input [channels][n], output
 *     [channels][n_out].
 *   Algorithms: SDSP_ALGO_EXACT (bit-identical to the EXACT interpolator's
 *     output taken at [D - 1 - c :: D]) and SDSP_ALGO_FMA; anything else fails
 *     with SDSP_E_INVALID_ARGUMENT, as sdsp_pfb_set_algo.  New handles follow
 *     the process default as interpolators do.
 *   Block entry points only: stream ordering, host staging, the refusal of
 *     overlapping blocks and the error strings follow
 *     sdsp_pfb_execute_block[_device].  A call that emits nothing (n_out = 0)
 *     still updates the window and advances c.
 * ------------------------------------------------------------------------ */
typedef struct sdsp_resamp sdsp_resamp;
SDSP_API int sdsp_resamp_create(sdsp_resamp** out, int dtype, const void* taps, size_t len, size_t interpolation,
                                size_t decimation, int device);
SDSP_API void sdsp_resamp_destroy(sdsp_resamp* h);
/* same taps, algorithm, kernel knob, window and phase */
SDSP_API int sdsp_resamp_clone(const sdsp_resamp* h, sdsp_resamp** out);
/* zeroed window, phase 0 */
SDSP_API int sdsp_resamp_reset(sdsp_resamp* h);
SDSP_API int sdsp_resamp_set_channels(sdsp_resamp* h, size_t channels); /* resets the windows and the phase */
SDSP_API int sdsp_resamp_set_algo(sdsp_resamp* h, int algo);
SDSP_API int sdsp_resamp_get_algo(const sdsp_resamp* h);
/* kernel-variant knob: SDSP_TUNE_RESAMP_KERNEL (performance only) */
SDSP_API int sdsp_resamp_set_tuning(sdsp_resamp* h, int key, int value);
SDSP_API size_t sdsp_resamp_interpolation(const sdsp_resamp* h);
SDSP_API size_t sdsp_resamp_decimation(const sdsp_resamp* h);
SDSP_API size_t sdsp_resamp_subfilter_len(const sdsp_resamp* h);
SDSP_API int sdsp_resamp_get_phase(const sdsp_resamp* h, size_t* phase);
SDSP_API int sdsp_resamp_set_phase(sdsp_resamp* h, size_t phase); /* phase >= D: SDSP_E_INVALID_ARGUMENT */
/* outputs per channel a block of n inputs produces from the handle's current phase */
SDSP_API size_t sdsp_resamp_output_count(const sdsp_resamp* h, size_t n);
SDSP_API int sdsp_resamp_execute_block(sdsp_resamp* h, const void* in, size_t n, void* out, size_t* n_out);
SDSP_API int sdsp_resamp_execute_block_device(sdsp_resamp* h, const void* d_in, size_t n, void* d_out,
                                              size_t* n_out, void* stream);
/* the kernel the next call runs (1 staged, 2 per output, 3 branch-stationary) and its outputs per workgroup */
SDSP_API int sdsp_resamp_info(const sdsp_resamp* h, int* kernel, size_t* tile);
SDSP_API int sdsp_resamp_synchronize(sdsp_resamp* h);
/* The two formulas above in 64-bit arithmetic; needs no handle and no device.
 * SDSP_E_INVALID_ARGUMENT when interpolation or decimation is 0, phase >= decimation, or
 * phase + n * interpolation does not fit 63 bits. */
SDSP_API int sdsp_resamp_count(size_t interpolation, size_t decimation, size_t phase, size_t n, size_t* n_out,
                               size_t* next_phase);

/* ------------------------------------------------------------------------
 * Arbitrary-rate resampler: any rate from one polyphase bank.  A build-defined
 * composition on the reference's PolyPhaseFilterBank (pfb.rs: push, then
 * execute(index) with a caller-chosen branch): an interpolating FIR with P
 * branches whose interpolated stream is never written; each output is a linear
 * interpolation between two neighbouring interpolated samples, chosen by a
 * 64-bit fixed-point time accumulator.  A handle is an interpolator handle
 * (sdsp_interp_create with interpolation = P) plus two registers:
 *   step  input samples per output, unsigned Q32.32, 2^16 <= step <= 2^48 (the
 *         rate 2^32 / step lies in [2^-16, 2^16])
 *   t     time of the next output, Q32.32, measured from the first input of
 *         the next call; 0 after create and reset; all channels share it
 * Let z be the EXACT interpolator's stream over the handle's whole input
 * history, z(j * P + p) = sum_{i<K} cb[p][i] * x[j - i], with z(-1) = 0 after
 * create and reset.  A call of n inputs per channel, n < 2^31 (a larger n fails
 * with SDSP_E_INVALID_ARGUMENT), computes
 *     n_out = 0 if t >= n * 2^32, else ceil((n * 2^32 - t) / step)
 *     for k < n_out:
 *         T = t + k * step;  j = T >> 32;  f = T & (2^32 - 1)
 *         v = f * P (64-bit);  b = v >> 32;  m = v & (2^32 - 1)
 *         mu = (R)m * 2^-32       R = the sample's real type; (R)m is the
 *                                 ordinary round-to-nearest conversion
 *         u = j * P + b
 *         a = z(u - 1);  c = z(u)
 *         out[k] = a + mu * (c - a)       on re and im separately; mu is real
 *     t <- t + n_out * step - n * 2^32
 * For b >= 1, a and c are branches b - 1 and b on the window ending at x[j];
 * for b = 0, a is branch P - 1 on the window ending at x[j - 1] (it reaches
 * x[j - K]: for j = 0 the oldest sample of the window).  Outputs are
 * independent of each other: output k follows from k alone.
 *   No look-ahead: the handle interpolates between z(u - 1) and z(u), so it
 *     delays by 1 / P of an input sample relative to interpolating between
 *     z(u) and z(u + 1).
 *   dtype: any of the six pairs.  Check order of create: dtype out of range,
 *     null taps with len > 0, step out of range (the message names "step"),
 *     filters > 2^31 - 1 (all SDSP_E_INVALID_ARGUMENT), then the interpolator's
 *     own checks (SDSP_E_COEFFICIENTS_LENGTH_ZERO, filters = 0 reported as
 *     SDSP_E_INTERPOLATION_LESS_THAN_ONE, the device).  *out is null after
 *     every failure.
 *   Sub-filter length K (computed in f32), zero padding of the taps, the
 *     branch layout and the window of the last K inputs per channel are
 *     sdsp_interp_create's.  There is no scale.
 *   Channels are channel-major and share step and t: input [channels][n],
 *     output [channels][n_out].
 *   Algorithms, set as sdsp_pfb_set_algo does: SDSP_ALGO_EXACT (both dot
 *     products in the reference order; the subtraction, the product with mu
 *     and the addition each rounded once, nothing contracted: bit-identical to
 *     the same formula applied on the host to the EXACT interpolator's output)
 *     and SDSP_ALGO_FMA (fused dot products, the last line fma(mu, c - a, a)).
 *     New handles follow the process default as interpolators do.
 *   Block entry points only: stream ordering, host staging, the refusal of
 *     overlapping blocks and the error strings follow
 *     sdsp_pfb_execute_block[_device].  A call that emits nothing (n_out = 0)
 *     still moves the window and t.
 * ------------------------------------------------------------------------ */
typedef struct sdsp_arb sdsp_arb;
SDSP_API int sdsp_arb_create(sdsp_arb** out, int dtype, const void* taps, size_t len, size_t filters, uint64_t step,
                             int device);
SDSP_API void sdsp_arb_destroy(sdsp_arb* h);
/* same taps, algorithm, kernel knob, window, step and t */
SDSP_API int sdsp_arb_clone(const sdsp_arb* h, sdsp_arb** out);
/* zeroed window, t = 0; the step stays */
SDSP_API int sdsp_arb_reset(sdsp_arb* h);
SDSP_API int sdsp_arb_set_channels(sdsp_arb* h, size_t channels); /* zeroes the windows and t */
SDSP_API int sdsp_arb_set_algo(sdsp_arb* h, int algo);
SDSP_API int sdsp_arb_get_algo(const sdsp_arb* h);
/* kernel-variant knob: SDSP_TUNE_ARB_KERNEL (performance only) */
SDSP_API int sdsp_arb_set_tuning(sdsp_arb* h, int key, int value);
SDSP_API size_t sdsp_arb_filters(const sdsp_arb* h);
SDSP_API size_t sdsp_arb_subfilter_len(const sdsp_arb* h);
SDSP_API int sdsp_arb_get_step(const sdsp_arb* h, uint64_t* step);
/* takes effect at the next output; t stays unchanged.  Out of range: SDSP_E_INVALID_ARGUMENT */
SDSP_API int sdsp_arb_set_step(sdsp_arb* h, uint64_t step);
SDSP_API int sdsp_arb_get_time(const sdsp_arb* h, uint64_t* t);
SDSP_API int sdsp_arb_set_time(sdsp_arb* h, uint64_t t); /* t >= 2^63: SDSP_E_INVALID_ARGUMENT */
/* outputs per channel a block of n inputs produces from the handle's current step and t */
SDSP_API size_t sdsp_arb_output_count(const sdsp_arb* h, size_t n);
SDSP_API int sdsp_arb_execute_block(sdsp_arb* h, const void* in, size_t n, void* out, size_t* n_out);
SDSP_API int sdsp_arb_execute_block_device(sdsp_arb* h, const void* d_in, size_t n, void* d_out, size_t* n_out,
                                           void* stream);
/* the kernel the next call runs (1 staged, 2 per output) and its outputs per workgroup */
SDSP_API int sdsp_arb_info(const sdsp_arb* h, int* kernel, size_t* tile);
SDSP_API int sdsp_arb_synchronize(sdsp_arb* h);
/* The two formulas above (n_out and the next t) in 64-bit arithmetic; needs no handle and no
 * device; both results are optional.  SDSP_E_INVALID_ARGUMENT when step is out of range,
 * t >= 2^63 or n >= 2^31. */
SDSP_API int sdsp_arb_count(uint64_t step, uint64_t t, size_t n, size_t* n_out, uint64_t* next_t);
/* step = floor(ldexp(1.0 / rate, 32) + 0.5).  SDSP_E_INVALID_ARGUMENT for a rate that is not
 * finite, is not positive, or whose step leaves the range (and for a null step). */
SDSP_API int sdsp_arb_step_from_rate(double rate, uint64_t* step);

/* ------------------------------------------------------------------------
 * AGC (src/auto_gain_control/mod.rs:97-677), SURVEY §8f row 4.  A handle is a
 * bank of `channels` independent AGCs (channel-major sample buffers) with
 * device-resident state; one lane per channel runs the reference's per-sample
 * recurrence (execute :214-246) in f64, with the squelch state machine
 * (update_squelch_mode :631-677).  Samples are f64 (sample_type 0) or
 * Complex<f64> (1), the two types the reference's trait bounds admit.  The
 * recurrence calls exp/ln/log10 per sample: results agree with the reference to
 * libm rounding (the device's f64 exp/log are not glibc's), not bit for bit.
 * Setters apply to every channel; sdsp_agc_get_state reads one channel.
 * ------------------------------------------------------------------------ */
typedef struct sdsp_agc sdsp_agc;
typedef enum {  /* SquelchMode  :84-94 */
    SDSP_SQUELCH_UNKNOWN = 0,
    SDSP_SQUELCH_ENABLED = 1,
    SDSP_SQUELCH_RISE = 2,
    SDSP_SQUELCH_SIGNALHI = 3,
    SDSP_SQUELCH_FALL = 4,
    SDSP_SQUELCH_SIGNALLO = 5, /* the reference's SINGALLO */
    SDSP_SQUELCH_TIMEOUT = 6,
    SDSP_SQUELCH_DISABLED = 7
} sdsp_squelch_mode;
typedef struct {  /* struct AGC  :96-108 */
    double gain, scale, bandwidth, alpha, energy_estimate;
    int32_t lock, squelch_mode;
    double squelch_threshold;
    uint64_t squelch_timeout, squelch_timer;
} sdsp_agc_state;
SDSP_API int sdsp_agc_create(sdsp_agc** out, size_t channels, int device);      /* AGC::new  :136-149 */
SDSP_API void sdsp_agc_destroy(sdsp_agc* h);
SDSP_API size_t sdsp_agc_channels(const sdsp_agc* h);
/* kernel-variant knob: SDSP_TUNE_AGC_KERNEL (performance only) */
SDSP_API int sdsp_agc_set_tuning(sdsp_agc* h, int key, int value);
SDSP_API int sdsp_agc_reset(sdsp_agc* h);                                       /* :178-188 */
/* execute_block  :273-285 (execute per sample :214-246); n samples per channel */
SDSP_API int sdsp_agc_execute_block(sdsp_agc* h, int sample_type, const void* in, size_t n, void* out);
SDSP_API int sdsp_agc_execute_block_device(sdsp_agc* h, int sample_type, const void* d_in, size_t n, void* d_out,
                                           void* stream);
/* init  :568-586 — per channel: gain = 1 / (sqrt(mean |x|^2) + 1e-16); levels[c] receives the level */
SDSP_API int sdsp_agc_init(sdsp_agc* h, int sample_type, const void* in, size_t n, double* levels);
SDSP_API int sdsp_agc_lock(sdsp_agc* h);                                        /* :303-305 */
SDSP_API int sdsp_agc_unlock(sdsp_agc* h);                                      /* :322-324 */
SDSP_API int sdsp_agc_set_bandwidth(sdsp_agc* h, double bandwidth);             /* :374-386 */
SDSP_API int sdsp_agc_set_signal_level(sdsp_agc* h, double level);              /* :416-428 */
SDSP_API int sdsp_agc_set_rssi(sdsp_agc* h, double rssi);                       /* :458-466 */
SDSP_API int sdsp_agc_set_gain(sdsp_agc* h, double gain);                       /* :497-504 */
SDSP_API int sdsp_agc_set_scale(sdsp_agc* h, double scale);                     /* :535-542 */
SDSP_API int sdsp_agc_update_squelch_mode(sdsp_agc* h);                        /* :631-677, each channel */
SDSP_API int sdsp_agc_squelch_enable(sdsp_agc* h);                              /* :589-591 */
SDSP_API int sdsp_agc_squelch_disable(sdsp_agc* h);                             /* :594-596 */
SDSP_API int sdsp_agc_squelch_set_threshold(sdsp_agc* h, double threshold);     /* :612-614 */
SDSP_API int sdsp_agc_squelch_set_timeout(sdsp_agc* h, uint64_t timeout);       /* :622-624 */
SDSP_API int sdsp_agc_get_state(sdsp_agc* h, size_t channel, sdsp_agc_state* st);
SDSP_API int sdsp_agc_set_state(sdsp_agc* h, size_t channel, const sdsp_agc_state* st);
SDSP_API int sdsp_agc_synchronize(sdsp_agc* h);

/* ------------------------------------------------------------------------
 * Device utilities
 * ------------------------------------------------------------------------ */
/* Synthetic stream (build-defined): `count` f32 scalars
 * x(i) = ((mix64(seed ^ channel*G + (start+i+1)*G) >> 40) * 2^-24) * 2 - 1 */
SDSP_API int sdsp_synth_f32_device(void* d_out, uint64_t seed, uint64_t channel, uint64_t start,
                                   size_t count, void* stream);
/* STREAM-style 16-B-per-lane device copy (HBM bandwidth calibration) */
SDSP_API int sdsp_bandwidth_copy_device(const void* d_src, void* d_dst, size_t bytes, void* stream);
/* Host-side reference FIR tap design (src/filter/firdes/mod.rs:278-305) */
SDSP_API int sdsp_firdes_kaiser(size_t n, double fc, double as, double mu, double* h);
SDSP_API int sdsp_firdes_notch(size_t m, double f0, double as, double* h);
SDSP_API double sdsp_kaiser_beta(double as);
/* The rest of solid::filter::firdes (src/filter/firdes/mod.rs:46-640), host f64 like the
 * reference.  Status codes are FirdesErrorCode + 1: 1 Bandwidth, 2 StopBandLevel, 3 Mu,
 * 4 SemiLength, 5 FilterSize, 6 FFTSize.  `method`: 0 EstimationMethod::Kaiser, 1 Herrmann. */
/* estimate_required_filter_length :71-94 (the f64 estimate `as usize`, saturating) */
SDSP_API int sdsp_firdes_estimate_length(double df, double as, int method, size_t* len);
/* estimate_required_filter_length_kaiser :199-211 / _herrmann :213-240 */
SDSP_API int sdsp_firdes_estimate_length_kaiser(double df, double as, double* len);
SDSP_API int sdsp_firdes_estimate_length_herrmann(double df, double as, double* len);
/* estimate_required_filter_stop_band_attenuation :117-145 (bisection, 20 steps) */
SDSP_API int sdsp_firdes_estimate_stop_band_attenuation(double df, size_t n, int method, double* as);
/* estimate_required_filter_transition :168-196 */
SDSP_API int sdsp_firdes_estimate_transition(double as, size_t n, int method, double* df);
/* firdes_doppler :389-419 (Bessel J0 of src/math/mod.rs:102-146, Kaiser window beta 4) */
SDSP_API int sdsp_firdes_doppler(size_t n, double fd, double k, double theta, double* h);
/* filter_autocorrelation :443-456, filter_crosscorrelation :487-527 */
SDSP_API double sdsp_filter_autocorrelation(const double* h, size_t n, ptrdiff_t lag);
SDSP_API double sdsp_filter_crosscorrelation(const double* h, size_t nh, const double* g, size_t ng, ptrdiff_t lag);
/* filter_isi :552-577: (rms, max); (0, 0) when n != 2 sps delay + 1 */
SDSP_API int sdsp_filter_isi(const double* h, size_t n, size_t sps, size_t delay, double* rms, double* max);
/* filter_energy :602-640: relative out-of-band energy over fft_size bins (DotProduct FORWARD per bin) */
SDSP_API int sdsp_filter_energy(const double* h, size_t n, double fc, size_t fft_size, double* energy);
/* PLL loop filters (src/filter/iirdes/pll/mod.rs:24-99) */
SDSP_API int sdsp_active_lag(double bw, double zeta, double k, double* num3, double* den3);
SDSP_API int sdsp_active_proportional_integral(double bw, double zeta, double k, double* num3, double* den3);
/* group delay helpers (src/group_delay/mod.rs:51-129) */
SDSP_API int sdsp_fir_group_delay_taps(const double* h, size_t n, double f, double* out);
SDSP_API int sdsp_iir_group_delay_taps(const double* b, size_t nb, const double* a, size_t na, double f,
                                       double* out);

#ifdef __cplusplus
}
#endif
#endif /* SDSP_H */

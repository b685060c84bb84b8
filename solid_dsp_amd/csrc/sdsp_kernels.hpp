// Internal launcher interface between the C-ABI runtime (runtime.cpp) and the
// kernel translation units.  Not installed; no torch types anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdsp {

struct FirArgs {
    const void* x;         // device input, channel-major [channels][n]
    const void* hist;      // device history [channels][L-1], oldest first
    const void* taps_rev;  // device reversed taps cr[i] = h[L-1-i]
    const void* scale;     // host pointer to one Coef
    void* y;               // device output [channels][nout]
    size_t n, nout, channels;
    int L, M;
    size_t j0;             // block-relative index of the first emitting input (decimator)
    bool exact;
    int seg = 0;           // polyphase decimator: outputs per lane group (0 = auto)
};

hipError_t launch_fir_direct(int dtype, const FirArgs& a, hipStream_t s);
hipError_t launch_decim_direct(int dtype, const FirArgs& a, hipStream_t s);
// column-parallel polyphase decimator (kern_decim.hip); false = not applicable
bool try_launch_decim_poly(int dtype, const FirArgs& a, hipStream_t s, hipError_t* err);
hipError_t launch_hist_update(int dtype, const void* x, const void* old_hist, void* new_hist, size_t n, int Lm1,
                              size_t channels, hipStream_t s);

// overlap-save (N = 4096) for 32-bit complex samples and for real f32 samples with real taps
constexpr int kOlsOneShot = 0;     // interior segments: one-shot XCD-ordered kernel (kern_fir_ols_os.hip)
constexpr int kOlsPersistent = 1;  // persistent packed kernel, kOlsSegsPerBlock segments per workgroup
constexpr int kOlsScalar = 2;      // scalar persistent kernel for every segment (kern_fir_ols.hip)
constexpr int kOlsOneShotWide = 3;  // the one-shot kernel with 16-byte lanes (pair exchange by DPP);
                                    // real f32: 8-byte lanes, every other value the 4-byte default
constexpr int kOlsSegsPerBlock = 16;
// W4096 column bases [3][256], W256 row bases [3][16], then the first powers alone: {C1, D1}
// per column [256] and {E1, F1} per row [16] (kern_fir_ols_os.hip, ols_tables.cpp ols_os_bases)
constexpr int kOlsOsTabCD = 768 + 48, kOlsOsTabEF = kOlsOsTabCD + 256;
constexpr int kOlsOsTabF4 = kOlsOsTabEF + 16;

struct OlsPlan {
    void* d_H;    // [256][16] c32: H[k0 + 16 k1 + 256 k2] / N * scale, row t = 16 k0 + k1
    void* d_tw1;  // [256][16] c32: W4096^(t*k)
    void* d_tw2;  // [16][16]  c32: W256^(a*b)
    int halo_rows;  // h2: halo = 256*h2 >= L-1
    int kernel = kOlsOneShot;
    void* d_pkt = nullptr;    // k-pair major tables: [0, 2048) float4 spectrum rows, [2048, 4096) W4096 rows,
                              // [4096, 4224) W256 rows (ols_tables.cpp ols_pack_pkt)
    void* d_ostab = nullptr;  // one-shot kernel tables (kOlsOsTabF4 float4, ols_tables.cpp ols_os_bases)
                              // (C1 C2 | C3 D1 | D2 D3), then [16][8] float4 W256 rows
    // real taps (conjugate-symmetric spectrum): the half-spectrum table of the one-shot kernel,
    // float4 [4][kOlsHalfRow] (ols_tables.cpp ols_half_table), else null
    void* d_hhalf = nullptr;
    int sample_bytes = 8;  // 8: c32 samples; 4: real f32 samples and taps (kern_fir_ols_real.hip,
                           // which reads d_pkt and d_ostab only)
};
constexpr int kOlsHalfRow = 257;  // 256 lanes + the tail entry of lane (0, 0)
constexpr int kOlsN = 4096;
// new_hist: the next call's history buffer.  *hist_done = true when the launch also wrote it
// (the one-shot kernel does, for n >= L - 1); otherwise the caller runs the history update.
hipError_t launch_fir_ols(const OlsPlan& p, const void* x, const void* hist, void* new_hist, void* y, size_t n,
                          int L, size_t channels, int num_cus, hipStream_t s, bool* hist_done);
// interior segments [lo, hi) of a call: whole input window and all outputs inside the stream
void ols_interior_range(long long n, int h2, long long* lo, long long* hi);
// interior-segment kernels (16-byte rows)
hipError_t launch_fir_ols_os(const OlsPlan& p, const void* x, const void* hist, void* new_hist, void* y, size_t n,
                             int Lm1, size_t channels, hipStream_t s, bool wide);
// real f32 samples: pairs of segments packed as one complex segment (kern_fir_ols_real.hip)
hipError_t launch_fir_ols_real(const OlsPlan& p, const void* x, const void* hist, void* new_hist, void* y, size_t n,
                               int Lm1, size_t channels, hipStream_t s, bool lane8);
hipError_t launch_fir_ols_pk(const OlsPlan& p, const void* x, void* y, size_t n, size_t channels, hipStream_t s,
                             long long lo, long long hi);

// overlap-save for long filters on c32 samples (kern_fir_ols_long.hip): one transform of
// N = 2^log2n = N1 N2 points per N - (L-1) outputs, N1 = 2^(log2n / 2), in three passes
constexpr int kOlsLongMinLog2N = 13, kOlsLongMaxLog2N = 22;
constexpr size_t kOlsLongMaxLm1 = (size_t)1 << 20;
struct OlsLongPlan {
    const void* d_G = nullptr;    // [N1][N2] c32: G[k1 + N1 k2] * scale / N (ols_tables.cpp ols_long_spectrum)
    const void* d_tw1 = nullptr;  // [N1] c32 e^{-j 2 pi m / N1}
    const void* d_tw2 = nullptr;  // [N2] c32 e^{-j 2 pi m / N2}
    int log2n = 0;
    int Lm1 = 0;
};
// segments of one channel's block of n samples
size_t ols_long_segments(size_t n, int log2n, int Lm1);
// tmp: min(segs_per_round, channels * segments) * N c32 samples of scratch; a call with more
// segments runs in rounds.  Writes y only; the caller runs the history update.
hipError_t launch_fir_ols_long(const OlsLongPlan& p, const void* x, const void* hist, void* y, void* tmp, size_t n,
                               size_t channels, size_t segs_per_round, hipStream_t s);

// polyphase filterbank / interpolator: out[j*M + p] = sum_{i<K} cb[p*K + i] * ext(j - i)
struct PfbArgs {
    const void* x;
    const void* hist;  // [channels][H] oldest first; ext(j<0) = hist[H + j]
    const void* cb;    // device branch coefs [M][K] (stored order, pfb.rs:33-40)
    void* y;           // [channels][n*M]
    size_t n, channels;
    int K, M, H;
    bool exact;
};
hipError_t launch_pfb(int dtype, const PfbArgs& a, hipStream_t s);

// one-sample FIR step (kern_fir_step.hip): shifts the delay line (last Lm1 of
// hist_in + sample -> hist_out), if emit writes one output to `out`, then
// releases *flag = seq (both host-mapped); the sample is passed by value
struct FirStepArgs {
    const void* sample;  // host pointer, copied into the launch
    const void* hist_in;
    void* hist_out;
    const void* taps_rev;
    const void* scale;  // host pointer to one Coef
    void* out;
    unsigned* flag;
    unsigned seq;
    int Lm1, L;
    bool emit, exact;
};
hipError_t launch_fir_step(int dtype, const FirStepArgs& a, hipStream_t s);

// IIR: SOS cascade (sections > 0) or Normal DF-II (sections == 0)
struct IirArgs {
    const void* x;
    void* y;
    const void* coefs;   // SOS: [S][5] (b0,b1,b2,a1,a2)/a0 ; Normal: num[nb] then den[na-1]
    const void* P;       // scan: [8][2S][2S] A^(B 2^k) (Coef type)
    const void* st_in;   // [channels][state]
    void* st_out;
    size_t n, nout, channels;
    int sections, nb, na, cap;
    int Mi, Md;          // interpolation (zero stuffing) / decimation factors
    size_t phase;        // DecimatingIIRFilter index before this block
    bool algo_scan;
    int wc;              // warm-up chunks (scan)
    const void* Cr = nullptr;  // wave scan: [B][2S] output response to the state, c A^i (Coef type)
    int ws_variant = 0;        // wave scan chunk: 0 = 256 bytes, 1 = 128 bytes
    // exact inter-wave carries (wc == 0: cascades whose state response does not decay):
    // Phi[t-1] = A^(64 B t) (t = tiles per wave, 1..8), scratch G / Cin [channels][waves][2S]
    const void* Phi = nullptr;
    void* G = nullptr;
    void* Cin = nullptr;
    size_t scratch_waves = 0;  // capacity of G / Cin per channel
};
// waves the exact-carry wave scan launches for this call (sizes G / Cin)
size_t iir_wscan_waves(int dtype, const IirArgs& a, int* tpw = nullptr);  // waves (and tiles per wave) of one call
hipError_t launch_iir(int dtype, const IirArgs& a, hipStream_t s);
int iir_scan_chunk(int dtype);  // samples per lane chunk of the scan kernel
// wave-level scan (kern_iir_wscan.hip): SOS cascades, with rate changes; wc <= 32
// warm-up chunks, or wc == 0 with Phi/G/Cin: aggregate pass, carry scan, output pass
hipError_t launch_iir_wscan(int dtype, const IirArgs& a, hipStream_t s);
int iir_wscan_chunk(int dtype, int variant);  // samples per lane chunk of the wave scan

// batched FFT (power of two: Stockham in LDS; otherwise direct DFT)
struct FftArgs {
    const void* x;
    void* y;
    const void* tw;  // [N] e^{-j 2 pi m / N}
    int N, logN;
    bool pow2, inverse;
    size_t batch;
};
hipError_t launch_fft(bool f64, const FftArgs& a, hipStream_t s);
// strided pass of the four-step FFT (kern_fft.hip fft_pass_kernel); Ntw = 0: no inter-pass twiddle
struct FftPass {
    const void* x;
    void* y;
    const void* tw;  // [L] e^{-j 2 pi m / L}
    int L, logL;
    long long count, G, S0, S1, Si, T1, So, Ntw;
    bool inverse;
    const void* twx = nullptr;  // c32 [Tl | Th] inter-pass twiddle tables when Ntw = 2^20 (L = 1024 path)
    int group = 4;      // generic pass: at most this many transforms per workgroup (SDSP_TUNE_FFT_GROUP)
    int wave1024 = 16;  // L = 1024 c32 passes (SDSP_TUNE_FFT_WAVE1024): 16 pipelined persistent kernel,
                        // 1 / 8 one-shot with 16 / 8 transforms per workgroup, 0 the generic pass
};
// L = 1024, complex f32 pass on the wave FFT (kern_chan1024.hip); false = not applicable
bool try_launch_fft1024_pass(const FftPass& p, hipStream_t s, hipError_t* err);
hipError_t launch_fft_pass(bool f64, const FftPass& p, hipStream_t s);
// Bluestein steps: 0 chirp in (x[N] -> a[M], zero padded), 1 a *= B, 2 chirp out (a -> y[N])
hipError_t launch_bluestein(bool f64, int step, const void* in, void* out, const void* w_or_B, long long N, long long M,
                            long long batch, hipStream_t s);

// PFB + FFT channeliser (M power of two)
struct ChanArgs {
    const void* x;     // [streams][n]
    const void* hist;  // [streams][(K-1) M]
    const void* cb;    // [M][K] real branch coefficients (stored order)
    void* y;           // [streams][frames][M]
    const void* tw;
    int M, logM, K;
    size_t n, frames, streams;
    int fast = 3;  // streaming kernel where it applies: 0 off, 1/3 = 1024-thread, 2/4 = 512-thread, 3/4 prefetching (sdsp_chan_set_tuning)
    int frames_per_block = 0;  // streaming kernel: frames per workgroup (0 = default)
    bool xcd_order = true;     // streaming kernel: XCD-contiguous chunk order
};
hipError_t launch_chan(bool f64, const ChanArgs& a, hipStream_t s);
// streaming M = 1024 kernel (kern_chan1024.hip); false = not applicable
bool try_launch_chan1024(const ChanArgs& a, hipStream_t s, hipError_t* err);

// synthesis channeliser (kern_ichan.hip): frames of M channel samples in, n = frames * M time samples out
constexpr int kIchanPerFrame = 1;  // one workgroup per (frame, stream), K transforms per frame
constexpr int kIchanRing = 2;      // one workgroup per (chunk of frames, stream), transformed frames kept in LDS
struct IchanArgs {
    const void* x;     // [streams][frames][M]
    const void* hist;  // [streams][(K-1) M] untransformed input frames, oldest first
    const void* cbt;   // [K][M] real branch coefficients, cbt[i][r] = g[r + (K-1-i) M]
    void* y;           // [streams][n]
    const void* tw;
    int M, logM, K;
    size_t n, frames, streams;
    int kernel;            // SDSP_TUNE_ICHAN_KERNEL: 0 automatic, or a kIchan* value
    int frames_per_block;  // SDSP_TUNE_ICHAN_FRAMES_PER_BLOCK: ring kernel, 0 automatic
};
struct IchanPlan {
    int kernel;               // kIchanPerFrame / kIchanRing
    size_t frames_per_block;  // frames per workgroup on a long block (1 on the per-frame kernel)
};
IchanPlan ichan_plan(bool f64, int M, int K, int kernel, int frames_per_block);
hipError_t launch_ichan(bool f64, const IchanArgs& a, hipStream_t s);

// oversampled analysis channeliser (kern_oschan.hip): n = frames * D time samples in, frames of M channel samples out
constexpr int kOschanPerFrame = 1;  // one workgroup per (frame, stream), branch sums from global memory
constexpr int kOschanSlide = 2;     // one workgroup per (chunk of frames, stream), the stream's window kept in LDS
struct OschanArgs {
    const void* x;     // [streams][n]
    const void* hist;  // [streams][K M - D] input samples, oldest first
    const void* cbt;   // [K][M] real branch coefficients, cbt[i][p] = h[p + (K-1-i) M]
    void* y;           // [streams][frames][M]
    const void* tw;
    int M, logM, K, D;
    int phase;         // (frames before this call * D) mod M
    size_t n, frames, streams;
    int kernel;            // SDSP_TUNE_OSCHAN_KERNEL: 0 automatic, or a kOschan* value
    int frames_per_block;  // SDSP_TUNE_OSCHAN_FRAMES_PER_BLOCK: sliding kernel, 0 automatic
};
struct OschanPlan {
    int kernel;               // kOschanPerFrame / kOschanSlide
    size_t frames_per_block;  // frames per workgroup on a long block (1 on the per-frame kernel)
};
OschanPlan oschan_plan(bool f64, int M, int K, int D, int kernel, int frames_per_block);
hipError_t launch_oschan(bool f64, const OschanArgs& a, hipStream_t s);

// spectrometer (kern_spec.hip): the oversampled channeliser's frames squared and integrated A at a time
constexpr int kSpecPerFrame = 1;  // branch sums from global memory, as kOschanPerFrame
constexpr int kSpecSlide = 2;     // the stream's window kept in LDS, as kOschanSlide
struct SpecArgs {
    const void* x;       // [streams][n]
    const void* hist;    // [streams][K M - D] input samples, oldest first
    const void* cbt;     // [K][M] real branch coefficients, as OschanArgs
    const void* tw;
    const void* sub_in;  // [streams][M] reals: the open sub-block's running sum (read when filled % 32 > 0)
    void* sub_out;       // the same after the call (written when the call ends inside a sub-block)
    const void* tot_in;  // [streams][M] reals: the open integration's closed sub-blocks (read when filled >= 32)
    void* tot_out;       // the same after the call (written when the call ends inside an integration)
    void* part;          // scratch [streams][spec_subblocks()][M] reals
    void* out;           // [streams][spectra][M] reals, spectra = (filled + frames) / A
    int M, logM, K, D;
    int phase;           // (frames before this call * D) mod M
    int A, filled;       // integration length; frames in the open integration before the call, < A
    double scale;        // already rounded to the real type
    size_t n, frames, streams;
    int kernel;          // SDSP_TUNE_SPEC_KERNEL: 0 automatic, or a kSpec* value
    int subblocks;       // SDSP_TUNE_SPEC_SUBBLOCKS: sub-blocks per workgroup, 0 automatic
};
struct SpecPlan {
    int kernel;        // kSpecPerFrame / kSpecSlide
    size_t subblocks;  // sub-blocks (of up to 32 frames) per workgroup on a long block
};
SpecPlan spec_plan(bool f64, int M, int K, int D, int A, int kernel, int subblocks);
// sub-blocks a call of `frames` frames touches when it starts `filled` frames into an integration of A
size_t spec_subblocks(size_t filled, size_t A, size_t frames);
hipError_t launch_spec(bool f64, const SpecArgs& a, hipStream_t s);

// batched DotProduct::execute
struct DotArgs {
    const void* coefs;
    int it;  // min(samples, len)
    const void* s;
    size_t stride, batch;
    void* out;
};
hipError_t launch_dot(int dtype, const DotArgs& a, hipStream_t s);

// AutoCorrelator (kern_rx.hip); prec 0 = complex f32, 1 = complex f64.  hist: [channels][H]
// oldest first (H = window size), K = max(W - delay, 0) product terms per output
// kernel (SDSP_TUNE_ACORR_KERNEL): 0 the pipelined kernel on interior tiles where it applies, else the
// one-shot kernel staging the delayed input in LDS; 1 the one-shot kernel everywhere (staged); 2 the
// one-shot kernel with two loads per product (no staging)
// slots (SDSP_TUNE_ACORR_SLOTS): 0 one pipelined wave per resident slot of the device, else at most
// this many per channel (whole eights)
hipError_t launch_acorr(int prec, const void* x, const void* hist, void* y, size_t n, int H, int d, int K,
                        size_t channels, hipStream_t s, int kernel = 0, int slots = 0);
hipError_t launch_acorr_current(int prec, const void* hist, void* out, int H, int d, int K, size_t channels,
                                hipStream_t s);
hipError_t launch_acorr_energy(int prec, const void* x, const void* hist, size_t n, int H, int W, size_t channels,
                               double* energy, hipStream_t s);
// NCO mix_up / mix_down over a block (kern_rx.hip): theta_i = theta0 + i dtheta (u32)
hipError_t launch_nco_mix(int prec, bool down, const void* x, void* y, size_t n, const double* table, uint32_t theta0,
                          uint32_t dtheta, int num_cus, hipStream_t s);
// Digital down-converter (kern_ddc.hip): the decimator of `fir` (complex-sample dtypes; exact = the
// reference-order walk, else the polyphase walk where its shape rule admits L and M) with every
// sample of the call multiplied by the oscillator's phasor at theta0 + i dtheta on the load path;
// fir.hist holds mixed samples.  launch_ddc_hist writes the next history to new_hist.
struct DdcArgs {
    FirArgs fir;
    const double* table;  // device copy of the 1024-entry f64 sine table
    uint32_t theta0, dtheta;
    bool down;
};
hipError_t launch_ddc(int dtype, const DdcArgs& d, hipStream_t s);
hipError_t launch_ddc_hist(int dtype, const DdcArgs& d, void* new_hist, hipStream_t s);
// Digital up-converter (kern_duc.hip): the interpolator of `pfb` (complex-sample dtypes, the kernels
// and selection rule of launch_pfb) with every output o of a channel multiplied by the oscillator's
// phasor at theta0 + o dtheta on the store path; pfb.hist holds unmixed inputs.
struct DucArgs {
    PfbArgs pfb;
    const double* table;  // device copy of the 1024-entry f64 sine table
    uint32_t theta0, dtheta;
    bool down;
};
hipError_t launch_duc(int dtype, const DucArgs& d, hipStream_t s);
// Rational resampler (kern_resamp.hip): the interpolator's stream z[u] = sum_{i<K} cb[u % M][i] ext(u / M - i)
// taken at u_k = (k + 1) D - 1 - c, k < n_out; only those dot products are computed.
constexpr int kResampStaged = 1, kResampPerOutput = 2, kResampBranch = 3;
struct ResampArgs {
    const void* x;     // [channels][n]
    const void* hist;  // [channels][H] oldest first, as PfbArgs
    const void* cb;    // [M][K]
    void* y;           // [channels][n_out]
    size_t n, n_out, channels;
    int K, M, H;
    size_t D, c;       // decimation, phase counter before the call (c < D)
    bool exact;
    int kernel;        // SDSP_TUNE_RESAMP_KERNEL: 0 automatic, or a kResamp* value
};
// which kernel a shape runs on and how it is tiled: a function of the shape alone, never of n
struct ResampPlan {
    int kernel;       // kResampStaged / kResampPerOutput / kResampBranch
    size_t tile;      // outputs per workgroup
    int T;            // staged: outputs per workgroup
    int A, R, step;   // branch: lanes, outputs per lane, inputs a lane advances per output
    int S;            // staged and branch: samples of the LDS span
    bool cb_lds;      // staged: branch table in LDS
    size_t lds;       // dynamic LDS bytes
};
ResampPlan resamp_plan(int dtype, int M, size_t D, int K, int forced);
hipError_t launch_resamp(int dtype, const ResampArgs& a, hipStream_t s);
// Arbitrary-rate resampler (kern_arb.hip): output k sits at time T = t + k step (Q32.32 input samples);
// with j = T >> 32, v = (T & (2^32 - 1)) P, b = v >> 32 and mu = (v & (2^32 - 1)) 2^-32 it is
// a + mu (c - a), c = z[j P + b] and a = z[j P + b - 1] of the interpolator's stream z above (M = P).
constexpr int kArbStaged = 1, kArbPerOutput = 2;
struct ArbArgs {
    const void* x;     // [channels][n]
    const void* hist;  // [channels][H] oldest first, as PfbArgs; H = K (a reaches x[j - K] when b = 0)
    const void* cb;    // [P][K]
    void* y;           // [channels][n_out]
    size_t n, n_out, channels;
    int K, P, H;
    uint64_t step, t;  // inputs per output and time of output 0, Q32.32 (sdsp_arb_count keeps every T < 2^63)
    bool exact;
    int kernel;        // SDSP_TUNE_ARB_KERNEL: 0 automatic, or a kArb* value
};
// which kernel a shape runs on and how it is tiled: a function of the shape and the step, never of n or t
struct ArbPlan {
    int kernel;   // kArbStaged / kArbPerOutput
    size_t tile;  // outputs per workgroup
    int S;        // staged: samples of the LDS span, for the largest fraction a tile can start on
    bool cb_lds;  // staged: branch table in LDS
    size_t lds;   // dynamic LDS bytes
};
ArbPlan arb_plan(int dtype, int P, uint64_t step, int K, int forced);
hipError_t launch_arb(int dtype, const ArbArgs& a, hipStream_t s);
// AGC bank (src/auto_gain_control/mod.rs): state is sdsp_agc_state[channels] in
// device memory; cplx = Complex<f64> samples, else f64
// pipe: agc_pipe_kernel for calls it admits (SDSP_TUNE_AGC_KERNEL 0), else agc_kernel
hipError_t launch_agc(bool cplx, const void* x, void* y, size_t n, void* state, size_t channels, hipStream_t s,
                      bool pipe = true);
hipError_t launch_agc_init(bool cplx, const void* x, size_t n, void* state, double* levels, size_t channels,
                           hipStream_t s);

hipError_t launch_bw_copy(const void* a, void* b, size_t bytes, int num_cus, hipStream_t s);
hipError_t launch_synth_f32(float* out, uint64_t seed, uint64_t channel, uint64_t start, size_t count,
                            hipStream_t s);

}  // namespace sdsp

// One-shot, XCD-ordered overlap-save FIR for real f32 streams with real f32 taps (gfx950):
// FIRFilter<f32, f32> under SDSP_ALGO_FFT.
//
// Same filter and the same segmentation as kern_fir_ols_os.hip on 4-byte samples: real segment
// s reads x[s V - H, s V - H + 4096) and writes y[s V, (s + 1) V), H = 256 h2 >= L - 1,
// V = 4096 - H.  With real taps g the circular convolution is linear over the reals,
//     conv(a + i b, g) = conv(a, g) + i conv(b, g),
// so one 4096-point complex transform filters two real windows: pair p packs the adjacent
// segments A = 2p and B = 2p + 1 as z = A + i B, runs the transform of the c32 kernel on z
// (ols_os_transform of sdsp_ols_os.hpp, the one copy both kernels share: pdft16f, the C/D/E/F
// twiddle bases of d_ostab, the spectrum of d_pkt, the 34 KB aliased LDS image, 4 workgroups per
// CU), and stores rows >= h2 of Re to A's outputs and of Im to B's.  The taps are real, but this
// kernel runs the full-table form of the transform, not its half-spectrum (REALG) form.
//
// Adjacent segments pair up (not distant halves of the call): B's halo is A's tail and A's halo
// is the previous pair's tail, which the same XCD has just read (workgroup b runs on XCD b % 8
// and takes pair lo + (b % 8) q + b / 8).  Traffic is 8 B per real sample, the arithmetic per
// real sample half of the c32 kernel's.
//
// Lane shapes of the interior kernel (SDSP_TUNE_OLS_KERNEL):
//   0 (default)  4-byte lanes: lane t owns column t, per row one 4-byte buffer load from A and
//                one from B (1 KB contiguous per row and wave group), row offsets in SGPRs.  No
//                alignment beyond 4 bytes.  With a one-row halo B's row 0 is A's row 15 and is
//                not loaded a second time.
//   3            8-byte lanes: lane t = 2c + h loads columns (2c, 2c + 1) of rows k + 8h from A
//                and from B, then the DPP pair exchange of the c32 WIDE path gives it column t;
//                stores mirror this.  Needs 8-byte aligned rows (else the launcher runs shape 0).
// Measured on 2^30 samples, 256 taps (tools/ols_real_ab.py, profiles/r07/ols_real_ab.json, median
// of 12 shuffled rounds): 4-byte lanes 1.456 ms (0.737 of 8 TB/s at 8 B/sample), 8-byte lanes
// 1.574 ms (the exchange costs more than the wider accesses save, as for c32); the direct
// kernels of the same handle 6.295 ms (FMA) and 11.831 ms (EXACT).
//
// The boundary pairs run in a separate small launch (EDGE): a window that starts before the
// stream reads the f32 history (the last L - 1 inputs, oldest first; before the history: 0),
// a window past the end reads 0 and its stores are dropped, an absent B (odd segment count)
// reads 0 and stores nothing, and the pair holding the call's last segment writes the next
// history.  Every edge offset is computed explicitly from a descriptor based inside the stream.
//
// Numerics: the rounding error of a real segment is relative to the energy of its pair.
// Deterministic for a given sequence of calls, but not bit-invariant to where the stream is cut
// into calls (the cut decides which segments pair).
#include "sdsp_ols_os.hpp"

namespace sdsp {

namespace {

constexpr int kOutOfRange = 0x7ffffff0;  // a buffer offset past every descriptor here: loads return 0

template <int POL> __device__ __forceinline__ float ld32(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, POL));
}

}  // namespace

// One pair of real segments per workgroup.  Template parameters:
//   HALO1  the halo is one row (L <= 257): rows 1..15 are stored without a test per row, B's
//          row 0 is taken from A's row 15, and the two rows a neighbouring pair also reads (A's
//          row 0 and B's row 15) load with the default cache policy, the others nontemporal;
//   LANE8  8-byte lanes with the DPP pair exchange (interior only);
//   EDGE   the boundary pairs [0, plo) and [phi, npair) of a call (block b takes pair
//          b < plo ? b : phi + b - plo), the last one writing the next history (new_hist).
// Interior pairs [plo, phi): both windows inside the stream.
template <bool HALO1, bool LANE8, bool EDGE>
__global__ void __launch_bounds__(256, 4)
fir_ols_real_kernel(const float* __restrict__ x, const float* __restrict__ hist, float* __restrict__ new_hist,
                    const float4* __restrict__ Hs, const float4* __restrict__ tb, float* __restrict__ y, long long n,
                    long long plo, long long phi, long long q, long long nseg, int h2, int Lm1) {
    __shared__ __attribute__((aligned(16))) f2 img[16 * kRow];
    long long pair;
    if constexpr (EDGE) {
        pair = (long long)blockIdx.x < plo ? (long long)blockIdx.x : phi + ((long long)blockIdx.x - plo);
    } else {
        const int xc = blockIdx.x & 7;
        pair = plo + (long long)xc * q + (long long)(blockIdx.x >> 3);
        const long long xe = plo + (long long)(xc + 1) * q;
        if (pair >= (xe < phi ? xe : phi)) return;  // uniform over the workgroup
    }
    if constexpr (HALO1) h2 = 1;  // compiled in (the launcher checks h2 == 1)
    const int t = threadIdx.x;
    const long long V = 4096 - 256 * h2;
    const long long ch = blockIdx.y;
    x += ch * n;
    y += ch * n;
    const auto rt = __builtin_amdgcn_make_buffer_rsrc((void*)tb, (short)0, kOlsOsTabF4 * 16, kBufWord3);
    // twiddle bases: {C1, D1} of column t and {E1, F1} of row t & 15, requested before the rows
    const float4 cd = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rt, 16 * t, 16 * kOlsOsTabCD, 0));
    const float4 ef = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rt, 16 * (t & 15), 16 * kOlsOsTabEF, 0));
    f2 v[16];
    if constexpr (EDGE) {
        // segment c of the pair (0 = A, 1 = B): window [base, base + 4096).  Its descriptors start
        // at stream position b0 = max(base, 0) and cover what of the window lies inside the
        // stream; an absent segment (seg >= nseg) gets empty descriptors: loads 0, no stores.
        hist += ch * Lm1;
        long long base[2], b0[2];
        __amdgpu_buffer_rsrc_t rx[2], ry[2], rp[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const long long seg = 2 * pair + c;
            const bool present = seg < nseg;
            base[c] = seg * V - 256 * h2;
            b0[c] = present && base[c] > 0 ? base[c] : 0;  // < n for a present segment
            long long rem = n - b0[c];
            if (rem > 4096) rem = 4096;
            const int nrec = present ? (int)(4 * rem) : 0;
            rx[c] = __builtin_amdgcn_make_buffer_rsrc((void*)(x + b0[c]), (short)0, nrec, kBufWord3);
            ry[c] = __builtin_amdgcn_make_buffer_rsrc((void*)(y + b0[c]), (short)0, nrec, kBufWord3);
            rp[c] = __builtin_amdgcn_make_buffer_rsrc((void*)hist, (short)0, present ? 4 * Lm1 : 0, kBufWord3);
        }
        // rows inside the stream through rx (window rows start at multiples of 256 from base, so a
        // row lies wholly before the stream or wholly at or after its start), rows before it from
        // the history; positions before the history read 0 through an out-of-range offset
        float w[2][16];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long pos = base[c] + 256 * r;
                if (pos >= 0) {
                    w[c][r] = ld32<0>(rx[c], (int)(4 * (pos - b0[c] + t)), 0);
                } else {
                    const long long e = Lm1 + pos + t;  // < Lm1
                    w[c][r] = ld32<0>(rp[c], e >= 0 ? (int)(4 * e) : kOutOfRange, 0);
                }
            }
        }
        if (new_hist != nullptr && (2 * pair == nseg - 1 || 2 * pair + 1 == nseg - 1)) {
            // the call's last segment: its window holds the last Lm1 inputs (halo >= Lm1), which
            // become the history of the next call (ping-pong buffer: never the one read above)
            const bool c = (nseg - 1) & 1;
            const long long h0 = n - Lm1, bl = c ? base[1] : base[0];
            float* nh = new_hist + ch * Lm1;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long i = bl + 256 * r + t - h0;
                if (i >= 0 && i < Lm1) nh[i] = c ? w[1][r] : w[0][r];
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = f2{w[0][r], w[1][r]};
        ols_os_transform<false>(v, cd, ef, Hs, img, t, t & 15);
        // rows >= h2 start at seg V + 256 (r - h2) >= 0; positions past the stream fall outside
        // the descriptor (dropped)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (r >= h2) {
                const float re = v[kout(r)].x, im = v[kout(r)].y;
                const long long pa = base[0] + 256 * r - b0[0] + t, pb = base[1] + 256 * r - b0[1] + t;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(re), ry[0], (int)(4 * pa), 0, kNT);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(im), ry[1], (int)(4 * pb), 0, kNT);
            }
        }
    } else {
        // both windows inside the stream: A at x + base, B one V further on
        const long long base = 2 * pair * V - 256 * h2;
        const auto rxa = __builtin_amdgcn_make_buffer_rsrc((void*)(x + base), (short)0, 16384, kBufWord3);
        const auto rxb = __builtin_amdgcn_make_buffer_rsrc((void*)(x + base + V), (short)0, 16384, kBufWord3);
        const auto rya = __builtin_amdgcn_make_buffer_rsrc((void*)(y + base), (short)0, 16384, kBufWord3);
        const auto ryb = __builtin_amdgcn_make_buffer_rsrc((void*)(y + base + V), (short)0, 16384, kBufWord3);
        if constexpr (LANE8) {
            // lane t = 2c + h: columns (2c, 2c + 1) of rows k + 8h of A and of B, i.e. z of two
            // columns; one DPP exchange with lane t ^ 1 gives it column t over the 16 rows
            const int vo = 8 * (t >> 1) + 8192 * (t & 1);
            f2 qa[8], qb[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                qa[k] = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(rxa, vo, 1024 * k, kNT));
                qb[k] = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(rxb, vo, 1024 * k, kNT));
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) pair_exchange(f2{qa[k].x, qb[k].x}, f2{qa[k].y, qb[k].y}, v[k], v[8 + k]);
            ols_os_transform<false>(v, cd, ef, Hs, img, t, t & 15);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                f2 a, b;  // z of columns (2c, 2c + 1) of row k + 8h
                pair_exchange(v[kout(k)], v[kout(8 + k)], a, b);
                if (k + 8 * (t & 1) >= h2) {
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, f2{a.x, b.x}), rya, vo, 1024 * k, kNT);
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, f2{a.y, b.y}), ryb, vo, 1024 * k, kNT);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (HALO1 && r == 0) {
                    v[r].x = ld32<0>(rxa, 4 * t, 0);  // the previous pair's last row
                } else if (HALO1 && r == 15) {
                    v[r].x = ld32<kNT>(rxa, 4 * t, 1024 * r);
                    v[r].y = ld32<0>(rxb, 4 * t, 1024 * r);  // the next pair's halo
                } else {
                    v[r].x = ld32<kNT>(rxa, 4 * t, 1024 * r);
                    v[r].y = ld32<kNT>(rxb, 4 * t, 1024 * r);
                }
            }
            if constexpr (HALO1) v[0].y = v[15].x;  // B's halo is A's last row
            ols_os_transform<false>(v, cd, ef, Hs, img, t, t & 15);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (r >= h2) {
                    const float re = v[kout(r)].x, im = v[kout(r)].y;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(re), rya, 4 * t, 1024 * r, kNT);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(im), ryb, 4 * t, 1024 * r, kNT);
                }
            }
        }
    }
}

namespace {

// interior pair range of a call: [plo, phi) with both input windows inside the stream
void ols_real_interior_range(long long n, int h2, long long* plo, long long* phi) {
    const long long V = 4096 - 256LL * h2, H = 256LL * h2;
    const long long nseg = (n + V - 1) / V, npair = (nseg + 1) / 2;
    long long a = (H + 2 * V - 1) / (2 * V);  // first p with 2 p V - H >= 0
    if (a > npair) a = npair;
    // last p with (2 p + 1) V - H + 4096 <= n
    const long long num = n - 4096 + H - V;
    long long b = num >= 0 ? num / (2 * V) + 1 : 0;
    if (b > npair) b = npair;
    if (b < a) b = a;
    *plo = a;
    *phi = b;
}

// every pair of every channel: the boundary pairs (and the next history) in one small launch,
// the interior ones in the XCD-ordered grid
template <bool HALO1, bool LANE8>
hipError_t launch_fir_ols_real_t(const OlsPlan& p, const void* x, const void* hist, void* new_hist, void* y, size_t n,
                                 int Lm1, size_t channels, hipStream_t s) {
    const int h2 = p.halo_rows;
    const long long V = 4096 - 256 * h2;
    const long long nseg = ((long long)n + V - 1) / V, npair = (nseg + 1) / 2;
    long long lo, hi;
    ols_real_interior_range((long long)n, h2, &lo, &hi);
    if (hi > npair - 1) hi = npair - 1;  // the last pair always runs in the boundary launch (history)
    if (hi < lo) hi = lo;
    const long long nedge = lo + (npair - hi);
    const long long q = (hi - lo + 7) / 8;
    hipLaunchKernelGGL((fir_ols_real_kernel<false, false, true>), dim3((unsigned)nedge, (unsigned)channels), dim3(256),
                       0, s, (const float*)x, (const float*)hist, (float*)new_hist, (const float4*)p.d_pkt,
                       (const float4*)p.d_ostab, (float*)y, (long long)n, lo, hi, 0LL, nseg, h2, Lm1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || hi <= lo) return e;
    hipLaunchKernelGGL((fir_ols_real_kernel<HALO1, LANE8, false>), dim3((unsigned)(8 * q), (unsigned)channels),
                       dim3(256), 0, s, (const float*)x, (const float*)hist, (float*)nullptr, (const float4*)p.d_pkt,
                       (const float4*)p.d_ostab, (float*)y, (long long)n, lo, hi, q, nseg, h2, Lm1);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_fir_ols_real(const OlsPlan& p, const void* x, const void* hist, void* new_hist, void* y, size_t n,
                               int Lm1, size_t channels, hipStream_t s, bool lane8) {
    if (n == 0) return hipSuccess;
    const int h2 = p.halo_rows;
    if (h2 < 1 || h2 > 15 || Lm1 > 256 * h2) return hipErrorInvalidValue;
    // 8-byte lanes need 8-byte aligned rows in every channel
    const bool rows8 = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 7) == 0 &&
                       (channels == 1 || n % 2 == 0);
    if (lane8 && rows8) return launch_fir_ols_real_t<false, true>(p, x, hist, new_hist, y, n, Lm1, channels, s);
    if (h2 == 1) return launch_fir_ols_real_t<true, false>(p, x, hist, new_hist, y, n, Lm1, channels, s);
    return launch_fir_ols_real_t<false, false>(p, x, hist, new_hist, y, n, Lm1, channels, s);
}

}  // namespace sdsp

// One-shot, XCD-ordered overlap-save FIR for 32-bit complex streams (gfx950):
// the default interior-segment kernel of FIRFilter::execute_block for c32.
//
// Same filter as FIRFilter::execute (src/filter/fir/mod.rs:209-212),
//     y[n] = scale * sum_{i<L} h[L-1-i] x[n-i],
// per 4096-sample segment as a circular convolution with the zero-padded
// g[i] = scale h[L-1-i] (spectrum H/N precomputed in f64 on the host).
// Segment s reads x[s V - H, s V - H + 4096) and writes the V = 4096 - H
// outputs that do not wrap (H = 256 h2 >= L - 1).  The transform is the one of
// kern_fir_ols.hip / kern_fir_ols_pk.hip (three radix-16 passes each way,
// n = 256 n2 + 16 n1 + n0, k = k0 + 16 k1 + 256 k2, no bit reversal), in packed
// FP32 with the fused DFT16 of sdsp_pk.hpp (72 packed instructions per DFT16).
// What differs is the shape, chosen for the HBM stream:
//
//  * one segment per 256-thread workgroup, one workgroup per segment (no
//    persistent loop): the dispatcher deals workgroup b to XCD b % 8, so
//    segment(b) = lo + (b % 8) q + b / 8 makes every XCD stream one contiguous
//    eighth of the call in order (the halo row of a segment is the tail its XCD
//    neighbour just read, an L2 hit);
//  * 4 workgroups per CU (16 waves): 116 VGPRs and one 34 KB LDS image.  The
//    image is ALIASED across phases: in P2/P4 lane (k0, n0) owns the 16
//    positions (k0, 16 j + n0), in P3 lane (k0, k1) owns (k0, 16 k1 + j), in
//    P1/P5 lane t owns column t -- each lane reads and rewrites only its own
//    positions inside a phase, so one region suffices.  P2, P3 and P4 of wave w
//    touch only four rows of its own (k0 = 4w .. 4w + 3; with a real g the rows
//    of ols_rg_row, 122 VGPRs), so only P1 -> P2 and P4 -> P5 need a workgroup
//    barrier;
//  * lane t owns column t in P1 / P5: 8-byte buffer loads and stores per row
//    (row offsets in SGPRs, no address arithmetic in VGPRs);
//  * no twiddle tables in LDS or per-lane tables in registers: W4096^(t k) =
//    D_{k>>2} C_{k&3} and W256^(l k) = F_{k>>2} E_{k&3} from per-lane bases
//    (C1, D1, E1, F1: two float4 from L2; C2 = C1 C1, C3 = C2 C1, ...), the
//    spectrum slice of P3 loaded from L2 in P2 (eight 16-byte loads per lane;
//    four when g is real, the other half read from the mirror lane's registers
//    through DPP: the REALG instances below);
//  * nontemporal input loads and stores (the stream is read and written once).
//
// The transform between "rows loaded" and "rows ready to store" (phases P1..P5, the LDS image,
// the lane map of the REALG instances) is ols_os_transform of sdsp_ols_os.hpp, shared with the
// real-stream kernel kern_fir_ols_real.hip.
//
// Numerics: bit-identical across calls and launch shapes; against the f64
// restatement rel-RMS ~2.2e-7 on the cfg2 taps (§8d tolerance 1e-6).
//
// The variants measured against this kernel (ablations, load orders, table forms, segment
// pairs, half spectra, ...) live in the lab copy tools/lab/ols_os_lab_kernel.hip (tools only);
// the history is in profiles/LABLOG.md and profiles/r06/LAB.md.
#include "sdsp_ols_os.hpp"

namespace sdsp {

// One segment of the transform.  Template parameters (the product's instances only):
//   HALO1  the halo is one row (L <= 257, every cfg2-like filter): rows 1..15 are stored without a
//          test per row, and the two rows a neighbouring segment also reads (row 0, the halo, and
//          row 15, the next segment's halo) load with the default cache policy, the others
//          nontemporal (traffic 1.00005x instead of 1.029x, profiles/r05);
//   WIDE   16-byte lanes (SDSP_TUNE_OLS_KERNEL = 3): lane pair (2c, 2c + 1) moves columns
//          (2c, 2c + 1) of rows k + 8h and swaps halves by DPP (1-2.5 % slower: the exchange costs
//          more than the wider accesses save);
//   EDGE   the boundary segments of a call (launched apart, so the interior kernel carries no
//          boundary code): past the end of the stream loads return 0 and stores are dropped, rows
//          before it come from the history, and the call's last segment writes the next history;
//   REALG  g is real (OlsPlan::d_hhalf): Hs is the half table, float4 [4][kOlsHalfRow], and the
//          transform loads four spectrum k-pairs per lane instead of eight (ols_os_transform).
//
// xw / yw point at the segment's window x[base, base + 4096) of its channel (the callers add the
// segment's offset once, for both); base, n, hist, new_hist and Lm1 are read by EDGE only.
template <bool HALO1, bool WIDE, bool EDGE, bool REALG>
__device__ __forceinline__ void ols_os_segment(const f2* __restrict__ xw, const f2* __restrict__ hist,
                                               f2* __restrict__ new_hist, const float4* __restrict__ Hs,
                                               const float4* __restrict__ tb, f2* __restrict__ yw, long long base,
                                               long long n, int Lm1, int h2, f2* img, int t) {
    static_assert(!(EDGE && REALG), "the boundary segments read the full table");
    const int lo4 = t & 15;
    if constexpr (HALO1) h2 = 1;  // compiled in (the launcher checks h2 == 1)
    // the segment's window as a raw buffer
    int nrec = 32768;
    if constexpr (EDGE) {
        const long long rem = n - base;
        if (rem < 4096) nrec = (int)(8 * rem);
    }
    const auto rx = __builtin_amdgcn_make_buffer_rsrc((void*)xw, (short)0, nrec, kBufWord3);
    const auto ry = __builtin_amdgcn_make_buffer_rsrc((void*)yw, (short)0, nrec, kBufWord3);
    const auto rt = __builtin_amdgcn_make_buffer_rsrc((void*)tb, (short)0, kOlsOsTabF4 * 16, kBufWord3);
    // twiddle bases: {C1, D1} of column t and {E1, F1} of row lo4 (ols_tables.cpp ols_os_bases), requested
    // before the segment's rows (L2 hits that land while the rows stream in)
    const float4 cd = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rt, 16 * t, 16 * kOlsOsTabCD, 0));
    const float4 ef = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rt, 16 * lo4, 16 * kOlsOsTabEF, 0));
    f2 v[16];
    if constexpr (EDGE) {
        // rows inside the stream through rx, rows before it from the handle's history (the last
        // Lm1 inputs, oldest first; positions before the history read as 0 through an
        // out-of-range offset)
        const auto rp = __builtin_amdgcn_make_buffer_rsrc((void*)hist, (short)0, 8 * Lm1, kBufWord3);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long pos = base + 256 * r;
            if (pos >= 0) {
                v[r] = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(rx, 8 * t, 2048 * r, 0));
            } else {
                const long long e = Lm1 + pos + t;
                v[r] = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(rp, e >= 0 ? (int)(8 * e) : 0x7ffffff0, 0, 0));
            }
        }
        if (new_hist != nullptr) {
            // the call's last segment: its window holds the last Lm1 inputs (halo >= Lm1), which
            // become the history of the next call (ping-pong buffer: never the one read above)
            const long long h0 = n - Lm1;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long i = base + 256 * r + t - h0;
                if (i >= 0 && i < Lm1) new_hist[i] = v[r];
            }
        }
    } else if constexpr (WIDE) {
        // 16-byte lanes: lane t = 2c + h loads columns (2c, 2c + 1) of rows k + 8h, then one DPP
        // exchange per dword with its partner lane t ^ 1 gives it column t over the rows
        f4v q[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            q[k] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rx, 16 * (t >> 1) + 16384 * (t & 1),
                                                                                2048 * k, kNT));
#pragma unroll
        for (int k = 0; k < 8; ++k) pair_exchange(f2{q[k].x, q[k].y}, f2{q[k].z, q[k].w}, v[k], v[8 + k]);
    } else {
        // the rows in row order (behind the two table loads the compiler issues them as 0, 1, 4, 5,
        // 8, 12, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15): 2 % faster than the first radix-4 stage's order
        // and than either order enforced with scheduling barriers (profiles/r05/lab/
        // r05h_olsburst.log, r05i_olsburst.log); the issue order moves the time by 2-3 %, so it is
        // read off the disassembly with every change to this prologue (profiles/r07/LAB.md)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (HALO1 && (r == 0 || r == 15))
                v[r] = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(rx, 8 * t, 2048 * r, 0));
            else
                v[r] = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(rx, 8 * t, 2048 * r, kNT));
        }
    }
    ols_os_transform<REALG>(v, cd, ef, Hs, img, t, lo4);
    // nontemporal stores (3.14 -> 3.08 ms on cfg2); rows < h2 wrap and are dropped, positions past
    // the stream fall outside the descriptor (dropped)
    if constexpr (WIDE && !EDGE) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            f2 a, b;
            pair_exchange(v[kout(k)], v[kout(8 + k)], a, b);
            if (k + 8 * (t & 1) >= h2)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, f4v{a.x, a.y, b.x, b.y}), ry,
                                                       16 * (t >> 1) + 16384 * (t & 1), 2048 * k, kNT);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (r >= h2) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2v, v[kout(r)]), ry, 8 * t, 2048 * r, kNT);
    }
}

// Interior segments [lo, hi) of every channel (whole window inside the stream): workgroup b runs on
// XCD b % 8 and takes segment lo + (b % 8) q + b / 8, so each XCD streams one contiguous eighth of
// the call in order.  The grid is 8 q wide, so b / 8 < q and the segment lies inside its XCD's
// eighth; only the ragged end of the range (seg >= hi) has to be refused.
//
// The first row load waits for everything before it while the workgroup's slot moves no bytes,
// so the start-up path is kept short: 12 argument dwords, ordered by first use, which the
// translation unit is compiled to preload into SGPRs (csrc/Makefile; a fetch of the same list is
// the compiler's fallback), and segment arithmetic in 32 bits on the scalar unit (the launcher
// refuses 2^31 or more segments): no scalar-memory wait and no vector compare before the loads.
// stride is the distance between channels in samples.
template <bool HALO1, bool WIDE, bool EDGE, bool REALG>
__global__ void __launch_bounds__(256, 4)
fir_ols_os_kernel(const f2* __restrict__ x, f2* __restrict__ y, const float4* __restrict__ Hs,
                  const float4* __restrict__ tb, long long stride, unsigned lo, unsigned hi, unsigned q, int h2) {
    static_assert(!EDGE, "the boundary segments take the long argument list");
    __shared__ __attribute__((aligned(16))) f2 img[16 * kRow];
    const unsigned seg = lo + (blockIdx.x & 7u) * q + (blockIdx.x >> 3);
    if (seg >= hi) return;  // uniform over the workgroup
    if constexpr (HALO1) h2 = 1;
    // window start in samples: seg V - 256 h2 >= 0 (lo >= 1), one 32 x 32 -> 64 multiply
    const unsigned H = 256u * (unsigned)h2;
    const long long off = (long long)((unsigned long long)seg * (4096u - H)) - (long long)H +
                          (long long)blockIdx.y * stride;
    ols_os_segment<HALO1, WIDE, false, REALG>(x + off, nullptr, nullptr, Hs, tb, y + off, 0, 0, 0, h2, img, threadIdx.x);
}

// The boundary segments [0, lo) and [hi, nseg) of every channel (block b takes segment
// b < lo ? b : hi + b - lo), the last one writing the next history (new_hist): a launch of its
// own, so the interior kernel carries none of this.
template <bool HALO1, bool WIDE, bool EDGE>
__global__ void __launch_bounds__(256, 4)
fir_ols_os_kernel(const f2* __restrict__ x, const f2* __restrict__ hist, f2* __restrict__ new_hist,
                  const float4* __restrict__ Hs, const float4* __restrict__ tb, f2* __restrict__ y, long long n,
                  long long lo, long long hi, long long nseg, int h2, int Lm1) {
    static_assert(EDGE && !HALO1 && !WIDE, "the interior segments take the short argument list");
    __shared__ __attribute__((aligned(16))) f2 img[16 * kRow];
    const long long seg = (long long)blockIdx.x < lo ? (long long)blockIdx.x : hi + ((long long)blockIdx.x - lo);
    const int V = 4096 - 256 * h2;
    const long long ch = blockIdx.y;
    const long long base = seg * V - 256 * h2;
    ols_os_segment<false, false, true, false>(x + ch * n + base, hist + ch * Lm1,
                                       (new_hist != nullptr && seg == nseg - 1) ? new_hist + ch * Lm1 : nullptr, Hs, tb,
                                       y + ch * n + base, base, n, Lm1, h2, img, threadIdx.x);
}

// every segment of every channel: the boundary segments (and the next history) in one small
// launch from the full table, the interior ones in the XCD-ordered grid (REALG: from the half table)
template <bool HALO1, bool WIDE, bool REALG>
hipError_t launch_fir_ols_os_t(const OlsPlan& p, const void* x, const void* hist, void* new_hist, void* y, size_t n,
                               int Lm1, size_t channels, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const int h2 = p.halo_rows;
    if (h2 < 1 || h2 > 15 || Lm1 > 256 * h2 || (HALO1 && h2 != 1)) return hipErrorInvalidValue;
    const long long V = 4096 - 256 * h2;
    const long long nseg = ((long long)n + V - 1) / V;
    if (nseg >= (1LL << 31)) return hipErrorInvalidValue;  // the interior kernel's segment numbers are 32-bit
    long long lo, hi;
    ols_interior_range((long long)n, h2, &lo, &hi);
    if (hi > nseg - 1) hi = nseg - 1;  // the last segment always runs in the boundary launch (history)
    if (hi < lo) hi = lo;
    const long long nedge = lo + (nseg - hi);
    const long long q = (hi - lo + 7) / 8;
    hipLaunchKernelGGL((fir_ols_os_kernel<false, false, true>), dim3((unsigned)nedge, (unsigned)channels), dim3(256),
                       0, s, (const f2*)x, (const f2*)hist, (f2*)new_hist, (const float4*)p.d_pkt,
                       (const float4*)p.d_ostab, (f2*)y, (long long)n, lo, hi, nseg, h2, Lm1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || hi <= lo) return e;
    hipLaunchKernelGGL((fir_ols_os_kernel<HALO1, WIDE, false, REALG>), dim3((unsigned)(8 * q), (unsigned)channels), dim3(256),
                       0, s, (const f2*)x, (f2*)y, (const float4*)(REALG ? p.d_hhalf : p.d_pkt), (const float4*)p.d_ostab, (long long)n,
                       (unsigned)lo, (unsigned)hi, (unsigned)q, h2);
    return hipGetLastError();
}

hipError_t launch_fir_ols_os(const OlsPlan& p, const void* x, const void* hist, void* new_hist, void* y, size_t n,
                             int Lm1, size_t channels, hipStream_t s, bool wide) {
    if (p.d_hhalf != nullptr) {  // g is real: the half-spectrum interior instances
        if (wide) return launch_fir_ols_os_t<false, true, true>(p, x, hist, new_hist, y, n, Lm1, channels, s);
        if (p.halo_rows == 1) return launch_fir_ols_os_t<true, false, true>(p, x, hist, new_hist, y, n, Lm1, channels, s);
        return launch_fir_ols_os_t<false, false, true>(p, x, hist, new_hist, y, n, Lm1, channels, s);
    }
    if (wide) return launch_fir_ols_os_t<false, true, false>(p, x, hist, new_hist, y, n, Lm1, channels, s);
    if (p.halo_rows == 1) return launch_fir_ols_os_t<true, false, false>(p, x, hist, new_hist, y, n, Lm1, channels, s);
    return launch_fir_ols_os_t<false, false, false>(p, x, hist, new_hist, y, n, Lm1, channels, s);
}

}  // namespace sdsp

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
// LDS image: element (r, c) at r * 272 + c + (c >> 4) (one 8-byte pad per
// 16-column block; rows 544 dwords apart, i.e. opposite halves of the 64
// banks).  Every access is a per-lane base plus a compile-time offset and is
// conflict-free except P5's reads (lanes 0 and 31 of a 32-lane group share a
// bank pair: SQ_LDS_BANK_CONFLICT counts 2 extra cycles per ds_read_b64,
// tools/lds_probe.hip).
//
// Numerics: bit-identical across calls and launch shapes; against the f64
// restatement rel-RMS ~2.2e-7 on the cfg2 taps (§8d tolerance 1e-6).
//
// The variants measured against this kernel (ablations, load orders, table forms, segment
// pairs, half spectra, ...) live in the lab copy tools/lab/ols_os_lab_kernel.hip (tools only);
// the history is in profiles/LABLOG.md and profiles/r06/LAB.md.
#include "sdsp_device.hpp"
#include "sdsp_kernels.hpp"
#include "sdsp_pk.hpp"

namespace sdsp {

using namespace pk;

namespace {

constexpr int kRow = 272;

typedef unsigned int u2v __attribute__((ext_vector_type(2)));
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
constexpr int kBufWord3 = 0x00020000;  // raw buffer descriptor word 3 (gfx9 family)
constexpr int kNT = 2;                 // nontemporal cache policy of a buffer access

// P2 -> P3 -> P4 hand-offs stay inside one wave: the next phase reads only what this wave wrote
// (the LDS operations of one wave complete in order), so a compiler-level fence replaces the
// block barrier
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// x = D_{k>>2} C_{k&3} for C_b = c[b-1], D_a = d[a-1] (k = 0 -> 1)
__device__ __forceinline__ f2 tw_pair(const f2 (&c)[3], const f2 (&d)[3], int k) {
    const int a = k >> 2, b = k & 3;
    if (a == 0) return b == 0 ? f2{1.0f, 0.0f} : c[b - 1];
    if (b == 0) return d[a - 1];
    return pmul(d[a - 1], c[b - 1]);
}

// lane pair (2c, 2c + 1) exchange: even lanes lo = a, odd lanes lo = the partner's b; odd lanes
// hi = b, even lanes hi = the partner's a.  Loads: (a, b) = columns (2c, 2c + 1) of row k + 8h ->
// (lo, hi) = rows (k, 8 + k) of column 2c + h.  Stores: (a, b) = rows (k, 8 + k) of column 2c + h
// -> (lo, hi) = columns (2c, 2c + 1) of row k + 8h.  One v_cndmask_b32 with a quad_perm DPP
// operand per dword (the partner's register read in the same instruction); the s_nop covers
// the DPP read-after-VALU-write hazard of an operand the compiler computed just before.
__device__ __forceinline__ void pair_exchange(f2 a, f2 b, f2& lo, f2& hi) {
    float l0, l1, h0, h1;
    asm("s_nop 1\n\t"
        "s_mov_b32 vcc_lo, 0x55555555\n\t"
        "s_mov_b32 vcc_hi, 0x55555555\n\t"
        "v_cndmask_b32_dpp %0, %6, %4, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %1, %7, %5, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_not_b64 vcc, vcc\n\t"
        "v_cndmask_b32_dpp %2, %4, %6, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %3, %5, %7, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
        : "=&v"(l0), "=&v"(l1), "=&v"(h0), "=&v"(h1)
        : "v"(a.x), "v"(a.y), "v"(b.x), "v"(b.y)
        : "vcc");
    lo = f2{l0, l1};
    hi = f2{h0, h1};
}

// ---- real circular kernel g (real taps, real scale): H[N - k] = conj H[k] ----
//
// Bin (k0, k1, k2) = k0 + 16 k1 + 256 k2 mirrors (16 - k0, 15 - k1, 15 - k2) for k0 >= 1, so the
// bins k2 >= 8 of lane (k0, k1) are the conjugates of the bins k2' = 15 - k2 < 8 of lane
// (16 - k0, 15 - k1).  The REALG instances deal the P2 - P4 rows to the lanes so that this mirror
// lane is the lane at the mirrored position of the same 16-lane DPP row: with g = (t >> 4) & 3 and
// j = t & 15, wave w < 3 holds the row pairs (2w + 1, 15 - 2w) in its groups g = 0, 1 and
// (2w + 2, 14 - 2w) in g = 2, 3; in the first group of a pair (a, 16 - a) lanes j < 8 take row a and
// lanes j >= 8 row 16 - a, in the second the reverse.  Wave 3 holds rows 0 and 8 whole (g = 0, 1;
// row 8 mirrors within itself, row 0 is the exception below) and the pair (7, 9).  The index
// within the row stays j, a wave still owns four rows, and the rows of a pair lie an even number
// of rows (a multiple of 2 * 544 dwords) apart, so the LDS bank pattern is the plain layout's.
constexpr int ols_rg_row(int t) {
    const int w = t >> 6, g = (t >> 4) & 3, j = t & 15;
    if (w == 3 && g < 2) return 8 * g;
    const int a = w == 3 ? 7 : 2 * w + 1 + (g >> 1);
    return (g & 1) != (j >> 3) ? 16 - a : a;
}
// the same map for the kernel, without a branch: the rows of the two halves (j < 8, j >= 8) of the
// sixteen 16-lane groups, four bits each, in two 64-bit constants
constexpr unsigned long long ols_rg_pack(int half) {
    unsigned long long v = 0;
    for (int grp = 0; grp < 16; ++grp) v |= (unsigned long long)ols_rg_row(16 * grp + 8 * half) << (4 * grp);
    return v;
}
constexpr int ols_rg_row_packed(int t) {
    return (int)(((t & 8) ? ols_rg_pack(1) : ols_rg_pack(0)) >> (4 * (t >> 4))) & 15;
}
constexpr bool ols_rg_packed_is_the_map() {
    for (int t = 0; t < 256; ++t)
        if (ols_rg_row_packed(t) != ols_rg_row(t)) return false;
    return true;
}
static_assert(ols_rg_packed_is_the_map(), "the packed form is ols_rg_row");
constexpr bool ols_rg_bijective() {
    bool seen[256] = {};
    for (int t = 0; t < 256; ++t) {
        const int r = ols_rg_row(t);
        if (r < 0 || r > 15 || seen[16 * r + (t & 15)]) return false;
        seen[16 * r + (t & 15)] = true;
    }
    return true;
}
constexpr bool ols_rg_four_rows_per_wave() {
    for (int w = 0; w < 4; ++w) {
        int rows = 0, count = 0;
        for (int l = 0; l < 64; ++l) rows |= 1 << ols_rg_row(64 * w + l);
        for (int r = 0; r < 16; ++r) count += (rows >> r) & 1;
        if (count != 4) return false;
    }
    return true;
}
constexpr bool ols_rg_mirror_in_dpp_row() {
    for (int t = 0; t < 256; ++t) {
        const int r = ols_rg_row(t), m = (t & ~15) | (15 - (t & 15));  // row_mirror's source lane
        if (r != 0 && (ols_rg_row(m) != 16 - r || (m & 15) != 15 - (t & 15))) return false;
    }
    return true;
}
static_assert(ols_rg_bijective(), "the lane map covers 16 rows x 16 indices once");
static_assert(ols_rg_four_rows_per_wave(), "P2 - P4 of a wave touch four rows (wave-level hand-offs)");
static_assert(ols_rg_mirror_in_dpp_row(), "row != 0: position 15 - j of the group holds (16 - row, 15 - k1)");

// a * conj(b) with the operations of pmul(a, {b.x, -b.y}), bit for bit: what the boundary
// instance computes from the full table, whose entry is that conjugate
__device__ __forceinline__ f2 pmul_cj(f2 a, f2 b) {
    f2 t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,0]" : "=v"(t) : "v"(a), "v"(b));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] neg_hi:[0,1,0]" : "=v"(r) : "v"(a), "v"(b), "v"(t));
    return r;
}

// The two bins of one k-pair whose spectrum values are the conjugates of the MIRROR lane's pair m
// (halves swapped): r0 = a0 * conj(m.zw), r1 = a1 * conj(m.xy), m read from the lane at the
// mirrored position of the 16-lane row: four v_mov_b32 with a row_mirror DPP operand, then the
// packed products.  (The lab's other form, the products themselves as v_mul / v_fmac with the DPP
// operand and no copy, measured 1.4 % slower: profiles/r08/LAB.md.)  Every lane of the wave must
// be active (a DPP read of an inactive lane writes nothing); the s_nop covers the DPP
// read-after-VALU-write hazard should the compiler have moved m just before.
__device__ __forceinline__ void mirror_products(f2 a0, f2 a1, float4 m, f2& r0, f2& r1) {
    float bx, by, cx, cy;
    asm("s_nop 1\n\t"
        "v_mov_b32_dpp %0, %4 row_mirror row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %1, %5 row_mirror row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %2, %6 row_mirror row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b32_dpp %3, %7 row_mirror row_mask:0xf bank_mask:0xf"
        : "=&v"(bx), "=&v"(by), "=&v"(cx), "=&v"(cy)
        : "v"(m.z), "v"(m.w), "v"(m.x), "v"(m.y));
    r0 = pmul_cj(a0, f2{bx, by});
    r1 = pmul_cj(a1, f2{cx, cy});
}

}  // namespace

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
//   REALG  g is real (OlsPlan::d_hhalf): Hs is the half table, float4 [4][kOlsHalfRow], the rows of
//          P2 - P4 are dealt by ols_rg_row, every lane loads the four k-pairs k2 < 8 of its own
//          (row, k1) and multiplies the bins k2 >= 8 by the conjugates of its mirror lane's, read
//          through DPP (mirror_products): four 16-byte spectrum loads per lane instead of eight.  The 16
//          lanes of row 0, whose mirror (0, 16 - k1) is no DPP partner, load their mirror's four
//          pairs as well (wave 3 only).  Same bits as the full-table form on a table with
//          H[N - k] = conj H[k] exactly (runtime.cpp ols_build makes it so).
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
    const auto rh = __builtin_amdgcn_make_buffer_rsrc((void*)Hs, (short)0, (REALG ? 4 * kOlsHalfRow : 2048) * 16, kBufWord3);
    // twiddle bases: {C1, D1} of column t and {E1, F1} of row lo4 (runtime.cpp ols_build), requested
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
    // the first power of each base from L2, the others as products (W^2 = W W, W^3 = W^2 W)
    f2 Cb[3], Da[3], Eb[3], Fa[3];
    {
        const f2 c1 = f2{cd.x, cd.y}, d1 = f2{cd.z, cd.w}, e1 = f2{ef.x, ef.y}, f1 = f2{ef.z, ef.w};
        const f2 c2 = pmul(c1, c1), d2 = pmul(d1, d1), e2 = pmul(e1, e1), f2_ = pmul(f1, f1);
        Cb[0] = c1, Cb[1] = c2, Cb[2] = pmul(c2, c1);
        Da[0] = d1, Da[1] = d2, Da[2] = pmul(d2, d1);
        Eb[0] = e1, Eb[1] = e2, Eb[2] = pmul(e2, e1);
        Fa[0] = f1, Fa[1] = f2_, Fa[2] = pmul(f2_, f1);
    }
    f2* col = img + t + (t >> 4);  // (r, t) at col[r * kRow]
    const int hi4 = REALG ? ols_rg_row_packed(t) : t >> 4;  // the lane's row in P2 - P4

    // P1: DFT16 n2 -> k0, * W4096^(t k0) -> (k0, t)
    pdft16f<false>(v);
#pragma unroll
    for (int k = 0; k < 16; ++k) col[k * kRow] = k == 0 ? v[0] : pmul(v[kout(k)], tw_pair(Cb, Da, k));
    __syncthreads();

    // P2: lane (k0 = hi4, n0 = lo4): DFT16 n1 -> k1, * W256^(n0 k1) -> (k0, 16 k1 + n0)
    f2* r2 = img + hi4 * kRow + lo4;  // (hi4, 16 j + lo4) at r2[17 j]
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = r2[17 * j];
    float4 hq[8];  // the spectrum slice of lane (k0, k1) for P3, k-pair major
    if constexpr (REALG) {
        // pairs p < 4 of this lane; row 0 alone also pair 7 - p of its mirror (0, 16 - k1) into
        // hq[p], p >= 4 (k1 = 0: the table's tail entry) -- the other lanes never read theirs
#pragma unroll
        for (int p = 0; p < 4; ++p)
            hq[p] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rh, 16 * (16 * hi4 + lo4), 16 * kOlsHalfRow * p, 0));
        if (hi4 == 0) {
            const int ml = lo4 ? 16 - lo4 : 256;
#pragma unroll
            for (int p = 0; p < 4; ++p)
                hq[7 - p] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rh, 16 * ml, 16 * kOlsHalfRow * p, 0));
        }
    } else {
#pragma unroll
        for (int p = 0; p < 8; ++p) hq[p] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rh, 16 * t, 4096 * p, 0));
    }
    f2 w2[16];  // W256^(lo4 k), used by P2 (n0 = lo4) and P3 (k1 = lo4)
#pragma unroll
    for (int k = 1; k < 16; ++k) w2[k] = tw_pair(Eb, Fa, k);
    pdft16f<false>(v);
#pragma unroll
    for (int k = 0; k < 16; ++k) r2[17 * k] = k == 0 ? v[0] : pmul(v[kout(k)], w2[k]);
    wave_sync();

    // P3: lane (k0 = hi4, k1 = lo4) over n0: DFT16 n0 -> k2, * H, IDFT16 k2 -> n0, * conj W256^(k1 n0)
    {
        f2* r3 = img + hi4 * kRow + 17 * lo4;  // (hi4, 16 lo4 + j) at r3[j]
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = r3[j];
        pdft16f<false>(v);
        f2 u[16];
#pragma unroll
        for (int p = 0; p < (REALG ? 4 : 8); ++p) {
            u[2 * p] = pmul(v[kout(2 * p)], f2{hq[p].x, hq[p].y});
            u[2 * p + 1] = pmul(v[kout(2 * p + 1)], f2{hq[p].z, hq[p].w});
        }
        if constexpr (REALG) {
            // bins k2 = 2p, 2p + 1 >= 8: conj of bins 15 - 2p, 14 - 2p (pair 7 - p, halves swapped) of
            // the mirror lane; all lanes first (DPP needs the whole wave), then row 0 over its own
#pragma unroll
            for (int p = 4; p < 8; ++p) mirror_products(v[kout(2 * p)], v[kout(2 * p + 1)], hq[7 - p], u[2 * p], u[2 * p + 1]);
            if (hi4 == 0) {
#pragma unroll
                for (int p = 4; p < 8; ++p) {
                    u[2 * p] = pmul_cj(v[kout(2 * p)], f2{hq[p].z, hq[p].w});
                    u[2 * p + 1] = pmul_cj(v[kout(2 * p + 1)], f2{hq[p].x, hq[p].y});
                }
            }
        }
        pdft16f<true>(u);
#pragma unroll
        for (int j = 0; j < 16; ++j) r3[j] = j == 0 ? u[kout(0)] : pmulc(u[kout(j)], w2[j]);
    }
    wave_sync();

    // P4: lane (k0 = hi4, n0 = lo4): IDFT16 k1 -> n1 -> (k0, 16 n1 + n0)
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = r2[17 * j];
    pdft16f<true>(v);
#pragma unroll
    for (int k = 0; k < 16; ++k) r2[17 * k] = v[kout(k)];
    __syncthreads();

    // P5: lane t: * conj W4096^(t k0), IDFT16 k0 -> n2; row n2 at v[kout(n2)].  The bases are
    // made opaque first so the products are recomputed here rather than kept live from P1.
#pragma unroll
    for (int i = 0; i < 3; ++i) asm volatile("" : "+v"(Cb[i]), "+v"(Da[i]));
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = k == 0 ? col[0] : pmulc(col[k * kRow], tw_pair(Cb, Da, k));
    pdft16f<true>(v);
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

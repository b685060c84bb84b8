// The 4096-point segment transform of the one-shot overlap-save kernels (gfx950), between "rows
// loaded" and "rows ready to store": the single copy that kern_fir_ols_os.hip (c32 streams) and
// kern_fir_ols_real.hip (pairs of real f32 segments) both run, with its helpers, its constants
// and the lane map of the half-spectrum (REALG) form.  Internal to those two translation units;
// the shape of the kernel around it (one segment per 256-thread workgroup, 4 workgroups per CU,
// the phase-aliased 34 KB LDS image, the twiddle bases) is described in kern_fir_ols_os.hip.
//
// LDS image: element (r, c) at r * 272 + c + (c >> 4) (one 8-byte pad per
// 16-column block; rows 544 dwords apart, i.e. opposite halves of the 64
// banks).  Every access is a per-lane base plus a compile-time offset and is
// conflict-free except P5's reads (lanes 0 and 31 of a 32-lane group share a
// bank pair: SQ_LDS_BANK_CONFLICT counts 2 extra cycles per ds_read_b64,
// tools/lds_probe.hip).
#pragma once
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

// The transform between "rows loaded" and "rows ready to store": rows[r] = z(256 r + t) in, row n2
// of the circular convolution with g at rows[kout(n2)] out.  cd = {C1, D1} of column t and
// ef = {E1, F1} of row lo4 = t & 15 (d_ostab; the callers request them ahead of their row loads
// and so hold lo4 already), Hs the spectrum table H/N, img the workgroup's 16 * kRow image, t the
// lane.
//   REALG  g is real (OlsPlan::d_hhalf): Hs is the half table, float4 [4][kOlsHalfRow], the rows of
//          P2 - P4 are dealt by ols_rg_row, every lane loads the four k-pairs k2 < 8 of its own
//          (row, k1) and multiplies the bins k2 >= 8 by the conjugates of its mirror lane's, read
//          through DPP (mirror_products): four 16-byte spectrum loads per lane instead of eight.  The 16
//          lanes of row 0, whose mirror (0, 16 - k1) is no DPP partner, load their mirror's four
//          pairs as well (wave 3 only).  Same bits as the full-table form on a table with
//          H[N - k] = conj H[k] exactly (ols_tables.cpp ols_spectrum makes it so).  Otherwise Hs is
//          the full table, float4 [8][256].
// The form of this function decides the instruction schedule of its callers, their prologues'
// load order included (kern_fir_ols_os.hip), so each of these is load-bearing; with them the c32
// translation unit compiles to the instructions it had with the phases written out in
// ols_os_segment:
//   * the rows are copied into a local array and back.  The copies cost nothing, but a local
//     array becomes registers before the loops over it are unrolled, which lets the compiler
//     compute each DFT output next to the product and the store that consume it; through the
//     reference it computes them in DFT order (2.2 % slower on the default full-table c32
//     instance, profiles/r09/LAB.md);
//   * the table comes as a pointer and its descriptor is made here, lo4 comes from the caller,
//     and hi4 is declared after col.
// A change here is read off the disassembly of both translation units.
template <bool REALG>
__device__ __forceinline__ void ols_os_transform(f2 (&rows)[16], const float4 cd, const float4 ef, const float4* Hs,
                                                 f2* img, int t, int lo4) {
    const auto rh = __builtin_amdgcn_make_buffer_rsrc((void*)Hs, (short)0, (REALG ? 4 * kOlsHalfRow : 2048) * 16, kBufWord3);
    f2 v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = rows[r];
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

    // P5: lane t: * conj W4096^(t k0), IDFT16 k0 -> n2; row n2 at v[kout(n2)] (out: rows).  The bases are
    // made opaque first so the products are recomputed here rather than kept live from P1.
#pragma unroll
    for (int i = 0; i < 3; ++i) asm volatile("" : "+v"(Cb[i]), "+v"(Da[i]));
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = k == 0 ? col[0] : pmulc(col[k * kRow], tw_pair(Cb, Da, k));
    pdft16f<true>(v);
#pragma unroll
    for (int r = 0; r < 16; ++r) rows[r] = v[r];
}

}  // namespace

}  // namespace sdsp

// One-shot, XCD-ordered overlap-save FIR for real f32 streams with real f32 taps (gfx950):
// FIRFilter<f32, f32> under SDSP_ALGO_FFT.
//
// Same filter and the same segmentation as kern_fir_ols_os.hip on 4-byte samples: real segment
// s reads x[s V - H, s V - H + 4096) and writes y[s V, (s + 1) V), H = 256 h2 >= L - 1,
// V = 4096 - H.  With real taps g the circular convolution is linear over the reals,
//     conv(a + i b, g) = conv(a, g) + i conv(b, g),
// so one 4096-point complex transform filters two real windows: pair p packs the adjacent
// segments A = 2p and B = 2p + 1 as z = A + i B, runs the transform of the c32 kernel on z
// (phases P1..P5 below are those of ols_os_segment: pdft16f, the C/D/E/F twiddle bases of
// d_ostab, the spectrum of d_pkt, the 34 KB aliased LDS image, 4 workgroups per CU), and stores
// rows >= h2 of Re to A's outputs and of Im to B's.  The phase code is a copy, not a shared
// header, so that the c32 translation unit stays instruction for instruction what it was.
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
#include "sdsp_device.hpp"
#include "sdsp_kernels.hpp"
#include "sdsp_pk.hpp"

namespace sdsp {

using namespace pk;

namespace {

constexpr int kRow = 272;

constexpr int kBufWord3 = 0x00020000;  // raw buffer descriptor word 3 (gfx9 family)
constexpr int kNT = 2;                 // nontemporal cache policy of a buffer access
constexpr int kOutOfRange = 0x7ffffff0;  // a buffer offset past every descriptor here: loads return 0

typedef unsigned int u2v __attribute__((ext_vector_type(2)));

// see kern_fir_ols_os.hip: P2 -> P3 -> P4 stay inside one wave
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

// lane pair (2c, 2c + 1) exchange of kern_fir_ols_os.hip: even lanes lo = a, odd lanes lo = the
// partner's b; odd lanes hi = b, even lanes hi = the partner's a
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

template <int POL> __device__ __forceinline__ float ld32(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, POL));
}

// The transform between "rows loaded" and "rows ready to store" (P1..P5 of ols_os_segment):
// v[r] = z(256 r + t) in, circular convolution row n2 at v[kout(n2)] out.
__device__ __forceinline__ void ols_real_transform(f2 (&v)[16], const float4 cd, const float4 ef,
                                                   __amdgpu_buffer_rsrc_t rh, f2* img, int t) {
    const int hi4 = t >> 4, lo4 = t & 15;
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

    // P1: DFT16 n2 -> k0, * W4096^(t k0) -> (k0, t)
    pdft16f<false>(v);
#pragma unroll
    for (int k = 0; k < 16; ++k) col[k * kRow] = k == 0 ? v[0] : pmul(v[kout(k)], tw_pair(Cb, Da, k));
    __syncthreads();

    // P2: lane (k0 = hi4, n0 = lo4): DFT16 n1 -> k1, * W256^(n0 k1) -> (k0, 16 k1 + n0)
    f2* r2 = img + hi4 * kRow + lo4;  // (hi4, 16 j + lo4) at r2[17 j]
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = r2[17 * j];
    float4 hq[8];  // the spectrum slice of lane (k0, k1) = t for P3, k-pair major
#pragma unroll
    for (int p = 0; p < 8; ++p) hq[p] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rh, 16 * t, 4096 * p, 0));
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
        for (int p = 0; p < 8; ++p) {
            u[2 * p] = pmul(v[kout(2 * p)], f2{hq[p].x, hq[p].y});
            u[2 * p + 1] = pmul(v[kout(2 * p + 1)], f2{hq[p].z, hq[p].w});
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
    const auto rh = __builtin_amdgcn_make_buffer_rsrc((void*)Hs, (short)0, 2048 * 16, kBufWord3);
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
        ols_real_transform(v, cd, ef, rh, img, t);
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
            ols_real_transform(v, cd, ef, rh, img, t);
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
            ols_real_transform(v, cd, ef, rh, img, t);
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

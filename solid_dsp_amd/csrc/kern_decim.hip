// Column-parallel polyphase decimator (gfx950), SDSP_ALGO_FMA path.
//
// DecimatingFIRFilter (src/filter/fir/decim.rs:115-118, 221-228) emits
//     y[m] = scale * sum_{i<L} cr[i] * ext(j0 + m*M - i),   cr[i] = h[L-1-i]
// With L = K*M, write i = k*M + p and q = M-1-p.  Row rho of the stream is the
// M contiguous samples X[rho][q] = ext(j0 + rho*M - (M-1) + q), so
//     y[m] = scale * sum_{k<K} sum_{q<M} h[(K-1-k)*M + q] * X[m-k][q].
//
// A group of M lanes walks rows in stream order: lane q loads X[rho][q] (one
// coalesced M-sample load per row), keeps its K taps in registers and adds
// tap[k]*X[rho][q] into a ring of K per-output accumulators (output rho+k).
// After row rho the lane's partial for output rho is final; the partials of a
// chunk of CH rows go through an LDS tile [CH][M]; P = M/CH lanes sum one row
// (CH columns each) and combine by lane exchange, so every input sample is read
// from HBM once, touches LDS twice and costs K fused multiply-adds.  Each
// group owns `seg` consecutive outputs and starts K rows early (warm-up,
// outputs discarded); a wave holds G = 64/M groups.
//
// Summation order differs from the reference (phase-major partials, fused
// multiply-add), so this is the FMA path; SDSP_ALGO_EXACT keeps the
// reference-order kernel in kern_fir_direct.hip.  The walk itself (poly_group) lives in
// sdsp_decim_walk.hpp, which the down-converter shares; this unit instantiates it with the
// identity load hook.
#include "sdsp_decim_walk.hpp"
#include "sdsp_device.hpp"
#include "sdsp_kernels.hpp"

namespace sdsp {

namespace {

template <typename C, typename I, int M, int K, int V>
__global__ void __launch_bounds__(kPolyThreads)
decim_poly_kernel(const I* __restrict__ x, const I* __restrict__ hist, const C* __restrict__ cr, C scale,
                  I* __restrict__ y, long long n, long long nout, long long j0, long long seg) {
    using Geo = PolyGeom<I, M, K, V>;
    constexpr int G = Geo::G, CH = Geo::CH, MV = Geo::MV;
    constexpr int L = K * M;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane / MV, q = lane % MV;
    const int ch = blockIdx.y;
    x += (long long)ch * n;
    y += (long long)ch * nout;
    hist += (long long)ch * (L - 1);

    const long long wave_id = (long long)xcd_order(blockIdx.x, gridDim.x) * kPolyWaves + wave;  // XCD-ordered
    const long long gid = wave_id * G + g;
    const long long m_begin = gid * seg;
    if (m_begin >= nout) return;
    const long long m_end = m_begin + seg < nout ? m_begin + seg : nout;

    C tap[K][V];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int e = 0; e < V; ++e) tap[k][e] = cr[k * M + (M - 1 - (q * V + e))];

    char* tile = lds + (wave * G + g) * CH * Geo::RB;
    // wave-uniform interior test over all groups of this wave (rows warm-up .. last chunk)
    const long long first_j = j0 - (M - 1) + (wave_id * G * seg - K) * M;
    const long long last_row = (wave_id * G + G - 1) * seg + (seg + CH - 1) / CH * CH - 1;
    const long long last_j = j0 + last_row * M;
    if (first_j >= 0 && last_j < n)
        poly_group<C, I, M, K, V, true>(x, hist, tap, scale, y, tile, n, L - 1, j0, m_begin, m_end, q,
                                        LoadIdentity{});
    else
        poly_group<C, I, M, K, V, false>(x, hist, tap, scale, y, tile, n, L - 1, j0, m_begin, m_end, q,
                                        LoadIdentity{});
}

template <typename C, typename I, int M, int K, int V>
hipError_t launch_poly_t(const FirArgs& a, hipStream_t s) {
    using Geo = PolyGeom<I, M, K, V>;
    const long long nout = (long long)a.nout;
    const long long seg = poly_seg(a.seg, nout, Geo::CH);  // outputs per group: a multiple of CH
    const long long groups = (nout + seg - 1) / seg;
    const long long waves = (groups + Geo::G - 1) / Geo::G;
    dim3 grid((unsigned)((waves + kPolyWaves - 1) / kPolyWaves), (unsigned)a.channels);
    const size_t lds = (size_t)kPolyWaves * Geo::LDS_WAVE;
    const C scale = *reinterpret_cast<const C*>(a.scale);
    hipLaunchKernelGGL((decim_poly_kernel<C, I, M, K, V>), grid, dim3(kPolyThreads), lds, s, (const I*)a.x,
                       (const I*)a.hist, (const C*)a.taps_rev, scale, (I*)a.y, (long long)a.n, nout,
                       (long long)a.j0, seg);
    return hipGetLastError();
}

template <typename C, typename I, int M, int K>
hipError_t poly_by_v(const FirArgs& a, hipStream_t s) {
    constexpr int VW = sizeof(I) >= 16 ? 1 : 16 / (int)sizeof(I);
    if constexpr (VW > 1) {
        // 16-byte rows: every row start j0 - (M-1) + rho*M a multiple of VW, and 16-byte
        // aligned channel bases
        const bool aligned = (a.j0 + 1) % VW == 0 && (a.channels == 1 || a.n % VW == 0) &&
                             reinterpret_cast<uintptr_t>(a.x) % 16 == 0;
        if (aligned) return launch_poly_t<C, I, M, K, VW>(a, s);
    }
    return launch_poly_t<C, I, M, K, 1>(a, s);
}

template <typename C, typename I, int M>
bool poly_by_k(const FirArgs& a, hipStream_t s, hipError_t* err) {
    switch (a.L / M) {
        case 2: *err = poly_by_v<C, I, M, 2>(a, s); return true;
        case 4: *err = poly_by_v<C, I, M, 4>(a, s); return true;
        case 8: *err = poly_by_v<C, I, M, 8>(a, s); return true;
        case 16: *err = poly_by_v<C, I, M, 16>(a, s); return true;
    }
    return false;
}

template <typename C, typename I>
bool poly_by_m(const FirArgs& a, hipStream_t s, hipError_t* err) {
    constexpr int sz = (int)sizeof(I);
    switch (a.M) {
        case 8: if constexpr (8 * sz >= 32 && 8 * sz <= 256) return poly_by_k<C, I, 8>(a, s, err); break;
        case 16: if constexpr (16 * sz >= 32 && 16 * sz <= 256) return poly_by_k<C, I, 16>(a, s, err); break;
        case 32: if constexpr (32 * sz >= 32 && 32 * sz <= 256) return poly_by_k<C, I, 32>(a, s, err); break;
        case 64: if constexpr (64 * sz >= 32 && 64 * sz <= 256) return poly_by_k<C, I, 64>(a, s, err); break;
    }
    return false;
}

}  // namespace

// true when the column-parallel kernel handles this decimator (FMA path,
// L = K*M with K in {2,4,8,16}, M in {8..64} with an M-sample row of 32..256 bytes)
bool try_launch_decim_poly(int dtype, const FirArgs& a, hipStream_t s, hipError_t* err) {
    if (a.exact || a.M < 8 || a.L % a.M != 0) return false;
    switch (dtype) {
        case 0: return poly_by_m<float, float>(a, s, err);
        case 1: return poly_by_m<float, c32>(a, s, err);
        case 2: return poly_by_m<c32, c32>(a, s, err);
        case 3: return poly_by_m<double, double>(a, s, err);
        case 4: return poly_by_m<double, c64>(a, s, err);
        case 5: return poly_by_m<c64, c64>(a, s, err);
    }
    return false;
}

}  // namespace sdsp

// The decimating FIR's column-parallel polyphase walk (poly_group; FMA path, derivation in
// kern_decim.hip) with a load hook, shared by the decimator (kern_decim.hip) and the
// down-converter (kern_ddc.hip).  kern_decim.hip instantiates it with the identity hook and its
// device code is instruction for instruction what it was before the walk moved here.
//
// Every sample of the call passes through hook.at() between its load and its first use.
// LoadIdentity returns it as it is; the down-converter's hook (LoadNcoMix) multiplies the sample by the
// oscillator's phasor at the sample's stream index.  Samples before the call (index < 0) come from
// the history, which holds what an earlier call already passed through its hook, and are returned
// as they are (CHECK); where the caller knows every index is >= 0 the test is compiled out.
#pragma once
#include "sdsp_device.hpp"
#include "sdsp_nco_dev.hpp"

namespace sdsp {

struct LoadIdentity {
    // once per workgroup, by every thread, after the first loads of the walk are issued
    __device__ __forceinline__ void stage() const {}
    // the sample at stream index jb + off
    template <bool CHECK, typename I> __device__ __forceinline__ I at(I v, long long, int) const { return v; }
};

// NCO mix on load: v * phasor(theta0 + (jb + off) dtheta), the phase formed as nco_one does
// (u32, wrapping; jb dtheta and off dtheta wrap separately to the same sum mod 2^32)
template <typename T> struct LoadNcoMix {
    T* lut;               // LDS, 1024 entries
    const double* table;  // the handle's f64 sine table
    uint32_t theta0, dtheta;
    bool down;
    __device__ __forceinline__ void stage() const {
        for (int i = threadIdx.x; i < 1024; i += blockDim.x) lut[i] = (T)table[i];
        __syncthreads();
    }
    template <bool CHECK, typename I> __device__ __forceinline__ I at(I v, long long jb, int off) const {
        if constexpr (CHECK)
            if (jb + off < 0) return v;
        const uint32_t th = theta0 + (uint32_t)jb * dtheta + (uint32_t)off * dtheta;
        return nco_mix_at(lut, v, th, down);
    }
};

// ---------------------------------------------------------------- column-parallel polyphase walk
template <typename I>
__device__ __forceinline__ I ext_at(const I* __restrict__ x, const I* __restrict__ hist, long long j, long long n,
                                    int Lm1) {
    if (j >= 0) return j < n ? x[j] : zero_v<I>();
    const long long h = (long long)Lm1 + j;
    return h >= 0 ? hist[h] : zero_v<I>();
}

__device__ __forceinline__ float shfl_xor_v(float v, int d) { return __shfl_xor(v, d); }
__device__ __forceinline__ double shfl_xor_v(double v, int d) { return __shfl_xor(v, d); }
template <typename T> __device__ __forceinline__ cpx<T> shfl_xor_v(cpx<T> v, int d) {
    return {__shfl_xor(v.re, d), __shfl_xor(v.im, d)};
}

// streaming (non-temporal) load of a 4/8/16-byte value: the input is read once
template <typename T> __device__ __forceinline__ T nt_load(const T* p) {
    typedef unsigned u1v __attribute__((ext_vector_type(1)));
    typedef unsigned u2v __attribute__((ext_vector_type(2)));
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    T out;
    if constexpr (sizeof(T) == 16) {
        const u4v v = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(p));
        __builtin_memcpy(&out, &v, 16);
    } else if constexpr (sizeof(T) == 8) {
        const u2v v = __builtin_nontemporal_load(reinterpret_cast<const u2v*>(p));
        __builtin_memcpy(&out, &v, 8);
    } else {
        static_assert(sizeof(T) == 4, "nt_load size");
        const u1v v = __builtin_nontemporal_load(reinterpret_cast<const u1v*>(p));
        __builtin_memcpy(&out, &v, 4);
    }
    return out;
}

// V adjacent columns per lane: one 16-byte load per lane and row when the row
// start is 16-byte aligned (V = 16 / sizeof(I)), else one sample per lane.
template <typename I, int V> struct alignas(V * sizeof(I)) IVec {
    I e[V];
};

constexpr int kPolyThreads = 256;
constexpr int kPolyWaves = kPolyThreads / 64;

template <typename I, int M, int K, int V> struct PolyGeom {
    static constexpr int MV = M / V;                      // lanes per group
    static constexpr int G = 64 / MV;                     // groups per wave
    static constexpr int CH = K > MV / 4 ? K : MV / 4;    // rows per reduction chunk
    static constexpr int P = MV > CH ? MV / CH : 1;       // lanes per output in the reduction (<= 4)
    static constexpr int RPL = CH > MV ? CH / MV : 1;     // outputs per lane when CH >= MV
    // one 8-byte slot of padding per row: lane (r, part) of the reduction reads
    // slot r*(MV*sizeof(I)/8 + 1) + part*CH*sizeof(I)/8, distinct mod 32 within a group
    static constexpr int RB = MV * (int)sizeof(I) + 8;
    static constexpr int LDS_WAVE = G * CH * RB;
};

template <typename C, typename I, int M, int K, int V, bool INTERIOR, typename Hook>
__device__ __forceinline__ void poly_group(const I* __restrict__ x, const I* __restrict__ hist,
                                           const C (&tap)[K][V], C scale, I* __restrict__ y,
                                           char* __restrict__ tile, long long n, int Lm1, long long j0,
                                           long long m_begin, long long m_end, int q, const Hook& hook) {
    using Geo = PolyGeom<I, M, K, V>;
    constexpr int CH = Geo::CH, MV = Geo::MV, RB = Geo::RB;
    constexpr int SPC = CH / K;  // K-row steps per chunk
    const long long nchunks = (m_end - m_begin + CH - 1) / CH;
    const long long nsteps = 1 + nchunks * SPC;
    const long long rho0 = m_begin - K;
    // sample index of X[rho][q*V] = jq + rho*M
    const long long jq = j0 - (M - 1) + q * V;

    using Vec = IVec<I, V>;
    I acc[K];
    Vec cur[K], nxt[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = zero_v<I>();

    auto load = [&](Vec (&v)[K], long long rho) {
#pragma unroll
        for (int u = 0; u < K; ++u) {
            const long long j = jq + (rho + u) * M;
            if constexpr (INTERIOR) {
                v[u] = nt_load(reinterpret_cast<const Vec*>(x + j));
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) v[u].e[e] = ext_at(x, hist, j + e, n, Lm1);
            }
        }
    };

    load(cur, rho0);
    // LoadNcoMix::stage() ends in a workgroup barrier, and a kernel reaches it through either
    // instantiation of this function (INTERIOR or not, chosen per wave): the waves of a workgroup
    // then meet the barrier at different program points.  That is sound on this hardware, where
    // s_barrier counts arriving waves and knows no program point, provided every wave of the
    // workgroup arrives exactly once -- which is why the caller lets no wave return early.
    hook.stage();
    for (long long s = 0; s < nsteps; ++s) {
        if (s + 1 < nsteps) load(nxt, rho0 + (s + 1) * K);
        const int trow = (int)((s - 1) % SPC) * K;  // tile row of this step's first row (s >= 1)
        const long long js = jq + (rho0 + s * K) * M;  // sample index of cur[0].e[0]
#pragma unroll
        for (int u = 0; u < K; ++u) {
            // the hook runs here, not at the load: the next step's loads stay in flight across it
#pragma unroll
            for (int e = 0; e < V; ++e) cur[u].e[e] = hook.template at<!INTERIOR>(cur[u].e[e], js, u * M + e);
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int e = 0; e < V; ++e) acc[(u + k) % K] = fmac_(acc[(u + k) % K], tap[k][e], cur[u].e[e]);
            if (s > 0) *reinterpret_cast<I*>(tile + (trow + u) * RB + q * (int)sizeof(I)) = acc[u];
            acc[u] = zero_v<I>();
        }
        if (s > 0 && s % SPC == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const long long c = m_begin + (s / SPC - 1) * CH;
            if constexpr (CH >= MV) {
                // lane q sums whole rows q, q + MV, ...
#pragma unroll
                for (int t = 0; t < Geo::RPL; ++t) {
                    const int r = q + t * MV;
                    const I* row = reinterpret_cast<const I*>(tile + r * RB);
                    I sum = row[0];
#pragma unroll
                    for (int e = 1; e < MV; ++e) sum = add_(sum, row[e]);
                    if (c + r < m_end) y[c + r] = mul_(sum, scale);
                }
            } else {
                // output r = q % CH: lane part q / CH sums columns [part*CH, part*CH+CH),
                // then the P parts combine across lanes q ^ CH, q ^ 2CH
                const int r = q % CH, part = q / CH;
                const I* row = reinterpret_cast<const I*>(tile + r * RB) + part * CH;
                I sum = row[0];
#pragma unroll
                for (int e = 1; e < CH; ++e) sum = add_(sum, row[e]);
#pragma unroll
                for (int d = CH; d < MV; d *= 2) sum = add_(sum, shfl_xor_v(sum, d));
                if (part == 0 && c + r < m_end) y[c + r] = mul_(sum, scale);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
#pragma unroll
        for (int u = 0; u < K; ++u) cur[u] = nxt[u];
    }
}

// outputs per lane group of the polyphase walk: the caller's value, else sized to the call with
// at most 256 (64-256 measured fastest on cfg4; 256 keeps the K warm-up rows per group, re-read
// input, to ~3% of the traffic); always a multiple of the reduction chunk CH
inline long long poly_seg(int seg_arg, long long nout, int CH) {
    long long seg = seg_arg > 0 ? seg_arg : (nout + 8191) / 8192;
    if (seg_arg <= 0 && seg > 256) seg = 256;
    seg = (seg + CH - 1) / CH * CH;
    if (seg < CH) seg = CH;
    return seg;
}

}  // namespace sdsp

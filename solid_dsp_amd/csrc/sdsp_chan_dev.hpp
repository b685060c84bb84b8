// What the fused channeliser kernels share (kern_ichan.hip, kern_oschan.hip, kern_spec.hip): the
// branch sum's step, the oversampled walk's sample fetch and rotation, the LDS budget and the
// launchers' dispatch and chunk rule; and the workgroup size of all three channelisers
// (launch_chan_t in kern_fft.hip too).
#pragma once
#include <type_traits>

#include "sdsp_fft_dev.hpp"

namespace sdsp {

constexpr size_t kChanLdsCap = 128 * 1024;  // what a chunked kernel's frames or samples may take
constexpr size_t kChanLdsAll = 160 * 1024;  // LDS per CU: those plus, where it fits, the twiddle table

// one step of a branch sum: a rounded multiply and a rounded add (-ffp-contract=off)
template <typename T>
__device__ __forceinline__ void chan_mac(c2<T>& acc, T c, c2<T> v) {
    acc.re = acc.re + c * v.re;
    acc.im = acc.im + c * v.im;
}

// sample j of one stream's call: from the block, or from the history ([H], oldest first) when j < 0
template <typename T>
__device__ __forceinline__ c2<T> oschan_sample(const c2<T>* __restrict__ x, const c2<T>* __restrict__ hist,
                                               long long j, long long H) {
    return j >= 0 ? x[j] : hist[H + j];
}

// the rotation of the call's frame f
__device__ __forceinline__ int oschan_shift(int c, long long f, int D, int M) {
    return (int)(((unsigned long long)c + (unsigned long long)(f + 1) * (unsigned long long)D) &
                 (unsigned long long)(M - 1));
}

// lanes per workgroup: 64 below M = 256, M / 4 at 256 and 512, 256 from 1024 up
inline int chan_threads(int M) { return M >= 1024 ? 256 : (M >= 256 ? M / 4 : 64); }

template <int N> using chan_int = std::integral_constant<int, N>;

// f(chan_int<NPT>) -> hipError_t with NPT = M / thr points per lane (M a power of two in [4, 4096])
template <typename F>
hipError_t chan_dispatch_npt(int M, int thr, F f) {
    switch ((M + thr - 1) / thr) {
        case 1: return f(chan_int<1>{});
        case 2: return f(chan_int<2>{});
        case 4: return f(chan_int<4>{});
        case 8: return f(chan_int<8>{});
        case 16: return f(chan_int<16>{});
    }
    return hipErrorInvalidValue;  // not reached
}

// f(chan_int<K>) for K = 1 .. 8 (the depths the streaming analysis kernel has too), f(chan_int<0>) else
template <typename F>
void chan_dispatch_k(int K, F f) {
    switch (K) {
        case 1: f(chan_int<1>{}); break;
        case 2: f(chan_int<2>{}); break;
        case 3: f(chan_int<3>{}); break;
        case 4: f(chan_int<4>{}); break;
        case 5: f(chan_int<5>{}); break;
        case 6: f(chan_int<6>{}); break;
        case 7: f(chan_int<7>{}); break;
        case 8: f(chan_int<8>{}); break;
        default: f(chan_int<0>{}); break;
    }
}

// Frames per workgroup of a chunked kernel.  An automatic chunk (`planned`, no knob) shrinks on a
// block too short to give four workgroups to each of 256 CUs at the planned size, never below
// `least` frames (the chunk's warm-up or fill then doubles the reads at most).  A chunk set by the
// knob is taken as it is.  No chunk is longer than the block.
inline size_t chunk_frames(size_t planned, bool knob_set, size_t frames, size_t streams, size_t least) {
    size_t F = planned;
    if (!knob_set) {
        const size_t spread = (frames * streams + 1023) / 1024;
        if (spread > least) least = spread;
        if (least < F) F = least;
    }
    return F > frames ? frames : F;
}

}  // namespace sdsp

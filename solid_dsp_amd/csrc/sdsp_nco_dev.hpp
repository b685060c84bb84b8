// The NCO's per-sample arithmetic on the device (src/nco/mod.rs:94-172), shared by the mixing
// kernel (kern_rx.hip) and the down-converter's load path (kern_ddc.hip).
//
// theta_i = theta_0 + i * dtheta (u32, wrapping); the phasor is
// (table[(idx + 256) & 1023], table[idx]), idx = ((theta + 2^21) >> 22) & 1023, from the
// f32 / f64 copy of the handle's 1024-entry sine table; mix_up = phasor * x,
// mix_down = conj(phasor) * x (num-complex Mul: every product rounded, no contraction).
#pragma once
#include "sdsp_device.hpp"

namespace sdsp {

template <typename T> __device__ inline cpx<T> conj_(cpx<T> a) { return {a.re, -a.im}; }

template <typename T> __device__ __forceinline__ cpx<T> nco_phasor(const T* lut, uint32_t th) {
    const uint32_t idx = ((th + (1u << 21)) >> 22) & 0x3ffu;
    return {lut[(idx + 256) & 0x3ffu], lut[idx]};
}

template <typename T, bool DOWN>
__device__ __forceinline__ cpx<T> nco_one(const T* lut, cpx<T> v, long long i, uint32_t theta0, uint32_t dtheta) {
    const uint32_t th = theta0 + (uint32_t)i * dtheta;  // wrapping u32: theta_0 + i dtheta mod 2^32
    cpx<T> ph = nco_phasor(lut, th);
    if constexpr (DOWN) ph = conj_(ph);
    return mul_(ph, v);
}

// the same product with the direction as a (wave-uniform) run-time flag: the conjugate is a sign
// flip of the sine, so both directions round exactly as nco_one<T, DOWN> does
template <typename T> __device__ __forceinline__ cpx<T> nco_mix_at(const T* lut, cpx<T> v, uint32_t th, bool down) {
    cpx<T> ph = nco_phasor(lut, th);
    if (down) ph.im = -ph.im;
    return mul_(ph, v);
}

}  // namespace sdsp

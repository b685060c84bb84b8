// Polyphase filterbank / interpolating FIR kernel (gfx950).
//
// PolyPhaseFilterBank (src/filter/fir/pfb.rs:24-90): branch p holds
// cb[p][i] = h[p + (K-1-i) M] (stored FORWARD after the in-place reversal at
// pfb.rs:33-40) and execute(p) = sum_{i<K} cb[p][i] * w[i] over the shared
// newest-first Window(K) — no scale.  InterpolatingFIRFilter::execute_block
// (src/filter/fir/interp.rs:102-111) pushes each input and emits all M
// branches, so
//     out[j*M + p] = sum_{i<K} cb[p][i] * x[j-i]
// Three kernels, same sums: interp_tile_kernel (M = 2^m, K in {4, 8, 16}, the
// interpolator shape), pfb_stage_kernel (every other shape whose tile fits in
// LDS) and pfb_kernel (one lane per output, the fallback for very long
// branches).  Summation order is the reference's (EXACT) or fused.
#include "sdsp_device.hpp"
#include "sdsp_kernels.hpp"
#include "sdsp_pfb_walk.hpp"

namespace sdsp {

// The kernels live in sdsp_pfb_walk.hpp (shared with the up-converter, kern_duc.hip); here their
// store hook is the identity.
template <typename C, typename I>
hipError_t launch_pfb_t(const PfbArgs& a, hipStream_t s) {
    return pfb_route<C, I, StoreIdentity>(a, StoreIdentity::Args{}, s);
}

hipError_t launch_pfb(int dtype, const PfbArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    switch (dtype) {
        case 0: return launch_pfb_t<float, float>(a, s);
        case 1: return launch_pfb_t<float, c32>(a, s);
        case 2: return launch_pfb_t<c32, c32>(a, s);
        case 3: return launch_pfb_t<double, double>(a, s);
        case 4: return launch_pfb_t<double, c64>(a, s);
        case 5: return launch_pfb_t<c64, c64>(a, s);
    }
    return hipErrorInvalidValue;
}

// ---- synthetic stream (build-defined generator) ---------------
__device__ inline uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__global__ void synth_kernel(float* __restrict__ out, uint64_t key, uint64_t start, long long count) {
    const uint64_t g = 0x9E3779B97F4A7C15ULL;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += stride) {
        const uint64_t v = mix64(key + (start + (uint64_t)j + 1) * g);
        out[j] = (float)(v >> 40) * (1.0f / 16777216.0f) * 2.0f - 1.0f;
    }
}

hipError_t launch_synth_f32(float* out, uint64_t seed, uint64_t channel, uint64_t start, size_t count,
                            hipStream_t s) {
    if (count == 0) return hipSuccess;
    const uint64_t key = seed ^ (channel * 0x9E3779B97F4A7C15ULL);
    long long blocks = ((long long)count + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(synth_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, key, start, (long long)count);
    return hipGetLastError();
}

}  // namespace sdsp

namespace sdsp {
// ---- STREAM-style copy used to calibrate achievable HBM bandwidth ----------
// One-shot grid, one 16-byte vector per lane: the fastest copy shape measured
// on the box (tools/bw_probe.hip: 6.3 TB/s read + write vs 5.0-5.9 for
// persistent grid-stride copies).
__global__ void __launch_bounds__(256) bw_copy_kernel(const float4* __restrict__ a, float4* __restrict__ b,
                                                      long long n16) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) b[i] = a[i];
}
hipError_t launch_bw_copy(const void* a, void* b, size_t bytes, int num_cus, hipStream_t s) {
    (void)num_cus;
    const long long n16 = (long long)(bytes / 16);
    if (n16 == 0) return hipSuccess;
    const long long blocks = (n16 + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bw_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float4*)a, (float4*)b, n16);
    return hipGetLastError();
}
}  // namespace sdsp

// Digital up-converter (gfx950): the NCO's mix-up on the store path of the interpolating FIR.
//
// A DUC handle is by definition the composition, sample for sample,
//     y = interpolator.execute(x[j]);  out[j*M + p] = nco.mix_up(y[p]); nco.step()
// (src/filter/fir/interp.rs:93-111 into src/nco/mod.rs:94-172).  The oscillator is a pure function
// of the output's index in the call, theta_0 + o * dtheta mod 2^32, so the interpolated stream is
// never written: each kernel here multiplies a finished dot product by its phasor between the
// last add of the sum and the store.  Stream traffic is the interpolator's own, 8 + 8/M bytes per
// c32 output; the only addition is the f32 / f64 copy of the 1024-entry sine table each workgroup
// stages in LDS (4 / 8 KB) ahead of the barrier the walks already have.  The window holds unmixed
// inputs, so the interpolator's window update serves as it is.
//
// Shared, not copied: the three kernels and their selection rule are those of kern_pfb.hip
// (sdsp_pfb_walk.hpp), instantiated here with the StoreNcoMix hook; kern_pfb.hip instantiates them
// with the identity and its generated code is unchanged.  The mix is nco_mix_at's product
// (num-complex roundings; this unit is built with -ffp-contract=off, so it does not contract with
// the sum's last multiply-add), hence EXACT is bit-identical to the EXACT interpolator followed by
// the NCO handle, and FMA to the FMA interpolator followed by it.
//
// The direction is a run-time flag (mix_down differs by one conjugate, a sign flip of the sine).
#include "sdsp_device.hpp"
#include "sdsp_kernels.hpp"
#include "sdsp_nco_dev.hpp"
#include "sdsp_pfb_walk.hpp"

namespace sdsp {

namespace {

// the staged kernel's dynamic tile (at most kPfbStageBytes) and the sine table share the 64 KB a
// workgroup may hold
static_assert(kPfbStageBytes + 1024 * sizeof(double) <= 64 * 1024, "stage tile + sine table exceed LDS");

template <typename C, typename T>
hipError_t launch_duc_t(const DucArgs& d, hipStream_t s) {
    using Hook = StoreNcoMix<T>;
    return pfb_route<C, cpx<T>, Hook>(d.pfb, typename Hook::Args{d.table, d.theta0, d.dtheta, d.down}, s);
}

}  // namespace

hipError_t launch_duc(int dtype, const DucArgs& d, hipStream_t s) {
    if (d.pfb.n == 0) return hipSuccess;
    switch (dtype) {
        case 1: return launch_duc_t<float, float>(d, s);
        case 2: return launch_duc_t<c32, float>(d, s);
        case 4: return launch_duc_t<double, double>(d, s);
        case 5: return launch_duc_t<c64, double>(d, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace sdsp

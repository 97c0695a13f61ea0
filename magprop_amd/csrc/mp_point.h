// mp_point.h — the shell of a device-resident driver's kernel: one workgroup that evaluates, with walker_eval, a point its lane 0
// parked in LDS (opt_trial_kernel, nm_eval_kernel, nest_walk_kernel, nest_slice_kernel; the host side is launch_point_kernel of
// mp_device.h).  What such a kernel evaluates, and so whether it stays equal bit for bit to mp_lnprob_batch, is stated here once
// (nest_walk_kernel restates point_eval's block, for speed: mp_nest.hip says why).
#pragma once
#include "mp_eval.hpp"

namespace mp {

// The attributes of a kernel on the builds of launch_lnprob, `template <int SPL, bool LONG, int W = 1, int OCC = 0>`: W = 4
// wavefronts per point with SPL = 1 step per lane, made for OCC = 1 or 2 wavefronts per SIMD (lnprob_team_kernel<1, 4, OCC>), or
// W = 1 with SPL = 4 steps per lane and one wavefront per SIMD, or SPL = 2 and two (lnprob_kernel<false, SPL>); LONG: handles with
// light curves of more than 64 points.  The launcher picks among them by the launch's workgroup count (launch_point_kernel; the
// sampler's stretch_kernel and stretch_step_kernel, which carry the same line, by stretch_waves of a whole step).
#define MP_POINT_KERNEL(SPL, W, OCC) \
    __global__ __launch_bounds__(64 * (W)) \
    __attribute__((amdgpu_waves_per_eu((W) > 1 ? (OCC) : ((SPL) >= 4 ? 1 : 2), (W) > 1 ? (OCC) : ((SPL) >= 4 ? 1 : 2))))

// The LDS of walker_eval in such a kernel: declare `__shared__ PointLds<SPL, W> ws` and call tables_init<SPL * W, 64 * W>(sh, ws.tt)
// once, with every thread, before the first point_eval.
template <int SPL, int W>
struct PointLds {
    TileImage<SPL * W> im;
    TimeTable<SPL * W> tt;
    double lds[1];
    TeamLds<SPL * W, (W > 1)> tl;
};

// The log-posterior (and status) of the point parked[0 .. ndim) in LDS, by the whole workgroup, behind the barrier that published
// it: the arithmetic of mp_lnprob_batch for sampler coordinates with dataset ds_id[walker], NaN counted (and kept) as -inf.
// target 1: the isotropic unit Gaussian, 2: the same on terraces along x_0 (ties and shrinks) -- unfused, for the tests of the
// algorithms themselves.  Every thread gets lnp and status; the coordinates live in registers in here only, so nothing of them
// stays live in the caller across walker_eval, which needs every register.
template <int SPL, bool LONG, int W, int OCC>
MP_DEV void point_eval(const DevShared &sh, PointLds<SPL, W> &ws, const int32_t *ds_id, int ndim, int target, int walker,
                       const double *parked, double &lnp, int &status) {
    double par[MP_MAX_NDIM];
#pragma unroll
    for (int d = 0; d < MP_MAX_NDIM; ++d) par[d] = d < ndim ? parked[d] : 0.0;
    lnp = 0.0;
    status = MP_STATUS_OK;
    if (target != 0) {
#pragma unroll
        for (int d = 0; d < MP_MAX_NDIM; ++d) lnp = d < ndim ? sub_rn(lnp, mul_rn(mul_rn(0.5, par[d]), par[d])) : lnp;
        if (target == 2) lnp = sub_rn(lnp, mul_rn(1.0e-3, floor(mul_rn(37.0, par[0]))));
    } else {
        int sweeps, tiles;
        LaunchArgs a{};
        a.ds_id = ds_id;
        a.ndim = ndim;
        a.physical = 0;
        a.want_chi2 = 1;
        if constexpr (W > 1) walker_eval<false, SPL, LONG, false, W, OCC >= 2>(sh, a, walker, par, ws.im, ws.tt, ws.lds, lnp, status, sweeps, tiles, ws.tl.ptr());
        else walker_eval<false, SPL, LONG>(sh, a, walker, par, ws.im, ws.tt, ws.lds, lnp, status, sweeps, tiles);
    }
    if (lnp != lnp) lnp = -INFINITY;
}

}  // namespace mp

// mp_flows.hip — gfx950 kernels behind mp_model_flows and mp_model_flow_band (include/magprop_amd.h; the arguments and the order
// of the sums are stated in mp_flows.h): the radii, mass-flow rates and torques of the model along a finished trajectory, and
// their reduction to a mass budget, an angular-momentum budget and the propeller / accretor regime of every row.
//
// flow_cells_kernel is elementwise over rows x n_grid.  A workgroup of 256 threads takes 512 consecutive grid points of ONE row
// (blockIdx.y), a lane two consecutive points, so that every curve is read and written with one 16-byte access per lane and
// consecutive lanes sit on consecutive pairs (a row that does not start on a 16-byte boundary -- every other row of an odd
// grid -- falls back to 8-byte accesses; which points a lane owns never depends on the address, so a row's cells do not depend
// on where the row sits).  The per-row constants come from walker_setup, the function the curve kernels call on the same
// parameter row; the physics is disc_point, flow_state (with cfg.n_ode: the flows describe the integrated system) and mdot_fb of
// mp_eval.hpp, nothing restated.  flow_state votes over the wavefront, so whole wavefronts run: lanes behind the row's end repeat
// its last point and store nothing.
//
// flow_reduce_kernel takes one row per workgroup of 256 threads.  Five passes of the segment walk of mp_segwalk.h (the sums of
// MDOT_FB, MDOT_PROP, MDOT_ACC, N_ACC, N_DIP), then one pass with thread k on points k, k + 256, ... for the counts, the first
// and last indices and the extrema, none of which depends on the order of the visit.
#include <hip/hip_runtime.h>

#include <climits>

#include "mp_eval.hpp"
#include "mp_flows.h"
#include "mp_segwalk.h"
#include "mp_wg.h"

namespace mp {

namespace {

static_assert(kFlowLane == 2, "a lane of flow_cells_kernel owns one 16-byte pair of every curve");
typedef double flow_d2 __attribute__((ext_vector_type(2)));

__device__ inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// the pair (j, j + 1) of a row; have1: j + 1 is a point of the row (else both indices are the row's last point)
__device__ inline void load2(const double *row, int j0, int j1, bool vec, double &x0, double &x1) {
    if (vec) {
        const flow_d2 v = *reinterpret_cast<const flow_d2 *>(row + j0);
        x0 = v.x;
        x1 = v.y;
    } else {
        x0 = row[j0];
        x1 = row[j1];
    }
}
__device__ inline void store2(double *row, int j0, bool have0, bool have1, double x0, double x1) {
    if (have1 && aligned16(row)) {
        flow_d2 v;
        v.x = x0;
        v.y = x1;
        *reinterpret_cast<flow_d2 *>(row + j0) = v;
    } else {
        if (have0) row[j0] = x0;
        if (have1) row[j0 + 1] = x1;
    }
}

__global__ __launch_bounds__(kFlowThreads) void flow_cells_kernel(const DevShared sh, const FlowCellsArgs a) {
    const int row = blockIdx.y;
    const int G = a.n_grid;
    const int j0 = 2 * (blockIdx.x * kFlowThreads + threadIdx.x);
    const bool have0 = j0 < G, have1 = j0 + 1 < G;
    const size_t off = (size_t)row * (size_t)G;
    if (a.status[row] != MP_STATUS_OK) {                     // (uniform over the workgroup)
        const double nan = __builtin_nan("");
#pragma unroll
        for (int c = 0; c < MP_FLOW_NCURVES; ++c)
            if (a.cell[c]) store2(a.cell[c] + off, j0, have0, have1, nan, nan);
        return;
    }
    ktab_init();
    // lanes behind the end repeat the row's last point (wave-wide votes inside flow_state)
    const int c0 = min(j0, G - 1), c1 = min(j0 + 1, G - 1);
    double par[MP_MAX_NDIM];
#pragma unroll
    for (int k = 0; k < MP_MAX_NDIM; ++k) par[k] = k < a.ndim ? a.pars[(size_t)row * a.ndim + k] : 0.0;
    LaunchArgs la{};
    la.ndim = a.ndim;
    la.physical = a.physical;
    Walker w;
    (void)walker_setup(sh, la, par, w);                      // (a row outside the prior has a status that is not OK)

    Vd<2> M, om, t;
    const double *mrow = a.mdisc + off, *orow = a.omega + off, *trow = a.t + (size_t)row * (size_t)a.t_row_stride;
    load2(mrow, c0, c1, have1 && aligned16(mrow), M[0], M[1]);
    load2(orow, c0, c1, have1 && aligned16(orow), om[0], om[1]);
    load2(trow, c0, c1, have1 && aligned16(trow), t[0], t[1]);

    const DiscPt<2> p = disc_point(sh, w, M);
    const Flow<2> f = flow_state(w, sh.cfg.n_ode, p, om);
    const Vd<2> fb = mdot_fb(w, t);
    Vd<2> u, irm;
#pragma unroll
    for (int i = 0; i < 2; ++i) { const double x = om[i] * sh.inv_sqrtGM; u[i] = x * x; }   // omega^2 / GM
    const Vd<2> rc = rcbrt_fast(u);                          // (GM / omega^2)^(1/3)
    const bool alt = sh.cfg.dipole_torque == 1;
    if (alt) irm = rcp_fast(f.Rm);
    double rlc[2], prop[2], acc[2], nacc[2], ndip[2], br[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        rlc[i] = kC * f.inv_om[i];
        // eta2 = (1 + tanh x) / 2 and eta1 = (1 - tanh x) / 2 from e = exp(-2 |x|), r = 1 / (1 + e), as the luminosity stage forms eta2
        const double small = f.e[i] * f.r[i], large = f.r[i];
        const double eta2 = f.th[i] >= 0.0 ? large : small;
        const double eta1 = f.th[i] >= 0.0 ? small : large;
        prop[i] = eta2 * p.mdot[i];
        acc[i] = eta1 * p.mdot[i];
        // the accretion torque by the ODE's rule (omega_rhs): arm sqrt(GM max(Rm, R)), Mdot_acc - Mdot_prop = -tanh(x) Mdisc / tvisc,
        // nothing beyond break-up
        const double rot = sh.crot * (om[i] * om[i]);
        const double arm = sh.sqrtGM * fmax(f.sq[i], sh.sqrtR);
        nacc[i] = rot > 0.27 ? 0.0 : -(arm * p.mdot[i]) * f.th[i];
        if (alt) {
            const double cr = kC * irm[i];                   // c / Rm
            ndip[i] = -4.0 * w.D * (cr * cr * cr);           // -(2/3) mu^2 / Rm^3
        } else {
            ndip[i] = -(w.D * (om[i] * om[i])) * om[i];
        }
        br[i] = (double)((f.capped[i] ? 1 : 0) | (f.big[i] ? 2 : 0));
    }
    const auto put = [&](int c, double x0, double x1) {
        if (a.cell[c]) store2(a.cell[c] + off, j0, have0, have1, x0, x1);
    };
    put(MP_FLOW_CURVE_RM, f.Rm[0], f.Rm[1]);
    put(MP_FLOW_CURVE_RC, rc[0], rc[1]);
    put(MP_FLOW_CURVE_RLC, rlc[0], rlc[1]);
    put(MP_FLOW_CURVE_FASTNESS, f.fast[0], f.fast[1]);
    put(MP_FLOW_CURVE_MDOT_PROP, prop[0], prop[1]);
    put(MP_FLOW_CURVE_MDOT_ACC, acc[0], acc[1]);
    put(MP_FLOW_CURVE_MDOT_FB, fb[0], fb[1]);
    put(MP_FLOW_CURVE_N_ACC, nacc[0], nacc[1]);
    put(MP_FLOW_CURVE_N_DIP, ndip[0], ndip[1]);
    put(MP_FLOW_CURVE_BRANCH, br[0], br[1]);
}

__global__ __launch_bounds__(kFlowThreads) void flow_reduce_kernel(const FlowReduceArgs a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    __shared__ double lc[kSlots], lt[kSlots];
    __shared__ double tot[kFlowThreads];       // segment totals of the curve being summed
    __shared__ double res[MP_FLOW_N];
    __shared__ double rv[kWaves];
    __shared__ int ri[kWaves];
    __shared__ uint32_t rn[kWaves];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int G = a.n_grid, seg = derive_seg(G);
    double *out = a.out + (size_t)row * MP_FLOW_N;
    if (a.status[row] != MP_STATUS_OK) {       // (uniform over the workgroup)
        if (tid < MP_FLOW_N) out[tid] = __builtin_nan("");
        return;
    }
    const size_t off = (size_t)row * (size_t)G;
    const double *t = a.tgrid;
    const double *fast = a.cell[MP_FLOW_CURVE_FASTNESS] + off, *rm = a.cell[MP_FLOW_CURVE_RM] + off,
                 *branch = a.cell[MP_FLOW_CURVE_BRANCH] + off;

    // the five budgets: segment sums, then the segment totals in segment order
    const int summed[5] = {MP_FLOW_CURVE_MDOT_FB, MP_FLOW_CURVE_MDOT_PROP, MP_FLOW_CURVE_MDOT_ACC, MP_FLOW_CURVE_N_ACC, MP_FLOW_CURVE_N_DIP};
    const int column[5] = {MP_FLOW_M_FB, MP_FLOW_M_PROP, MP_FLOW_M_ACC, MP_FLOW_J_ACC, MP_FLOW_J_DIP};
    for (int q = 0; q < 5; ++q) {
        double s;
        Best unused;
        walk<true, false, false>(a.cell[summed[q]] + off, t, G, seg, lc, lt, s, unused, 0.0, nullptr, nullptr);
        tot[tid] = s;
        __syncthreads();
        if (tid == 0) {
            double e = 0.0;
            for (int k = 0; k < kFlowThreads; ++k) e = e + tot[k];
            res[column[q]] = e;
        }
        __syncthreads();
    }

    // counts, first and last indices, extrema: thread k on points k, k + 256, ...
    uint32_t n_prop = 0, n_switch = 0, n_capped = 0, n_inside = 0;
    int first = INT_MAX, last_neg = INT_MAX;   // (the last index as the least of the negated ones)
    Best wmax{-INFINITY, INT_MAX}, rmin{-INFINITY, INT_MAX};   // rmin: of -RM
    for (int i = tid; i < G; i += kFlowThreads) {
        const double w = fast[i];
        const bool prop = w >= 1.0;
        if (prop) {
            ++n_prop;
            first = min(first, i);
            last_neg = min(last_neg, -i);
        }
        if (i + 1 < G) n_switch += prop != (fast[i + 1] >= 1.0) ? 1u : 0u;
        const int b = (int)branch[i];
        n_capped += (b & 1) ? 1u : 0u;
        n_inside += (b & 2) ? 0u : 1u;
        if (wg_better(w, i, wmax.v, wmax.i)) { wmax.v = w; wmax.i = i; }
        const double nr = -rm[i];
        if (wg_better(nr, i, rmin.v, rmin.i)) { rmin.v = nr; rmin.i = i; }
    }
    n_prop = wg_count(n_prop, rn);
    n_switch = wg_count(n_switch, rn);
    n_capped = wg_count(n_capped, rn);
    n_inside = wg_count(n_inside, rn);
    first = wg_least(first, ri);
    last_neg = wg_least(last_neg, ri);
    wmax = wg_best(wmax, rv, ri);
    rmin = wg_best(rmin, rv, ri);
    if (tid == 0) {
        const double nan = __builtin_nan("");
        const bool have_w = wmax.i != INT_MAX, have_r = rmin.i != INT_MAX;   // (false: nothing but NaN in the curve)
        res[MP_FLOW_W_MAX] = have_w ? wmax.v : nan;
        res[MP_FLOW_T_W_MAX] = have_w ? t[wmax.i] : nan;
        res[MP_FLOW_W_END] = fast[G - 1];
        res[MP_FLOW_N_PROP] = (double)n_prop;
        res[MP_FLOW_T_PROP_FIRST] = first != INT_MAX ? t[first] : nan;
        res[MP_FLOW_T_PROP_LAST] = last_neg != INT_MAX ? t[-last_neg] : nan;
        res[MP_FLOW_N_SWITCH] = (double)n_switch;
        res[MP_FLOW_N_CAPPED] = (double)n_capped;
        res[MP_FLOW_N_INSIDE] = (double)n_inside;
        res[MP_FLOW_RM_MIN] = have_r ? -rmin.v : nan;
        res[MP_FLOW_T_RM_MIN] = have_r ? t[rmin.i] : nan;
    }
    __syncthreads();
    if (tid < MP_FLOW_N) out[tid] = res[tid];
}

}  // namespace

int launch_flow_cells(const DevShared &sh, const FlowCellsArgs &a, void *stream) {
    if (a.rows <= 0) return 0;
    if (a.rows > 65535 || a.n_grid < 1) return (int)hipErrorInvalidValue;   // (rows are the grid's y dimension)
    const int pairs = (a.n_grid + kFlowLane - 1) / kFlowLane;
    const dim3 grid((unsigned)((pairs + kFlowThreads - 1) / kFlowThreads), (unsigned)a.rows);
    hipLaunchKernelGGL(flow_cells_kernel, grid, dim3(kFlowThreads), 0, (hipStream_t)stream, sh, a);
    return (int)hipGetLastError();
}

int launch_flow_reduce(const FlowReduceArgs &a, void *stream) {
    if (a.rows <= 0) return 0;
    hipLaunchKernelGGL(flow_reduce_kernel, dim3((unsigned)a.rows), dim3(kFlowThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mp

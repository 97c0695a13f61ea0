// mp_opt.hip — gfx950 kernels of the differential-evolution optimizer (include/magprop_amd.h mp_optimizer_*): scipy's
// differential_evolution with deferred updating, one launch per generation.
//
// opt_trial_kernel: one workgroup per member, on the shell of mp_point.h.  Lane 0 builds the member's trial vector from the
// population of the previous generation (OptArgs::pop_cur) in LDS, the workgroup evaluates it (point_eval), lane 0 decides (greedy)
// and writes the member's row of the next generation (pop_next).  Nothing is written that another workgroup of the launch reads, so
// the workgroups need no hand-off among themselves.  Generation 0 runs the same builds on the population as it is.
// opt_reduce_kernel: one workgroup per population behind every generation: the best member, scipy's stop rule, the counters.
#include <hip/hip_runtime.h>

#include "mp_point.h"

namespace mp {

namespace {

// uniform j of member `member` of population `pop` in generation o.gen (the layout of include/magprop_amd.h)
MP_DEV double opt_u(const OptArgs &o, int pop, int member, int j) {
    uint32_t r[4];
    philox4x32_10((uint32_t)o.seed, (uint32_t)(o.seed >> 32), o.gen, (uint32_t)pop, (uint32_t)member, 0xDE00u + (uint32_t)(j >> 1), r);
    return (j & 1) ? u01(r[2], r[3]) : u01(r[0], r[1]);
}

// The trial vector of member i of population p into t[0 .. ndim) (lane 0 only; runtime loops over the coordinates: t is LDS).
MP_DEV void opt_build_trial(const OptArgs &o, int p, int i, double *t) {
    const int base = p * o.popsize, m = o.popsize - 1, nd = o.ndim;
    const int a0 = pick(opt_u(o, p, i, 0), m);
    const int a1 = pick_skip(opt_u(o, p, i, 1), m, a0);
    const int a2 = pick_skip2(opt_u(o, p, i, 2), m, a0, a1);
    const int r0 = base + a0 + (a0 >= i), r1 = base + a1 + (a1 >= i), r2 = base + a2 + (a2 >= i);
    uint32_t rf[4];
    philox4x32_10((uint32_t)o.seed, (uint32_t)(o.seed >> 32), o.gen, 0xFFFFu, 0u, 0xDEFFu, rf);
    const double F = add_rn(o.f_lo, mul_rn(sub_rn(o.f_hi, o.f_lo), u01(rf[0], rf[1])));
    const bool best1 = o.strategy == MP_DE_BEST1BIN;
    const double *xb = o.pop_cur + (size_t)(best1 ? base + o.best[p] : r0) * nd;
    const double *x1 = o.pop_cur + (size_t)(best1 ? r0 : r1) * nd;
    const double *x2 = o.pop_cur + (size_t)(best1 ? r1 : r2) * nd;
    const double *xi = o.pop_cur + (size_t)(base + i) * nd;
    const int fill = pick(opt_u(o, p, i, 3), nd);
    for (int d = 0; d < nd; ++d) {
        double v = (d == fill || opt_u(o, p, i, 4 + d) < o.cr) ? add_rn(xb[d], mul_rn(F, sub_rn(x1[d], x2[d]))) : xi[d];
        if (!(v >= o.lower[d] && v <= o.upper[d])) v = add_rn(o.lower[d], mul_rn(opt_u(o, p, i, 4 + nd + d), sub_rn(o.upper[d], o.lower[d])));
        t[d] = v;
    }
}

// The builds of mp_point.h for the launch's n_pops * popsize members (launch_opt_trial).
template <int SPL, bool LONG, int W = 1, int OCC = 0>
MP_POINT_KERNEL(SPL, W, OCC) void opt_trial_kernel(const DevShared sh, const OptArgs o) {
    const int k = (int)blockIdx.x, p = k / o.popsize, i = k - p * o.popsize;
    if (o.trial && o.converged[p]) return;   // frozen population (uniform for the workgroup): nothing to do
    __shared__ PointLds<SPL, W> ws;
    __shared__ double park[MP_MAX_NDIM];     // the member's trial (generation 0: the member itself) across the evaluation
    tables_init<SPL * W, 64 * W>(sh, ws.tt);
    if (threadIdx.x == 0) {
        if (o.trial) opt_build_trial(o, p, i, park);
        else for (int d = 0; d < o.ndim; ++d) park[d] = o.pop_cur[(size_t)k * o.ndim + d];
    }
    __syncthreads();
    double lnp;
    int status;
    point_eval<SPL, LONG, W, OCC>(sh, ws, o.ds_id, o.ndim, o.target, k, park, lnp, status);
    if (threadIdx.x == 0) {
        const bool take = !o.trial || lnp >= o.lnp_cur[k];
        const double *src = take ? park : o.pop_cur + (size_t)k * o.ndim;
        for (int d = 0; d < o.ndim; ++d) o.pop_next[(size_t)k * o.ndim + d] = src[d];
        o.lnp_next[k] = take ? lnp : o.lnp_cur[k];
        o.st_next[k] = take ? status : o.st_cur[k];
    }
}

// Behind a generation (o.trial = 1) or the initial evaluation (o.trial = 0), on the new generation (the next buffers): the best
// member (largest lnprob, lowest index on ties), nfev += popsize, and for a generation nit += 1 and the stop rule
// std(E) <= atol + tol |mean(E)|, E = -lnprob, sums in member order (one thread: include/magprop_amd.h states the arithmetic).
// A population that converges gets its final state copied into the cur buffers as well, so that it stays frozen whichever
// buffer the host hands the next launches as cur.
__global__ __launch_bounds__(64) void opt_reduce_kernel(const OptArgs o) {
    const int p = (int)blockIdx.x;
    if (o.converged[p]) return;
    const int base = p * o.popsize;
    __shared__ int conv;
    if (threadIdx.x == 0) {
        const double *lnp = o.lnp_next + base;
        int b = 0;
        bool finite = true;
        double s = 0.0;
        for (int i = 0; i < o.popsize; ++i) {
            const double v = lnp[i];
            if (v > lnp[b]) b = i;
            finite = finite && v > -INFINITY;
            s = add_rn(s, -v);
        }
        const double mean = s / (double)o.popsize;
        double q = 0.0;
        for (int i = 0; i < o.popsize; ++i) {
            const double e = sub_rn(-lnp[i], mean);
            q = add_rn(q, mul_rn(e, e));
        }
        const double sd = sqrt(q / (double)o.popsize);
        const bool c = o.trial && finite && sd <= add_rn(o.atol, mul_rn(o.tol, fabs(mean)));
        o.best[p] = b;
        o.nfev[p] += o.popsize;
        if (o.trial) o.nit[p] += 1;
        o.converged[p] = c ? 1 : 0;
        conv = c;
    }
    __syncthreads();
    if (conv) {
        for (int j = (int)threadIdx.x; j < o.popsize * o.ndim; j += 64) o.pop_cur[(size_t)base * o.ndim + j] = o.pop_next[(size_t)base * o.ndim + j];
        for (int j = (int)threadIdx.x; j < o.popsize; j += 64) {
            o.lnp_cur[base + j] = o.lnp_next[base + j];
            o.st_cur[base + j] = o.st_next[base + j];
        }
    }
}

}  // namespace

// One workgroup per member: n = n_pops * popsize, fixed for the whole run, converged populations or not.  (The experiments
// build's two-wavefront team, force_waves = 2, has no build here: one wavefront there.)
int launch_opt_trial(const DevShared &sh, const OptArgs &o, void *stream) {
    const int n = o.popsize * o.n_pops;
    if (n <= 0) return 0;
    return launch_point_kernel(sh, n, [&](auto build, auto lng) {
        using B = decltype(build);
        hipLaunchKernelGGL((opt_trial_kernel<B::SPL, lng, B::W, B::OCC>), dim3((unsigned)n), dim3(64 * B::W), 0, (hipStream_t)stream, sh, o);
    });
}

int launch_opt_reduce(const OptArgs &o, void *stream) {
    if (o.n_pops <= 0) return 0;
    hipLaunchKernelGGL(opt_reduce_kernel, dim3((unsigned)o.n_pops), dim3(64), 0, (hipStream_t)stream, o);
    return (int)hipGetLastError();
}

}  // namespace mp

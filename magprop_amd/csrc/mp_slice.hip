// mp_slice.hip — gfx950 kernels of the ensemble slice-sampling move of the device-resident sampler (include/magprop_amd.h
// MP_MOVE_SLICE; Karamanis & Beutler 2021 over Neal 2003's stepping out and shrinkage).
//
// slice_half_kernel: one workgroup per slot of the active half, on the shell of mp_point.h; the block-to-ensemble mapping through
// slot_lo and ens_order is stretch_kernel's.  Lane 0 draws the direction (a difference of two walkers of the other half) and runs
// the slice update of its walker as a state machine in LDS (slice_step of mp_walk.h, the machine the nested sampler's slice mode
// states in mp_nest.hip: step out left, step out right, shrink) that names one point per round or ends the update; the workgroup
// evaluates the named point through the one point_eval call of the kernel.  The other half is only read and the active walker only written by its
// own workgroup, so the workgroups need no hand-off among themselves.
// slice_tune_kernel: one thread per ensemble, behind the second half-step: folds the step's counts into the totals and tunes mu.
#include <hip/hip_runtime.h>

#include "mp_point.h"
#include "mp_slice.h"
#include "mp_walk.h"

namespace mp {

namespace {

constexpr uint32_t kSliceMoveCtr = 0x51C00000u;   // fourth counter word: 0x51C00000 + c, c = 0 partners, 1 interval, 2 level, 3 + i shrink point i

MP_DEV void slice_draw(const StretchArgs &g, int k, uint32_t c, uint32_t (&out)[4]) {
    philox4x32_10((uint32_t)g.seed, (uint32_t)(g.seed >> 32), (uint32_t)g.step, (uint32_t)g.half, (uint32_t)k, kSliceMoveCtr + c, out);
}

// The update's state between rounds, in LDS (only lane 0 reads or writes it): the walker's one slice is open in c (mp_walk.h)
// until the update ends.
struct SliceWalk {
    double lnp, lny, mu, beta;   // the walker's (untempered) lnprob; the level; the ensemble's scale and inverse temperature
    SliceCore c;
    int st, moved, n_eval;
};

// Lane 0, before the first round: the walker's position, its direction x_c1 - x_c2, the interval, the budgets and the level.
MP_DEV void slice_begin(const StretchArgs &g, const SliceArgs &sl, int k, int w_ens, int base, const int32_t *perm, SliceWalk &z,
                        double *cur, double *dir) {
    const int nd = g.ndim, n_comp = g.n_walkers - g.n_half;
    const int32_t *comp = perm + (1 - g.half) * g.n_half;
    z = SliceWalk{};
    z.lnp = g.lnprob[k];
    z.st = MP_STATUS_OK;
    z.mu = sl.mu[w_ens];
    z.beta = g.beta ? g.beta[w_ens] : 1.0;
    for (int d = 0; d < nd; ++d) cur[d] = g.pos[(size_t)k * nd + d];
    uint32_t u[4];
    slice_draw(g, k, 0u, u);
    const int c1 = pick(u01(u[0], u[1]), n_comp), c2 = pick_skip(u01(u[2], u[3]), n_comp, c1);
    const double *x1 = g.pos + (size_t)(base + comp[c1]) * nd, *x2 = g.pos + (size_t)(base + comp[c2]) * nd;
    int nz = 0;
    for (int d = 0; d < nd; ++d) {
        dir[d] = sub_rn(x1[d], x2[d]);
        nz |= dir[d] != 0.0 ? 1 : 0;
    }
    if (!nz) {   // coinciding partners: the slice fails where it starts (none is opened)
        z.c.n_fail = 1;
        return;
    }
    slice_draw(g, k, 1u, u);
    slice_open(z.c, z.mu, u01(u[0], u[1]), u01(u[2], u[3]), sl.max_steps_out);
    slice_draw(g, k, 2u, u);
    z.lny = add_rn(mul_rn(z.beta, z.lnp), log(u01(u[0], u[1])));   // (ln 0 = -inf: everything finite is inside)
}

// Lane 0, once per round: takes the outcome of the point named last round (have: one was evaluated, lnprob lnp, status), then
// advances until it names the next point to evaluate (in prop; returns 1) or the update ends (returns 0; a walker that moved has
// its new position in cur).  Inside = in the prior box (target 0) and beta lnprob > the level.
MP_DEV int slice_move_round(const DevShared &sh, const StretchArgs &g, const SliceArgs &sl, int k, SliceWalk &z, double *cur,
                            const double *dir, double *prop, bool have, double lnp, int status) {
    if (z.c.phase == kSliceEnded) return 0;
    const int end = slice_step(z.c, z.mu, sl.max_shrink, have, have && mul_rn(z.beta, lnp) > z.lny, cur, dir, prop, g.ndim,
                               [&](int i) {
                                   uint32_t u[4];
                                   slice_draw(g, k, 3u + (uint32_t)i, u);
                                   return u01(u[0], u[1]);
                               },
                               [&](int d, double q) { return g.target != 0 || d >= sh.n_prior || (q >= sh.lower[d] && q <= sh.upper[d]); });
    if (end == kSliceNamed) return 1;
    if (end == kSliceMoved) {
        for (int d = 0; d < g.ndim; ++d) cur[d] = prop[d];
        z.lnp = lnp;
        z.st = status;
        z.moved = 1;
    }
    return 0;
}

// One workgroup per slot of the active half; builds and template arguments as the kernels of mp_point.h.
template <int SPL, bool LONG, int W = 1, int OCC = 0>
MP_POINT_KERNEL(SPL, W, OCC) void slice_half_kernel(const DevShared sh, const StretchArgs g, const SliceArgs sl) {
    __shared__ PointLds<SPL, W> ws;
    __shared__ double cur[MP_MAX_NDIM];      // the walker's position (the new one once it has moved)
    __shared__ double dir[MP_MAX_NDIM];      // the slice's direction
    __shared__ double prop[MP_MAX_NDIM];     // the named point across the evaluation
    __shared__ SliceWalk z;
    __shared__ int go;                       // 1: evaluate prop; 0: the update has ended
    tables_init<SPL * W, 64 * W>(sh, ws.tt);
    const int gs = g.slot_lo + (int)blockIdx.x;                    // slot of the active half, all ensembles flattened
    const int w_ens = ens_of_slot(g, gs / g.n_half);               // which ensemble (longest light curve first)
    const int slot = gs % g.n_half;                                // which walker of the active half
    const int32_t *perm = g.perm + (size_t)w_ens * g.n_walkers;    // this step's random split of the ensemble
    const int base = w_ens * g.n_walkers;
    const int k = base + perm[g.half * g.n_half + slot];           // active walker (global index)
    const int nd = g.ndim;
    if (threadIdx.x == 0) slice_begin(g, sl, k, w_ens, base, perm, z, cur, dir);
    double lnp = 0.0;
    int status = MP_STATUS_OK;
    for (bool have = false;; have = true) {
        __syncthreads();
        if (threadIdx.x == 0) go = slice_move_round(sh, g, sl, k, z, cur, dir, prop, have, lnp, status);
        __syncthreads();
        if (!go) break;                        // (uniform: LDS behind the barrier)
        point_eval<SPL, LONG, W, OCC>(sh, ws, g.ds_id, nd, g.target, k, prop, lnp, status);
        if (threadIdx.x == 0) {
            ++z.n_eval;
            fbad_append(g, status, prop);
        }
    }
    if (threadIdx.x == 0) {
        if (z.moved) {
            for (int d = 0; d < nd; ++d) g.pos[(size_t)k * nd + d] = cur[d];
            g.lnprob[k] = z.lnp;
            g.n_accepted[k] += 1;
        }
        if (g.chain) {
            double *c = g.chain + ((size_t)g.chain_row * g.n_total + k) * nd;
            for (int d = 0; d < nd; ++d) c[d] = cur[d];
            g.chain_lnp[(size_t)g.chain_row * g.n_total + k] = z.lnp;
        }
        if (z.c.n_exp) atomicAdd((unsigned long long *)&sl.nexpand_s[w_ens], (unsigned long long)z.c.n_exp);
        if (z.c.n_con) atomicAdd((unsigned long long *)&sl.ncontract_s[w_ens], (unsigned long long)z.c.n_con);
        if (z.c.n_fail) atomicAdd((unsigned long long *)&sl.nfail[w_ens], (unsigned long long)z.c.n_fail);
        if (z.n_eval) atomicAdd((unsigned long long *)&sl.neval[w_ens], (unsigned long long)z.n_eval);
    }
}

// zeus's rule on the step's counts of ensemble e: mu <- mu (2 a / (a + ncontract_s)), a = max(1, nexpand_s), while fewer than
// tune_steps slice steps have been taken.  The quotient and the product are rounded separately.
__global__ __launch_bounds__(64) void slice_tune_kernel(const SliceArgs sl, int n_ensembles) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= n_ensembles) return;
    const int64_t ex = sl.nexpand_s[e], co = sl.ncontract_s[e];
    sl.nexpand[e] += ex;
    sl.ncontract[e] += co;
    sl.nexpand_s[e] = 0;
    sl.ncontract_s[e] = 0;
    if (sl.n_tuned[e] < sl.tune_steps) {
        const double a = (double)(ex > 1 ? ex : 1);
        sl.mu[e] = mul_rn(sl.mu[e], mul_rn(2.0, a) / add_rn(a, (double)co));
    }
    sl.n_tuned[e] += 1;
}

}  // namespace

int launch_slice_half(const DevShared &sh, const StretchArgs &g, const SliceArgs &sl, void *stream) {
    const int n = g.n_half * g.n_ensembles;
    if (n <= 0) return 0;
    return launch_point_kernel(sh, n, [&](auto build, auto lng) {
        using B = decltype(build);
        hipLaunchKernelGGL((slice_half_kernel<B::SPL, lng, B::W, B::OCC>), dim3((unsigned)n), dim3(64 * B::W), 0, (hipStream_t)stream, sh, g, sl);
    });
}

int launch_slice_tune(const SliceArgs &sl, int n_ensembles, void *stream) {
    if (n_ensembles <= 0) return 0;
    hipLaunchKernelGGL(slice_tune_kernel, dim3((unsigned)((n_ensembles + 63) / 64)), dim3(64), 0, (hipStream_t)stream, sl, n_ensembles);
    return (int)hipGetLastError();
}

}  // namespace mp

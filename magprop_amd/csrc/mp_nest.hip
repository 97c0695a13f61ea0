// mp_nest.hip — gfx950 kernels of the nested sampler (include/magprop_amd.h mp_nested_*): Skilling's nested sampling with batch
// removal, constrained DE random walks, one select and one walk launch per iteration.
//
// nest_select_kernel: one workgroup per run.  It ranks the live lnL (by lnL, then slot; N <= 4096 keys in LDS), applies the stop
// rule to the live set as it stands, and otherwise writes the iteration's dead list (ascending lnL), the survivors in slot order,
// L*, the dead rows of the chunk and the new ln X and ln Z (one thread, in the order of the header).
// nest_walk_kernel: one workgroup per dead slot, on the shell of mp_point.h.  Lane 0 picks a survivor as the start and builds
// every DE step in LDS (de_walk_step of mp_walk.h), the workgroup evaluates the step, lane 0 decides (inside the box and lnL >
// L*).  Survivors are only read and dead slots only written, so the workgroups need no hand-off among themselves.  Mode 1
// evaluates the live set as the caller set it.  (The one kernel of the four that states point_eval's block itself: with the call
// its walks ran 3 % slower.)
// nest_slice_kernel: the walk of slice mode (mp_nested_set_slice), the same workgroups and builds.  Lane 0 runs the slice updates
// as a state machine in LDS (start a slice, step out left, step out right, shrink) that names one point per round or ends the
// walk; the workgroup evaluates the named point through the one point_eval call of the kernel.
//
// The phases of a slice are stated here a second time: slice_step of mp_walk.h, which the ensemble slice move runs
// (mp_slice.hip), is the same machine line for line.  On it this kernel spilled less on every build (scratch 92 .. 152 -> 72 ..
// 124 B/lane) and yet ran slice mode 2.2 % slower on one MI355X, on the posterior and on the Gaussian target alike: 2.786 ..
// 2.796 ms per iteration against 2.719 .. 2.733 on Humped, 0.304 .. 0.307 against 0.297 .. 0.300 on the 6-d Gaussian, five
// alternated runs against six (tools/nest_bench.py rate --sample both; profiles/r25_walk_shared_ab.json; DESIGN.md "What the walk
// kernels share").  A fix to the phase logic goes into both, and into tests/walk_restated.py, which restates them once.
#include <hip/hip_runtime.h>

#include "mp_point.h"
#include "mp_walk.h"

namespace mp {

namespace {

constexpr uint32_t kNestCtr = 0x4E000000u;   // third counter word: 0x4E000000 + j, j = 0 start, 2 s + 1 and 2 s + 2 step s

MP_DEV void nest_draw(const NestArgs &a, int r, int slot, uint32_t j, uint32_t (&out)[4]) {
    philox4x32_10((uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.iter, (uint32_t)r, (uint32_t)slot, kNestCtr + j, out);
}

// log(exp(x) + exp(y)), -inf when both are
MP_DEV double logaddexp(double x, double y) {
    const double m = fmax(x, y);
    if (m == -INFINITY) return m;
    return add_rn(m, log1p(exp(-fabs(sub_rn(x, y)))));
}

// The builds of mp_point.h for the launch's workgroup count (launch_nest_walk); a run's points are evaluated as walker r.
template <int SPL, bool LONG, int W = 1, int OCC = 0>
MP_POINT_KERNEL(SPL, W, OCC) void nest_walk_kernel(const DevShared sh, const NestArgs a) {
    const int b = (int)blockIdx.x, per = a.mode ? a.nlive : a.nbatch, r = b / per, k = b - r * per;
    if (a.mode == 0 && a.stopped[r]) return;   // frozen run (uniform for the workgroup): nothing to do
    __shared__ PointLds<SPL, W> ws;
    __shared__ double cur[MP_MAX_NDIM];      // the walk's current point
    __shared__ double prop[MP_MAX_NDIM];     // the step's proposal across the evaluation
    __shared__ int go;                       // 1: the proposal lies in the box (evaluate it)
    tables_init<SPL * W, 64 * W>(sh, ws.tt);
    const int nd = a.ndim, m = a.nlive - a.nbatch, base = r * a.nlive;
    const int slot = a.mode ? k : a.dead_slot[r * a.nbatch + k];
    const int steps = a.mode ? 1 : a.walks;
    double lnl_cur = -INFINITY, lstar = 0.0;
    int st_cur = MP_STATUS_OK, n_acc = 0, n_eval = 0;
    if (threadIdx.x == 0) {
        int from = base + slot;
        if (!a.mode) {
            uint32_t u[4];
            nest_draw(a, r, slot, 0u, u);
            from = base + a.surv[r * m + pick(u01(u[0], u[1]), m)];
            lnl_cur = a.lnl[from];
            st_cur = a.st[from];
            lstar = a.lstar[r];
        }
        for (int d = 0; d < nd; ++d) cur[d] = a.live[(size_t)from * nd + d];
    }
    for (int s = 0; s < steps; ++s) {
        __syncthreads();
        if (threadIdx.x == 0) {
            if (a.mode) {
                for (int d = 0; d < nd; ++d) prop[d] = cur[d];
                go = 1;
            } else {
                uint32_t u[4], v[4];
                nest_draw(a, r, slot, 2u * (uint32_t)s + 1u, u);
                nest_draw(a, r, slot, 2u * (uint32_t)s + 2u, v);
                const int c1 = pick(u01(u[0], u[1]), m), c2 = pick_skip(u01(u[2], u[3]), m, c1);
                const double *x1 = a.live + (size_t)(base + a.surv[r * m + c1]) * nd;
                const double *x2 = a.live + (size_t)(base + a.surv[r * m + c2]) * nd;
                go = de_walk_step(cur, x1, x2, a.g0, a.sig3, u01(v[0], v[1]), a.lower, a.upper, nd, prop);
            }
        }
        __syncthreads();
        if (!go) continue;                     // (uniform: LDS behind the barrier)
        // point_eval(sh, ws, a.ds_id, nd, a.target, r, prop, lnp, status), stated here: through the call the team build of up to
        // n_simd / 4 walks spills less and yet takes 1.611 ms per iteration where this takes 1.56
        double par[MP_MAX_NDIM];
#pragma unroll
        for (int d = 0; d < MP_MAX_NDIM; ++d) par[d] = d < nd ? prop[d] : 0.0;
        double lnp = 0.0;
        int status = MP_STATUS_OK, sweeps, tiles;
        if (a.target == 1) {   // isotropic unit Gaussian: exercises the algorithm itself (tests)
#pragma unroll
            for (int d = 0; d < MP_MAX_NDIM; ++d) lnp = d < nd ? sub_rn(lnp, mul_rn(mul_rn(0.5, par[d]), par[d])) : lnp;
        } else {
            LaunchArgs la{};
            la.ds_id = a.ds_id;
            la.ndim = nd;
            la.physical = 0;
            la.want_chi2 = 1;
            if constexpr (W > 1) walker_eval<false, SPL, LONG, false, W, OCC >= 2>(sh, la, r, par, ws.im, ws.tt, ws.lds, lnp, status, sweeps, tiles, ws.tl.ptr());
            else walker_eval<false, SPL, LONG>(sh, la, r, par, ws.im, ws.tt, ws.lds, lnp, status, sweeps, tiles);
        }
        if (threadIdx.x == 0) {
            if (lnp != lnp) lnp = -INFINITY;   // NaN counts (and is kept) as -inf
            ++n_eval;
            if (a.mode || lnp > lstar) {
                for (int d = 0; d < nd; ++d) cur[d] = prop[d];
                lnl_cur = lnp;
                st_cur = status;
                n_acc += a.mode ? 0 : 1;
            }
        }
    }
    if (threadIdx.x == 0) {
        const size_t row = (size_t)(base + slot);
        for (int d = 0; d < nd; ++d) a.live[row * nd + d] = cur[d];
        a.lnl[row] = lnl_cur;
        a.st[row] = st_cur;
        a.acc[row] = n_acc;
        if (!a.mode) {
            atomicAdd((unsigned long long *)&a.ncall[r], (unsigned long long)n_eval);
            atomicAdd((unsigned long long *)&a.nacc[r], (unsigned long long)n_acc);
            if (n_acc == 0) atomicAdd((unsigned long long *)&a.nzero[r], 1ull);
        }
    }
}

// ---------------------------------------------------------------- slice mode
constexpr uint32_t kSliceCtr = 0x4E400000u;   // third counter word: 0x4E400000 + 0x100 s + c, c = 0 .. 1 + max_shrink, slice s

// The walk's state between rounds, in LDS (only lane 0 reads or writes it).  phase: kStart begins slice s (ends the walk after
// the last), kLeft / kRight step out (budgets left / right), kShrink draws shrink point i of [lo, hi].
enum { kStart = 0, kLeft = 1, kRight = 2, kShrink = 3 };
struct SliceState {
    double lnl, lo, hi, t;    // the current point's lnL; the interval along dir; the parameter of the named point
    int st, s, phase, left, right, i, moved, n_eval, n_exp, n_con, n_fail;
};

// Lane 0, once per round: takes the outcome of the point named last round (have: one was evaluated, lnL lnp, status), then
// advances until it names the next point in the box (prop = cur + t dir, unfused; returns 1) or the walk ends (returns 0).
// Inside = in the box and lnL > L*; a point outside the box is outside without an evaluation.
MP_DEV int slice_round(const NestArgs &a, const NestSlice &sl, int r, int slot, SliceState &z, double *cur, double *dir,
                       double *prop, bool have, double lnp, int status) {
    const int nd = a.ndim, m = a.nlive - a.nbatch, base = r * a.nlive;
    const double lstar = a.lstar[r];
    bool in = have && lnp > lstar;
    for (;;) {
        if (have) {   // the named point's outcome (evaluated, or outside the box)
            have = false;
            if (z.phase == kLeft) {
                if (in) { z.lo = sub_rn(z.lo, sl.mu); --z.left; ++z.n_exp; } else z.phase = kRight;
            } else if (z.phase == kRight) {
                if (in) { z.hi = add_rn(z.hi, sl.mu); --z.right; ++z.n_exp; } else z.phase = kShrink;
            } else if (in) {
                for (int d = 0; d < nd; ++d) cur[d] = prop[d];
                z.lnl = lnp;
                z.st = status;
                ++z.moved;
                ++z.s;
                z.phase = kStart;
            } else {
                ++z.n_con;
                if (z.t < 0.0) z.lo = z.t;
                else z.hi = z.t;
            }
        }
        double t;
        if (z.phase == kStart) {
            if (z.s == sl.slices) return 0;
            uint32_t u[4];
            philox4x32_10((uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.iter, (uint32_t)r, (uint32_t)slot, kSliceCtr + 0x100u * (uint32_t)z.s, u);
            const int c1 = pick(u01(u[0], u[1]), m), c2 = pick_skip(u01(u[2], u[3]), m, c1);
            const double *x1 = a.live + (size_t)(base + a.surv[r * m + c1]) * nd;
            const double *x2 = a.live + (size_t)(base + a.surv[r * m + c2]) * nd;
            int nz = 0;
            for (int d = 0; d < nd; ++d) {
                dir[d] = sub_rn(x1[d], x2[d]);
                nz |= dir[d] != 0.0 ? 1 : 0;
            }
            if (!nz) {   // coinciding partners: the slice fails where it starts
                ++z.n_fail;
                ++z.s;
                continue;
            }
            philox4x32_10((uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.iter, (uint32_t)r, (uint32_t)slot, kSliceCtr + 0x100u * (uint32_t)z.s + 1u, u);
            z.lo = -mul_rn(sl.mu, u01(u[0], u[1]));
            z.hi = add_rn(z.lo, sl.mu);
            z.left = (int)(u01(u[2], u[3]) * (double)sl.max_steps_out);
            z.right = sl.max_steps_out - 1 - z.left;
            z.i = 0;
            z.phase = kLeft;
            continue;
        }
        if (z.phase == kLeft) {
            if (z.left == 0) { z.phase = kRight; continue; }
            t = z.lo;
        } else if (z.phase == kRight) {
            if (z.right == 0) { z.phase = kShrink; continue; }
            t = z.hi;
        } else {
            if (z.i == sl.max_shrink) {   // the cap: the slice fails where it starts
                ++z.n_fail;
                ++z.s;
                z.phase = kStart;
                continue;
            }
            uint32_t u[4];
            philox4x32_10((uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.iter, (uint32_t)r, (uint32_t)slot,
                          kSliceCtr + 0x100u * (uint32_t)z.s + 2u + (uint32_t)z.i, u);
            ++z.i;
            t = add_rn(z.lo, mul_rn(u01(u[0], u[1]), sub_rn(z.hi, z.lo)));
        }
        z.t = t;
        int box = 1;
        for (int d = 0; d < nd; ++d) {
            const double q = add_rn(cur[d], mul_rn(t, dir[d]));
            box &= (q >= a.lower[d] && q <= a.upper[d]) ? 1 : 0;
            prop[d] = q;
        }
        if (box) return 1;
        have = true;   // outside the box: outside, not evaluated
        in = false;
    }
}

// One workgroup per dead slot of a running run; builds and template arguments as nest_walk_kernel.
template <int SPL, bool LONG, int W = 1, int OCC = 0>
MP_POINT_KERNEL(SPL, W, OCC) void nest_slice_kernel(const DevShared sh, const NestArgs a, const NestSlice sl) {
    const int b = (int)blockIdx.x, r = b / a.nbatch, k = b - r * a.nbatch;
    if (a.stopped[r]) return;   // frozen run (uniform for the workgroup): nothing to do
    __shared__ PointLds<SPL, W> ws;
    __shared__ double cur[MP_MAX_NDIM];      // the walk's current point
    __shared__ double dir[MP_MAX_NDIM];      // the slice's direction
    __shared__ double prop[MP_MAX_NDIM];     // the named point across the evaluation
    __shared__ SliceState z;
    __shared__ int go;                       // 1: evaluate prop; 0: the walk has ended
    tables_init<SPL * W, 64 * W>(sh, ws.tt);
    const int nd = a.ndim, m = a.nlive - a.nbatch, base = r * a.nlive;
    const int slot = a.dead_slot[r * a.nbatch + k];
    if (threadIdx.x == 0) {
        uint32_t u[4];
        nest_draw(a, r, slot, 0u, u);
        const int from = base + a.surv[r * m + pick(u01(u[0], u[1]), m)];
        for (int d = 0; d < nd; ++d) cur[d] = a.live[(size_t)from * nd + d];
        z = SliceState{};
        z.lnl = a.lnl[from];
        z.st = a.st[from];
        z.phase = kStart;
    }
    double lnp = 0.0;
    int status = MP_STATUS_OK;
    for (bool have = false;; have = true) {
        __syncthreads();
        if (threadIdx.x == 0) go = slice_round(a, sl, r, slot, z, cur, dir, prop, have, lnp, status);
        __syncthreads();
        if (!go) break;                        // (uniform: LDS behind the barrier)
        point_eval<SPL, LONG, W, OCC>(sh, ws, a.ds_id, nd, a.target, r, prop, lnp, status);
        if (threadIdx.x == 0) ++z.n_eval;
    }
    if (threadIdx.x == 0) {
        const size_t row = (size_t)(base + slot);
        for (int d = 0; d < nd; ++d) a.live[row * nd + d] = cur[d];
        a.lnl[row] = z.lnl;
        a.st[row] = z.st;
        a.acc[row] = z.moved;
        atomicAdd((unsigned long long *)&a.ncall[r], (unsigned long long)z.n_eval);
        atomicAdd((unsigned long long *)&a.nacc[r], (unsigned long long)z.moved);
        if (z.moved == 0) atomicAdd((unsigned long long *)&a.nzero[r], 1ull);
        atomicAdd((unsigned long long *)&sl.nexpand[r], (unsigned long long)z.n_exp);
        atomicAdd((unsigned long long *)&sl.ncontract[r], (unsigned long long)z.n_con);
        atomicAdd((unsigned long long *)&sl.nfail[r], (unsigned long long)z.n_fail);
    }
}

constexpr int kSelThreads = 1024;

// Ranks, the stop rule and the bookkeeping of one iteration of run blockIdx.x (include/magprop_amd.h states the arithmetic).
__global__ __launch_bounds__(kSelThreads) void nest_select_kernel(const NestArgs a) {
    const int r = (int)blockIdx.x, n = a.nlive, K = a.nbatch, m = n - K, base = r * n, tid = (int)threadIdx.x;
    if (a.stopped[r]) return;
    __shared__ double key[MP_NEST_MAX_LIVE];
    __shared__ int rank[MP_NEST_MAX_LIVE];
    __shared__ int dslot[MP_NEST_MAX_LIVE / 2];
    __shared__ double shell[MP_NEST_MAX_LIVE / 2];   // log(-expm1(-1 / n_k)) of dead k
    __shared__ double lmax;
    __shared__ int stop;
    for (int j = tid; j < n; j += kSelThreads) {
        const double v = a.lnl[base + j];
        key[j] = v != v ? -INFINITY : v;
    }
    __syncthreads();
    // rank of slot j: the live points before it in the order (lnL, slot)
    for (int j = tid; j < n; j += kSelThreads) {
        const double kj = key[j];
        int c = 0;
        for (int i = 0; i < n; ++i) {
            const double ki = key[i];
            c += (ki < kj || (ki == kj && i < j)) ? 1 : 0;
        }
        rank[j] = c;
        if (c == n - 1) lmax = kj;
    }
    __syncthreads();
    if (tid == 0) {
        stop = log1p(exp(sub_rn(add_rn(lmax, a.lnx[r]), a.lnz[r]))) < a.dlogz;
        if (stop) a.stopped[r] = 1;
    }
    __syncthreads();
    if (stop || a.mode) return;
    for (int j = tid; j < n; j += kSelThreads) {
        const int c = rank[j];
        if (c < K) {
            dslot[c] = j;
            a.dead_slot[r * K + c] = j;
        } else {
            int before = 0;   // dead slots in front of j
            for (int i = 0; i < j; ++i) before += rank[i] < K ? 1 : 0;
            a.surv[r * m + j - before] = j;
        }
    }
    __syncthreads();
    const size_t drow = ((size_t)a.slot * a.n_runs + r) * K;
    for (int e = tid; e < K * a.ndim; e += kSelThreads) {
        const int k = e / a.ndim, d = e - k * a.ndim;
        a.dead_pars[(drow + k) * a.ndim + d] = a.live[(size_t)(base + dslot[k]) * a.ndim + d];
    }
    for (int k = tid; k < K; k += kSelThreads) {
        a.dead_lnl[drow + k] = key[dslot[k]];
        a.dead_n[drow + k] = n - k;
        shell[k] = log(-expm1(-(1.0 / (double)(n - k))));
    }
    __syncthreads();
    if (tid == 0) {   // (the chain of ln X and ln Z in order; the shell terms came from every thread)
        double lnx = a.lnx[r], lnz = a.lnz[r];
        for (int k = 0; k < K; ++k) {
            const double inv = 1.0 / (double)(n - k);
            const double lnw = add_rn(add_rn(key[dslot[k]], lnx), shell[k]);
            lnx = sub_rn(lnx, inv);
            lnz = logaddexp(lnz, lnw);
        }
        a.lstar[r] = key[dslot[K - 1]];
        a.lnx[r] = lnx;
        a.lnz[r] = lnz;
        a.nit[r] += 1;
    }
}

}  // namespace

// One workgroup per dead slot: n = n_runs * nbatch (mode 1: one per live point, n_runs * nlive).
int launch_nest_walk(const DevShared &sh, const NestArgs &a, void *stream) {
    const int n = a.n_runs * (a.mode ? a.nlive : a.nbatch);
    if (n <= 0) return 0;
    return launch_point_kernel(sh, n, [&](auto build, auto lng) {
        using B = decltype(build);
        hipLaunchKernelGGL((nest_walk_kernel<B::SPL, lng, B::W, B::OCC>), dim3((unsigned)n), dim3(64 * B::W), 0, (hipStream_t)stream, sh, a);
    });
}

// slice mode: the builds of launch_nest_walk for its n_runs * nbatch workgroups
int launch_nest_slice(const DevShared &sh, const NestArgs &a, const NestSlice &sl, void *stream) {
    const int n = a.n_runs * a.nbatch;
    if (n <= 0 || a.mode) return 0;
    return launch_point_kernel(sh, n, [&](auto build, auto lng) {
        using B = decltype(build);
        hipLaunchKernelGGL((nest_slice_kernel<B::SPL, lng, B::W, B::OCC>), dim3((unsigned)n), dim3(64 * B::W), 0, (hipStream_t)stream, sh, a, sl);
    });
}

int launch_nest_select(const NestArgs &a, void *stream) {
    if (a.n_runs <= 0) return 0;
    hipLaunchKernelGGL(nest_select_kernel, dim3((unsigned)a.n_runs), dim3(kSelThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace mp

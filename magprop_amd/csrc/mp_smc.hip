// mp_smc.hip — gfx950 kernels of the tempered SMC sampler (include/magprop_amd.h mp_smc_*): N particles per run move from the
// prior (beta = 0) to the posterior (beta = 1) through stages whose beta the particles' own weights choose; one stage and one
// move launch per stage.
//
// smc_stage_kernel: one workgroup of kWgThreads per run, reductions of mp_wg.h.  It finds the increment d of beta that brings the
// effective sample size of the weights exp(d (lnl - M)) down to the target (bisection; every probe is one pass of exp over the
// run's lnl, read from global memory: a run of 16 384 does not fit LDS), advances ln Z, turns the weights into integer units,
// scans them and resamples systematically in integers: anc[j], the particle slot j continues from.
// smc_move_kernel: one workgroup per slot, on the shell of mp_point.h.  Lane 0 starts from the slot's ancestor and builds every
// DE step in LDS from two other slots' ancestors (de_walk_step of mp_walk.h, the nested sampler's), the workgroup evaluates the
// step through the one point_eval call, lane 0 takes the tempered Metropolis decision.  The stage's buffer is only read and the other one only written, so the workgroups need no
// hand-off among themselves.  Mode 1 evaluates the particles as the caller set them.
// Adaptation (mp_smc_set_adaptive): a stage's moves are rounds of `walks` steps.  Round 0 is the launch above; in round k >= 1
// slot j continues in place from its own row of the other buffer, its partners still drawn over the stage's buffer, which stays
// unwritten until the next stage.  smc_tune_kernel: one workgroup of kWgThreads per run behind every round; from the correlation
// between where the slots started and where they are it decides whether the run makes another round, and at the round that stops
// it writes the stage's row of the tuning log and the run's scale g for the next stage.  The launches of a round act on the runs
// whose flags (rounds, moving) say the round is theirs; the workgroups of the others return at once.
#include <hip/hip_runtime.h>

#include "mp_point.h"
#include "mp_smc.h"
#include "mp_walk.h"
#include "mp_wg.h"

namespace mp {

namespace {

// w_i(d) = exp(d (lnl_i - M)); 0 for a particle whose lnl is not finite
MP_DEV double smc_weight(double l, double M, double d) { return fabs(l) < INFINITY ? exp(mul_rn(d, sub_rn(l, M))) : 0.0; }

struct SmcSums {
    double s1, s2, wmax;   // sum w, sum w^2, max w
};

// The sums at increment d: every thread adds its particles tid, tid + 256, ... in that order, then the order of mp_wg.h.
__device__ SmcSums smc_sums(const double *lnl, int n, double M, double d, double *sh) {
    double s1 = 0.0, s2 = 0.0, wmax = 0.0;
    for (int i = (int)threadIdx.x; i < n; i += kWgThreads) {
        const double w = smc_weight(lnl[i], M, d);
        s1 = add_rn(s1, w);
        s2 = add_rn(s2, mul_rn(w, w));
        wmax = fmax(wmax, w);
    }
    return {wg_sum(s1, sh), wg_sum(s2, sh), wg_max(wmax, sh)};
}

MP_DEV double smc_ess(const SmcSums &s) { return mul_rn(s.s1, s.s1) / s.s2; }

// One stage of run blockIdx.x (include/magprop_amd.h states the arithmetic).
__global__ __launch_bounds__(kWgThreads) void smc_stage_kernel(const SmcArgs a) {
    const int r = (int)blockIdx.x, n = a.n, base = r * n, tid = (int)threadIdx.x;
    if (a.status[r] != MP_SMC_RUNNING) return;   // (uniform for the workgroup, and read before the first barrier)
    const int made = a.nstage[r];
    const double beta = a.beta[r];
    __shared__ double shd[kWgWaves];
    __shared__ uint32_t shc[kWgWaves];
    __shared__ unsigned long long shu[kWgWaves];
    __shared__ unsigned long long total;
    if (made >= MP_SMC_MAX_STAGES) {
        if (tid == 0) a.status[r] = MP_SMC_STAGE_LIMIT;
        return;
    }
    const double *lnl = a.lnl_cur + base;
    double m = -INFINITY;
    uint32_t fin = 0;
    for (int i = tid; i < n; i += kWgThreads) {
        const double v = lnl[i];
        if (fabs(v) < INFINITY) {
            m = fmax(m, v);
            ++fin;
        }
    }
    const double M = wg_max(m, shd);
    const uint32_t n_fin = wg_count(fin, shc);
    if (n_fin == 0) {
        if (tid == 0) a.status[r] = MP_SMC_FAILED;
        return;
    }
    const double target = mul_rn(a.ess, (double)n_fin), rem = sub_rn(1.0, beta);
    double d = rem;
    bool last = true;
    if (!(smc_ess(smc_sums(lnl, n, M, rem, shd)) >= target)) {
        last = false;
        double lo = 0.0, hi = rem;
        for (int k = 0; k < 128; ++k) {
            const double mid = mul_rn(0.5, add_rn(lo, hi));
            if (mid == lo || mid == hi) break;
            if (smc_ess(smc_sums(lnl, n, M, mid, shd)) >= target) lo = mid;
            else hi = mid;
        }
        d = lo > 0.0 ? lo : hi;
    }
    const SmcSums s = smc_sums(lnl, n, M, d, shd);
    // integer weights, their cumulative sums (thread t: the particles [t c, (t + 1) c), behind the scan of the threads' sums)
    for (int i = tid; i < n; i += kWgThreads)
        a.units[base + i] = (uint32_t)rint(mul_rn(2147483648.0, smc_weight(lnl[i], M, d)) / s.wmax);
    __syncthreads();
    const int c = (n + kWgThreads - 1) / kWgThreads, i0 = min(tid * c, n), i1 = min(i0 + c, n);
    unsigned long long mine = 0;
    for (int i = i0; i < i1; ++i) mine += a.units[base + i];
    const unsigned long long incl = wg_inclusive_scan(mine, shu);
    unsigned long long run = incl - mine;
    for (int i = i0; i < i1; ++i) {
        run += a.units[base + i];
        a.cum[base + i] = run;
    }
    if (tid == kWgThreads - 1) total = incl;
    __syncthreads();
    // systematic resampling in integers: slot j continues the least i with C_i > P_j
    const unsigned long long U = total;
    uint32_t u[4];
    philox4x32_10((uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.stage, (uint32_t)r, 0u, kSmcCtr, u);
    const unsigned long long off = (unsigned long long)mul_rn(u01(u[0], u[1]), (double)U);
    const unsigned long long *cum = a.cum + base;
    for (int j = tid; j < n; j += kWgThreads) {
        const unsigned long long P = ((unsigned long long)j * U + off) / (unsigned long long)n;
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cum[mid] > P) hi = mid;
            else lo = mid + 1;
        }
        a.anc[base + j] = lo;
    }
    if (tid == 0) {
        const double nb = last ? 1.0 : add_rn(beta, d);
        const double lnz = add_rn(a.lnz[r], add_rn(mul_rn(d, M), log(s.s1 / (double)n)));
        double *row = a.log + ((size_t)r * MP_SMC_MAX_STAGES + made) * kSmcLogCols;
        row[0] = nb;
        row[1] = d;
        row[2] = smc_ess(s);
        row[3] = lnz;
        a.log_cnt[((size_t)r * MP_SMC_MAX_STAGES + made) * 2] = a.ncall[r];
        a.log_cnt[((size_t)r * MP_SMC_MAX_STAGES + made) * 2 + 1] = a.nacc[r];
        a.beta[r] = nb;
        a.lnz[r] = lnz;
        a.nstage[r] = made + 1;
        if (a.adapt_max) {                          // the stage's rounds start over
            a.rounds[r] = 0;
            a.moving[r] = 1;
        }
        if (nb >= 1.0) a.status[r] = MP_SMC_DONE;   // (its moves of this stage still run: they go by nstage)
    }
}

// The builds of mp_point.h for the launch's workgroup count (launch_smc_move); a run's points are evaluated as walker r.
template <int SPL, bool LONG, int W = 1, int OCC = 0>
MP_POINT_KERNEL(SPL, W, OCC) void smc_move_kernel(const DevShared sh, const SmcArgs a) {
    const int b = (int)blockIdx.x, r = b / a.n, j = b - r * a.n;
    if (a.mode == 0 && a.nstage[r] != (int)a.stage + 1) return;   // no stage made (uniform for the workgroup): nothing to do
    // adaptive: round a.round is this run's only while its moves go on and it has made that many rounds (uniform as well)
    if (a.mode == 0 && a.adapt_max && (!a.moving[r] || a.rounds[r] != a.round)) return;
    const int round = a.mode ? 0 : a.round;  // 0 without adaptation; k >= 1: the slot continues in place from its row of next
    __shared__ PointLds<SPL, W> ws;
    __shared__ double cur[MP_MAX_NDIM];      // the walk's current point
    __shared__ double prop[MP_MAX_NDIM];     // the step's proposal across the evaluation
    __shared__ double lnu;                   // the step's ln u
    __shared__ int go;                       // 1: the proposal lies in the box (evaluate it)
    tables_init<SPL * W, 64 * W>(sh, ws.tt);
    const int nd = a.ndim, n = a.n, base = r * n;
    const int steps = a.mode ? 1 : a.walks;
    double lnl_cur = -INFINITY, beta = 0.0, g = a.g0;
    int st_cur = MP_STATUS_OK, n_acc = 0, n_eval = 0, n_bad = 0;
    if (threadIdx.x == 0) {
        int from = base + j;
        if (!a.mode) {
            if (round == 0) from = base + a.anc[base + j];
            lnl_cur = (round ? a.lnl_next : a.lnl_cur)[from];
            st_cur = (round ? a.st_next : a.st_cur)[from];
            beta = a.beta[r];
            if (a.adapt_max) g = a.g[r];
        }
        const double *x0 = round ? a.x_next : a.x_cur;
        for (int d = 0; d < nd; ++d) cur[d] = x0[(size_t)from * nd + d];
    }
    for (int s = round * steps; s < (round + 1) * steps; ++s) {   // the stage's steps, counted across its rounds
        __syncthreads();
        if (threadIdx.x == 0) {
            if (a.mode) {
                for (int d = 0; d < nd; ++d) prop[d] = cur[d];
                go = 1;
            } else {
                uint32_t u[4], v[4];
                philox4x32_10((uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.stage, (uint32_t)r, (uint32_t)j, kSmcCtr + 2u * (uint32_t)s + 1u, u);
                philox4x32_10((uint32_t)a.seed, (uint32_t)(a.seed >> 32), a.stage, (uint32_t)r, (uint32_t)j, kSmcCtr + 2u * (uint32_t)s + 2u, v);
                const int c1 = pick(u01(u[0], u[1]), n), c2 = pick_skip(u01(u[2], u[3]), n, c1);
                const double *x1 = a.x_cur + (size_t)(base + a.anc[base + c1]) * nd;
                const double *x2 = a.x_cur + (size_t)(base + a.anc[base + c2]) * nd;
                go = de_walk_step(cur, x1, x2, g, a.sig3, u01(v[0], v[1]), a.lower, a.upper, nd, prop);
                lnu = log(u01(v[2], v[3]));
            }
        }
        __syncthreads();
        if (!go) continue;                     // (uniform: LDS behind the barrier)
        double lnp;
        int status;
        point_eval<SPL, LONG, W, OCC>(sh, ws, a.ds_id, nd, a.target, r, prop, lnp, status);
        if (threadIdx.x == 0) {
            ++n_eval;
            n_bad += status != MP_STATUS_OK ? 1 : 0;
            // prior x L^beta: beta lnl(q) - beta lnl(cur) > ln u, the products rounded on their own
            if (a.mode || sub_rn(mul_rn(beta, lnp), mul_rn(beta, lnl_cur)) > lnu) {
                for (int d = 0; d < nd; ++d) cur[d] = prop[d];
                lnl_cur = lnp;
                st_cur = status;
                n_acc += a.mode ? 0 : 1;
            }
        }
    }
    if (threadIdx.x == 0) {
        const size_t row = (size_t)(base + j);
        double *xo = a.mode ? a.x_cur : a.x_next;
        for (int d = 0; d < nd; ++d) xo[row * nd + d] = cur[d];
        (a.mode ? a.lnl_cur : a.lnl_next)[row] = lnl_cur;
        (a.mode ? a.st_cur : a.st_next)[row] = st_cur;
        a.acc[row] = round ? a.acc[row] + n_acc : n_acc;
        atomicAdd((unsigned long long *)&a.ncall[r], (unsigned long long)n_eval);
        if (n_acc) atomicAdd((unsigned long long *)&a.nacc[r], (unsigned long long)n_acc);
        if (n_bad) atomicAdd((unsigned long long *)&a.nfail[r], (unsigned long long)n_bad);
    }
}

// Behind round a.round of an adaptive stage, run blockIdx.x (include/magprop_amd.h states the arithmetic): per dimension the
// correlation over the slots between where a slot started, cur[anc[j]], and where it is, next[j]; the decision; at the round
// that stops, the stage's row of the tuning log and the run's g for the next stage.
__global__ __launch_bounds__(kWgThreads) void smc_tune_kernel(const SmcArgs a) {
    const int r = (int)blockIdx.x, n = a.n, nd = a.ndim, base = r * n, tid = (int)threadIdx.x;
    if (a.nstage[r] != (int)a.stage + 1 || !a.moving[r] || a.rounds[r] != a.round) return;   // (uniform, before the first barrier)
    __shared__ double shd[kWgWaves];
    __shared__ uint32_t shc[kWgWaves];
    const double *xa = a.x_cur, *xb = a.x_next + (size_t)base * nd;
    const int32_t *anc = a.anc + base;
    double rho = -INFINITY;
    for (int d = 0; d < nd; ++d) {
        double sa = 0.0, sb = 0.0, la = INFINITY, ua = -INFINITY, lb = INFINITY, ub = -INFINITY;
        for (int i = tid; i < n; i += kWgThreads) {
            const double va = xa[(size_t)(base + anc[i]) * nd + d], vb = xb[(size_t)i * nd + d];
            sa = add_rn(sa, va);
            sb = add_rn(sb, vb);
            la = fmin(la, va);
            ua = fmax(ua, va);
            lb = fmin(lb, vb);
            ub = fmax(ub, vb);
        }
        const double ma = wg_sum(sa, shd) / (double)n, mb = wg_sum(sb, shd) / (double)n;
        la = wg_min(la, shd);
        ua = wg_max(ua, shd);
        lb = wg_min(lb, shd);
        ub = wg_max(ub, shd);
        double rho_d;
        if (lb == ub) rho_d = 1.0;               // every slot at one value, Sbb = 0: nothing has spread
        else if (la == ua) rho_d = 0.0;          // Saa = 0: every slot started from one point
        else {
            double ha = 0.0, hb = 0.0;           // the largest centred sizes: 2^-ilogb of them scales the squares into range
            for (int i = tid; i < n; i += kWgThreads) {
                ha = fmax(ha, fabs(sub_rn(xa[(size_t)(base + anc[i]) * nd + d], ma)));
                hb = fmax(hb, fabs(sub_rn(xb[(size_t)i * nd + d], mb)));
            }
            ha = wg_max(ha, shd);
            hb = wg_max(hb, shd);
            const int ea = -ilogb(ha), eb = -ilogb(hb);
            double saa = 0.0, sbb = 0.0, sab = 0.0;
            for (int i = tid; i < n; i += kWgThreads) {
                const double u = ldexp(sub_rn(xa[(size_t)(base + anc[i]) * nd + d], ma), ea);
                const double v = ldexp(sub_rn(xb[(size_t)i * nd + d], mb), eb);
                saa = add_rn(saa, mul_rn(u, u));
                sbb = add_rn(sbb, mul_rn(v, v));
                sab = add_rn(sab, mul_rn(u, v));
            }
            saa = wg_sum(saa, shd);
            sbb = wg_sum(sbb, shd);
            sab = wg_sum(sab, shd);
            rho_d = sab / sqrt(mul_rn(saa, sbb));
        }
        if (a.rho_d && tid == 0) a.rho_d[(size_t)r * nd + d] = rho_d;
        if (rho_d > rho || rho_d != rho_d) rho = rho_d;   // the largest; a NaN stays
    }
    uint32_t mine = 0;
    for (int i = tid; i < n; i += kWgThreads) mine += (uint32_t)a.acc[base + i];
    const uint32_t accepted = wg_count(mine, shc);
    if (tid == 0) {
        const int made = a.round + 1;
        a.rounds[r] = made;
        if (made < a.adapt_min || (!(rho <= a.corr) && made < a.adapt_max)) return;   // another round
        a.moving[r] = 0;
        const size_t row = (size_t)r * MP_SMC_MAX_STAGES + (size_t)a.stage;
        const double g = a.g[r];
        a.tune_rounds[row] = made;
        a.tune_log[row * kSmcTuneCols] = g;
        a.tune_log[row * kSmcTuneCols + 1] = rho;
        const double share = (double)accepted / mul_rn((double)n, (double)(made * a.walks));
        a.g[r] = fmin(fmax(mul_rn(g, exp(mul_rn(a.gain, sub_rn(share, a.accept_target)))), a.g_min), a.g_max);
    }
}

}  // namespace

int launch_smc_stage(const SmcArgs &a, void *stream) {
    if (a.n_runs <= 0) return 0;
    hipLaunchKernelGGL(smc_stage_kernel, dim3((unsigned)a.n_runs), dim3(kWgThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int launch_smc_tune(const SmcArgs &a, void *stream) {
    if (a.n_runs <= 0) return 0;
    hipLaunchKernelGGL(smc_tune_kernel, dim3((unsigned)a.n_runs), dim3(kWgThreads), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// One workgroup per particle: n_runs * n
int launch_smc_move(const DevShared &sh, const SmcArgs &a, void *stream) {
    const int n = a.n_runs * a.n;
    if (n <= 0) return 0;
    return launch_point_kernel(sh, n, [&](auto build, auto lng) {
        using B = decltype(build);
        hipLaunchKernelGGL((smc_move_kernel<B::SPL, lng, B::W, B::OCC>), dim3((unsigned)n), dim3(64 * B::W), 0, (hipStream_t)stream, sh, a);
    });
}

}  // namespace mp

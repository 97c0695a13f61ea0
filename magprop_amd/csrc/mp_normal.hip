// mp_normal.hip — gfx950 kernels of the Gaussian (Metropolis) and walk moves of the device-resident sampler
// (include/magprop_amd.h MP_MOVE_GAUSSIAN: emcee's GaussianMove; MP_MOVE_WALK: Goodman & Weare 2010's walk move, emcee's WalkMove).
//
// normal_half_kernel: one workgroup per slot of the active half, on the shell of mp_point.h; the block-to-ensemble mapping through
// slot_lo and ens_order is stretch_kernel's.  The workgroup forms the proposal into an LDS park -- the walk move with every lane
// (members of the other half, strided sums, one normal per member), the Gaussian move with lane 0 -- evaluates it through the one
// point_eval call of the kernel, and lane 0 decides and commits.  The other half is only read and the active walker only written
// by its own workgroup, so the workgroups need no hand-off among themselves.
// gauss_tune_kernel: one thread per ensemble, behind the second half-step of a Gaussian step: folds the step's count of accepted
// proposals into the totals and tunes sigma.
#include <hip/hip_runtime.h>

#include "mp_normal.h"
#include "mp_normal_pair.h"
#include "mp_point.h"

namespace mp {

namespace {

constexpr uint32_t kGaussCtr = 0x47410000u;        // fourth counter word: axis and ln u; + 1 + p: normals 2p, 2p + 1
constexpr uint32_t kWalkCtr = 0x57410000u;         // ln u
constexpr uint32_t kWalkMemberCtr = 0x57410100u;   // + i / 2: Floyd's draws i (words 0, 1 for even i, 2, 3 for odd i)
constexpr uint32_t kWalkNormalCtr = 0x57800000u;   // + p: normals 2p, 2p + 1

MP_DEV void normal_draw(const StretchArgs &g, int k, uint32_t c3, uint32_t (&out)[4]) {
    philox4x32_10((uint32_t)g.seed, (uint32_t)(g.seed >> 32), (uint32_t)g.step, (uint32_t)g.half, (uint32_t)k, c3, out);
}

// The LDS of a proposal beside the parked proposal itself (an array of its own, as in slice_half_kernel): what outlives the
// proposal stage is lnu, beta and lnp_old, read by lane 0 behind the evaluation.
template <int W>
struct NormalPark {
    double part[W][MP_MAX_NDIM];      // walk: per wavefront, its sums over the members
    double lnu, beta, lnp_old;        // ln u, the ensemble's inverse temperature, the walker's lnprob now
    int32_t member[MP_WALK_MAX_S];    // walk: Floyd's subset of the other half's slots
};

// Every thread of the workgroup (W wavefronts) calls this; leaves the proposal in prop (zero beyond ndim) behind a workgroup
// barrier.  Sums over the members: thread t takes i = t, t + 64 W, ... in order, then a butterfly over the wavefront (wave_sum),
// then the W wavefronts' partials in order (kde_proposal's order).  Unfused, like the other moves.
template <int W>
MP_DEV void walk_proposal(const StretchArgs &g, int s_arg, int k, int base, const int32_t *perm, NormalPark<W> &pk, double *prop) {
    constexpr int NT = 64 * W;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, d = g.ndim;
    const int n_comp = g.n_walkers - g.n_half;
    const int32_t *comp = perm + (1 - g.half) * g.n_half;
    const double *pos = g.pos + (size_t)base * d;
    const bool all = s_arg >= n_comp;                               // member_i = i
    const int s = all ? n_comp : min(s_arg, MP_WALK_MAX_S);
    if (!all && t == 0) {   // Floyd: s distinct slots of n_comp
        for (int i = 0; i < s; ++i) {
            uint32_t u[4];
            normal_draw(g, k, kWalkMemberCtr + (uint32_t)(i >> 1), u);
            const int j = n_comp - s + i;
            int m = pick((i & 1) ? u01(u[2], u[3]) : u01(u[0], u[1]), j + 1);
            for (int e = 0; e < i; ++e)
                if (pk.member[e] == m) {
                    m = j;
                    break;
                }
            pk.member[i] = m;
        }
    }
    __syncthreads();
    // 1. the mean of the members
    double mu[MP_MAX_NDIM];
    {
        double acc[MP_MAX_NDIM];
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a) acc[a] = 0.0;
        for (int i = t; i < s; i += NT) {
            const double *x = pos + (size_t)comp[all ? i : pk.member[i]] * d;
#pragma unroll
            for (int a = 0; a < MP_MAX_NDIM; ++a)
                if (a < d) acc[a] = add_rn(acc[a], x[a]);
        }
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a)
            if (a < d) {
                const double v = wave_sum(acc[a]);
                if (lane == 0) pk.part[wave][a] = v;
            }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a) {
            double m = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) m = a < d ? add_rn(m, pk.part[w][a]) : 0.0;
            mu[a] = m / (double)s;
        }
        __syncthreads();   // (part is written again below)
    }
    // 2. sum_i z_i (x_member_i - m)
    {
        double acc[MP_MAX_NDIM];
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a) acc[a] = 0.0;
        for (int i = t; i < s; i += NT) {
            const double *x = pos + (size_t)comp[all ? i : pk.member[i]] * d;
            uint32_t s4[4];
            normal_draw(g, k, kWalkNormalCtr + (uint32_t)(i >> 1), s4);
            double n0, n1;
            normal_pair(s4, n0, n1);
            const double z = (i & 1) ? n1 : n0;
#pragma unroll
            for (int a = 0; a < MP_MAX_NDIM; ++a)
                if (a < d) acc[a] = add_rn(acc[a], mul_rn(z, sub_rn(x[a], mu[a])));
        }
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a)
            if (a < d) {
                const double v = wave_sum(acc[a]);
                if (lane == 0) pk.part[wave][a] = v;
            }
    }
    __syncthreads();
    if (t == 0) {
        const double den = sqrt((double)(s - 1));
        const double *xk = g.pos + (size_t)k * d;
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a) {
            double m = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) m = a < d ? add_rn(m, pk.part[w][a]) : 0.0;
            prop[a] = a < d ? add_rn(xk[a], m / den) : 0.0;
        }
    }
    __syncthreads();
}

// Lane 0: the Gaussian proposal of walker k into prop.  r: the draw of kGaussCtr (its words 0, 1 choose the axis of RANDOM).
MP_DEV void gauss_proposal(const StretchArgs &g, const NormalArgs &na, int k, int w_ens, const uint32_t (&r)[4], double *prop) {
    const int d = g.ndim;
    const double *xk = g.pos + (size_t)k * d;
    const double sigma = na.sigma[w_ens];
    if (na.mode == MP_GAUSS_VECTOR) {
        double nrm[MP_MAX_NDIM + 1];
#pragma unroll
        for (int p = 0; p < (MP_MAX_NDIM + 1) / 2; ++p)
            if (2 * p < d) {
                uint32_t s4[4];
                normal_draw(g, k, kGaussCtr + 1u + (uint32_t)p, s4);
                normal_pair(s4, nrm[2 * p], nrm[2 * p + 1]);
            }
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a) {
            double q = 0.0;
            if (a < d) {
                double s = 0.0;
#pragma unroll
                for (int b = 0; b <= a; ++b) s = add_rn(s, mul_rn(na.L[a * (a + 1) / 2 + b], nrm[b]));
                q = add_rn(xk[a], mul_rn(sigma, s));
            }
            prop[a] = q;
        }
        return;
    }
    const int axis = na.mode == MP_GAUSS_RANDOM ? pick(u01(r[0], r[1]), d) : (int)(g.step % (uint32_t)d);
    uint32_t s4[4];
    normal_draw(g, k, kGaussCtr + 1u, s4);
    double n0, n1;
    normal_pair(s4, n0, n1);
    for (int a = 0; a < MP_MAX_NDIM; ++a) prop[a] = a < d ? xk[a] : 0.0;
    prop[axis] = add_rn(xk[axis], mul_rn(sigma, mul_rn(na.L[axis * (axis + 1) / 2 + axis], n0)));
}

// One workgroup per slot of the active half; builds and template arguments as the kernels of mp_point.h.
template <int SPL, bool LONG, int W = 1, int OCC = 0>
MP_POINT_KERNEL(SPL, W, OCC) void normal_half_kernel(const DevShared sh, const StretchArgs g, const NormalArgs na) {
    __shared__ PointLds<SPL, W> ws;
    __shared__ NormalPark<W> pk;
    __shared__ double prop[MP_MAX_NDIM];     // the proposal across the evaluation
    tables_init<SPL * W, 64 * W>(sh, ws.tt);
    const int gs = g.slot_lo + (int)blockIdx.x;                    // slot of the active half, all ensembles flattened
    const int w_ens = ens_of_slot(g, gs / g.n_half);               // which ensemble (longest light curve first)
    const int slot = gs % g.n_half;                                // which walker of the active half
    const int32_t *perm = g.perm + (size_t)w_ens * g.n_walkers;    // this step's random split of the ensemble
    const int base = w_ens * g.n_walkers;
    const int k = base + perm[g.half * g.n_half + slot];           // active walker (global index)
    const int nd = g.ndim;
    const bool gauss = g.move == MP_MOVE_GAUSSIAN;
    if (threadIdx.x == 0) {
        uint32_t r[4];
        normal_draw(g, k, gauss ? kGaussCtr : kWalkCtr, r);
        pk.lnu = log(u01(r[2], r[3]));
        pk.beta = g.beta ? g.beta[w_ens] : 1.0;
        pk.lnp_old = g.lnprob[k];
        if (gauss) gauss_proposal(g, na, k, w_ens, r, prop);
    }
    if (gauss) __syncthreads();                                    // (uniform: a launch argument)
    else walk_proposal<W>(g, na.walk_s, k, base, perm, pk, prop);
    // Nothing of the proposal stays live across point_eval (which needs every register): it is read back from LDS behind it.
    double lnp = 0.0;
    int status = MP_STATUS_OK;
    point_eval<SPL, LONG, W, OCC>(sh, ws, g.ds_id, nd, g.target, k, prop, lnp, status);
    if (threadIdx.x == 0) {
        const double lnp_old = pk.lnp_old;
        const bool accept = sub_rn(mul_rn(pk.beta, lnp), mul_rn(pk.beta, lnp_old)) > pk.lnu;   // false for NaN / -inf proposals
        if (accept) {
            for (int d = 0; d < nd; ++d) g.pos[(size_t)k * nd + d] = prop[d];
            g.lnprob[k] = lnp;
            g.n_accepted[k] += 1;
            if (gauss) atomicAdd((unsigned long long *)&na.acc_s[w_ens], 1ull);
        }
        if (g.chain) {
            double *c = g.chain + ((size_t)g.chain_row * g.n_total + k) * nd;
            for (int d = 0; d < nd; ++d) c[d] = g.pos[(size_t)k * nd + d];   // (the position AFTER the decision)
            g.chain_lnp[(size_t)g.chain_row * g.n_total + k] = accept ? lnp : lnp_old;
        }
        fbad_append(g, status, prop);
    }
}

// The rule of include/magprop_amd.h on the step's accepted proposals a of ensemble e: r = a / n_walkers, f = (r + t) / (2 t), g =
// 8 / (8 + n_tuned), sigma <- sigma (1 + g (f - 1)), while fewer than tune_steps updates have been made.  Every operation is
// rounded separately.
__global__ __launch_bounds__(64) void gauss_tune_kernel(const NormalArgs na, int n_ensembles, int n_walkers) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= n_ensembles) return;
    const int64_t a = na.acc_s[e];
    na.n_accepted[e] += a;
    na.n_proposed[e] += n_walkers;
    na.acc_s[e] = 0;
    if (na.n_tuned[e] < na.tune_steps) {
        const double t = na.target_accept;
        const double r = (double)a / (double)n_walkers;
        const double f = add_rn(r, t) / mul_rn(2.0, t);
        const double gain = 8.0 / add_rn(8.0, (double)na.n_tuned[e]);
        na.sigma[e] = mul_rn(na.sigma[e], add_rn(1.0, mul_rn(gain, sub_rn(f, 1.0))));
        na.n_tuned[e] += 1;
    }
}

}  // namespace

int launch_normal_half(const DevShared &sh, const StretchArgs &g, const NormalArgs &na, void *stream) {
    const int n = g.n_half * g.n_ensembles;
    if (n <= 0) return 0;
    return launch_point_kernel(sh, n, [&](auto build, auto lng) {
        using B = decltype(build);
        hipLaunchKernelGGL((normal_half_kernel<B::SPL, lng, B::W, B::OCC>), dim3((unsigned)n), dim3(64 * B::W), 0, (hipStream_t)stream, sh, g, na);
    });
}

int launch_gauss_tune(const NormalArgs &na, int n_ensembles, int n_walkers, void *stream) {
    if (n_ensembles <= 0) return 0;
    hipLaunchKernelGGL(gauss_tune_kernel, dim3((unsigned)((n_ensembles + 63) / 64)), dim3(64), 0, (hipStream_t)stream, na, n_ensembles, n_walkers);
    return (int)hipGetLastError();
}

}  // namespace mp

// mp_kernels.hip — gfx950 (CDNA4) kernels of the magnetar log-posterior hot path and their launchers.
//
// Layout: ONE WALKER PER WAVEFRONT, SPL CONSECUTIVE TIME STEPS PER LANE.  The 10 000 grid intervals are processed in
// tiles of 64*SPL steps; inside a tile all steps advance at once (parallel in time).  Scheme = exponential
// Adams-Moulton of order 5 on geometric grids (serial restatement: oracle/mp_oracle.c
// mpo_trajectory_mode): a tile's step spans 1/8 (the first 32 intervals), 1, 2, 4 or 8 grid intervals, chosen tile by tile
// from the solution's smoothness; the states at skipped grid points come from the step's Hermite interpolant.
// Per tile (mp_eval.hpp, walker_eval):
//
//   1. Mdisc obeys dM/dt = Mdotfb(t) - M/tvisc (linear, omega-independent; reference RHS
//      code/synthetic_datasets/funcs.py:122-129, magnetar/funcs.py:86-92).  Every lane evaluates Mdotfb at its step
//      ends, fetches the four previous values from its neighbour (DPP), builds and composes the affine maps
//      M_{j+1} = e^{-h/tvisc} M_j + b_j of its steps; a wavefront scan of affine maps yields Mdisc at all step ends.
//   2. omega obeys a scalar nonlinear ODE fed by Mdisc(t).  Every lane evaluates omega_dot and its Jacobian lambda
//      ONCE per sweep at its current guess of omega at its step ends, fetches (omega_dot, omega) of the four
//      previous points, and forms the step maps omega_{j+1} = e^{h lambda} omega_j + h sum_m phi_{m+1}(h lambda) g_m.
//      A second affine scan propagates the tile's start value through all linearised maps.  This Newton-type sweep
//      contracts by 1e-2..1e-3 per pass (about 2 sweeps from an extrapolated guess, the last one being the convergence
//      check), terminates in any case after at most tile-length sweeps, and reproduces the serial recurrence to ~1e-11.
//   3. Observations.  np.interp needs the model only at the two grid points bracketing each observed time: when an
//      observation falls in the tile, the tile's (Mdisc, omega) image goes to LDS and the lane that owns the
//      observation keeps the two bracketing states (the first 64 observations, register-resident; their luminosity --
//      reference luminosity stage, code/synthetic_datasets/funcs.py:175-229, magnetar/funcs.py:157-210 -- is evaluated
//      once, after the last tile) or scores it at once from the image (observations 64.. of a longer light curve).
//      When curve outputs are requested (CURVES) the luminosity is evaluated at every step end instead, the
//      tile's light curve is staged in LDS for the interpolation and written to HBM with coalesced stores.
//   4. A wavefront reduction of the per-lane chi^2 terms gives -0.5*chi^2 (code/synthetic_datasets/mcmc_eqns.py:25).
//
// Kernels: lnprob_kernel<CURVES, SPL, LONG> (one wavefront per walker), stretch_kernel<SPL, LONG> (emcee's stretch
// move fused around it) and stretch_apply_kernel (the state update of a half-step whose proposals were evaluated
// on several GPUs); LONG = built with the path for light curves of more than 64 points.  Tempered samplers (parallel
// tempering) take their decisions against beta x lnprob and run stretch_swap_kernel after every step.  The DIFF builds of
// stretch_kernel propose emcee's differential-evolution and snooker moves instead, the KDE builds emcee's KDE move
// (mp_sampler_set_moves).
// No MFMA (no dense contraction anywhere on this path), fp64 throughout; bound by the VALU issue rate of one wave per
// SIMD (profiles/, tools/ubench).  The arithmetic is algebraically simplified with respect to the reference formulas
// (e.g. fastness w = (Rm/Rc)^1.5 = omega*Rm^1.5/sqrt(GM), eta1-eta2 = -tanh); oracle/mp_oracle.c keeps the literal
// formulas and the tests compare the two.
#include <hip/hip_runtime.h>

#include "mp_point.h"

namespace mp {

// ---------------------------------------------------------------- batched log-posterior kernel
// LOG: the build with the per-tile diagnostics (mp_tile_log(h, 1); developer builds: always), launched only on request
#if defined(MP_PHASE_PROFILE) || defined(MP_SWEEP_TRACE) || defined(MP_CORR_TRACE) || defined(MP_ABORT_STUDY)
constexpr bool kAlwaysLog = true;
#else
constexpr bool kAlwaysLog = false;
#endif
template <bool CURVES, int SPL, bool LONG, bool LOG = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SPL >= 4 ? 1 : 2, SPL >= 4 ? 1 : 2))) void lnprob_kernel(const DevShared sh, const LaunchArgs a) {
    __shared__ TileImage<SPL> im;
    __shared__ TimeTable<SPL> tt;
    __shared__ double Lbuf[CURVES ? 8 * 64 * SPL + 1 : 1];   // up to 8 grid points per step
    tables_init<SPL, 64>(sh, tt);
    const int walker = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    double par[MP_MAX_NDIM];
    const double *pw = a.pars + (size_t)walker * a.ndim;
#pragma unroll
    for (int i = 0; i < MP_MAX_NDIM; ++i) par[i] = i < a.ndim ? pw[i] : 0.0;
    double lnp;
    int status, sweeps, tiles;
    if constexpr (CURVES) {
        walker_eval<CURVES, SPL, LONG, LOG>(sh, a, walker, par, im, tt, Lbuf, lnp, status, sweeps, tiles);
    } else {
        // (only the curve kernels serve mp_model_lc: here the parameters are the sampler's and chi^2 is wanted, at compile time)
        LaunchArgs aa = a;
        aa.physical = 0;
        aa.want_chi2 = 1;
        walker_eval<CURVES, SPL, LONG, LOG>(sh, aa, walker, par, im, tt, Lbuf, lnp, status, sweeps, tiles);
    }
    if (threadIdx.x == 0) {
        a.lnprob[walker] = lnp;
        if (a.status) a.status[walker] = status;
        if (a.sweeps) a.sweeps[walker] = sweeps;
        if (a.tiles) a.tiles[walker] = tiles;
    }
}

// The same on a team of W wavefronts per walker (mp_eval.hpp TeamX): launches that would leave SIMDs idle.  One wavefront per
// SIMD (each takes what it needs of the register file), so a workgroup is spread over W SIMDs of its CU.
// OCC = wavefronts resident per SIMD the build is made for: 1 while the launch has a SIMD for every wavefront (n <= n_simd / W),
// 2 for twice as many walkers (256 registers; the walker's constants in scalar registers).
// LONG: built with the path for light curves of more than 64 points (their observations 64.. are scored chunk by chunk, the
// chunks dealt to the team's wavefronts in turn: a walker on a 1 944-point light curve spends a quarter of its time there).
template <int SPL, int W, int OCC, bool LOG = false, bool LONG = false>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(OCC, OCC))) void lnprob_team_kernel(const DevShared sh, const LaunchArgs a) {
    __shared__ TileImage<SPL * W> im;
    __shared__ TimeTable<SPL * W> tt;
    __shared__ TeamX<SPL * W> tx;
    __shared__ double Lbuf[1];
    tables_init<SPL * W, 64 * W>(sh, tt);
    const int walker = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
    double par[MP_MAX_NDIM];
    const double *pw = a.pars + (size_t)walker * a.ndim;
#pragma unroll
    for (int i = 0; i < MP_MAX_NDIM; ++i) par[i] = i < a.ndim ? pw[i] : 0.0;
    double lnp;
    int status, sweeps, tiles;
    LaunchArgs aa = a;
    aa.physical = 0;
    aa.want_chi2 = 1;
    walker_eval<false, SPL, LONG, LOG, W, OCC >= 2>(sh, aa, walker, par, im, tt, Lbuf, lnp, status, sweeps, tiles, &tx);
    if (threadIdx.x == 0) {
        a.lnprob[walker] = lnp;
        if (a.status) a.status[walker] = status;
        if (a.sweeps) a.sweeps[walker] = sweeps;
        if (a.tiles) a.tiles[walker] = tiles;
    }
}

// ---------------------------------------------------------------- launch order of a mixed-length batch
// The hardware starts workgroups in index order, a new one whenever a wave slot frees up.  In a batch whose walkers refer to
// light curves of very different lengths (BASELINE config 5: 8 ... 1 944 points; a walker on the longest costs twice a walker
// on a 50-point set) and that needs more than one round of the device's wave slots, a long walker that starts in the last
// round decides the launch time.  This kernel (one workgroup) sorts the walker indices by the length class of their light
// curve, longest first (counting sort; the order inside a class is immaterial: every walker writes its own outputs only), and
// lnprob_kernel evaluates walker order[blockIdx.x].  4 096-walker launch of config 5: 0.391 -> 0.313 ms on one box.
constexpr int kOrderClasses = 6;
MP_DEV int order_class(const DevShared &sh, const int32_t *ds_id, int i) {
    const int d = ds_id[i];
    const int n_obs = (sh.ds != nullptr && d >= 0 && d < sh.n_ds) ? sh.ds[d].n_obs : 0;
    return n_obs > 1024 ? 0 : (n_obs > 512 ? 1 : (n_obs > 256 ? 2 : (n_obs > 128 ? 3 : (n_obs > 64 ? 4 : 5))));
}
__global__ __launch_bounds__(1024) void order_kernel(const DevShared sh, const int32_t *ds_id, int n, int32_t *order) {
    __shared__ int cnt[kOrderClasses], fill[kOrderClasses];
    const int t = threadIdx.x;
    if (t < kOrderClasses) cnt[t] = 0;
    __syncthreads();
    for (int i = t; i < n; i += 1024) atomicAdd(&cnt[order_class(sh, ds_id, i)], 1);
    __syncthreads();
    if (t == 0) {
        int acc = 0;
        for (int c = 0; c < kOrderClasses; ++c) { fill[c] = acc; acc += cnt[c]; }
    }
    __syncthreads();
    for (int i = t; i < n; i += 1024) order[atomicAdd(&fill[order_class(sh, ds_id, i)], 1)] = i;
}

int launch_order(const DevShared &sh, const int32_t *ds_id, int n, int32_t *order, void *stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(order_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, sh, ds_id, n, order);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- fused stretch-move half-step kernel
// (unfused arithmetic: mul_rn / add_rn / sub_rn, mp_math.hpp)

// One wavefront = one walker of the active half: draw the partner and the stretch factor, form the
// proposal (emcee's StretchMove.get_proposal), evaluate its log-posterior with walker_eval, accept or
// reject against the walker's current value, update position / lnprob / counters in place and write the
// step's row of the chain.  Walkers of the complementary half are only read, so the update is race-free.
// A launch covers the slots [slot_lo, slot_lo + gridDim.x) of the active half (all ensembles flattened).  With g.upd set
// (walker-sharded ensembles, one process per GPU) nothing is updated in place: the outcome of slot s goes to row
// s - slot_lo of g.upd as (proposal[ndim], its lnprob, accepted 0/1) and stretch_apply_kernel commits the rows of all
// ranks after the all-gather.  The random numbers (Philox, mp_device.h) are keyed by (seed; step, half, walker), so every rank
// draws what the single-GPU launch would have drawn for the same walker.
// Half-step launches run the ensembles in the order of StretchArgs::ens_order (mp_sampler.cpp: longest light curve first, four
// bits per position; 0 = the ensembles as they are numbered; ens_of_slot, mp_device.h): the waves that take longest start first,
// as in order_kernel.

// ---- differential-evolution and snooker proposals (the DIFF builds of stretch_kernel; include/magprop_amd.h MP_MOVE_*)
// (index draws over the m slots of the complementary half: pick / pick_skip / pick_skip2, mp_math.hpp)
// The proposal par[] of walker k and, for the snooker move, the sums behind its Hastings term (qq = sum (q - z)^2, dd =
// sum (x_k - z)^2, in index order).  r = Philox(...; c3 = 2), r2 = Philox(...; c3 = 3).  Unfused, like the stretch move.
//   DE (ter Braak 2006):        partners j1, j2;  gamma = g0 (1 + s (2 u - 1));  q = x_k + gamma (x_j1 - x_j2)
//   snooker (ter Braak & Vrugt 2008): partners z, z1, z2;  d = x_k - z;  q = x_k + (gamma_s (d.(z1 - z2)) / (d.d)) d
MP_DEV void diff_proposal(const StretchArgs &g, int k, int base, const int32_t *perm, int n_comp, const uint32_t (&r)[4],
                          const uint32_t (&r2)[4], double (&par)[MP_MAX_NDIM], double &qq, double &dd) {
    const int32_t *comp = perm + (1 - g.half) * g.n_half;
    const double *xk = g.pos + (size_t)k * g.ndim;
    if (g.move == MP_MOVE_DE) {
        const int c1 = pick(u01(r[0], r[1]), n_comp);
        const int c2 = pick_skip(u01(r[2], r[3]), n_comp, c1);
        const double *x1 = g.pos + (size_t)(base + comp[c1]) * g.ndim, *x2 = g.pos + (size_t)(base + comp[c2]) * g.ndim;
        const double gamma = mul_rn(g.de_g0, add_rn(1.0, mul_rn(g.de_s, sub_rn(mul_rn(2.0, u01(r2[0], r2[1])), 1.0))));
#pragma unroll
        for (int i = 0; i < MP_MAX_NDIM; ++i) par[i] = i < g.ndim ? add_rn(xk[i], mul_rn(gamma, sub_rn(x1[i], x2[i]))) : 0.0;
        qq = dd = 1.0;
        return;
    }
    const int cz = pick(u01(r[0], r[1]), n_comp);
    const int c1 = pick_skip(u01(r[2], r[3]), n_comp, cz);
    const int c2 = pick_skip2(u01(r2[0], r2[1]), n_comp, cz, c1);
    const double *z = g.pos + (size_t)(base + comp[cz]) * g.ndim;
    const double *z1 = g.pos + (size_t)(base + comp[c1]) * g.ndim, *z2 = g.pos + (size_t)(base + comp[c2]) * g.ndim;
    double d[MP_MAX_NDIM], p = 0.0;
    dd = 0.0;
#pragma unroll
    for (int i = 0; i < MP_MAX_NDIM; ++i) {
        d[i] = i < g.ndim ? sub_rn(xk[i], z[i]) : 0.0;
        if (i < g.ndim) {
            dd = add_rn(dd, mul_rn(d[i], d[i]));
            p = add_rn(p, mul_rn(d[i], sub_rn(z1[i], z2[i])));
        }
    }
    const double f = mul_rn(g.gamma_s, p / dd);   // dd = 0: NaN, and the Hastings term rejects the proposal
    qq = 0.0;
#pragma unroll
    for (int i = 0; i < MP_MAX_NDIM; ++i) {
        par[i] = i < g.ndim ? add_rn(xk[i], mul_rn(f, d[i])) : 0.0;
        if (i < g.ndim) {
            const double e = sub_rn(par[i], z[i]);
            qq = add_rn(qq, mul_rn(e, e));
        }
    }
}

// ---- the KDE proposal (the KDE builds of stretch_kernel; include/magprop_amd.h MP_MOVE_KDE)
// Emcee's KDEMove over the two-way split: a Gaussian kernel density estimate of the other half C (kernel covariance f^2 S, S
// the sample covariance of C) is both the proposal density, q = x_c + L n, and, through the ratio of its values at x_k and
// q, the Hastings term.  Every workgroup computes the covariance of its ensemble's complement itself: n_comp d^2 operations
// spread over the workgroup's lanes against an evaluation of ~190 k cycles.  Its LDS scratch aliases the tile image, which
// is unused before walker_eval.
constexpr int kKdeTri = MP_MAX_NDIM * (MP_MAX_NDIM + 1) / 2;   // lower triangle, by rows: entry (a, b <= a) at a (a + 1) / 2 + b
constexpr uint32_t kKdeCtr = 0x4B00u;                          // Philox c3: 0x4B00 partner and ln u, 0x4B01 + p normals 2p, 2p + 1
template <int W>
struct KdeScratch {
    double mean[W][MP_MAX_NDIM];   // per wavefront: its sums of the slots
    double cov[W][kKdeTri];        // per wavefront: its sums of the centred products
    double L[kKdeTri];             // Cholesky factor of f^2 S
    double inv_diag[MP_MAX_NDIM];  // 1 / L_aa
    double xk[MP_MAX_NDIM], q[MP_MAX_NDIM];
    double lse[W][4];              // per wavefront: the running log-sum-exp pairs (m, s) at x_k and at q
    int ok;                        // S positive definite
};

// Every thread of the workgroup (W wavefronts) calls this.  Leaves the proposal in park[0 .. MP_MAX_NDIM - 1] (zero beyond
// ndim; NaN where S is not positive definite), the Hastings term in park[MP_MAX_NDIM] and ln u in park[MP_MAX_NDIM + 1],
// behind a workgroup barrier; nothing else outlives it.  Sums over C: thread t takes slots t, t + 64 W, ... in order, then a
// butterfly over the wavefront (wave_sum, wave_lse), then the W wavefronts' partials in order.  Unfused, like the other moves.
template <int W>
MP_DEV void kde_proposal(const StretchArgs &g, int k, int base, const int32_t *perm, int n_comp, const uint32_t (&r)[4],
                         KdeScratch<W> &ks, double *park) {
    constexpr int NT = 64 * W;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, d = g.ndim;
    const int32_t *comp = perm + (1 - g.half) * g.n_half;
    const double *pos = g.pos + (size_t)base * d;
    // 1. the mean of C
    {
        double acc[MP_MAX_NDIM];
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a) acc[a] = 0.0;
        for (int c = t; c < n_comp; c += NT) {
            const double *x = pos + (size_t)comp[c] * d;
#pragma unroll
            for (int a = 0; a < MP_MAX_NDIM; ++a)
                if (a < d) acc[a] = add_rn(acc[a], x[a]);
        }
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a)
            if (a < d) {
                const double v = wave_sum(acc[a]);
                if (lane == 0) ks.mean[wave][a] = v;
            }
    }
    __syncthreads();
    // 2. the centred products, summed over C
    {
        double mu[MP_MAX_NDIM], acc[kKdeTri];
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a) {
            double m = 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) m = a < d ? add_rn(m, ks.mean[w][a]) : 0.0;
            mu[a] = m / n_comp;
        }
#pragma unroll
        for (int p = 0; p < kKdeTri; ++p) acc[p] = 0.0;
        for (int c = t; c < n_comp; c += NT) {
            const double *x = pos + (size_t)comp[c] * d;
            double e[MP_MAX_NDIM];
#pragma unroll
            for (int a = 0; a < MP_MAX_NDIM; ++a) e[a] = a < d ? sub_rn(x[a], mu[a]) : 0.0;
#pragma unroll
            for (int a = 0; a < MP_MAX_NDIM; ++a)
                if (a < d) {
#pragma unroll
                    for (int b = 0; b <= a; ++b) acc[a * (a + 1) / 2 + b] = add_rn(acc[a * (a + 1) / 2 + b], mul_rn(e[a], e[b]));
                }
        }
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a)
            if (a < d) {
#pragma unroll
                for (int b = 0; b <= a; ++b) {
                    const double v = wave_sum(acc[a * (a + 1) / 2 + b]);
                    if (lane == 0) ks.cov[wave][a * (a + 1) / 2 + b] = v;
                }
            }
    }
    __syncthreads();
    // 3. one thread: Sigma = f^2 S (S = sums / (n_comp - 1)), its Cholesky factor by rows, the partner, the normals, q
    if (t == 0) {
        const double f2 = mul_rn(g.kde_f, g.kde_f), nm1 = n_comp - 1.0;
        double L[kKdeTri];
        bool ok = true;
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a)
            if (a < d) {
#pragma unroll
                for (int b = 0; b <= a; ++b) {
                    double s = 0.0;
#pragma unroll
                    for (int w = 0; w < W; ++w) s = add_rn(s, ks.cov[w][a * (a + 1) / 2 + b]);
                    s = mul_rn(f2, s / nm1);
#pragma unroll
                    for (int c = 0; c < b; ++c) s = sub_rn(s, mul_rn(L[a * (a + 1) / 2 + c], L[b * (b + 1) / 2 + c]));
                    if (b == a) {
                        ok = ok && s > 0.0 && s < INFINITY;   // a zero, negative or non-finite pivot
                        L[a * (a + 1) / 2 + a] = sqrt(s);
                    } else {
                        L[a * (a + 1) / 2 + b] = s / L[b * (b + 1) / 2 + b];
                    }
                }
            }
        double nrm[MP_MAX_NDIM + 1];
#pragma unroll
        for (int p = 0; p < (MP_MAX_NDIM + 1) / 2; ++p)
            if (2 * p < d) {   // Box-Muller: sqrt(-2 ln(1 - u_a)) cos, sin (2 pi u_b)
                uint32_t s4[4];
                philox4x32_10((uint32_t)g.seed, (uint32_t)(g.seed >> 32), (uint32_t)g.step, (uint32_t)g.half, (uint32_t)k, kKdeCtr + 1u + p, s4);
                const double rad = sqrt(mul_rn(-2.0, log(sub_rn(1.0, u01(s4[0], s4[1])))));
                const double ang = mul_rn(6.283185307179586, u01(s4[2], s4[3]));
                nrm[2 * p] = mul_rn(rad, cos(ang));
                nrm[2 * p + 1] = mul_rn(rad, sin(ang));
            }
        const double *xc = pos + (size_t)comp[pick(u01(r[0], r[1]), n_comp)] * d;
        const double *xk = g.pos + (size_t)k * d;
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a) {
            double qa = 0.0;
            if (a < d) {
                double s = 0.0;
#pragma unroll
                for (int b = 0; b <= a; ++b) s = add_rn(s, mul_rn(L[a * (a + 1) / 2 + b], nrm[b]));
                qa = ok ? add_rn(xc[a], s) : NAN;
                ks.xk[a] = xk[a];
                ks.q[a] = qa;
                ks.inv_diag[a] = 1.0 / L[a * (a + 1) / 2 + a];
#pragma unroll
                for (int b = 0; b <= a; ++b) ks.L[a * (a + 1) / 2 + b] = L[a * (a + 1) / 2 + b];
            }
            park[a] = qa;
        }
        ks.ok = ok ? 1 : 0;
        park[MP_MAX_NDIM + 1] = log(u01(r[2], r[3]));
    }
    __syncthreads();
    // 4. the two log-sum-exps over C of -|L^-1 (x - x_j)|^2 / 2, x = x_k and x = q (forward substitution)
    const bool ok = ks.ok != 0;
    if (ok) {
        double Lr[kKdeTri], ivd[MP_MAX_NDIM], xk[MP_MAX_NDIM], q[MP_MAX_NDIM];
#pragma unroll
        for (int a = 0; a < MP_MAX_NDIM; ++a)
            if (a < d) {
                ivd[a] = ks.inv_diag[a];
                xk[a] = ks.xk[a];
                q[a] = ks.q[a];
#pragma unroll
                for (int b = 0; b < a; ++b) Lr[a * (a + 1) / 2 + b] = ks.L[a * (a + 1) / 2 + b];
            }
        double m0 = -INFINITY, s0 = 0.0, m1 = -INFINITY, s1 = 0.0;
        for (int c = t; c < n_comp; c += NT) {
            const double *x = pos + (size_t)comp[c] * d;
            double y0[MP_MAX_NDIM], y1[MP_MAX_NDIM], v0 = 0.0, v1 = 0.0;
#pragma unroll
            for (int a = 0; a < MP_MAX_NDIM; ++a)
                if (a < d) {
                    double u0 = sub_rn(xk[a], x[a]), u1 = sub_rn(q[a], x[a]);
#pragma unroll
                    for (int b = 0; b < a; ++b) {
                        u0 = sub_rn(u0, mul_rn(Lr[a * (a + 1) / 2 + b], y0[b]));
                        u1 = sub_rn(u1, mul_rn(Lr[a * (a + 1) / 2 + b], y1[b]));
                    }
                    y0[a] = mul_rn(u0, ivd[a]);
                    y1[a] = mul_rn(u1, ivd[a]);
                    v0 = add_rn(v0, mul_rn(y0[a], y0[a]));
                    v1 = add_rn(v1, mul_rn(y1[a], y1[a]));
                }
            lse_add(m0, s0, mul_rn(-0.5, v0));
            lse_add(m1, s1, mul_rn(-0.5, v1));
        }
        wave_lse(m0, s0);
        wave_lse(m1, s1);
        if (lane == 0) {
            ks.lse[wave][0] = m0;
            ks.lse[wave][1] = s0;
            ks.lse[wave][2] = m1;
            ks.lse[wave][3] = s1;
        }
    }
    __syncthreads();
    if (t == 0) {
        double h = NAN;
        if (ok) {
            double m0 = ks.lse[0][0], s0 = ks.lse[0][1], m1 = ks.lse[0][2], s1 = ks.lse[0][3];
#pragma unroll
            for (int w = 1; w < W; ++w) {
                lse_merge(m0, s0, ks.lse[w][0], ks.lse[w][1]);
                lse_merge(m1, s1, ks.lse[w][2], ks.lse[w][3]);
            }
            h = sub_rn(add_rn(m0, log(s0)), add_rn(m1, log(s1)));
        }
        park[MP_MAX_NDIM] = h;
    }
    __syncthreads();   // (the tile image is free for walker_eval again; park is read behind it)
}

// W, OCC: small ensembles evaluate every proposal on a team of W = 4 wavefronts (lnprob_team_kernel; OCC = wavefronts resident
// per SIMD the build is made for), chosen by the size of a WHOLE step of the sampler (stretch_waves, mp_device.h) so that one
// launch per step and one per half-step run the same arithmetic: the chains stay equal bit for bit.
// TEMPERED: the builds of tempered samplers (g.beta set), which decide against beta x lnprob.  Separate builds, because even a
// read of beta behind the evaluation moves the register allocation of walker_eval (scratch and SGPR spills of the untempered
// builds would change with it); the untempered builds are the code they were.
// DIFF: the builds of the differential-evolution and snooker moves (g.move, decided at run time): only the proposal stage
// differs -- partners, proposal, Hastings term and ln u, from the counters c3 = 2, 3 -- and the stretch builds are the code
// they were.  Evaluation, decision, commit, chain row and failure log are shared.
// KDE: the builds of the KDE move (kde_proposal, DIFF false): the workgroup's proposal stage over the other half, counters
// c3 = 0x4B00 + j; a NaN proposal (S not positive definite) is not evaluated and is rejected.
template <int SPL, bool LONG, int W = 1, int OCC = 0, bool TEMPERED = false, bool DIFF = false, bool KDE = false>
MP_POINT_KERNEL(SPL, W, OCC) void stretch_kernel(const DevShared sh, const StretchArgs g) {
    __shared__ TileImage<SPL * W> im;
    __shared__ TimeTable<SPL * W> tt;
    __shared__ double lds[1];
    __shared__ double park[MP_MAX_NDIM + 3];
    __shared__ TeamLds<SPL * W, (W > 1)> tl;
    TeamX<SPL * W> *const tx = tl.ptr();
    tables_init<SPL * W, 64 * W>(sh, tt);
    const int gs = g.slot_lo + (int)blockIdx.x;                    // slot of the active half, all ensembles flattened
    const int w_ens = ens_of_slot(g, gs / g.n_half);               // which ensemble (longest light curve first)
    const int slot = gs % g.n_half;                                // which walker of the active half
    const int32_t *perm = g.perm + (size_t)w_ens * g.n_walkers;    // this step's random split of the ensemble
    const int base = w_ens * g.n_walkers;
    const int k = base + perm[g.half * g.n_half + slot];           // active walker (global index)
    uint32_t r[4], r2[4];
    philox4x32_10((uint32_t)g.seed, (uint32_t)(g.seed >> 32), (uint32_t)g.step, (uint32_t)g.half, (uint32_t)k, KDE ? kKdeCtr : (DIFF ? 2u : 0u), r);
    philox4x32_10((uint32_t)g.seed, (uint32_t)(g.seed >> 32), (uint32_t)g.step, (uint32_t)g.half, (uint32_t)k, DIFF ? 3u : 1u, r2);
    const int n_comp = g.n_walkers - g.n_half;
    const int jc = (int)(u01(r[0], r[1]) * n_comp);                // partner from the complementary half
    const int j = base + perm[(1 - g.half) * g.n_half + min(jc, n_comp - 1)];
    // (unfused arithmetic below, so that a numpy restatement of the move reproduces the chain bit for bit)
    const double zr = add_rn(mul_rn(g.a - 1.0, u01(r[2], r[3])), 1.0);
    const double zz = mul_rn(zr, zr) / g.a;                      // g(z) ~ 1/sqrt(z) on [1/a, a]
    double par[MP_MAX_NDIM];
    double qq = 1.0, dd = 1.0;   // (DIFF: the snooker move's sums)
    if constexpr (KDE) {
        static_assert(sizeof(KdeScratch<W>) <= sizeof(TileImage<SPL * W>), "the KDE scratch must fit the tile image");
        kde_proposal<W>(g, k, base, perm, n_comp, r, *reinterpret_cast<KdeScratch<W> *>(&im), park);
#pragma unroll
        for (int i = 0; i < MP_MAX_NDIM; ++i) par[i] = park[i];
    } else if constexpr (DIFF) {
        // (the stretch draw above is dead code here; it stays first because moving it into the else branch changed the SGPR
        // spills of four stretch builds)
        diff_proposal(g, k, base, perm, n_comp, r, r2, par, qq, dd);
    } else {
#pragma unroll
        for (int i = 0; i < MP_MAX_NDIM; ++i) {
            const double xk = i < g.ndim ? g.pos[(size_t)k * g.ndim + i] : 0.0;
            const double xj = i < g.ndim ? g.pos[(size_t)j * g.ndim + i] : 0.0;
            par[i] = sub_rn(xj, mul_rn(sub_rn(xj, xk), zz));
        }
    }
    // Nothing of the draw stays live across walker_eval (which needs every register): lane 0 parks the proposal, the
    // acceptance threshold and the walker's current value in LDS and reads them back behind the evaluation.
    //   park[0 .. ndim-1] proposal, [ndim] Hastings term ((ndim - 1) ln z; DE 0; snooker (ndim - 1)/2 ln(qq / dd)),
    //   [ndim + 1] ln u, [ndim + 2] lnprob of the walker now
    const bool lane0 = W > 1 ? threadIdx.x == 0 : (threadIdx.x & 63) == 0;   // (of the team's first wavefront)
    double lnp = 0.0;
    if (g.target == 1) {   // isotropic unit Gaussian: exercises the move itself (tests)
#pragma unroll
        for (int i = 0; i < MP_MAX_NDIM; ++i) lnp = i < g.ndim ? sub_rn(lnp, mul_rn(mul_rn(0.5, par[i]), par[i])) : lnp;
    }
    if (lane0) {
        if constexpr (!KDE) {   // (the KDE stage has parked its proposal, Hastings term and ln u)
#pragma unroll
            for (int i = 0; i < MP_MAX_NDIM; ++i) park[i] = par[i];
            if constexpr (!DIFF) {
                park[MP_MAX_NDIM] = mul_rn(g.ndim - 1.0, log(zz));
                park[MP_MAX_NDIM + 1] = log(u01(r2[0], r2[1]));
            } else {
                park[MP_MAX_NDIM] = g.move == MP_MOVE_DE ? 0.0 : mul_rn(mul_rn(0.5, g.ndim - 1.0), sub_rn(log(qq), log(dd)));
                park[MP_MAX_NDIM + 1] = log(u01(r2[2], r2[3]));
            }
        }
        park[MP_MAX_NDIM + 2] = g.lnprob[k];
    }
    int status = MP_STATUS_OK, sweeps, tiles;
    if (g.target != 1 && !(KDE && par[0] != par[0])) {   // (KDE: a NaN proposal keeps lnp = 0, its Hastings term NaN rejects it)
        LaunchArgs a{};
        a.ds_id = g.ds_id;
        a.ndim = g.ndim;
        a.physical = 0;
        a.want_chi2 = 1;
        if constexpr (W > 1) walker_eval<false, SPL, LONG, false, W, OCC >= 2>(sh, a, k, par, im, tt, lds, lnp, status, sweeps, tiles, tx);
        else walker_eval<false, SPL, LONG>(sh, a, k, par, im, tt, lds, lnp, status, sweeps, tiles);
    }
    if (lane0) {   // lane 0 of the evaluating wavefront (team: of its first one)
        const double lnp_old = park[MP_MAX_NDIM + 2];
        double lnpdiff;
        if constexpr (TEMPERED) {
            // target prior x L^beta: with a box prior the test is beta (lnprob(proposal) - lnprob(walker)); beta = 1 gives the
            // untempered test bit for bit (mul_rn(1, x) == x).  beta is read here, behind the evaluation, from the walker's ensemble
            const double beta = g.beta[k / g.n_walkers];
            lnpdiff = sub_rn(add_rn(park[MP_MAX_NDIM], mul_rn(beta, lnp)), mul_rn(beta, lnp_old));
        } else {
            lnpdiff = sub_rn(add_rn(park[MP_MAX_NDIM], lnp), lnp_old);
        }
        const bool accept = lnpdiff > park[MP_MAX_NDIM + 1];      // false for NaN / -inf proposals
        if (g.upd) {
            double *u = g.upd + (size_t)blockIdx.x * (g.ndim + 3);
            for (int i = 0; i < g.ndim; ++i) u[i] = park[i];
            u[g.ndim] = lnp;
            u[g.ndim + 1] = accept ? 1.0 : 0.0;
            u[g.ndim + 2] = (double)status;
        } else {
            // (commit_outcome's sequence, written out: routing this kernel through the helper changes its register allocation)
            if (accept) {
                for (int i = 0; i < g.ndim; ++i) g.pos[(size_t)k * g.ndim + i] = park[i];
                g.lnprob[k] = lnp;
                g.n_accepted[k] += 1;
            }
            if (g.chain) {
                double *c = g.chain + ((size_t)g.chain_row * g.n_total + k) * g.ndim;
                // (the walker's position AFTER the decision: written just above when the proposal was accepted.  A select between
                // the LDS slot and the global row made the compiler select the ADDRESS and load through a generic pointer:
                // nine flat loads and a private segment reserved for their sake)
                for (int i = 0; i < g.ndim; ++i) c[i] = g.pos[(size_t)k * g.ndim + i];
                g.chain_lnp[(size_t)g.chain_row * g.n_total + k] = accept ? lnp : lnp_old;
            }
            if (g.bad_log && (status == MP_STATUS_FLAG || status == MP_STATUS_NONFINITE)) {
                // the reference appends such parameter sets to its `fbad` file (code/synthetic_datasets/mcmc_eqns.py:72-79)
                const unsigned slot_b = atomicAdd(g.bad_count, 1u);
                if (slot_b < g.bad_cap)
                    for (int i = 0; i < g.ndim; ++i) g.bad_log[(size_t)slot_b * g.ndim + i] = park[i];
            }
        }
    }
}

// The commit of a decision on walker k (see stretch_kernel, which commits the same way from LDS): an accepted proposal u[0 ..
// ndim - 1] of log-posterior lnp becomes the walker's state, the step's chain row is written from the state after the update, and
// a proposal whose model failed goes to the fbad log.  lnp_old: the walker's log-posterior before the decision.
MP_DEV void commit_outcome(const StretchArgs &g, int k, bool accept, const double *u, double lnp, double lnp_old, int status) {
    if (accept) {
        for (int i = 0; i < g.ndim; ++i) g.pos[(size_t)k * g.ndim + i] = u[i];
        g.lnprob[k] = lnp;
        g.n_accepted[k] += 1;
    }
    if (g.chain) {
        double *c = g.chain + ((size_t)g.chain_row * g.n_total + k) * g.ndim;
        for (int i = 0; i < g.ndim; ++i) c[i] = g.pos[(size_t)k * g.ndim + i];
        g.chain_lnp[(size_t)g.chain_row * g.n_total + k] = accept ? lnp : lnp_old;
    }
    fbad_append(g, status, u);
}

// Commit one half-step from the gathered outcome rows (see stretch_kernel): one thread per slot of the active half.
__global__ __launch_bounds__(256) void stretch_apply_kernel(const StretchArgs g) {
    const int gs = blockIdx.x * 256 + threadIdx.x;
    if (gs >= g.n_half * g.n_ensembles) return;
    const int w_ens = ens_of_slot(g, gs / g.n_half), slot = gs % g.n_half;
    const int k = w_ens * g.n_walkers + g.perm[(size_t)w_ens * g.n_walkers + g.half * g.n_half + slot];
    const double *u = g.upd + (size_t)gs * (g.ndim + 3);
    commit_outcome(g, k, u[g.ndim + 1] != 0.0, u, u[g.ndim], g.lnprob[k], (int)u[g.ndim + 2]);
}

// ---------------------------------------------------------------- a whole stretch-move step in one launch
// A half-step of a small ensemble leaves most of the chip idle: 512 proposals on the 1 024 SIMDs of an MI355X, and the second
// half-step cannot start before the first has decided.  But everything the second half needs is known up front except those
// decisions: walker k of the second half moves along the line to its partner j of the first half, who will stand either
// where it stands now or at its own proposal Y_j, and Y_j is known before it is evaluated.  One launch therefore evaluates
// the n/2 proposals of the first half AND, for every walker of the second half, BOTH candidate proposals (3 n/2 evaluations,
// n/2 of them discarded); stretch_step_commit_kernel then takes the first half's decisions, picks the candidate that matches
// the partner's outcome and decides on it.  The chain is the one the two half-step launches produce, bit for bit (same
// random numbers, same arithmetic, same order of decisions).  Used when 3 n/2 waves fit the device two per SIMD.
//
// Block b of 3 * slots: type = b / slots (0: first half; 1: second half, partner where it stands; 2: second half, partner at
// its proposal), slot = b % slots.  Outcome row of block b = proposal[ndim], lnprob, status, (ndim - 1) ln z, ln u,
// lnprob of the walker before the move, partner's slot; written at row b - slot_lo of g.spec (walker-sharded ensembles: every
// rank evaluates its share of the blocks, the rows are all-gathered, stretch_step_commit_kernel runs on every rank).
MP_DEV void stretch_draw(const StretchArgs &g, int half, int k, int n_comp, int &jc, double &zz, double &logu) {
    uint32_t r[4], r2[4];
    philox4x32_10((uint32_t)g.seed, (uint32_t)(g.seed >> 32), (uint32_t)g.step, (uint32_t)half, (uint32_t)k, 0u, r);
    philox4x32_10((uint32_t)g.seed, (uint32_t)(g.seed >> 32), (uint32_t)g.step, (uint32_t)half, (uint32_t)k, 1u, r2);
    jc = min((int)(u01(r[0], r[1]) * n_comp), n_comp - 1);
    const double zr = add_rn(mul_rn(g.a - 1.0, u01(r[2], r[3])), 1.0);
    zz = mul_rn(zr, zr) / g.a;
    logu = log(u01(r2[0], r2[1]));
}

template <int SPL, bool LONG, int W = 1, int OCC = 0>   // (W, OCC: as in stretch_kernel)
MP_POINT_KERNEL(SPL, W, OCC) void stretch_step_kernel(const DevShared sh, const StretchArgs g) {
    __shared__ TileImage<SPL * W> im;
    __shared__ TimeTable<SPL * W> tt;
    __shared__ double lds[1];
    __shared__ TeamLds<SPL * W, (W > 1)> tl;
    TeamX<SPL * W> *const tx = tl.ptr();
    tables_init<SPL * W, 64 * W>(sh, tt);
    const int n_slots = g.n_half * g.n_ensembles;
    const int blk = g.slot_lo + (int)blockIdx.x;                    // a launch covers blocks [slot_lo, slot_lo + gridDim.x) (sharded: a rank's share)
    const int type = blk / n_slots, gs = blk - type * n_slots;
    const int half = type == 0 ? 0 : 1;
    const int w_ens = gs / g.n_half, slot = gs - w_ens * g.n_half;
    const int32_t *perm = g.perm + (size_t)w_ens * g.n_walkers;
    const int base = w_ens * g.n_walkers;
    const int n_comp = g.n_walkers - g.n_half;
    const int k = base + perm[half * g.n_half + slot];
    int jc;
    double zz, logu;
    stretch_draw(g, half, k, n_comp, jc, zz, logu);
    const int j = base + perm[(1 - half) * g.n_half + jc];
    double xj[MP_MAX_NDIM];
#pragma unroll
    for (int i = 0; i < MP_MAX_NDIM; ++i) xj[i] = i < g.ndim ? g.pos[(size_t)j * g.ndim + i] : 0.0;
    bool skip = false;
    if (type == 2) {
        // the partner's own proposal of the first half-step (the arithmetic of its type-0 block, bit for bit)
        int jcj;
        double zzj, loguj;
        stretch_draw(g, 0, j, n_comp, jcj, zzj, loguj);
        const int jj = base + perm[g.n_half + jcj];
        bool outside = false;
#pragma unroll
        for (int i = 0; i < MP_MAX_NDIM; ++i) {
            const double xjj = i < g.ndim ? g.pos[(size_t)jj * g.ndim + i] : 0.0;
            xj[i] = sub_rn(xjj, mul_rn(sub_rn(xjj, xj[i]), zzj));
            if (g.target == 0 && i < sh.n_prior && (!(xj[i] >= sh.lower[i]) || !(xj[i] <= sh.upper[i]))) outside = true;
        }
        skip = outside;   // a proposal outside the prior box is never accepted: this candidate cannot be the one
    }
    double par[MP_MAX_NDIM];
#pragma unroll
    for (int i = 0; i < MP_MAX_NDIM; ++i) {
        const double xk = i < g.ndim ? g.pos[(size_t)k * g.ndim + i] : 0.0;
        par[i] = sub_rn(xj[i], mul_rn(sub_rn(xj[i], xk), zz));
    }
    double lnp = -INFINITY;
    int status = MP_STATUS_PRIOR, sweeps, tiles;
    if (!skip && g.target == 1) {   // isotropic unit Gaussian: exercises the move itself (tests)
        lnp = 0.0;
        status = MP_STATUS_OK;
#pragma unroll
        for (int i = 0; i < MP_MAX_NDIM; ++i) lnp = i < g.ndim ? sub_rn(lnp, mul_rn(mul_rn(0.5, par[i]), par[i])) : lnp;
    }
    // Everything of the outcome row that does not depend on the evaluation is written NOW: nothing of the draw stays live
    // across walker_eval, which needs every register (round 3 held the proposal, the partner and the thresholds in registers
    // there: 180 B of scratch per lane, 16 MB of spill traffic per launch).
    const bool lane0 = W > 1 ? threadIdx.x == 0 : (threadIdx.x & 63) == 0;   // (of the team's first wavefront)
    if (lane0) {
        double *u = g.spec + (size_t)blockIdx.x * (g.ndim + kSpecExtra);
        for (int i = 0; i < g.ndim; ++i) u[i] = par[i];
        u[g.ndim] = lnp;
        u[g.ndim + 1] = (double)status;
        u[g.ndim + 2] = mul_rn(g.ndim - 1.0, log(zz));
        u[g.ndim + 3] = logu;
        u[g.ndim + 4] = g.lnprob[k];
        u[g.ndim + 5] = (double)jc;
    }
    if (!skip && g.target != 1) {
        LaunchArgs a{};
        a.ds_id = g.ds_id;
        a.ndim = g.ndim;
        a.physical = 0;
        a.want_chi2 = 1;
        if constexpr (W > 1) walker_eval<false, SPL, LONG, false, W, OCC >= 2>(sh, a, k, par, im, tt, lds, lnp, status, sweeps, tiles, tx);
        else walker_eval<false, SPL, LONG>(sh, a, k, par, im, tt, lds, lnp, status, sweeps, tiles);
        if (lane0) {
            double *u = g.spec + (size_t)blockIdx.x * (g.ndim + kSpecExtra);
            u[g.ndim] = lnp;
            u[g.ndim + 1] = (double)status;
        }
    }
}

// The decisions of a whole step from the outcome rows of stretch_step_kernel: one thread per walker.  TEMPERED: as in
// stretch_kernel (the untempered build stays the code it was).
template <bool TEMPERED>
__global__ __launch_bounds__(256) void stretch_step_commit_kernel(const StretchArgs g) {
    const int n_slots = g.n_half * g.n_ensembles, R = g.ndim + kSpecExtra;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2 * n_slots) return;
    const int half = idx / n_slots, gs = idx - half * n_slots;
    const int w_ens = gs / g.n_half, slot = gs - w_ens * g.n_half;
    const int k = w_ens * g.n_walkers + g.perm[(size_t)w_ens * g.n_walkers + half * g.n_half + slot];
    auto accepted = [&](const double *u) {   // emcee: lnpdiff = (ndim - 1) ln z + lnprob(proposal) - lnprob(walker) > ln u
        if constexpr (TEMPERED) {            // (ndim - 1) ln z + beta lnprob(proposal) - beta lnprob(walker), beta of the ensemble
            const double beta = g.beta[w_ens];
            return sub_rn(add_rn(u[g.ndim + 2], mul_rn(beta, u[g.ndim])), mul_rn(beta, u[g.ndim + 4])) > u[g.ndim + 3];
        }
        return sub_rn(add_rn(u[g.ndim + 2], u[g.ndim]), u[g.ndim + 4]) > u[g.ndim + 3];
    };
    const double *u = g.spec + (size_t)gs * R;
    if (half == 1) {
        const double *u1 = g.spec + (size_t)(n_slots + gs) * R;
        const int gs_j = w_ens * g.n_half + (int)u1[g.ndim + 5];                  // the partner's slot in the first half
        const bool moved = accepted(g.spec + (size_t)gs_j * R);
        u = moved ? g.spec + (size_t)(2 * n_slots + gs) * R : u1;
    }
    commit_outcome(g, k, accepted(u), u, u[g.ndim], u[g.ndim + 4], (int)u[g.ndim + 1]);
}

// ---------------------------------------------------------------- parallel tempering: the swap sweep of a step
// A tempered sampler holds n_groups x n_temps ensembles; ensemble e is group e / n_temps at temperature t = e % n_temps.  After
// the decisions of a step every group runs one sweep over its neighbouring pairs, hottest first (t = n_temps - 1 .. 1), each
// pair seeing the outcome of the one before.  Slot i of temperature t - 1 pairs with slot i of temperature t, slot i of an
// ensemble being walker perm_e[i] of the step's split: the pairing is fixed before the state is looked at, so the swap, like
// the move, leaves the joint target invariant given the permutation.  Accept if ln u < (beta_{t-1} - beta_t)(L_hot - L_cold)
// (unfused; NaN and -inf reject), u from Philox keyed (seed; step, 2, cold walker, 0): half index 2 is never drawn by the move.
// An accepted swap exchanges positions and lnprob of the two walkers and rewrites their entries of the step's chain row;
// the acceptance counters stay with the walkers.
// One workgroup per group, thread i owns slot i of EVERY temperature of the group, so the chain of pairs t, t - 1 that a slot
// runs through is one thread's sequence of reads and writes: the sweep needs no barrier between the pairs.
__global__ __launch_bounds__(256) void stretch_swap_kernel(const StretchArgs g, int n_temps, unsigned long long *n_swaps) {
    const int e0 = blockIdx.x * n_temps;   // first (coldest) ensemble of this group
    for (int t = n_temps - 1; t >= 1; --t) {
        const int ec = e0 + t - 1, eh = e0 + t;
        const double dbeta = sub_rn(g.beta[ec], g.beta[eh]);
        for (int i = (int)threadIdx.x; i < g.n_walkers; i += (int)blockDim.x) {
            const int kc = ec * g.n_walkers + g.perm[(size_t)ec * g.n_walkers + i];
            const int kh = eh * g.n_walkers + g.perm[(size_t)eh * g.n_walkers + i];
            uint32_t r[4];
            philox4x32_10((uint32_t)g.seed, (uint32_t)(g.seed >> 32), (uint32_t)g.step, 2u, (uint32_t)kc, 0u, r);
            const double lc = g.lnprob[kc], lh = g.lnprob[kh];
            const bool accept = log(u01(r[0], r[1])) < mul_rn(dbeta, sub_rn(lh, lc));
            if (accept) {
                for (int d = 0; d < g.ndim; ++d) {
                    const double xc = g.pos[(size_t)kc * g.ndim + d];
                    g.pos[(size_t)kc * g.ndim + d] = g.pos[(size_t)kh * g.ndim + d];
                    g.pos[(size_t)kh * g.ndim + d] = xc;
                }
                g.lnprob[kc] = lh;
                g.lnprob[kh] = lc;
                if (g.chain) {
                    double *cc = g.chain + ((size_t)g.chain_row * g.n_total + kc) * g.ndim;
                    double *ch = g.chain + ((size_t)g.chain_row * g.n_total + kh) * g.ndim;
                    for (int d = 0; d < g.ndim; ++d) {
                        cc[d] = g.pos[(size_t)kc * g.ndim + d];
                        ch[d] = g.pos[(size_t)kh * g.ndim + d];
                    }
                    g.chain_lnp[(size_t)g.chain_row * g.n_total + kc] = lh;
                    g.chain_lnp[(size_t)g.chain_row * g.n_total + kh] = lc;
                }
            }
            // one atomic per wavefront: lane 0 holds the smallest i of its wavefront, so it is active whenever any lane is
            const unsigned long long acc_mask = __ballot(accept);
            if ((threadIdx.x & 63) == 0 && acc_mask)
                atomicAdd(n_swaps + (size_t)blockIdx.x * (n_temps - 1) + (t - 1), (unsigned long long)__popcll(acc_mask));
        }
    }
}

// ---------------------------------------------------------------- the right-hand side at arbitrary states
// One state per lane, evaluated by the device functions the solver kernels use (mdot_fb, disc_point, omega_rhs):
// dMdisc/dt = Mdotfb - Mdisc/tvisc (eta1 + eta2 = 1, code/synthetic_datasets/funcs.py:122-129) and domega/dt
// (funcs.py:119,131-140).  Serves `odes`/`ODEs` of the Python front end and pins the simplified algebra of the kernels
// against the reference's literal formulas point by point.
__global__ __launch_bounds__(64) void rhs_kernel(const DevShared sh, const RhsArgs r) {
    ktab_init();
    const int i = blockIdx.x * 64 + threadIdx.x;
    const int ii = min(i, r.n - 1);                       // idle lanes repeat the last point (wave-wide votes inside)
    double par[MP_MAX_NDIM];
#pragma unroll
    for (int k = 0; k < MP_MAX_NDIM; ++k) par[k] = k < r.ndim ? r.pars[(size_t)ii * r.ndim + k] : 0.0;
    LaunchArgs a{};
    a.ndim = r.ndim;
    a.physical = 1;
    Walker w;
    (void)walker_setup(sh, a, par, w);
    const Vd<1> tv{{r.t[ii]}}, Mv{{r.y[2 * (size_t)ii]}}, ov{{r.y[2 * (size_t)ii + 1]}};
    const Vd<1> S = mdot_fb(w, tv);
    const DiscPt<1> d = disc_point(sh, w, Mv);
    Vd<1> rot, lam;
    const Vd<1> f = omega_rhs<true, true>(sh, w, d, ov, rot, lam);
    if (i < r.n) {
        r.dydt[2 * (size_t)i] = S[0] - Mv[0] * w.inv_tau;
        r.dydt[2 * (size_t)i + 1] = f[0];
        if (r.lam) r.lam[i] = lam[0];
    }
}

int launch_rhs(const DevShared &sh, const RhsArgs &r, void *stream) {
    if (r.n <= 0) return 0;
    hipLaunchKernelGGL(rhs_kernel, dim3((unsigned)((r.n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, sh, r);
    return (int)hipGetLastError();
}

int launch_lnprob(const DevShared &sh, const LaunchArgs &a, void *stream) {
    if (a.n <= 0) return 0;
    // (the alternative dipole torque, cfg.dipole_torque = 1, lives in the curve kernels only: such a handle runs them for
    // every batch, with or without curve outputs)
    const bool curves = a.ltot || a.lprop || a.ldip || a.mdisc || a.omega || sh.cfg.dipole_torque != 0;
    dim3 grid((unsigned)a.n), block(64);
    // Variants (results agree to rounding); sh.n_simd = SIMDs of the device:
    //  - up to n_simd walkers (one wave per SIMD): four steps per lane (256-step tiles amortise the wavefront scans best;
    //    needs the whole register file of a SIMD);
    //  - beyond: two steps per lane, which keeps two waves resident per SIMD (they fill each other's issue gaps);
    //  - a handle that holds a light curve of more than 64 points runs the LONG builds of the same kernels.
    //  - curve outputs (mode B): by rounds of resident workgroups, kernel_spl_curves (mp_device.h);
    //  - diagnostics requested (a.tile_log): the LOG builds, which record the tile words.
    const bool lng = sh.has_long != 0, log = a.tile_log != nullptr || kAlwaysLog;
    hipStream_t st = (hipStream_t)stream;
    //  - launches that would leave SIMDs idle (n <= n_simd / 2): a team of four wavefronts per walker, one step per lane each
    //    (the same 256-step tiles and policy; mode A; LONG builds for handles with longer light curves).  Up to n_simd / 4 walkers every
    //    wavefront has a SIMD of its own; up to n_simd / 2 two share one and fill each other's stalls.  Measured on one box
    //    (profiles/r05_team_*.log): 256 walkers 0.0755 -> 0.0577 ms, 512 walkers 0.0767 -> 0.0699 ms near the truth
    //    (0.197 -> 0.165 ms prior-wide); a team of two (2 steps per lane) at 512 walkers 0.0701 / 0.197 ms.
    const int waves = (curves || !a.want_chi2 || a.physical) ? 1 : kernel_waves(sh, a.n);
    if (curves) {
        const bool wide = (sh.force_spl ? sh.force_spl : kernel_spl_curves(sh, a.n)) == 4;
        dispatch([&](auto wide_) { hipLaunchKernelGGL((lnprob_kernel<true, wide_ ? 4 : 2, false>), grid, block, 0, st, sh, a); }, wide);
#ifdef MP_EXPERIMENTS
    } else if (waves == 2) {   // (force_waves = 2: the two-wavefront team)
        dispatch([&](auto occ1, auto log_) {
            hipLaunchKernelGGL((lnprob_team_kernel<2, 2, occ1 ? 1 : 2, log_>), grid, dim3(128), 0, st, sh, a);
        }, 2 * a.n <= sh.n_simd, log);
#endif
    } else {   // mode A: the rule of every walker launch (walker_variant, mp_device.h)
        const Variant v = walker_variant(sh, a.n, waves == 4);
        dispatch([&](auto team, auto roomy, auto log_, auto lng_) {
            using B = Build<team, roomy>;
            if constexpr (team) hipLaunchKernelGGL((lnprob_team_kernel<B::SPL, B::W, B::OCC, log_, lng_>), grid, dim3(64 * B::W), 0, st, sh, a);
            else hipLaunchKernelGGL((lnprob_kernel<false, B::SPL, lng_, log_>), grid, block, 0, st, sh, a);
        }, v.team, v.roomy, log, lng);
    }
    return (int)hipGetLastError();
}

// The build of a stretch launch of n_blocks blocks, one rule for stretch_kernel and stretch_step_kernel (walker_variant): small
// samplers, by the size of a WHOLE step (stretch_waves), evaluate every proposal on a team of four wavefronts.
// n_blocks slots of the active half starting at g.slot_lo; the DIFF builds (DE / snooker) and the KDE builds are chosen by the
// same rule.  variant_blocks: the launch size that chooses the build -- n_blocks itself, or the 3 x slots of the whole-step launch
// whose chain this half-step launch has to reproduce bit for bit (mp_sampler_run with mp_sampler_set_whole_step(0))
int launch_stretch(const DevShared &sh, const StretchArgs &g, int n_blocks, int variant_blocks, void *stream) {
    if (n_blocks <= 0) return 0;
    const Variant v = walker_variant(sh, variant_blocks, stretch_waves(sh, 3 * g.n_half * g.n_ensembles) == 4);
    if (g.move == MP_MOVE_KDE) {
        dispatch([&](auto team, auto roomy, auto lng, auto tempered) {
            using B = Build<team, roomy>;
            hipLaunchKernelGGL((stretch_kernel<B::SPL, lng, B::W, B::OCC, tempered, false, true>), dim3((unsigned)n_blocks), dim3(64 * B::W),
                               0, (hipStream_t)stream, sh, g);
        }, v.team, v.roomy, sh.has_long != 0, g.beta != nullptr);
        return (int)hipGetLastError();
    }
    dispatch([&](auto team, auto roomy, auto lng, auto tempered, auto diff) {
        using B = Build<team, roomy>;
        hipLaunchKernelGGL((stretch_kernel<B::SPL, lng, B::W, B::OCC, tempered, diff>), dim3((unsigned)n_blocks), dim3(64 * B::W), 0,
                           (hipStream_t)stream, sh, g);
    }, v.team, v.roomy, sh.has_long != 0, g.beta != nullptr, g.move != MP_MOVE_STRETCH);
    return (int)hipGetLastError();
}

int launch_stretch_step(const DevShared &sh, const StretchArgs &g, int n_blocks, void *stream) {
    if (n_blocks <= 0) return 0;
    const Variant v = walker_variant(sh, n_blocks, stretch_waves(sh, 3 * g.n_half * g.n_ensembles) == 4);
    dispatch([&](auto team, auto roomy, auto lng) {
        using B = Build<team, roomy>;
        hipLaunchKernelGGL((stretch_step_kernel<B::SPL, lng, B::W, B::OCC>), dim3((unsigned)n_blocks), dim3(64 * B::W), 0,
                           (hipStream_t)stream, sh, g);
    }, v.team, v.roomy, sh.has_long != 0);
    return (int)hipGetLastError();
}

int launch_stretch_step_commit(const StretchArgs &g, void *stream) {
    const int n = 2 * g.n_half * g.n_ensembles;
    if (n <= 0) return 0;
    dispatch([&](auto tempered) {
        hipLaunchKernelGGL(stretch_step_commit_kernel<tempered>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g);
    }, g.beta != nullptr);
    return (int)hipGetLastError();
}

int launch_stretch_swap(const StretchArgs &g, int n_temps, int64_t *n_swaps, void *stream) {
    if (n_temps < 2 || g.n_ensembles % n_temps || !g.beta) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(stretch_swap_kernel, dim3((unsigned)(g.n_ensembles / n_temps)), dim3(256), 0, (hipStream_t)stream, g, n_temps,
                       (unsigned long long *)n_swaps);
    return (int)hipGetLastError();
}

int launch_stretch_apply(const StretchArgs &g, void *stream) {
    const int n = g.n_half * g.n_ensembles;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(stretch_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g);
    return (int)hipGetLastError();
}

}  // namespace mp

// mp_device.h — structures shared by the host sources of the C ABI (mp_host.h) and the gfx950 kernels (mp_kernels.hip).
#pragma once
#include <stdint.h>

#include <cmath>
#include <type_traits>

#include "../../include/magprop_amd.h"

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime_api.h>   // (launch_point_kernel)
#define MP_HD __host__ __device__
#else
#define MP_HD
#endif

namespace mp {

// Counter-based RNG (Philox4x32-10, Salmon et al. 2011): one independent stream per key and counter.  The kernels draw the
// moves and swaps with it, the host the random splits and the move of every step, so the chains depend on this one definition.
MP_HD inline void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

MP_HD inline double u01(uint32_t hi, uint32_t lo) {   // 53-bit uniform in [0, 1)
    return (double)((((uint64_t)hi << 32) | lo) >> 11) * (1.0 / 9007199254740992.0);
}

constexpr int kTile = 64;    // observation bucket size in grid intervals (the kernels' tiles are 64*SPL steps)
constexpr int kTile64 = 64;  // the same, for code inside the kernels where kTile names their own tile length

// physical constants, magnetar/funcs.py:7-13 (cgs)
constexpr double kG = 6.674e-8;
constexpr double kC = 3.0e10;
constexpr double kR = 1.0e6;
constexpr double kMsol = 1.99e33;

// One observed light curve, pre-digested on the host for the grid it will be interpolated on.
// Observations are sorted by time and bucketed by the 64-step tile whose light-curve values they need.
struct DsDesc {
    int32_t n_obs;
    int32_t obs_off;   // first observation in the packed obs_* arrays
    int32_t tile_off;  // first entry of this dataset's tile_ptr[n_tiles + 1]
    int32_t flags;     // bit 0: every observed time IS a grid point (x - tgrid[g] == 0 throughout: the reference's synthetic sets,
                       // code/synthetic_datasets/generate_data.py:61-67) -- np.interp then returns the model at grid point g itself and
                       // the state at g + 1 is never needed
};
constexpr int kDsOnKnots = 1;

// What a tile of the time-parallel solver needs to know about its step: tiles step over 1/8 of a grid interval (kind 0,
// the first intervals), 1, 2, 4 or 8 intervals (kinds 1 .. 4).  The grid is geometric, so the ratio Q of consecutive step
// end times, the quadrature matrices of the exponential Adams-Moulton formulas and the positions of the skipped grid
// points inside a step are constants of the kind (host-computed, oracle/mp_oracle.c mpo_eam_weights).
constexpr int kKinds = 5;
struct StrideK {
    double lnQ;          // ln of the ratio of consecutive step end times
    double inv_Q;        // 1/Q
    double one_m_invQ;   // 1 - 1/Q: step length = (step end time) * this
};

// The other constants of the kinds live in a device table (DevShared::wtab) that every workgroup copies into LDS once:
// per kind kWtabStride doubles,
//   [6 k + m]      W5[k][m], k, m = 0..4: order-5 quadrature on nodes t_{j+1} .. t_{j-3}; rows padded to 6
//   [32 + i]       theta_i, i = 1..7: time fraction of the i-th skipped grid point inside a step, (q^i - 1)/(Q - 1)
// (25 wave-uniform doubles per kind do not fit the scalar registers next to the walker constants; from LDS they are read
// where they are used, two per broadcast ds_read_b128).
constexpr int kWtabStride = 40;
constexpr int kWtabTheta = 32;
// behind the kinds' blocks: the dense-output weights of Mdisc where the step is longer than the viscous time (cubic Lagrange
// interpolation of Mdisc / (tvisc Mdotfb) through four nodes), [((kind - 2) * 7 + (i - 1)) * 12 + variant * 4 + k]:
// kinds 2 .. 4, skipped grid point i = 1 .. 7, variant = position of the step among the three intervals of its four nodes
// (0: the first, the step is the first of the tile's kept part; 1: the middle; 2: the last), k = node
constexpr int kWtabDense = kKinds * kWtabStride;
constexpr int kWtabSize = kWtabDense + 3 * 7 * 12;
constexpr int kTtabN = 257;

// Everything the kernel reads that is shared by all walkers (resident in HBM, L2-hot).
struct DevShared {
    const double *tgrid;  // [n_grid]
    int32_t n_grid;
    int32_t n_tiles;      // ceil((n_grid - 1) / 64): number of 64-step observation buckets
    const DsDesc *ds;     // [n_ds]
    int32_t n_ds;
    int32_t pad0;
    const int32_t *tile_ptr;  // per dataset: [n_tiles + 1] prefix offsets into the obs arrays (relative to obs_off)
    const int32_t *obs_g;     // grid interval index g: tgrid[g] <= x <= tgrid[g + 1]
    const double *obs_dx;     // x - tgrid[g]
    const double *obs_idt;    // 1 / (tgrid[g + 1] - tgrid[g])
    const double *obs_y;
    const double *obs_yerr;
    int32_t has_long;         // 1: some registered light curve has more than 64 points (the launchers pick the LONG kernel builds)
    int32_t pre_fine;         // grid intervals at the start that are covered with 1/8-interval sub-steps (32, or fewer on a tiny grid)
    // prior
    double lower[MP_MAX_NDIM];
    double upper[MP_MAX_NDIM];
    int32_t n_prior;
    uint32_t log_mask;
    // derived star constants (host-computed once from cfg)
    double GM, inertia, inv_inertia, crot /* 0.5*I/|W| */, sqrtGM, inv_sqrtGM, sqrtR;
    double crm_unit;      // (1e15 R^3)^(4/7) GM^(-1/7) f_Rm^(-2/7): Alfven-radius constant of a 1e15 G field
    // geometric grid t_i = t0 q^i
    double t0, lnq8;      // first grid time; ln(q)/8
    double sweep_tol;     // relative change of the step-end values that ends the Newton sweeps of a tile
    double stop_factor;   // the sweeps end when the next correction, estimated from the contraction, is below stop_factor x the tolerance
    double stride_tol;    // smoothness indicator above which a tile at a coarse stride is cut (cfg.stride_tol)
    double coarse_tol_factor;   // sweep tolerance of tiles over 2, 4 or 8 grid intervals, relative to sweep_tol
    double k4_tol_factor;       // stride_tol of tiles over 8 grid intervals, relative to stride_tol (0.1; oracle/mp_oracle.c)
    int32_t n_simd;       // SIMDs of the device (multiProcessorCount x 4): batch sizes up to this get one wave per SIMD
    int32_t force_spl;    // experiments: 0 = automatic, else steps per lane (2, 4) of the one-wavefront kernels
    int32_t force_waves;  // experiments: 0 = automatic, else wavefronts per walker (1, 2, 4)
    int32_t pad1;
    int32_t max_kind;     // coarsest tile kind allowed: 1, 2, 3, 4 for cfg.max_stride 1, 2, 4, 8
    int32_t coarse_max_sweeps, fine_max_sweeps, trouble_limit;   // sweeps after which a slowly converging tile keeps its converged lanes
    double early_hold_t;  // coarse tiles that start before this TIME (MP_EARLY_HOLD_SECONDS = 4 s: where the spin-up transients
                          // live; a physical time, so the "S" grid, whose index 1 024 is at 8 ms, gets the same protection) are
                          // held to a tenth of stride_tol, like the tile behind the sub-steps
    StrideK sk[kKinds];
    const double *wtab;   // [kWtabSize] quadrature matrices, skipped-point positions and dense-output weights of the tile kinds
    const double *ttab;   // [kKinds - 1][kTtabN] Q^k of the kinds 1 .. 4, k = 0 .. 256 (host-computed once per handle: the kernels
                          // used to spend 16 double-precision exponentials per lane on it at every launch)
    mp_model_cfg cfg;
};

// The derived star constants of DevShared from the model configuration (host; evaluator_create of mp_capi.cpp, and the probe of
// the flow kernels, which has no handle)
inline void star_constants(DevShared &s, const mp_model_cfg &cfg) {
    // star constants, magnetar/funcs.py:7-13,75-76
    const double M = 1.4 * kMsol;
    s.GM = kG * M;
    s.inertia = cfg.inertia_factor * M * kR * kR;
    s.inv_inertia = 1.0 / s.inertia;
    const double beta = s.GM / (kR * kC * kC);
    const double modW = 0.6 * M * kC * kC * (beta / (1.0 - 0.5 * beta));
    s.crot = 0.5 * s.inertia / modW;
    s.sqrtGM = std::sqrt(s.GM);
    s.inv_sqrtGM = 1.0 / s.sqrtGM;
    s.sqrtR = std::sqrt(kR);
    s.crm_unit = std::pow(1.0e15 * kR * kR * kR, 4.0 / 7.0) * std::pow(s.GM, -1.0 / 7.0) *
                 std::pow(cfg.rm_massflow_factor, -2.0 / 7.0);
}

// Per-launch arguments.
struct LaunchArgs {
    const double *pars;     // [n][ndim], device
    const int32_t *ds_id;   // [n] or nullptr
    const int32_t *order;   // [n] or nullptr: workgroup b evaluates walker order[b] (mixed-length batches: the walkers with the
                            // longest light curves first, see order_kernel); nullptr: walker b
    int32_t n;
    int32_t ndim;
    int32_t physical;       // 1: pars are physical, skip prior + un-logging (model_lc)
    int32_t want_chi2;      // 0: skip observations (model_lc only)
    double *lnprob;         // [n]
    int32_t *status;        // [n] or nullptr
    int32_t *sweeps;        // [n] or nullptr: total Newton sweeps over all tiles
    int32_t *tiles;         // [n] or nullptr: tiles solved (kept or not)
    int32_t *tile_log;      // diagnostics, or nullptr: [n][MP_TILE_LOG] one word per tile solved: kind | sweeps << 4 | kept lanes << 16
    double *ltot;           // [n][n_grid] or nullptr   (1e50 erg/s)
    double *lprop;          // [n][n_grid] or nullptr
    double *ldip;           // [n][n_grid] or nullptr
    double *mdisc;          // [n][n_grid] or nullptr
    double *omega;          // [n][n_grid] or nullptr
};

// Arguments of one fused stretch-move half-step (mp_kernels.hip: stretch_kernel).
struct StretchArgs {
    double *pos;            // [n_total][ndim] current positions, updated in place
    double *lnprob;         // [n_total]
    int64_t *n_accepted;    // [n_total]
    const int32_t *perm;    // [n_ensembles][n_walkers]: this step's random split (first n_half entries = half 0)
    const int32_t *ds_id;   // [n_total] or nullptr (dataset 0)
    double *chain;          // [n_rows][n_total][ndim] or nullptr
    double *chain_lnp;      // [n_rows][n_total]
    double *upd;            // nullptr: update in place.  Else outcome rows [slots][ndim + 3] = (proposal, lnprob, accepted,
                            // status): written by stretch_kernel (row = slot - slot_lo), read by stretch_apply_kernel (row = slot)
    double *spec;           // whole-step launches (stretch_step_kernel / stretch_step_commit_kernel): outcome rows
                            // [3][slots][ndim + kSpecExtra], see mp_kernels.hip
    double *bad_log;        // [bad_cap][ndim] or nullptr: proposals inside the prior whose model failed (the reference's fbad file)
    uint32_t *bad_count;    // number of such proposals so far (may exceed bad_cap)
    uint32_t bad_cap;
    int32_t slot_lo;        // first slot of the active half (all ensembles flattened) covered by this launch
    int32_t chain_row;
    int32_t n_walkers;      // walkers per ensemble (even)
    int32_t n_half;         // n_walkers / 2
    int32_t n_ensembles;
    int32_t n_total;        // n_walkers * n_ensembles
    int32_t ndim;
    int32_t half;           // 0 or 1: which half moves
    int32_t target;         // 0: magnetar posterior, 1: isotropic unit Gaussian (move tests)
    uint32_t step;
    uint32_t pad;
    uint64_t seed;
    double a;               // stretch scale (emcee default 2)
    uint64_t ens_order;     // half-step launches: ensemble at position p of the launch = (ens_order >> 4p) & 15; 0 = identity
    const double *beta;     // [n_ensembles] inverse temperature of every ensemble (parallel tempering), or nullptr: 1 for all.
                            // Only the decisions use it; stored log-probabilities stay untempered
    // the proposal of a half-step launch (mp_sampler_set_moves; appended so that the stretch builds read what they read before)
    int32_t move;           // MP_MOVE_STRETCH (a above), MP_MOVE_DE or MP_MOVE_SNOOKER (the DIFF builds of stretch_kernel),
                            // MP_MOVE_KDE (the KDE builds)
    uint32_t pad2;
    double de_g0;           // DE: gamma = de_g0 (1 + de_s (2u - 1)), de_s = sigma sqrt(3)
    double de_s;
    double gamma_s;         // snooker scale
    double kde_f;           // KDE: bandwidth factor f (resolved by mp_sampler_set_moves), kernel covariance f^2 S
};

// The ensemble at position e_pos of a half-step launch (StretchArgs::ens_order: longest light curve first).
MP_HD inline int ens_of_slot(const StretchArgs &g, int e_pos) {
    return g.ens_order ? (int)((g.ens_order >> (4 * e_pos)) & 15u) : e_pos;
}

// ---------------------------------------------------------------- compile-time constants of the stride policy
// (used by mp_eval.hpp; reported by mp_get_policy so that an A/B build made with -D overrides cannot pass for the shipped one)
// Tile kinds from this one on start their sweeps from the log-space extrapolation (5: none).  Tiles of 256 steps (4 steps
// per lane) over 2, 4, 8 grid intervals reach 0.6 - 1.2 decades ahead; at 128 steps (2 steps per lane) the quartic in the
// index is as good and cheaper (same-box A/B, profiles/r04_ab_predictor.log: 4 096 near-truth walkers +3 % slower with it).
#ifndef MP_LOGPRED_MIN_KIND
#define MP_LOGPRED_MIN_KIND 2
#endif
#ifndef MP_ABORT_SKIP_RATIO
#define MP_ABORT_SKIP_RATIO 32.0   // excess of the indicator over its bound beyond which a given-up coarse tile skips a stride
#endif
// A coarse tile that is cut at a fast feature of the solution (no kink) is followed by the stride its excess over the bound
// asks for, judged over this many lanes from the cut on (0: always single intervals, as until round 3)
#ifndef MP_CUT_BY_RATIO
#define MP_CUT_BY_RATIO 24
#endif
// 2-steps-per-lane kernels, adaptive stride: the sub-stepped start ends after its first tile (16 grid intervals) when that tile's
// indicator, scaled to a step of a whole interval (8^5 with the margin of 2 = 65 536) and held to a HUNDREDTH of the bound
// (MP_PRE_EARLY_END_FACTOR = 65 536 x 100; a tenth raised the soak's maximum from 5.6e-8 to 8.0e-8 for 1 % more speed:
// profiles/r04_ab_substeps_spl2.log), stays below the bound everywhere and no kink lies in it.  (Simply halving the sub-stepped stretch put one
// golden point -- a spin-up transient at t = 1 s -- at 1.01 of the tight bound in the serial restatement: tests/test_oracle.py.)
// Corrections below this (relative) let the next sweep keep the Jacobian, e^{h lambda} and the weights ("light" sweep).  1e-4
// until the tiles ended on the contraction estimate; scanned then on one box (profiles/r04_ab_light_tol.log): 3e-4 / 1e-3 / 3e-3 /
// 1e-2 speed up the passes near the truths by 0.7 / 1.3 / 1.3 / 2 %, and from 3e-3 on the slowest prior-wide walkers need
// more sweeps (chord iterations stall where the Jacobian changes from step to step): 0.228 -> 0.220 -> 0.239 ms.
#ifndef MP_LIGHT_TOL
#define MP_LIGHT_TOL 1.0e-3
#endif
#ifndef MP_PRE_EARLY_END_FACTOR
#define MP_PRE_EARLY_END_FACTOR 6553600.0
#endif
// 1 if any of the above differs from its shipped value (mp_get_policy()[MP_POLICY_EXPERIMENTS] is then set as for MP_EXPERIMENTS)
#define MP_POLICY_MACROS_MODIFIED (MP_LOGPRED_MIN_KIND != 2 || MP_ABORT_SKIP_RATIO != 32.0 || MP_CUT_BY_RATIO != 24 || MP_LIGHT_TOL != 1.0e-3 || MP_PRE_EARLY_END_FACTOR != 6553600.0)

// Steps per lane of the kernel variant used for a batch of n walkers (tiles are 64*spl steps): see launch_lnprob.
// Up to one wave per SIMD (256 CUs x 4 on MI355X) four steps per lane; beyond, two resident waves win (tools/spl_scan.sh).
inline int kernel_spl(const DevShared &sh, int n) { return n <= sh.n_simd ? 4 : 2; }
// The same for the kernels that write light curves to HBM (mode B), whose time is rounds of resident workgroups.  The
// 2-steps-per-lane build keeps 22.6 KB of LDS per workgroup: 7 workgroups per CU, not 8 -- 1 792 resident walkers on an MI355X,
// so that 2 048 walkers take TWO rounds (0.49 ms) where the 4-steps-per-lane build, one wavefront per SIMD and no scratch
// memory, takes two rounds of 1 024 in 0.34 ms.  Measured per round on one box (profiles/r05_ab_curve_spl.log): 0.171 ms
// (4 steps per lane, sharp rounds: the workgroups of a round end together) and 0.277 ms (2 steps per lane; beyond two rounds
// the workgroups overlap and the time grows linearly).  The cheaper one by that model: 2 048 walkers 4.16 -> 5.97 M
// evaluations/s, 3 072 5.45 -> 6.01 M, 4 096 5.66 -> 6.03 M, unchanged elsewhere.
inline int kernel_spl_curves(const DevShared &sh, int n) {
    if (n <= sh.n_simd) return 4;
    const double cap2 = 7.0 * (sh.n_simd / 4);                            // resident workgroups of the 2-steps-per-lane build
    const double r4 = (double)((n + sh.n_simd - 1) / sh.n_simd);          // rounds of the 4-steps-per-lane build
    const double x2 = n / cap2;
    const double r2 = 1.62 * (x2 <= 2.0 ? (x2 <= 1.0 ? 1.0 : 2.0) : x2 + 0.2);   // the other one's, in units of the former's
    return r4 <= r2 ? 4 : 2;
}
// Wavefronts per walker: launches that would leave SIMDs idle (n <= n_simd / 2) put a team of 4 wavefronts on every walker
// (mp_eval.hpp TeamX; mode A; handles with light curves of more than 64 points: the LONG builds of the same kernels); see
// launch_lnprob.  (force_waves = 2: the two-wavefront team, experiments build only.)
inline int kernel_waves(const DevShared &sh, int n) {
#ifdef MP_EXPERIMENTS
    if (sh.force_waves) return sh.force_waves;
#endif
    if (sh.force_spl) return 1;
    return 2 * n <= sh.n_simd ? 4 : 1;
}

// The same for the kernels of the device-resident sampler, by the size of a WHOLE step of the ensembles (3 x slots of a half:
// what mp_sampler_run evaluates per launch when that fits) -- for one launch per step and one per half-step alike, so that the
// two forms run the same arithmetic and their chains stay equal bit for bit; likewise every rank of a walker-sharded run.
// Team or not is all this decides.  The rest of the build (walker_variant: a team one or two wavefronts per SIMD, a single
// wavefront 4 or 2 steps per lane) goes by a block count, and the two forms launch different ones, 3 x slots and slots: for
// n_simd / 12 < slots <= n_simd / 6 and for n_simd / 3 < slots <= 19 n_simd / 24 those choose different builds, whose values
// differ (at 3 n_simd / 8 slots 557 of 768 stored lnprob differed after one step).  So mp_sampler_run hands launch_stretch the
// whole step's block count for the stretch move's half-step launches of a sampler whose whole step fits; the walker-sharded
// entry points choose by the blocks of the call (a rank's share), which is why their promise carries "while both run the same
// kernel variant".
// Ensembles of up to n_simd / 6 walkers in all (170 on an MI355X: what emcee is usually run with; the reference's own example
// has 24, code/synthetic_datasets/synth_mcmc.py): a step 0.091 -> 0.075 ms.
inline int stretch_waves(const DevShared &sh, int whole_step_blocks) {
    if (sh.force_spl) return 1;
#ifdef MP_EXPERIMENTS
    if (sh.force_waves) return sh.force_waves == 4 ? 4 : 1;
#endif
    return 2 * whole_step_blocks <= sh.n_simd ? 4 : 1;
}

// mp_sampler_run evaluates a whole step per launch (3 x slots evaluations, a third of them discarded) while that beats two
// half-step launches: up to 19/8 x n_simd evaluations (2 432 on an MI355X: ensembles of up to 1 621 walkers).  Two wavefronts per
// SIMD hold 2 x n_simd of them at once; a little beyond, the second round is still shorter than a second launch (ms per step, whole
// step / two half-steps: 1 364 walkers 0.140 / 0.191, 1 536 walkers 0.173 / 0.193, 1 700 walkers 0.201 / 0.193, 2 048 walkers
// 0.216 / 0.195; until round 5 the limit was 2 x n_simd).
inline bool stretch_whole_step_fits(const DevShared &sh, long long whole_step_blocks) { return 8 * whole_step_blocks <= 19 * (long long)sh.n_simd; }

// The build of a mode-A launch of n walker workgroups (launch_lnprob, the optimizer's trials, the nested sampler's walks, the
// stretch launches), given whether it is a team launch (kernel_waves(sh, n) == 4; stretch launches: stretch_waves of the whole
// step).  A team of 4 wavefronts per walker runs OCC = 1 wavefront per SIMD while every wavefront of the launch has a SIMD of its
// own, else 2; one wavefront per walker runs SPL = 4 steps per lane up to one wavefront per SIMD, else 2 (kernel_spl, or
// force_spl).  roomy: OCC = 1 for a team, else SPL = 4.
struct Variant {
    bool team, roomy;
};
inline Variant walker_variant(const DevShared &sh, int n, bool team) {
    if (team) return {true, 4 * n <= sh.n_simd};
    return {false, (sh.force_spl ? sh.force_spl : kernel_spl(sh, n)) == 4};
}
// the variant as the kernels' template arguments: SPL steps per lane, W wavefronts per walker, OCC wavefronts per SIMD of a team
template <bool TEAM, bool ROOMY>
struct Build {
    static constexpr int SPL = TEAM ? 1 : (ROOMY ? 4 : 2), W = TEAM ? 4 : 1, OCC = TEAM ? (ROOMY ? 1 : 2) : 0;
};

// Run-time flags to compile-time ones: dispatch(f, b0, b1, ...) calls f(std::integral_constant<bool, b0>(), ...), so that a
// launcher states its choice of kernel build once, as one template expression.  Every combination of the flags is instantiated.
template <class F>
void dispatch(F &&f) {
    f();
}
template <class F, class... B>
void dispatch(F &&f, bool b, B... rest) {
    if (b) dispatch([&](auto... c) { f(std::true_type(), c...); }, rest...);
    else dispatch([&](auto... c) { f(std::false_type(), c...); }, rest...);
}
#if defined(__HIP__) || defined(__HIPCC__)
// The launch of a resident driver's kernel (mp_point.h) on n workgroups, one evaluated point each: launch(Build<...>(), lng) is
// called with the build of launch_lnprob for a batch of n walkers -- walker_variant with a team where kernel_waves says so; lng:
// the LONG builds, for handles with light curves of more than 64 points -- and launches the kernel.  Returns hipError_t as int.
template <class F>
int launch_point_kernel(const DevShared &sh, int n, F &&launch) {
    const Variant v = walker_variant(sh, n, kernel_waves(sh, n) == 4);
    dispatch([&](auto team, auto roomy, auto lng) { launch(Build<team, roomy>(), lng); }, v.team, v.roomy, sh.has_long != 0);
    return (int)hipGetLastError();
}
#endif

// Arguments of the batched right-hand-side evaluation (mp_kernels.hip: rhs_kernel), device pointers.
struct RhsArgs {
    const double *pars;     // [n][ndim], physical units
    const double *t;        // [n]
    const double *y;        // [n][2] = (Mdisc, omega)
    double *dydt;           // [n][2]
    double *lam;            // [n] or nullptr
    int32_t n;
    int32_t ndim;
};

// implemented in mp_kernels.hip; returns hipError_t as int
int launch_rhs(const DevShared &sh, const RhsArgs &r, void *stream);
int launch_lnprob(const DevShared &sh, const LaunchArgs &a, void *stream);
int launch_order(const DevShared &sh, const int32_t *ds_id, int n, int32_t *order, void *stream);   // fills order[n] (see order_kernel)
int launch_stretch(const DevShared &sh, const StretchArgs &g, int n_blocks, int variant_blocks, void *stream);   // variant_blocks: the launch size the build is chosen by
int launch_stretch_apply(const StretchArgs &g, void *stream);
int launch_stretch_step(const DevShared &sh, const StretchArgs &g, int n_blocks, void *stream);   // blocks [g.slot_lo, + n_blocks) of 3 * n_half * n_ensembles
int launch_stretch_step_commit(const StretchArgs &g, void *stream);
// the swap sweep of a tempered step (stretch_swap_kernel): one workgroup per group of n_temps ensembles; n_swaps[group][n_temps - 1]
int launch_stretch_swap(const StretchArgs &g, int n_temps, int64_t *n_swaps, void *stream);
// columns behind the proposal in an outcome row of a whole-step launch
constexpr int kSpecExtra = 6;   // lnprob, status, (ndim - 1) ln z, ln u, lnprob of the walker before the move, partner's slot

// Arguments of one generation of the differential-evolution optimizer (mp_opt.hip; include/magprop_amd.h mp_optimizer_*).
// Member k = p * popsize + i is member i of population p; the population is double-buffered (cur -> next): a trial launch reads
// only the cur buffers and writes only the next ones, so no workgroup reads what another one writes.  (The reduction writes the
// cur buffers of a population that has just converged: both buffers then hold its final state.)
struct OptArgs {
    double *pop_cur;         // [n_total][ndim]
    double *pop_next;
    double *lnp_cur;         // [n_total]
    double *lnp_next;
    int32_t *st_cur;         // [n_total] status of every member (MP_STATUS_*)
    int32_t *st_next;
    const int32_t *ds_id;    // [n_total] dataset of every member
    int32_t *best;           // [n_pops] best member of the last generation (index inside the population)
    int32_t *converged;      // [n_pops] 1: frozen
    int32_t *nit;            // [n_pops] generations run (scipy's nit)
    int64_t *nfev;           // [n_pops] evaluations
    double lower[MP_MAX_NDIM], upper[MP_MAX_NDIM];   // the bounds box (sampler coordinates)
    int32_t popsize, n_pops, ndim, strategy;         // strategy: MP_DE_BEST1BIN or MP_DE_RAND1BIN
    int32_t target;          // 0: posterior, 1: isotropic unit Gaussian
    int32_t trial;           // 0: evaluate pop_cur as it is (generation 0), 1: a generation of trials
    uint32_t gen;            // generation number (the Philox counter); 0 = the initial evaluation
    uint32_t pad;
    uint64_t seed;
    double f_lo, f_hi, cr, tol, atol;
};
// one workgroup per member (trial = 0 or 1), then one per population (best member, stop rule, counters); include/magprop_amd.h
int launch_opt_trial(const DevShared &sh, const OptArgs &o, void *stream);
int launch_opt_reduce(const OptArgs &o, void *stream);

// Arguments of one iteration of the nested sampler (mp_nest.hip; include/magprop_amd.h mp_nested_*).  Live slot j of run r is
// row r * nlive + j.  The select launch ranks the live set and writes this iteration's dead list, survivor list and L*; the walk
// launch reads only survivors (and those lists) and writes only dead slots, so no workgroup reads what another one writes.
struct NestArgs {
    double *live;            // [n_runs * nlive][ndim]
    double *lnl;             // [n_runs * nlive] (NaN stored as -inf)
    int32_t *st;             // [n_runs * nlive] status of every live point (MP_STATUS_*)
    int32_t *acc;            // [n_runs * nlive] accepted steps of the walk that put the point there (0: set by the caller)
    const int32_t *ds_id;    // [n_runs] dataset of every run
    int32_t *dead_slot;      // [n_runs][nbatch] this iteration's dead slots, ascending lnL
    int32_t *surv;           // [n_runs][nlive - nbatch] this iteration's survivors in slot order
    double *lstar;           // [n_runs] this iteration's L* (largest dead lnL)
    double *dead_pars;       // [chunk][n_runs][nbatch][ndim] the dead rows of the chunk's iterations
    double *dead_lnl;        // [chunk][n_runs][nbatch]
    int32_t *dead_n;         // [chunk][n_runs][nbatch] live count n_i of every dead point
    double *lnx;             // [n_runs] ln X after the run's last iteration
    double *lnz;             // [n_runs] running ln Z
    int32_t *stopped;        // [n_runs] 1: frozen
    int32_t *nit;            // [n_runs] iterations run
    int64_t *ncall;          // [n_runs] evaluations inside walks
    int64_t *nacc;           // [n_runs] accepted walk steps
    int64_t *nzero;          // [n_runs] walks that accepted nothing
    double lower[MP_MAX_NDIM], upper[MP_MAX_NDIM];   // the prior box (sampler coordinates)
    int32_t nlive, nbatch, n_runs, ndim;
    int32_t walks;           // steps per walk
    int32_t target;          // 0: posterior, 1: isotropic unit Gaussian
    int32_t mode;            // select: 0 iteration, 1 stop check only; walk: 0 iteration, 1 evaluate the live set as it is
    int32_t slot;            // chunk slot of this iteration's dead rows
    uint32_t iter;           // iteration number (the Philox counter)
    uint32_t pad;
    uint64_t seed;
    double g0, sig3, dlogz;  // sig3 = sigma sqrt(3)
};
// one workgroup per run (rank, dead rows, L*, survivors, ln X, ln Z, stop rule), then one per dead slot (the constrained walk;
// mode 1: one per live point, evaluated as it is); include/magprop_amd.h
int launch_nest_select(const NestArgs &a, void *stream);
int launch_nest_walk(const DevShared &sh, const NestArgs &a, void *stream);
// Slice mode of the nested sampler (mp_nested_set_slice): the walk into a dead slot is `slices` slice updates along survivor
// differences (include/magprop_amd.h states the scheme).  Passed beside NestArgs, which the random walk's kernels keep as it is.
struct NestSlice {
    int64_t *nexpand;        // [n_runs] stepping-out steps that widened an interval
    int64_t *ncontract;      // [n_runs] shrink points that were rejected
    int64_t *nfail;          // [n_runs] slices that ended where they started (shrink cap, or a zero direction)
    double mu;               // initial interval width, in units of the direction
    int32_t slices;          // slice updates per walk (0: the random walk)
    int32_t max_steps_out;   // Neal's stepping-out budget m
    int32_t max_shrink;      // shrink points per slice before it counts as failed
    int32_t pad;
};
// one workgroup per dead slot (mode 0 only), the builds of launch_nest_walk
int launch_nest_slice(const DevShared &sh, const NestArgs &a, const NestSlice &sl, void *stream);

}  // namespace mp

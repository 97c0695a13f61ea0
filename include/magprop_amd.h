/*
 * magprop_amd.h — C ABI of the MI355X-native magnetar log-posterior hot path.
 *
 * This is the drop-in boundary for the ONE data-parallel path of sgibson91/magprop
 * that this project accelerates: for each of N walkers, lnprior + integrate the
 * (Mdisc, omega) ODEs over the 10 001-point log grid + luminosity light curve +
 * linear interpolation at the observed times + -0.5*chi^2.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   - lnprob(pars, x, y, yerr, fbad)            code/synthetic_datasets/mcmc_eqns.py:52-81
 *   - lnlike(pars, x, y, yerr)                  code/synthetic_datasets/mcmc_eqns.py:5-25
 *   - lnprior(pars)                             code/synthetic_datasets/mcmc_eqns.py:28-49
 *   - model_lum(pars, xdata=None, n, alpha, cs7, k, dipeff, propeff, f_beam)
 *                                               code/synthetic_datasets/funcs.py:146-236
 *   - lnprob(pars, data, GRBtype, custom_lims)  magnetar/mcmc_eqns.py:87-119
 *   - lnlike(pars, data, GRBtype)               magnetar/mcmc_eqns.py:6-37
 *   - lnprior(pars, custom_lims)                magnetar/mcmc_eqns.py:40-84
 *   - model_lc(pars, xdata, GRBtype, ...)       magnetar/funcs.py:105-220
 *   - init_conds / odes / ODEs                  magnetar/funcs.py:17-101,
 *                                               code/synthetic_datasets/funcs.py:51-142
 * The reference is pure Python; its "FFI" for this path is the emcee log_prob_fn
 * callable (code/synthetic_datasets/synth_mcmc.py:180-185).  The ctypes binding a
 * maintainer would add is shown in INTEGRATION.md and shipped in
 * magprop_amd/_capi.py.
 *
 * Conventions
 *   - plain C, no torch / C++ types in any signature; caller owns every buffer.
 *   - every function returning int returns MP_OK (0) or a negative MP_E* code and
 *     records a message retrievable with mp_last_error() (thread-local).
 *   - per-walker physics failures are NOT errors: lnprob = -inf and a status code
 *     (reference: the string 'flag', magnetar/funcs.py:153-154).
 *   - all floating point is IEEE fp64.
 *
 * Threads and streams
 *   - A handle (and the samplers created on it) may be used from several host threads: every entry point
 *     that takes one serialises on a mutex inside the handle for the duration of the call.  The host-buffer
 *     entry points (mp_lnprob_batch, mp_model_lc, mp_rhs_batch, mp_sampler_run ...) run on the handle's own
 *     stream and return when their results are in the caller's buffers.
 *   - mp_lnprob_batch_dev and the mp_sampler_halfstep_* / mp_sampler_step_* calls only enqueue work on the stream
 *     they are given.  Launches of one handle on different streams may overlap on the device: a launch writes nothing
 *     but its own outputs (since ABI 4 also for handles that hold light curves of more than 64 points, which until
 *     ABI 3 owned per-walker scratch rows and were ordered by the library).  A batch that mixes light curves of more
 *     than 64 points with short ones and exceeds two wavefronts per SIMD is launched longest light curves first
 *     (results do not depend on it); its index buffer comes from a ring of eight per handle, so of such launches only
 *     those eight apart are ordered (by an event, on the device).
 *   - Buffers passed to an asynchronous call must stay valid until the work has completed on that stream;
 *     replacing a dataset (mp_set_dataset) waits for the device first.
 *   - All mp_sampler_halfstep_* calls of one sampler must use one stream.
 */
#ifndef MAGPROP_AMD_H
#define MAGPROP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MP_ABI_VERSION 5

/* return codes */
#define MP_OK 0
#define MP_EINVAL (-1)  /* bad argument (NULL, size, ds_id, ndim ...)            */
#define MP_EHIP (-2)    /* a HIP runtime call failed; see mp_last_error()         */
#define MP_ERANGE (-3)  /* observed time outside the model grid (interp1d raises  */
                        /* ValueError there: magnetar/funcs.py:214-215)           */
#define MP_ENODEV (-4)  /* no usable gfx950 device                                */
#define MP_ESTATE (-5)  /* call order problem (dataset / prior not set)           */

/* per-walker status (reference: success / 'flag' string / non-finite lnlike) */
#define MP_STATUS_OK 0
#define MP_STATUS_FLAG 1      /* break-up limit reached: the reference's LSODA 'flag'   */
#define MP_STATUS_NONFINITE 2 /* state or chi^2 went non-finite                         */
#define MP_STATUS_PRIOR 3     /* outside the prior box, model never evaluated           */
#define MP_STATUS_BADDATASET 4 /* ds_id names no registered light curve (out of range or never set): lnprob = -inf.  The   */
                              /* host-buffer entry rejects such a batch with MP_EINVAL; the device-pointer entries cannot */
                              /* read the ids and report it per walker instead                                            */
#define MP_STATUS_ZEROERR 5   /* mp_simulate only: a simulated observation of the row has error 0 (a model value of 0)   */

/* limits */
#define MP_MAX_NDIM 9        /* 6 physics parameters + up to dipeff, propeff, f_beam */
#define MP_MAX_DATASETS 64

/*
 * The two physics variants of the reference are data, not code forks
 * (SURVEY.md section 2.1).  mp_cfg_synth()/mp_cfg_lib() fill the two presets.
 */
typedef struct mp_model_cfg {
    double inertia_factor;     /* I = f*M*R^2 : 0.8 (magnetar/funcs.py:12) | 0.35 (code/synthetic_datasets/funcs.py:17) */
    double rm_massflow_factor; /* Rm ~ (f*Mdisc/tvisc)^(-2/7): 1 (magnetar/funcs.py:64) | 3 (synth funcs.py:105)        */
    double n_ode;              /* propeller switch-on inside the ODE right-hand side                                    */
    double n_lum;              /* propeller switch-on in the luminosity stage                                           */
    double alpha;              /* sound-speed prescription                                                              */
    double cs7;                /* sound speed, 1e7 cm/s                                                                 */
    double k;                  /* light-cylinder capping fraction                                                       */
    double dipeff;             /* default dipole efficiency   (overridden per walker when ndim is 8 or 9)               */
    double propeff;            /* default propeller efficiency (overridden per walker when ndim is 8 or 9)              */
    double f_beam;             /* default beaming fraction     (overridden per walker when ndim is 7 or 9)              */
    double nacc_lum_threshold; /* luminosity-stage break-up test: 0.27 (synth funcs.py:206) | 0.0 (magnetar/funcs.py:193) */
    int32_t lprop_gm_term;     /* 1: Lprop includes -(GM/Rm)*eta2*Mdisc/tvisc (synth funcs.py:222-223); 0: lib          */
    int32_t max_stride;        /* grid intervals a step of the solver may span: 0 = MP_MAX_STRIDE_DEFAULT (8), or 1, 2, 4, 8. */
                               /* 1 = every grid interval is a step (the serial restatement oracle/mp_oracle.c mode 0)       */
    double sweep_tol;          /* relative change of omega at the step ends that ends the Newton sweeps of a tile of the   */
                               /* time-parallel solver; 0 = MP_SWEEP_TOL_DEFAULT.  What it buys and costs: DESIGN.md 3     */
    double stride_tol;         /* smoothness indicator h |4th difference of (f - lambda omega)| / omega above which a tile   */
                               /* stepping over 2, 4 or 8 grid intervals is cut back to single intervals; 0 =                */
                               /* MP_STRIDE_TOL_DEFAULT                                                                      */
    int32_t dipole_torque;     /* ABI 5.  0: Ndip = -mu^2 omega^3 / (6 c^3), every model of the reference's packages          */
                               /* (magnetar/funcs.py:78; "Piro & Ott" in code/figure_3.py:79).  1: the alternative torque law */
                               /* of code/figure_3.py:105-165 ("Bucciantini"): Ndip = -(2/3) (mu^2 omega^3 / c^3) (Rlc/Rm)^3  */
                               /* with Rm after the light-cylinder cap.  It changes the ODE's torque only, as in that script  */
                               /* (which integrates and plots radii and torques, no luminosity).  Served by the curve kernels */
                               /* (mp_model_lc, mp_rhs_batch, mp_lnprob_batch); the device-resident sampler refuses it        */
    int32_t reserved;          /* 0                                                                                           */
} mp_model_cfg;

/* Stride adaptivity of the solver: where the solution is smooth on the scale of the output grid the
 * order-5 formula steps over 2, 4 or 8 grid intervals at once and the states at the skipped grid points come from the
 * step's dense output (<= 4e-10 relative); tiles that contain a kink of the right-hand side (Alfven-radius cap, torque
 * arm) or a fast transient are cut there and continued finer.  Measured on the 6 256 golden prior-wide points: same
 * maximum deviation from the reference's tight-integrator values as with max_stride = 1 (5e-8), 13.6 instead of 40 tiles
 * per walker (9 near the truths). */
#define MP_MAX_STRIDE_DEFAULT 8
#define MP_STRIDE_TOL_DEFAULT 1.0e-7
/* Coarse tiles that START before this time (seconds; the spin-up transients of heavy discs around strongly magnetised
 * stars live here) are held to a tenth of stride_tol.  A physical time, not a grid index: the reference's "L" grid
 * reaches it at index 1 003, its "S" grid (t0 = 1 ms) at index 4 003. */
#define MP_EARLY_HOLD_SECONDS 4.0

/* The sweeps contract by 1e-2..1e-3 per pass, so a tile whose last correction was <= 1e-7 relative is converged to
 * <= 4.5e-9 relative in lnprob (measured over the golden clouds and the prior-wide scans, tools/tol_scan.py) — 10x below
 * the 6e-8 by which the scheme itself differs from the reference integrated at rtol = atol = 1e-12, and 3000x below the
 * reference's own LSODA noise (1.4e-5).  The sweeps of a tile also end when every lane's correction fell at least tenfold
 * from the previous sweep and the next one -- estimated linearly from that factor -- would be below MP_STOP_FACTOR (a hundredth) of the
 * tolerance: the verification pass of a fast-converging tile is not run (round 4; near the truths 4 of a walker's 25
 * sweeps), and what is left is <= 0.01 x sweep_tol per tile.  MP_SWEEP_TOL_STRICT (1e-11) is what the tests use when they
 * compare kernel variants with each other and with the serial restatement of the scheme. */
#define MP_SWEEP_TOL_DEFAULT 1.0e-7
#define MP_SWEEP_TOL_STRICT 1.0e-11
#define MP_STOP_FACTOR 0.01

typedef struct mp_handle mp_handle;

int mp_abi_version(void);
const char *mp_last_error(void);

void mp_cfg_synth(mp_model_cfg *cfg); /* code/synthetic_datasets/funcs.py:146-147 defaults */
void mp_cfg_lib(mp_model_cfg *cfg);   /* magnetar/funcs.py:105-106 defaults; ODE always n=1 (funcs.py:150-151) */

/*
 * Create an evaluator bound to HIP device `device` (-1: the calling thread's current
 * device).  `tgrid` (host pointer, n_grid >= 2 strictly increasing doubles) is the
 * output/integration grid: np.logspace(0,6,10001) or np.logspace(-3,6,10001)
 * (magnetar/funcs.py:132-137).  The grid is copied to the device.
 */
mp_handle *mp_create(const mp_model_cfg *cfg, const double *tgrid, int n_grid, int device);
int mp_destroy(mp_handle *h);

/*
 * The same evaluator over SEVERAL devices of the node in ONE process (SURVEY.md 8(b)'s `device_mask`; ABI 5): what a
 * plain, single-process emcee user of `EnsembleSampler(..., vectorize=True)` needs to use more than one GPU -- the
 * reference's counterpart is `Pool()` over walkers, code/synthetic_datasets/synth_mcmc.py:178-185.  devices[n_devices]
 * lists HIP device indices (a device may be listed more than once: its share of every batch grows accordingly).
 * mp_set_dataset / mp_set_prior reach every device; mp_lnprob_batch (host buffers) deals the rows out in contiguous blocks
 * of ceil(n / n_devices) -- the partitioning of SURVEY.md 8(e) -- enqueues every device's kernel before it waits for the
 * first, and returns one vector: no torch, no RCCL, no second process.  mp_model_lc / mp_rhs_batch run on the first
 * device.  The device-pointer entry (mp_lnprob_batch_dev) and the device-resident sampler belong to one device and
 * return MP_ESTATE on such a handle; walker-sharded SAMPLING across devices is magprop_amd/distributed.py (one process per
 * GPU, RCCL).  Not measured on several GPUs by the builder (one-GPU boxes): tested with the same device listed twice.
 */
mp_handle *mp_create_multi(const mp_model_cfg *cfg, const double *tgrid, int n_grid, const int *devices, int n_devices);
int mp_n_devices(const mp_handle *h);   /* 1 for mp_create's handles */

/*
 * Register (or replace) observed light curve `ds_id` (0 <= ds_id < MP_MAX_DATASETS):
 * x = times [s], y = luminosity [1e50 erg/s], yerr = 1-sigma errors; host pointers.
 * Returns MP_ERANGE if any x lies outside [tgrid[0], tgrid[n_grid-1]].
 * Registering a NEW slot appends to the device-resident arrays (only the new light curve is uploaded, nothing waits
 * for the device unless the arrays have to grow); REPLACING a slot waits for the device first.
 */
int mp_set_dataset(mp_handle *h, int ds_id, const double *x, const double *y, const double *yerr, int n_obs);

/*
 * Box prior (inclusive), lower/upper[ndim].  Bit i of log_mask set: sampler
 * coordinate i is log10 of the physical parameter and is un-logged before the
 * model is evaluated (code/synthetic_datasets/mcmc_eqns.py:16-17).  ndim = 0
 * disables the prior (lnlike only; pars then taken as given, un-logged per log_mask).
 */
int mp_set_prior(mp_handle *h, const double *lower, const double *upper, int ndim, uint32_t log_mask);

/*
 * Batched log-posterior, host buffers.  pars[n][ndim] row-major (ndim 6..9:
 * B, P, MdiscI, RdiscI, epsilon, delta [, f_beam | dipeff, propeff [, f_beam]],
 * magnetar/mcmc_eqns.py:22-34).  ds_id[n] selects the dataset per walker (NULL:
 * dataset 0).  lnprob_out[n] required; status_out[n] and ltot_out[n][n_grid]
 * (model light curve in 1e50 erg/s on the grid) optional (NULL).
 */
int mp_lnprob_batch(mp_handle *h, const double *pars, const int32_t *ds_id, int n, int ndim,
                    double *lnprob_out, int32_t *status_out, double *ltot_out);

/*
 * Same, every pointer a DEVICE pointer on the handle's device; the kernel is
 * enqueued on `stream` (a hipStream_t passed as void*; NULL is HIP's default
 * stream, mp_stream(h) the handle's own) and the call returns without
 * synchronising.  Rows of d_ltot whose walker did not finish (status != MP_STATUS_OK)
 * are filled with NaN by the kernel, as in the host-buffer form.
 */
int mp_lnprob_batch_dev(mp_handle *h, const double *d_pars, const int32_t *d_ds_id, int n, int ndim,
                        double *d_lnprob, int32_t *d_status, double *d_ltot, void *stream);

/*
 * Full model light curve for one parameter vector in PHYSICAL units (no prior,
 * no un-logging): out[4][n_grid] = tarr, Ltot, Lprop, Ldip (luminosities in
 * 1e50 erg/s) as returned by model_lc/model_lum with xdata=None
 * (magnetar/funcs.py:219-220).  traj (optional) receives [2][n_grid] = Mdisc, omega.
 */
int mp_model_lc(mp_handle *h, const double *pars, int ndim, double *out, double *traj, int32_t *status);

/*
 * The ODE right-hand side itself, batched: replaces calls of `odes(y, t, B, MdiscI, RdiscI, epsilon, delta, ...)`
 * (magnetar/funcs.py:33-101) / `ODEs(...)` (code/synthetic_datasets/funcs.py:75-142).  For point i:
 * pars[i][ndim] PHYSICAL parameters (B, P, MdiscI, RdiscI, epsilon, delta[, ...]; P is not used by the RHS),
 * t[i], y[i] = (Mdisc [g], omega [rad/s])  ->  dydt[i] = (dMdisc/dt, domega/dt).  lam (optional, [n]) receives
 * d(omega_dot)/d(omega), the Jacobian entry the time-parallel solver linearises with.  Host buffers; evaluated by
 * the same device functions as the log-posterior kernels (one point per lane).
 */
int mp_rhs_batch(mp_handle *h, const double *pars, int ndim, const double *t, const double *y, int n, double *dydt,
                 double *lam);

/*
 * Posterior-predictive band of the model light curves (ABI 5, additive): per grid point the quantiles q[nq] of the curves
 * of n parameter rows, computed on the device.  The reference's post-processing takes percentiles of the PARAMETERS and
 * draws one curve at their medians (code/synthetic_datasets/plot_synth.py:143-206); this is the band over the samples.
 *   pars[n][ndim]  host rows; physical = 0: sampler coordinates, prior and log_mask of mp_set_prior applied exactly as in
 *                  mp_lnprob_batch (ndim = 0 there: no prior); physical = 1: physical parameters taken as given (mp_model_lc)
 *   q[nq]          each finite and in [0, 1], any order; 1 <= nq <= MP_BAND_MAX_Q
 *   components     non-empty mask of MP_BAND_LTOT | MP_BAND_LPROP | MP_BAND_LDIP
 *   band_out       [k][nq][n_grid]: k over the set component bits in ascending order, j over q in the caller's order
 *   status_out[n]  (optional) what mp_lnprob_batch reports for these rows; *n_used (optional) the rows with MP_STATUS_OK
 * Per grid point the result is np.nanquantile(curves, q, axis=0) (method "linear") bit for bit, where rows that did not
 * finish are NaN; no row finished: all NaN and MP_OK.  The curves come from ONE launch of the curve kernels (the build
 * kernel_spl_curves(n) names, as mp_lnprob_batch(..., ltot_out) runs for the same n rows), without a dataset.  Host
 * buffers; returns when the results are in them.  A multi-device handle runs the call on its first device.
 * Workspace: up to n * n_grid * (components + 1) doubles on the device (5.2 GB at the cap with all three components),
 * owned by the handle, grow-only, freed by mp_destroy.
 */
#define MP_BAND_MAX_SAMPLES 16384
#define MP_BAND_MAX_Q 16
#define MP_BAND_LTOT 1u
#define MP_BAND_LPROP 2u
#define MP_BAND_LDIP 4u
int mp_model_band(mp_handle *h, const double *pars, int n, int ndim, int physical, const double *q, int nq, uint32_t components,
                  double *band_out, int32_t *status_out, int32_t *n_used);

/*
 * The band of WEIGHTED samples (ABI 5, additive): per grid point the quantiles q[nq] of the weighted empirical distribution of
 * the curves of n parameter rows under weights[n] -- the dead and live points of a nested run with exp(logwt), or a chain
 * reweighted to another prior, error model or temperature -- computed on the device, without resampling.  Every argument but
 * weights is mp_model_band's, and so are the curve pass (one launch of all n rows, the build kernel_spl_curves(n) names), the
 * limits, the component order, status_out, *n_used and the workspace (plus n uint32 on the device).
 *
 * Definition.  A floating-point sum of weights depends on its order and a band must not, so the weights become integers once
 * and every sum after that is exact.
 *   units      wmax = the largest weight; u_i = (uint32) floor((w_i / wmax) * 2147483648.0).  The division rounds once, the
 *              product with 2^31 and the floor are exact.  The heaviest row has exactly 2^31 units; a row below 2^-31 of it has
 *              none and drops out.  The weights have to be finite and >= 0 with at least one > 0: MP_EINVAL otherwise, judged
 *              before a handle is needed.  mp_band_weight_units is this conversion alone (host only, no handle).
 *   per grid point   the used values are the column's non-NaN ones (a row that did not finish is NaN everywhere).  W = the sum
 *              of their units (below 2^46 at n <= MP_BAND_MAX_SAMPLES, so exact in a double); W == 0: NaN.  Target
 *              T = ceil(q * (double)W), the product rounded once, clamped to [1, W].  The answer is the least used value v whose
 *              cumulative units over the used values <= v reach T.  Values are ordered as mp_model_band orders them, -0.0 below
 *              +0.0.  No interpolation: this is the weighted empirical distribution function, the rule of numpy's
 *              method="inverted_cdf" (equal weights give np.nanquantile(curves, q, axis=0, method="inverted_cdf")).  q = 0
 *              answers the least value that carries weight, q = 1 the largest.
 * No floating-point atomic and no floating-point sum anywhere: the result is a function of the rows and their weights, bit for
 * bit, in whatever order they come.  No row finished, or no weight on those that did: all NaN and MP_OK.  (tests/wband_restated.py
 * is this definition in numpy.)
 */
int mp_band_weight_units(const double *weights, int n, uint32_t *units_out);
int mp_model_band_weighted(mp_handle *h, const double *pars, int n, int ndim, int physical, const double *weights, const double *q,
                           int nq, uint32_t components, double *band_out, int32_t *status_out, int32_t *n_used);

/*
 * Energy budgets and light-curve landmarks of the model of n parameter rows, computed on the device (ABI 5, additive): the
 * physical quantities a fit implies, which are functions of a sample's whole curves and trajectory (how much energy it
 * radiates and through which channel, when and how high it peaks, by when half of the energy is out, how far accretion spins
 * the star up).  pars, ndim and physical are mp_model_band's; out[n][MP_DERIVED_N], status_out[n] (optional) and *n_used
 * (optional: the rows with MP_STATUS_OK) are host buffers, and the call returns when the results are in them.  A row whose
 * status is not MP_STATUS_OK gets MP_DERIVED_N NaNs; no row finished: all NaN and MP_OK.  No dataset is needed.  A
 * multi-device handle runs the call on its first device.
 *
 * n has no cap: the rows go through the device in chunks of mp_n_simd(h) rows (1 024 on an MI355X), each one launch of the
 * curve kernels with all five curves (the 4-steps-per-lane build, the one mp_model_lc runs for a single row), one reduction
 * launch and one copy, all on the handle's stream with one wait at the end.  A row's columns are therefore bit for bit the
 * definition below applied to what mp_model_lc returns for that row alone, whatever n is and wherever the row sits.
 * Workspace: 5 * min(n, mp_n_simd) * n_grid doubles (410 MB), owned by the handle, grow-only, freed by mp_destroy.
 *
 * Columns.  G = n_grid, t_i the grid, dt_i = t_{i+1} - t_i, luminosities in 1e50 erg/s as mp_model_lc returns them:
 *   E_TOT, E_PROP, E_DIP   trapezoid of Ltot, Lprop, Ldip over the grid (1e50 erg): the sum of 0.5 * dt_i * (L_i + L_{i+1}),
 *                          formed as (0.5 * dt_i) * (L_i + L_{i+1}) with every difference, product and sum rounded on its own
 *   L_PEAK, T_PEAK         the largest Ltot and its grid time (the first one of equal values); LPROP_PEAK, T_LPROP_PEAK: of Lprop
 *   T10, T50, T90          the first grid time t_{i+1} at which the cumulative trapezoid of Ltot up to t_{i+1} is >= f * E_TOT,
 *                          f = 0.1, 0.5, 0.9 (the product rounded once); E_TOT == 0: t_1; never reached (a negative total):
 *                          t_{G-1}
 *   OMEGA_END              omega at the last grid point (rad/s); OMEGA_MAX, T_OMEGA_MAX its largest value and that value's
 *                          time, first occurrence (the accretion spin-up)
 *   MDISC_END, MDISC_MAX, T_MDISC_MAX   the same of the disc mass (g)
 * Order of the sums (a function of the row's curves and G only): the G - 1 intervals are cut into 256 contiguous segments of
 * ceil((G - 1) / 256) intervals (the last ones may be short or empty); inside a segment the terms are added in increasing i
 * from 0.0; the 256 segment totals are added in segment order from 0.0 (an empty segment adds 0.0); the cumulative energy up
 * to t_{i+1} is the total of the segments before i's plus the running sum of its segment.  No FMA contraction and no
 * floating-point atomic anywhere.  (tests/derive_restated.py is this definition in numpy.)
 */
#define MP_DERIVED_N 16
#define MP_DERIVED_E_TOT 0
#define MP_DERIVED_E_PROP 1
#define MP_DERIVED_E_DIP 2
#define MP_DERIVED_L_PEAK 3
#define MP_DERIVED_T_PEAK 4
#define MP_DERIVED_LPROP_PEAK 5
#define MP_DERIVED_T_LPROP_PEAK 6
#define MP_DERIVED_T10 7
#define MP_DERIVED_T50 8
#define MP_DERIVED_T90 9
#define MP_DERIVED_OMEGA_END 10
#define MP_DERIVED_OMEGA_MAX 11
#define MP_DERIVED_T_OMEGA_MAX 12
#define MP_DERIVED_MDISC_END 13
#define MP_DERIVED_MDISC_MAX 14
#define MP_DERIVED_T_MDISC_MAX 15
int mp_model_derived(mp_handle *h, const double *pars, int64_t n, int ndim, int physical, double *out, int32_t *status_out,
                     int64_t *n_used);

/*
 * Pointwise predictive scores of a fit, computed on the device (ABI 5, additive): per observation of dataset ds_id, the
 * reductions over the n samples' pointwise log-likelihoods from which WAIC, importance-sampling and Pareto-smoothed
 * leave-one-out (PSIS-LOO) scores and their Pareto-k diagnostics follow on the host (magprop_amd/pointwise.py), without the
 * n x n_obs matrix ever leaving the device.  pars, n, ndim and physical are mp_model_derived's; the dataset has to be set (as in
 * mp_lnprob_batch: MP_ESTATE otherwise).  Observations are in the order mp_set_dataset keeps them: ascending time (stable).
 *   obs_out[n_obs][MP_POINTWISE_N]              the columns below
 *   tail_out[n_obs][mp_pointwise_tail_len(n)]   (optional) the min(T, N_USED) largest r of the observation, ascending, then NaN
 *   z_out[n_obs][n]                             (optional) the cell matrix itself, for small calls and tests
 *   status_out[n], *n_used                      (optional) as in mp_model_derived
 * Limits: 1 <= n <= MP_POINTWISE_MAX_SAMPLES and n * n_obs <= MP_POINTWISE_MAX_CELLS.  The rows go through the device in chunks
 * of mp_n_simd(h) rows, each one launch of the curve kernels (Ltot only, the build mp_model_lc runs for a single row) and one
 * launch that turns the chunk's curves into cells; two reduction launches per call follow.  Workspace, owned by the handle,
 * grow-only, freed by mp_destroy: n * n_obs + min(n, mp_n_simd) * n_grid doubles.  A multi-device handle runs the call on its
 * first device.
 *
 * Cell of sample s (status MP_STATUS_OK) and observation j, with La, Lb the sample's Ltot (1e50 erg/s, as mp_model_lc returns
 * it) at grid points g_j and g_j + 1, t[g_j] <= x_j < t[g_j + 1] (the last point: the last interval), dx_j = x_j - t[g_j],
 * idt_j = 1 / (t[g_j + 1] - t[g_j]):
 *   mod = ((Lb - La) * idt_j) * dx_j + La,   z = (y_j - mod) / yerr_j,   r = 0.5 * (z * z),   ll = -r
 * every operation rounded on its own (no FMA contraction).  ll is the term of the unnormalised lnlike = -0.5 chi^2 the library
 * samples; -0.5 ln(2 pi yerr_j^2) per point normalises it.  A sample whose status is not OK has NaN cells; the used cells of an
 * observation are its non-NaN ones, N_USED of them.  T = mp_pointwise_tail_len(N_USED) = M + 1, M = ceil(min(N_USED / 5,
 * 3 sqrt(N_USED))) the length of the Pareto tail of PSIS, computed in integers.  Columns, over the used cells:
 *   N_USED                   their number
 *   Z_MEAN, R_MEAN           means of z and of r (sum / N_USED; NaN for N_USED = 0)
 *   LL_VAR                   variance of ll, two passes: the mean -R_MEAN, then the sum of squared deviations / (N_USED - 1); NaN
 *                            for N_USED < 2
 *   R_MIN, R_MAX             least and largest r (NaN for N_USED = 0)
 *   LPPD_M, LPPD_S           running log-sum-exp pair of ll: sum exp(ll) = e^M S, M the largest ll ((-inf, 0): none)
 *   CUT                      the min(T, N_USED)-th largest r: the first entry of the tail row (NaN for N_USED = 0)
 *   NONTAIL_COUNT            cells with r <= CUT; the N_USED - NONTAIL_COUNT cells above the cut are the last entries of the tail
 *   NONTAIL_M, NONTAIL_S     log-sum-exp pair of r (the log importance ratios) over exactly those cells
 * Order of the sums: thread k of 256 takes the cells of samples k, k + 256, ... in increasing index from the empty sum, a
 * wavefront's 64 partial results are combined by an xor butterfly (distances 32 .. 1), the four wavefronts in wavefront
 * order.  Every number is a function of the cells and their sample indices, not of the chunking.  (tests/pointwise_restated.py
 * is this definition in numpy.)
 */
#define MP_POINTWISE_MAX_SAMPLES 262144
#define MP_POINTWISE_MAX_CELLS 268435456
#define MP_POINTWISE_N 12
#define MP_POINTWISE_N_USED 0
#define MP_POINTWISE_Z_MEAN 1
#define MP_POINTWISE_R_MEAN 2
#define MP_POINTWISE_LL_VAR 3
#define MP_POINTWISE_R_MIN 4
#define MP_POINTWISE_R_MAX 5
#define MP_POINTWISE_LPPD_M 6
#define MP_POINTWISE_LPPD_S 7
#define MP_POINTWISE_CUT 8
#define MP_POINTWISE_NONTAIL_COUNT 9
#define MP_POINTWISE_NONTAIL_M 10
#define MP_POINTWISE_NONTAIL_S 11
int mp_pointwise_tail_len(int64_t n_used);              /* T above; 0 for n_used < 1 */
int mp_model_pointwise(mp_handle *h, const double *pars, int64_t n, int ndim, int physical, int ds_id, double *obs_out,
                       double *tail_out, double *z_out, int32_t *status_out, int64_t *n_used);

/*
 * Importance reweighting of a fit to other error models and data subsets, computed on the device (ABI 5, additive): per sample
 * the log weight that carries a chain sampled under lnlike = -0.5 chi^2 (the light curve's own yerr, every observation counted
 * once) to each of n_alt alternative likelihoods, and per alternative the reductions from which the Bayes factor between the
 * error models, Kish's effective sample size and the Pareto-k diagnostic follow on the host (magprop_amd/reweight.py).  The
 * weights are what mp_model_band_weighted and the weights= arguments of the summaries take.  pars, n, ndim, physical,
 * status_out and n_used are mp_model_pointwise's; the dataset has to be set (MP_ESTATE otherwise).
 *   kind[n_alt]                       MP_REWEIGHT_GAUSS or MP_REWEIGHT_STUDENT
 *   alt[n_alt][3]                     scale (finite, > 0), jitter (finite, >= 0), nu (Student-t: finite, > 0; Gaussian: ignored)
 *   obs_w[n_alt][n_obs]               (optional) a weight per alternative and observation, finite and >= 0, in the order
 *                                     mp_set_dataset keeps the observations: ascending time (stable).  NULL: every weight 1
 *   lw_out[n_alt][n]                  (optional) the log weights, alternative-major
 *   alt_out[n_alt][MP_REWEIGHT_N]     the columns below
 *   tail_out[n_alt][mp_pointwise_tail_len(n)]   (optional) the min(T, N_USED) largest lw of the alternative, ascending, then NaN
 * Limits: 1 <= n <= MP_POINTWISE_MAX_SAMPLES (the tail row relies on it), 1 <= n_alt <= MP_REWEIGHT_MAX_ALT; there is no cell
 * matrix, so n * n_obs has no cap.  The rows go through the device in chunks of mp_n_simd(h) rows, each one launch of the curve
 * kernels (Ltot only) and one launch that turns the chunk's curves into log weights; two reduction launches per call follow.
 * The alternatives and obs_w are uploaded once per call.  Workspace, owned by the handle, grow-only, freed by mp_destroy:
 * n_alt * (n + n_obs + T(n) + MP_REWEIGHT_N + 3) + min(n, mp_n_simd) * n_grid doubles.  A multi-device handle runs the call on
 * its first device and cfg.dipole_torque = 1 is served.
 *
 * Term of sample s (status MP_STATUS_OK), observation j and alternative k, with mod mp_model_pointwise's and every operation
 * rounded on its own (no FMA contraction), log and log1p the device runtime's:
 *   res = y_j - mod,   se = scale_k * yerr_j,   a = se * se,   jm = jitter_k * mod,   b = jm * jm,   var = a + b
 *   q = (res * res) / var,   g = 0.5 * log(var)
 *   MP_REWEIGHT_GAUSS:     t_k = -(0.5 * q + g)
 *   MP_REWEIGHT_STUDENT:   u = q / nu_k,   p = (0.5 * (nu_k + 1)) * log1p(u),   t_k = -(p + g)
 * The base term t_0 is the Gaussian one with scale 1 and jitter 0, formed by the same arithmetic (var = yerr_j * yerr_j).  The
 * difference is d = t_k - t_0 without obs_w, d = w_kj * t_k - t_0 for w_kj != 0 and d = -t_0 for w_kj == 0 (whatever t_k is,
 * NaN or infinite included).  The constants of the densities (-0.5 ln 2 pi per Gaussian point, the Student-t's ratio of gamma functions) are left
 * to the host: magprop_amd.reweight.shape_constant.
 *
 * Row sum: one wavefront owns a sample; lane l adds d of observations l, l + 64, ... in increasing order from 0.0, and the 64
 * partial sums are combined by the xor butterfly (distances 32 .. 1).  lw[k][s] is that sum: a sum of differences, so that an
 * alternative equal to the base gives exactly +0.0, leaving one observation out gives exactly -t_0 of that observation and no
 * cancellation error grows with n_obs.  A sample whose status is not OK has NaN in every alternative (its curve is not read).
 * A row's numbers are a function of the row, the dataset and the alternative, NOT of the chunking, of n or of the row's place.
 *
 * Columns, per alternative over the used samples (the non-NaN lw, N_USED of them; -inf is a used value), T =
 * mp_pointwise_tail_len(N_USED); values order as their sign-magnitude keys do: -0.0 below +0.0:
 *   N_USED                   their number
 *   LW_MEAN                  sum / N_USED (NaN for N_USED = 0)
 *   LW_MIN, LW_MAX           least and largest lw (NaN for N_USED = 0)
 *   LSE1_M, LSE1_S           running log-sum-exp pair of lw: sum exp(lw) = e^M S ((-inf, 0): none)
 *   LSE2_M, LSE2_S           the pair of 2 * lw
 *   CUT                      the min(T, N_USED)-th largest lw: the first entry of the tail row (NaN for N_USED = 0)
 *   NONTAIL_COUNT            samples with lw <= CUT
 *   NONTAIL_M, NONTAIL_S     log-sum-exp pair of lw over exactly those samples
 * in the order of mp_model_pointwise's sums (thread k of 256 takes samples k, k + 256, ...; butterfly; wavefront order).
 *
 * Returns MP_EINVAL for n, ndim, ds_id or n_alt out of range; for a NULL h, pars, kind, alt or alt_out; for a bad alternative
 * (all of this is judged without a handle), in this order; then MP_ESTATE for an unset dataset; then MP_EINVAL for a bad obs_w
 * value.  (tests/reweight_restated.py is this definition in numpy.)
 */
#define MP_REWEIGHT_MAX_ALT 64
#define MP_REWEIGHT_GAUSS 0
#define MP_REWEIGHT_STUDENT 1
#define MP_REWEIGHT_N 12
#define MP_REWEIGHT_N_USED 0
#define MP_REWEIGHT_LW_MEAN 1
#define MP_REWEIGHT_LW_MIN 2
#define MP_REWEIGHT_LW_MAX 3
#define MP_REWEIGHT_LSE1_M 4
#define MP_REWEIGHT_LSE1_S 5
#define MP_REWEIGHT_LSE2_M 6
#define MP_REWEIGHT_LSE2_S 7
#define MP_REWEIGHT_CUT 8
#define MP_REWEIGHT_NONTAIL_COUNT 9
#define MP_REWEIGHT_NONTAIL_M 10
#define MP_REWEIGHT_NONTAIL_S 11
int mp_model_reweight(mp_handle *h, const double *pars, int64_t n, int ndim, int physical, int ds_id, int n_alt,
                      const int32_t *kind, const double *alt, const double *obs_w, double *lw_out, double *alt_out,
                      double *tail_out, int32_t *status_out, int64_t *n_used);

/*
 * Simulated light curves of n parameter rows, computed on the device (ABI 5, additive): the model of every row at observed
 * times, an error per observation and Gaussian noise -- the synthetic datasets of the reference's
 * code/synthetic_datasets/generate_data.py:61-67 (the model at grid points, yerr = 0.25 y, normal noise), for any times inside
 * the grid, and the first step of an injection-recovery study (magprop_amd/calibration.py).  pars, n, ndim and physical are
 * mp_model_derived's.  Host buffers; the call returns when the results are in them:
 *   x[x_rows][n_obs]      observed times; x_rows = 1: every row is observed at the same times, x_rows = n: row i at x[i]
 *   yerr[x_rows][n_obs]   absolute errors, or NULL: the error is frac_err * |model|
 *   y_out, yerr_out, model_out, z_out   [n][n_obs] the data, the errors, the noiseless model (1e50 erg/s, as mp_model_lc returns
 *                         Ltot) and the standard normals; y_out is required, the others may be NULL
 *   status_out[n], *n_ok  (optional) the rows' statuses and the number of rows with MP_STATUS_OK
 * Limits: 1 <= n <= MP_SIM_MAX_ROWS, n_obs >= 1, n * n_obs <= MP_SIM_MAX_CELLS.  The rows go through the device in chunks of
 * mp_n_simd(h) rows, each one launch of the curve kernels (Ltot only, the build mp_model_lc runs for a single row), one launch
 * that turns the chunk's curves into cells, and the copies of the chunk's cells.  Workspace, owned by the handle, grow-only,
 * freed by mp_destroy: min(n, mp_n_simd) * (n_grid + 4 n_obs) doubles of curves and cells, and 3 n_obs doubles and n_obs
 * integers per table row on the device (one row with x_rows = 1, a chunk's rows otherwise).
 * A multi-device handle runs the call on its first device and cfg.dipole_torque = 1 is served, as in mp_model_derived: no
 * state of the handle makes the call return MP_ESTATE.  No dataset is needed.
 *
 * Rows.  A row whose status is not MP_STATUS_OK gets NaN in every output.  Every output number of a row is a function of the
 * row's parameters, its times, its errors, its index i in the call (0 .. n - 1) and the seed; it is NOT a function of the
 * chunking, of n or of the other rows.
 *
 * Model value.  The bracket of a time x on the grid t[0 .. G - 1] is formed on the host, by the code mp_set_dataset digests a
 * light curve with: g the largest index with t[g] <= x, dx = x - t[g], and for g < G - 1 idt = 1 / (t[g + 1] - t[g]) (the
 * last grid point: g = G - 1, dx = 0).  Times need not be sorted and may repeat; outputs are in the caller's order.  A time
 * outside [t[0], t[G - 1]] or not finite: MP_ERANGE.  On the device, with L the row's Ltot:
 *   dx == 0 (x is the knot t[g], the last one included):   mod = L[g]
 *   otherwise:                                             mod = ((L[g + 1] - L[g]) * idt) * dx + L[g]
 * every operation rounded on its own (no FMA contraction).  At grid times model_out therefore equals mp_model_lc's Ltot bit for
 * bit: the reference's recipe.
 *
 * Error.  yerr given: used as is; every value has to be finite and > 0 (MP_EINVAL).  yerr NULL: yerr_out = frac_err * fabs(mod),
 * frac_err finite and > 0 (MP_EINVAL).  A row with a resulting error of 0 (a model value of 0, or a product that underflows)
 * cannot be a dataset: its status is MP_STATUS_ZEROERR and all its outputs are NaN.
 *
 * Noise.  Observation j of row i takes a standard normal z from Philox4x32-10 with key (seed & 0xFFFFFFFF, seed >> 32) and
 * counter ((uint32) i, (uint32) (j / 2), 0, 0x53494D00): with w the four words of the draw, ua = u01(w0, w1), ub = u01(w2, w3),
 * u01(hi, lo) = ((hi << 32 | lo) >> 11) * 2^-53,
 *   rad = sqrt(-2 * log(1 - ua)),   ang = 6.283185307179586 * ub,   z = rad * cos(ang) for even j, rad * sin(ang) for odd j
 * (the one Box-Muller step of the device code, with the device runtime's log, cos, sin and sqrt), and
 *   y = mod + yerr * z
 * product and sum rounded separately.  z_out returns z.  An odd n_obs leaves the second normal of its last pair unused.
 *
 * Returns MP_EINVAL for n, ndim, n_obs, n * n_obs or x_rows out of range, a NULL h, pars, x or y_out, a bad yerr or (yerr NULL) a
 * bad frac_err, in this order; then MP_ERANGE for a bad time.  (tests/simulate_restated.py is this definition in numpy.)
 */
#define MP_SIM_MAX_ROWS 262144
#define MP_SIM_MAX_CELLS 268435456 /* n * n_obs */
int mp_simulate(mp_handle *h, const double *pars, int64_t n, int ndim, int physical, const double *x, int n_obs, int64_t x_rows,
                const double *yerr, double frac_err, uint64_t seed, double *y_out, double *yerr_out, double *model_out,
                double *z_out, int32_t *status_out, int64_t *n_ok);

/*
 * Radii, mass flows and torques of the model of n parameter rows, computed on the device (ABI 5, additive): the quantities
 * INSIDE the model, recovered from the integrated (Mdisc, omega) as code/figure_3.py:202-286 recovers them and
 * code/figure_4.py:139-175 plots them -- the Alfven, corotation and light-cylinder radii, the fastness parameter, the
 * propelled, accreted and fallback mass-flow rates, the accretion and dipole torques -- and per row their reduction to a mass
 * budget, an angular-momentum budget and the answer to whether the sample lives as a propeller or as an accretor.  pars, ndim,
 * physical, status_out and n_used are mp_model_derived's; out[n][MP_FLOW_N] and curves_out are host buffers, and the call
 * returns when the results are in them.  curve_mask selects the cell curves that are returned: bit c is curve MP_FLOW_CURVE_c,
 * curves_out[n][popcount(curve_mask)][n_grid] holds them in the order of the bits (NULL with curve_mask == 0 only).  A row whose
 * status is not MP_STATUS_OK gets NaN columns and NaN cells; no row finished: all NaN and MP_OK.  No dataset is needed; a
 * multi-device handle runs the call on its first device; cfg.dipole_torque = 1 is served.
 *
 * Cell curves, cgs, at every grid point from the row's Mdisc and omega there (what mp_model_lc returns in traj).  They describe
 * the integrated system: the switch is cfg.n_ode (not the luminosity stage's n_lum), cfg.rm_massflow_factor and
 * cfg.inertia_factor apply as in the right-hand side, and the arithmetic is the right-hand side's own (the device functions
 * the solver calls, with the row's constants un-logged once, by the function the curve kernels call):
 *   RM         Alfven radius mu^(4/7) GM^(-1/7) (f Mdisc / tvisc)^(-2/7) after the cap Rm >= k Rlc -> k Rlc
 *   RC, RLC    corotation radius (GM / omega^2)^(1/3); light-cylinder radius c / omega
 *   FASTNESS   w = (Rm / Rc)^1.5
 *   MDOT_PROP  eta2 Mdisc / tvisc, eta2 = (1 + tanh(n (w - 1))) / 2;  MDOT_ACC: eta1 Mdisc / tvisc, eta1 = (1 - tanh(..)) / 2
 *              formed from e = exp(-2 n |w - 1|) as e / (1 + e) or 1 / (1 + e), never as 1 - eta2: the small one of the two keeps
 *              its relative accuracy (and is exactly 0 where a whole wavefront has n |w - 1| > 19.5: it is below 1.2e-17 there)
 *   MDOT_FB    (M0 / tfb) ((t + tfb) / tfb)^(-5/3)
 *   N_ACC      sqrt(GM max(Rm, R)) (Mdot_acc - Mdot_prop), 0 where the rotation parameter T/|W| exceeds 0.27 (the ODE's rule)
 *   N_DIP      -mu^2 omega^3 / (6 c^3); cfg.dipole_torque = 1: -(2/3) (mu^2 omega^3 / c^3) (Rlc / Rm)^3
 *   BRANCH     0 .. 3 as a double: bit 0 = the cap is active, bit 1 = Rm >= R
 * dMdisc/dt = MDOT_FB - MDOT_PROP - MDOT_ACC and domega/dt = (N_ACC + N_DIP) / I are what mp_rhs_batch returns there.
 *
 * Columns.  G = n_grid, t_i the grid:
 *   M_FB, M_PROP, M_ACC    trapezoids of MDOT_FB, MDOT_PROP, MDOT_ACC over the grid (g), formed as mp_model_derived forms E_TOT
 *   J_ACC, J_DIP           trapezoids of N_ACC, N_DIP (g cm^2 / s): angular momentum gained by accretion, lost to the dipole
 *   W_MAX, T_W_MAX, W_END  the largest fastness, its grid time (first occurrence), the fastness at the last grid point
 *   N_PROP                 grid points with FASTNESS >= 1 (the propeller side, eta2 >= 1/2)
 *   T_PROP_FIRST, T_PROP_LAST   grid time of the first and of the last such point; NaN when there is none
 *   N_SWITCH               intervals i with (w_i >= 1) != (w_{i+1} >= 1)
 *   N_CAPPED, N_INSIDE     grid points with BRANCH bit 0 set; with bit 1 clear (the Alfven radius inside the star)
 *   RM_MIN, T_RM_MIN       the smallest RM and its grid time (first occurrence)
 * Every column is a function of the row's cells and the grid alone.  Order of the sums: mp_model_derived's (256 contiguous
 * segments of ceil((G - 1) / 256) intervals, terms in increasing i from 0.0, segment totals in segment order from 0.0, no FMA
 * contraction, no floating-point atomic).  Counts are integers, and extrema and first / last indices are taken under total
 * orders (larger value then lower index; least index), so they have no order to state.  (tests/flows_restated.py is the cells
 * and the reduction in numpy.)
 *
 * n has no cap: the rows go through the device in chunks of mp_n_simd(h) rows, each one launch of the curve kernels with the
 * Mdisc and omega curves only (the build mp_model_lc runs for a single row), the cells launch, the reduction launch and the
 * copies, all on the handle's stream with one wait at the end.  A row's numbers are therefore bit for bit the two kernels
 * applied to what mp_model_lc returns in traj for that row alone, whatever n is and wherever the row sits.  Workspace:
 * 12 * min(n, mp_n_simd) * n_grid doubles (the two curves and the ten cell curves of a chunk; 983 MB at 1 024 x 10 001), owned
 * by the handle's evaluator, grow-only, freed by mp_destroy.
 */
#define MP_FLOW_NCURVES 10
#define MP_FLOW_CURVE_RM 0
#define MP_FLOW_CURVE_RC 1
#define MP_FLOW_CURVE_RLC 2
#define MP_FLOW_CURVE_FASTNESS 3
#define MP_FLOW_CURVE_MDOT_PROP 4
#define MP_FLOW_CURVE_MDOT_ACC 5
#define MP_FLOW_CURVE_MDOT_FB 6
#define MP_FLOW_CURVE_N_ACC 7
#define MP_FLOW_CURVE_N_DIP 8
#define MP_FLOW_CURVE_BRANCH 9
#define MP_FLOW_N 16
#define MP_FLOW_M_FB 0
#define MP_FLOW_M_PROP 1
#define MP_FLOW_M_ACC 2
#define MP_FLOW_J_ACC 3
#define MP_FLOW_J_DIP 4
#define MP_FLOW_W_MAX 5
#define MP_FLOW_T_W_MAX 6
#define MP_FLOW_W_END 7
#define MP_FLOW_N_PROP 8
#define MP_FLOW_T_PROP_FIRST 9
#define MP_FLOW_T_PROP_LAST 10
#define MP_FLOW_N_SWITCH 11
#define MP_FLOW_N_CAPPED 12
#define MP_FLOW_N_INSIDE 13
#define MP_FLOW_RM_MIN 14
#define MP_FLOW_T_RM_MIN 15
int mp_model_flows(mp_handle *h, const double *pars, int64_t n, int ndim, int physical, double *out, uint32_t curve_mask,
                   double *curves_out, int32_t *status_out, int64_t *n_used);

/*
 * Bands of the cell curves above over n samples (ABI 5, additive): per grid point and selected curve, the quantiles q[nq] over
 * the rows that finished, band_out[popcount(curve_mask)][nq][n_grid] in the order of the mask's bits.  weights == NULL: every
 * row counts once and a quantile is np.nanquantile(..., method="linear") of the column, as in mp_model_band; else weights[n]
 * under mp_model_band_weighted's rule (mp_band_weight_units).  Limits are mp_model_band's: 1 <= n <= MP_BAND_MAX_SAMPLES,
 * 1 <= nq <= MP_BAND_MAX_Q, q in [0, 1]; curve_mask is a non-empty mask of MP_FLOW_CURVE_* bits without BRANCH (a flag has no
 * quantile: MP_EINVAL).  status_out[n] and *n_used are optional.
 *
 * The rows go through the chunked pass of mp_model_flows (only the selected curves are written), every chunk's cells landing at
 * its row offset of an n x n_grid matrix per selected curve; those matrices then go through mp_model_band's transpose and select
 * kernels.  The band is therefore the band of what mp_model_flows returns in curves_out for the same rows.  Workspace:
 * (popcount(curve_mask) + 1) * n * n_grid + 2 * min(n, mp_n_simd) * n_grid + popcount(curve_mask) * nq * n_grid doubles, owned
 * by the handle's evaluator.  It is grow-only as mp_model_band's is, except that the popcount(curve_mask) * n * n_grid matrices
 * of a band of more than one curve (11.8 GB at 9 curves x 16 384 rows) are freed before the call returns.
 */
int mp_model_flow_band(mp_handle *h, const double *pars, int n, int ndim, int physical, const double *weights, const double *q,
                       int nq, uint32_t curve_mask, double *band_out, int32_t *status_out, int32_t *n_used);

/*
 * Ensemble sampler: emcee's affine-invariant stretch move (Goodman & Weare 2010) with a random red/blue
 * split per step, as driven by code/synthetic_datasets/synth_mcmc.py:175-185
 * (em.EnsembleSampler(Nwalk, Npars, lnprob, ...).run_mcmc(pos, Nstep)).  Positions, log-posteriors,
 * acceptance counters and the chain stay resident on the device; every half-step is ONE kernel launch that
 * proposes, evaluates the log-posterior, accepts/rejects and stores the chain row (small ensembles: a whole step per
 * launch, mp_sampler_set_whole_step).
 *   n_walkers   walkers per ensemble (even, >= 2*ndim recommended as in emcee)
 *   n_ensembles independent ensembles advanced together (e.g. one per GRB dataset); ens_ds_id[e] is the
 *               dataset of ensemble e (NULL: dataset 0 for all)
 *   a           stretch scale (emcee default 2.0)
 *   target      0: the magnetar log-posterior of this handle; 1: isotropic unit Gaussian (tests of the move)
 * Random numbers: Philox4x32-10 keyed by (seed; step, half, walker) for partner / stretch factor / accept;
 * the split permutations are Fisher-Yates shuffles driven by the same generator on the host.  Same seed => same chain.
 */
typedef struct mp_sampler mp_sampler;
mp_sampler *mp_sampler_create(mp_handle *h, int n_walkers, int n_ensembles, int ndim, const int32_t *ens_ds_id,
                              uint64_t seed, double a, int target);
int mp_sampler_destroy(mp_sampler *s);
/* pos[n_ensembles*n_walkers][ndim] (host): sets the state and evaluates its log-posterior */
int mp_sampler_set_positions(mp_sampler *s, const double *pos);
/* n_steps full steps; chain[n_steps][n_total][ndim] and chain_lnprob[n_steps][n_total] (host, both or neither) */
int mp_sampler_run(mp_sampler *s, int n_steps, double *chain, double *chain_lnprob);
/* mp_sampler_run evaluates a whole step in one launch while 3/2 x the walkers (all ensembles) are at most 19/8 x the SIMDs of
 * the device (2 432 evaluations on an MI355X: they fit two wavefronts per SIMD, or nearly): the proposals of the first half and, for every walker of the second half, both proposals it can end up making
 * (its partner of the first half moved or not); a small kernel then takes the decisions in emcee's order.  Same chain, bit
 * for bit, as one launch per half-step (enable = 0; what larger ensembles get anyway): the half-step launches of the stretch
 * move of a sampler whose whole step fits run the kernel build of the whole-step launch (chosen by its 3/2 x walkers blocks),
 * not the one their own size would choose, so enable = 0 is the check of the default and may be slower than it needs to be.
 * Default: enabled. */
int mp_sampler_set_whole_step(mp_sampler *s, int enable);
/* any of the outputs may be NULL */
int mp_sampler_get_state(mp_sampler *s, double *pos, double *lnprob, int64_t *n_accepted, int64_t *steps_done);
/*
 * Parallel tempering (ABI 5, additive; Earl & Deem 2005, Vousden, Farr & Mandel 2016).  The n_ensembles ensembles form
 * n_ensembles / n_temps groups of n_temps: ensemble e is group e / n_temps at inverse temperature betas[e % n_temps], and all
 * ensembles of a group must be on the same dataset.  The ladder: betas[0] == 1, strictly decreasing, every entry finite and
 * > 0 (beta = 0 is refused: failed models have lnprob = -inf), n_temps >= 2.  Call before the first mp_sampler_set_positions
 * (else MP_ESTATE); a bad ladder, n_ensembles % n_temps != 0 or mixed datasets in a group give MP_EINVAL.
 * The move decides against prior x L^beta: (ndim - 1) ln z + beta lnprob(proposal) - beta lnprob(walker) > ln u (unfused;
 * beta = 1 is the untempered test bit for bit).  After every step of mp_sampler_run each group runs one swap sweep, hottest
 * pair first (t = n_temps - 1 .. 1): slot i of temperature t - 1 (walker perm[i] of that step's split) against slot i of
 * temperature t, accepted if ln u < (beta_{t-1} - beta_t)(lnprob_hot - lnprob_cold), u from Philox keyed
 * (seed; step, 2, cold walker, 0).  An accepted swap exchanges the two walkers' positions and lnprob (acceptance counters stay
 * with the walkers); chain row s is the state after step s's swaps.  Stored and reported lnprob stay untempered.
 * The walker-sharded entry points (mp_sampler_halfstep_*, mp_sampler_step_*) return MP_ESTATE on a tempered sampler.
 */
int mp_sampler_set_temperatures(mp_sampler *s, int n_temps, const double *betas);
/* accepted swaps since the ladder was set, n_swaps_accepted[n_ensembles / n_temps][n_temps - 1] (pair t - 1, t at index t - 1);
 * each pair is proposed n_walkers times per step.  MP_ESTATE on an untempered sampler. */
int mp_sampler_get_swaps(mp_sampler *s, int64_t *n_swaps_accepted);
/*
 * Ladder adaptation (ABI 5, additive; the dynamics of Vousden, Farr & Mandel 2016, ptemcee's, carried from differences of T to
 * the gaps of ln beta).  While it adapts, every group spaces its own ladder on the device until each neighbouring pair swaps
 * equally often.  Both ends stay as set: beta_0 = 1, and the hot end beta_{T-1}, which the evidence estimate relies on, are never
 * written.  A sampler without this call, and an untempered one, launch what they launched before.
 * State per group of T = n_temps >= 3 ensembles: the gaps g_i = ln beta_i - ln beta_{i+1} > 0 (i = 0 .. T - 2) and their sum
 * L = -ln beta_{T-1}.  This call forms them once on the device: lb_i = log(beta_i) with lb_0 = 0, g_i = lb_i - lb_{i+1},
 * L = -lb_{T-1}, and prev_i = the pair's accepted swaps so far.
 * Update t = 0, 1, .. n_adapt - 1: one launch behind the swap sweep of each of the first n_adapt steps of mp_sampler_run (t is the
 * sampler's: it counts on across calls, whatever their lengths).  With kappa_t = lag / (time * (t + lag)), formed on the host in
 * double by these three operations, per group and in double, every operation rounded on its own (no FMA):
 *     A_i   = (double)(swaps_i - prev_i) / (double)n_walkers;  prev_i = swaps_i       the step's acceptance of pair (i, i + 1)
 *     Abar  = (A_0 + A_1 + ... in index order from 0.0) / (double)(T - 1)
 *     h_i   = g_i * exp(kappa_t * (A_i - Abar))
 *     G     = h_0 + h_1 + ... in index order from 0.0;  c = L / G;  g'_i = c * h_i
 *     cum_i = g'_0 + ... + g'_i in index order from 0.0;  beta_{i+1} = exp(-cum_i), i = 0 .. T - 3
 * exp and log are the device runtime's.  A pair that swapped more often than the mean gets a wider gap; the fixed points are the
 * ladders on which every pair is accepted equally often.  The update is taken only if every g'_i is finite and > 0 and the new
 * ladder, both ends included, is strictly decreasing; otherwise g and the ladder stay as they were and the group's count of
 * dropped updates goes up (prev advances either way).  mp_sampler_get_swaps keeps its meaning.
 * Order: a step's moves and its swap sweep read the ladder of the previous update; the new one holds from the next step on.
 * Validity: kappa_t -> 0 (diminishing adaptation), and after update n_adapt - 1 the ladder is frozen for good: steps >= n_adapt
 * are the steps of a fixed-ladder sampler and enqueue no ladder launch.  Use only those steps for estimates (mp_sampler_get_thermo
 * passes over the others by itself).  ptemcee's defaults: lag = 10000, time = 100.
 * mp_sampler_set_ladder_adaptation: after mp_sampler_set_temperatures and before the first mp_sampler_set_positions, else
 * MP_ESTATE.  MP_EINVAL: n_temps < 3, n_adapt < 1, lag or time not finite and > 0, or keep_history with n_adapt x n_ensembles
 * doubles beyond MP_LADDER_MAX_HISTORY_BYTES.  keep_history != 0: row t of a device buffer receives the ladders after update t.
 * mp_sampler_get_temperatures: betas[n_ensembles], the ladders now, one per group (groups adapt independently); *n_updates, the
 * updates made so far; n_dropped[n_ensembles / n_temps].  On a fixed ladder: the ladder as set, 0 and zeros.  Any output may be
 * NULL.  MP_ESTATE on an untempered sampler.
 * mp_sampler_get_ladder_history: rows [first_row, first_row + max_rows) of group `group`, as far as they exist, into
 * betas[rows][n_temps]; *n_rows: the rows written.  MP_ESTATE without a history, MP_EINVAL on a bad group or range.
 */
#define MP_LADDER_MAX_HISTORY_BYTES 268435456   /* 256 MB */
int mp_sampler_set_ladder_adaptation(mp_sampler *s, int64_t n_adapt, double lag, double time, int keep_history);
int mp_sampler_get_temperatures(mp_sampler *s, double *betas, int64_t *n_updates, int64_t *n_dropped);
int mp_sampler_get_ladder_history(mp_sampler *s, int group, int64_t first_row, int64_t max_rows, double *betas, int64_t *n_rows);
/*
 * Proposal moves (ABI 5, additive; emcee 3's moves=).  Every move is a red-blue move over the step's two-way split: walker k
 * of the active half draws its partners from the n_comp = n_walkers - n_half slots of the other half.  Random numbers are
 * Philox4x32-10 keyed (seed; step, half, k, c3): the stretch move uses c3 = 0, 1, DE and snooker c3 = 2 (r) and 3 (r2).
 * pick(u, m) = min(floor(u m), m - 1); a second index distinct from a first is pick(u', m - 1), plus 1 if >= the first; a third
 * is drawn over m - 2 and steps over the first two in increasing order.  u01(a, b) = 53-bit uniform of the pair.  All proposal
 * arithmetic is unfused (separately rounded products and sums, IEEE division), so a numpy restatement reproduces the chain.
 *   MP_MOVE_STRETCH  params[0] = a (> 1): the stretch move of mp_sampler_create.
 *   MP_MOVE_DE       (ter Braak 2006) params[0] = g0 (0: 2.38 / sqrt(2 ndim)), params[1] = sigma in [0, 1/sqrt(3)).
 *                    Partners c1 = pick(u01(r0, r1), n_comp), c2 distinct from c1 by u01(r2, r3); gamma = g0 (1 + s (2 u01(r2_0,
 *                    r2_1) - 1)), s = sigma sqrt(3): gamma is uniform with standard deviation sigma g0 (emcee draws it normal).
 *                    q = x_k + gamma (x_c1 - x_c2), Hastings term 0.
 *   MP_MOVE_SNOOKER  (ter Braak & Vrugt 2008) params[0] = gamma_s (> 0; emcee's default 1.7).  Partners z, z1, z2 from (r0, r1),
 *                    (r2, r3), (r2_0, r2_1), all three distinct.  d = x_k - z, dd = sum d_i^2, p = sum d_i (z1_i - z2_i) (index
 *                    order), q = x_k + (gamma_s (p / dd)) d, Hastings term h = (ndim - 1)/2 (ln sum (q - z)_i^2 - ln dd) (dd = 0:
 *                    NaN, rejected).  emcee splits the walkers four ways for this move; here the split is two-way.
 *   MP_MOVE_KDE      (emcee's KDEMove) params[0] = bandwidth: 0 Scott, f = n_comp^(-1/(ndim+4)); -1 Silverman, f = (n_comp
 *                    (ndim + 2)/4)^(-1/(ndim+4)); > 0 (finite) the factor f itself; params[1] = 0.  Over the slots C of the other
 *                    half: mu = their mean, S = their sample covariance (ddof 1), Sigma = f^2 S = L L^T (Cholesky).  Partner c =
 *                    pick(u01(r0, r1), n_comp) from r = Philox(...; c3 = 0x4B00); n_i standard normals by Box-Muller, pair p from
 *                    Philox(...; c3 = 0x4B01 + p): n_2p, n_2p+1 = sqrt(-2 ln(1 - u01(s0, s1))) cos, sin (2 pi u01(s2, s3)).
 *                    q = x_c + L n.  Hastings term h = lse_j(-|L^-1 (x_k - x_j)|^2 / 2) - lse_j(-|L^-1 (q - x_j)|^2 / 2), j over
 *                    C, lse = log-sum-exp with the maximum subtracted first (the kernel's normalising constants cancel).  ln u =
 *                    ln u01(r2, r3).  Where S is not positive definite (a pivot of the factorisation not finite and > 0), every
 *                    proposal of that ensemble in that half-step is NaN, is rejected and is never stored.  Sums and the
 *                    log-sum-exp run in a fixed order of their own (workgroup reductions), so a restatement agrees to rounding
 *                    and to the accuracy of log, exp, sqrt, cos, sin; n_comp >= ndim + 1 is required.
 * ln u = ln u01(r2_2, r2_3) for DE and snooker.  Decision (every move but the slice move): h + beta lnprob(q) - beta lnprob(x_k) >
 * ln u, beta of the walker's ensemble (1 untempered); the stretch move's h is (ndim - 1) ln z.
 *   MP_MOVE_SLICE    (ensemble slice sampling: Karamanis & Beutler 2021 over Neal 2003's stepping out and shrinkage) params[0] =
 *                    mu0 (finite, > 0), params[1] = tune_steps (a whole number in [0, 2^31 - 1]); at most one entry per table,
 *                    n_half >= 2.  Not a propose-then-reject move: every update that does not fail moves the walker.  A slice step
 *                    is two half-step launches over the step's split, a tune launch, then the swap sweep when tempered.  Walker
 *                    k at x with stored lnprob lnp_x, its ensemble e at inverse temperature beta_e (1 untempered) and scale mu_e;
 *                    r = Philox(...; c3 = 0x51C00000 + c):
 *                      c = 0      partners c1 = pick(u01(r0, r1), n_comp), c2 distinct from c1 by u01(r2, r3) (the DE rule), from the
 *                                 other half as it stands; direction d = x_c1 - x_c2.
 *                      c = 1      L = -(mu_e u01(r0, r1)), R = L + mu_e; of the stepping-out budget m = max_steps_out, J = floor(m
 *                                 u01(r2, r3)) steps go left and K = m - 1 - J right.
 *                      c = 2      level lny = beta_e lnp_x + ln u01(r0, r1) (product and sum rounded separately; ln 0 = -inf).
 *                      c = 3 + i  shrink point i = 0 .. max_shrink - 1: t = L + u01(r0, r1) (R - L).
 *                    Points on the line: q(t)_i = x_i + t d_i (unfused).  q is inside if it lies in the handle's prior box (target 0
 *                    only, sampler coordinates; a point outside the box is not evaluated) and beta_e lnprob(q) > lny, a NaN lnprob
 *                    counting as -inf.  Stepping out: while J > 0 and q(L) is inside, L -= mu_e, J -= 1; then while K > 0 and q(R)
 *                    is inside, R += mu_e, K -= 1.  Shrinkage: if q(t) is inside the walker moves there (n_accepted[k] += 1, its
 *                    stored lnprob the untempered value of q), else L = t if t < 0, else R = t.  The slice fails, and the walker
 *                    stays, after max_shrink rejected points, and at once when d = 0 in every coordinate.  A walker whose own
 *                    lnprob is -inf has lny = -inf: any point with a finite lnprob is inside, and it escapes.  Every evaluated
 *                    point whose model failed goes to the fbad window (mp_sampler_get_bad): a slice step evaluates several
 *                    points per walker, so the window fills sooner than with the other moves.
 *                    Tuning (zeus's rule, a function of the chain alone): behind the second half-step, for every ensemble, with
 *                    that step's stepping-out steps nexpand_s and rejected shrink points ncontract_s: while fewer than tune_steps
 *                    slice steps have been taken since mp_sampler_set_moves, mu_e <- mu_e (2 a / (a + ncontract_s)), a = max(1,
 *                    nexpand_s) (IEEE quotient in double, the product rounded separately).  mu_e, the count of slice steps and
 *                    the totals live on the device and survive mp_sampler_run calls and mp_sampler_set_positions; only
 *                    mp_sampler_set_moves resets them, so a run does not depend on how it is split into calls.  Steps of a
 *                    mixture that draw another move change nothing of it.  Behind the tuning steps, which the user discards, the
 *                    chain is a plain Markov chain.
 *   MP_MOVE_GAUSSIAN (emcee's GaussianMove: plain Metropolis with a given covariance; the one move that reads nothing of the
 *                    other walkers, so it runs with 2 walkers) params[0] = scale0 (finite, > 0), params[1] = tune_steps (a whole
 *                    number in [0, 2^31 - 1]); at most one entry per table; mp_sampler_set_gaussian must have been called, else
 *                    MP_ESTATE (the params are checked first).  L = the Cholesky factor of the covariance and the mode of
 *                    mp_sampler_set_gaussian, sigma_e = the scale of the walker's ensemble e (it starts at scale0).  r =
 *                    Philox(...; c3 = 0x47410000), ln u = ln u01(r2, r3); normals n_2p, n_2p+1 by the KDE move's Box-Muller
 *                    formula from Philox(...; c3 = 0x47410001 + p).  MP_GAUSS_VECTOR: q_a = x_a + sigma_e (sum_{b <= a} L_ab n_b),
 *                    the sum in index order from 0.  MP_GAUSS_RANDOM: axis a = pick(u01(r0, r1), ndim), MP_GAUSS_SEQUENTIAL: a =
 *                    step mod ndim; q_a = x_a + sigma_e (L_aa n_0), the other coordinates unchanged.  Hastings term 0.
 *                    Tuning (a function of the chain alone, every operation a separately rounded double operation): behind the
 *                    second half-step of a Gaussian step, for every ensemble, with a = that step's accepted walkers of the
 *                    ensemble, r = a / n_walkers and t = target_accept: while n_tuned_e < tune_steps, f = (r + t) / (2 t), g = 8 /
 *                    (8 + n_tuned_e), sigma_e <- sigma_e (1 + g (f - 1)), n_tuned_e += 1.  f is 1 at the target and 1/2 at r = 0,
 *                    the gain decays like 1/n; the constants are the move's definition.  sigma_e, n_tuned_e and the totals live
 *                    on the device and survive mp_sampler_run calls and mp_sampler_set_positions; only mp_sampler_set_moves
 *                    resets them, so split runs give one run's chain.  Steps of a mixture that draw another move change nothing
 *                    of it.  Behind the tuning steps, which the user discards, the chain is a plain Markov chain.
 *   MP_MOVE_WALK     (Goodman & Weare 2010's walk move, emcee's WalkMove) params[0] = s: 0 = all n_comp slots of the other half,
 *                    else a whole number in 2 .. min(n_comp, MP_WALK_MAX_S) (or n_comp itself, which is s = 0); params[1] = 0;
 *                    n_half >= 2.  r = Philox(...; c3 = 0x57410000), ln u = ln u01(r2, r3).  Members: with s = n_comp, member_i =
 *                    i; otherwise s distinct slots by Floyd's algorithm, for i = 0 .. s - 1: j = n_comp - s + i, t = pick(u_i, j +
 *                    1), u_i = u01 of the words (0, 1) for even i, (2, 3) for odd i, of Philox(...; c3 = 0x57410100 + i / 2);
 *                    member_i = t unless t is a member already, then j.  z_i standard normals by the KDE move's Box-Muller
 *                    formula, pair p from Philox(...; c3 = 0x57800000 + p).  m = (sum_i x_member_i) / s, q = x_k + (sum_i z_i
 *                    (x_member_i - m)) / sqrt(s - 1): the covariance of q - x_k is the sample covariance (ddof 1) of the members,
 *                    without a factorisation, so s < ndim + 1 is allowed.  Both sums run in the KDE move's order over i (thread
 *                    t of the workgroup takes i = t, t + 64 W, ..., a butterfly over the wavefront, the wavefronts in order).
 *                    Hastings term 0.
 * The Gaussian and walk moves run two half-step launches of a kernel of their own (normal_half_kernel; the Gaussian move a tune
 * launch behind them) and decide beta lnprob(q) - beta lnprob(x_k) > ln u; failed models go to the fbad window.
 * Philox counters c3 in use: 0, 1 (stretch), 2, 3 (DE, snooker), 0x4B00 .. 0x4B05 (KDE), 0x5117 (splits), 0x30FE (move of a
 * step), 0 with half = 2 (swaps), 0x51C00000 + c, c = 0 .. 2 + max_shrink (slice move), 0x47410000 .. 0x47410000 + (ndim + 1) / 2
 * (Gaussian move), 0x57410000, 0x57410100 .. 0x5741011F and 0x57800000 + p, p < 2^22 (walk move); the optimizer 0xDE00 .. and 0xDEFF, the
 * nested sampler 0x4E000000 + j (random walk) and 0x4E400000 + 0x100 s + c (slice mode), the SMC sampler 0x534D0000 + c, c = 0
 * (a stage's resampling offset) .. 2 walks (its moves).
 * Mixtures: one move per step for the whole sampler.  With n_moves > 1, step s draws r = Philox(seed; s, 3, 0, 0x30FE) and takes
 * the first move m with u01(r0, r1) C_last < C_m, C the cumulative weights (summed in order, double): the move of a step depends
 * on (seed, s, table) only, so split runs give the chain of one run.  DE, snooker, KDE and slice steps run two half-step launches (plus the
 * swap sweep when tempered); stretch steps run as mp_sampler_set_whole_step decides.
 * n_moves == 0 restores the default (the stretch move with the a of mp_sampler_create); may be called between runs.
 * MP_EINVAL: NULL sampler or arrays, n_moves outside [0, MP_MAX_MOVES], an unknown kind, a weight that is not finite and > 0,
 * bad params (NaN and inf included), DE with n_half < 2, snooker with n_half < 3, KDE with n_comp < ndim + 1, slice with n_half < 2 or a second slice entry,
 * a second Gaussian entry, walk with a non-whole s, s = 1, s > n_comp, s > MP_WALK_MAX_S (unless s = n_comp), params[1] != 0 or
 * n_half < 2.  MP_ESTATE: a Gaussian entry before mp_sampler_set_gaussian.  With a table
 * set (n_moves > 0), the walker-sharded entry points (mp_sampler_halfstep_*, mp_sampler_step_*) return MP_ESTATE.
 */
#define MP_MOVE_STRETCH 0   /* params: a (> 1)                                              */
#define MP_MOVE_DE      1   /* params: g0 (0: 2.38/sqrt(2 ndim)), sigma in [0, 1/sqrt(3))    */
#define MP_MOVE_SNOOKER 2   /* params: gamma_s (> 0)                                         */
#define MP_MOVE_KDE     3   /* params: bandwidth (0 Scott, -1 Silverman, > 0 factor), 0      */
#define MP_MOVE_SLICE   4   /* params: mu0 (> 0), tune_steps (whole, 0 .. 2^31 - 1)            */
#define MP_MOVE_GAUSSIAN 5  /* params: scale0 (finite, > 0), tune_steps (whole, 0 .. 2^31 - 1) */
#define MP_MOVE_WALK    6   /* params: s (0: all of the other half; else whole, 2 .. min(n_comp, MP_WALK_MAX_S)), 0 */
#define MP_WALK_MAX_S   64
#define MP_MAX_MOVES    8
int mp_sampler_set_moves(mp_sampler *s, int n_moves, const int32_t *kinds, const double *weights,
                         const double *params /* [n_moves][2] */);
/* The limits of a slice of MP_MOVE_SLICE: the stepping-out budget (1 .. MP_NEST_MAX_STEPS_OUT, default 32) and the shrink points
 * before a slice counts as failed (1 .. MP_SLICE_MAX_SHRINK, default 64).  May be called between runs; MP_EINVAL outside the ranges. */
#define MP_SLICE_MAX_SHRINK 252
int mp_sampler_set_slice_limits(mp_sampler *s, int max_steps_out, int max_shrink);
/* The state of MP_MOVE_SLICE, each output [n_ensembles] and optional (NULL): the scale mu now and, since mp_sampler_set_moves,
 * the stepping-out steps taken, the shrink points rejected, the slices that failed, the points evaluated and the slice steps taken
 * (mu is tuned while that is below tune_steps).  MP_ESTATE when the move table has no slice move. */
int mp_sampler_get_slice(mp_sampler *s, double *mu, int64_t *nexpand, int64_t *ncontract, int64_t *nfail, int64_t *neval,
                         int64_t *n_tuned);
/* The covariance and mode of MP_MOVE_GAUSSIAN, to be set before a table with that move.  L[ndim (ndim + 1) / 2]: the Cholesky
 * factor of the covariance in sampler coordinates, lower triangle by rows (entry (a, b <= a) at a (a + 1) / 2 + b).  mode:
 * MP_GAUSS_VECTOR (all coordinates at once), MP_GAUSS_RANDOM (one axis drawn per proposal) or MP_GAUSS_SEQUENTIAL (axis step mod
 * ndim); target_accept: the acceptance fraction the tuning aims at.  May be called between runs; the scales and counters stay.
 * MP_EINVAL: NULL argument, an unknown mode, a non-finite entry, a diagonal entry that is not > 0, an off-diagonal entry other
 * than 0 with a single-axis mode (emcee's rule), target_accept outside (0, 1). */
#define MP_GAUSS_VECTOR     0
#define MP_GAUSS_RANDOM     1
#define MP_GAUSS_SEQUENTIAL 2
int mp_sampler_set_gaussian(mp_sampler *s, const double *L, int mode, double target_accept);
/* The state of MP_MOVE_GAUSSIAN, each output [n_ensembles] and optional (NULL): the scale sigma now and, since
 * mp_sampler_set_moves, the proposals made, the proposals accepted and the tuning updates made (at most tune_steps).  MP_ESTATE
 * when the move table has no Gaussian move. */
int mp_sampler_get_gaussian(mp_sampler *s, double *sigma, int64_t *n_proposed, int64_t *n_accepted, int64_t *n_tuned);
/*
 * Proposals inside the prior whose model evaluation failed ('flag' / non-finite): what the reference's lnprob appends
 * to its `fbad` file (code/synthetic_datasets/mcmc_eqns.py:72-79).  The kernels collect them in a device-side window of
 * MP_BAD_WINDOW rows which the library drains into a host-side log (after every chunk of mp_sampler_run and in this
 * call), so the log holds every failed proposal unless more than MP_BAD_WINDOW of them arrive between two drains.
 * *n_bad = how many there were since the sampler was created (exact); *n_logged (optional) = rows in the log;
 * rows [first_row, first_row + max_rows) of the log are copied to pars[max_rows][ndim] (sampler coordinates).
 * Returns the number of rows copied (>= 0) or a negative MP_E* code.
 */
#define MP_BAD_WINDOW 65536
int mp_sampler_get_bad(mp_sampler *s, int64_t first_row, double *pars, int max_rows, int64_t *n_bad, int64_t *n_logged);

/*
 * Walker-sharded ensembles (one process per GPU; the reference's counterpart is emcee's pool.map over
 * walkers, code/synthetic_datasets/synth_mcmc.py:178-185).  Every process holds a sampler with the same seed and the
 * full ensemble state.  A half-step has n_slots = mp_sampler_n_slots() proposals (the active half of every ensemble);
 * the process that owns slots [slot_lo, slot_hi) runs
 *     mp_sampler_halfstep_shard(s, half, slot_lo, slot_hi, d_rows + slot_lo*R, stream)    R = mp_sampler_row_doubles()
 * which draws, evaluates and accept-tests exactly what the single-GPU launch would for those walkers (the random numbers
 * are keyed by (seed; step, half, walker)) and writes one outcome row per slot: proposal[ndim], its lnprob, accepted
 * (0/1), status.  After the rows of all processes have been gathered (ONE all-gather per half-step; RCCL through
 * torch.distributed in magprop_amd/distributed.py) every process commits them with
 *     mp_sampler_halfstep_apply(s, half, d_rows, d_chain_row, d_chain_lnp_row, stream)
 * (d_rows[n_slots][R]; the optional d_chain_row[n_total][ndim] / d_chain_lnp_row[n_total] receive this step's entries of
 * the walkers that moved; both NULL or both set).  half = 0 then 1; the apply of half 1 ends the step.  All pointers
 * are device pointers; nothing synchronises with the host.  The resulting chain is the one mp_sampler_run produces
 * (bit for bit while both run the same kernel variant).
 */
int mp_sampler_n_slots(const mp_sampler *s);
int mp_sampler_row_doubles(const mp_sampler *s);
int mp_sampler_halfstep_shard(mp_sampler *s, int half, int slot_lo, int slot_hi, double *d_rows, void *stream);
int mp_sampler_halfstep_apply(mp_sampler *s, int half, const double *d_rows, double *d_chain_row,
                              double *d_chain_lnp_row, void *stream);
/*
 * The same with a WHOLE step per launch and ONE all-gather per step (mp_sampler_set_whole_step describes the launch):
 * a step has mp_sampler_step_blocks() = 3 * n_slots evaluations; every process runs
 *     mp_sampler_step_shard(s, block_lo, block_hi, d_rows, stream)
 * on its share of them, which writes one row of R' = mp_sampler_step_row_doubles() doubles per block to d_rows[b - block_lo]
 * (proposal[ndim], its lnprob, status, (ndim - 1) ln z, ln u, the walker's lnprob before the move, its partner's slot);
 * after the rows of all processes have been gathered every process commits the step with
 *     mp_sampler_step_apply(s, d_rows, d_chain_row, d_chain_lnp_row, stream)
 * (d_rows[3 * n_slots][R'], row index = block index).  Two launches and one collective per step instead of four and two;
 * a third of the evaluations is discarded, so this pays while a rank's share of the blocks fits its device two wavefronts
 * per SIMD (magprop_amd/distributed.py decides).  Same chain as the half-step protocol and as mp_sampler_run (bit for bit
 * while both run the same kernel variant, see DESIGN.md section 7: a launch of the sharded entry points chooses its build by
 * its own block count).
 */
int mp_sampler_step_blocks(const mp_sampler *s);
int mp_sampler_step_row_doubles(const mp_sampler *s);
int mp_sampler_step_shard(mp_sampler *s, int block_lo, int block_hi, double *d_rows, void *stream);
int mp_sampler_step_apply(mp_sampler *s, const double *d_rows, double *d_chain_row, double *d_chain_lnp_row, void *stream);
/* device pointers of the resident state: pos[n_total][ndim], lnprob[n_total] (read-only for the caller) */
int mp_sampler_state_ptrs(mp_sampler *s, double **d_pos, double **d_lnprob);

/*
 * Autocorrelation monitor (ABI 5, additive): the integrated autocorrelation time that emcee's get_autocorr_time() reports
 * (Sokal's automatic window, Goodman & Weare 2010; code/synthetic_datasets/synth_mcmc.py:216), accumulated on the device while
 * mp_sampler_run runs.  Off by default; while it is off nothing about the sampler changes.
 * A series is one coordinate d of one walker w of one ensemble e: the positions the sampler writes to its chain row, in sampler
 * coordinates.  Sample t = 0 is the first step `discard` steps after the monitor was (re)started, n the number of samples so far.
 * With the pivot p = x_0, y_t = x_t - p and K = max_lag the monitor keeps, per series and for the lags k = 0 .. K - 1,
 *     S_k = sum_{t >= k} y_t y_{t-k},   T = sum_t y_t,   the head sums H_k = sum_{t < k} y_t,   the last K values of y,
 * whose sums give the tails L_k = sum_{t >= n - k} y_t.  Every sum runs in increasing t from 0.0, and every product, sum and
 * difference is rounded on its own (no FMA), so the accumulators are a function of the sample sequence alone: they do not depend
 * on how mp_sampler_run chunks its steps or on how a run was split into calls, and a numpy restatement reproduces them bit for bit.
 * Finalisation is emcee's estimator in moment form:
 *     m = T / n,   c_k = (S_k - m ((2 T - H_k) - L_k)) + (n - k) (m m),   rho_k = c_k / c_0 (0 where c_0 = 0),
 *     f_k = (sum of rho_k over the ensemble's walkers in walker order) / n_walkers,
 *     taus_M = 2 (f_0 + ... + f_M) - 1 (summed in lag order),   window = the smallest M for which M < c taus_M is false,
 *     tau = taus_window.
 * Lags below min(K, n) are known.  Where none of them is a window: with n <= K the window is the last lag n - 1 (what the host
 * estimator magprop_amd.mcmc_io.integrated_time falls back to); with n > K tau is NaN and the window -1: max_lag was too small,
 * and a truncated sum is never returned as a number.
 *
 * mp_sampler_set_autocorr(s, max_lag, discard): max_lag = 0 turns the monitor off and frees it; 1 .. MP_ACF_MAX_LAG (re)starts
 * it empty, accumulation beginning `discard` (>= 0) steps from now.  MP_EINVAL: max_lag or discard out of range, or accumulators
 * (the ring of kept values, S, H and the finalisation's work array: about 4 max_lag + the rows of 64 MB of chain, times 8 bytes,
 * per series) beyond MP_ACF_MAX_BYTES; the monitor is then off.
 * While the monitor is on: mp_sampler_run writes its chain rows to the device slab also when `chain` is NULL (nothing is copied
 * to the host then) and feeds the monitor once per chunk, on the handle's stream, behind the chunk's last step;
 * mp_sampler_set_positions restarts the monitor (the series is broken; `discard` applies again); the walker-sharded entry points
 * (mp_sampler_halfstep_*, mp_sampler_step_*) do not feed it and return MP_ESTATE.
 * mp_sampler_get_autocorr: tau[n_ensembles][ndim], window[n_ensembles][ndim] (either may be NULL) for the window constant c
 * (emcee's default 5); *n_samples = n (optional).  MP_ESTATE without a monitor or with n < 2.
 * mp_sampler_get_acf: the walker-mean f_k of one ensemble, acf[rows][ndim] with rows = min(max_rows, max_lag, n), which it returns
 * (or a negative MP_E* code; MP_ESTATE as above).
 * mp_sampler_get_autocorr_sums: the raw accumulators of one ensemble (tests): S[max_lag][n_walkers][ndim], T[n_walkers][ndim],
 * H[max_lag][n_walkers][ndim] (H_k = T for k > n), tail[max_lag][n_walkers][ndim] (row i is y_{n - max_lag + i}; zeros before
 * sample 0), pivot[n_walkers][ndim]; any may be NULL.  MP_ESTATE without a monitor.
 */
#define MP_ACF_MAX_LAG 4096
#define MP_ACF_MAX_BYTES 8589934592   /* 8 GiB */
int mp_sampler_set_autocorr(mp_sampler *s, int max_lag, int64_t discard);
int mp_sampler_get_autocorr(mp_sampler *s, double c, double *tau, int32_t *window, int64_t *n_samples);
int mp_sampler_get_acf(mp_sampler *s, int ensemble, int max_rows, double *acf);
int mp_sampler_get_autocorr_sums(mp_sampler *s, int ensemble, double *S, double *T, double *H, double *tail, double *pivot,
                                 int64_t *n_samples);

/*
 * Posterior monitor (ABI 5, additive): histograms, moments and the best sample of the chain, accumulated on the device while
 * mp_sampler_run runs, so that credible intervals, the marginals of a corner plot and the best fit need no chain on the host.
 * Off by default; while it is off nothing about the sampler changes.  Everything below is a function of the set or sequence
 * of samples alone: it does not depend on how mp_sampler_run chunks its steps or on how a run was split into calls, and a numpy
 * restatement (tests/post_restated.py) reproduces every number bit for bit.
 * A sample is the position x[0 .. ndim) (sampler coordinates) and the stored, untempered lnprob of one walker w of one ensemble
 * e at one step.  Only steps from `discard` steps after the monitor was (re)started count; t counts them from 0, n of them so
 * far.  Sample index inside an ensemble: i = t * n_walkers + w.  Every ensemble is monitored on its own; the temperatures of a
 * tempered sampler are ensembles like any other.
 * Settings: bins1 (1 .. MP_POST_MAX_BINS), bins2 (0 .. MP_POST_MAX_BINS2; 0: no 2-D histograms), lower[ndim] < upper[ndim],
 * all finite with a finite width.  The host forms once, in double, per dimension d
 *     inv1_d = bins1 / (upper_d - lower_d),   inv2_d = bins2 / (upper_d - lower_d),   pivot_d = lower_d + 0.5 (upper_d - lower_d).
 * Bin rule, for a coordinate value v, a bin count B and its inverse width inv: NaN or +-inf is "non-finite"; v < lower is
 * "below"; v >= upper is "above"; otherwise b = (int)floor((v - lower) * inv), and b = B - 1 where that gives B (the difference
 * and the product are each rounded on their own; with lower = -5, upper = 5, B = 256 the largest double below 5 gives 256.0).
 * 1-D: per dimension hist1[d][bins1], below[d], above[d], nonfinite[d], int64 counts; every sample lands in exactly one of them
 * per dimension.
 * 2-D (bins2 > 0): one histogram per pair a < b in lexicographic order (0,1), (0,2), ..., npairs = ndim (ndim - 1) / 2 of them;
 * hist2[p][ba][bb] under the bin rule with bins2; a sample with either coordinate not in a bin counts in outside2[p] instead.
 * Moments: over the samples whose coordinates are all finite (n_finite of them), with y = x - pivot, per walker and in
 * increasing t from 0.0:  s1[w][d] = sum y_d,  s2[w][a][b] = sum (y_a * y_b) for a <= b, the product rounded before the sum, no
 * FMA.  Per ensemble the walkers are summed in walker order from 0.0.  The ABI returns those totals, the pivot and n_finite;
 * mean and covariance are formed above the ABI (magprop_amd.posterior.mean_cov).
 * Best sample: the largest lnprob over the monitored samples, its position and its sample index.  A sample replaces the holder
 * iff its lnprob is greater, or equal with a lower index; the holder starts at "none" (index -1, lnprob -inf, position NaN).
 * So -inf and NaN never win, and ties go to the first occurrence.
 *
 * mp_sampler_set_posterior(s, bins1, bins2, lower, upper, discard): bins1 = 0 turns the monitor off and frees it (the other
 * arguments are ignored); otherwise it (re)starts empty, accumulation beginning `discard` (>= 0) steps from now.  MP_EINVAL:
 * bins1 or bins2 out of range, NULL, non-finite or empty ranges, discard < 0, more than 65 535 ensembles, or accumulators of
 *     8 (n_ensembles (ndim (bins1 + 3) + npairs (bins2^2 + 1) + ndim + 2) + n_total (ndim + ndim (ndim + 1) / 2 + 1)) bytes
 * beyond MP_POST_MAX_BYTES; the monitor is then off.
 * While the monitor is on, the rules of the autocorrelation monitor hold: mp_sampler_run writes its chain rows and their lnprob
 * to the device slab also when `chain` is NULL and feeds the monitor once per chunk, on the handle's stream, behind the chunk's
 * last step (chunks of at most 64 MB of chain rows; next to the autocorrelation monitor, the smaller of the two caps);
 * mp_sampler_set_positions restarts it (`discard` applies again); the walker-sharded entry points (mp_sampler_halfstep_*,
 * mp_sampler_step_*) do not feed it and return MP_ESTATE.  It runs with tempering, move tables, whole-step and half-step launches.
 * Read-outs (one ensemble each; any output pointer may be NULL; MP_ESTATE without a monitor, MP_EINVAL on a bad ensemble; with
 * no sample yet they succeed with zeros and best = none):
 * mp_sampler_get_posterior_hist1: hist1[ndim][bins1], below, above, nonfinite[ndim], *n_samples = n * n_walkers.
 * mp_sampler_get_posterior_hist2: hist2[npairs][bins2][bins2], outside2[npairs]; MP_ESTATE when bins2 = 0.
 * mp_sampler_get_posterior_moments: sum1[ndim], sum2[ndim][ndim] (both triangles filled), pivot[ndim], *n_finite.
 * mp_sampler_get_posterior_best: x[ndim], *lnprob, *index.
 */
#define MP_POST_MAX_BINS 4096
#define MP_POST_MAX_BINS2 128
#define MP_POST_MAX_BYTES 1073741824   /* 1 GiB */
int mp_sampler_set_posterior(mp_sampler *s, int bins1, int bins2, const double *lower, const double *upper, int64_t discard);
int mp_sampler_get_posterior_hist1(mp_sampler *s, int ensemble, int64_t *hist1, int64_t *below, int64_t *above,
                                   int64_t *nonfinite, int64_t *n_samples);
int mp_sampler_get_posterior_hist2(mp_sampler *s, int ensemble, int64_t *hist2, int64_t *outside2);
int mp_sampler_get_posterior_moments(mp_sampler *s, int ensemble, double *sum1, double *sum2, double *pivot, int64_t *n_finite);
int mp_sampler_get_posterior_best(mp_sampler *s, int ensemble, double *x, double *lnprob, int64_t *index);

/*
 * Thermodynamic monitor (ABI 5, additive): per ensemble the sum of the stored, untempered lnprob over the monitored steps, which
 * is all that thermodynamic integration over a ladder needs of a run, so that the evidence needs no chain on the host.  Off by
 * default; fed like the two monitors above (once per chunk from the device slab's lnprob rows; mp_sampler_set_positions restarts
 * it; the walker-sharded entry points return MP_ESTATE while it is on).
 * A step is monitored if it lies `discard` or more steps behind the (re)start AND, on a sampler with ladder adaptation, is a step
 * >= n_adapt: the steps on a ladder that still moved are passed over.  Per ensemble e and monitored step, in step order:
 *     rowsum = the sum of the walkers' finite lnprob: thread k of 256 adds walkers k, k + 256, ... in increasing index from 0.0,
 *              then the xor butterfly over distances 32 .. 1 inside each wavefront and the four wavefronts in order;
 *     sum[e] = sum[e] + rowsum, one add per step;  n_finite[e], n_nonfinite[e]: the counts of the cells (-inf, +inf and NaN are
 *              non-finite and enter no sum).
 * So the numbers are a function of the samples alone, not of chunks or of how a run was split into calls.
 * mp_sampler_set_thermo(s, discard): discard >= 0 (re)starts the monitor empty, discard = -1 turns it off; else MP_EINVAL.
 * mp_sampler_get_thermo: sum_lnl, n_finite, n_nonfinite [n_ensembles], *n_steps the monitored steps; any output may be NULL;
 * MP_ESTATE while the monitor is off.
 */
int mp_sampler_set_thermo(mp_sampler *s, int64_t discard);
int mp_sampler_get_thermo(mp_sampler *s, double *sum_lnl, int64_t *n_finite, int64_t *n_nonfinite, int64_t *n_steps);

/*
 * Sample reservoir (ABI 5, additive): per ensemble a uniform random subset of fixed size of the run's samples, kept on the device
 * with their lnprob and where they came from, so that the light-curve band, the derived quantities, the flows and the pointwise
 * scores of a fit (mp_model_band, mp_model_derived, mp_model_flows, mp_model_pointwise) need no chain on the host.  Off by
 * default; fed like the three monitors above (once per chunk from the device slab's rows and their lnprob, behind them on the
 * handle's stream; mp_sampler_set_positions restarts it; the walker-sharded entry points return MP_ESTATE while it is on).
 * The reservoir is a function of the samples alone: it does not depend on how mp_sampler_run chunks its steps or on how a run was
 * split into calls, and a numpy restatement (tests/reservoir_restated.py) reproduces the held set bit for bit.
 * A sample is the position x[0 .. ndim), and the stored, untempered lnprob, of walker w of ensemble e at step t, t the sampler's
 * absolute step index (steps_done of mp_sampler_get_state before the step).  Eligible are the samples of the steps from `discard`
 * steps after the monitor was (re)started.  Every sample has the key
 *     key = (r[0] << 32) | r[1],   r = Philox4x32-10(key words seed_lo, seed_hi; counter t_lo32, t_hi32, e * n_walkers + w, 0x52455300),
 * `seed` the monitor's own.  The reservoir of size K of ensemble e holds the K eligible samples that are least in the total
 * order (key, t, w), and all of them while fewer than K were seen.  The keys are independent and identically distributed and do
 * not depend on the state, so the held set is a uniform random K-subset, without replacement, of the eligible samples.  The
 * bottom K of a union is the bottom K of the union of the parts' bottom K: reservoirs of runs with other seeds or in other
 * processes merge on the host by their keys (magprop_amd.reservoir.merge).
 *
 * mp_sampler_set_reservoir(s, size, seed, discard): size = 0 turns the monitor off and frees it (the other arguments are
 * ignored); otherwise it (re)starts empty.  MP_EINVAL: size outside 0 .. MP_RESERVOIR_MAX_ROWS, discard < 0; the monitor is then
 * off.
 * mp_sampler_get_reservoir: the held rows of one ensemble sorted by (step, walker) ascending, the first max_rows of them:
 * x[rows][ndim], lnprob, step, walker, key [rows], *n_rows the rows written, *n_seen the eligible samples so far; any output may
 * be NULL.  MP_ESTATE while the monitor is off, MP_EINVAL on max_rows < 0 or a bad ensemble.
 */
#define MP_RESERVOIR_MAX_ROWS 65536
int mp_sampler_set_reservoir(mp_sampler *s, int size, uint64_t seed, int64_t discard);   /* size 0: off */
int mp_sampler_get_reservoir(mp_sampler *s, int ensemble, int max_rows, double *x, double *lnprob, int64_t *step,
                             int32_t *walker, uint64_t *key, int *n_rows, int64_t *n_seen);

/*
 * Differential-evolution optimizer (ABI 5, additive): scipy.optimize.differential_evolution with deferred updating, without
 * the polish step, every generation one launch that builds, evaluates and judges every trial (plus one small reduction).
 * n_pops populations of popsize members each (5 <= popsize <= 1024, 1 <= n_pops <= MP_MAX_DATASETS); population p runs on
 * dataset pop_ds_id[p] (NULL: dataset 0 for all; several populations may share a dataset: multiple starts).  Member k =
 * p * popsize + i.  The bounds box lower[ndim] < upper[ndim] (finite) is in sampler coordinates.  target: 0 the log-posterior
 * of the handle, 1 the isotropic unit Gaussian (tests).  Maximises lnprob, i.e. minimises the energy E = -lnprob.
 * Generation g >= 1 of population p, member i (all from the population of generation g - 1):
 *   u_j = j-th uniform of Philox4x32-10 keyed (seed; g, p, i, 0xDE00 + j / 2): u01(r0, r1) for even j, u01(r2, r3) for odd j;
 *   F = f_lo + (f_hi - f_lo) u01(r0, r1) of Philox (seed; g, 0xFFFF, 0, 0xDEFF), once per generation (scipy's dither);
 *   a0 = pick(u_0, m), a1 = distinct from a0 by u_1, a2 = distinct from both by u_2, m = popsize - 1 (the pick rule of
 *   mp_sampler_set_moves), slot r_j = a_j + (a_j >= i): three distinct members other than i;
 *   mutant  MP_DE_BEST1BIN: x_b + F (x_r0 - x_r1), b = best member of generation g - 1;  MP_DE_RAND1BIN: x_r0 + F (x_r1 - x_r2);
 *   binomial crossover: coordinate d takes the mutant if d == pick(u_3, ndim) (scipy's fill point) or u_{4+d} < cr, else x_i;
 *   a trial coordinate outside [lower_d, upper_d] (or NaN) becomes lower_d + u_{4+ndim+d} (upper_d - lower_d).
 * All of it unfused (separately rounded products and sums).  Greedy decision: the trial replaces member i iff
 * lnprob(trial) >= lnprob(member) (scipy's energy test <=; a NaN lnprob counts as -inf, and is stored as such).
 * After each generation the best member is the largest lnprob, lowest index on ties; the population has converged when
 * std(E) <= atol + tol |mean(E)| (population std, sums in member order: mean = (sum E) / popsize, var = (sum (E - mean)^2) /
 * popsize; a -inf lnprob means not converged).  A converged population is frozen: its members, lnprob, status, nit and nfev
 * stay as they are, and its later generations evaluate nothing.
 * Kernel build: the rule of mp_lnprob_batch for a batch of n_pops * popsize walkers, so that (shipped build) a member's lnprob is
 * bit for bit what mp_lnprob_batch returns for the same row in a batch of that size.
 * mp_optimizer_create: MP_EINVAL on bad sizes, strategy, f_lo > f_hi (or outside [0, 2)), cr outside [0, 1], tol / atol not
 * finite and >= 0, an empty or non-finite box; MP_ESTATE on multi-device handles and (target 0) handles with
 * cfg.dipole_torque = 1 or a population on an unset dataset.
 * mp_optimizer_set_population(pop[n_pops * popsize][ndim]) evaluates it (generation 0: nit = 0, nfev =
 * popsize) and clears the converged flags.  mp_optimizer_run runs up to max_generations more generations of every population
 * that has not converged, in chunks of launches with one read-back of the flags per chunk; *n_running (optional) = populations
 * still running.  mp_optimizer_get_state: any output may be NULL; pop[n_total][ndim], lnprob[n_total], status[n_total],
 * best[n_pops] (index inside the population), nit[n_pops], converged[n_pops], nfev[n_pops].
 */
#define MP_DE_BEST1BIN 0
#define MP_DE_RAND1BIN 1
typedef struct mp_optimizer mp_optimizer;
mp_optimizer *mp_optimizer_create(mp_handle *h, int popsize, int n_pops, int ndim, const int32_t *pop_ds_id, uint64_t seed,
                                  int strategy, double f_lo, double f_hi, double cr, double tol, double atol,
                                  const double *lower, const double *upper, int target);
int mp_optimizer_set_population(mp_optimizer *o, const double *pop);
int mp_optimizer_run(mp_optimizer *o, int max_generations, int *n_running);
int mp_optimizer_get_state(mp_optimizer *o, double *pop, double *lnprob, int32_t *status, int32_t *best, int32_t *nit,
                           int32_t *converged, int64_t *nfev);
int mp_optimizer_destroy(mp_optimizer *o);

/*
 * Nested sampler (ABI 5, additive): Skilling's nested sampling (2006) with batch removal (dynesty's), the dead points replaced by
 * constrained DE random walks or (slice mode) slice updates; one select and one walk launch per iteration.  n_runs independent
 * runs (1 <= n_runs <= MP_MAX_DATASETS) of nlive live points each (MP_NEST_MIN_LIVE <= N <= MP_NEST_MAX_LIVE); run r runs on
 * dataset run_ds_id[r] (NULL: dataset 0 for all; several runs may share a dataset).  Live slot j of run r is row r * N + j.  The prior is uniform
 * over the box lower[ndim] < upper[ndim] (finite; sampler coordinates).  target: 0 the log-posterior of the handle (lnL), 1 the
 * isotropic unit Gaussian -0.5 sum x^2 (tests).  A NaN lnL counts (and is stored) as -inf.
 * Iteration t of run r (t = the run's own iteration count, from 0), K = nbatch (1 <= K <= N / 2), M = N - K:
 *   order the live points by (lnL, slot); the first K die, in that order (dead k = 0 .. K-1), L* = lnL of dead K - 1;
 *   survivors s_0 < s_1 < ... < s_{M-1}: the other slots in slot order;
 *   the walk into dead slot j draws from Philox4x32-10 keyed (seed; t, r, j, 0x4E000000 + c):
 *     c = 0:          start x = live point s_{pick(u01(r0, r1), M)} (its lnL and status come with it);
 *     c = 2 s + 1:    step s's partners c1 = pick(u01(r0, r1), M), c2 = distinct from c1 by u01(r2, r3) (mp_sampler_set_moves' rule);
 *     c = 2 s + 2:    gamma = g0 (1 + s3 (2 u01(r0, r1) - 1)), s3 = sigma sqrt(3), g0 = 2.38 / sqrt(2 ndim) when given as <= 0;
 *   step s = 0 .. walks-1:  q_d = x_d + gamma (x_{s_c1, d} - x_{s_c2, d}) (unfused); accepted iff lower_d <= q_d <= upper_d for
 *   every d (a proposal outside is not evaluated) and lnL(q) > L*; then x = q.  The difference set (the survivors) is fixed
 *   during the walk: the proposal is symmetric, and this is Metropolis for the prior restricted to lnL > L*.
 *   The walk's end point, its lnL, status and accepted-step count replace dead slot j.
 * Slice mode (mp_nested_set_slice with slices > 0, from the next iteration on): the walk into dead slot j is `slices` slice
 * updates along survivor differences (ensemble slice sampling's differential direction, Karamanis & Beutler 2021, on the
 * constrained prior; Neal 2003's stepping out and shrinkage).  Start: the random walk's, c = 0 above.  Slice s = 0 .. slices-1
 * draws from Philox4x32-10 keyed (seed; t, r, j, 0x4E400000 + 0x100 s + c):
 *     c = 0:          partners c1 = pick(u01(r0, r1), M), c2 = distinct from c1 by u01(r2, r3); d = x_{s_c1} - x_{s_c2};
 *                     points on the line q(t)_d = x_d + t d_d (unfused);
 *     c = 1:          L = -(mu u01(r0, r1)), R = L + mu; of the stepping-out budget m = max_steps_out, J = floor(m u01(r2, r3))
 *                     steps go left and K = m - 1 - J right;
 *     c = 2 + i:      shrink point i = 0 .. max_shrink-1: t = L + u01(r0, r1) (R - L).
 *   Inside means lower_d <= q_d <= upper_d for every d (a point outside the box is outside and is not evaluated) and lnL(q) >
 *   L*.  Stepping out: while J > 0 and q(L) is inside, L = L - mu, J = J - 1; then while K > 0 and q(R) is inside, R = R + mu,
 *   K = K - 1.  Shrinkage: if q(t) is inside, x = q(t) (with its lnL and status) and the slice ends; otherwise L = t if t < 0,
 *   else R = t.  After max_shrink rejected points, or at once when d = 0 (coinciding survivors), the slice ends where it
 *   started and counts as failed.  A start whose lnL equals L* (a tie with dead K - 1) is not inside: its slices run as any
 *   other, a shrink point inside moves it, and a slice that finds none fails with x unchanged, as a random walk that accepts
 *   nothing.  In slice mode acc counts the walk's slices that moved, nacc the slices that moved, nzero the walks in which no
 *   slice moved; nexpand counts stepping-out steps taken, ncontract rejected shrink points, nfail failed slices.
 * Volume bookkeeping, one thread per run, dead k = 0 .. K-1 with n_k = N - k live points:
 *   lnw_k = (lnL_k + ln X) + log(-expm1(-1 / n_k));  ln X = ln X - 1 / n_k;  ln Z = logaddexp(ln Z, lnw_k)
 *   (logaddexp(x, y) = m + log1p(exp(-|x - y|)), m = max(x, y); -inf when both are), from ln X = 0, ln Z = -inf.
 * Stop rule, on the live set as it stands before an iteration (and behind every chunk of mp_nested_run): the run stops (is frozen:
 * it evaluates nothing more and keeps its full live set) when log1p(exp((lnL_max + ln X) - ln Z)) < dlogz, lnL_max the largest
 * live lnL.  The state does not depend on how mp_nested_run is split into calls.
 * Every iteration writes the dead rows (pars, lnL, n_k) of every running run; mp_nested_run reads them back behind every chunk
 * of iterations (one wait per chunk) and keeps them per run in order.  The final estimate (adding the live points, the
 * information H, the error, resampling) is the caller's (magprop_amd.nested).
 * Kernel build: the rule of mp_lnprob_batch for a batch of n_runs * nbatch walkers (the live-set evaluation: n_runs * nlive), so
 * that (shipped build) every evaluation of a walk, random-walk step or slice point, and every live point's first lnL and status are
 * bit for bit what mp_lnprob_batch returns for that row on dataset run_ds_id[r] in a batch of the launch's size.
 * mp_nested_create: MP_EINVAL on bad sizes (ndim < 6 for target 0, walks outside 1 .. MP_NEST_MAX_WALKS), g0 > 0 not finite,
 * sigma outside [0, 1/sqrt(3)), dlogz not finite and > 0, an empty or non-finite box; MP_ESTATE on multi-device handles and
 * (target 0) handles with cfg.dipole_torque = 1 or a run on an unset dataset.  mp_nested_set_live(live[n_runs * nlive][ndim], inside
 * the box) evaluates the live set and resets every run (no dead rows, ln X = 0, ln Z = -inf, counters 0).  mp_nested_run runs up
 * to max_iterations more iterations of every run not yet stopped; *n_running (optional) = runs still running.
 * mp_nested_get_dead(run): *n_rows = the run's dead rows so far; the first min(max_rows, *n_rows) are copied into pars[][ndim],
 * lnl[], n_live[] (each may be NULL).  mp_nested_get_state: any output may be NULL; live[n_runs * nlive][ndim], lnl, status,
 * acc (accepted steps of the walk that put the point there; 0 for the caller's points) [n_runs * nlive]; per run: nit, stopped,
 * lnx, lnz, ncall (evaluations inside walks), nacc (accepted steps), nzero (walks that accepted nothing).
 * mp_nested_set_slice(slices, mu, max_steps_out, max_shrink): slices = 0 restores the random walk; may be called between runs
 * (the state depends on the iteration it was called before, not on how mp_nested_run is split).  MP_EINVAL: NULL sampler, slices
 * outside 0 .. MP_NEST_MAX_SLICES, mu not finite and > 0, max_steps_out outside 1 .. MP_NEST_MAX_STEPS_OUT, max_shrink outside 1 ..
 * MP_NEST_MAX_SHRINK (the counters c = 2 + i stay below 0x100).  mp_nested_get_slice_stats: per run since mp_nested_set_live,
 * nexpand, ncontract, nfail [n_runs] (each may be NULL; 0 while only random walks ran); MP_ESTATE before mp_nested_set_live.
 */
#define MP_NEST_MIN_LIVE 16
#define MP_NEST_MAX_LIVE 4096
#define MP_NEST_MAX_WALKS 4096
#define MP_NEST_MAX_SLICES 4096
#define MP_NEST_MAX_STEPS_OUT 4096
#define MP_NEST_MAX_SHRINK 254
typedef struct mp_nested mp_nested;
mp_nested *mp_nested_create(mp_handle *h, int nlive, int nbatch, int n_runs, int ndim, const int32_t *run_ds_id, uint64_t seed,
                            int walks, double g0, double sigma, double dlogz, const double *lower, const double *upper, int target);
int mp_nested_set_live(mp_nested *ns, const double *live);
int mp_nested_run(mp_nested *ns, int max_iterations, int *n_running);
int mp_nested_get_dead(mp_nested *ns, int run, int64_t max_rows, double *pars, double *lnl, int32_t *n_live, int64_t *n_rows);
int mp_nested_get_state(mp_nested *ns, double *live, double *lnl, int32_t *status, int32_t *acc, int32_t *nit, int32_t *stopped,
                        double *lnx, double *lnz, int64_t *ncall, int64_t *nacc, int64_t *nzero);
int mp_nested_set_slice(mp_nested *ns, int slices, double mu, int max_steps_out, int max_shrink);
int mp_nested_get_slice_stats(mp_nested *ns, int64_t *nexpand, int64_t *ncontract, int64_t *nfail);
int mp_nested_destroy(mp_nested *ns);

/*
 * Nelder-Mead simplex search (ABI 5, additive): scipy.optimize.minimize(method="Nelder-Mead", bounds=...), its iterate sequence
 * exactly, for n_simplex simplexes at once (1 <= n_simplex <= 1024); simplex s runs on dataset simplex_ds_id[s] (NULL: dataset 0
 * for all; several simplexes may share a dataset: multiple starts).  N = ndim; a simplex is N + 1 vertices v_0 .. v_N sorted by
 * f = -lnprob ascending (v_0 the best).  The bounds box lower[ndim] < upper[ndim] (finite) is in sampler coordinates.  target: 0
 * the log-posterior of the handle, 1 the isotropic unit Gaussian G(x) = -0.5 sum x^2 (lnp = lnp - (0.5 x_d) x_d in index order),
 * 2 the terraced Gaussian G(x) - 1e-3 floor(37 x_0), whose plateaus and ties make every branch below occur (1 and 2: tests).
 * A NaN lnprob counts (and is stored) as -inf.
 * An iteration of the serial algorithm asks for 1 or 2 points, or N + 2 on a shrink, each after the last; all N + 4 it may ask
 * for depend on the sorted simplex alone, so one launch evaluates them all (one workgroup per simplex and candidate) and a small
 * launch behind it takes scipy's decisions.  Candidate c of a simplex, with xbar = ((v_0 + v_1) + ... + v_{N-1}) / N in vertex
 * order and clip(x) = min(max(x, lower), upper) per coordinate:
 *   c = 0  reflection           clip((1 + rho) xbar - rho v_N)
 *   c = 1  expansion            clip((1 + rho chi) xbar - rho chi v_N)
 *   c = 2  outside contraction  clip((1 + psi rho) xbar - psi rho v_N)
 *   c = 3  inside contraction   clip((1 - psi) xbar + psi v_N)
 *   c = 4 + (j - 1)             the shrink of vertex j = 1 .. N: clip(v_0 + sigma (v_j - v_0))
 * All of it unfused (separately rounded products, sums and the division); the coefficients 1 + rho, rho chi, 1 + rho chi, psi rho,
 * 1 + psi rho and 1 - psi are formed once, each operation rounded on its own.  The decision, fr, fe, fo, fi the values of c = 0 .. 3:
 *   fr < f_0:           v_N = the expansion if fe < fr, else the reflection;
 *   else fr < f_{N-1}:  v_N = the reflection;
 *   else fr < f_N:      v_N = the outside contraction if fo <= fr, else shrink;
 *   else:               v_N = the inside contraction if fi < f_N, else shrink;
 *   shrink: v_j = candidate 4 + (j - 1) for j = 1 .. N.
 * Then the vertices are sorted by f, stably (equal values keep their order, the replaced vertex having sat last), nit += 1, one
 * of the outcome counters (reflect, expand, outside, inside, shrink) += 1, and nfev grows by what the serial algorithm would have
 * evaluated: 1 for a reflection taken without trying the expansion (the second line), 2 for every other outcome but a shrink,
 * N + 2 for a shrink.  A simplex stops -- scipy's test at the top of its loop, made here on the sorted simplex for the next
 * iteration -- when |v_j[d] - v_0[d]| <= xatol for every j, d and |f_0 - f_j| <= fatol for every j: every term has to pass, so a
 * NaN difference (inf - inf) means go on.  A stopped simplex is frozen: its vertices, lnprob, status and counters stay as they
 * are, and its later iterations evaluate nothing.  There is no maxfev: the budget is the iteration count alone.
 * Kernel build: the rule of mp_lnprob_batch for a batch of n_simplex * (N + 4) walkers, the initial evaluation included, so that
 * (shipped build) every stored lnprob is bit for bit what mp_lnprob_batch returns for the same row in a batch of that size.
 * mp_simplex_create: MP_EINVAL on bad sizes (ndim outside 1 .. MP_MAX_NDIM, < 6 for target 0), rho, chi, psi or sigma not finite
 * and > 0, psi or sigma >= 1, xatol / fatol not finite and >= 0, an empty or non-finite box; MP_ESTATE on multi-device handles
 * and (target 0) handles with cfg.dipole_torque = 1 or a simplex on an unset dataset.  mp_simplex_set_vertices(sim[n_simplex][N + 1][N])
 * refuses non-finite coordinates (MP_EINVAL), applies scipy's rule to vertices outside the box (a coordinate above upper becomes
 * 2 upper - it, then everything is clipped), evaluates the vertices and sorts them (nit = 1 as scipy counts, nfev = N + 1) and
 * clears the flags and counters.  mp_simplex_run runs up to max_iterations more iterations of every simplex that has not
 * stopped, in chunks of launches with one read-back of the flags per chunk; the state does not depend on how a run is split
 * into calls; *n_running (optional) = simplexes still running.  mp_simplex_get_state: any output may be NULL;
 * sim[n_simplex][N + 1][N], lnprob[n_simplex][N + 1], status[n_simplex][N + 1], nit, stopped, nfev [n_simplex],
 * outcomes[n_simplex][5] in the order above.  The object behind the void pointers is an mp_simplex.
 */
typedef struct mp_simplex mp_simplex;
void *mp_simplex_create(mp_handle *h, int n_simplex, int ndim, const int32_t *simplex_ds_id, double rho, double chi, double psi,
                        double sigma, double xatol, double fatol, const double *lower, const double *upper, int target);
int mp_simplex_set_vertices(void *s, const double *sim);
int mp_simplex_run(void *s, int max_iterations, int *n_running);
int mp_simplex_get_state(void *s, double *sim, double *lnprob, int32_t *status, int32_t *nit, int32_t *stopped, int64_t *nfev,
                         int64_t *outcomes);
int mp_simplex_destroy(void *s);

/*
 * Tempered sequential Monte Carlo (ABI 5, additive): SMC over the path prior x L^beta, beta from 0 to 1 (Del Moral, Doucet &
 * Jasra 2006), every next beta chosen from the particles' own weights, so that no temperature ladder is given; one stage and one
 * move launch per stage.  The run ends with ln Z and N equally weighted posterior samples.  n_runs independent runs (1 <= n_runs
 * <= MP_MAX_DATASETS) of N = n_particles each (MP_SMC_MIN_PARTICLES <= N <= MP_SMC_MAX_PARTICLES); run r runs on dataset
 * run_ds_id[r] (NULL: dataset 0 for all; several runs may share a dataset) and differs from the others by r in the Philox key
 * alone.  Particle j of run r is row r * N + j.  The prior is uniform over the box lower[ndim] < upper[ndim] (finite; sampler
 * coordinates).  target: 0 the log-posterior of the handle (lnl), 1 the isotropic unit Gaussian -0.5 sum x^2, 2 the same on
 * terraces along x_0 (1 and 2: tests).  A NaN lnl counts (and is stored) as -inf.  A run keeps x[N][ndim], the untempered lnl[N],
 * beta, ln Z, its stage count and a status (MP_SMC_RUNNING, _DONE, _FAILED, _STAGE_LIMIT); two particle buffers alternate from
 * stage to stage: a stage reads one and its moves write the other.
 * Start (mp_smc_set_particles): the caller's particles (inside the box) are evaluated as they are; beta = 0, ln Z = 0.
 * Stage t (t = the run's own stage count, from 0) of run r, one workgroup:
 *   M = the largest finite lnl, n_fin = the number of finite lnl; n_fin = 0: the run ends with status MP_SMC_FAILED;
 *   w_i(d) = exp(d (lnl_i - M)) (the product rounded on its own), 0 where lnl_i is not finite;
 *   ESS(d) = (sum w)^2 / sum w^2, the square and the quotient rounded on their own; the sums: thread k of 256 adds its particles
 *   k, k + 256, ... in that order, the threads' sums combine in the order of mp_wg.h (xor butterfly over 32, 16, .. 1 inside a
 *   wavefront, then the four wavefronts in order);
 *   the target is ess * n_fin; if ESS(1 - beta) >= target then d = 1 - beta and the new beta is exactly 1.0; otherwise bisect
 *   with lo = 0, hi = 1 - beta, mid = 0.5 (lo + hi): ESS(mid) >= target moves lo to mid, else hi; stop when mid equals lo or hi,
 *   or after 128 halvings; d = lo if lo > 0, else hi; the new beta is beta + d;
 *   ln Z += d M + log(sum w / N): N counts every particle, failed ones included, so that the first stage carries ln f_valid;
 *   integer weights u_i = rint((2^31 w_i) / max w) (mp_band_weight_units' idea: their sums are exact and order-free),
 *   U = sum u_i, C_i = u_0 + ... + u_i;
 *   systematic resampling in integers: s = floor(u01(r0, r1) * U), one separately rounded product, from Philox4x32-10 keyed
 *   (seed; t, r, 0, 0x534D0000); P_j = floor((j U + s) / N) in 64 bits (j U < 2^59); the ancestor anc[j] of slot j is the least
 *   i with C_i > P_j.  A particle of zero units, every failed one among them, is nobody's ancestor.
 *   The stage's row of the log is (beta, d, ESS(d), ln Z); a run keeps MP_SMC_MAX_STAGES rows, and one that would need another
 *   ends with status MP_SMC_STAGE_LIMIT.
 * Moves of stage t, one workgroup per slot j: the slot starts at x = particle anc[j] of the stage's buffer (its lnl and status
 * come with it) and takes `walks` Metropolis steps against prior x L^beta, beta the stage's new one.  Step s = 0 .. walks-1
 * draws u from Philox4x32-10 keyed (seed; t, r, j, 0x534D0000 + 2 s + 1) and v from (..., 0x534D0000 + 2 s + 2):
 *   partners c1 = pick(u01(u0, u1), N), c2 = distinct from c1 by u01(u2, u3) (mp_sampler_set_moves' rule);
 *   gamma = g0 (1 + s3 (2 u01(v0, v1) - 1)), s3 = sigma sqrt(3), g0 = 2.38 / sqrt(2 ndim) when given as <= 0;
 *   q_d = x_d + gamma (y_d - z_d), y = particle anc[c1], z = particle anc[c2] of the stage's buffer (unfused): the differences
 *   are drawn over the resampled population;
 *   a q outside the box is rejected without an evaluation; otherwise q is accepted iff
 *   beta lnl(q) - beta lnl(x) > log(u01(v2, v3)), the two products rounded on their own.
 *   The end point, its lnl, status and accepted-step count go to slot j of the other buffer.  The resampled population is fixed
 *   during the launch, so the proposal is symmetric and does not depend on the moving particle's path: this is Metropolis for
 *   prior x L^beta.  A run whose beta reached 1 makes the moves of that stage and has status MP_SMC_DONE; a stopped run's
 *   workgroups return at once.
 * Kernel build: the rule of mp_lnprob_batch for a batch of n_runs * N walkers, so that (shipped build) every evaluation is bit for
 * bit what mp_lnprob_batch returns for that row on dataset run_ds_id[r] in a batch of the launch's size.
 * mp_smc_create: MP_EINVAL on bad sizes (N, n_runs, ndim < 6 for target 0, walks outside 1 .. MP_SMC_MAX_WALKS), ess outside
 * (0, 1), g0 not finite, sigma outside [0, 1/sqrt(3)), an empty or non-finite box; MP_ESTATE on multi-device handles and (target
 * 0) handles with cfg.dipole_torque = 1 or a run on an unset dataset.  mp_smc_run runs up to max_stages more stages of every run still
 * running, enqueued without a wait in between but for one look at the status per chunk; the state does not depend on how a run is
 * split into calls; *n_running (optional) = runs still running.  mp_smc_get_state: any output may be NULL; x[n_runs * N][ndim],
 * lnl, status, acc (accepted steps of the slot's last move) [n_runs * N]; per run beta, lnz, nstage, run_status, ncall
 * (evaluations, those of mp_smc_set_particles included), nacc (accepted steps), nfail (evaluations whose model failed).
 * mp_smc_get_stages(run): *n_rows = the run's stages so far; the first min(max_rows, *n_rows) rows of the log go to beta[], d[],
 * ess[], lnz[], accept[] (accepted steps of the stage's moves / (N walks)) and ncall[] (their evaluations), each may be NULL.
 * mp_smc_get_ancestors: anc[n_runs * N] of every run's last stage (a diagnostic of the genealogy).  The getters return MP_ESTATE
 * before mp_smc_set_particles.  The object behind the void pointers is an mp_smc.
 * Adaptive moves (mp_smc_set_adaptive, additive; off after mp_smc_create, and then every result, counter and log row above is
 * what it is without this paragraph): every run chooses the length of its moves and its scale g on the device.  The moves of
 * a stage are rounds of `walks` steps each.  Round 0 is the move launch above.  In round k >= 1 slot j continues in place from
 * its own row of the other buffer (x, lnl, status); the partners y, z are still particles anc[c1], anc[c2] of the stage's
 * buffer, which nobody writes until the next stage, so the snapshot argument above holds for every round.  Step s of the
 * stage, counted across its rounds (round k: s = k walks .. (k + 1) walks - 1), draws from 0x534D0000 + 2 s + 1 and + 2 s + 2;
 * walks * max_rounds <= MP_SMC_MAX_WALKS.  gamma takes the run's g in place of g0; g = g0 at mp_smc_set_particles.  acc[] of
 * a slot is its accepted steps over all rounds of the stage.
 *   Tune, behind every round, one workgroup of 256 threads per run: for every dimension d, with a_j = x_d of particle anc[j]
 *   of the stage's buffer (where slot j started) and b_j = x_d of slot j now: the sums of a and of b (thread k adds its slots
 *   k, k + 256, ... in that order, then the order of mp_wg.h, as every sum here), the means ma = sum a / N, mb = sum b / N;
 *   if min b = max b then rho_d = 1 (Sbb = 0: nothing has spread), else if min a = max a then rho_d = 0 (Saa = 0: all slots
 *   started from one point); else ha = max |a_j - ma|, hb = max |b_j - mb|, the centred values u_j = (a_j - ma) 2^-ilogb(ha),
 *   v_j = (b_j - mb) 2^-ilogb(hb) (the difference rounded, the scaling exact: it changes no correlation and keeps the squares
 *   of coordinates of any size in range), Saa = sum u^2, Sbb = sum v^2, Sab = sum u v, every product rounded on its own,
 *   rho_d = Sab / sqrt(Saa * Sbb).  rho = the largest rho_d; a NaN rho_d makes rho NaN.
 *   With r = the rounds the stage has made, this one included, the run makes another round iff r < min_rounds, or
 *   !(rho <= corr) and r < max_rounds (a NaN rho goes on up to the cap).
 *   At the round that stops: the stage's row of the tuning log is (r, the g its moves used, rho);
 *   share = A / (N * (r walks)), A = the sum of the slots' acc (an integer), product and quotient rounded on their own;
 *   g = min(max(g * exp(gain * (share - accept_target)), g_min), g_max), every product rounded on its own, the device's exp
 *   (PyMC's rule).  gain = 0 leaves g at g0 exactly.
 *   Control is on the device: per run the rounds made in the current stage and a flag "still moving", both reset by the
 *   stage; the launches of round k (move, tune) act on the runs that are still moving and have made k rounds, the workgroups
 *   of every other run return at once.  The host enqueues, per stage, the stage and then max_rounds times (move, tune)
 *   without a look.  A run that is MP_SMC_DONE still makes and tunes the rounds of its last stage.
 * mp_smc_set_adaptive: between mp_smc_create and mp_smc_set_particles (MP_ESTATE after it).  max_rounds = 0 turns adaptation
 * off and reads no other argument.  MP_EINVAL: min_rounds outside 1 .. max_rounds, walks * max_rounds > MP_SMC_MAX_WALKS,
 * corr outside [0, 1), gain negative or not finite, accept_target outside (0, 1), g_min or g_max (<= 0: g0 / 16 and 4 g0) not
 * finite or not g_min <= g0 <= g_max.  mp_smc_get_stages: accept[] divides by N times the steps the stage made, r walks.
 * mp_smc_get_tuning(run): like mp_smc_get_stages, one row per stage made, to rounds[], g[] and rho[], each may be NULL;
 * without adaptation the rows are (1, g0, NaN).
 */
#define MP_SMC_MIN_PARTICLES 4
#define MP_SMC_MAX_PARTICLES 16384
#define MP_SMC_MAX_WALKS 4096
#define MP_SMC_MAX_STAGES 1024
#define MP_SMC_RUNNING 0
#define MP_SMC_DONE 1
#define MP_SMC_FAILED 2
#define MP_SMC_STAGE_LIMIT 3
typedef struct mp_smc mp_smc;
void *mp_smc_create(mp_handle *h, int n_particles, int n_runs, int ndim, const int32_t *run_ds_id, uint64_t seed,
                    const double *lower, const double *upper, double ess, int walks, double g0, double sigma, int target);
int mp_smc_set_particles(void *s, const double *particles);
int mp_smc_run(void *s, int max_stages, int *n_running);
int mp_smc_get_state(void *s, double *x, double *lnl, int32_t *status, int32_t *acc, double *beta, double *lnz, int32_t *nstage,
                     int32_t *run_status, int64_t *ncall, int64_t *nacc, int64_t *nfail);
int mp_smc_get_stages(void *s, int run, int max_rows, double *beta, double *d, double *ess, double *lnz, double *accept,
                      int64_t *ncall, int *n_rows);
int mp_smc_get_ancestors(void *s, int32_t *anc);
int mp_smc_set_adaptive(void *s, int min_rounds, int max_rounds, double corr, double gain, double accept_target,
                        double g_min, double g_max);
int mp_smc_get_tuning(void *s, int run, int max_rows, int32_t *rounds, double *g, double *rho, int *n_rows);
int mp_smc_destroy(void *s);

/*
 * Bridge-sampling evidence (ABI 5, additive): ln Z from the samples of an ordinary, untempered run and their lnprob (Meng & Wong
 * 1996 with the optimal bridge; Gronau et al. 2017).  One call with no state.  A Gaussian N(m, L L^T) is fitted to the rows
 * x_fit[n_fit][ndim], N2 = n_draws points are drawn from it per repetition and evaluated, and a one-dimensional fixed point is
 * iterated over the log-ratios of the N1 = n_est rows x_est (with their lnprob lnp_est) and of the draws.  n_rep repetitions
 * (1 .. MP_BRIDGE_MAX_REP) share the proposal and the estimator rows and differ by their draws.  All rows are sampler
 * coordinates.  target as in mp_smc_create: 0 the log-posterior of the handle on dataset ds_id, 1 the isotropic unit Gaussian
 * -0.5 sum x^2, 2 the same on terraces along x_0 (1 and 2: tests; ds_id is not read).  The box lower[ndim] < upper[ndim] is the
 * support of the prior, uniform over it; NULL (both; targets 1 and 2 only): no box.  Every product, sum and difference below is
 * rounded on its own (nothing is fused); exp, log, cos, sin, sqrt are the device's unless "the host's" is said.
 * Moments (device): pivot = row 0 of x_fit.  s_a = sum_i (x_ia - pivot_a) and P_ab = sum_i (x_ia - pivot_a)(x_ib - pivot_b), b <= a,
 *   over the n_fit rows: the rows are cut into blocks of MP_BRIDGE_BLOCK consecutive rows from row 0, one workgroup per block;
 *   inside a block thread k of 256 adds its rows k, k + 256, ... in that order from 0.0, the threads' sums combine in the order
 *   of mp_wg.h (xor butterfly over 32, 16, .. 1 inside a wavefront, then the four wavefronts in order); the blocks' sums are
 *   added in block order starting from block 0's.  The sums are a function of the rows alone, not of how the call moves them
 *   to the device.  moments (optional) [ndim + ndim (ndim + 1) / 2]: s, then P with entry (a, b <= a) at ndim + a (a + 1) / 2 + b.
 * Factor (host, doubles): m_a = pivot_a + s_a / n_fit; S_ab = P_ab - (s_a s_b) / n_fit; C_ab = S_ab / (n_fit - 1); the lower
 *   Cholesky factor L by rows: for a = 0 .., for b = 0 .. a: t = C_ab - L_a0 L_b0 - ... - L_a,b-1 L_b,b-1 (subtracted in that
 *   order); L_ab = t / L_bb for b < a, L_aa = sqrt(t).  A pivot sqrt(t) that is not finite and > 0 returns MP_ERANGE and names
 *   the dimension (a constant or linearly dependent column).  c = (ln L_00 + ln L_11 + ..., added in order from 0.0) +
 *   (0.5 ndim) * 1.8378770664093453, the host's log.
 * Draws (device, one thread per draw j of repetition r, row r * n_draws + j of draws / draw_lnp / draw_lnq): pair p = 0, 1, ..
 *   of normals z_2p, z_2p+1 from the words w of Philox4x32-10 keyed (seed; j, r, p, 0x42524700) by Box-Muller (the KDE move's
 *   formula): rad = sqrt(-2 log(1 - u01(w0, w1))), ang = 6.283185307179586 u01(w2, w3), z_2p = rad cos(ang), z_2p+1 = rad sin(ang).
 *   x_a = m_a + (L_a0 z_0 + ... + L_aa z_a), the sum from 0.0 in that order; lnq = -0.5 (z_0^2 + ... , from 0.0 in order) - c.
 * Evaluation: target 0: one launch of mp_lnprob_batch_dev over the n_rep * n_draws rows, all on ds_id: every draw_lnp is bit for
 *   bit what mp_lnprob_batch returns for that row in a batch of that size.  Targets 1 and 2: point_eval's arithmetic,
 *   lnp = 0 - (0.5 x_0) x_0 - (0.5 x_1) x_1 - ... (target 2: - 1e-3 floor(37 x_0)).  b_j = lnp_j - lnq_j where the draw lies in
 *   [lower, upper] in every coordinate (no box: everywhere) and lnp_j is finite; otherwise b_j = -inf: a draw outside the
 *   support, a NaN, a failed model or a prior miss has posterior density zero.
 * Proposal density at the estimator rows (device, one thread per row): forward substitution z_a = (x_a - m_a - L_a0 z_0 - ... -
 *   L_a,a-1 z_a-1) / L_aa, subtracted in that order, then lnq by the formula above (est_lnq, optional) and a_i = lnp_est_i - lnq_i.
 * Fixed point (device, one workgroup of 256 threads per repetition).  From the host: ln s1 = log(neff / (neff + N2)), ln s2 =
 *   log(N2 / (neff + N2)), ln N1, ln N2, tau = N1 / neff, ln_volume = log(upper_0 - lower_0) + ... in order from 0.0 (no box:
 *   0), the host's log.  lse2(u, v) = max(u, v) + log(1 + exp(min(u, v) - max(u, v))).  LSE of values v: a pair (M, s) per thread
 *   from (-inf, 0), thread k takes elements k, k + 256, ... in order: a v > M makes s = s exp(M - v) + 1, M = v; any other
 *   v > -inf makes s = s + exp(v - M); -inf is skipped; the pairs merge in the order of mp_wg.h, two pairs as s = s exp(M - max)
 *   + s' exp(M' - max) (a zero s contributes 0), M = max; LSE = M + log(s).
 *   lambda_0 = LSE_j b_j - ln N2, the plain importance-sampling estimate; n_finite = the draws with b_j > -inf.  n_finite = 0:
 *   status MP_BRIDGE_NO_OVERLAP, lnz, lambda, dlnz and the four moments NaN, lambda_0 = -inf, nothing is iterated.
 *   Update t: c2 = ln s2 + lambda_t;
 *   lambda_t+1 = [LSE_j (b_j - lse2(ln s1 + b_j, c2)) - ln N2] - [LSE_i (-lse2(ln s1 + a_i, c2)) - ln N1].
 *   The loop stops with MP_BRIDGE_OK once |lambda_t+1 - lambda_t| <= tol, with MP_BRIDGE_ITER_LIMIT after max_iter updates;
 *   lambda = the last lambda_t+1.  Nothing is subtracted for stability: every term stays a logarithm, so a common offset of
 *   the lnprob of any size moves lambda by that offset and nothing else.
 *   Behind the loop f1_i = exp(-lse2((ln s1 + a_i) - lambda, ln s2)), f2_j = exp((b_j - lambda) - lse2((ln s1 + b_j) - lambda,
 *   ln s2)) (0 for b_j = -inf); mean = (sum f) / N and var = (sum (f - mean)^2) / N in a second pass, sums in the order of the
 *   moments above (thread k its elements in order, then mp_wg.h).
 *   dlnz = sqrt(var2 / (N2 (mean2 mean2)) + tau (var1 / (N1 (mean1 mean1)))): Fruehwirth-Schnatter's (2004) approximate relative
 *   mean-squared error of the bridge estimate, with the normalised spectral density of f1 at frequency zero replaced by
 *   tau = N1 / neff, the caller's integrated autocorrelation time of the estimator rows.  It leaves out the error of the
 *   proposal's fit (x_fit is taken as given) and any bias of a chain that has not converged.
 * out[n_rep][MP_BRIDGE_NOUT]: lnz = lambda - ln_volume, lambda, ln_volume, dlnz, the updates made, the status, n_finite,
 * lambda_0, mean1, var1, mean2, var2 (MP_BRIDGE_LNZ .. MP_BRIDGE_VAR2).
 * MP_EINVAL: a NULL handle, row or out pointer; target outside 0 .. 2; ndim outside 1 .. MP_MAX_NDIM or < 6 for target 0;
 * n_fit < ndim + 2, n_est < 1, n_draws < 1; n_rep outside 1 .. MP_BRIDGE_MAX_REP; n_fit, n_est or n_rep * n_draws above
 * MP_BRIDGE_MAX_ROWS; neff outside (0, n_est]; tol not finite or < 0; max_iter < 1; a NULL box for target 0 or one bound NULL;
 * an empty or non-finite box; a non-finite row of x_fit or x_est; a non-finite lnp_est; (target 0) ds_id out of range.
 * MP_ESTATE: a multi-device handle; (target 0) cfg.dipole_torque = 1 or an unset dataset.  The rows of x_fit and x_est go through
 * the device in chunks of whole blocks; the draws, a and b stay there.
 */
#define MP_BRIDGE_BLOCK 4096
#define MP_BRIDGE_MAX_REP 64
#define MP_BRIDGE_MAX_ROWS 4194304
#define MP_BRIDGE_NOUT 12
#define MP_BRIDGE_OK 0
#define MP_BRIDGE_ITER_LIMIT 1
#define MP_BRIDGE_NO_OVERLAP 2
enum { MP_BRIDGE_LNZ = 0, MP_BRIDGE_LAMBDA, MP_BRIDGE_LN_VOLUME, MP_BRIDGE_DLNZ, MP_BRIDGE_NITER, MP_BRIDGE_STATUS,
       MP_BRIDGE_NFINITE, MP_BRIDGE_LAMBDA0, MP_BRIDGE_MEAN1, MP_BRIDGE_VAR1, MP_BRIDGE_MEAN2, MP_BRIDGE_VAR2 };
int mp_bridge_logz(mp_handle *h, const double *x_fit, int64_t n_fit, const double *x_est, const double *lnp_est, int64_t n_est,
                   int ndim, int ds_id, const double *lower, const double *upper, int64_t n_draws, int n_rep, uint64_t seed,
                   double neff, int max_iter, double tol, int target, double *out, double *moments, double *draws,
                   double *draw_lnp, double *draw_lnq, double *est_lnq);

/*
 * Bridge sampling with a Student-t proposal and with Warp-III (ABI 5, additive; Meng & Schilling 2002; "warp3" of Gronau et al.'s
 * bridgesampling).  Everything mp_bridge_logz takes means here what it means there: the moments, the factor (m, L, c), the
 * counters of z, the fixed point, dlnz and the status codes are those of mp_bridge_logz, and with proposal = MP_BRIDGE_NORMAL and
 * warp = 0 every output both entries have is bit for bit mp_bridge_logz's (formed by kernels of this entry's own).  As there,
 * every product, sum and difference is rounded on its own, sums run in the order written, and exp, log, sqrt are the device's
 * unless "the host's" is said.
 * target: 0 .. 2 as in mp_bridge_logz; 3 and 4 are test targets of this entry alone.  3, the split normal: u_d = x_d for
 *   x_d < 0, else 0.25 x_d; lnp = 0 - (0.5 u_0) u_0 - (0.5 u_1) u_1 - ... (ln of its integral: ndim (ln 2.5 + 0.5 ln 2 pi)).
 *   4, the product of t_3 densities: lnp = 0 - 2 log(1 + (x_0 x_0) / 3) - 2 log(1 + (x_1 x_1) / 3) - ... (ndim ln(sqrt(3) pi / 2)).
 * proposal = MP_BRIDGE_STUDENT: the multivariate t with nu (3 .. MP_BRIDGE_MAX_NU, read for this proposal only) degrees of
 *   freedom and the covariance L L^T.  Host (doubles; the host's sqrt, log, lgamma): k = sqrt((nu - 2) / nu); L_t,ab = k L_ab;
 *   c_t = ((ln L_t,00 + ln L_t,11 + ..., in order from 0.0) + (0.5 ndim) log(nu 3.141592653589793)) + lgamma(nu / 2) -
 *   lgamma((nu + ndim) / 2); h = 0.5 (nu + ndim).
 *   Draw (device, one thread per draw): z as in mp_bridge_logz.  Pairs p = 0 .. ceil(nu / 2) - 1 of normals g_2p, g_2p+1 by the
 *   same Box-Muller formula from Philox4x32-10 keyed (seed; j, r, p, 0x42524701); w = g_0 g_0 + g_1 g_1 + ... + g_nu-1 g_nu-1 in
 *   order from 0.0 (an odd nu leaves the second normal of its last pair unused); scale = sqrt(nu / w);
 *   s_a = L_t,a0 z_0 + ... + L_t,aa z_a from 0.0 in order; x_a = m_a + scale s_a; xi_a = scale z_a; Q = xi_0 xi_0 + ... from 0.0
 *   in order; lnq = (-h) log(1 + Q / nu) - c_t.  Estimator rows: xi by mp_bridge_logz's forward substitution with L_t for L,
 *   then Q and lnq by the same formula.  (MP_BRIDGE_NORMAL: x_a = m_a + s_a with L, lnq as in mp_bridge_logz.)
 * warp = 1: the posterior is replaced by its symmetrisation about m, q~(x) = (q(x) + q(2 m - x)) / 2, which either proposal,
 *   symmetric about m, covers with the lnq of the point itself.  The mirror of a draw is x'_a = m_a - scale s_a (m_a - s_a for
 *   the Gaussian), formed beside the draw from the same rounded product; the mirror of an estimator row is
 *   x'_a = m_a - (x_a - m_a).  v, v' the lnprob of a point and of its mirror: a point counts where it lies in [lower, upper] in
 *   every coordinate (no box: everywhere) and its lnprob is finite; an estimator row itself always counts (its lnp_est is
 *   finite by the checks and it is taken as the caller's sample).  t = lse2(v, v') where both count, the one that counts where
 *   one does; a_i = (t - 0.6931471805599453) - lnq_i, b_j likewise, b_j = -inf where neither the draw nor its mirror counts; no
 *   lse2 of an infinite value is formed.  warp = 0: a_i = lnp_est_i - lnq_i, b_j = lnp_j - lnq_j or -inf, as in mp_bridge_logz.
 *   n_finite counts the b_j > -inf.
 * Evaluation.  Targets 1 .. 4: the arithmetic above (1, 2: mp_bridge_logz's) at every draw and at every mirror.  Target 0,
 *   warp = 0: one launch of mp_lnprob_batch_dev over the n_rep n_draws draws.  Target 0, warp = 1: one launch over
 *   2 n_rep n_draws rows, all draws first, then all mirrors in the same order: draw_lnp and draw_mirror_lnp are bit for bit what
 *   mp_lnprob_batch returns for those rows in one batch of that size and order; the estimator rows go through the device in
 *   chunks of 64 MP_BRIDGE_BLOCK consecutive rows from row 0 (the last one shorter), and the mirrors of each chunk are one
 *   launch of mp_lnprob_batch_dev of the chunk's size: est_mirror_lnp is bit for bit mp_lnprob_batch of those rows in batches
 *   of those sizes.  The mirror arrays hold the lnprob as evaluated, whether or not the point counts.
 * Optional outputs beside mp_bridge_logz's (NULL: not wanted): a_out[n_est], b_out[n_rep n_draws], the log-ratios the fixed
 *   point reads; with warp = 1 draw_mirrors[n_rep n_draws][ndim], est_mirror_lnp[n_est], draw_mirror_lnp[n_rep n_draws] (not
 *   written with warp = 0).
 * out[n_rep][MP_BRIDGE_WARP_NOUT]: the MP_BRIDGE_NOUT columns of mp_bridge_logz in their places, then MP_BRIDGE_EST_MIRRORS, the
 *   estimator rows whose mirror counts (the same in every row), and MP_BRIDGE_DRAW_MIRRORS, the draws of the repetition whose
 *   mirror counts (both 0 with warp = 0).
 * MP_EINVAL: whatever mp_bridge_logz refuses, with target outside 0 .. 4 in place of 0 .. 2 and a NULL box allowed for targets
 * 1 .. 4; proposal outside 0 .. 1; nu outside 3 .. MP_BRIDGE_MAX_NU for MP_BRIDGE_STUDENT; warp outside 0 .. 1; with warp = 1,
 * 2 n_rep n_draws above MP_BRIDGE_MAX_ROWS.  MP_ERANGE and MP_ESTATE as in mp_bridge_logz.
 */
#define MP_BRIDGE_NORMAL 0
#define MP_BRIDGE_STUDENT 1
#define MP_BRIDGE_MAX_NU 32
#define MP_BRIDGE_WARP_NOUT 14
enum { MP_BRIDGE_EST_MIRRORS = 12, MP_BRIDGE_DRAW_MIRRORS };
int mp_bridge_logz_warp(mp_handle *h, const double *x_fit, int64_t n_fit, const double *x_est, const double *lnp_est, int64_t n_est,
                        int ndim, int ds_id, const double *lower, const double *upper, int64_t n_draws, int n_rep, uint64_t seed,
                        double neff, int max_iter, double tol, int target, int proposal, int nu, int warp, double *out,
                        double *moments, double *draws, double *draw_lnp, double *draw_lnq, double *est_lnq, double *a_out,
                        double *b_out, double *draw_mirrors, double *est_mirror_lnp, double *draw_mirror_lnp);

/* wait for everything enqueued on the handle's own stream */
int mp_synchronize(mp_handle *h);

/* introspection used by the measurement harness */
int mp_device(const mp_handle *h);
void *mp_stream(const mp_handle *h); /* the handle's own hipStream_t */
int mp_n_grid(const mp_handle *h);
/* mean Newton sweeps per tile of the most recent host-buffer batch (diagnostic) */
double mp_last_mean_sweeps(const mp_handle *h);
/* mean number of tiles solved per walker (kept or redone) in that batch: 40 / 79 with max_stride = 1 (4 / 2 steps per lane) */
double mp_last_mean_tiles(const mp_handle *h);
/* total Newton sweeps of every walker of that batch (all tiles; 0 for walkers that never started); returns the count copied */
int mp_last_sweeps(const mp_handle *h, int32_t *out, int n);
/* Diagnostics of the solver: with mp_tile_log(h, 1) every later host-buffer batch records, per walker, one word per tile it
 * solved (the first MP_TILE_LOG of them): kind (0: 1/8-interval sub-steps, 1 .. 4: steps over 1, 2, 4, 8 grid intervals) |
 * sweeps << 4 | lanes kept << 16 | why << 24 (bits: 1 a branch of the right-hand side changed inside the tile; 2 / 4 / 8 /
 * 32 the smoothness indicator exceeded stride_tol / its 64th / 2048th / 65536th; 16 lanes had not converged when the
 * sweeps were stopped; 64 the tile was given up after its second or third sweep).  mp_last_tile_log copies walker i's
 * words of the most recent batch; returns how many. */
#define MP_TILE_LOG 96
int mp_tile_log(mp_handle *h, int enable);
int mp_last_tile_log(const mp_handle *h, int walker, int32_t *out, int n);
/* tiles solved (kept or redone) by every walker of that batch; returns the count copied */
int mp_last_tiles(const mp_handle *h, int32_t *out, int n);
double mp_sweep_tol(const mp_handle *h); /* the tolerance in force (cfg.sweep_tol or the default) */
/* The solver settings in force for this handle, out[i] for i < min(n, MP_POLICY_COUNT); returns how many were written.
 * The shipped library takes them from cfg and the constants above only; the developer build
 * (`make -C magprop_amd/csrc experiments`) also reads MAGPROP_AMD_* environment overrides and says so in
 * out[MP_POLICY_EXPERIMENTS] (bench.py copies the whole vector into its JSON line). */
enum {
    MP_POLICY_MAX_STRIDE = 0,        /* grid intervals a step may span                                         */
    MP_POLICY_STRIDE_TOL,            /* smoothness bound of coarse tiles                                       */
    MP_POLICY_SWEEP_TOL,             /* end of the Newton sweeps                                               */
    MP_POLICY_EARLY_HOLD_SECONDS,    /* MP_EARLY_HOLD_SECONDS                                                  */
    MP_POLICY_K4_TOL_FACTOR,         /* stride_tol of tiles over 8 intervals, relative to stride_tol           */
    MP_POLICY_COARSE_TOL_FACTOR,     /* sweep_tol of tiles over 2, 4, 8 intervals, relative to sweep_tol       */
    MP_POLICY_COARSE_MAX_SWEEPS,     /* sweeps after which a coarse tile keeps its converged lanes             */
    MP_POLICY_FINE_MAX_SWEEPS,       /* the same for tiles over single intervals                               */
    MP_POLICY_TROUBLE_LIMIT,         /* failed coarse attempts after which stride 8 is no longer tried         */
    MP_POLICY_STOP_FACTOR,           /* MP_STOP_FACTOR: estimated next correction / sweep_tol that ends a tile  */
    MP_POLICY_FORCED_STEPS_PER_LANE, /* 0 = by batch size                                                      */
    MP_POLICY_EXPERIMENTS,           /* 1: developer build that honours MAGPROP_AMD_* environment overrides, or a build */
                                     /*    whose compile-time policy constants (the five below) were overridden with -D  */
    MP_POLICY_LIGHT_TOL,             /* correction below which the next sweep keeps the Jacobian and the weights         */
    MP_POLICY_CUT_BY_RATIO,          /* lanes behind a cut over which a fast feature's excess picks the next stride     */
    MP_POLICY_ABORT_SKIP_RATIO,      /* excess over the bound beyond which a given-up coarse tile skips a stride         */
    MP_POLICY_LOGPRED_MIN_KIND,      /* tile kinds from this one on start from the log-space extrapolation               */
    MP_POLICY_PRE_EARLY_END_FACTOR,  /* 65 536 x 100: the calm-first-tile test of the 128-step kernels' sub-stepped start */
    MP_POLICY_COUNT
};
int mp_get_policy(const mp_handle *h, double *out, int n);
int mp_n_simd(const mp_handle *h);       /* SIMDs of the handle's device: batch-size thresholds of the kernel variants */

#ifdef __cplusplus
}
#endif
#endif /* MAGPROP_AMD_H */

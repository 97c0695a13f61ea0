"""ctypes binding of include/magprop_amd.h (libmagprop_amd.so: C ABI + gfx950 kernels).

This is the stub a magprop maintainer would add next to ``magnetar/funcs.py`` to call the HIP path
(see INTEGRATION.md).  There is no CPU fallback here: if the shared library is missing or no HIP
device is visible, importing/creating raises ``MagpropAmdError`` loudly.
"""
import ctypes as C
import sys
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MAGPROP_AMD_LIB") or os.path.join(_PKG, "libmagprop_amd.so")  # override: A/B builds

MP_OK, MP_EINVAL, MP_EHIP, MP_ERANGE, MP_ENODEV, MP_ESTATE = 0, -1, -2, -3, -4, -5
STATUS_OK, STATUS_FLAG, STATUS_NONFINITE, STATUS_PRIOR, STATUS_BADDATASET, STATUS_ZEROERR = 0, 1, 2, 3, 4, 5
MAX_NDIM = 9
MAX_DATASETS = 64
BAND_MAX_SAMPLES, BAND_MAX_Q = 16384, 16                      # include/magprop_amd.h MP_BAND_*
BAND_LTOT, BAND_LPROP, BAND_LDIP = 1, 2, 4
BAND_COMPONENTS = {"Ltot": BAND_LTOT, "Lprop": BAND_LPROP, "Ldip": BAND_LDIP}
DERIVED_N = 16                                                # include/magprop_amd.h MP_DERIVED_N (columns: magprop_amd/derived.py)
POINTWISE_N, POINTWISE_MAX_SAMPLES, POINTWISE_MAX_CELLS = 12, 262144, 1 << 28   # include/magprop_amd.h MP_POINTWISE_* (columns: magprop_amd/pointwise.py)
REWEIGHT_N, REWEIGHT_MAX_ALT = 12, 64                         # include/magprop_amd.h MP_REWEIGHT_* (columns: magprop_amd/reweight.py)
SIM_MAX_ROWS, SIM_MAX_CELLS = 262144, 1 << 28                 # include/magprop_amd.h MP_SIM_*
FLOW_N, FLOW_NCURVES = 16, 10                                 # include/magprop_amd.h MP_FLOW_* (columns and curves: magprop_amd/flows.py)
# cell curves of mp_model_flows in the order of their mask bits MP_FLOW_CURVE_*
FLOW_CURVES = ("Rm", "Rc", "Rlc", "fastness", "Mdot_prop", "Mdot_acc", "Mdot_fb", "N_acc", "N_dip", "branch")
DE_BEST1BIN, DE_RAND1BIN = 0, 1                               # include/magprop_amd.h MP_DE_*
NEST_MIN_LIVE, NEST_MAX_LIVE, NEST_MAX_WALKS = 16, 4096, 4096  # include/magprop_amd.h MP_NEST_*
NEST_MAX_SLICES, NEST_MAX_STEPS_OUT, NEST_MAX_SHRINK = 4096, 4096, 254
SMC_MIN_PARTICLES, SMC_MAX_PARTICLES, SMC_MAX_WALKS, SMC_MAX_STAGES = 4, 16384, 4096, 1024   # include/magprop_amd.h MP_SMC_*
SMC_RUNNING, SMC_DONE, SMC_FAILED, SMC_STAGE_LIMIT = 0, 1, 2, 3
MOVE_SLICE, SLICE_MAX_SHRINK = 4, 252                         # include/magprop_amd.h MP_MOVE_SLICE, MP_SLICE_MAX_SHRINK
MOVE_GAUSSIAN, MOVE_WALK, WALK_MAX_S = 5, 6, 64               # include/magprop_amd.h MP_MOVE_GAUSSIAN, MP_MOVE_WALK, MP_WALK_MAX_S
GAUSS_MODES = {"vector": 0, "random": 1, "sequential": 2}    # include/magprop_amd.h MP_GAUSS_*
ACF_MAX_LAG, ACF_MAX_BYTES = 4096, 8 << 30                   # include/magprop_amd.h MP_ACF_*
POST_MAX_BINS, POST_MAX_BINS2, POST_MAX_BYTES = 4096, 128, 1 << 30   # include/magprop_amd.h MP_POST_*
LADDER_MAX_HISTORY_BYTES = 1 << 28                           # include/magprop_amd.h MP_LADDER_MAX_HISTORY_BYTES
RESERVOIR_MAX_ROWS = 65536                                   # include/magprop_amd.h MP_RESERVOIR_MAX_ROWS
BRIDGE_BLOCK, BRIDGE_MAX_REP, BRIDGE_MAX_ROWS, BRIDGE_NOUT = 4096, 64, 1 << 22, 12   # include/magprop_amd.h MP_BRIDGE_*
BRIDGE_OK, BRIDGE_ITER_LIMIT, BRIDGE_NO_OVERLAP = 0, 1, 2
# columns of mp_bridge_logz's out rows, in the order of MP_BRIDGE_LNZ .. MP_BRIDGE_VAR2
BRIDGE_COLUMNS = ("lnz", "lambda", "ln_volume", "dlnz", "niter", "status", "n_finite", "lambda0", "mean1", "var1", "mean2", "var2")
BRIDGE_NORMAL, BRIDGE_STUDENT, BRIDGE_MAX_NU, BRIDGE_WARP_NOUT = 0, 1, 32, 14   # include/magprop_amd.h mp_bridge_logz_warp
BRIDGE_PROPOSALS = {"normal": BRIDGE_NORMAL, "t": BRIDGE_STUDENT}
# columns of mp_bridge_logz_warp's out rows: mp_bridge_logz's, then MP_BRIDGE_EST_MIRRORS and MP_BRIDGE_DRAW_MIRRORS
BRIDGE_WARP_COLUMNS = BRIDGE_COLUMNS + ("est_mirrors", "draw_mirrors")

ABI_VERSION = 5
# order of mp_get_policy()'s vector (include/magprop_amd.h MP_POLICY_*)
POLICY_FIELDS = ("max_stride", "stride_tol", "sweep_tol", "early_hold_seconds", "k4_tol_factor", "coarse_tol_factor",
                 "coarse_max_sweeps", "fine_max_sweeps", "trouble_limit", "stop_factor", "forced_steps_per_lane", "experiments_build",
                 "light_tol", "cut_by_ratio", "abort_skip_ratio", "logpred_min_kind", "pre_early_end_factor")


class MagpropAmdError(RuntimeError):
    pass


class ModelCfg(C.Structure):
    """mp_model_cfg (include/magprop_amd.h)."""
    _fields_ = [(n, C.c_double) for n in (
        "inertia_factor", "rm_massflow_factor", "n_ode", "n_lum", "alpha", "cs7", "k",
        "dipeff", "propeff", "f_beam", "nacc_lum_threshold")] + [
        ("lprop_gm_term", C.c_int32), ("max_stride", C.c_int32), ("sweep_tol", C.c_double), ("stride_tol", C.c_double),
        ("dipole_torque", C.c_int32), ("reserved", C.c_int32)]


_i, _u32, _i64, _u64, _d = C.c_int, C.c_uint32, C.c_int64, C.c_uint64, C.c_double
_vp, _dp, _ip, _i64p, _cfgp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(ModelCfg)
_u32p, _u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
# name -> (restype, argtypes) of every function of include/magprop_amd.h, in header order (tests/test_capi_cpu.py holds the two
# together).  Handles, samplers, optimizers, nested samplers and streams are c_void_p; so are the host pointers of
# mp_lnprob_batch, passed as integers (the hot entry), and the device pointers.
SIGNATURES = {
    "mp_abi_version": (_i, []),
    "mp_last_error": (C.c_char_p, []),
    "mp_cfg_synth": (None, [_cfgp]),
    "mp_cfg_lib": (None, [_cfgp]),
    "mp_create": (_vp, [_cfgp, _dp, _i, _i]),
    "mp_destroy": (_i, [_vp]),
    "mp_create_multi": (_vp, [_cfgp, _dp, _i, _ip, _i]),
    "mp_n_devices": (_i, [_vp]),
    "mp_set_dataset": (_i, [_vp, _i, _dp, _dp, _dp, _i]),
    "mp_set_prior": (_i, [_vp, _dp, _dp, _i, _u32]),
    "mp_lnprob_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "mp_lnprob_batch_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "mp_model_lc": (_i, [_vp, _dp, _i, _dp, _dp, _ip]),
    "mp_rhs_batch": (_i, [_vp, _dp, _i, _dp, _dp, _i, _dp, _dp]),
    "mp_model_band": (_i, [_vp, _dp, _i, _i, _i, _dp, _i, _u32, _dp, _ip, _ip]),
    "mp_band_weight_units": (_i, [_dp, _i, _u32p]),
    "mp_model_band_weighted": (_i, [_vp, _dp, _i, _i, _i, _dp, _dp, _i, _u32, _dp, _ip, _ip]),
    "mp_model_derived": (_i, [_vp, _dp, _i64, _i, _i, _dp, _ip, _i64p]),
    "mp_pointwise_tail_len": (_i, [_i64]),
    "mp_model_pointwise": (_i, [_vp, _dp, _i64, _i, _i, _i, _dp, _dp, _dp, _ip, _i64p]),
    "mp_model_reweight": (_i, [_vp, _dp, _i64, _i, _i, _i, _i, _ip, _dp, _dp, _dp, _dp, _dp, _ip, _i64p]),
    "mp_simulate": (_i, [_vp, _dp, _i64, _i, _i, _dp, _i, _i64, _dp, _d, _u64, _dp, _dp, _dp, _dp, _ip, _i64p]),
    "mp_model_flows": (_i, [_vp, _dp, _i64, _i, _i, _dp, _u32, _dp, _ip, _i64p]),
    "mp_model_flow_band": (_i, [_vp, _dp, _i, _i, _i, _dp, _dp, _i, _u32, _dp, _ip, _ip]),
    "mp_sampler_create": (_vp, [_vp, _i, _i, _i, _ip, _u64, _d, _i]),
    "mp_sampler_destroy": (_i, [_vp]),
    "mp_sampler_set_positions": (_i, [_vp, _dp]),
    "mp_sampler_run": (_i, [_vp, _i, _dp, _dp]),
    "mp_sampler_set_whole_step": (_i, [_vp, _i]),
    "mp_sampler_get_state": (_i, [_vp, _dp, _dp, _i64p, _i64p]),
    "mp_sampler_set_temperatures": (_i, [_vp, _i, _dp]),
    "mp_sampler_get_swaps": (_i, [_vp, _i64p]),
    "mp_sampler_set_ladder_adaptation": (_i, [_vp, _i64, _d, _d, _i]),
    "mp_sampler_get_temperatures": (_i, [_vp, _dp, _i64p, _i64p]),
    "mp_sampler_get_ladder_history": (_i, [_vp, _i, _i64, _i64, _dp, _i64p]),
    "mp_sampler_set_moves": (_i, [_vp, _i, _ip, _dp, _dp]),
    "mp_sampler_set_slice_limits": (_i, [_vp, _i, _i]),
    "mp_sampler_get_slice": (_i, [_vp, _dp, _i64p, _i64p, _i64p, _i64p, _i64p]),
    "mp_sampler_set_gaussian": (_i, [_vp, _dp, _i, _d]),
    "mp_sampler_get_gaussian": (_i, [_vp, _dp, _i64p, _i64p, _i64p]),
    "mp_sampler_get_bad": (_i, [_vp, _i64, _dp, _i, _i64p, _i64p]),
    "mp_sampler_n_slots": (_i, [_vp]),
    "mp_sampler_row_doubles": (_i, [_vp]),
    "mp_sampler_halfstep_shard": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "mp_sampler_halfstep_apply": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "mp_sampler_step_blocks": (_i, [_vp]),
    "mp_sampler_step_row_doubles": (_i, [_vp]),
    "mp_sampler_step_shard": (_i, [_vp, _i, _i, _vp, _vp]),
    "mp_sampler_step_apply": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "mp_sampler_state_ptrs": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "mp_sampler_set_autocorr": (_i, [_vp, _i, _i64]),
    "mp_sampler_get_autocorr": (_i, [_vp, _d, _dp, _ip, _i64p]),
    "mp_sampler_get_acf": (_i, [_vp, _i, _i, _dp]),
    "mp_sampler_get_autocorr_sums": (_i, [_vp, _i, _dp, _dp, _dp, _dp, _dp, _i64p]),
    "mp_sampler_set_posterior": (_i, [_vp, _i, _i, _dp, _dp, _i64]),
    "mp_sampler_get_posterior_hist1": (_i, [_vp, _i, _i64p, _i64p, _i64p, _i64p, _i64p]),
    "mp_sampler_get_posterior_hist2": (_i, [_vp, _i, _i64p, _i64p]),
    "mp_sampler_get_posterior_moments": (_i, [_vp, _i, _dp, _dp, _dp, _i64p]),
    "mp_sampler_get_posterior_best": (_i, [_vp, _i, _dp, _dp, _i64p]),
    "mp_sampler_set_thermo": (_i, [_vp, _i64]),
    "mp_sampler_get_thermo": (_i, [_vp, _dp, _i64p, _i64p, _i64p]),
    "mp_sampler_set_reservoir": (_i, [_vp, _i, _u64, _i64]),
    "mp_sampler_get_reservoir": (_i, [_vp, _i, _i, _dp, _dp, _i64p, _ip, _u64p, C.POINTER(C.c_int), _i64p]),
    "mp_optimizer_create": (_vp, [_vp, _i, _i, _i, _ip, _u64, _i, _d, _d, _d, _d, _d, _dp, _dp, _i]),
    "mp_optimizer_set_population": (_i, [_vp, _dp]),
    "mp_optimizer_run": (_i, [_vp, _i, _ip]),
    "mp_optimizer_get_state": (_i, [_vp, _dp, _dp, _ip, _ip, _ip, _ip, _i64p]),
    "mp_optimizer_destroy": (_i, [_vp]),
    "mp_nested_create": (_vp, [_vp, _i, _i, _i, _i, _ip, _u64, _i, _d, _d, _d, _dp, _dp, _i]),
    "mp_nested_set_live": (_i, [_vp, _dp]),
    "mp_nested_run": (_i, [_vp, _i, _ip]),
    "mp_nested_get_dead": (_i, [_vp, _i, _i64, _dp, _dp, _ip, _i64p]),
    "mp_nested_get_state": (_i, [_vp, _dp, _dp, _ip, _ip, _ip, _ip, _dp, _dp, _i64p, _i64p, _i64p]),
    "mp_nested_set_slice": (_i, [_vp, _i, _d, _i, _i]),
    "mp_nested_get_slice_stats": (_i, [_vp, _i64p, _i64p, _i64p]),
    "mp_nested_destroy": (_i, [_vp]),
    "mp_simplex_create": (_vp, [_vp, _i, _i, _ip, _d, _d, _d, _d, _d, _d, _dp, _dp, _i]),
    "mp_simplex_set_vertices": (_i, [_vp, _dp]),
    "mp_simplex_run": (_i, [_vp, _i, _ip]),
    "mp_simplex_get_state": (_i, [_vp, _dp, _dp, _ip, _ip, _ip, _i64p, _i64p]),
    "mp_simplex_destroy": (_i, [_vp]),
    "mp_smc_create": (_vp, [_vp, _i, _i, _i, _ip, _u64, _dp, _dp, _d, _i, _d, _d, _i]),
    "mp_smc_set_particles": (_i, [_vp, _dp]),
    "mp_smc_run": (_i, [_vp, _i, _ip]),
    "mp_smc_get_state": (_i, [_vp, _dp, _dp, _ip, _ip, _dp, _dp, _ip, _ip, _i64p, _i64p, _i64p]),
    "mp_smc_get_stages": (_i, [_vp, _i, _i, _dp, _dp, _dp, _dp, _dp, _i64p, _ip]),
    "mp_smc_get_ancestors": (_i, [_vp, _ip]),
    "mp_smc_set_adaptive": (_i, [_vp, _i, _i, _d, _d, _d, _d, _d]),
    "mp_smc_get_tuning": (_i, [_vp, _i, _i, _ip, _dp, _dp, _ip]),
    "mp_smc_destroy": (_i, [_vp]),
    "mp_bridge_logz": (_i, [_vp, _dp, _i64, _dp, _dp, _i64, _i, _i, _dp, _dp, _i64, _i, _u64, _d, _i, _d, _i, _dp, _dp, _dp, _dp, _dp, _dp]),
    "mp_bridge_logz_warp": (_i, [_vp, _dp, _i64, _dp, _dp, _i64, _i, _i, _dp, _dp, _i64, _i, _u64, _d, _i, _d, _i, _i, _i, _i, _dp, _dp, _dp,
                                 _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "mp_synchronize": (_i, [_vp]),
    "mp_device": (_i, [_vp]),
    "mp_stream": (_vp, [_vp]),
    "mp_n_grid": (_i, [_vp]),
    "mp_last_mean_sweeps": (_d, [_vp]),
    "mp_last_mean_tiles": (_d, [_vp]),
    "mp_last_sweeps": (_i, [_vp, _ip, _i]),
    "mp_tile_log": (_i, [_vp, _i]),
    "mp_last_tile_log": (_i, [_vp, _i, _ip, _i]),
    "mp_last_tiles": (_i, [_vp, _ip, _i]),
    "mp_sweep_tol": (_d, [_vp]),
    "mp_get_policy": (_i, [_vp, _dp, _i]),
    "mp_n_simd": (_i, [_vp]),
}
EXPORTS = tuple(SIGNATURES)


def build(force=False, verbose=False):
    """Compile the HIP library in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    src = os.path.join(_PKG, "csrc")
    args = ["make", "-C", src, "-s"] + (["-B"] if force else [])
    subprocess.check_call(args, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as the
    system one, different file name), and two HIP/HSA runtimes in one process do not work: whichever
    initialises second sees no GPU.  If torch is loaded first, the dynamic linker already resolves our
    NEEDED libamdhip64.so.7 to torch's copy.  For the other order (magprop_amd first, torch later) torch's
    copy is preloaded here, found without importing torch.  No torch, or MAGPROP_AMD_SYSTEM_HIP=1: the
    runtime under /opt/rocm is used."""
    import sys
    if "torch" in sys.modules or os.environ.get("MAGPROP_AMD_SYSTEM_HIP") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    bundled = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(bundled):
        try:
            C.CDLL(bundled, mode=C.RTLD_GLOBAL)
        except OSError:
            pass  # fall back to the system runtime (fine as long as torch is not used in this process)


def lib():
    """Load libmagprop_amd.so (building it if hipcc is available and it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        try:
            build()
        except Exception as exc:  # noqa: BLE001
            raise MagpropAmdError(
                f"{LIB_PATH} is missing and could not be built ({exc}); run `python -c 'import "
                "__graft_entry__ as g; g.build()'` on a machine with hipcc") from exc
    _share_hip_runtime_with_torch()
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as exc:
        raise MagpropAmdError(f"cannot load {LIB_PATH}: {exc}") from exc
    # the ABI check comes before any other symbol is touched: a stale build must fail with the rebuild hint, not with an
    # AttributeError on a symbol it does not have yet
    try:
        abi = L.mp_abi_version()            # (ctypes' default restype: int)
    except AttributeError:
        abi = None
    if abi != ABI_VERSION:
        raise MagpropAmdError(f"{LIB_PATH} has ABI version {abi}, this binding expects {ABI_VERSION}: "
                              "rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def last_error():
    return lib().mp_last_error().decode("utf-8", "replace")


def check(rc, what):
    if rc == MP_OK:
        return
    msg = last_error()
    if rc == MP_ERANGE:
        raise ValueError(msg)  # scipy's interp1d raises ValueError there (magnetar/funcs.py:214-215)
    if rc == MP_EINVAL:
        raise ValueError(f"{what}: {msg}")
    raise MagpropAmdError(f"{what} failed (rc={rc}): {msg}")


SWEEP_TOL_DEFAULT, SWEEP_TOL_STRICT = 1.0e-7, 1.0e-11   # include/magprop_amd.h MP_SWEEP_TOL_*
DEFAULT_SWEEP_TOL = 0.0   # what cfg_synth()/cfg_lib() put into mp_model_cfg.sweep_tol (0 = the library default); the test
                          # suite sets SWEEP_TOL_STRICT here for its kernel-vs-serial-restatement comparisons
DEFAULT_MAX_STRIDE = 0    # likewise mp_model_cfg.max_stride (0 = the library default, adaptive up to 8 grid intervals per
                          # step); the strict test mode sets 1: every grid interval a step, the scheme of the serial restatement


def cfg_synth(**kw):
    c = ModelCfg()
    lib().mp_cfg_synth(C.byref(c))
    c.sweep_tol = DEFAULT_SWEEP_TOL
    c.max_stride = DEFAULT_MAX_STRIDE
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def cfg_lib(**kw):
    c = ModelCfg()
    lib().mp_cfg_lib(C.byref(c))
    c.sweep_tol = DEFAULT_SWEEP_TOL
    c.max_stride = DEFAULT_MAX_STRIDE
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def curve_steps_per_lane(n, n_simd):
    """Steps per lane of the curve kernel (mode B: light curves to HBM) a batch of n walkers runs on: the rule of
    magprop_amd/csrc/mp_device.h kernel_spl_curves, restated for labels (bench.py) and tests (tests/test_capi_cpu.py holds the
    two together)."""
    if n <= n_simd:
        return 4
    x2 = n / (7.0 * (n_simd // 4))
    r2 = 1.62 * ((1.0 if x2 <= 1.0 else 2.0) if x2 <= 2.0 else x2 + 0.2)
    return 4 if -(-n // n_simd) <= r2 else 2


def whole_step_fits(whole_step_blocks, n_simd):
    """mp_sampler_run evaluates a whole step per launch up to this many evaluations (3/2 x the walkers of all ensembles): the
    rule of magprop_amd/csrc/mp_device.h stretch_whole_step_fits, restated for labels (tests/test_capi_cpu.py holds the two
    together)."""
    return 8 * int(whole_step_blocks) <= 19 * int(n_simd)


def band_args(q, components):
    """Validated (q as float64, component mask, component names in output order) of a band request (mp_model_band's limits)."""
    qa = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
    if qa.ndim != 1 or not 1 <= qa.size <= BAND_MAX_Q:
        raise ValueError(f"q must hold 1 to {BAND_MAX_Q} (MP_BAND_MAX_Q) quantiles, got shape {np.shape(q)}")
    if not np.all((qa >= 0.0) & (qa <= 1.0)):
        raise ValueError("every quantile in q must be finite and in [0, 1]")
    names = (components,) if isinstance(components, str) else tuple(components)
    if not names or any(c not in BAND_COMPONENTS for c in names) or len(set(names)) != len(names):
        raise ValueError(f"components must be a non-empty selection of {tuple(BAND_COMPONENTS)} without repeats, got {components!r}")
    mask = 0
    for c in names:
        mask |= BAND_COMPONENTS[c]
    return qa, mask, tuple(c for c in BAND_COMPONENTS if mask & BAND_COMPONENTS[c])


def flow_curve_args(curves, band=False):
    """(mask, names in output order) of a selection of FLOW_CURVES (a name or a sequence of names, no repeats); band=True: not
    empty and without "branch" (mp_model_flow_band's conditions)."""
    names = (curves,) if isinstance(curves, str) else tuple(curves)
    if any(c not in FLOW_CURVES for c in names) or len(set(names)) != len(names):
        raise ValueError(f"curves must be a selection of {FLOW_CURVES} without repeats, got {curves!r}")
    if band and (not names or "branch" in names):
        raise ValueError(f"a flow band takes a non-empty selection of curves without 'branch' (a flag has no quantile), got {curves!r}")
    mask = 0
    for c in names:
        mask |= 1 << FLOW_CURVES.index(c)
    return mask, tuple(c for k, c in enumerate(FLOW_CURVES) if mask >> k & 1)


def band_rows(pars, ndim=None):
    """pars as contiguous float64 rows (n, ndim), 1 <= n <= BAND_MAX_SAMPLES (mp_model_band's limit)."""
    p = np.ascontiguousarray(pars, dtype=np.float64)
    if p.ndim != 2 or (ndim is not None and p.shape[1] != ndim):
        raise ValueError(f"pars must be 2-D (n, {ndim if ndim is not None else 'ndim'}), got shape {p.shape}")
    if not 1 <= p.shape[0] <= BAND_MAX_SAMPLES:
        raise ValueError(f"a band takes 1 to {BAND_MAX_SAMPLES} (MP_BAND_MAX_SAMPLES) rows, got {p.shape[0]}: thin the chain")
    return p


def ptr(a):
    """Typed pointer to the buffer of ndarray a (double *, int32_t *, int64_t * ... by its dtype)."""
    return a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def read_back(fn, obj, spec, *lead):
    """fn(obj, *lead, out...) of an ABI getter, checked: one output per (key, shape, dtype) of spec in argument order, a new
    array of that shape and dtype (shape (): a scalar), or NULL where shape is None.  Returns {key: array} of the non-NULL ones."""
    out = {k: np.empty(shape, dtype) for k, shape, dtype in spec if shape is not None}
    check(fn(obj, *lead, *(ptr(out[k]) if k in out else None for k, _, _ in spec)), fn.__name__)
    return out


def band_weights(weights, n):
    """weights as contiguous float64 (n,), one per row of a band request: finite, >= 0 and not all zero (mp_band_weight_units'
    conditions, judged here so that the message names the argument)."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (n,):
        raise ValueError(f"weights must be of shape ({n},), one per row, got {w.shape}")
    if not np.all(np.isfinite(w)) or np.any(w < 0.0) or not np.any(w > 0.0):
        raise ValueError("weights must be finite and >= 0 with at least one > 0")
    return w


def band_weight_units(weights):
    """The integer units the weighted band gives the rows (mp_band_weight_units): floor(w / max(w) * 2^31) as uint32."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.size < 1:
        raise ValueError(f"weights must be 1-D and not empty, got shape {w.shape}")
    u = np.empty(w.size, dtype=np.uint32)
    check(lib().mp_band_weight_units(_dptr(w), int(w.size), u.ctypes.data_as(_u32p)), "mp_band_weight_units")
    return u


def kish_n_eff(weights, status):
    """Kish's effective sample size (sum w)^2 / sum w^2 over the rows that finished (0.0: none of them carries weight)."""
    w = np.asarray(weights, dtype=np.float64)[np.asarray(status) == STATUS_OK]
    s2 = float(np.sum(w * w))
    return float(np.sum(w)) ** 2 / s2 if s2 > 0.0 else 0.0


def bridge_proposal(proposal, nu=5, warp=False):
    """(proposal, nu, warp) as mp_bridge_logz_warp takes them, of proposal "normal" | "t" (or MP_BRIDGE_NORMAL | MP_BRIDGE_STUDENT),
    nu and warp, judged by the entry's own rules; nu is 0 where it is not read."""
    prop = BRIDGE_PROPOSALS.get(proposal, proposal) if isinstance(proposal, str) else proposal
    if isinstance(prop, bool) or prop not in (BRIDGE_NORMAL, BRIDGE_STUDENT):
        raise ValueError(f"proposal must be one of {tuple(BRIDGE_PROPOSALS)}, got {proposal!r}")
    if prop == BRIDGE_STUDENT and not (isinstance(nu, (int, np.integer)) and not isinstance(nu, bool) and 3 <= nu <= BRIDGE_MAX_NU):
        raise ValueError(f"nu must be an integer in 3..{BRIDGE_MAX_NU} (MP_BRIDGE_MAX_NU), got {nu!r}")
    if not isinstance(warp, (bool, np.bool_)) and warp not in (0, 1):
        raise ValueError(f"warp must be True or False, got {warp!r}")
    return int(prop), int(nu) if prop == BRIDGE_STUDENT else 0, int(bool(warp))


class _Owner:
    """close() on `with`-exit and when garbage-collected."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if sys is None or sys.is_finalizing():      # interpreter shutdown: the HIP runtime may already be gone; the OS reclaims the rest
            return
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class Driver(_Owner):
    """Owns one device-resident driver object (mp_sampler, mp_optimizer, mp_nested, mp_simplex, mp_smc) of `handle`:
    `name`_create(handle, *args), freed once by `name`_destroy.  Passed to the ABI as its pointer (NULL once closed); holds the handle, so the
    handle outlives it."""

    def __init__(self, name, handle, *args):
        L = lib()
        self.handle, self._destroy = handle, getattr(L, name + "_destroy")
        self.ptr = getattr(L, name + "_create")(handle._h, *args)
        if not self.ptr:
            raise MagpropAmdError(f"{name}_create failed: " + last_error())

    @property
    def _as_parameter_(self):
        return self.ptr

    def close(self):
        if getattr(self, "ptr", None):
            self._destroy(self.ptr)
            self.ptr = None


class Handle(_Owner):
    """Owns one mp_handle: a model configuration + time grid bound to one GPU."""

    def __init__(self, cfg, tgrid, device=-1):
        """device: a HIP device index (-1: the current one), or a sequence of indices for a multi-device handle
        (mp_create_multi: host-buffer batches are dealt out over the listed devices inside the library)."""
        self._L = lib()
        self.tgrid = np.ascontiguousarray(tgrid, dtype=np.float64)
        self.cfg = cfg
        if np.ndim(device) > 0:
            devs = np.ascontiguousarray(device, dtype=np.int32)
            self._h = self._L.mp_create_multi(C.byref(cfg), _dptr(self.tgrid), int(self.tgrid.size), _iptr(devs), int(devs.size))
        else:
            self._h = self._L.mp_create(C.byref(cfg), _dptr(self.tgrid), int(self.tgrid.size), int(device))
        if not self._h:
            raise MagpropAmdError("mp_create failed: " + last_error())

    @property
    def n_devices(self):
        return self._L.mp_n_devices(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.mp_destroy(self._h)
            self._h = None

    @property
    def device(self):
        return self._L.mp_device(self._h)

    def set_dataset(self, ds_id, x, y, yerr):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        yerr = np.ascontiguousarray(yerr, dtype=np.float64)
        if not (x.ndim == y.ndim == yerr.ndim == 1 and x.size == y.size == yerr.size):
            raise ValueError("x, y, yerr must be 1-D arrays of equal length")
        check(self._L.mp_set_dataset(self._h, int(ds_id), _dptr(x), _dptr(y), _dptr(yerr), int(x.size)),
              "mp_set_dataset")
        self.__dict__.setdefault("_ds_size", {})[int(ds_id)] = int(x.size)

    def dataset_size(self, ds_id):
        """Observations of the light curve registered under ds_id through this object (0: none)."""
        return self.__dict__.get("_ds_size", {}).get(int(ds_id), 0)

    def set_prior(self, lower, upper, log_mask=0):
        if lower is None:
            check(self._L.mp_set_prior(self._h, None, None, 0, C.c_uint32(log_mask)), "mp_set_prior")
            return
        lo = np.ascontiguousarray(lower, dtype=np.float64)
        hi = np.ascontiguousarray(upper, dtype=np.float64)
        if lo.shape != hi.shape or lo.ndim != 1:
            raise ValueError("lower/upper must be 1-D arrays of equal length")
        check(self._L.mp_set_prior(self._h, _dptr(lo), _dptr(hi), int(lo.size), C.c_uint32(log_mask)),
              "mp_set_prior")

    def lnprob_batch(self, pars, ds_id=None, want_status=False, want_ltot=False):
        p = np.ascontiguousarray(pars, dtype=np.float64)
        if p.ndim != 2:
            raise ValueError("pars must be 2-D (n_walkers, ndim)")
        n, nd = p.shape
        out = np.empty(n, dtype=np.float64)
        st = np.empty(n, dtype=np.int32)
        lt = np.empty((n, self.tgrid.size), dtype=np.float64) if want_ltot else None
        ids = None
        if ds_id is not None:
            ids = (np.full(n, ds_id, dtype=np.int32) if np.ndim(ds_id) == 0
                   else np.ascontiguousarray(np.broadcast_to(np.asarray(ds_id, dtype=np.int32), (n,))))
        rc = self._L.mp_lnprob_batch(self._h, p.ctypes.data, ids.ctypes.data if ids is not None else None, n, nd,
                                     out.ctypes.data, st.ctypes.data, lt.ctypes.data if lt is not None else None)
        if rc:
            check(rc, "mp_lnprob_batch")
        res = (out,)
        if want_status:
            res += (st,)
        if want_ltot:
            res += (lt,)
        return res if len(res) > 1 else out

    def lnprob_batch_dev(self, d_pars, n, ndim, d_lnprob, d_ds_id=0, d_status=0, d_ltot=0, stream=0):
        """Device-pointer entry (ints from e.g. torch.Tensor.data_ptr()); asynchronous on `stream`
        (a hipStream_t as int; 0 = HIP's default stream, which is also torch's default stream)."""
        check(self._L.mp_lnprob_batch_dev(self._h, C.c_void_p(d_pars), C.c_void_p(d_ds_id or None), int(n),
                                          int(ndim), C.c_void_p(d_lnprob), C.c_void_p(d_status or None),
                                          C.c_void_p(d_ltot or None), C.c_void_p(stream or None)),
              "mp_lnprob_batch_dev")

    def model_lc(self, pars, want_traj=False):
        p = np.ascontiguousarray(pars, dtype=np.float64).ravel()
        out = np.empty((4, self.tgrid.size), dtype=np.float64)
        traj = np.empty((2, self.tgrid.size), dtype=np.float64)
        st = C.c_int32(0)
        check(self._L.mp_model_lc(self._h, _dptr(p), int(p.size), _dptr(out), _dptr(traj), C.byref(st)),
              "mp_model_lc")
        return (st.value, out, traj) if want_traj else (st.value, out)

    def model_band(self, pars, q, components=("Ltot",), physical=False, weights=None):
        """Quantiles q of the model light curves of the rows of pars over the handle's grid (mp_model_band): returns
        (band[ncomp, nq, n_grid], status[n], n_used); components in the order Ltot, Lprop, Ldip whatever order they are
        named in.  physical=False: sampler coordinates under the handle's prior, as lnprob_batch takes them.  weights (n,),
        finite and >= 0: the quantiles of the weighted empirical distribution of the curves instead (mp_model_band_weighted:
        no interpolation, weights in integer units of max(weights) / 2^31)."""
        qa, mask, names = band_args(q, components)
        p = band_rows(pars)
        n, nd = p.shape
        w = None if weights is None else band_weights(weights, n)
        band = np.empty((len(names), qa.size, self.tgrid.size), dtype=np.float64)
        st = np.empty(n, dtype=np.int32)
        used = C.c_int32(0)
        if w is None:
            check(self._L.mp_model_band(self._h, _dptr(p), n, nd, int(bool(physical)), _dptr(qa), int(qa.size), C.c_uint32(mask),
                                        _dptr(band), _iptr(st), C.byref(used)), "mp_model_band")
        else:
            check(self._L.mp_model_band_weighted(self._h, _dptr(p), n, nd, int(bool(physical)), _dptr(w), _dptr(qa), int(qa.size),
                                                 C.c_uint32(mask), _dptr(band), _iptr(st), C.byref(used)), "mp_model_band_weighted")
        return band, st, int(used.value)

    def model_derived(self, pars, physical=False):
        """Energy budgets and light-curve landmarks of the models of the rows of pars (mp_model_derived; the columns are
        magprop_amd.derived.NAMES): returns (values[n, DERIVED_N], status[n], n_used), rows that did not finish all NaN.  Any
        number of rows: the library works through them in chunks.  physical=False: sampler coordinates under the handle's
        prior, as lnprob_batch takes them."""
        p = np.ascontiguousarray(pars, dtype=np.float64)
        if p.ndim != 2 or p.shape[0] < 1:
            raise ValueError(f"pars must be 2-D (n >= 1, ndim), got shape {p.shape}")
        n, nd = p.shape
        out = np.empty((n, DERIVED_N), dtype=np.float64)
        st = np.empty(n, dtype=np.int32)
        used = C.c_int64(0)
        check(self._L.mp_model_derived(self._h, _dptr(p), n, nd, int(bool(physical)), _dptr(out), _iptr(st), C.byref(used)),
              "mp_model_derived")
        return out, st, int(used.value)

    def model_flows(self, pars, curves=(), physical=False):
        """Mass budget, angular-momentum budget and propeller / accretor regime of the models of the rows of pars
        (mp_model_flows; the columns are magprop_amd.flows.NAMES): returns (values[n, FLOW_N], cells[n, ncurves, n_grid],
        status[n], n_used), rows that did not finish all NaN.  curves: names of FLOW_CURVES whose cell curves (radii, fastness,
        mass-flow rates, torques, cgs) come back too, in the order of FLOW_CURVES whatever order they are named in; none: cells
        is None.  Any number of rows: the library works through them in chunks.  physical=False: sampler coordinates under the
        handle's prior, as lnprob_batch takes them."""
        mask, names = flow_curve_args(curves)
        p = np.ascontiguousarray(pars, dtype=np.float64)
        if p.ndim != 2 or p.shape[0] < 1:
            raise ValueError(f"pars must be 2-D (n >= 1, ndim), got shape {p.shape}")
        n, nd = p.shape
        out = np.empty((n, FLOW_N), dtype=np.float64)
        cells = np.empty((n, len(names), self.tgrid.size), dtype=np.float64) if names else None
        st = np.empty(n, dtype=np.int32)
        used = C.c_int64(0)
        check(self._L.mp_model_flows(self._h, _dptr(p), n, nd, int(bool(physical)), _dptr(out), C.c_uint32(mask),
                                     _dptr(cells) if names else None, _iptr(st), C.byref(used)), "mp_model_flows")
        return out, cells, st, int(used.value)

    def model_flow_band(self, pars, q, curves=("fastness",), physical=False, weights=None):
        """Quantiles q over the rows of pars of the cell curves of model_flows at every grid point (mp_model_flow_band): returns
        (band[ncurves, nq, n_grid], status[n], n_used), curves in the order of FLOW_CURVES.  Rows, q and weights as in
        model_band; "branch" is refused."""
        qa, _, _ = band_args(q, "Ltot")
        mask, names = flow_curve_args(curves, band=True)
        p = band_rows(pars)
        n, nd = p.shape
        w = None if weights is None else band_weights(weights, n)
        band = np.empty((len(names), qa.size, self.tgrid.size), dtype=np.float64)
        st = np.empty(n, dtype=np.int32)
        used = C.c_int32(0)
        check(self._L.mp_model_flow_band(self._h, _dptr(p), n, nd, int(bool(physical)), None if w is None else _dptr(w), _dptr(qa),
                                         int(qa.size), C.c_uint32(mask), _dptr(band), _iptr(st), C.byref(used)), "mp_model_flow_band")
        return band, st, int(used.value)

    def model_pointwise(self, pars, ds_id=0, physical=False, cells=False):
        """Per-observation reductions of the pointwise log-likelihoods of the rows of pars against dataset ds_id
        (mp_model_pointwise; the columns are magprop_amd.pointwise.NAMES): returns (obs[n_obs, POINTWISE_N], tail[n_obs, T(n)],
        status[n], n_used) and, with cells=True, the matrix z[n_obs, n] of standardised residuals behind them.  Observations
        are in ascending time, as the library keeps them.  physical=False: sampler coordinates under the handle's prior, as
        lnprob_batch takes them."""
        p = np.ascontiguousarray(pars, dtype=np.float64)
        if p.ndim != 2 or p.shape[0] < 1:
            raise ValueError(f"pars must be 2-D (n >= 1, ndim), got shape {p.shape}")
        n, nd = p.shape
        n_obs = self.dataset_size(ds_id)                     # (0: never set here; the library refuses the call then)
        tlen = int(self._L.mp_pointwise_tail_len(n))
        obs = np.empty((max(n_obs, 1), POINTWISE_N), dtype=np.float64)
        tail = np.empty((max(n_obs, 1), max(tlen, 1)), dtype=np.float64)
        z = np.empty((max(n_obs, 1), n), dtype=np.float64) if cells else None
        st = np.empty(n, dtype=np.int32)
        used = C.c_int64(0)
        check(self._L.mp_model_pointwise(self._h, _dptr(p), n, nd, int(bool(physical)), int(ds_id), _dptr(obs), _dptr(tail),
                                         _dptr(z) if cells else None, _iptr(st), C.byref(used)), "mp_model_pointwise")
        res = (obs, tail[:, :tlen], st, int(used.value))
        return res + (z,) if cells else res

    def model_reweight(self, pars, kind, alt, obs_w=None, ds_id=0, physical=False):
        """Log importance weights of the rows of pars against dataset ds_id under the alternatives kind[n_alt], alt[n_alt, 3]
        (scale, jitter, nu) and the observation weights obs_w[n_alt, n_obs] (None: 1 each; observations in ascending time, as
        the library keeps them) (mp_model_reweight; the columns are magprop_amd.reweight.NAMES): returns (lw[n_alt, n],
        table[n_alt, REWEIGHT_N], tail[n_alt, T(n)], status[n], n_used), the rows that did not finish NaN in lw.
        physical=False: sampler coordinates under the handle's prior, as lnprob_batch takes them."""
        p = np.ascontiguousarray(pars, dtype=np.float64)
        if p.ndim != 2 or p.shape[0] < 1:
            raise ValueError(f"pars must be 2-D (n >= 1, ndim), got shape {p.shape}")
        n, nd = p.shape
        kd = np.ascontiguousarray(kind, dtype=np.int32)
        al = np.ascontiguousarray(alt, dtype=np.float64)
        if kd.ndim != 1 or kd.size < 1 or al.shape != (kd.size, 3):
            raise ValueError(f"kind (n_alt,) and alt (n_alt, 3) expected, got {kd.shape} and {al.shape}")
        n_alt = int(kd.size)
        n_obs = self.dataset_size(ds_id)                     # (0: never set here; the library refuses the call then)
        ow = None if obs_w is None else np.ascontiguousarray(obs_w, dtype=np.float64)
        if ow is not None and ow.shape != (n_alt, n_obs):
            raise ValueError(f"obs_w must be of shape ({n_alt}, {n_obs}), one weight per alternative and observation, got {ow.shape}")
        tlen = int(self._L.mp_pointwise_tail_len(n))
        lw = np.empty((n_alt, n), dtype=np.float64)
        table = np.empty((n_alt, REWEIGHT_N), dtype=np.float64)
        tail = np.empty((n_alt, max(tlen, 1)), dtype=np.float64)
        st = np.empty(n, dtype=np.int32)
        used = C.c_int64(0)
        check(self._L.mp_model_reweight(self._h, _dptr(p), n, nd, int(bool(physical)), int(ds_id), n_alt, _iptr(kd), _dptr(al),
                                        None if ow is None else _dptr(ow), _dptr(lw), _dptr(table), _dptr(tail), _iptr(st),
                                        C.byref(used)), "mp_model_reweight")
        return lw, table, tail[:, :tlen], st, int(used.value)

    def simulate(self, pars, x, yerr=None, frac_err=0.25, seed=0, physical=False):
        """Simulated light curves of the rows of pars (mp_simulate): the model at the times x, an error per observation and
        Gaussian noise.  x: (n_obs,) times shared by the rows, or (n, n_obs) a row of times each; yerr: absolute errors of x's
        shape, or None for frac_err * |model|.  Returns {"y", "yerr", "model", "z": (n, n_obs), "status": (n,), "n_ok"}; a row
        that did not finish, or whose error came out 0 (STATUS_ZEROERR), is all NaN.  Row i's noise depends on seed, i and the
        observation alone.  physical=False: sampler coordinates under the handle's prior, as lnprob_batch takes them."""
        p = np.ascontiguousarray(pars, dtype=np.float64)
        if p.ndim != 2 or p.shape[0] < 1:
            raise ValueError(f"pars must be 2-D (n >= 1, ndim), got shape {p.shape}")
        n, nd = p.shape
        xa = np.ascontiguousarray(x, dtype=np.float64)
        if xa.ndim not in (1, 2) or xa.shape[-1] < 1 or (xa.ndim == 2 and xa.shape[0] != n):
            raise ValueError(f"x must be (n_obs,) or (n = {n}, n_obs), got shape {xa.shape}")
        ye = None if yerr is None else np.ascontiguousarray(yerr, dtype=np.float64)
        if ye is not None and ye.shape != xa.shape:
            raise ValueError(f"yerr must have x's shape {xa.shape}, got {ye.shape}")
        n_obs, x_rows = xa.shape[-1], (1 if xa.ndim == 1 else n)
        out = {k: np.empty((n, n_obs), dtype=np.float64) for k in ("y", "yerr", "model", "z")}
        st = np.empty(n, dtype=np.int32)
        ok = C.c_int64(0)
        check(self._L.mp_simulate(self._h, _dptr(p), n, nd, int(bool(physical)), _dptr(xa), int(n_obs), x_rows,
                                  None if ye is None else _dptr(ye), float(frac_err), C.c_uint64(int(seed) & (2**64 - 1)),
                                  _dptr(out["y"]), _dptr(out["yerr"]), _dptr(out["model"]), _dptr(out["z"]), _iptr(st), C.byref(ok)),
              "mp_simulate")
        out.update(status=st, n_ok=int(ok.value))
        return out

    def bridge_logz(self, x_fit, x_est, lnp_est, lower=None, upper=None, ds_id=0, n_draws=None, n_rep=1, seed=0, neff=None,
                    max_iter=1000, tol=1.0e-10, target=0, details=False, proposal="normal", nu=5, warp=False):
        """The bridge-sampling evidence of mp_bridge_logz: a Gaussian fitted to the rows x_fit, n_draws draws from it per
        repetition, and the fixed point over the rows x_est with their lnprob lnp_est (sampler coordinates; the box lower,
        upper is the prior's support, None for the test targets).  n_draws=None: as many as x_est has rows; neff=None:
        that number too (independent rows).  Returns {"out": (n_rep, BRIDGE_NOUT), columns BRIDGE_COLUMNS}; details=True adds
        "moments", "draws" (n_rep, n_draws, ndim), "draw_lnp", "draw_lnq" (n_rep, n_draws) and "est_lnq" (n_est,).
        proposal="t" (a Student-t with nu degrees of freedom and the rows' covariance), warp=True (Warp-III: the posterior
        symmetrised about the rows' mean) or a target above 2 go to mp_bridge_logz_warp: "out" is (n_rep, BRIDGE_WARP_NOUT),
        columns BRIDGE_WARP_COLUMNS, and details=True adds "a" (n_est,) and "b" (n_rep, n_draws) too, with warp also
        "draw_mirrors", "draw_mirror_lnp" and "est_mirror_lnp".  With the defaults the call is mp_bridge_logz's as before."""
        prop = bridge_proposal(proposal, nu, warp)
        new = prop != (BRIDGE_NORMAL, 0, 0) or int(target) > 2
        xf = np.ascontiguousarray(x_fit, dtype=np.float64)
        xe = np.ascontiguousarray(x_est, dtype=np.float64)
        le = np.ascontiguousarray(lnp_est, dtype=np.float64)
        if xf.ndim != 2 or xe.ndim != 2 or xf.shape[1] != xe.shape[1] or le.shape != (xe.shape[0],):
            raise ValueError(f"x_fit (n_fit, ndim), x_est (n_est, ndim) and lnp_est (n_est,) expected, got {xf.shape}, {xe.shape}, {le.shape}")
        nd, n_est = xf.shape[1], xe.shape[0]
        n_draws = n_est if n_draws is None else int(n_draws)
        n_rep = int(n_rep)
        if (lower is None) != (upper is None):
            raise ValueError("lower and upper go together")
        lo = hi = None
        if lower is not None:
            lo = np.ascontiguousarray(lower, dtype=np.float64)
            hi = np.ascontiguousarray(upper, dtype=np.float64)
            if lo.shape != (nd,) or hi.shape != (nd,):
                raise ValueError(f"lower and upper must have shape ({nd},), got {lo.shape}, {hi.shape}")
        out = np.full((max(n_rep, 1), BRIDGE_WARP_NOUT if new else BRIDGE_NOUT), np.nan)
        nm, tot, ne = nd + nd * (nd + 1) // 2, max(n_rep, 1) * max(n_draws, 1), max(n_est, 1)
        # the optional outputs in the entries' order: mp_bridge_logz's five, then mp_bridge_logz_warp's
        shapes = {"moments": nm, "draws": (tot, nd), "draw_lnp": tot, "draw_lnq": tot, "est_lnq": ne}
        if new:
            shapes.update(a=ne, b=tot, draw_mirrors=(tot, nd), est_mirror_lnp=ne, draw_mirror_lnp=tot)
        mirrors = ("draw_mirrors", "est_mirror_lnp", "draw_mirror_lnp")
        det = {k: np.full(shape, np.nan) for k, shape in shapes.items() if details and (prop[2] or k not in mirrors)}
        opt = [(_dptr(det[k]) if k in det else None) for k in shapes]
        lead = (self._h, _dptr(xf), xf.shape[0], _dptr(xe), _dptr(le), n_est, nd, int(ds_id), None if lo is None else _dptr(lo),
                None if hi is None else _dptr(hi), n_draws, n_rep, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                float(n_est if neff is None else neff), int(max_iter), float(tol), int(target))
        if new:
            check(self._L.mp_bridge_logz_warp(*lead, *prop, _dptr(out), *opt), "mp_bridge_logz_warp")
        else:
            check(self._L.mp_bridge_logz(*lead, _dptr(out), *opt), "mp_bridge_logz")
        res = {"out": out}
        for k, v in det.items():      # per call, per estimator row, or per draw of a repetition
            res[k] = v if k == "moments" else v[:n_est] if k in ("est_lnq", "a", "est_mirror_lnp") else v.reshape((n_rep, n_draws) + v.shape[1:])
        return res

    def rhs_batch(self, pars, t, y, want_lam=False):
        """(dMdisc/dt, domega/dt) at n states: pars (n, ndim) physical, t (n,), y (n, 2) = (Mdisc, omega)."""
        p = np.ascontiguousarray(pars, dtype=np.float64)
        tt = np.ascontiguousarray(t, dtype=np.float64).ravel()
        yy = np.ascontiguousarray(y, dtype=np.float64)
        if p.ndim != 2 or yy.shape != (p.shape[0], 2) or tt.shape != (p.shape[0],):
            raise ValueError("pars (n, ndim), t (n,), y (n, 2) expected")
        n = p.shape[0]
        out = np.empty((n, 2), dtype=np.float64)
        lam = np.empty(n, dtype=np.float64)
        check(self._L.mp_rhs_batch(self._h, _dptr(p), int(p.shape[1]), _dptr(tt), _dptr(yy), n, _dptr(out), _dptr(lam)),
              "mp_rhs_batch")
        return (out, lam) if want_lam else out

    def synchronize(self):
        check(self._L.mp_synchronize(self._h), "mp_synchronize")

    @property
    def last_mean_sweeps(self):
        return self._L.mp_last_mean_sweeps(self._h)

    @property
    def last_mean_tiles(self):
        """Tiles solved per walker in the most recent host-buffer batch (kept or redone)."""
        return self._L.mp_last_mean_tiles(self._h)

    def last_sweeps(self, n):
        """Total Newton sweeps (over all tiles) of each of the first n walkers of the most recent host-buffer batch."""
        out = np.zeros(n, dtype=np.int32)
        m = self._L.mp_last_sweeps(self._h, _iptr(out), int(n))
        return out[:max(m, 0)]

    def last_tiles(self, n):
        """Tiles solved (kept or redone) by each of the first n walkers of the most recent host-buffer batch."""
        out = np.zeros(n, dtype=np.int32)
        m = self._L.mp_last_tiles(self._h, _iptr(out), int(n))
        return out[:max(m, 0)]

    def tile_log(self, enable=True):
        """Record, in every later host-buffer batch, what each walker's tiles were (diagnostics)."""
        check(self._L.mp_tile_log(self._h, int(bool(enable))), "mp_tile_log")

    def last_tile_log(self, walker):
        """[(kind, sweeps, lanes kept, why), ...] of `walker` in the most recent host-buffer batch (tile_log() on): kind 0 =
        1/8-interval sub-steps, 1 .. 4 = steps over 1 / 2 / 4 / 8 grid intervals; 0 lanes kept = the tile was redone; why =
        bits: 1 a branch of the right-hand side changed inside the tile, 2 / 4 / 8 / 32 the smoothness indicator exceeded
        stride_tol / its 64th / its 2048th / its 65536th somewhere, 16 lanes had not converged when the sweeps were
        stopped, 64 the tile was given up after its second sweep."""
        buf = np.zeros(96, dtype=np.int32)
        m = self._L.mp_last_tile_log(self._h, int(walker), _iptr(buf), 96)
        return [(int(w) & 15, (int(w) >> 4) & 0xFFF, (int(w) >> 16) & 0xFF, (int(w) >> 24) & 0xFF) for w in buf[:max(m, 0)]]

    @property
    def sweep_tol(self):
        return self._L.mp_sweep_tol(self._h)

    @property
    def policy(self):
        """The solver settings in force (mp_get_policy): a dict keyed by POLICY_FIELDS.  experiments_build = 1.0 marks the
        developer build that honours MAGPROP_AMD_* environment overrides; the shipped library reports 0."""
        buf = np.zeros(len(POLICY_FIELDS))
        m = self._L.mp_get_policy(self._h, _dptr(buf), int(buf.size))
        if m < 0:
            check(m, "mp_get_policy")
        return dict(zip(POLICY_FIELDS[:m], (float(v) for v in buf[:m])))

    @property
    def n_simd(self):
        """SIMDs of the device: batches up to n_simd walkers run the 4-steps-per-lane kernel, larger ones the
        2-steps-per-lane kernel (mp_device.h)."""
        return self._L.mp_n_simd(self._h)

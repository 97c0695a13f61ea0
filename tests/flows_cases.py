"""Named cases for the two kernels behind mp_model_flows (magprop_amd/csrc/mp_flows.hip) and their numpy restatement
(tests/flows_restated.py).

Cell cases (cell_cases()): dicts of name, preset ("synth", "lib" or "fig3") with cfg overrides, ndim, physical parameter rows
pars[rows][ndim], states t / mdisc / omega [rows][G], status[rows] and `either`[rows][G]: the bit of BRANCH (1: the cap rmu == k
c / omega, 2: Rm == R; 0: none) on whose boundary the state was constructed, to within an ulp of Mdisc, so that this bit may
fall on either side of the tie while the other one is as restated; every other curve is continuous there.  A workgroup of the cells kernel takes 512 points of one row and a wavefront 128 of them (two per
lane), which is what the grid sizes and the "wave" cases are built around.

Reduce cases (reduce_cases()): (name, t[G], cells[10][n][G], status[n]), crafted cell curves on crafted grids, in the manner of
tests/derive_cases.py (whose segment and window corners they share)."""
import functools

import numpy as np

import derive_cases as dc
import flows_restated as fr

PRESETS = {
    "synth": dict(inertia_factor=0.35, rm_massflow_factor=3.0, n_ode=10.0, alpha=0.1, cs7=1.0, k=0.9, dipole_torque=0),
    "lib": dict(inertia_factor=0.8, rm_massflow_factor=1.0, n_ode=1.0, alpha=0.1, cs7=1.0, k=0.9, dipole_torque=0),
    "fig3": dict(inertia_factor=0.8, rm_massflow_factor=3.0, n_ode=10.0, alpha=0.1, cs7=1.0, k=0.9, dipole_torque=0),
}
CELL_GRID_SIZES = (2, 3, 257, 258, 511, 513)        # 511 / 513: either side of a workgroup's 512 points
CELL_ROW_COUNTS = (1, 63, 64, 65, 257)
WAVE_POINTS = 128                                    # points of a wavefront of the cells kernel


class Cfg:
    """the fields of mp_model_cfg the flows read, as attributes (what flows_restated.cells takes)"""

    def __init__(self, preset, **over):
        self.__dict__.update(PRESETS[preset])
        self.__dict__.update(over)


def cfg_of(case):
    return Cfg(case["preset"], **case["over"])


def draw_pars(rng, rows, ndim):
    """physical rows inside the synthetic prior box (B, P, MdiscI, RdiscI, epsilon, delta) and efficiencies behind them"""
    p = np.empty((rows, ndim))
    p[:, 0] = 10.0 ** rng.uniform(-2.0, 1.0, rows)
    p[:, 1] = rng.uniform(0.69, 10.0, rows)
    p[:, 2] = 10.0 ** rng.uniform(-5.0, -2.0, rows)
    p[:, 3] = 10.0 ** rng.uniform(np.log10(50.0), np.log10(2000.0), rows)
    p[:, 4] = 10.0 ** rng.uniform(-1.0, 1.0, rows)
    p[:, 5] = 10.0 ** rng.uniform(-1.0, 2.0, rows)
    p[:, 6:] = rng.uniform(0.05, 1.0, (rows, ndim - 6))
    return p


def draw_states(rng, rows, G):
    """states along a log grid: disc masses of 1e-8 .. 1e-2 Msol, spins of 30 .. 6 000 rad/s"""
    t = np.broadcast_to(np.logspace(0.0, 6.0, G) if G > 1 else np.ones(1), (rows, G)).copy()
    mdisc = fr.M_SOL * 10.0 ** rng.uniform(-8.0, -2.0, (rows, G))
    omega = 10.0 ** rng.uniform(1.5, 3.78, (rows, G))
    return t, mdisc, omega


def rmu_constants(cfg, par):
    """(A, tvisc) with the uncapped Alfven radius rmu = A (f Mdisc / tvisc)^(-2/7)"""
    tvisc = (par[3] * 1.0e5) / (cfg.alpha * cfg.cs7 * 1.0e7)
    mu = 1.0e15 * par[0] * fr.R_STAR ** 3.0
    return mu ** (4.0 / 7.0) * fr.GM ** (-1.0 / 7.0), tvisc


def mdisc_for_rmu(cfg, par, rmu):
    """the disc mass whose uncapped Alfven radius is rmu (to rounding)"""
    A, tvisc = rmu_constants(cfg, par)
    return (tvisc / cfg.rm_massflow_factor) * np.power(rmu / A, -3.5)


def omega_breakup(cfg):
    """the spin at which the rotation parameter T / |W| is 0.27"""
    return np.sqrt(0.27 * fr.mod_w() / (0.5 * fr.inertia(cfg)))


@functools.lru_cache(maxsize=None)
def cell_cases():
    rng = np.random.default_rng(20271)
    out = []

    def add(name, preset, pars, t, mdisc, omega, status=None, either=None, **over):
        pars = np.ascontiguousarray(np.atleast_2d(pars), dtype=np.float64)
        t, mdisc, omega = (np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64) for a in (t, mdisc, omega))
        assert t.shape == mdisc.shape == omega.shape and t.shape[0] == pars.shape[0]
        st = np.zeros(pars.shape[0], dtype=np.int32) if status is None else np.asarray(status, dtype=np.int32)
        ei = np.zeros(t.shape, dtype=np.int64) if either is None else np.asarray(either, dtype=np.int64).reshape(t.shape)
        out.append(dict(name=name, preset=preset, over=over, ndim=pars.shape[1], pars=pars, t=t, mdisc=mdisc, omega=omega,
                        status=st, either=ei))

    def random_case(name, preset, rows, G, ndim=6, status=None, **over):
        t, m, o = draw_states(rng, rows, G)
        add(name, preset, draw_pars(rng, rows, ndim), t, m, o, status, **over)

    # presets, torque laws, ndim, grid sizes, row counts, failed rows
    for preset in ("synth", "lib", "fig3"):
        for torque in (0, 1):
            random_case(f"{preset}_torque{torque}", preset, 3, 300, dipole_torque=torque)
    for ndim in (6, 7, 8, 9):
        random_case(f"ndim_{ndim}", "lib", 2, 130, ndim=ndim)
    for G in CELL_GRID_SIZES:
        random_case(f"grid_{G}", "synth", 3, G)
    for rows in CELL_ROW_COUNTS:
        st = np.zeros(rows, dtype=np.int32)
        st[2::5] = np.array([1, 2, 3])[np.arange(len(st[2::5])) % 3]       # flagged, non-finite and outside-the-prior rows between finished ones
        random_case(f"rows_{rows}", "synth", rows, 33, status=st)
    random_case("other_k_alpha", "synth", 2, 200, k=0.6, alpha=0.3)

    # constructed states, on the figure's parameter row
    par = np.array([1.0, 5.0, 1.0e-3, 1000.0, 0.1, 1.0])
    for preset, torque in (("fig3", 0), ("fig3", 1), ("lib", 0)):
        cfg = Cfg(preset, dipole_torque=torque)
        tag = f"{preset}{torque}"
        om = np.array([300.0, 1256.6370614359173, 4000.0])
        # the cap: rmu == k c / omega, and one ulp of Mdisc to either side
        m0 = mdisc_for_rmu(cfg, par, cfg.k * fr.C_LIGHT / om)
        m = np.stack([np.nextafter(m0, 0.0), m0, np.nextafter(m0, np.inf)], axis=1).reshape(1, -1)
        add(f"cap_tie_{tag}", preset, par, np.full(m.shape, 10.0), m, np.repeat(om, 3).reshape(1, -1), either=np.full(m.shape, 1),
            dipole_torque=torque)
        # Rm == R without the cap (k c / omega > R for these spins)
        m0 = np.full(3, mdisc_for_rmu(cfg, par, fr.R_STAR))
        m = np.stack([np.nextafter(m0, 0.0), m0, np.nextafter(m0, np.inf)], axis=1).reshape(1, -1)
        add(f"rm_equals_r_{tag}", preset, par, np.full(m.shape, 10.0), m, np.repeat(om, 3).reshape(1, -1), either=np.full(m.shape, 2),
            dipole_torque=torque)
        # w == 1: Rm == Rc (uncapped: Rc < k Rlc for these spins), and close to it on either side
        rc = np.cbrt(fr.GM / om ** 2.0)
        f = np.array([1.0 - 1e-9, 1.0 - 1e-15, 1.0, 1.0 + 1e-15, 1.0 + 1e-9])
        m = mdisc_for_rmu(cfg, par, rc[:, None] * f[None, :]).reshape(1, -1)
        add(f"w_equals_1_{tag}", preset, par, np.full(m.shape, 100.0), m, np.repeat(om, f.size).reshape(1, -1), dipole_torque=torque)
        # the rotation parameter just below and just above 0.27, uncapped and capped
        ob = omega_breakup(cfg) * np.array([1.0 - 1e-9, 1.0 + 1e-9, 1.0 - 1e-9, 1.0 + 1e-9])
        m = mdisc_for_rmu(cfg, par, np.array([2.0e6, 2.0e6, 1.0e8, 1.0e8])).reshape(1, -1)   # (k c / omega is 2.9e6 cm there)
        add(f"breakup_{tag}", preset, par, np.full(m.shape, 1000.0), m, ob.reshape(1, -1), dipole_torque=torque)
    # t at both ends of the reference's grids, and far outside them
    tt = np.array([1.0e-3, 1.0, 1.0e6, 1.0e7]).reshape(1, -1)
    add("t_ends", "synth", par, tt, np.full(tt.shape, 1e-4 * fr.M_SOL), np.full(tt.shape, 1000.0))
    # the switch saturated on both sides: n = 100 reaches n (w - 1) < -19.5 on the accretion side (n = 10 cannot: w > 0)
    cfg = Cfg("fig3", n_ode=100.0)
    om1 = 1256.6370614359173
    rc1 = np.cbrt(fr.GM / om1 ** 2.0)
    deep_acc = mdisc_for_rmu(cfg, par, rc1 * 0.5 ** (2.0 / 3.0))       # w = 0.5: x = -50
    deep_prop = mdisc_for_rmu(cfg, par, rc1 * 3.0 ** (2.0 / 3.0))      # w = 3: x = 200
    near = mdisc_for_rmu(cfg, par, rc1 * 1.01 ** (2.0 / 3.0))          # w = 1.01: x = 1
    G = 3 * WAVE_POINTS
    m = np.empty((4, G))
    m[0] = deep_acc                                   # every wavefront uniformly saturated, accretion side
    m[1] = deep_prop                                  # ... propeller side
    m[2] = np.where(np.arange(G) % 2 == 0, deep_acc, deep_prop)   # saturated on both sides inside every wavefront
    m[3] = deep_acc                                   # wavefront 0 uniformly saturated, wavefront 1 mixed, wavefront 2 one state short of uniform
    m[3, WAVE_POINTS:2 * WAVE_POINTS:3] = near
    m[3, 2 * WAVE_POINTS + 77] = near
    add("saturated_waves", "fig3", np.tile(par, (4, 1)), np.broadcast_to(np.logspace(0, 6, G), (4, G)), m, np.full((4, G), om1),
        n_ode=100.0)
    return out


def cell_names():
    return [c["name"] for c in cell_cases()]


def cell_case(name):
    return next(c for c in cell_cases() if c["name"] == name)


# ---------------------------------------------------------------- reduce cases
REDUCE_GRID_SIZES = (2, 3, 256, 257, 258, 513, 514, 10001)
REDUCE_WINDOW_GRID_SIZES = dc.WINDOW_GRID_SIZES[:3] + dc.WINDOW_GRID_SIZES[4:6]


def random_cells(rng, n, G):
    """n rows of plausible cell curves: positive radii and rates, torques of either sign, a fastness that crosses 1, flags 0 .. 3"""
    c = np.empty((fr.NCURVES, n, G))
    for k in range(fr.NCURVES):
        c[k] = dc.smooth(rng, n, G)
    c[fr.FASTNESS] = 0.4 + c[fr.FASTNESS]
    c[fr.N_ACC] -= 0.5
    c[fr.N_DIP] *= -1.0
    c[fr.BRANCH] = rng.integers(0, 4, (n, G)).astype(np.float64)
    return c


@functools.lru_cache(maxsize=None)
def reduce_cases():
    rng = np.random.default_rng(20272)
    out = []

    def add(name, t, cells, status=None):
        cells = np.ascontiguousarray(cells, dtype=np.float64)
        assert cells.ndim == 3 and cells.shape[0] == fr.NCURVES and cells.shape[2] == len(t)
        st = np.zeros(cells.shape[1], dtype=np.int32) if status is None else np.asarray(status, dtype=np.int32)
        out.append((name, np.ascontiguousarray(t, dtype=np.float64), cells, st))

    for G in REDUCE_GRID_SIZES + REDUCE_WINDOW_GRID_SIZES:
        add(f"grid_{G}", dc.log_grid(G), random_cells(rng, 2, G))
    G = 1000                                             # seg = 4: segment 7 holds intervals 28 .. 31
    t = dc.log_grid(G)

    def with_fastness(w, n=1):
        c = random_cells(rng, n, G)
        c[fr.FASTNESS] = w
        return c

    add("never_propeller", t, with_fastness(np.full(G, 0.5)))
    add("always_propeller", t, with_fastness(np.full(G, 1.5)))
    add("exactly_one", t, with_fastness(np.full(G, 1.0)))            # w == 1 is the propeller side
    first, last = np.full(G, 0.5), np.full(G, 0.5)
    first[0], last[-1] = 2.0, 2.0
    add("propeller_first_point_only", t, with_fastness(first))
    add("propeller_last_point_only", t, with_fastness(last))
    add("alternating", t, with_fastness(np.where(np.arange(G) % 2 == 0, 0.5, 1.5)))      # N_SWITCH = G - 1
    add("switch_on_segment_boundary", t, with_fastness(np.where(np.arange(G) < 28, 0.5, 1.5)))
    add("switch_before_segment_boundary", t, with_fastness(np.where(np.arange(G) < 27, 1.5, 0.5)))
    # ties: plateaus of the largest fastness and of the smallest radius (the first point of each is the answer), also at the ends
    c = random_cells(rng, 3, G)
    c[fr.FASTNESS, 0, 100:140] = c[fr.FASTNESS, 0].max() + 1.0
    c[fr.RM, 0, 500:520] = c[fr.RM, 0].min() - 1e-4
    c[fr.FASTNESS, 1, [0, G - 1]] = 9.0
    c[fr.RM, 1, [0, G - 1]] = 1e-5
    c[fr.FASTNESS, 2, [255, 256, 511, 512]] = 9.0                     # across the strided visit: thread 255, 0, 255, 0
    c[fr.RM, 2, [511, 256, 768]] = 1e-5
    add("ties", t, c)
    # a switch on a window boundary: seg = 29 at G = 256 * 28 + 2, windows of 14 intervals
    Gw = 256 * 28 + 2
    tw = dc.log_grid(Gw)
    cw = random_cells(rng, 2, Gw)
    cw[fr.FASTNESS, 0] = np.where(np.arange(Gw) < 5 * 29 + 14, 0.5, 1.5)
    cw[fr.FASTNESS, 1] = np.where(np.arange(Gw) < 5 * 29 + 28, 1.5, 0.5)
    add("switch_on_window_boundary", tw, cw)
    # zeros and signs of zero, tiny and huge values
    G = 300
    t = dc.log_grid(G)
    add("all_zero", t, np.zeros((fr.NCURVES, 1, G)))
    add("negative_zero", t, np.full((fr.NCURVES, 1, G), -0.0))
    base = random_cells(rng, 1, G)
    for name, s in (("tiny", 1e-300), ("huge", 1e290)):
        c = base * s
        c[fr.BRANCH] = base[fr.BRANCH]
        add(name, t, c)
    # row counts around a wavefront, failed rows between finished ones
    for n in (1, 63, 64, 65, 257):
        st = np.zeros(n, dtype=np.int32)
        st[1::4] = np.array([1, 2, 3])[np.arange(len(st[1::4])) % 3]
        add(f"rows_{n}", dc.log_grid(40), random_cells(rng, n, 40), st)
    return out


def reduce_names():
    return [c[0] for c in reduce_cases()]


def reduce_case(name):
    return next(c for c in reduce_cases() if c[0] == name)

"""numpy restatement of mp_model_flows' definition (include/magprop_amd.h; magprop_amd/csrc/mp_flows.h): the cell curves written
from the reference's formulas (code/figure_3.py:202-286 and its right-hand sides :40-165, with libm's tanh-free exp, cbrt and
power), and the reduction of a row's cells to the 16 columns in tests/derive_restated.py's manner.  What
tests/test_gpu_flows_kernels.py and tests/test_gpu_flows.py hold the device against -- the cells under the bound cell_bounds()
derives, the reduction bit for bit -- and what tests/test_flows_cases_cpu.py holds against the reference's recorded arrays, the
recorded right-hand sides and a long-double definition.

Cells.  The reference forms eta2 = (1 + tanh x) / 2 and eta1 = 1 - eta2, x = n (w - 1); 1 - eta2 loses the smaller of the two to
the rounding of the larger (an absolute 1.1e-16).  Here, as on the device, (1 + tanh x) / 2 = 1 / (1 + exp(-2 x)): with
e = exp(-2 |x|) the larger is 1 / (1 + e) and the smaller e / (1 + e), each to its own relative accuracy."""
import numpy as np

import derive_restated as dr

NCURVES = 10
RM, RC, RLC, FASTNESS, MDOT_PROP, MDOT_ACC, MDOT_FB, N_ACC, N_DIP, BRANCH = range(NCURVES)
CURVE_NAMES = ("Rm", "Rc", "Rlc", "fastness", "Mdot_prop", "Mdot_acc", "Mdot_fb", "N_acc", "N_dip", "branch")
REDUCE_MASK = sum(1 << c for c in (RM, FASTNESS, MDOT_PROP, MDOT_ACC, MDOT_FB, N_ACC, N_DIP, BRANCH))

N = 16
M_FB, M_PROP, M_ACC, J_ACC, J_DIP, W_MAX, T_W_MAX, W_END, N_PROP, T_PROP_FIRST, T_PROP_LAST, N_SWITCH, N_CAPPED, N_INSIDE = range(14)
RM_MIN, T_RM_MIN = 14, 15
SUMS = ((M_FB, MDOT_FB), (M_PROP, MDOT_PROP), (M_ACC, MDOT_ACC), (J_ACC, N_ACC), (J_DIP, N_DIP))

# code/figure_3.py:9-13 (cgs)
G_NEWTON, C_LIGHT, R_STAR, M_SOL = 6.674e-8, 3.0e10, 1.0e6, 1.99e33
M_STAR = 1.4 * M_SOL
GM = G_NEWTON * M_STAR
EPS = 2.0 ** -52
SATURATED = np.exp(-39.0)      # e = exp(-2 |x|) at |x| = 19.5, where flow_state (mp_eval.hpp) takes tanh for +-1: 1.15e-17


def inertia(cfg):
    return cfg.inertia_factor * M_STAR * R_STAR ** 2.0


def mod_w():
    b = GM / (R_STAR * C_LIGHT ** 2.0)
    return 0.6 * M_STAR * C_LIGHT ** 2.0 * (b / (1.0 - 0.5 * b))


def exponent_error(num, den):
    """|fl(num / den) - num / den| as a float: by how much the double nearest to a rational exponent misses it"""
    from fractions import Fraction
    return float(abs(Fraction(num / den) - Fraction(num, den)))


# x^fl(p) = x^p exp((fl(p) - p) ln x): a power with an inexact exponent is off by |fl(p) - p| |ln x| relative, whatever libm does
D_1_3, D_2_7, D_4_7, D_5_3 = exponent_error(1, 3), exponent_error(2, 7), exponent_error(4, 7), exponent_error(5, 3)


def cells(cfg, par, t, mdisc, omega, k=None, alpha=None, literal_rc=False):
    """The ten cell curves (10, ...) at states (t, mdisc, omega) (arrays of one shape) of the physical parameter row par =
    (B, P, MdiscI, RdiscI, epsilon, delta, ...), under the model configuration cfg (k, alpha: in place of cfg's).  The
    corotation radius is the cube root (libm's cbrt); literal_rc=True forms it as the reference writes it, (GM / omega^2) **
    (1 / 3), for comparisons with the reference's own numbers: fl(1/3) is not 1/3, and at ln(GM / omega^2) = 46 that is four
    units of the last place.  Also returns the intermediate numbers the bounds need: {"mdot", "x", "arm_mdot", "rot"} and the
    relative errors of the inexact exponents, "xrm" (the restated -2/7 and 4/7 powers against the device's exact ones, where
    the radius is not capped), "xrc" (the reference's 1/3 power) and "xfb" (the -5/3 power)."""
    t, mdisc, omega = (np.asarray(a, dtype=np.float64) for a in (t, mdisc, omega))
    k = cfg.k if k is None else k
    alpha = cfg.alpha if alpha is None else alpha
    B, MdiscI, RdiscI, epsilon, delta = par[0], par[2], par[3], par[4], par[5]
    tvisc = (RdiscI * 1.0e5) / (alpha * cfg.cs7 * 1.0e7)
    mu = 1.0e15 * B * R_STAR ** 3.0
    M0 = delta * MdiscI * M_SOL
    tfb = epsilon * tvisc
    with np.errstate(all="ignore"):
        mdot = mdisc / tvisc
        rm = mu ** (4.0 / 7.0) * GM ** (-1.0 / 7.0) * np.power((cfg.rm_massflow_factor * mdisc) / tvisc, -2.0 / 7.0)
        rc = np.power(GM / omega ** 2.0, 1.0 / 3.0) if literal_rc else np.cbrt(GM / omega ** 2.0)
        rlc = C_LIGHT / omega
        capped = rm >= k * rlc
        rm = np.where(capped, k * rlc, rm)
        w = np.power(rm / rc, 1.5)
        x = cfg.n_ode * (w - 1.0)
        e = np.exp(-2.0 * np.abs(x))
        large, small = 1.0 / (1.0 + e), e / (1.0 + e)
        eta2 = np.where(x >= 0.0, large, small)
        eta1 = np.where(x >= 0.0, small, large)
        prop, acc = eta2 * mdot, eta1 * mdot
        fb = (M0 / tfb) * np.power((t + tfb) / tfb, -5.0 / 3.0)
        rot = 0.5 * inertia(cfg) * omega ** 2.0 / mod_w()
        arm = np.sqrt(GM * np.maximum(rm, R_STAR))
        nacc = np.where(rot > 0.27, 0.0, arm * (acc - prop))
        if cfg.dipole_torque == 1:
            ndip = (-2.0 / 3.0) * ((mu ** 2.0 * omega ** 3.0) / C_LIGHT ** 3.0) * (rlc / rm) ** 3.0
        else:
            ndip = (-1.0 * mu ** 2.0 * omega ** 3.0) / (6.0 * C_LIGHT ** 3.0)
        branch = capped * 1.0 + (rm >= R_STAR) * 2.0
    out = np.stack([np.broadcast_to(a, t.shape) for a in (rm, rc, rlc, w, prop, acc, fb, nacc, ndip, branch)]).astype(np.float64)
    with np.errstate(all="ignore"):
        xrm = np.where(capped, 0.0, D_2_7 * np.abs(np.log(mdot)) + D_4_7 * np.abs(np.log(B)))
        xrc = D_1_3 * np.abs(np.log(GM / omega ** 2.0))
        xfb = D_5_3 * np.abs(np.log((t + tfb) / tfb))
    return out, {"mdot": mdot, "x": x, "arm_mdot": arm * mdot, "rot": rot, "xrm": xrm + 0.0 * x, "xrc": xrc + 0.0 * x, "xfb": xfb + 0.0 * x}


# Relative error budgets in units of EPS = 2^-52, counted operation by operation (a correctly rounded operation adds 1/2, a libm
# power or cbrt 1, a device primitive -- rcp, rsqrt, rcbrt, pow_m1_7, exp of mp_math.hpp -- 2, its tested bound; a power p
# multiplies what its argument carries by |p|), device plus restatement, rounded up:
#   Mdisc / tvisc        device Mdisc * (1 / tau), tau three operations: 3; restated 3                                     -> 6
#   RM uncapped          device Crm * t^2: Crm = crm_unit (three powers, five products: 6) * B * b17^3 (b17 2: 8, +2) -> 16,
#                        t = pow_m1_7(mdot): 3 / 7 + 2, squared 6, product 1 -> 23; restated: mu 2, mu^(4/7) 2, GM^(-1/7) 1,
#                        (f Mdisc / tvisc)^(-2/7) 2, two products 1 -> 8                                                   -> 32
#   RM capped, RLC       device kc * y^2, y = rsqrt(omega) 2: 6; restated 2                                               -> 8
#   RC                   device rcbrt((omega / sqrt GM)^2): (3 squared 7) / 3 + 2 -> 5; restated 3                         -> 8
#   FASTNESS uncapped    device omega * Crm15 * t^3: Crm15 = Crm sqrt(Crm) / sqrt(GM) 16 + 8 + 4 = 28, t^3 9, products 2 -> 39;
#                        restated (Rm / Rc)^1.5: (8 + 3 + 1) * 1.5 + 1 = 19                                                -> 58
#   MDOT_FB              device S_amp 8, u = fma(t, 1 / tfb, 1) 6, rcbrt 6 / 3 + 2 = 4, fifth power 20 + 3, product 1 -> 32;
#                        restated M0 / tfb 6, ((t + tfb) / tfb)^(-5/3): 6 * 5 / 3 + 1 = 11, product 1 -> 18                -> 50
#   N_DIP                law 0: mu^2 / (6 c^3) 5 and omega^3 2 on either side -> 14; law 1: three times RM's 32 plus 16
E_MDOT, E_RM, E_RLC, E_RC, E_W, E_FB, E_NDIP0, E_NDIP1 = 6.0, 32.0, 8.0, 8.0, 58.0, 50.0, 14.0, 3 * 32.0 + 16.0


def cell_bounds(cfg, c, aux, against_reference=False):
    """Absolute bounds (10, ...) on |device cell - restated cell| at the states behind c, aux = cells(...), derived, not measured.

    Besides the counts above, the inexact exponents (aux "xrm", "xfb"; against the reference's recorded arrays also "xrc": the
    device and np.cbrt take the cube root, the reference the power fl(1/3)) enter RM, MDOT_FB and RC, and through them what is
    built on them: the fastness carries ew = E_W EPS + 1.5 xrm (+ 1.5 xrc) relative, N_DIP of law 1 three times xrm, the arm
    of N_ACC half of it.

    The switch.  x = n (w - 1) carries the absolute error dx = n w ew of the fastness and the roundings of its own: one on the
    device (an fma), two restated, 1.5 |x| EPS together.  With e = exp(-2 |x|): de / e = 2 dx + 3 |x| EPS + 3 EPS (the device's
    exp to 2.26 ulp, libm's to 1/2) =: re.
      the SMALLER efficiency e / (1 + e) inherits re whole -- the relative "2 n w" propagation -- plus the sum, the reciprocal
        (2 ulp on the device) and the product on either side, 5 EPS;
      the LARGER one, 1 / (1 + e), changes by e / (1 + e) <= e times re, plus the same 5 EPS: where the switch is decided its rate
        is good to a few units of the last place, and the bound says so.
    Either rate then takes E_MDOT and a product, 1 EPS.  Absolute, on both: SATURATED * Mdisc / tvisc -- where every state of a
    wavefront has |x| > 19.5 the device takes the smaller efficiency for 0, and it is below exp(-39) there (1.2e-17 of the
    larger one, so far below its last place); the same floor covers e below the normal range.
    N_ACC = arm (Mdot_acc - Mdot_prop) = -arm mdot tanh x passes through zero at w = 1, so the switch enters it absolutely:
    tanh x = (1 - e) / (1 + e) changes by 2 e / (1 + e)^2 (de / e) = (sech^2 x / 2) re, which vanishes with e where the switch
    is saturated; times arm mdot.  Relative, on the value: the arm mdot product (sqrt of RM's error, E_MDOT, two products:
    E_RM / 2 + E_MDOT + 2, and xrm / 2) and the forming of tanh on either side (difference, reciprocal, products: 8 EPS).
    against_reference: the recorded arrays form eta2 from libm's tanh (1 ulp of a number up to 1) and eta1 = 1 - eta2, an
    absolute EPS of Mdisc / tvisc on either rate whichever is the smaller: 2 EPS mdot is added to both rates and, for the
    difference of the two, 4 EPS arm mdot to N_ACC."""
    n = cfg.n_ode
    w, x, mdot, arm_mdot = np.abs(c[FASTNESS]), np.abs(aux["x"]), np.abs(aux["mdot"]), np.abs(aux["arm_mdot"])
    xrm, xfb = aux["xrm"], aux["xfb"]
    xrc = aux["xrc"] if against_reference else 0.0
    ew = E_W * EPS + 1.5 * xrm + 1.5 * xrc
    dx = n * w * ew
    with np.errstate(all="ignore"):
        e = np.exp(-2.0 * x)
    re = 2.0 * dx + (3.0 * x + 3.0) * EPS
    sech2 = 4.0 * e / (1.0 + e) ** 2
    small = re + (5.0 + E_MDOT + 1.0) * EPS
    large = e * re + (5.0 + E_MDOT + 1.0) * EPS
    prop_is_large = aux["x"] >= 0.0
    b = np.empty_like(c)
    b[RM] = (E_RM * EPS + xrm) * np.abs(c[RM])
    b[RC] = (E_RC * EPS + xrc) * np.abs(c[RC])
    b[RLC] = E_RLC * EPS * np.abs(c[RLC])
    b[FASTNESS] = ew * w
    extra = 2.0 * EPS * mdot if against_reference else 0.0
    b[MDOT_PROP] = np.where(prop_is_large, large, small) * np.abs(c[MDOT_PROP]) + SATURATED * mdot + extra
    b[MDOT_ACC] = np.where(prop_is_large, small, large) * np.abs(c[MDOT_ACC]) + SATURATED * mdot + extra
    b[MDOT_FB] = (E_FB * EPS + xfb) * np.abs(c[MDOT_FB])
    b[N_ACC] = (0.5 * sech2 * re + (4.0 * EPS if against_reference else 0.0)) * arm_mdot + \
        ((E_RM / 2.0 + E_MDOT + 2.0 + 8.0) * EPS + 0.5 * xrm) * np.abs(c[N_ACC])
    b[N_DIP] = ((E_NDIP1 * EPS + 3.0 * xrm) if cfg.dipole_torque == 1 else E_NDIP0 * EPS) * np.abs(c[N_DIP])
    b[BRANCH] = 0.0
    return b


# ---------------------------------------------------------------- the reduction
def best(v):
    """(largest value, its index) under the device's total order (larger value, then lower index; NaN never): (NaN, -1) if none"""
    v = np.asarray(v, dtype=np.float64)
    ok = ~np.isnan(v)
    if not ok.any():
        return np.nan, -1
    i = int(np.argmax(np.where(ok, v, -np.inf)))
    return v[i], i


def reduce_row(c, t):
    """The 16 columns of one finished row: c (10, G) cell curves on the grid t (G,)."""
    c, t = np.asarray(c, dtype=np.float64), np.asarray(t, dtype=np.float64)
    out = np.empty(N)
    for col, curve in SUMS:
        out[col] = dr.running_sums(c[curve], t)[2]
    w = c[FASTNESS]
    out[W_MAX], i = best(w)
    out[T_W_MAX] = t[i] if i >= 0 else np.nan
    out[W_END] = w[-1]
    prop = w >= 1.0
    hit = np.nonzero(prop)[0]
    out[N_PROP] = float(hit.size)
    out[T_PROP_FIRST] = t[hit[0]] if hit.size else np.nan
    out[T_PROP_LAST] = t[hit[-1]] if hit.size else np.nan
    out[N_SWITCH] = float(np.count_nonzero(prop[1:] != prop[:-1]))
    with np.errstate(invalid="ignore"):
        b = c[BRANCH].astype(np.int64)
    out[N_CAPPED] = float(np.count_nonzero(b & 1))
    out[N_INSIDE] = float(np.count_nonzero((b & 2) == 0))
    v, i = best(-c[RM])
    out[RM_MIN] = -v
    out[T_RM_MIN] = t[i] if i >= 0 else np.nan
    return out


def reduce(c, status, t):
    """out (n, 16) of cells (10, n, G) and status (n,): rows whose status is not 0 are NaN."""
    c = np.asarray(c, dtype=np.float64)
    out = np.full((c.shape[1], N), np.nan)
    for r in range(c.shape[1]):
        if status[r] == 0:
            out[r] = reduce_row(c[:, r], t)
    return out


def reduce_longdouble(c, t):
    """The sums of one row in np.longdouble, added in plain index order: the definition without its order."""
    c, t = np.asarray(c, dtype=np.longdouble), np.asarray(t, dtype=np.longdouble)
    h = 0.5 * (t[1:] - t[:-1])
    return {col: (h * (c[curve, :-1] + c[curve, 1:])).sum() for col, curve in SUMS}

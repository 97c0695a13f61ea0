"""Writes tests/golden/golden_math.npz: inputs of the device math primitives (magprop_amd/csrc/mp_math.hpp) and their
correctly rounded values as double-double pairs, hi = float(v), lo = float(v - hi), from mpmath at 400 bits.

    python tests/golden/make_math_golden.py          # rewrites the fixture and its entry in MANIFEST.json

numpy and mpmath only; every input is built from SEED.  parts() returns the arrays of one group, so a test can regenerate
a slice (tests/test_math_cpu.py)."""
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261016
PREC = 400
GROUPS = ("recip", "root", "exp", "exp10", "phi", "scan", "lse", "merge")

# sampler coordinates that exp10_fast un-logs (log mask 0b111100: coordinates 2 .. 5), at the bounds of the prior boxes
SYNTH_LOWER = [-6.0, math.log10(50.0), -2.0, -1.0]            # magprop_amd/synth.py PRIOR_LOWER[2:]
SYNTH_UPPER = [-2.0, math.log10(2000.0), 2.0, 3.0]
LIB_LOWER = [-3.0, math.log10(50.0), -1.0, -5.0]              # magprop_amd/mcmc_eqns.py DEFAULT_LIMITS_LOWER[2:6]
LIB_UPPER = [-1.0, math.log10(2000.0), 3.0, math.log10(50.0)]


def _mp():
    import mpmath
    mpmath.mp.prec = PREC
    return mpmath


def _to_float(mp, v):
    """Nearest double of v, also where it is subnormal (one rounding)."""
    if v == 0:
        return 0.0
    if abs(v) < mp.mpf(2) ** -1022:
        return math.ldexp(int(mp.nint(v * mp.mpf(2) ** 1074)), -1074)
    return float(v)


def dd(mp, values):
    """hi, lo arrays of a list of mpf."""
    hi = np.array([_to_float(mp, v) for v in values])
    lo = np.array([_to_float(mp, v - mp.mpf(h)) if math.isfinite(h) else 0.0 for v, h in zip(values, hi)])
    return hi, lo


def neighbours(x):
    x = np.asarray(x, float)
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


def _pad(x, n, rng, lo, hi, log=False):
    """x filled up to n elements with random ones (uniform, or log-uniform, over [lo, hi])."""
    k = n - len(x)
    assert k >= 0, (len(x), n)
    u = rng.uniform(math.log(lo), math.log(hi), k) if log else rng.uniform(lo, hi, k)
    return np.concatenate([x, np.exp(u) if log else u])


def positive_inputs(rng, e_lo, e_hi, n):
    """Positive normal doubles over 2^e_lo .. 2^e_hi: powers of two with both neighbours, mantissas of all ones and of
    one set bit, the rest log-uniform."""
    es = np.linspace(e_lo + 1, e_hi - 1, 15).round().astype(int)
    p2 = np.ldexp(1.0, es)
    ones = np.ldexp(2.0 - 2.0 ** -52, es[::2])
    bits = np.concatenate([np.ldexp(1.0 + 2.0 ** -b, es[1::3]) for b in (1, 26, 52)])
    edge = np.concatenate([neighbours(p2), ones, bits, neighbours([1.0, 2.0, 3.0, 7.0, 8.0, 10.0])])
    return _pad(edge, n, rng, 2.0 ** e_lo, 2.0 ** e_hi, log=True)


# ---------------------------------------------------------------- the groups
def part_recip(mp, rng):
    x = positive_inputs(rng, -996, 996, 512)                  # 1e-300 .. 1e300
    out = {"recip_x": x}
    out["rcp_hi"], out["rcp_lo"] = dd(mp, [1 / mp.mpf(v) for v in x])
    out["rsqrt_hi"], out["rsqrt_lo"] = dd(mp, [1 / mp.sqrt(mp.mpf(v)) for v in x])
    return out


def part_root(mp, rng):
    # 2^-100 .. 2^100 as stated, extended to 2^-126 .. 2^127 (every normal float): disc_point applies pow_m1_7_fast to
    # Mdisc / tvisc in g/s, up to ~4e33 over the prior boxes, which 2^100 = 1.3e30 does not cover
    x = np.concatenate([positive_inputs(rng, -100, 100, 512), positive_inputs(rng, 100, 127, 128),
                        positive_inputs(rng, -126, -100, 128)])
    out = {"root_x": x}
    out["rcbrt_hi"], out["rcbrt_lo"] = dd(mp, [mp.power(mp.mpf(v), mp.mpf(-1) / 3) for v in x])
    out["pow17_hi"], out["pow17_lo"] = dd(mp, [mp.power(mp.mpf(v), mp.mpf(-1) / 7) for v in x])
    return out


def part_exp(mp, rng):
    """k ln2 / 2 for EVERY odd k inside [-750, 700], the worst reduced argument; both neighbours of every 16th of them (the
    file's size: tests/test_math_cpu.py measures the restatement on all of them with both neighbours, and
    tests/test_gpu_math.py holds the device bit for bit to the restatement on all of them); the clamps, zeros, tiny values
    and subnormal results; few random ones."""
    ln2h = math.log(2.0) / 2.0
    worst = np.arange(-2163, 2020, 2) * ln2h
    worst = worst[(worst >= -750.0) & (worst <= 700.0)]
    nb = worst[::16]
    edge = np.concatenate([worst, np.nextafter(nb, -np.inf), np.nextafter(nb, np.inf),
                           [-750.0, 700.0, np.nextafter(-750.0, 0), np.nextafter(700.0, 0), 0.0, -0.0,
                            1e-300, -1e-300, 5e-324, -5e-324, 2.0 ** -53, -2.0 ** -53, 1.0, -1.0],
                           rng.uniform(-750.0, -708.0, 96), [-745.2, -745.1, -744.5, -708.4, -708.3]])
    x = _pad(edge, 2560, rng, -750.0, 700.0)
    out = {"exp_x": x}
    out["exp_hi"], out["exp_lo"] = dd(mp, [mp.exp(mp.mpf(v)) for v in x])
    return out


def part_exp10(mp, rng):
    """Every bound of the prior boxes with its neighbours, the integers -300 .. 300, a dense uniform sample of the span of
    the boxes (where the sampler's coordinates lie) and a thinner one of [-300, 300]."""
    bounds = np.unique(np.array(SYNTH_LOWER + SYNTH_UPPER + LIB_LOWER + LIB_UPPER))
    edge = np.concatenate([neighbours(bounds), np.arange(-300.0, 301.0)])
    dense = rng.uniform(bounds.min(), bounds.max(), 2048 - 256 - len(edge))
    x = _pad(np.concatenate([edge, dense]), 2048, rng, -300.0, 300.0)
    out = {"exp10_x": x}
    out["exp10_hi"], out["exp10_lo"] = dd(mp, [mp.power(10, mp.mpf(v)) for v in x])
    return out


def _phi_exact(mp, z):
    """e^z, phi_1 .. phi_6 of a double z."""
    z = mp.mpf(z)
    out = [mp.exp(z)]
    if abs(z) < 1:
        for j in range(1, 7):
            s, term, k = mp.mpf(0), 1 / mp.factorial(j), 0
            while True:
                s += term
                k += 1
                term = term * z / (k + j)
                if term == 0 or abs(term) < mp.mpf(2) ** -(PREC + 20):
                    break
            out.append(s)
    else:
        p = (out[0] - 1) / z
        out.append(p)
        for j in range(1, 6):
            p = (p - 1 / mp.factorial(j)) / z
            out.append(p)
    return out


def _signed_log(rng, lo, hi, n):
    """n log-uniform |z| over [lo, hi), half of each sign."""
    a = np.exp(rng.uniform(math.log(lo), math.log(hi), n))
    a = np.clip(a, lo, np.nextafter(hi, 0))
    return a * np.where(np.arange(n) % 2, -1.0, 1.0)


def phi_inputs(rng):
    """Six blocks of 256 elements; a block is one wavefront at 4 values per lane, two at 2, four at 1.
    0: all |z| < 1/32.  1: all in [1/32, 1/2).  2: all in [1/2, 4).  3: all in [4, 750] and the clamp below -750.
    4: one big z among tiny ones (element 5).  5: one tiny z among big ones (element 70)."""
    t, h = 0.03125, 0.5
    b0 = np.concatenate([[0.0, -0.0, 1e-300, -1e-300, 5e-324, -5e-324, 2.0 ** -1030, np.nextafter(t, 0), -np.nextafter(t, 0)],
                         _signed_log(rng, 1e-12, t, 247)])
    b1 = np.concatenate([[t, -t, np.nextafter(t, 1), -np.nextafter(t, 1), np.nextafter(h, 0), -np.nextafter(h, 0)],
                         _signed_log(rng, t, h, 250)])
    b2 = np.concatenate([[h, -h, np.nextafter(h, 1), -np.nextafter(h, 1), 1.0, -1.0], _signed_log(rng, h, 1.0, 126),
                         _signed_log(rng, 1.0, 4.0, 124)])
    b3 = np.concatenate([[-750.0, np.nextafter(-750.0, 0), np.nextafter(-750.0, -1e3), -760.0, -800.0, -1000.0, -1e6, 700.0],
                         _signed_log(rng, 4.0, 40.0, 124), -np.exp(rng.uniform(math.log(40.0), math.log(750.0), 76)),
                         np.exp(rng.uniform(math.log(40.0), math.log(700.0), 48))])
    b4 = _signed_log(rng, 1e-8, t, 256)
    b4[5] = -3.0
    b5 = np.concatenate([_signed_log(rng, h, 4.0, 128), _signed_log(rng, 4.0, 300.0, 128)])
    b5[70] = 1.0e-3
    z = np.concatenate([b0, b1, b2, b3, b4, b5])
    assert z.shape == (1536,)
    return z


def part_phi(mp, rng):
    z = phi_inputs(rng)
    vals = [_phi_exact(mp, v) for v in z]
    hi = np.empty((len(z), 7))
    lo = np.empty((len(z), 7))
    for c in range(7):
        hi[:, c], lo[:, c] = dd(mp, [v[c] for v in vals])
    return {"phi_z": z, "phi_hi": hi, "phi_lo": lo}


def part_scan(mp, rng):
    """Four wavefronts of maps x -> a x + b with 0 < a <= 1, b > 0 (nothing cancels), and the exact serial composition."""
    a = rng.uniform(0.0, 1.0, (4, 64)) ** np.array([[0.02], [0.3], [1.0], [3.0]])
    a[0, ::7] = 1.0
    b = np.exp(rng.uniform(math.log(1e-3), math.log(1e3), (4, 64)))
    A, B = [], []
    for w in range(4):
        pa, pb = mp.mpf(1), mp.mpf(0)
        for l in range(64):
            pb = mp.mpf(a[w, l]) * pb + mp.mpf(b[w, l])
            pa = mp.mpf(a[w, l]) * pa
            A.append(pa)
            B.append(pb)
    out = {"scan_a": a.ravel(), "scan_b": b.ravel()}
    out["scan_a_hi"], out["scan_a_lo"] = dd(mp, A)
    out["scan_b_hi"], out["scan_b_lo"] = dd(mp, B)
    return out


LSE_K = 4


def part_lse(mp, rng):
    """Eight wavefronts of 64 lanes x LSE_K terms and ln sum e^term over each (-inf for the empty sum).
    0: all -inf.  1: one finite term.  2: one term 700 above the rest.  3: equal terms.  4 .. 7: normal draws of spread
    1, 10, 100 around -1000, 0, 300, and a wave that mixes -inf in."""
    n = 64 * LSE_K
    t = np.full((8, n), -np.inf)
    t[1, 137] = -12.25
    t[2] = rng.normal(-3.0, 1.0, n)
    t[2, 200] = 700.0 + t[2].max()
    t[3] = 1.7
    t[4] = rng.normal(-1000.0, 1.0, n)
    t[5] = rng.normal(0.0, 10.0, n)
    t[6] = rng.normal(300.0, 100.0, n)
    t[7] = np.where(rng.uniform(size=n) < 0.5, -np.inf, rng.normal(0.0, 3.0, n))
    vals = []
    for w in range(8):
        fin = [mp.mpf(v) for v in t[w] if np.isfinite(v)]
        vals.append(mp.log(sum(mp.exp(v) for v in fin)) if fin else mp.mpf("-inf"))
    hi = np.array([float(v) for v in vals])
    lo = np.array([float(v - mp.mpf(h)) if math.isfinite(h) else 0.0 for v, h in zip(vals, hi)])
    return {"lse_terms": t.ravel(), "lse_hi": hi, "lse_lo": lo}


def part_merge(mp, rng):
    """256 pairs of running sums (m, s), (mo, so) and ln(e^m s + e^mo so): empty operands on either side and on both."""
    n = 256
    m, mo = rng.normal(0.0, 30.0, n), rng.normal(0.0, 30.0, n)
    s, so = rng.uniform(1.0, 64.0, n), rng.uniform(1.0, 64.0, n)
    m[:4], s[:4] = -np.inf, 0.0
    mo[2:8], so[2:8] = -np.inf, 0.0
    mo[8:12] = m[8:12]
    mo[12:16] = m[12:16] + 720.0
    vals = []
    for i in range(n):
        tot = mp.mpf(0)
        for mm, ss in ((m[i], s[i]), (mo[i], so[i])):
            if ss != 0.0:
                tot += mp.exp(mp.mpf(mm)) * mp.mpf(ss)
        vals.append(mp.log(tot) if tot != 0 else mp.mpf("-inf"))
    hi = np.array([float(v) for v in vals])
    lo = np.array([float(v - mp.mpf(h)) if math.isfinite(h) else 0.0 for v, h in zip(vals, hi)])
    return {"merge_m": m, "merge_s": s, "merge_mo": mo, "merge_so": so, "merge_hi": hi, "merge_lo": lo}


def parts(group):
    """The arrays of one group; every group draws from a generator of its own, seeded with (SEED, index of the group)."""
    mp = _mp()
    rng = np.random.default_rng([SEED, GROUPS.index(group)])
    return globals()["part_" + group](mp, rng)


def main():
    mp = _mp()
    arrays = {}
    for g in GROUPS:
        arrays.update(parts(g))
    path = os.path.join(HERE, "golden_math.npz")
    np.savez_compressed(path, **arrays)
    mpath = os.path.join(HERE, "MANIFEST.json")
    man = json.load(open(mpath))
    man["golden_math.npz"] = {"generator": "tests/golden/make_math_golden.py", "seed": SEED, "mpmath": mp.__version__,
                              "precision_bits": PREC, "numpy": np.__version__,
                              "python": "%d.%d.%d" % sys.version_info[:3]}
    with open(mpath, "w") as f:
        json.dump(man, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

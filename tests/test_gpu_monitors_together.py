"""The sampler's four chain monitors on together (autocorrelation, posterior, thermodynamic sums, sample reservoir): what each
holds after a run equals, bit for bit, what it holds when it is the only one on, the walkers end where they end without any,
set_positions restarts all four, and the walker-sharded entry point refuses with the message of the first monitor that is on.
Exact equality is the bar because every monitor caps the chunks of mp_sampler_run by the same rule (mp_monitor.h
ChainMonitor::capped), so the run is cut into the same chunks alone and together, and the monitors share no buffer.
The unit Gaussian on an adapting ladder: no model is evaluated."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NW, ND, BETAS, ADAPT, STEPS, DISCARD, SEED = 8, 2, (1.0, 0.5, 0.25), 4, 12, 2, 20261020
NE = len(BETAS)
P0 = np.random.default_rng(SEED).standard_normal((NW * NE, ND))
ON = {
    "acf": lambda s: s.monitor_autocorr(max_lag=4, discard=DISCARD),
    "post": lambda s: s.monitor_posterior(bins=8, bins2=4, range=np.array([[-4.0, 4.0]] * ND), discard=DISCARD),
    "thermo": lambda s: s.monitor_thermo(discard=DISCARD),
    "res": lambda s: s.monitor_samples(size=16, discard=DISCARD),
}
OFF = {"acf": lambda s: s.monitor_autocorr(0), "post": lambda s: s.monitor_posterior(0), "thermo": lambda s: s.monitor_thermo(None),
       "res": lambda s: s.monitor_samples(None)}
NAMES = {"acf": "the autocorrelation monitor (mp_sampler_set_autocorr)", "post": "the posterior monitor (mp_sampler_set_posterior)",
         "thermo": "the thermodynamic monitor (mp_sampler_set_thermo)", "res": "the sample reservoir (mp_sampler_set_reservoir)"}


def read(s, name):
    """Everything monitor `name` of sampler s holds, as a flat dict of arrays."""
    out = {}
    if name == "acf":
        for e in range(NE):
            out.update({f"{k}{e}": np.asarray(v) for k, v in s.get_autocorr_sums(e).items()})
        tau, window, n = s.get_autocorr_device()
        out.update(tau=tau, window=window, n=np.asarray(n))
    elif name == "post":
        for e in range(NE):
            out.update({f"{k}{e}": np.asarray(v) for k, v in s.get_posterior(e).items() if v is not None})
    elif name == "thermo":
        out.update({k: np.asarray(v) for k, v in s.get_thermo().items()})
    else:
        for t in range(NE):
            out.update({f"{k}{t}": np.asarray(v) for k, v in s.get_samples(0, temp=t).items()})
    return out


def counters(s):
    """The four counters of a sampler with every monitor on: steps, samples, steps, samples."""
    return (s.get_autocorr_sums(0)["n"], s.get_posterior(0)["n"], s.get_thermo()["n_steps"], s.get_samples(0)["n_seen"])


def test_four_monitors_on_together_hold_what_each_holds_alone():
    from magprop_amd import EnsembleSampler, _capi

    def start(names):
        s = EnsembleSampler(NW, ND, target="gaussian", seed=SEED, betas=BETAS, adapt_ladder=ADAPT)
        for name in names:
            ON[name](s)
        return s, s.run_mcmc(P0, STEPS, store=False)

    four, pos = start(ON)
    assert four.get_chain() is None
    # the ladder froze at step ADAPT, behind the discard: the thermodynamic monitor counts from there
    assert counters(four) == (STEPS - DISCARD, (STEPS - DISCARD) * NW, STEPS - ADAPT, (STEPS - DISCARD) * NW)
    held = {name: read(four, name) for name in ON}
    assert held["post"]["hist10"].sum() > 0 and held["res"]["n_seen0"] > len(held["res"]["step0"]) == 16   # (rows were evicted)
    for name in ON:
        one, pos1 = start([name])
        alone = read(one, name)
        one.close()
        assert np.array_equal(pos1, pos), name
        assert alone.keys() == held[name].keys(), name
        for k, v in alone.items():
            w = held[name][k]
            assert v.dtype == w.dtype and np.array_equal(v, w, equal_nan=v.dtype.kind == "f"), (name, k)
    none, pos0 = start([])
    none.close()
    assert np.array_equal(pos0, pos)
    # set_positions restarts all four, and the discard applies again to the steps that follow
    four.set_positions(pos)
    assert counters(four) == (0, 0, 0, 0)
    four.run_mcmc(None, DISCARD + 1, store=False)
    assert counters(four) == (1, NW, 1, NW)
    four.close()

    # the walker-sharded entry point, which feeds no monitor: refused by each in turn, and by the first in feeding order of several
    s = EnsembleSampler(NW, ND, target="gaussian", seed=SEED)
    s.set_positions(P0[:NW])
    for names in [[name] for name in ON] + [["res", "thermo"], ["res", "thermo", "post", "acf"]]:
        for name in names:
            ON[name](s)
        with pytest.raises(_capi.MagpropAmdError):
            s.halfstep_shard(0, 0, s.n_slots, 0)
        first = min(names, key=list(ON).index)
        assert _capi.last_error() == f"mp_sampler_halfstep_shard: {NAMES[first]} is fed by mp_sampler_run only; turn it off first"
        for name in names:
            OFF[name](s)
    s.halfstep_shard(0, 0, 0, 0)                # (nothing on, an empty block of slots: no launch)
    s.close()

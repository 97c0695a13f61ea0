"""One small injection-recovery study on the GPU (magprop_amd.calibration.injection_study, run with -m gpu on an MI355X): 16
truths uniform in a narrow box around the Humped set, the reference's recipe (50 grid points, 25 % errors), 32 walkers per
dataset, the default moves; once with the chain stored and once through the device monitors alone.

Required, not measured: every batch converges; at least 90 of the 96 PIT values lie in [0.005, 0.995] (95 expected; a
calibrated fit gives fewer than 90 with probability about 2e-5); every |z-score| is below 6; the PIT from the monitor's
histograms agrees with the PIT from the stored chain to the stated resolution, the mass of the truth's bin.

Observed on an MI355X (profiles/r29_injection_study.json holds the same numbers): every dataset converged after 9 000 steps
(2 500 of them discarded), 96 of the 96 PIT values inside [0.005, 0.995], largest |z-score| 2.28, largest tau 37.4 steps, mean
acceptance 0.150, no truth redrawn; histogram PIT against stored-chain PIT: worst difference 3.6e-4, worst resolution 4.2e-3."""
import numpy as np
import pytest

from conftest import TRUTHS

pytestmark = pytest.mark.gpu

SPREAD = (0.3, 0.5, 0.3, 0.15, 0.3, 0.3)       # half widths of the truths' box around the Humped set, sampler coordinates
KW = dict(n_datasets=16, centre=TRUTHS["Humped"], spread=SPREAD, n_obs=50, frac_err=0.25, nwalkers=32, max_steps=20000,
          check_every=200, seed=29)


@pytest.fixture(scope="module")
def stored():
    from magprop_amd import calibration
    return calibration.injection_study(store=True, **KW)


def test_the_study_recovers_its_truths(stored):
    r = stored
    assert r.truths.shape == (16, 6) and r.y.shape == (16, 50) and not np.any(r.status)
    assert np.all(r.converged), (r.left_out, r.steps, r.tau)
    assert r.left_out == []
    inside = int(np.sum((r.pit >= 0.005) & (r.pit <= 0.995)))
    print(f"injection study: {inside} of {r.pit.size} PIT values inside, max |z| {np.max(np.abs(r.zscore)):.2f}, steps {r.steps[0]}, "
          f"tau max {np.max(r.tau):.1f}, acceptance {r.acceptance.mean():.3f}, redrawn {r.redrawn}")
    assert r.pit.size == 96 and inside >= 90
    assert np.all(np.abs(r.zscore) < 6.0)
    assert np.all(np.isfinite(r.tau)) and np.all((r.acceptance > 0.0) & (r.acceptance < 1.0))
    assert np.all(r.contraction <= 1.0) and np.all(r.n_samples == (r.steps[0] - r.discard) * 32)
    s = r.summarize()
    assert s["n"].tolist() == [16] * 6 and len(s["coverage"]) == 2


def test_the_histogram_path_agrees_with_the_stored_chain(stored):
    from magprop_amd import calibration
    r = stored
    assert np.all(np.abs(r.pit_hist - r.pit) <= r.pit_resolution + 1.0e-12), np.max(np.abs(r.pit_hist - r.pit) - r.pit_resolution)
    print(f"histogram PIT: worst difference {np.max(np.abs(r.pit_hist - r.pit)):.2e}, worst resolution {np.max(r.pit_resolution):.2e}")
    m = calibration.injection_study(store=False, **KW)             # the same seeds: the same chain, never on the host
    assert m.chains is None and np.all(m.converged) and np.array_equal(m.steps, r.steps)
    assert np.array_equal(m.pit, m.pit_hist) and np.array_equal(m.pit_hist, r.pit_hist)
    assert np.array_equal(m.y, r.y) and np.array_equal(m.truths, r.truths)
    assert np.allclose(m.mean, r.mean, rtol=0, atol=1.0e-9) and np.allclose(m.sd, r.sd, rtol=1.0e-6)

"""One population fitted to several data sets on the device (mcsas_hip_analyse_sets; csrc/chain_sets.h) against the float64
restatement tests/sets_exact.py and, with one set, against the existing wavefront kernel.  The inputs are sets_exact.case(...):
tests/test_sets_host.py holds every one of them to a decisive margin |X_t - X| / X >= 1e-9 at every step, so the device is asked
for the restatement's decisions.  Tolerances are those of the closed-form oracle in test_parity_gpu.py: num_iter, num_moves and
draws equal, contributions rtol 1e-12, chi² (overall and per set), scale, background and fit rtol 1e-9."""
import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import engine
from helpers import make_models
import sets_checks
import sets_exact as SX

pytestmark = pytest.mark.gpu


def _run(name, **st_kw):
    c = SX.case(name)
    return (c,) + sets_checks.run_case(c, **st_kw)


def _check(name, res, ref):
    sets_checks.check(name, res, ref)                        # (rtol 1e-9)


@pytest.mark.parametrize("name", ["s1_n5_bg", "s1_n5_nobg", "s1_n70_bg", "s1_n70_nobg"])
def test_one_set_is_the_existing_wavefront_kernel(name):
    """65 points (two slots, one nearly empty), 5 and 70 contributions (more than one wave of them), with and without a background:
    the chain of mcsas_hip_analyse in wave mode with cached rows, and the restatement's."""
    c, m, st, res = _run(name)
    q, I, sig = c["sets"][0]
    one = engine.analyse(m.setup(), q, I, sig, engine.Settings(**{**st.__dict__, "exec_mode": engine.EXEC_WAVE, "cache_intensities": 1}),
                         replay=c["replay"])
    for f in ("num_iter", "num_moves", "draws", "attempts", "converged"):
        assert np.array_equal(getattr(res, f), getattr(one, f)), f
    np.testing.assert_allclose(res.contribs, one.contribs, rtol=1e-12)
    for f in ("chisq", "scaling", "background", "fit"):
        np.testing.assert_allclose(getattr(res, f), getattr(one, f), rtol=1e-9, atol=1e-300, err_msg=f)
    np.testing.assert_allclose(res.set_chisq[0], one.chisq, rtol=1e-9)
    _check(name, res, SX.reference(name))


@pytest.mark.parametrize("name", ["b2", "b4"])
def test_set_boundaries_and_padding(name):
    """(37, 100) points: slots 1 + 2 of 4, one slot all padding; (64, 3, 63, 130): slots 1 + 1 + 1 + 3 of 8.  The sets are one
    population seen through scales a factor 1000 apart and different backgrounds: a shared scale or a slot counted to the wrong set
    cannot give the restatement's chain."""
    c, m, st, res = _run(name)
    ref = SX.reference(name)
    _check(name, res, ref)
    assert res.set_scaling[1, 0] / res.set_scaling[0, 0] > 500.


def test_a_row_with_an_integral():
    c, m, st, res = _run("cyl")
    _check("cyl", res, SX.reference("cyl"))


@pytest.mark.parametrize("name", ["end_crit", "end_retry", "end_odd"])
def test_where_the_loop_ends(name):
    """The criterion reached inside a batch of 64 proposals; a repetition that needs a further attempt, its draws going on in the
    stream; max_iter not a multiple of 64."""
    c, m, st, res = _run(name)
    ref = SX.reference(name)
    _check(name, res, ref)
    assert res.converged[0] == (0 if name == "end_odd" else 1)
    if name == "end_retry":
        assert res.attempts[0] >= 2


def test_a_free_running_repetition_is_the_same_alone_and_in_a_group():
    """Philox keyed by rep_offset + rep: repetition r of three at offset 3 is bit for bit the single repetition at offset 3 + r."""
    c = SX.case("b4")
    m, _ = make_models(c["tag"], c["lo"], c["hi"])
    kw = dict(n_contrib=20, max_iter=300, conv_crit=1e-12, max_retries=0, seed=77, device=0)
    group = engine.analyse_sets(m.setup(), c["sets"], engine.Settings(n_reps=3, rep_offset=3, **kw))
    assert len({int(x) for x in group.num_moves}) > 1 or not np.array_equal(group.contribs[:, :, 0], group.contribs[:, :, 1])
    for r in range(3):
        alone = engine.analyse_sets(m.setup(), c["sets"], engine.Settings(n_reps=1, rep_offset=3 + r, **kw))
        for f in ("contribs", "fit", "chisq", "scaling", "background", "num_iter", "num_moves", "draws", "attempts", "converged",
                  "set_scaling", "set_background", "set_chisq"):
            a, g = getattr(alone, f), getattr(group, f)
            assert np.array_equal(a[..., 0], g[..., r]), (f, r)
        assert alone.num_moves[0] > 5


def test_two_overlapping_ranges_through_the_front_end():
    """The quick-start tri-modal sphere population on two overlapping q ranges of 50 points, scales 1 and 250, different backgrounds,
    1 % noise: every repetition converges, each set's chi² is at most 1.5, the scales' ratio is within 5 % of 250, and calc() fills
    the histogram of member 0.  (tests/test_sets_host.py: the restatement converges on these inputs within maxIterations.)"""
    spec, sets = SX.quickstart_sets()
    lo, hi = np.pi / 1e9, np.pi / 1e7
    m, _ = make_models("sphere", [lo], [hi])
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=30, xscale='log', yweight='vol'))
    algo = mcsas_amd.McSAS(seed=11, device=0)
    algo.numContribs.setValue(100); algo.numReps.setValue(4); algo.convergenceCriterion.setValue(1.0)
    algo.model = m
    algo.data = mcsas_amd.DataSets([mcsas_amd.SASData(*s) for s in sets])
    algo.calc()
    assert len(algo.result) == 1
    r, d = algo.result[0], algo.details
    print("chi2", d.chisq, "per set", d.set_chisq, "scales", d.set_scaling, "steps", d.num_iter, "attempts", d.attempts)
    assert (d.converged == 1).all() and (d.chisq <= 1.0).all()
    assert (d.set_chisq <= 1.5).all()
    np.testing.assert_allclose(d.set_scaling[1] / d.set_scaling[0], 250., rtol=0.05)
    assert [s["slice"] for s in r["sets"]] == [slice(0, 50), slice(50, 100)] and r["fitMeasValMean"].shape == (1, 100)
    np.testing.assert_allclose(r["sets"][1]["scaling"][0] / r["sets"][0]["scaling"][0], 250., rtol=0.05)
    h = m.radius.histograms()[0]
    assert h.bins.mean.shape == (30,) and np.isfinite(h.bins.mean).all() and h.bins.mean.sum() > 0
    # the histogram's own scale fit for member 0 is the joint fit's for that member
    np.testing.assert_allclose(r["scalingFactors"][0], d.set_scaling[0], rtol=1e-6)


# ------------------------------------------------------------------------------------------------ McSAS.stop
def test_a_stop_word_set_before_the_call_ends_every_chain_at_its_first_poll():
    """What test_stop_flag_ends_the_run asks of the wavefront kernel, of the joint fit on (37, 100) points: no step, no retry."""
    import ctypes
    c = SX.case("b2")
    m, _ = make_models(c["tag"], c["lo"], c["hi"])
    st = engine.Settings(n_contrib=c["st"].n_contrib, n_reps=2, max_iter=10**9, conv_crit=0.0, max_retries=0, seed=1, device=0)
    res = engine.analyse_sets(m.setup(), c["sets"], st, stop=ctypes.c_int32(1))
    print("iter", res.num_iter, "converged", res.converged, "attempts", res.attempts)
    assert (res.num_iter == 0).all() and (res.converged == 0).all() and (res.attempts == 1).all()


# steps: without a stop the call below ends by this budget.  Measured on one MI355X (profiles/r30_summary.md): 39.3 s at 10**6 steps,
# 4.0 s at 10**5; the budget is the largest power of ten that stays below 5 s
STOP_BUDGET = 10**5


def _cylinder_chains(max_iter, stop):
    """Six free-running chains of 64 cylinders (the model and sets of test_a_row_with_an_integral) that never converge."""
    c = SX.case("cyl")
    m, _ = make_models(c["tag"], c["lo"], c["hi"], **c["fixed"])
    st = engine.Settings(n_contrib=64, n_reps=6, max_iter=max_iter, conv_crit=0.0, max_retries=0, seed=3, device=0)
    return engine.analyse_sets(m.setup(), c["sets"], st, stop=stop)


def test_a_stop_word_raised_while_the_chains_run_ends_them():
    """McSAS.stop raised from another thread 30 ms into the call, as test_stop_word_set_while_chains_with_an_integral_are_running
    does for plans: the host forwards the word while it waits, every chain leaves early, not converged, without another attempt.
    The budget ends the call if the word is never seen."""
    import ctypes, threading
    _cylinder_chains(64, None)                                # (library, memory and kernel warm: the timer below is about the run)
    stop = ctypes.c_int32(0)
    timer = threading.Timer(0.03, lambda: setattr(stop, "value", 1))
    timer.start()
    res = _cylinder_chains(STOP_BUDGET, stop)
    timer.cancel()
    print("iter", res.num_iter, "converged", res.converged, "attempts", res.attempts)
    assert (res.num_iter < STOP_BUDGET).all() and (res.converged == 0).all() and (res.attempts == 1).all()

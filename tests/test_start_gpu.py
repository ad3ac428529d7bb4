"""Chains started from given contributions (mcsas_hip_plan_set_start / mcsas_hip_analyse_from; engine.analyse(start=),
Plan.set_start, engine.analyse_batch "start" key, McSAS.calc(start=), run_series(start=)) on the device.

The reference of a started chain is the oracle's own mc_fit, unchanged: while it runs, generate_parameters is replaced so that its
FIRST call returns a copy of the start set (the rset of mcsas.py:317) and every later call — the per-step draws, the fresh sets of
retry attempts — goes to the real function (chain_cases._oracle_from).  That is the contract: the first attempt takes the given set and consumes no uniforms
for it; everything after is mcFit as it always was."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mcsas_amd
from mcsas_amd import engine, _lib
from oracle import mcsas_oracle as O
from helpers import make_models, plugin_twin
from chain_cases import (CASES, MCSAS_ESTREAM, R, RANGES, REP_OFFSET, _alone, _check_against_oracle, _same, _synthetic, _wave_retry_workload,
                         _workload)


def _started(wl, replay=None, **over):
    st = engine.Settings(**{**wl["st"].__dict__, **over})
    return engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st, replay=replay, start=wl["start"][:, :, 1:1 + R])


@pytest.mark.parametrize("name,cache", CASES)
def test_oracle_parity_from_a_start_replayed(name, cache):
    """Every repetition's replay row holds exactly the draws the oracle consumed from index 0 on (behind them: other numbers):
    MCSAS_OK, the oracle's chains, draws == num_iter * P.  The longest row one draw short: MCSAS_ESTREAM."""
    wl = _workload(name)
    P = wl["spec"].n_active
    res = _started(wl, replay=wl["replay"], cache_intensities=cache)
    _check_against_oracle(wl["chains"], res, P)
    assert np.array_equal(res.draws, res.num_iter * P) and (res.attempts == 1).all()
    with pytest.raises(_lib.McSASHipError) as e:
        _started(wl, replay=np.array(wl["replay"][:, :-1]), cache_intensities=cache)
    assert e.value.code == MCSAS_ESTREAM


@pytest.mark.parametrize("name,cache", CASES)
def test_oracle_parity_from_a_start_free_running(name, cache):
    """The same chains on the device's own Philox streams: chain REP_OFFSET + r from position 0."""
    wl = _workload(name)
    res = _started(wl, cache_intensities=cache)
    _check_against_oracle(wl["chains"], res, wl["spec"].n_active)


def test_plan_reads_its_own_columns_of_the_start():
    """Plan.set_start(contribs, rep_first): the five-column array, its outer columns NaN, read from column 1 on — and refused
    where the repetitions asked for reach a NaN or the array's end."""
    wl = _workload("sphere100")
    pl = engine.Plan(wl["setup"], wl["q"], wl["I"], wl["sig"], engine.Settings(**{**wl["st"].__dict__, "exec_mode": engine.EXEC_WAVE}))
    try:
        with pytest.raises(_lib.McSASHipError, match="not finite"):
            pl.set_start(wl["start"], rep_first=0)
        with pytest.raises(ValueError):
            pl.set_start(wl["start"], rep_first=3)
        pl.set_start(wl["start"], rep_first=1)
        for slot in (0, 1):                                                     # (every later launch of any slot)
            pl.launch(slot=slot)
            _check_against_oracle(wl["chains"], pl.fetch(slot=slot), 1)
    finally:
        pl.close()


# ----------------------------------------------------------------------------- retries
@pytest.mark.parametrize("cache", [1, 0])
def test_retries_after_a_started_attempt_draw_fresh_sets(cache):
    wl = _wave_retry_workload()
    st = engine.Settings(**{**wl["st"].__dict__, "cache_intensities": cache})
    res = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st, start=wl["start"])
    _check_against_oracle(wl["chains"], res, 1)
    L = max(c["pos"][-1] for c in wl["chains"])
    replay = np.stack([O.philox_uniform(wl["st"].seed, REP_OFFSET + r, np.arange(L, dtype=np.uint64)) for r in range(R)])
    again = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st, replay=replay, start=wl["start"])
    _same(again, res, "replayed")


# ----------------------------------------------------------------------------- a start that already meets the criterion
def test_a_converged_start_returns_itself():
    wl = _workload("sphere100")
    cold = engine.Settings(n_contrib=60, n_reps=R, max_iter=400, conv_crit=1e-9, max_retries=0, seed=21, exec_mode=engine.EXEC_WAVE)
    first = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], cold)
    assert (first.num_moves > 0).all()
    for from_min in (False, True):
        st = engine.Settings(n_contrib=60, n_reps=R, max_iter=400, conv_crit=1.5 * float(first.chisq.max()), max_retries=2, seed=22,
                             start_from_minimum=from_min)
        res = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st, start=first.contribs)
        assert np.array_equal(res.contribs, first.contribs)                     # bit for bit
        assert not res.num_iter.any() and not res.num_moves.any() and not res.draws.any()
        assert (res.converged == 1).all() and (res.attempts == 1).all()
        np.testing.assert_allclose(res.chisq, first.chisq, rtol=1e-7)


# ----------------------------------------------------------------------------- batches
def _batch_problems():
    """Four data sets of one model: 100 and 200 q-points (two q-slot classes), with and without a start in each class."""
    a, b = _workload("sphere100"), _workload("sphere200")
    out = []
    for k, (wl, with_start) in enumerate(((a, True), (b, False), (a, False), (b, True))):
        st = engine.Settings(**{**wl["st"].__dict__, "seed": 40 + k, "max_iter": 200, "conv_crit": 1e-9, "cache_intensities": k % 2})
        pr = dict(model=wl["setup"], q=wl["q"], intensity=wl["I"], sigma=wl["sig"], st=st)
        if with_start:
            pr["start"] = wl["start"][:, :, 1:1 + R]
        out.append(pr)
    return out


def _one(pr):
    if "start" not in pr:
        return _alone(pr)
    return engine.analyse(pr["model"], pr["q"], pr["intensity"], pr["sigma"], pr["st"], start=pr["start"])


def test_batch_of_started_and_cold_analyses():
    probs = _batch_problems()
    ones = [_one(pr) for pr in probs]
    assert all(int(o.num_moves.sum()) > 0 for o in ones)
    assert not np.array_equal(ones[0].contribs, _alone(probs[0]).contribs)       # (the start is not ignored)
    for i, g in enumerate(engine.analyse_batch(probs)):
        _same(g, ones[i], ("batch", i))
    for g, one in zip(engine.analyse_batch(probs[::-1])[::-1], ones):
        _same(g, one, "reversed")


def test_resident_plans_with_and_without_a_start_in_one_batch():
    probs = _batch_problems()
    ones = [_one(pr) for pr in probs]
    plans = [engine.Plan(pr["model"], pr["q"], pr["intensity"], pr["sigma"], engine.Settings(**{**pr["st"].__dict__, "exec_mode": engine.EXEC_WAVE}))
             for pr in probs]
    try:
        for pr, pl in zip(probs, plans):
            if "start" in pr:
                pl.set_start(pr["start"])
        engine.launch_batch(plans)
        for k, pl in enumerate(plans):
            _same(pl.fetch(), ones[k], ("plans", k))
        for pl in plans:
            pl.set_start(None)
        engine.launch_batch(plans)
        for k, pl in enumerate(plans):
            _same(pl.fetch(), _alone(probs[k]), ("plans, start cleared", k))
        plans[0].launch()
        _same(plans[0].fetch(), _alone(probs[0]), "own launch, start cleared")
    finally:
        for pl in plans:
            pl.close()


# ----------------------------------------------------------------------------- plug-ins, several devices
def test_plugin_model_with_a_start_equals_the_built_in_one():
    q, I, sig = _synthetic(100)
    lo, hi = RANGES["gausschain"]
    st = engine.Settings(n_contrib=24, n_reps=R, max_iter=150, conv_crit=1e-9, max_retries=0, seed=9, exec_mode=engine.EXEC_WAVE)
    res = []
    for as_plugin in (False, True):
        m, _ = make_models("gausschain", lo, hi)
        if as_plugin:
            plugin_twin(m, "gausschain")
        setup = m.setup()
        assert (setup.model_id >= engine.MODEL_PLUGIN0) == as_plugin
        if not res:
            start = engine.analyse(setup, q, I, sig, engine.Settings(**{**st.__dict__, "max_iter": 60, "seed": 8})).contribs
        res.append(engine.analyse(setup, q, I, sig, st, start=start))
        batch = engine.analyse_batch([dict(model=setup, q=q, intensity=I, sigma=sig, st=st, start=start)])[0]
        _same(batch, res[-1], ("batch kernel", as_plugin))
    assert int(res[0].num_moves.sum()) > 0
    _same(res[1], res[0], "plug-in against built-in")


def _algo(device=0, reps=R, crit=60.0, **kw):
    """Sphere, 60 contributions, a criterion cold chains reach in about a thousand steps (budget 4000)."""
    algo = mcsas_amd.McSAS.factory()(seed=17, device=device, **kw)
    algo.numContribs.setValue(60); algo.numReps.setValue(reps); algo.maxIterations.setValue(4000)
    algo.convergenceCriterion.setValue(crit); algo.maxRetries.setValue(1)
    lo, hi = RANGES["sphere"]
    algo.model, _ = make_models("sphere", lo, hi)
    algo.model.radius.histograms().append(mcsas_amd.Histogram(algo.model.radius, lo[0], hi[0], binCount=12, xscale='log', yweight='vol'))
    return algo


def _dataset(nq=100, scale=1.0):
    q, I, sig = _synthetic(nq)
    return mcsas_amd.SASData(q * scale, I, sig)


def test_device_list_with_a_start_equals_one_device():
    """McSAS(device=[0, 0]): three repetitions in blocks of two and one, each block reading its own columns of the start."""
    wl = _workload("sphere100")
    details = []
    for device in (0, [0, 0]):
        algo = _algo(device)
        algo.data = mcsas_amd.SASData(wl["q"], wl["I"], wl["sig"])
        algo.calc(start=wl["start"][:, :, 1:1 + R])
        details.append(algo.details)
    assert int(details[0].num_moves.sum()) > 0 and len({int(x) for x in details[0].num_moves}) > 1
    _same(details[1], details[0], "device list")


# ----------------------------------------------------------------------------- the front end
def test_calc_refines_its_own_result():
    algo = _algo(crit=100.0)
    algo.data = _dataset()
    algo.calc()
    before = algo.details
    assert (before.converged == 1).all() and len(algo.result) == 1
    start = algo.result[0]['contribs']
    algo.convergenceCriterion.setValue(50.0)                                    # the tighter criterion
    algo.calc(start=start)
    after = algo.details
    assert len(algo.result) == 1 and (after.converged == 1).all() and (after.attempts == 1).all()
    assert (after.num_moves > 0).all() and (after.chisq <= 50.0).all()
    # the chain only accepts improvements: chi² cannot rise, up to ft being summed again from the start's rows
    assert (after.chisq <= before.chisq * (1 + 1e-7)).all(), (after.chisq, before.chisq)
    h = algo.model.radius.histograms()[0]
    assert np.isfinite(h.bins.mean).all() and h.bins.mean.sum() > 0


def test_run_series_warm_started_from_the_previous_data_set():
    datasets = [_dataset(scale=s) for s in (1.0, 1.03, 1.06)]
    algo = _algo()
    results, series = mcsas_amd.run_series(algo, datasets, start="previous")
    assert all(r is not None for r in results) and len(series) == 1
    hand, prev = _algo(), None
    for i, d in enumerate(datasets):
        hand.data = d
        hand.calc(start=prev)
        prev = hand.result[0]['contribs']
        assert np.array_equal(results[i]['contribs'], prev), i
    cold = _algo()
    cold.data = datasets[1]
    cold.calc()
    assert not np.array_equal(cold.result[0]['contribs'], results[1]['contribs'])    # (the second data set did start warm)
    # one array for every data set; a list with a cold entry
    res_a, _ = mcsas_amd.run_series(_algo(), datasets[:2], start=results[0]['contribs'], batch=True)
    res_l, _ = mcsas_amd.run_series(_algo(), datasets[:2], start=[None, results[0]['contribs']])
    assert np.array_equal(res_a[1]['contribs'], res_l[1]['contribs']) and np.array_equal(res_l[0]['contribs'], results[0]['contribs'])


# ----------------------------------------------------------------------------- refusal on the device
def test_a_pipeline_plan_refuses_a_start_and_still_runs():
    wl = _workload("sphere100")
    st = engine.Settings(**{**wl["st"].__dict__, "exec_mode": engine.EXEC_PIPELINE, "max_iter": 100, "conv_crit": 1e-9})
    pl = engine.Plan(wl["setup"], wl["q"], wl["I"], wl["sig"], st)
    try:
        assert pl.info["exec_mode"] == "pipeline"
        with pytest.raises(_lib.McSASHipError, match="MCSAS_EXEC_PIPELINE") as e:
            pl.set_start(wl["start"], rep_first=1)
        assert e.value.code == -1 and "MCSAS_EXEC_WAVE" in str(e.value)
        pl.launch()
        got = pl.fetch()
    finally:
        pl.close()
    _same(got, engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st), "cold run after the refusal")

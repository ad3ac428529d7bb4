"""Chains started from given contributions (mcsas_hip_plan_set_start / mcsas_hip_analyse_from; engine.analyse(start=),
Plan.set_start, engine.analyse_batch "start" key, McSAS.calc(start=), run_series(start=)) on the device.

The reference of a started chain is the oracle's own mc_fit, unchanged: while it runs, generate_parameters is replaced so that its
FIRST call returns a copy of the start set (the rset of mcsas.py:317) and every later call — the per-step draws, the fresh sets of
retry attempts — goes to the real function.  That is the contract: the first attempt takes the given set and consumes no uniforms
for it; everything after is mcFit as it always was."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mcsas_amd
from mcsas_amd import engine, _lib
from oracle import mcsas_oracle as O
from helpers import make_models, plugin_twin
from test_batch_gpu import FIELDS, RANGES, _synthetic, _same, _alone

MCSAS_ESTREAM = -5
SEED, REP_OFFSET, R = 5, 3, 3


def _oracle_from(spec, q, I, sig, ost, start, stream, retries):
    """The retry loop of tests/test_chain_end_gpu.py::_oracle_chain with the first initial set given."""
    real, calls = O.generate_parameters, [0]

    def given_first(spec_, stream_, count=1):
        calls[0] += 1
        if calls[0] == 1:
            assert count == start.shape[0]
            return np.array(start, dtype=float)
        return real(spec_, stream_, count)

    lim = ([I.min(), I.max()], [q.min(), q.max()])
    iters, pos = [], []
    O.generate_parameters = given_first
    try:
        while True:
            ref = O.mc_fit(spec, q, I, sig, lim[0], lim[1], ost, stream, method="closed")
            iters.append(ref.num_iter); pos.append(stream.pos)
            if ref.conval <= ost.conv_crit or len(iters) > retries:
                break
    finally:
        O.generate_parameters = real
    assert calls[0] == 1 + sum(iters) + (len(iters) - 1)          # the start, one call per step, one per fresh set
    return dict(attempts=len(iters), iters=iters, pos=pos, ref=ref, converged=int(ref.conval <= ost.conv_crit))


# name: model, q-points, contributions, steps of the started run, steps of the cold run the start comes from, criterion (chosen with
# the oracle so that chains end mid-run), fixed model parameters
SHAPES = {
    "sphere100": ("sphere", 100, 60, 700, 150, 50.0, {}),
    "sphere200": ("sphere", 200, 60, 700, 150, 50.0, {}),
    "cyl100": ("cyl_aspect", 100, 24, 120, 40, 7000.0, {"intDiv": 12.}),
    "sphere1500": ("sphere", 1500, 16, 64, 20, 450.0, {}),          # 32 q slots per lane: a cache-only class
}


@functools.lru_cache(maxsize=None)
def _workload(name):
    """The start (a short cold run of the oracle: a realistic mid-fit state, one column per repetition, stored in columns 1..3 of
    a five-column array) and the oracle's started chains on the Philox streams of chains REP_OFFSET + r — the same numbers serve
    the replayed and the free-running run.  Computed once, shared, read-only."""
    tag, nq, N, steps, steps0, crit, fixed = SHAPES[name]
    q, I, sig = _synthetic(nq)
    m, spec = make_models(tag, *RANGES[tag], **fixed)
    lim = ([I.min(), I.max()], [q.min(), q.max()])
    cold = O.Settings(n_contrib=N, n_reps=1, max_iter=steps0, conv_crit=1e-9, max_retries=0)
    start = np.zeros((N, spec.n_active, 5))
    start[:, :, 0] = start[:, :, 4] = np.nan                                 # (columns a correct rep_first never reads)
    for r in range(R):
        start[:, :, 1 + r] = O.mc_fit(spec, q, I, sig, lim[0], lim[1], cold, O.PhiloxStream(11, r), method="closed").rset
    ost = O.Settings(n_contrib=N, n_reps=1, max_iter=steps, conv_crit=crit, max_retries=0)
    chains = [_oracle_from(spec, q, I, sig, ost, start[:, :, 1 + r], O.PhiloxStream(SEED, REP_OFFSET + r, pos=0), 0) for r in range(R)]
    P = spec.n_active
    for c in chains:
        assert c["attempts"] == 1 and c["pos"][-1] == P * c["iters"][0]         # no uniforms for the initial set
        assert c["ref"].num_moves > 0
    early = [c["iters"][0] for c in chains if c["iters"][0] < steps]
    assert early and all(c["converged"] for c in chains if c["iters"][0] < steps)   # a mid-run end that is not the budget
    assert len({c["iters"][0] for c in chains}) > 1
    L = max(c["pos"][-1] for c in chains)
    replay = np.stack([O.philox_uniform(SEED, REP_OFFSET + r, np.arange(L, dtype=np.uint64)) for r in range(R)])
    for r, c in enumerate(chains):                                             # what a chain did not consume: OTHER uniforms
        u = replay[r, c["pos"][-1]:]
        replay[r, c["pos"][-1]:] = np.where(u < 0.5, u + 0.25, u - 0.25)
    st = engine.Settings(n_contrib=N, n_reps=R, max_iter=steps, conv_crit=crit, max_retries=0, seed=SEED, rep_offset=REP_OFFSET)
    for a in (start, replay):
        a.setflags(write=False)
    return dict(setup=m.setup(), spec=spec, q=q, I=I, sig=sig, st=st, start=start, chains=chains, replay=replay)


def _check_against_oracle(chains, res, P):
    """The comparison of tests/test_chain_end_gpu.py::_check_against_oracle, fit and scaling included."""
    for r, c in enumerate(chains):
        ref = c["ref"]
        got = (res.num_iter[r], res.num_moves[r], res.attempts[r], res.converged[r], res.draws[r])
        print("chain %d: iter, moves, attempts, converged, draws = %s; oracle %s"
              % (r, got, (ref.num_iter, ref.num_moves, c["attempts"], c["converged"], c["pos"][-1])))
        assert got == (ref.num_iter, ref.num_moves, c["attempts"], c["converged"], c["pos"][-1]), r
        np.testing.assert_allclose(res.contribs[:, :, r], ref.rset, rtol=1e-12)
        np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-7)
        np.testing.assert_allclose(res.fit[:, r], ref.fit, rtol=1e-6, atol=1e-12 * np.abs(ref.fit).max())
        np.testing.assert_allclose(res.scaling[r], ref.scaling, rtol=1e-6)


def _started(wl, replay=None, **over):
    st = engine.Settings(**{**wl["st"].__dict__, **over})
    return engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st, replay=replay, start=wl["start"][:, :, 1:1 + R])


CASES = [("sphere100", 1), ("sphere100", 0), ("sphere200", 1), ("sphere200", 0), ("cyl100", 1), ("sphere1500", -1)]


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
@functools.lru_cache(maxsize=None)
def _retry_workload():
    """A start the chain cannot bring to the criterion within its budget (every contribution at one small radius), two retries.
    Seed and criterion chosen with the oracle: chains 0 and 2 converge in their second attempt, chain 1 in none of its three."""
    nq, N, steps, crit, seed = 100, 40, 300, 90.0, 3
    q, I, sig = _synthetic(nq)
    m, spec = make_models("sphere", *RANGES["sphere"])
    start = np.full((N, 1, R), 2e-9) * np.array([1.0, 1.5, 2.0])[None, None, :]
    ost = O.Settings(n_contrib=N, n_reps=1, max_iter=steps, conv_crit=crit, max_retries=2)
    chains = [_oracle_from(spec, q, I, sig, ost, start[:, :, r], O.PhiloxStream(seed, REP_OFFSET + r, pos=0), 2) for r in range(R)]
    assert [c["attempts"] for c in chains] == [2, 3, 2] and [c["converged"] for c in chains] == [1, 0, 1]
    for c in chains:                                                            # the started attempt ran to its budget, a retry WAS taken
        assert c["iters"][0] == steps and c["pos"][0] == steps                  # ... and the start cost no draws
        assert c["pos"][-1] == sum(c["iters"]) + N * (c["attempts"] - 1)        # N * P for each later initial set
    assert chains[0]["iters"][1] < steps and chains[2]["iters"][1] < steps      # converged mid-run in the later attempt
    st = engine.Settings(n_contrib=N, n_reps=R, max_iter=steps, conv_crit=crit, max_retries=2, seed=seed, rep_offset=REP_OFFSET)
    start.setflags(write=False)
    return dict(setup=m.setup(), spec=spec, q=q, I=I, sig=sig, st=st, start=start, chains=chains)


@pytest.mark.parametrize("cache", [1, 0])
def test_retries_after_a_started_attempt_draw_fresh_sets(cache):
    wl = _retry_workload()
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

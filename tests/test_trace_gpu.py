"""The accepted moves of wavefront-per-chain analyses (mcsas_hip_plan_set_trace / _fetch_trace / mcsas_hip_analyse_traced;
engine.analyse(trace=), Plan.set_trace, McSAS.calc(trace=)) on the device.

The reference is the oracle's own mc_fit, unchanged.  While it runs, two of the functions it calls are wrapped: generate_parameters
(as chain_cases._oracle_from wraps it: the first call may return a given start) records the proposal of every step,
and bgfit_calc records its conval call by call — the second call of an attempt is the chi² of the initial set (mcsas.py:343),
call 2 + s belongs to step s (mcsas.py:376).  ref.accepted names the steps of the moves; together: step, chi², values of every move.
(chain_cases._oracle_traced).  Tolerances are those of chain_cases._check_against_oracle: steps and counts exact, values rtol 1e-12, chi² rtol 1e-7."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mcsas_amd import engine, _lib
from oracle import mcsas_oracle as O
from helpers import _quickstart_algo, load, make_models, plugin_twin
from chain_cases import (CASES, K, MCSAS_EINVAL, R, RANGES, REP_OFFSET, SEED, SHAPES, _check_against_oracle, _check_trace, _guarded_trace,
                         _oracle_traced, _same, _same_trace, _synthetic, _traced_workload, _wave_retry_workload, _workload)


@functools.lru_cache(maxsize=None)
def _run(name, cache, started, replayed, trace):
    wl = _traced_workload(name, started)
    st = engine.Settings(**{**wl["st"].__dict__, "cache_intensities": cache, "exec_mode": engine.EXEC_WAVE})
    return engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st, replay=wl["replay"] if replayed else None, start=wl["start"],
                          trace=trace)


ALL = [(name, cache, started, replayed) for name, cache in CASES for started in (False, True) for replayed in (False, True)]


@pytest.mark.parametrize("name,cache,started,replayed", ALL)
def test_oracle_parity_of_the_trace(name, cache, started, replayed):
    wl = _traced_workload(name, started)
    res = _run(name, cache, started, replayed, K)
    _check_against_oracle(wl["chains"], res, wl["spec"].n_active)
    _check_trace(wl["chains"], res.trace, K)


@pytest.mark.parametrize("name,cache,started,replayed", ALL)
def test_the_trace_only_observes(name, cache, started, replayed):
    """The same call without a trace: every result array bit for bit."""
    traced, plain = _run(name, cache, started, replayed, K), _run(name, cache, started, replayed, None)
    assert traced.trace is not None and plain.trace is None and int(plain.num_moves.sum()) > 0
    _same(traced, plain, "traced against untraced")


@pytest.mark.parametrize("name,cache", CASES)
def test_the_records_rebuild_the_result(name, cache):
    """No oracle: the records written in order over the initial set, at row step % N, are the final parameter sets."""
    N = SHAPES[name][2]
    for started in (True, False):
        wl, res = _traced_workload(name, started), _run(name, cache, started, False, K)
        for r in range(R):
            if started:
                rset = np.array(wl["start"][:, :, r])
            else:                                       # the initial set of the chain: generateParameters(N) on its Philox stream
                rset = O.generate_parameters(wl["spec"], O.PhiloxStream(SEED, REP_OFFSET + r, pos=0), N)
            for i in range(int(res.trace.count[r])):
                rset[res.trace.step[i, r] % N] = res.trace.values[i, :, r]
            if started:
                assert np.array_equal(rset, res.contribs[:, :, r]), r
            else:
                np.testing.assert_allclose(rset, res.contribs[:, :, r], rtol=1e-12)


@pytest.mark.parametrize("capacity", [1, 3])
@pytest.mark.parametrize("started", [False, True])
def test_small_capacity_keeps_the_first_moves_and_writes_nothing_else(capacity, started):
    name, cache = "sphere100", 1
    wl, full = _traced_workload(name, started), _run(name, cache, started, False, K)
    P = wl["spec"].n_active
    st = engine.Settings(**{**wl["st"].__dict__, "cache_intensities": cache, "exec_mode": engine.EXEC_WAVE})
    prob = engine.HipProblem(wl["setup"], wl["q"], wl["I"], wl["sig"], st)
    res = engine.ChainResults(st.n_contrib, P, R, len(prob.q))
    t, big, where = _guarded_trace(capacity, P, R)
    lib = _lib.load()
    given = np.ascontiguousarray(wl["start"]) if started else None
    _lib.check(lib.mcsas_hip_analyse_traced(C.byref(prob.c), _lib.as_dp(given) if started else None, C.byref(res.c), C.byref(t)), lib)
    _same(res, full, "small capacity")
    got = {f: big[f][g:g + n] for f, (g, n) in where.items()}
    assert np.array_equal(got["count"], full.num_moves) and np.array_equal(got["count"], full.trace.count) and (got["count"] > capacity).all()
    assert np.array_equal(got["chisq0"], full.trace.chisq0)
    assert np.array_equal(got["step"].reshape(capacity, R), full.trace.step[:capacity])
    assert np.array_equal(got["chisq"].reshape(capacity, R), full.trace.chisq[:capacity])
    assert np.array_equal(got["values"].reshape(capacity, P, R), full.trace.values[:capacity])
    for f, (g, n) in where.items():                     # nothing on either side of the caller's arrays
        assert (big[f][:g] == big[f][0]).all() and (big[f][g + n:] == big[f][0]).all() and big[f][0] in (-77, -77.5), f
    # ... and through the Python front: the same records
    small = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st, start=wl["start"], trace=capacity)
    assert np.array_equal(small.trace.step, full.trace.step[:capacity]) and np.array_equal(small.trace.values, full.trace.values[:capacity])
    _check_trace(wl["chains"], small.trace, capacity)


@pytest.mark.parametrize("cache", [1, 0])
def test_retries_leave_the_trace_of_the_last_attempt(cache):
    """chain_cases._wave_retry_workload: a start the chain cannot bring to the criterion within its budget, two retries — chains 0 and
    2 converge in their second attempt, chain 1 in none of its three.  The first attempt's records are overwritten or dropped."""
    wl = _wave_retry_workload()
    st, N = wl["st"], wl["st"].n_contrib
    ost = O.Settings(n_contrib=N, n_reps=1, max_iter=st.max_iter, conv_crit=st.conv_crit, max_retries=2)
    chains = [_oracle_traced(wl["spec"], wl["q"], wl["I"], wl["sig"], ost, O.PhiloxStream(st.seed, REP_OFFSET + r, pos=0),
                             start=wl["start"][:, :, r], retries=2) for r in range(R)]
    assert [c["attempts"] for c in chains] == [2, 3, 2] and [c["iters"] for c in chains] == [c["iters"] for c in wl["chains"]]
    assert all(3 < c["ref"].num_moves < K for c in chains)
    st = engine.Settings(**{**st.__dict__, "cache_intensities": cache})
    res = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st, start=wl["start"], trace=K)
    _check_against_oracle(chains, res, 1)
    _check_trace(chains, res.trace, K)
    _same(res, engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st, start=wl["start"]), "traced against untraced")


def test_a_converged_start_leaves_an_empty_trace():
    wl = _workload("sphere100")
    cold = engine.Settings(n_contrib=60, n_reps=R, max_iter=400, conv_crit=1e-9, max_retries=0, seed=21, exec_mode=engine.EXEC_WAVE)
    first = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], cold)
    st = engine.Settings(n_contrib=60, n_reps=R, max_iter=400, conv_crit=1.5 * float(first.chisq.max()), max_retries=2, seed=22)
    res = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st, start=first.contribs, trace=5)
    assert np.array_equal(res.contribs, first.contribs) and not res.num_iter.any() and (res.attempts == 1).all()
    tr = res.trace
    assert not tr.count.any()
    np.testing.assert_allclose(tr.chisq0, res.chisq, rtol=1e-7)
    assert (tr.step == -1).all() and np.isnan(tr.chisq).all() and np.isnan(tr.values).all()


def test_plan_slots_reseed_clear_and_batch():
    wl = _traced_workload("sphere100", False)
    st = engine.Settings(**{**wl["st"].__dict__, "exec_mode": engine.EXEC_WAVE})
    one = _run("sphere100", -1, False, False, K)
    pl = engine.Plan(wl["setup"], wl["q"], wl["I"], wl["sig"], st)
    other = engine.Plan(wl["setup"], wl["q"], wl["I"], wl["sig"], engine.Settings(**{**st.__dict__, "seed": SEED + 1}))
    lib = pl.lib
    try:
        pl.launch()
        plain = pl.fetch()
        with pytest.raises(_lib.McSASHipError, match="no trace") as e:       # no trace yet
            pl.fetch_trace(capacity=K)
        assert e.value.code == MCSAS_EINVAL
        pl.set_trace(K)
        with pytest.raises(_lib.McSASHipError, match="no traced launch"):     # slot 0 holds the untraced launch
            pl.fetch_trace()
        # two slots, two seeds: each slot keeps its own trace
        pl.launch(slot=0)
        pl.reseed(SEED + 1, REP_OFFSET)
        pl.launch(slot=1)
        b = pl.fetch(slot=1)
        a = pl.fetch(slot=0)
        _same(a, plain, "slot 0"); _same(a, one, "slot 0 against the one-shot call"); _same_trace(a.trace, one.trace, "slot 0")
        assert not np.array_equal(b.trace.step, a.trace.step) and not np.array_equal(b.trace.values, a.trace.values)   # a reseed changes the trace
        assert np.array_equal(b.trace.count, b.num_moves) and (b.num_moves > 3).all()
        _same_trace(pl.fetch_trace(slot=0), a.trace, "slot 0 again, after slot 1 was fetched")
        with pytest.raises(_lib.McSASHipError, match="capacity") as e:
            pl.fetch_trace(capacity=K - 1)
        assert e.value.code == MCSAS_EINVAL
        # a batch refuses a traced plan and launches nothing; afterwards the plans still launch alone
        with pytest.raises(_lib.McSASHipError, match="launch_batch.*trace") as e:
            engine.launch_batch([other, pl])
        assert e.value.code == MCSAS_EINVAL
        pl.launch(); other.launch()
        again, o = pl.fetch(), other.fetch()
        _same(again, b, "own launch after the refused batch"); _same_trace(again.trace, b.trace)
        _same(o, b, "the untraced plan with the same seed")
        assert o.trace is None
        # cleared: no trace to fetch, the untraced kernel's results
        pl.set_trace(0)
        pl.reseed(SEED, REP_OFFSET)
        pl.launch()
        cleared = pl.fetch()
        assert cleared.trace is None
        _same(cleared, plain, "trace cleared")
        tr = engine.ChainTrace(K, 1, R)
        assert lib.mcsas_hip_plan_fetch_trace(pl.h, 0, C.byref(tr.c)) == MCSAS_EINVAL
        engine.launch_batch([other, pl])                                        # ... and a batch takes the plan again
        _same(pl.fetch(), plain, "batch after the trace was cleared")
    finally:
        pl.close(); other.close()


def test_plans_of_other_modes_refuse_a_trace_and_still_run():
    wl = _traced_workload("sphere100", False)
    for mode, name in ((engine.EXEC_PIPELINE, "MCSAS_EXEC_PIPELINE"), (engine.EXEC_WORKGROUP, "MCSAS_EXEC_WORKGROUP")):
        st = engine.Settings(**{**wl["st"].__dict__, "exec_mode": mode, "max_iter": 100, "conv_crit": 1e-9})
        pl = engine.Plan(wl["setup"], wl["q"], wl["I"], wl["sig"], st)
        try:
            with pytest.raises(_lib.McSASHipError, match=name) as e:
                pl.set_trace(K)
            assert e.value.code == MCSAS_EINVAL and "MCSAS_EXEC_WAVE" in str(e.value) and pl.trace_capacity == 0
            pl.launch()
            got = pl.fetch()
        finally:
            pl.close()
        assert got.trace is None
        _same(got, engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st), "cold run after the refusal")


def test_plugin_model_gives_the_trace_of_the_built_in_one():
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
        res.append((engine.analyse(setup, q, I, sig, st, trace=K), engine.analyse(setup, q, I, sig, st, start=start, trace=K)))
    for k, what in enumerate(("cold", "started")):
        assert (res[0][k].trace.count > 3).all() and (res[0][k].trace.count < K).all()
        _same(res[1][k], res[0][k], what); _same_trace(res[1][k].trace, res[0][k].trace, what)


def test_calc_stores_the_trace():
    g = load("g13_quickstart.npz")
    reps, cap = 4, 4096
    algo, m = _quickstart_algo(g, reps, 77)
    algo.calc(trace=cap)
    tr, d = algo.result[0]["trace"], algo.details
    P = 1
    assert set(tr) == {"count", "chisq0", "step", "chisq", "values"}
    assert tr["count"].shape == (reps,) and tr["chisq0"].shape == (reps,) and tr["step"].shape == (cap, reps)
    assert tr["chisq"].shape == (cap, reps) and tr["values"].shape == (cap, P, reps)
    assert np.array_equal(tr["count"], d.num_moves) and (d.converged == 1).all()
    checked = 0
    for r in range(reps):
        n = int(tr["count"][r])
        if n <= cap:
            np.testing.assert_allclose(tr["chisq"][n - 1, r], d.chisq[r], rtol=1e-7)
            checked += 1
    assert checked > 0
    contribs = algo.result[0]["contribs"]
    plain, _ = _quickstart_algo(g, reps, 77)
    plain.execMode = engine.EXEC_WAVE
    plain.calc()
    assert "trace" not in plain.result[0]
    assert np.array_equal(plain.result[0]["contribs"], contribs)
    # ... and with a start: the tighter criterion, from the result
    algo.convergenceCriterion.setValue(0.9)
    algo.calc(start=contribs, trace=16)
    tr2 = algo.result[0]["trace"]
    assert tr2["step"].shape == (16, reps) and np.array_equal(tr2["count"], algo.details.num_moves) and tr2["count"].any()
    assert (tr2["chisq0"] <= d.chisq * (1 + 1e-7)).all()                     # the refined run starts where the first one ended

"""Chains of the q-split workgroup kernel (csrc/chain_wide.h: more than 1024 q-points, one workgroup per chain) started from given
contributions: chain_wide_kernel<M, QPL, true> behind mcsas_hip_analyse_from / mcsas_hip_plan_set_start with MCSAS_EXEC_WORKGROUP, and
behind McSAS.calc(start=) on un-binned data.

The machinery is tests/test_start_gpu.py's (chain_cases.py): the reference of a started chain is the oracle's own mc_fit with its first
generate_parameters call answered by the start (_oracle_from), compared with that file's tolerances (_check_against_oracle: counts
exact, contribs 1e-12, chi-squared 1e-7, fit and scaling 1e-6).

Shapes: the smallest at which each instantiation can go wrong — 8 slots per lane at 1500 q (three waves; the workload of
test_start_gpu.py) and at 1025 q (the third wave holds one real point), 16 slots at 4097 q, 32 slots at 8193 q (five waves, the last
with one real point).  Steps and criteria were chosen with the oracle so that chains end mid-run by convergence, at different steps,
each after an accepted move (_workload asserts it), and with a margin: a criterion 10 lower ends every chain at the same step, so no
chain's end sits on a numerically tied comparison.  Should a free-running chain ever do, the seed is what changes, not a tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mcsas_amd
from mcsas_amd import engine, _lib
from oracle import mcsas_oracle as O
from helpers import make_models, plugin_twin, product_smearing
from chain_cases import (GEOMETRY, MCSAS_ESTREAM, R, RANGES, REP_OFFSET, WG, _check_against_oracle, _same, _synthetic, _wide_retry_workload,
                         _workload)


def _settings(wl, **over):
    return engine.Settings(**{**wl["st"].__dict__, "exec_mode": WG, **over})


def _started(wl, replay=None, **over):
    return engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], _settings(wl, **over), replay=replay, start=wl["start"][:, :, 1:1 + R])


def _info(wl, **over):
    pl = engine.Plan(wl["setup"], wl["q"], wl["I"], wl["sig"], _settings(wl, **over))
    try:
        return pl.info
    finally:
        pl.close()


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_oracle_parity_from_a_start_replayed(name):
    """Every repetition's replay row holds exactly the draws the oracle consumed from index 0 on (behind them: other numbers):
    MCSAS_OK, the oracle's chains, draws == num_iter * P (the chain-end contract).  The longest row one draw short: MCSAS_ESTREAM."""
    wl = _workload(name)
    info = _info(wl)
    assert info["exec_mode"] == "workgroup" and (info["q_per_lane"], info["waves_per_chain"]) == GEOMETRY[name], info
    P = wl["spec"].n_active
    res = _started(wl, replay=wl["replay"])
    _check_against_oracle(wl["chains"], res, P)
    assert np.array_equal(res.draws, res.num_iter * P) and (res.attempts == 1).all()
    with pytest.raises(_lib.McSASHipError) as e:
        _started(wl, replay=np.array(wl["replay"][:, :-1]))
    assert e.value.code == MCSAS_ESTREAM


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_oracle_parity_from_a_start_free_running(name):
    """The same chains on the device's own Philox streams: chain REP_OFFSET + r from position 0."""
    wl = _workload(name)
    assert wl["st"].rep_offset == REP_OFFSET != 0
    _check_against_oracle(wl["chains"], _started(wl), wl["spec"].n_active)


def test_plan_slots_read_their_columns_and_a_cleared_start_runs_cold():
    """Plan.set_start(contribs, rep_first = 1) on the five-column array whose outer columns are NaN: every later launch of either
    slot starts from columns 1..3; set_start(None) gives the cold result again."""
    wl = _workload("sphere1025")
    cold = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], _settings(wl))
    pl = engine.Plan(wl["setup"], wl["q"], wl["I"], wl["sig"], _settings(wl))
    try:
        with pytest.raises(_lib.McSASHipError, match="not finite"):
            pl.set_start(wl["start"], rep_first=0)
        pl.set_start(wl["start"], rep_first=1)
        for slot in (0, 1):
            pl.launch(slot=slot)
            started = pl.fetch(slot=slot)
            _check_against_oracle(wl["chains"], started, 1)
        pl.set_start(None)
        pl.launch()
        again = pl.fetch()
    finally:
        pl.close()
    assert not np.array_equal(cold.contribs, started.contribs)                  # (a started run is not the cold one)
    _same(again, cold, "start cleared")


def test_retries_after_a_started_attempt_draw_fresh_sets():
    wl = _wide_retry_workload()
    res = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], wl["st"], start=wl["start"])
    _check_against_oracle(wl["chains"], res, 1)
    L = max(c["pos"][-1] for c in wl["chains"])
    replay = np.stack([O.philox_uniform(wl["st"].seed, REP_OFFSET + r, np.arange(L, dtype=np.uint64)) for r in range(R)])
    again = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], wl["st"], replay=replay, start=wl["start"])
    _same(again, res, "replayed")


def test_a_converged_start_returns_itself():
    wl = _workload("sphere1025")
    cold = engine.Settings(n_contrib=16, n_reps=R, max_iter=40, conv_crit=1e-9, max_retries=0, seed=21, exec_mode=WG)
    first = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], cold)
    assert (first.num_moves > 0).all()
    for from_min in (False, True):
        st = engine.Settings(n_contrib=16, n_reps=R, max_iter=40, conv_crit=1.5 * float(first.chisq.max()), max_retries=2, seed=22,
                             start_from_minimum=from_min, exec_mode=WG)
        res = engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st, start=first.contribs)
        assert np.array_equal(res.contribs, first.contribs)                     # bit for bit
        assert not res.num_iter.any() and not res.num_moves.any() and not res.draws.any()
        assert (res.converged == 1).all() and (res.attempts == 1).all()
        np.testing.assert_allclose(res.chisq, first.chisq, rtol=1e-7)


@pytest.mark.parametrize("tag", ["cyl_aspect", "smeared_sphere"])
def test_started_q_split_run_equals_the_started_wave_run(tag):
    """A model with an integral (isotropic cylinders, intDiv 12) and a smeared sphere at 1025 q-points, which the wave kernel still
    takes: both kernels started from the same set decide the same, and their sums agree to the bound test_wide_flags_gpu.py holds
    the two kernels to (1e-10: the q-split kernel adds a chain's weighted sums per wave first)."""
    q, I, sig = _synthetic(1025)
    smear = None
    if tag == "cyl_aspect":
        m, _ = make_models("cyl_aspect", *RANGES["cyl_aspect"], intDiv=12.)
    else:
        m, _ = make_models("sphere", *RANGES["sphere"])
        _, smear = product_smearing("trapezoid", False, 9, q, I, sig, umbra=2e-3 * q.max(), penumbra=4e-3 * q.max())
    setup = m.setup()
    st = engine.Settings(n_contrib=12, n_reps=R, max_iter=40, conv_crit=1e-9, max_retries=0, seed=9, exec_mode=engine.EXEC_WAVE)
    start = engine.analyse(setup, q, I, sig, engine.Settings(**{**st.__dict__, "max_iter": 16, "seed": 8}), smear=smear).contribs
    wave = engine.analyse(setup, q, I, sig, st, smear=smear, start=start)
    wide = engine.analyse(setup, q, I, sig, engine.Settings(**{**st.__dict__, "exec_mode": WG}), smear=smear, start=start)
    assert (wave.num_moves > 0).all() and np.array_equal(wave.draws, wave.num_iter * setup.n_active)
    for name in ("num_iter", "num_moves", "attempts", "draws", "converged", "contribs"):
        np.testing.assert_array_equal(getattr(wide, name), getattr(wave, name), err_msg=name)
    for name in ("chisq", "fit"):
        np.testing.assert_allclose(getattr(wide, name), getattr(wave, name), rtol=1e-10, err_msg=name)


def test_plugin_model_with_a_start_equals_the_built_in_one():
    q, I, sig = _synthetic(1025)
    lo, hi = RANGES["gausschain"]
    st = engine.Settings(n_contrib=16, n_reps=R, max_iter=48, conv_crit=1e-9, max_retries=0, seed=9, exec_mode=WG)
    res = []
    for as_plugin in (False, True):
        m, _ = make_models("gausschain", lo, hi)
        if as_plugin:
            plugin_twin(m, "gausschain")
        setup = m.setup()
        assert (setup.model_id >= engine.MODEL_PLUGIN0) == as_plugin
        if not res:
            start = engine.analyse(setup, q, I, sig, engine.Settings(**{**st.__dict__, "max_iter": 16, "seed": 8})).contribs
        res.append(engine.analyse(setup, q, I, sig, st, start=start))
    assert int(res[0].num_moves.sum()) > 0
    _same(res[1], res[0], "plug-in against built-in")


def test_device_list_with_a_start_equals_one_device():
    """Device 0 listed twice: three repetitions in blocks of two and one, each block reading its own columns of the start."""
    wl = _workload("sphere4097")
    one = _started(wl)
    two = _started(wl, devices=(0, 0))
    assert len({int(x) for x in one.num_iter}) > 1
    _same(two, one, "device list")


def test_calc_refines_its_own_result_on_unbinned_data():
    """McSAS.calc() on 4097 points, then calc(start=) of its own result under a tighter criterion with execMode left at AUTO: the
    front end asks for the workgroup mode itself (no other kernel takes the data), and no chain ends above where it started."""
    q, I, sig = _synthetic(4097)
    algo = mcsas_amd.McSAS.factory()(seed=17, device=0)
    algo.numContribs.setValue(16); algo.numReps.setValue(R); algo.maxIterations.setValue(300)
    algo.convergenceCriterion.setValue(1500.0); algo.maxRetries.setValue(1)
    algo.model, _ = make_models("sphere", *RANGES["sphere"])
    algo.data = mcsas_amd.SASData(q, I, sig)
    assert algo.data.count == 4097 and algo.execMode == engine.EXEC_AUTO
    algo.calc()
    before = algo.details
    assert (before.converged == 1).all() and len(algo.result) == 1
    start = algo.result[0]['contribs']
    algo.convergenceCriterion.setValue(600.0)                                   # the tighter criterion
    assert algo._problem(start=start)["st"].exec_mode == WG
    algo.calc(start=start)
    after = algo.details
    assert (after.attempts >= 1).all() and (after.num_moves > 0).all()
    # the chain only accepts improvements: chi² cannot rise, up to ft being summed again from the start's rows
    assert (after.chisq <= before.chisq * (1 + 1e-7)).all(), (after.chisq, before.chisq)


def test_a_workgroup_window_plan_refuses_a_start_and_still_runs():
    """Up to 1024 q-points MCSAS_EXEC_WORKGROUP is the workgroup-window kernel, which has no start form."""
    q, I, sig = _synthetic(512)
    m, _ = make_models("sphere", *RANGES["sphere"])
    st = engine.Settings(n_contrib=60, n_reps=R, max_iter=100, conv_crit=1e-9, max_retries=0, seed=5, exec_mode=WG)
    pl = engine.Plan(m.setup(), q, I, sig, st)
    try:
        assert pl.info["exec_mode"] == "workgroup" and pl.info["window"] > 1
        with pytest.raises(_lib.McSASHipError, match="MCSAS_EXEC_WORKGROUP") as e:
            pl.set_start(np.full((60, 1, R), 5e-8))
        assert e.value.code == -1 and "MCSAS_EXEC_WAVE" in str(e.value) and "1024" in str(e.value)
        pl.launch()
        got = pl.fetch()
    finally:
        pl.close()
    _same(got, engine.analyse(m.setup(), q, I, sig, st), "cold run after the refusal")

"""One population fitted to several data sets with ONE scale for all of them, on the device (mcsas_hip_analyse_sets_mode with
MCSAS_SETS_SCALE_SHARED; csrc/chain_sets.h: chain_sets_kernel<M, QPL, true>) against the float64 restatement tests/sets_shared_exact.py, and
against the per-set kernel where the two must agree bit for bit.  The inputs are sets_shared_exact.case(...):
tests/test_sets_shared_host.py holds every one of them to a decisive margin |X_t - X| / X >= 1e-9 at every step, so the device is
asked for the restatement's decisions.  Tolerances are tests/test_sets_gpu.py's for the same quantities: num_iter, num_moves, draws
and attempts equal, contributions rtol 1e-12, chi² (overall and per set), scale, background and fit rtol 1e-9."""
import numpy as np
import pytest

from mcsas_amd import engine
from helpers import make_models
import sets_exact as SX
import sets_shared_exact as SH

pytestmark = pytest.mark.gpu

FIELDS = ("contribs", "fit", "chisq", "scaling", "background", "num_iter", "num_moves", "draws", "attempts", "converged",
          "set_scaling", "set_background", "set_chisq")


def _settings(c, **kw):
    ost = c["st"]
    return engine.Settings(n_contrib=ost.n_contrib, n_reps=1, max_iter=ost.max_iter, comp_exp=ost.comp_exp, conv_crit=ost.conv_crit,
                           find_background=ost.find_bg, max_retries=ost.max_retries, device=0, **kw)


def _run(c, scale):
    m, _ = make_models(c["tag"], c["lo"], c["hi"], **c["fixed"])
    return engine.analyse_sets(m.setup(), c["sets"], _settings(c), replay=c["replay"], scale=scale)


@pytest.mark.parametrize("name", tuple(SH.REPLAY_SEED))          # (the generated inputs: tests/test_sets_matrix_gpu.py)
def test_against_the_restatement(name):
    """(37, 100) points: slots 1 + 2 of 4; (64, 3, 63, 130): 1 + 1 + 1 + 3 of 8; a row with an integral; no background; max_iter not a
    multiple of 64; a repetition that needs a further attempt."""
    c = SH.case(name)
    res, ref = _run(c, "shared"), SH.reference(name)
    got = (res.num_iter[0], res.num_moves[0], res.draws[0], res.attempts[0])
    print(name, "iter, moves, draws, attempts =", got, "restatement", (ref.num_iter, ref.num_moves, ref.draws, ref.attempts),
          "chi2", res.chisq[0], ref.conval, "per set", res.set_chisq[:, 0], ref.set_chisq, "scale", res.set_scaling[:, 0], ref.set_scaling)
    assert got == (ref.num_iter, ref.num_moves, ref.draws, ref.attempts)
    np.testing.assert_allclose(res.contribs[:, :, 0], ref.rset, rtol=1e-12)
    np.testing.assert_allclose(res.chisq[0], ref.conval, rtol=1e-9)
    np.testing.assert_allclose(res.set_chisq[:, 0], ref.set_chisq, rtol=1e-9)
    np.testing.assert_allclose(res.set_scaling[:, 0], ref.set_scaling, rtol=1e-9)
    np.testing.assert_allclose(res.set_background[:, 0], ref.set_background, rtol=1e-9, atol=1e-300)
    np.testing.assert_allclose(res.fit[:, 0], ref.fit, rtol=1e-9)
    assert (res.set_scaling[:, 0] == res.set_scaling[0, 0]).all()                           # all sets report one scaling
    assert res.scaling[0] == res.set_scaling[0, 0] and res.background[0] == res.set_background[0, 0]
    if name == "sh_nobg":
        assert (res.set_background == 0.).all()
    if name == "sh_end_retry":
        assert res.attempts[0] >= 2 and res.converged[0] == 1
    if name == "sh_end_odd":
        assert res.converged[0] == 0


@pytest.mark.parametrize("name", ["s1_n5_bg", "s1_n70_nobg"])
def test_with_one_set_the_modes_are_the_same_chain_bit_for_bit(name):
    c = SX.case(name)
    a, b = _run(c, "per_set"), _run(c, "shared")
    assert a.num_moves[0] > 3
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_mode_zero_is_analyse_sets_bit_for_bit():
    """mcsas_hip_analyse_sets_mode(..., 0, ...) against mcsas_hip_analyse_sets itself on b4, through the library"""
    import ctypes as C
    from mcsas_amd import _lib
    c = SX.case("b4")
    m, _ = make_models(c["tag"], c["lo"], c["hi"])
    lib = _lib.load()
    out = []
    for mode in (None, 0):
        cat = [np.concatenate([np.asarray(t[k], dtype=float) for t in c["sets"]]) for k in range(3)]
        prob = engine.HipProblem(m.setup(), cat[0], cat[1], cat[2], _settings(c), c["replay"], None, None)
        res = engine.SetsResults(c["st"].n_contrib, 1, 1, [len(t[0]) for t in c["sets"]])
        nqp = res.set_nq.ctypes.data_as(C.POINTER(C.c_int32))
        if mode is None:
            _lib.check(lib.mcsas_hip_analyse_sets(C.byref(prob.c), 4, nqp, C.byref(res.c), C.byref(res.sets_c)), lib)
        else:
            _lib.check(lib.mcsas_hip_analyse_sets_mode(C.byref(prob.c), 4, nqp, mode, C.byref(res.c), C.byref(res.sets_c)), lib)
        out.append(res)
    assert out[0].num_moves[0] > 3
    for f in FIELDS:
        assert np.array_equal(getattr(out[0], f), getattr(out[1], f)), f


def test_free_running_repetitions_are_the_same_alone_and_in_a_group_of_64():
    """Philox keyed by rep_offset + rep: repetitions 5 and 40 of 64 are bit for bit the single repetitions at those offsets"""
    c = SH.case("sh4")
    m, _ = make_models(c["tag"], c["lo"], c["hi"])
    kw = dict(n_contrib=20, max_iter=300, conv_crit=1e-12, max_retries=0, seed=77, device=0)
    group = engine.analyse_sets(m.setup(), c["sets"], engine.Settings(n_reps=64, **kw), scale="shared")
    assert not np.array_equal(group.contribs[:, :, 5], group.contribs[:, :, 40])
    for r in (5, 40):
        alone = engine.analyse_sets(m.setup(), c["sets"], engine.Settings(n_reps=1, rep_offset=r, **kw), scale="shared")
        for f in FIELDS:
            a, g = getattr(alone, f), getattr(group, f)
            assert np.array_equal(a[..., 0], g[..., r]), (f, r)
        assert alone.num_moves[0] > 5


def test_one_scale_cannot_follow_a_set_that_is_three_times_stronger():
    """sh2 with the second set's intensities times 3 (its uncertainties as they were): a scale per set absorbs the factor, one shared scale
    cannot — it ends at a higher chi², and reports one scale where the per-set mode reports two a factor 3 apart."""
    c = SH.case("sh2")
    (q0, I0, s0), (q1, I1, s1) = c["sets"]
    sets = [(q0, I0, s0), (q1, 3. * I1, s1)]
    m, _ = make_models(c["tag"], c["lo"], c["hi"])
    st = _settings(c, seed=5)
    per = engine.analyse_sets(m.setup(), sets, st, scale="per_set")
    sh = engine.analyse_sets(m.setup(), sets, st, scale="shared")
    print("chi2 per set", per.chisq[0], "shared", sh.chisq[0], "scales", per.set_scaling[:, 0], sh.set_scaling[:, 0])
    assert sh.chisq[0] > per.chisq[0]
    assert sh.set_scaling[0, 0] == sh.set_scaling[1, 0]
    assert 2. < per.set_scaling[1, 0] / per.set_scaling[0, 0] < 4.

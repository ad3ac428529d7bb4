"""Shared by the GPU test modules of the joint fit (test_sets_gpu.py, test_sets_matrix_gpu.py): one device run of a named input of
sets_exact.case / sets_shared_exact.case and its comparison with the restatement's chain.  A plain module like helpers.py: nothing
in here is collected.

Tolerances are those of the closed-form oracle in test_parity_gpu.py: num_iter, num_moves, draws and attempts equal, contributions
rtol 1e-12, chi² (overall and per set), scale, background and fit rtol 1e-9."""
import numpy as np

from mcsas_amd import engine
import sets_exact as SX

FIELDS = ("contribs", "fit", "chisq", "scaling", "background", "num_iter", "num_moves", "draws", "attempts", "converged",
          "set_scaling", "set_background", "set_chisq")


def settings(c, **st_kw):
    ost = c["st"]
    return engine.Settings(**{**dict(n_contrib=ost.n_contrib, n_reps=1, max_iter=ost.max_iter, comp_exp=ost.comp_exp, conv_crit=ost.conv_crit,
                                     find_background=ost.find_bg, start_from_minimum=ost.start_from_min, max_retries=ost.max_retries,
                                     device=0), **st_kw})


def run_case(c, scale="per_set", **st_kw):
    """-> (product model, settings, the device's result) of a case() dict"""
    m, _ = SX.case_models(c)
    st = settings(c, **st_kw)
    return m, st, engine.analyse_sets(m.setup(), c["sets"], st, replay=c["replay"], scale=scale)


def check(name, res, ref, rtol=1e-9):
    """`rtol` of the fitted quantities: 1e-9, wider only where a model's device row is held to its oracle less tightly (derived there)."""
    got = (res.num_iter[0], res.num_moves[0], res.draws[0], res.attempts[0])
    print(name, "iter, moves, draws, attempts =", got, "restatement", (ref.num_iter, ref.num_moves, ref.draws, ref.attempts),
          "chi2", res.chisq[0], ref.conval, "per set", res.set_chisq[:, 0], ref.set_chisq, "scale", res.set_scaling[:, 0], ref.set_scaling)
    assert got == (ref.num_iter, ref.num_moves, ref.draws, ref.attempts)
    np.testing.assert_allclose(res.contribs[:, :, 0], ref.rset, rtol=1e-12)
    np.testing.assert_allclose(res.chisq[0], ref.conval, rtol=rtol)
    np.testing.assert_allclose(res.set_chisq[:, 0], ref.set_chisq, rtol=rtol)
    np.testing.assert_allclose(res.set_scaling[:, 0], ref.set_scaling, rtol=rtol)
    np.testing.assert_allclose(res.set_background[:, 0], ref.set_background, rtol=rtol, atol=1e-300)
    np.testing.assert_allclose(res.fit[:, 0], ref.fit, rtol=rtol)
    assert res.scaling[0] == res.set_scaling[0, 0] and res.background[0] == res.set_background[0, 0]


def same(a, b, what=""):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)

"""Every instance of the joint fit's kernel (csrc/chain_sets.h: chain_sets_kernel<M, QPL, SHARED>, 8 built-in models x QPL in
{1, 2, 4, 8, 16} x 2 scale modes = 80) run on the device against exact chains, and the edges of its chain text.  The kernel carries
its own step, fits and outputs; with chain_body.inc it shares only how a chain draws (chain_common.h: the stream, a uniform's value,
the initial set, a proposal), so the other families' chain tests say nothing about the rest of it.

Against the float64 restatement (tests/sets_exact.py, tests/sets_shared_exact.py) on the generated inputs sets_exact.GENERATED:
tests/test_sets_host.py and tests/test_sets_shared_host.py hold every one of them to a decisive margin at every step, and
tests/test_plan_decisions_host.py holds its layout to the slot count its name says.  Tolerances are tests/test_sets_gpu.py's
(sets_checks.check): counts equal, contributions rtol 1e-12, chi², scale, background and fit rtol 1e-9.  Kholodenko alone: rtol 1e-7
on the fitted quantities, what test_replay_trajectories_vs_reference grants its Kholodenko replays for the same reason — the device's
row is held to the oracle's QUADPACK integral to 2e-8 (test_kholodenko_active_ranges_vs_quadpack_500_sets), not to float64 rounding.

Against the wavefront kernel with cached rows (chain_wave_kernel<M, QPL, true, false>, with a long test history of its own): one set
at QPL 1, 2 and 16 for every model, which holds those instances without any margin argument."""
import numpy as np
import pytest

from mcsas_amd import engine
from helpers import make_models
import sets_checks
import sets_exact as SX
import sets_shared_exact as SH

pytestmark = pytest.mark.gpu

MODES = {"per_set": SX, "shared": SH}
KHOLODENKO_RTOL = 1e-7


def _against_the_restatement(name, mode):
    mod = MODES[mode]
    c, ref = mod.case(name), mod.reference(name)
    _, _, res = sets_checks.run_case(c, scale=mode)
    sets_checks.check("%s %s" % (name, mode), res, ref, rtol=KHOLODENKO_RTOL if c["tag"] == "kholodenko" else 1e-9)
    if mode == "shared":
        assert (res.set_scaling[:, 0] == res.set_scaling[0, 0]).all()                       # one scaling for all sets
    elif len(c["sets"]) > 1:
        assert res.set_scaling[1, 0] / res.set_scaling[0, 0] > 50.                          # (made a factor 1000 apart)
    return c, res, ref


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("qpl", sorted(SX.MATRIX_SHAPES))
@pytest.mark.parametrize("tag", SX.MATRIX_MODELS)
def test_every_instance_against_the_restatement(tag, qpl, mode):
    """(50,): S = 1; (30, 64): a set of exactly 64 points; (37, 100): one slot all padding; (65, 3, 128, 70): a 3-point set and a set
    that ends on a slot edge; (300, 64, 385, 129): all 16 slots, bit 15 of end_mask.  Every model, both modes: every instance."""
    c, res, ref = _against_the_restatement(SX.matrix_name(tag, qpl), mode)
    assert ref.num_moves >= 5 and res.converged[0] == 0


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(SX.EDGES))
def test_the_edges_of_the_chain_text_against_the_restatement(name, mode):
    """1 contribution (no Monte-Carlo loop), 64 (the initial wave filled exactly), 65 and 128; start_from_minimum with non-zero lower
    bounds; the non-uniform generators; no background with three active parameters."""
    c, res, ref = _against_the_restatement(name, mode)
    P = len(c["lo"])
    if c["st"].n_contrib == 1:
        assert (res.num_iter[0], res.num_moves[0], res.draws[0], res.attempts[0]) == (0, 0, P, 1)
    if c["st"].start_from_min:
        assert res.draws[0] == P * res.num_iter[0]
    if not c["st"].find_bg:
        assert (res.set_background == 0.).all()


# one set: points -> the slot count of the instance
ONE_SET = {1: 50, 2: 65, 16: 1000}
INTEGRAL_MODELS = ("cyl_aspect", "ellcs", "kholodenko", "elliso")        # (a row costs an integral per point: fewer contributions and steps)


@pytest.mark.parametrize("qpl", sorted(ONE_SET))
@pytest.mark.parametrize("tag", SX.MATRIX_MODELS)
def test_one_set_is_the_wave_kernel_for_every_model(tag, qpl):
    """analyse_sets with one set against engine.analyse in EXEC_WAVE with cached rows, free-running on the same Philox stream: counts
    equal, contributions rtol 1e-12, numbers rtol 1e-9 (test_one_set_is_the_existing_wavefront_kernel's comparison); and with one set
    the two scale modes are the same chain bit for bit."""
    from bench import synthetic_data
    q, I, sig = synthetic_data(ONE_SET[qpl])
    lo, hi, fixed = SX.model_range(tag)
    m, _ = make_models(tag, lo, hi, **fixed)
    N, steps = (8, 40) if tag in INTEGRAL_MODELS else (12, 100)
    st = engine.Settings(n_contrib=N, n_reps=2, max_iter=steps, conv_crit=1e-12, max_retries=0, seed=21, rep_offset=qpl, device=0)
    res = engine.analyse_sets(m.setup(), [(q, I, sig)], st, scale="per_set")
    shared = engine.analyse_sets(m.setup(), [(q, I, sig)], st, scale="shared")
    one = engine.analyse(m.setup(), q, I, sig, engine.Settings(**{**st.__dict__, "exec_mode": engine.EXEC_WAVE, "cache_intensities": 1}))
    print(tag, qpl, "iter", res.num_iter, one.num_iter, "moves", res.num_moves, one.num_moves, "chi2", res.chisq, one.chisq)
    assert (res.num_iter == steps).all() and (res.num_moves > 0).all()
    for f in ("num_iter", "num_moves", "draws", "attempts", "converged"):
        assert np.array_equal(getattr(res, f), getattr(one, f)), f
    np.testing.assert_allclose(res.contribs, one.contribs, rtol=1e-12)
    for f in ("chisq", "scaling", "background", "fit"):
        np.testing.assert_allclose(getattr(res, f), getattr(one, f), rtol=1e-9, atol=1e-300, err_msg=f)
    np.testing.assert_allclose(res.set_chisq[0], one.chisq, rtol=1e-9)
    sets_checks.same(res, shared, (tag, qpl))


@pytest.mark.parametrize("mode", sorted(MODES))
def test_more_chains_than_the_chip_holds_at_16_slots(mode):
    """600 free-running chains of the 16-slot instance (one wave per SIMD, 256 CUs: a second round of blocks): repetitions 0, 299 and
    599 of the group are bit for bit the single repetitions at those offsets."""
    c = MODES[mode].case(SX.matrix_name("sphere", 16))
    m, _ = SX.case_models(c)
    kw = dict(n_contrib=20, max_iter=128, conv_crit=1e-12, max_retries=0, seed=77, device=0)
    group = engine.analyse_sets(m.setup(), c["sets"], engine.Settings(n_reps=600, **kw), scale=mode)
    assert not np.array_equal(group.contribs[:, :, 0], group.contribs[:, :, 599])
    for r in (0, 299, 599):
        alone = engine.analyse_sets(m.setup(), c["sets"], engine.Settings(n_reps=1, rep_offset=r, **kw), scale=mode)
        for f in sets_checks.FIELDS:
            a, g = getattr(alone, f), getattr(group, f)
            assert np.array_equal(a[..., 0], g[..., r]), (f, r)
        assert alone.num_moves[0] > 5

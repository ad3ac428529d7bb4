"""Pipeline mode, rows without an integral: the waves of a producer block claim the block's rows one by one from a counter in LDS
(csrc/pipe_prod.h), so which wave evaluates which row differs from launch to launch.  Nothing a chain decides may depend on it:
the same plan launched again gives the same arrays, and every shape below follows the plain-C oracle (oracle/c) on the same
Philox streams chain by chain — move counts, step counts and parameter sets exact, chi-squared within the 1e-7 that
tests/test_parity_gpu.py holds this comparison to.

The shapes come from pipe_geometry (csrc/pipe_layout.h) worked through by hand for a 256-CU device; all of them fit its LDS:
  64 q x 100 contributions, 3 chains     one q per lane, window 48, one producer block of one 48-row sub-window (six rows per wave)
  512 q x 50, 4 chains                   eight q per lane, window 24, one block of one 24-row sub-window
  512 q x 100, 86 chains                 window 48, one block of TWO 24-row sub-windows (a claim is carried across the Gram phase);
                                         up to 85 chains the same window is dealt to two blocks of one sub-window each
  512 q x 100, 4 chains                  those two blocks
Sphere rows cost no integral, so none of these plans runs the row-queue kernels (pipe_rowq.h), which are for rows that do.
Every case runs with the default lazy rows and, where the measurement library is built, with the eager slot tables (bit 16)."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mcsas_amd
from mcsas_amd import engine, _lib
from helpers import make_models

EAGER = 1 << 16
# name: q-points, contributions, chains, step budget, convergence criterion, seed, window
CASES = {
    "q64_repeat":        (64, 100, 3, 600, 0.0, 11, 48),
    "one_subwindow":     (512, 50, 4, 200, 0.0, 3, 24),
    "two_subwindows":    (512, 100, 86, 150, 0.0, 5, 48),
    # a budget that ends inside a window (Kb + 5) and inside a sub-window of a later one (2 Kb + W + 1, W = 24)
    "budget_kb_plus_5_one":     (512, 50, 4, 24 + 5, 0.0, 3, 24),
    "budget_2kb_w_1_one":       (512, 50, 4, 2 * 24 + 24 + 1, 0.0, 3, 24),
    "budget_kb_plus_5_two":     (512, 100, 86, 48 + 5, 0.0, 5, 48),
    "budget_2kb_w_1_two":       (512, 100, 86, 2 * 48 + 24 + 1, 0.0, 5, 48),
    # chi-squared falls through 1400 around step 100 (the oracle's four chains stop at steps 76 to 99): inside a window
    "converges_mid_window":     (512, 100, 4, 600, 1400.0, 7, 48),
}


def problem(name):
    from bench import synthetic_data
    nq, n, reps, steps, crit, seed, kb = CASES[name]
    q, I, sig = synthetic_data(nq)
    lo, hi = np.pi / q.max(), np.pi / q.min()
    return q, I, sig, lo, hi


@functools.lru_cache(maxsize=None)
def oracle_chains(name):
    """The C oracle's chains of a case, computed once and shared by the lazy and the eager run."""
    from oracle import c_oracle
    nq, n, reps, steps, crit, seed, kb = CASES[name]
    q, I, sig, lo, hi = problem(name)
    ref = c_oracle.analyse_sphere(q, I, sig, lo, hi, n, reps, steps, crit, seed=seed, threads=min(16, os.cpu_count() or 1))
    for a in (ref.contribs, ref.chisq, ref.num_iter, ref.num_moves):
        a.setflags(write=False)
    return ref


def pipeline_plan(name, flags):
    nq, n, reps, steps, crit, seed, kb = CASES[name]
    q, I, sig, lo, hi = problem(name)
    m, _ = make_models("sphere", [lo], [hi])
    assert isinstance(m, mcsas_amd.Sphere)                       # rows without an integral: never the row-queue kernels
    st = engine.Settings(n_contrib=n, n_reps=reps, max_iter=steps, conv_crit=crit, max_retries=0, seed=seed,
                         exec_mode=engine.EXEC_PIPELINE, debug_flags=flags)
    plan = engine.Plan(m.setup(), q, I, sig, st)
    info = plan.info
    assert info["exec_mode"] == "pipeline" and info["window"] == kb and info["q_per_lane"] == max(1, nq // 64), info
    return plan


def variants():
    out = [pytest.param(0, id="lazy")]
    if os.path.exists(_lib.TUNING_LIB_PATH):
        out.append(pytest.param(EAGER, id="eager"))
    return out


@pytest.mark.parametrize("flags", variants())
@pytest.mark.parametrize("name", list(CASES))
def test_claimed_rows_follow_the_c_oracle_chain_by_chain(name, flags):
    nq, n, reps, steps, crit, seed, kb = CASES[name]
    ref = oracle_chains(name)
    plan = pipeline_plan(name, flags)
    plan.launch(); res = plan.fetch(); plan.close()
    print(name, flags, "num_iter", res.num_iter[:4], "moves", res.num_moves[:4], "max chi2 rel",
          float(np.max(np.abs(res.chisq / ref.chisq - 1.0))))
    if crit > 0.0:
        assert ((ref.num_iter > 60) & (ref.num_iter < 140)).all() and (ref.num_iter % 24 != 0).any(), ref.num_iter
    else:
        assert (ref.num_iter == steps).all()
    np.testing.assert_array_equal(res.num_iter, ref.num_iter)
    np.testing.assert_array_equal(res.num_moves, ref.num_moves)
    np.testing.assert_allclose(res.contribs, ref.contribs, rtol=1e-12)
    np.testing.assert_allclose(res.chisq, ref.chisq, rtol=1e-7)
    assert ref.num_moves.min() >= 3                              # chains that decide something


@pytest.mark.parametrize("flags", variants())
def test_the_claim_order_leaves_no_trace_in_the_results(flags):
    """One plan, three launches with the same seed: identical arrays, whichever wave took which row."""
    plan = pipeline_plan("q64_repeat", flags)
    runs = []
    for _ in range(3):
        plan.launch()
        runs.append(plan.fetch())
    plan.close()
    for r in runs[1:]:
        for field in ("contribs", "chisq", "num_moves", "num_iter", "fit"):
            np.testing.assert_array_equal(getattr(r, field), getattr(runs[0], field), err_msg=field)
    assert runs[0].num_moves.min() > 50

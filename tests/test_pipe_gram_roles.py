"""Pipeline mode, rows without an integral: in the Gram phase of a producer block (csrc/pipe_gram.h, csrc/pipe_prod.h) waves 0-3 issue
the MFMAs of a sub-window — two q slices each, into the partial slots the eight waves used to fill — while waves 4-7 evaluate the row
of the NEXT sub-window they hold a claim on, keep it in registers and write its LDS copy behind the barrier that ends the operand
reads.  The Gram blocks are summed from the same eight partials in the same order, so nothing may change: every shape follows the
plain-C oracle (oracle/c) chain by chain within the bounds tests/test_pipe_row_claim.py holds that comparison to, one plan launched
three times gives identical arrays, and — where the measurement library is built — the arrays are equal with eight Gram waves
(tuning bit 17), with the eager slot tables (bit 16), and with both.

The shapes are cases of tests/test_pipe_row_claim.py, whose geometry is worked out there (and whose oracle chains are shared):
  two_subwindows          512 q x 100 x 86 chains: one block of two 24-row sub-windows — a row is held across the first Gram phase,
                          the second has nothing beside it
  budget_kb_plus_5_two    the same with 48 + 5 steps: the held rows of the second window lie behind max_iter
  budget_2kb_w_1_two      ... and 2 * 48 + 24 + 1: the budget ends one row into the sub-window of the held rows
  converges_mid_window    512 q x 100 x 4 chains, criterion 1400: two blocks of one sub-window each, nothing to hold, chains end mid-window
  q64_repeat              64 q x 100 x 3 chains: one q per lane, a matrix wave's two slices are 8 q each; a 48-row sub-window is six
                          tiles, three rounds of the reduction (five barriers for every wave, whatever its role)"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mcsas_amd import _lib
from test_pipe_row_claim import CASES, EAGER, oracle_chains, pipeline_plan

GRAM8 = 1 << 17
SHAPES = ["two_subwindows", "budget_kb_plus_5_two", "budget_2kb_w_1_two", "converges_mid_window", "q64_repeat"]
FIELDS = ("contribs", "chisq", "num_moves", "num_iter", "fit")


def test_the_shapes_are_what_the_roles_need():
    assert CASES["two_subwindows"][:4] == (512, 100, 86, 150) and CASES["two_subwindows"][6] == 48
    assert CASES["budget_kb_plus_5_two"][:4] == (512, 100, 86, 48 + 5)
    assert CASES["budget_2kb_w_1_two"][:4] == (512, 100, 86, 2 * 48 + 24 + 1)
    assert CASES["converges_mid_window"][:3] == (512, 100, 4) and CASES["converges_mid_window"][4] == 1400.0
    assert CASES["q64_repeat"][:3] == (64, 100, 3)


@functools.lru_cache(maxsize=None)
def launches(name, flags, n):
    """n launches of one plan of a case, their results read-only."""
    plan = pipeline_plan(name, flags)
    runs = []
    for _ in range(n):
        plan.launch()
        runs.append(plan.fetch())
    plan.close()
    for r in runs:
        for f in FIELDS:
            getattr(r, f).setflags(write=False)
    return runs


@pytest.mark.parametrize("name", SHAPES)
def test_roles_follow_the_c_oracle_chain_by_chain(name):
    nq, n, reps, steps, crit, seed, kb = CASES[name]
    ref = oracle_chains(name)
    res = launches(name, 0, 3)[0]
    print(name, "num_iter", res.num_iter[:4], "moves", res.num_moves[:4], "max chi2 rel", float(np.max(np.abs(res.chisq / ref.chisq - 1.0))))
    if crit > 0.0:
        assert (ref.num_iter < steps).all() and (ref.num_iter % 24 != 0).any(), ref.num_iter
    else:
        assert (ref.num_iter == steps).all()
    np.testing.assert_array_equal(res.num_iter, ref.num_iter)
    np.testing.assert_array_equal(res.num_moves, ref.num_moves)
    np.testing.assert_allclose(res.contribs, ref.contribs, rtol=1e-12)
    np.testing.assert_allclose(res.chisq, ref.chisq, rtol=1e-7)


@pytest.mark.parametrize("name", SHAPES)
def test_three_launches_of_one_plan_give_identical_arrays(name):
    runs = launches(name, 0, 3)
    for r in runs[1:]:
        for f in FIELDS:
            np.testing.assert_array_equal(getattr(r, f), getattr(runs[0], f), err_msg=f)
    assert runs[0].num_moves.min() >= 3                          # chains that decide something


def tuning_words():
    """The words of the measurement library whose arrays are compared with the release library's, one test case each; where that
    library is not built, one case that says so by its id and compares the release library's second launch instead."""
    if os.path.exists(_lib.TUNING_LIB_PATH):
        return [pytest.param(GRAM8, id="eight_gram_waves"), pytest.param(EAGER, id="eager"), pytest.param(EAGER | GRAM8, id="eager_eight_gram_waves")]
    return [pytest.param(0, id="no_tuning_library")]


@pytest.mark.parametrize("word", tuning_words())
@pytest.mark.parametrize("name", SHAPES)
def test_eight_gram_waves_and_eager_rows_give_the_same_arrays(name, word):
    base = launches(name, 0, 3)[0]
    r = launches(name, word, 1)[0] if word else launches(name, 0, 3)[1]
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(r, f), getattr(base, f), err_msg="%s, tuning word %#x" % (f, word))

"""Pipeline mode, rows without an integral: the roles of a producer block's Gram phase (csrc/pipe_gram.h, csrc/pipe_prod.h) are chosen
per SUB-WINDOW.  A sub-window whose successor in the block can lend a held row is split — waves 0-3 issue the MFMAs, two q slices each,
waves 4-7 evaluate the row beside them —; the last sub-window of a block, and the only one of a block that has one, has nothing to
hold and runs eight Gram waves with one slice each.  A sub-window with all its W rows in front of max_iter reads its operands without
the row masks; the masked code remains for the last window of a run.  Either way the eight partial slots of the reduction buffer hold
the same partials and are summed in the same order, so nothing may change: every shape follows the plain-C oracle (oracle/c) chain by
chain within the bounds tests/test_pipe_row_claim.py holds that comparison to, one plan launched three times gives identical arrays,
and — where the measurement library is built — the arrays are EQUAL between word 0, eight Gram waves everywhere (tuning bit 17), roles
in every sub-window as before this change (bit 21), and each of those with the eager slot tables (bit 16).

The shapes are cases of tests/test_pipe_row_claim.py, whose geometry is worked out there (and whose oracle chains are shared):
  two_subwindows          512 q x 100 x 86 chains, 150 steps: one block of two 24-row sub-windows — the first Gram phase is split and
                          rows are held, the second runs eight waves; a held row's LDS copy is written behind a split phase only
  budget_kb_plus_5_two    the same with 48 + 5 steps: in the second window 5 rows are valid in the split sub-window and none behind it
  budget_2kb_w_1_two      ... and 2 * 48 + 24 + 1: full split sub-windows in front, then one valid row in an eight-wave sub-window —
                          with the case above the masked code in both roles, the unmasked code in the sub-windows in front of them
  converges_mid_window    512 q x 100 x 4 chains, criterion 1400: blocks of one sub-window, eight waves everywhere, chains end inside one
  q64_repeat              64 q x 100 x 3 chains: a 48-row sub-window of six tiles in three reduction rounds — the general tile path in
                          the eight-wave form, without masks (five barriers for every wave)"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mcsas_amd import _lib
from test_pipe_row_claim import CASES, EAGER, oracle_chains, pipeline_plan

GRAM8 = 1 << 17          # eight Gram waves in every sub-window, no held row
ROLES_ALL = 1 << 21      # roles in every sub-window, the last of a block included
SHAPES = ["two_subwindows", "budget_kb_plus_5_two", "budget_2kb_w_1_two", "converges_mid_window", "q64_repeat"]
FIELDS = ("contribs", "chisq", "num_moves", "num_iter", "fit")


def test_the_shapes_are_what_the_gram_tail_needs():
    # (q-points, contributions, chains, steps) and the window: 48 = two 24-row sub-windows per block at 86 chains, two blocks of one
    # at 4 chains; 64 q x 100: one block of one 48-row sub-window
    assert CASES["two_subwindows"][:4] == (512, 100, 86, 150) and CASES["two_subwindows"][6] == 48
    assert CASES["budget_kb_plus_5_two"][:4] == (512, 100, 86, 48 + 5) and CASES["budget_kb_plus_5_two"][6] == 48
    assert CASES["budget_2kb_w_1_two"][:4] == (512, 100, 86, 2 * 48 + 24 + 1) and CASES["budget_2kb_w_1_two"][6] == 48
    assert CASES["converges_mid_window"][:3] == (512, 100, 4) and CASES["converges_mid_window"][4] == 1400.0
    assert CASES["q64_repeat"][:3] == (64, 100, 3) and CASES["q64_repeat"][6] == 48


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
def test_per_subwindow_roles_follow_the_c_oracle_chain_by_chain(name):
    nq, n, reps, steps, crit, seed, kb = CASES[name]
    ref = oracle_chains(name)
    res = launches(name, 0, 3)[0]
    print(name, "num_iter", res.num_iter[:4], "moves", res.num_moves[:4], "max chi2 rel", float(np.max(np.abs(res.chisq / ref.chisq - 1.0))),
          "max contribs rel", float(np.max(np.abs(res.contribs / ref.contribs - 1.0))))
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
        return [pytest.param(ROLES_ALL, id="roles_everywhere"), pytest.param(GRAM8, id="eight_gram_waves"),
                pytest.param(EAGER, id="eager"), pytest.param(EAGER | ROLES_ALL, id="eager_roles_everywhere"),
                pytest.param(EAGER | GRAM8, id="eager_eight_gram_waves")]
    return [pytest.param(0, id="no_tuning_library")]


@pytest.mark.parametrize("word", tuning_words())
@pytest.mark.parametrize("name", SHAPES)
def test_every_choice_of_roles_gives_the_same_arrays(name, word):
    """The base is word 0, which runs on the release library (engine.Plan loads the measurement library for a non-zero word only);
    the other five words run this change, the two older forms, and each of the three with the eager slot tables."""
    base = launches(name, 0, 3)[0]
    r = launches(name, word, 1)[0] if word else launches(name, 0, 3)[1]
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(r, f), getattr(base, f), err_msg="%s, tuning word %#x" % (f, word))

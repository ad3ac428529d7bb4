"""Plan creation and the life of a plan's result slots (csrc/host_decide.hip: decide_shape; csrc/mcsas_hip.hip: make_slot, plan_activate_slot,
mcsas_hip_plan_destroy): what the library decides for a fixed list of problems, and that plans closed with analyses in flight,
slots used out of order and a drained memory cache leave every later analysis bit for bit what it is alone."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mcsas_amd import engine
from mcsas_amd import _lib
from helpers import PLAN_SHAPE_CASES, PLAN_SHAPES_GOLDEN, load, make_models, plan_shape_problem

A, W, G, P = engine.EXEC_AUTO, engine.EXEC_WAVE, engine.EXEC_WORKGROUP, engine.EXEC_PIPELINE


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def plan_shape(case):
    """Plan.info of the case, or the library's refusal (code and message); nothing is launched."""
    m, q, I, sig, st, smear = plan_shape_problem(case)
    try:
        pl = engine.Plan(m.setup(), q, I, sig, st, smear=smear)
    except _lib.McSASHipError as e:
        return {"error_code": int(e.code), "error": str(e)}
    try:
        return dict(pl.info)
    finally:
        pl.close()


def _sphere_problem(mode):
    g = load("g4_sphere_q100_fixed.npz")
    m, _ = make_models("sphere", g["spec_lo"], g["spec_hi"])
    st = engine.Settings(n_contrib=120, n_reps=3, max_iter=300, conv_crit=1e-9, max_retries=0, seed=5, exec_mode=mode)
    return m.setup(), g["data_q"], g["data_I"], g["data_sigma"], st


def _assert_same(got, ref, what):
    for name in ("contribs", "fit", "chisq", "num_iter", "num_moves"):
        np.testing.assert_array_equal(getattr(got, name), getattr(ref, name), err_msg="%s: %s" % (what, name))


def test_plan_shapes_are_the_recorded_ones():
    """What plan creation decides — execution mode, waves per chain, q slots per lane, window, row cache — or refuses, for every
    branch of the decision, equals the recording taken before plan creation was split into functions
    (tests/golden/plan_shapes_mi355x.json).  Rows with an explicit mode hold on any device, MCSAS_EXEC_AUTO rows on a device with
    the recorded CU count.  After the refusals — each unwinds a half-made plan — an ordinary analysis is still what it was."""
    rec = json.load(open(PLAN_SHAPES_GOLDEN))
    same_device = cu_count() == rec["cu_count"]
    before = engine.analyse(*_sphere_problem(A))
    assert set(rec["rows"]) == set(c[0] for c in PLAN_SHAPE_CASES)
    for case in PLAN_SHAPE_CASES:
        if case[5] == A and not same_device:
            continue
        assert plan_shape(case) == rec["rows"][case[0]], case[0]
    _assert_same(engine.analyse(*_sphere_problem(A)), before, "after the refusals")


@pytest.mark.parametrize("mode", [W, G, P])
def test_slot_and_plan_lifecycle(mode):
    """Result slots are made on first use and freed with the plan, whichever were used and whether or not they were fetched."""
    prob = _sphere_problem(mode)
    alone = engine.analyse(*prob)
    # (a) both slots launched, neither fetched, the plan closed: the next analysis is untouched
    pl = engine.Plan(*prob)
    pl.launch(slot=0); pl.launch(slot=1)
    pl.close()
    _assert_same(engine.analyse(*prob), alone, "after a plan closed in flight")
    # (b) a fresh plan that only ever uses slot 1
    pl = engine.Plan(*prob)
    pl.launch(slot=1)
    _assert_same(pl.fetch(slot=1), alone, "slot 1 alone")
    # (c) ... and then goes through a batch launch, which writes slot 0
    if mode == W:
        engine.launch_batch([pl])
        _assert_same(pl.fetch(slot=0), alone, "batch launch after slot 1")
    pl.close()
    # (d) the memory the plans gave back is released; one more analysis
    engine.release_cached_memory()
    _assert_same(engine.analyse(*prob), alone, "after release_cached_memory")

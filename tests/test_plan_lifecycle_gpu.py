"""Plan creation and the life of a plan's result slots (csrc/mcsas_hip.hip: decide_shape, make_slot, plan_activate_slot,
mcsas_hip_plan_destroy): what the library decides for a fixed list of problems, and that plans closed with analyses in flight,
slots used out of order and a drained memory cache leave every later analysis bit for bit what it is alone."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from mcsas_amd import engine
from mcsas_amd import _lib
from helpers import load, make_models, product_smearing, plugin_twin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_shapes_mi355x.json")
RANGES = {"sphere": ([2e-9], [3e-7]), "cyl_aspect": ([1e-9, 0.5], [1e-7, 20.0]), "gausschain": ([1e-9, 1e-9], [1e-7, 1e-7])}
A, W, G, P = engine.EXEC_AUTO, engine.EXEC_WAVE, engine.EXEC_WORKGROUP, engine.EXEC_PIPELINE

# (id, model tag, nq, contributions, repetitions, exec mode, waves_per_chain, cache_intensities, variant) — every branch of the
# shape and mode decision, then its refusals.  All working sets stay under 1 GB: the free-memory gate decides no row.
PLAN_SHAPE_CASES = (
    [("auto_r%d" % r, "sphere", 100, 200, r, A, 0, -1, None) for r in (1, 64, 300, 3000)]
    + [("wave_cache%+d" % c, "sphere", 100, 200, 6, W, 0, c, None) for c in (-1, 0, 1)]
    + [("wg_waves%d" % w, "sphere", 100, 200, 6, G, w, -1, None) for w in (0, 2, 4)]
    + [("pipeline", "sphere", 100, 200, 6, P, 0, -1, None)]
    + [("auto_q%d" % nq, "sphere", nq, 200, 6, A, 0, -1, None) for nq in (1000, 1500, 5000)]
    + [("wave_q1500", "sphere", 1500, 200, 6, W, 0, -1, None),
       ("cyl_48x4", "cyl_aspect", 64, 48, 4, A, 0, -1, None),
       ("cyl_8x4", "cyl_aspect", 64, 8, 4, A, 0, -1, None),
       ("cyl_8x2000", "cyl_aspect", 64, 8, 2000, A, 0, -1, None),
       ("smeared_auto", "sphere", 100, 200, 6, A, 0, -1, "smear"),
       ("plugin_auto", "gausschain", 100, 200, 6, A, 0, -1, "plugin"),
       ("plugin_wave", "gausschain", 100, 200, 6, W, 0, -1, "plugin"),
       # refusals
       ("no_pipeline_n8", "sphere", 100, 8, 6, P, 0, -1, None),
       ("no_pipeline_q1500", "sphere", 1500, 200, 6, P, 0, -1, None),
       ("no_wave_q5000", "sphere", 5000, 200, 6, W, 0, -1, None),
       ("no_q20000", "sphere", 20000, 200, 6, A, 0, -1, None),
       ("no_wg_n2", "sphere", 100, 2, 6, G, 0, -1, None),
       ("no_plugin_wave_q1500", "gausschain", 1500, 200, 6, W, 0, -1, "plugin")])


def _synthetic(nq):
    from bench import synthetic_data
    return synthetic_data(nq)


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def plan_shape(case):
    """Plan.info of the case, or the library's refusal (code and message); nothing is launched."""
    _, tag, nq, n, reps, mode, waves, cache, variant = case
    q, I, sig = _synthetic(nq)
    lo, hi = RANGES[tag]
    m, _ = make_models(tag, lo, hi, **({"intDiv": 20.} if tag == "cyl_aspect" else {}))
    smear = None
    if variant == "plugin":
        plugin_twin(m, tag)
    if variant == "smear":
        d, _ = product_smearing("trapezoid", False, 15, q, I, sig, umbra=2e-3 * q.max(), penumbra=4e-3 * q.max())
        smear = d.smearArgs(m)
    st = engine.Settings(n_contrib=n, n_reps=reps, max_iter=100, max_retries=0, seed=1, exec_mode=mode, waves_per_chain=waves,
                         cache_intensities=cache)
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
    rec = json.load(open(GOLDEN))
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

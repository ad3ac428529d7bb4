"""Every entry point writes a mcsas_result through the one writer (csrc/host_result.h): a fetch (mcsas_hip_analyse), the blocks of a
device list at their repetition offsets, and the two entry points whose rows the caller evaluates.  One small workload through all
four; then once more with most arrays of the result NULL.  Tolerances: those of tests/test_device_rows_gpu.py (same_chains)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch                        # ahead of the library's first load: one HIP runtime in the process (engine._one_hip_runtime)
import mcsas_amd
from mcsas_amd import engine
from helpers import load, make_models
from test_parity_gpu import PythonOnlySphere
from test_device_rows_gpu import numpy_rows, same_chains, sphere_pair, torch_rows

ARRAYS = ("contribs", "fit", "chisq", "scaling", "background", "num_iter", "num_moves", "attempts", "converged", "seconds", "draws")
KEPT = ("chisq", "num_moves")


def _paths():
    """A Sphere at 65 q-points (rows of 128: 63 padding columns), 5 contributions, 5 repetitions (two blocks: 3 + 2), a fixed budget
    of 40 steps per attempt (convergenceCriterion 0: no attempt converges, every repetition makes both) — as callables that run it."""
    g = load("g4_sphere_q100_fixed.npz")
    q, I, sig = g["data_q"][:65], g["data_I"][:65], g["data_sigma"][:65]
    data = mcsas_amd.SASData(q, I, sig)
    st = engine.Settings(n_contrib=5, n_reps=5, max_iter=40, conv_crit=0.0, max_retries=1, seed=20, exec_mode=engine.EXEC_WAVE)
    builtin, _ = make_models("sphere", g["spec_lo"], g["spec_hi"], sld=float(g["spec_sld"]))
    mt, _ = sphere_pair(g)
    mn, _ = sphere_pair(g, PythonOnlySphere)
    return {
        "analyse": lambda: engine.analyse(builtin.setup(), q, I, sig, st),
        "device list": lambda: engine.analyse(builtin.setup(), q, I, sig, engine.Settings(**{**st.__dict__, "devices": (0, 0)})),
        "device rows": lambda: engine.analyse_device_rows(mt.setup(data), q, I, sig, st, torch_rows(mt, q, st.comp_exp), window=16),
        "host rows": lambda: engine.analyse_host_rows(mn.setup(data), q, I, sig, st, numpy_rows(mn, data, st.comp_exp), window=16),
    }


def test_four_entry_points_write_one_result(monkeypatch):
    paths = _paths()
    full = {name: run() for name, run in paths.items()}
    a = full["analyse"]
    assert engine.shard(5, 2, 0) == (0, 3) and engine.shard(5, 2, 1) == (3, 2)
    assert (a.attempts == 2).all() and (a.num_iter == 40).all() and (a.converged == 0).all() and a.num_moves.sum() > 0
    for name in ARRAYS:                                       # the device-list contract: bit for bit, but for the clock
        if name != "seconds":
            np.testing.assert_array_equal(getattr(full["device list"], name), getattr(a, name), err_msg=name)
    for name in ("device rows", "host rows"):
        same_chains(full[name], a)
    assert all((r.seconds >= 0).all() for r in full.values())

    # the same runs into a result that has chisq and num_moves only: MCSAS_OK (the engine raises on anything else), the same two
    # arrays, and nothing else written
    made = []

    def sparse(*shape):
        res = engine_results(*shape)
        for name in ARRAYS:
            if name not in KEPT:
                setattr(res.c, name, None)
        made.append(res)
        return res
    engine_results = engine.ChainResults
    monkeypatch.setattr(engine, "ChainResults", sparse)
    for name, run in paths.items():
        res = run()
        for kept in KEPT:
            np.testing.assert_array_equal(getattr(res, kept), getattr(full[name], kept), err_msg="%s: %s" % (name, kept))
        for other in ARRAYS:
            if other not in KEPT:
                assert not getattr(res, other).any(), (name, other)
    assert len(made) == 4

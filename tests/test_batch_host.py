"""The batch entry points without a GPU: header, binding and library agree (ABI 5), and engine.analyse_batch refuses what one
wavefront per chain cannot run before anything reaches the device."""
import os
import re

import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import engine, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_batch_entry_points_at_abi_5():
    h = open(os.path.join(ROOT, "include", "mcsas_hip.h")).read()
    assert re.search(r"#define MCSAS_ABI_VERSION 5\b", h)
    assert "int mcsas_hip_plan_launch_batch(mcsas_plan *const *plans, int32_t n, void *hip_stream);" in h
    assert "int mcsas_hip_analyse_batch(const mcsas_problem *problems, int32_t n, mcsas_result *results);" in h
    assert _lib.ABI_VERSION == 5
    assert {"mcsas_hip_plan_launch_batch", "mcsas_hip_analyse_batch"} <= set(_lib.SYMBOLS)


def test_library_exports_the_batch_entry_points():
    lib = _lib.load()                                     # (checks every symbol of _lib.SYMBOLS and the ABI number)
    assert lib.mcsas_hip_abi_version() == 5
    assert hasattr(lib, "mcsas_hip_plan_launch_batch") and hasattr(lib, "mcsas_hip_analyse_batch")


def test_analyse_batch_refuses_an_oversize_data_set_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("nothing may be launched")
    monkeypatch.setattr(engine, "analyse", no_launch)
    monkeypatch.setattr(engine, "HipProblem", no_launch)
    m = mcsas_amd.Sphere(); m.radius.setActiveRange((1e-9, 1e-7))
    small, big = np.linspace(0.1, 2.0, 100), np.linspace(0.1, 2.0, engine.WAVE_MAX_Q + 1)
    st = engine.Settings(n_contrib=10, n_reps=2, max_iter=10)
    with pytest.raises(ValueError, match="q-points"):
        engine.analyse_batch([(m.setup(), small, small, small, st), (m.setup(), big, big, big, st)])
    assert engine.analyse_batch([]) == []

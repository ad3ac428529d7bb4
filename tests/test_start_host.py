"""Chains started from given contributions (mcsas_hip_plan_set_start / mcsas_hip_analyse_from, engine.analyse(start=),
McSAS.calc(start=), run_series(start=)): what can be checked without a GPU — the additive C ABI and every refusal that is made
before a device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import _lib, engine
from helpers import PythonOnlySphere, make_models
from chain_cases import MCSAS_EINVAL, _NoLibrary, _algo_40q, _data, _from, _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcsas_hip.h")
# sizeof(mcsas_problem), sizeof(mcsas_result) of ABI 5 before the start entry points existed (x86-64)
PROBLEM_BYTES, RESULT_BYTES = 512, 96


def test_the_abi_is_extended_not_changed(tmp_path):
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(mcsas_hip_[a-z_0-9]+)\s*\(", text))
    assert {"mcsas_hip_plan_set_start", "mcsas_hip_analyse_from"} <= declared
    assert {"mcsas_hip_plan_set_start", "mcsas_hip_analyse_from"} <= set(_lib.SYMBOLS)
    assert re.search(r"#define\s+MCSAS_ABI_VERSION\s+5\b", text) and _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert hasattr(lib, "mcsas_hip_plan_set_start") and hasattr(lib, "mcsas_hip_analyse_from")
    assert lib.mcsas_hip_abi_version() == 5
    assert C.sizeof(_lib.Problem) == PROBLEM_BYTES and C.sizeof(_lib.Result) == RESULT_BYTES
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%d\\n", sizeof(mcsas_problem), sizeof(mcsas_result),'
                   ' MCSAS_ABI_VERSION); return 0;}\n' % HEADER)
    subprocess.check_call(["gcc", "-o", str(tmp_path / "sz"), str(src)])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()] == [PROBLEM_BYTES, RESULT_BYTES, 5]


def test_analyse_from_refuses_before_a_device_is_touched():
    start = np.full((8, 1, 2), 5e-8)
    prob, res = _problem()
    rc, msg = _from(prob, None, res)
    assert rc == MCSAS_EINVAL and "start" in msg and "NULL" in msg
    for mode, name in ((engine.EXEC_PIPELINE, "MCSAS_EXEC_PIPELINE"), (engine.EXEC_WORKGROUP, "MCSAS_EXEC_WORKGROUP")):
        prob, res = _problem(exec_mode=mode)
        rc, msg = _from(prob, start, res)
        assert rc == MCSAS_EINVAL and name in msg and "MCSAS_EXEC_WAVE" in msg, msg
    prob, res = _problem(nq=5000)
    rc, msg = _from(prob, start, res)
    assert rc == MCSAS_EINVAL and "5000" in msg and "4096" in msg, msg
    bad = start.copy()
    bad[5, 0, 1] = np.nan
    prob, res = _problem()
    rc, msg = _from(prob, bad, res)
    assert rc == MCSAS_EINVAL and "not finite" in msg and "[5][0][1]" in msg and "index 11" in msg, msg
    bad[5, 0, 1] = np.inf
    rc, msg = _from(prob, bad, res)
    assert rc == MCSAS_EINVAL and "index 11" in msg, msg


def test_set_start_on_a_null_plan():
    lib = _lib.load()
    start = np.zeros((2, 1, 1))
    assert lib.mcsas_hip_plan_set_start(None, _lib.as_dp(start), 1, 0) == MCSAS_EINVAL
    assert "null plan" in lib.mcsas_hip_last_error().decode()
    assert lib.mcsas_hip_plan_set_start(None, None, 0, 0) == MCSAS_EINVAL


def test_engine_shape_errors_come_before_any_library_call(monkeypatch):
    _NoLibrary(monkeypatch)
    q, I, sig = _data()
    m, _ = make_models("sphere", [2e-9], [3e-7])
    st = engine.Settings(n_contrib=8, n_reps=3, max_iter=10)
    for shape in ((7, 1, 3), (8, 2, 3), (8, 1), (8, 1, 2)):          # wrong N, wrong P, no repetition axis, too few repetitions
        with pytest.raises(ValueError):
            engine.analyse(m.setup(), q, I, sig, st, start=np.full(shape, 5e-8))
        with pytest.raises(ValueError):
            engine.analyse_batch([dict(model=m.setup(), q=q, intensity=I, sigma=sig, st=st, start=np.full(shape, 5e-8))])
    host = m.setup()
    host.model_id = engine.MODEL_HOST
    with pytest.raises(ValueError, match="host code"):
        engine.analyse(host, q, I, sig, st, start=np.full((8, 1, 3), 5e-8))


def test_front_end_refusals(monkeypatch):
    _NoLibrary(monkeypatch)
    good = np.full((8, 1, 3), 5e-8)
    for mode in (engine.EXEC_PIPELINE, engine.EXEC_WORKGROUP):
        with pytest.raises(ValueError, match="execMode"):
            _algo_40q(execMode=mode).calc(start=good)
    with pytest.raises(ValueError):
        _algo_40q().calc(start=np.full((8, 1, 2), 5e-8))                  # fewer start repetitions than numReps
    with pytest.raises(ValueError):
        _algo_40q().calc(start=np.full((9, 1, 3), 5e-8))
    algo = _algo_40q()
    with pytest.raises(ValueError, match="previous"):
        mcsas_amd.run_series(algo, [algo.data], start="previous", batch=True)
    with pytest.raises(ValueError, match="previous"):
        mcsas_amd.run_series(algo, [algo.data], start="previous", overlap=True)
    with pytest.raises(ValueError):
        mcsas_amd.run_series(algo, [algo.data, algo.data], start=[good])   # one entry per data set


def test_python_only_model_takes_no_start(monkeypatch):
    _NoLibrary(monkeypatch)
    algo = _algo_40q()
    hm = PythonOnlySphere()
    hm.radius.setActiveRange((2e-9, 3e-7))
    algo.model = hm
    with pytest.raises(ValueError, match="host code"):
        algo.calc(start=np.full((8, 1, 3), 5e-8))

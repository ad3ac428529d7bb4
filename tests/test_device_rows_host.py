"""CPU-side checks (no GPU) of the entry point whose rows the caller produces on the device (include/mcsas_hip.h:
mcsas_hip_analyse_device_rows): the two symbols, the shape rule, every refusal made before a device is touched, and the front end's
routing of a model that defines calcIntensityBatch."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import _lib, engine
from mcsas_amd.scatteringmodels import is_host_model, is_batch_model, setup_from_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcsas_hip.h")
NEW = ("mcsas_hip_device_rows_shape", "mcsas_hip_analyse_device_rows")


class BatchOnlySphere(mcsas_amd.SASModel):
    """A sphere that brings nothing but calcIntensityBatch: no numpy formfactor / volume, no kernel id, no HIP text."""
    shortName = "Sphere (torch batch only)"
    canSmear = True
    parameters = mcsas_amd.Sphere.parameters

    def __init__(self):
        super().__init__()
        self.radius.setActive(True)

    def calcIntensityBatch(self, q, pset, compensationExponent):
        raise AssertionError("not evaluated in these tests")


def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    declared = set(re.findall(r"\b(mcsas_hip_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "mcsas_device_rows_callback" in open(HEADER).read()
    assert lib.mcsas_hip_abi_version() == _lib.ABI_VERSION == 5          # additive: the ABI version stays


def _shape(nq, n_contrib, n_reps, window):
    m = mcsas_amd.Sphere()
    st = engine.Settings(n_contrib=n_contrib, n_reps=n_reps)
    return engine.device_rows_shape(m.setup(), np.linspace(1e8, 1e9, nq), st, window)


def test_shape_rule():
    assert _shape(100, 200, 10, 64) == (200, 2000, 128)
    assert _shape(64, 200, 10, 64)[2] == 64
    assert _shape(1300, 40, 3, 33) == (40, 120, 1344)
    assert _shape(100, 20, 3, 50) == (50, 150, 128)                       # min_rows = max(N, window)
    assert _shape(100, 20, 3, 0) == _shape(100, 20, 3, 64) == (64, 192, 128)    # window < 1: 64
    assert _shape(100, 20, 3, -5) == (64, 192, 128)
    # the 256 MiB rule: rows of 128 doubles -> 262144 rows at the most ...
    assert _shape(100, 300, 5000, 64) == (300, (256 << 20) // (128 * 8), 128)
    # ... and never fewer than one chain's round (16384 q: 2048 rows fit 256 MiB)
    assert _shape(16384, 5000, 7, 64) == (5000, 5000, 16384)
    lib = _lib.load()
    assert lib.mcsas_hip_device_rows_shape(None, 64, None, None, None) == -1
    prob = engine.HipProblem(mcsas_amd.Sphere().setup(), [1e8, 2e8], [1., 1.], [1., 1.], engine.Settings())
    assert lib.mcsas_hip_device_rows_shape(C.byref(prob.c), 64, None, None, None) == 0       # (any of the three may be NULL)
    prob.c.struct_size += 8
    assert lib.mcsas_hip_device_rows_shape(C.byref(prob.c), 64, None, None, None) == -1


# Runs in a process of its own with every device hidden: a call that passes all the checks made before a device is touched then ends
# with MCSAS_ENODEV (the control), so MCSAS_EINVAL shows that the refusal came first.  Nothing is ever read through the two
# buffer addresses.
_REFUSALS = r"""
import ctypes as C, json, sys
import numpy as np
import mcsas_amd
from mcsas_amd import _lib, engine

lib = _lib.load()
q = np.linspace(1e8, 1e9, 100)
out = {}

def call(tag, null=(), capacity=200, window=64, **change):
    prob = engine.HipProblem(mcsas_amd.Sphere().setup(), q, np.ones(100), np.ones(100), engine.Settings(n_contrib=200, n_reps=3, max_iter=50))
    prob.c.model_id = engine.MODEL_HOST
    for k, v in change.items():
        if k == "gen_kind0":
            prob.c.gen_kind[0] = v
        elif k == "no_q":
            prob.c.q = None
        else:
            setattr(prob.c, k, v)
    res = engine.ChainResults(200, 1, 3, 100)
    cb = _lib.DeviceRowsCallback() if "rows_cb" in null else _lib.DeviceRowsCallback(lambda user, n: 0)
    rc = lib.mcsas_hip_analyse_device_rows(None if "problem" in null else C.byref(prob.c),
                                           None if "d_pset" in null else C.c_void_p(0x10000),
                                           None if "d_rows" in null else C.c_void_p(0x20000), capacity, cb, None, window,
                                           None if "result" in null else C.byref(res.c))
    out[tag] = [rc, lib.mcsas_hip_last_error().decode()]

call("control")
call("control_min_capacity", capacity=200)
for name in ("problem", "rows_cb", "result", "d_pset", "d_rows"):
    call("null_" + name, null=(name,))
call("struct_size", struct_size=C.sizeof(_lib.Problem) - 8)
call("capacity", capacity=199)
call("capacity_window", capacity=299, window=300)
call("nq_0", nq=0)
call("nq_big", nq=16385)
call("no_q", no_q=True)
call("n_active_0", n_active=0)
call("n_active_5", n_active=5)
call("n_contrib_0", n_contrib=0)
call("n_reps_0", n_reps=0)
call("max_iter_neg", max_iter=-1)
call("max_retries_neg", max_retries=-1)
call("reserved0", reserved0=1)
call("gen_kind", gen_kind0=4)
out["torch_loaded"] = "torch" in sys.modules
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def refusals():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _REFUSALS], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_control_call_finds_no_device(refusals):
    assert refusals["control"][0] == -2, refusals["control"]             # MCSAS_ENODEV: every check before the device passed
    assert refusals["control_min_capacity"][0] == -2


@pytest.mark.parametrize("tag, words", [
    ("null_problem", "null"), ("null_rows_cb", "null"), ("null_result", "null"), ("null_d_pset", "d_pset"), ("null_d_rows", "d_rows"),
    ("struct_size", "ABI mismatch"), ("capacity", "199"), ("capacity_window", "299"),
    ("nq_0", "nq 0"), ("nq_big", "nq 16385"), ("no_q", "data pointers"), ("n_active_0", "n_active 0"), ("n_active_5", "n_active 5"),
    ("n_contrib_0", "n_contrib"), ("n_reps_0", "n_reps"), ("max_iter_neg", "max_iter"), ("max_retries_neg", "max_retries"),
    ("reserved0", "reserved0"), ("gen_kind", "gen_kind[0] = 4")])
def test_refused_before_a_device_is_touched(refusals, tag, words):
    rc, msg = refusals[tag]
    assert rc == -1, (tag, rc, msg)                                      # MCSAS_EINVAL, not MCSAS_ENODEV
    assert words in msg, (tag, msg)


def test_capacity_refusal_names_both_numbers(refusals):
    assert "199" in refusals["capacity"][1] and "200" in refusals["capacity"][1]
    assert "299" in refusals["capacity_window"][1] and "300" in refusals["capacity_window"][1]


def test_importing_the_package_does_not_import_torch(refusals):
    assert refusals["torch_loaded"] is False
    r = subprocess.run([sys.executable, "-c", _IMPORT_ORDER], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["torch_after_import"] is False
    # the library loaded BEFORE torch: where torch brings a HIP runtime of its own the process then holds two, a tensor would not be
    # device memory to the library's, and analyse_device_rows says so instead of running
    assert out["refused"] == (out["runtimes"] > 1), out


_IMPORT_ORDER = r"""
import json, sys
import mcsas_amd, mcsas_amd.engine, mcsas_amd.mcsas
out = {"torch_after_import": "torch" in sys.modules}
from mcsas_amd import _lib, engine
_lib.load()
import torch
out["runtimes"] = len({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line})
try:
    engine._one_hip_runtime()
    out["refused"] = False
except RuntimeError as e:
    out["refused"] = "two HIP runtimes" in str(e)
print(json.dumps(out))
"""


def test_a_class_with_only_the_batch_method_is_a_host_model():
    m = BatchOnlySphere()
    assert is_batch_model(m) and is_host_model(m)
    assert setup_from_model(m).model_id == engine.MODEL_HOST
    assert not is_batch_model(mcsas_amd.Sphere()) and not is_host_model(mcsas_amd.Sphere())

    class Neither(mcsas_amd.SASModel):
        parameters = mcsas_amd.Sphere.parameters
    assert not is_host_model(Neither())


class _Reached(Exception):
    pass


def _algo():
    q = np.logspace(8, 9.3, 40)
    algo = mcsas_amd.McSAS(seed=1)
    algo.numContribs.setValue(8); algo.numReps.setValue(3); algo.maxIterations.setValue(10)
    algo.model = BatchOnlySphere()
    algo.data = mcsas_amd.SASData(q, 1.0 / q, 0.01 / q)
    return algo


def test_front_end_routes_a_batch_model_to_device_rows(monkeypatch):
    def load(*a, **k):
        raise _Reached()
    monkeypatch.setattr(_lib, "load", load)
    called = []
    real = engine.analyse_device_rows

    def device_rows(*a, **k):
        called.append(k.get("window"))
        return real(*a, **k)

    def host_rows(*a, **k):
        raise AssertionError("a batch model must not run through analyse_host_rows")
    monkeypatch.setattr(engine, "analyse_device_rows", device_rows)
    monkeypatch.setattr(engine, "analyse_host_rows", host_rows)
    algo = _algo()
    algo.hostRowWindow = 37
    with pytest.raises(_Reached):                     # every check made in Python has passed, through analyse_device_rows
        algo.calc()
    assert called == [37]
    # a start and a trace are refused as for every model that exists only as host code
    with pytest.raises(ValueError, match="host code"):
        _algo().calc(start=np.full((8, 1, 3), 5e-8))
    with pytest.raises(ValueError, match="host code"):
        _algo().calc(trace=4)
    assert called == [37]


def test_batch_model_refuses_data_whose_smearing_would_apply(monkeypatch):
    def load(*a, **k):
        raise _Reached()
    monkeypatch.setattr(_lib, "load", load)
    from helpers import product_smearing
    algo = _algo()
    q = algo.data.q
    algo.data, _ = product_smearing("trapezoid", False, 9, q, 1.0 / q, 0.01 / q, umbra=2e-3 * q.max(), penumbra=4e-3 * q.max())
    assert algo.data.smearArgs(algo.model) is not None                   # (the model says canSmear, the data smears)
    with pytest.raises(NotImplementedError, match="smear"):
        algo.calc()
    with pytest.raises(NotImplementedError, match="smear"):
        algo.model.calc(algo.data, np.full((3, 1), 5e-8), 0.5)

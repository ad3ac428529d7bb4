"""The trace of a wavefront-per-chain analysis (mcsas_hip_plan_set_trace / _fetch_trace / mcsas_hip_analyse_traced,
engine.analyse(trace=), Plan.set_trace, McSAS.calc(trace=)): what can be checked without a GPU — the additive C ABI, the layout of
mcsas_trace and every refusal that is made before a device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import _lib, engine
from helpers import PythonOnlySphere, make_models
from chain_cases import MCSAS_EINVAL, _NoLibrary, _algo_40q, _data, _problem, _traced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcsas_hip.h")
NEW = {"mcsas_hip_plan_set_trace", "mcsas_hip_plan_fetch_trace", "mcsas_hip_analyse_traced"}
FIELDS = ("struct_size", "capacity", "count", "chisq0", "step", "chisq", "values")


def test_the_abi_is_extended_not_changed():
    text = open(HEADER).read()
    assert NEW <= set(re.findall(r"\b(mcsas_hip_[a-z_0-9]+)\s*\(", text)) and NEW <= set(_lib.SYMBOLS)
    assert re.search(r"#define\s+MCSAS_ABI_VERSION\s+5\b", text) and _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW) and lib.mcsas_hip_abi_version() == 5


def test_trace_layout_matches_the_header(tmp_path):
    src = tmp_path / "tr.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(mcsas_trace));\n%s\nprintf("\\n"); return 0;}\n'
                   % (HEADER, "\n".join('printf(" %%zu", offsetof(mcsas_trace, %s));' % f for f in FIELDS)))
    subprocess.check_call(["gcc", "-o", str(tmp_path / "tr"), str(src)])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "tr")]).split()]
    assert [name for name, _ in _lib.Trace._fields_] == list(FIELDS)
    assert out == [C.sizeof(_lib.Trace)] + [getattr(_lib.Trace, f).offset for f in FIELDS]


def test_analyse_traced_refuses_before_a_device_is_touched():
    if _lib.load().mcsas_hip_device_count() == 0:
        # the yardstick of "before a device is touched": here the untraced call has no device to answer with
        prob, res = _problem()
        assert _lib.load().mcsas_hip_analyse(C.byref(prob.c), C.byref(res.c)) == -2
    for mode, name in ((engine.EXEC_PIPELINE, "MCSAS_EXEC_PIPELINE"), (engine.EXEC_WORKGROUP, "MCSAS_EXEC_WORKGROUP")):
        prob, res = _problem(exec_mode=mode)
        rc, msg = _traced(prob, res, engine.ChainTrace(4, 1, 2))
        assert rc == MCSAS_EINVAL and name in msg and "MCSAS_EXEC_WAVE" in msg, msg
    prob, res = _problem(nq=5000)
    rc, msg = _traced(prob, res, engine.ChainTrace(4, 1, 2))
    assert rc == MCSAS_EINVAL and "5000" in msg and "4096" in msg, msg
    prob, res = _problem()
    prob.c.n_devices = 2
    rc, msg = _traced(prob, res, engine.ChainTrace(4, 1, 2))
    assert rc == MCSAS_EINVAL and "n_devices 2" in msg, msg
    # the trace block itself
    prob, res = _problem()
    rc, msg = _traced(prob, res, None)
    assert rc == MCSAS_EINVAL and "trace is NULL" in msg, msg
    for field in ("count", "chisq0", "step", "chisq", "values"):
        tr = engine.ChainTrace(4, 1, 2)
        setattr(tr.c, field, None)
        rc, msg = _traced(prob, res, tr)
        assert rc == MCSAS_EINVAL and ("trace array %s is NULL" % field) in msg, msg
    for capacity in (0, -3):
        tr = engine.ChainTrace(4, 1, 2)
        tr.c.capacity = capacity
        rc, msg = _traced(prob, res, tr)
        assert rc == MCSAS_EINVAL and ("capacity %d" % capacity) in msg, msg
    tr = engine.ChainTrace(4, 1, 2)
    tr.c.struct_size = C.sizeof(_lib.Trace) - 8
    rc, msg = _traced(prob, res, tr)
    assert rc == MCSAS_EINVAL and "mcsas_trace size" in msg, msg
    tr = engine.ChainTrace(4, 1, 2)
    tr.c.capacity = 2 ** 31 - 1                                    # 2 repetitions x 24 bytes per move: far beyond 2 GiB
    rc, msg = _traced(prob, res, tr)
    assert rc == MCSAS_EINVAL and "2 GiB" in msg, msg
    # a start that is not finite
    bad = np.full((8, 1, 2), 5e-8)
    bad[5, 0, 1] = np.nan
    rc, msg = _traced(prob, res, engine.ChainTrace(4, 1, 2), start=bad)
    assert rc == MCSAS_EINVAL and "not finite" in msg and "[5][0][1]" in msg, msg


def test_plan_trace_calls_on_a_null_plan():
    lib = _lib.load()
    assert lib.mcsas_hip_plan_set_trace(None, 4) == MCSAS_EINVAL and "null plan" in lib.mcsas_hip_last_error().decode()
    tr = engine.ChainTrace(4, 1, 2)
    assert lib.mcsas_hip_plan_fetch_trace(None, 0, C.byref(tr.c)) == MCSAS_EINVAL and "null plan" in lib.mcsas_hip_last_error().decode()


def test_chain_trace_starts_as_the_sentinel():
    tr = engine.ChainTrace(3, 2, 4)
    assert tr.step.shape == (3, 4) and tr.chisq.shape == (3, 4) and tr.values.shape == (3, 2, 4) and tr.count.shape == (4,)
    assert (tr.step == -1).all() and np.isnan(tr.chisq).all() and np.isnan(tr.values).all() and np.isnan(tr.chisq0).all()
    assert set(tr.asdict()) == {"count", "chisq0", "step", "chisq", "values"}


def test_engine_refusals_come_before_any_library_call(monkeypatch):
    _NoLibrary(monkeypatch)
    q, I, sig = _data()
    m, _ = make_models("sphere", [2e-9], [3e-7])
    for mode in (engine.EXEC_WORKGROUP, engine.EXEC_PIPELINE):
        with pytest.raises(ValueError, match="exec_mode %d" % mode):
            engine.analyse(m.setup(), q, I, sig, engine.Settings(n_contrib=8, n_reps=3, max_iter=10, exec_mode=mode), trace=16)
    st = engine.Settings(n_contrib=8, n_reps=3, max_iter=10)
    qq, II, ss = _data(engine.WAVE_MAX_Q + 1)
    with pytest.raises(ValueError, match=str(engine.WAVE_MAX_Q)):
        engine.analyse(m.setup(), qq, II, ss, st, trace=16)
    host = m.setup()
    host.model_id = engine.MODEL_HOST
    with pytest.raises(ValueError, match="host code"):
        engine.analyse(host, q, I, sig, st, trace=16)
    with pytest.raises(ValueError, match="device list"):
        engine.analyse(m.setup(), q, I, sig, engine.Settings(n_contrib=8, n_reps=3, max_iter=10, devices=(0, 0)), trace=16)
    with pytest.raises(ValueError, match=">= 1"):
        engine.analyse(m.setup(), q, I, sig, st, trace=0)


def test_front_end_refusals(monkeypatch):
    _NoLibrary(monkeypatch)
    for mode in (engine.EXEC_PIPELINE, engine.EXEC_WORKGROUP):
        for call in ("calc", "analyse"):
            with pytest.raises(ValueError, match="execMode %d" % mode):
                getattr(_algo_40q(execMode=mode), call)(trace=16)
    with pytest.raises(ValueError, match="device list"):
        _algo_40q(device=[0, 0]).calc(trace=16)
    algo = _algo_40q()
    qq, II, ss = _data(engine.WAVE_MAX_Q + 1)
    algo.data = mcsas_amd.SASData(qq, II, ss)
    with pytest.raises(ValueError, match=str(engine.WAVE_MAX_Q)):
        algo.calc(trace=16)
    algo = _algo_40q()
    hm = PythonOnlySphere()
    hm.radius.setActiveRange((2e-9, 3e-7))
    algo.model = hm
    with pytest.raises(ValueError, match="host code"):
        algo.calc(trace=16)
    with pytest.raises(ValueError, match=">= 1"):
        _algo_40q().calc(trace=0)

"""The trace of a q-split workgroup analysis (MCSAS_EXEC_WORKGROUP with more than 1024 q-points: chain_wide_trace_kernel behind
mcsas_hip_plan_set_trace / mcsas_hip_analyse_traced, engine.analyse(trace=), McSAS.calc(trace=)): what can be checked without a GPU —
the tables the seventh kernel family has to be entered into, and the acceptances and refusals that are made before a device is
touched, in the library and in Python."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import _lib, engine
from helpers import make_models
from chain_cases import CSRC, MCSAS_EINVAL, MCSAS_ENODEV, MCSAS_OK, WG, _LibraryReached, _algo_nq, _code, _data, _problem, _stub_library, _traced


def test_the_traced_q_split_family_is_entered_in_every_table():
    """Seven families; KF_WIDE_TRACE has its row in the table beside the enum (the q-split family's shape: no flag, startable), its
    pair of lookups in ROW_K, a unit per model through the shared q-split table, and its Makefile rule."""
    families = re.search(r"enum\s+KernelFamily\s*\{([^}]*)\}", _code("host_internal.h")).group(1).replace(" ", "").split(",")
    assert len(families) == 8 and families[-1] == "KF_COUNT" and len(set(families)) == 8, families
    k = families.index("KF_WIDE_TRACE")
    table = re.search(r"KERNEL_FAMILY\[KF_COUNT\]\s*=\s*\{(.*?)\};", _code("host_internal.h"), re.S).group(1)
    rows = re.findall(r'\{\s*"[\w -]*"\s*,\s*"(\w+)"\s*,\s*"([\w ]+)"\s*,\s*(true|false)\s*,\s*(true|false)\s*,\s*(?:true|false)\s*(?:,\s*FamilyInfo::\w+\s*)+\}', table)
    assert len(rows) == 7 and len({key for _, key, _, _ in rows}) == 7, rows
    assert rows[k][0] == "chain_wide_trace_kernel" and rows[k][2:] == ("false", "true"), rows[k]
    assert rows[k][2:] == rows[families.index("KF_WIDE")][2:]                   # (the arguments behind <model, qpl> of its untraced twin)
    row_k = re.search(r"#define ROW_K\(m\)(.*?)\n(?!\s)", _code("mcsas_hip.hip").replace("\\\n", " "), re.S).group(1)
    pairs = re.findall(r"\{\s*(\w+)##m\s*,\s*(\w+##m|nullptr)\s*\}", row_k)
    assert len(pairs) == 7 and pairs[k] == ("mcsas_wide_trace_kernel_m", "mcsas_wide_trace_kernel_given_m##m"), pairs
    unit = _code("kern_wide_trace.hip")
    assert re.search(r"MCSAS_WIDE_LOOKUP\(\s*mcsas_wide_trace_kernel_m\s*,\s*chain_wide_trace_kernel\s*,\s*false\s*\)", unit)
    assert re.search(r"MCSAS_WIDE_LOOKUP\(\s*mcsas_wide_trace_kernel_given_m\s*,\s*chain_wide_trace_kernel\s*,\s*true\s*\)", unit)
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "kern_wide_trace_m$(m).o" in make and re.search(r"kern_wide_trace_m%\.o:\s*kern_wide_trace\.hip \$\(WIDE_HDRS\)", make)
    # the kernel's text comes out of chain_wide.h, which is among the texts of the plug-in compiler: the library holds it
    assert "chain_wide_trace_kernel" in _code("chain_wide.h")
    _lib.load()
    assert b"#define MCSAS_WIDE_KERNEL chain_wide_trace_kernel" in open(_lib.LIB_PATH, "rb").read()   # (the embedded header's own line)


def test_analyse_traced_takes_the_workgroup_mode_beyond_1024_q():
    """Past the argument checks means as far as the device: where there is none the traced call answers what the untraced one answers
    (MCSAS_ENODEV), with one the ten steps run."""
    lib = _lib.load()
    for nq in (1025, 5000):
        prob, res = _problem(nq=nq, exec_mode=WG)
        plain = lib.mcsas_hip_analyse(C.byref(prob.c), C.byref(res.c))
        assert plain in (MCSAS_ENODEV, MCSAS_OK), lib.mcsas_hip_last_error().decode()
        if lib.mcsas_hip_device_count() == 0:
            assert plain == MCSAS_ENODEV
        for start in (None, np.full((8, 1, 2), 5e-8)):
            prob, res = _problem(nq=nq, exec_mode=WG)
            rc, msg = _traced(prob, res, engine.ChainTrace(4, 1, 2), start=start)
            assert rc == plain, (nq, rc, msg)
    prob, res = _problem(nq=20000, exec_mode=WG)
    rc, msg = _traced(prob, res, engine.ChainTrace(4, 1, 2))
    assert rc == MCSAS_EINVAL and "20000" in msg and "16384" in msg, msg


def test_refusals_that_stay():
    # the workgroup-window kernel's q range: the old sentence
    for nq in (40, 1024):
        prob, res = _problem(nq=nq, exec_mode=WG)
        rc, msg = _traced(prob, res, engine.ChainTrace(4, 1, 2))
        assert rc == MCSAS_EINVAL and "exec_mode 2 (MCSAS_EXEC_WORKGROUP) asked; a trace needs exec_mode = MCSAS_EXEC_WAVE (1, or 0)" in msg, msg
    prob, res = _problem(nq=1500, exec_mode=engine.EXEC_PIPELINE)
    rc, msg = _traced(prob, res, engine.ChainTrace(4, 1, 2))
    assert rc == MCSAS_EINVAL and "MCSAS_EXEC_PIPELINE" in msg and "a trace needs exec_mode = MCSAS_EXEC_WAVE" in msg, msg
    # AUTO and WAVE beyond 4096 q: the message keeps its numbers and names the way out
    for mode in (engine.EXEC_AUTO, engine.EXEC_WAVE):
        prob, res = _problem(nq=5000, exec_mode=mode)
        rc, msg = _traced(prob, res, engine.ChainTrace(4, 1, 2))
        assert rc == MCSAS_EINVAL and "5000" in msg and "4096" in msg and "MCSAS_EXEC_WORKGROUP" in msg and "1025" in msg and "16384" in msg, msg
    # a device list, a non-finite start and the 2 GiB rule in the new path
    prob, res = _problem(nq=1500, exec_mode=WG)
    prob.c.n_devices = 2
    rc, msg = _traced(prob, res, engine.ChainTrace(4, 1, 2))
    assert rc == MCSAS_EINVAL and "n_devices 2" in msg, msg
    bad = np.full((8, 1, 2), 5e-8)
    bad[5, 0, 1] = np.nan
    prob, res = _problem(nq=1500, exec_mode=WG)
    rc, msg = _traced(prob, res, engine.ChainTrace(4, 1, 2), start=bad)
    assert rc == MCSAS_EINVAL and "not finite" in msg, msg
    tr = engine.ChainTrace(4, 1, 2)
    tr.c.capacity = 2 ** 31 - 1
    rc, msg = _traced(prob, res, tr)
    assert rc == MCSAS_EINVAL and "2 GiB" in msg, msg


def test_python_checks_let_the_workgroup_mode_through_beyond_1024_points(monkeypatch):
    _stub_library(monkeypatch)
    m, _ = make_models("sphere", [2e-9], [3e-7])
    st = engine.Settings(n_contrib=8, n_reps=3, max_iter=10, exec_mode=WG)
    q, I, sig = _data(1025)
    for start in (None, np.full((8, 1, 3), 5e-8)):
        with pytest.raises(_LibraryReached):
            engine.analyse(m.setup(), q, I, sig, st, start=start, trace=16)
    q, I, sig = _data(1024)
    with pytest.raises(ValueError, match="exec_mode 2"):
        engine.analyse(m.setup(), q, I, sig, st, trace=16)
    with pytest.raises(ValueError, match="device list"):
        engine.analyse(m.setup(), *_data(1025), engine.Settings(n_contrib=8, n_reps=3, max_iter=10, exec_mode=WG, devices=(0, 0)), trace=16)
    # the front end: un-binned data with the workgroup mode asked, cold and started
    good = np.full((8, 1, 3), 5e-8)
    for kw in ({}, {"start": good}):
        with pytest.raises(_LibraryReached):
            _algo_nq(4097, execMode=WG).calc(trace=16, **kw)
        with pytest.raises(_LibraryReached):
            _algo_nq(1025, execMode=WG).analyse(trace=16, **kw)
    assert _algo_nq(4097, execMode=WG)._check_trace_mode(16) == WG and _algo_nq(1025, execMode=WG)._check_trace_mode(16) == WG
    assert _algo_nq(1500)._check_trace_mode(16) == engine.EXEC_WAVE and _algo_nq(1500, execMode=engine.EXEC_WAVE)._check_trace_mode(16) == engine.EXEC_WAVE
    for nq in (40, 1024):
        with pytest.raises(ValueError, match="execMode 2"):
            _algo_nq(nq, execMode=WG).calc(trace=16)
    with pytest.raises(ValueError, match="execMode 3"):
        _algo_nq(4097, execMode=engine.EXEC_PIPELINE).calc(trace=16)
    with pytest.raises(ValueError, match="device list"):
        _algo_nq(4097, execMode=WG, device=[0, 0]).calc(trace=16)


def test_the_trace_never_picks_the_mode(monkeypatch):
    """AUTO (and WAVE) beyond 4096 points still raise, with or without a start, and the message names the workgroup mode."""
    _stub_library(monkeypatch)
    m, _ = make_models("sphere", [2e-9], [3e-7])
    q, I, sig = _data(engine.WAVE_MAX_Q + 1)
    for mode in (engine.EXEC_AUTO, engine.EXEC_WAVE):
        with pytest.raises(ValueError, match=r"4096.*exec_mode to workgroup"):
            engine.analyse(m.setup(), q, I, sig, engine.Settings(n_contrib=8, n_reps=3, max_iter=10, exec_mode=mode), trace=16)
        for kw in ({}, {"start": np.full((8, 1, 3), 5e-8)}):
            with pytest.raises(ValueError, match=r"4096.*set execMode to workgroup"):
                _algo_nq(engine.WAVE_MAX_Q + 1, execMode=mode).calc(trace=16, **kw)

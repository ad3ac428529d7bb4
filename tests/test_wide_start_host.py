"""A start for the q-split workgroup kernel (MCSAS_EXEC_WORKGROUP with more than 1024 q-points): what can be checked without a GPU
— the refusals and acceptances that are made before a device is touched, in Python and in the library, and the tables a new kernel
family has to be entered into."""
import os
import re

import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import _lib, engine
from helpers import make_models
from chain_cases import CSRC, MCSAS_EINVAL, MCSAS_ENODEV, MCSAS_OK, _LibraryReached, _algo_nq, _code, _data, _from, _problem, _stub_library


def test_front_end_takes_the_workgroup_mode_beyond_1024_points(monkeypatch):
    _stub_library(monkeypatch)
    good = np.full((8, 1, 3), 5e-8)
    with pytest.raises(_LibraryReached):
        _algo_nq(1500, execMode=engine.EXEC_WORKGROUP).calc(start=good)
    with pytest.raises(ValueError, match="execMode"):
        _algo_nq(40, execMode=engine.EXEC_WORKGROUP).calc(start=good)
    with pytest.raises(ValueError, match="execMode"):
        _algo_nq(1024, execMode=engine.EXEC_WORKGROUP).calc(start=good)
    with pytest.raises(ValueError, match="execMode"):
        _algo_nq(1500, execMode=engine.EXEC_PIPELINE).calc(start=good)
    # the mode a started problem asks for: one wavefront per chain while it takes the data, the workgroup mode where nothing else does
    for nq, mode, asked in ((1500, engine.EXEC_AUTO, engine.EXEC_WAVE), (1500, engine.EXEC_WORKGROUP, engine.EXEC_WORKGROUP),
                            (4096, engine.EXEC_AUTO, engine.EXEC_WAVE), (4097, engine.EXEC_AUTO, engine.EXEC_WORKGROUP),
                            (4097, engine.EXEC_WAVE, engine.EXEC_WAVE), (40, engine.EXEC_AUTO, engine.EXEC_WAVE)):
        algo = _algo_nq(nq, execMode=mode)
        assert algo._problem(start=good)["st"].exec_mode == asked, (nq, mode)
        assert algo._problem()["st"].exec_mode == mode, (nq, mode)              # (without a start: what was set)
    # a series checks each data set against its own size
    algo = _algo_nq(40, execMode=engine.EXEC_WORKGROUP)
    with pytest.raises(ValueError, match="execMode"):
        mcsas_amd.run_series(algo, [_algo_nq(1500).data, _algo_nq(40).data], start=good)


def test_analyse_many_with_a_start_and_the_workgroup_mode(monkeypatch):
    m, _ = make_models("sphere", [2e-9], [3e-7])
    st = engine.Settings(n_contrib=8, n_reps=3, max_iter=10, exec_mode=engine.EXEC_WORKGROUP)
    q, I, sig = _data(40)
    monkeypatch.setattr(_lib, "load", lambda *a, **k: None)      # (asked for at the top of the call; the check must need nothing of it)
    with pytest.raises(ValueError, match="exec_mode 2"):
        engine.analyse_many([dict(model=m.setup(), q=q, intensity=I, sigma=sig, st=st, start=np.full((8, 1, 3), 5e-8))])


def test_analyse_from_takes_the_workgroup_mode_beyond_1024_q():
    """Past the argument checks means as far as the device: MCSAS_ENODEV where there is none, and with one the ten steps run."""
    start = np.full((8, 1, 2), 5e-8)
    for nq in (1500, 5000):
        prob, res = _problem(nq=nq, exec_mode=engine.EXEC_WORKGROUP)
        rc, msg = _from(prob, start, res)
        assert rc in (MCSAS_ENODEV, MCSAS_OK), (rc, msg)
    prob, res = _problem(nq=20000, exec_mode=engine.EXEC_WORKGROUP)
    rc, msg = _from(prob, start, res)
    assert rc == MCSAS_EINVAL and "20000" in msg and "16384" in msg, msg
    # the message of the wave limit names the way out
    prob, res = _problem(nq=5000)
    rc, msg = _from(prob, start, res)
    assert rc == MCSAS_EINVAL and "MCSAS_EXEC_WORKGROUP" in msg and "1025" in msg and "16384" in msg, msg
    # refusals that stay: the workgroup-window kernel's q range, a non-finite start in the new path
    prob, res = _problem(nq=1024, exec_mode=engine.EXEC_WORKGROUP)
    rc, msg = _from(prob, start, res)
    assert rc == MCSAS_EINVAL and "MCSAS_EXEC_WORKGROUP" in msg and "1024" in msg, msg
    bad = start.copy()
    bad[5, 0, 1] = np.nan
    prob, res = _problem(nq=1500, exec_mode=engine.EXEC_WORKGROUP)
    rc, msg = _from(prob, bad, res)
    assert rc == MCSAS_EINVAL and "not finite" in msg, msg


def test_the_new_family_is_entered_in_every_table():
    """A kernel is (family, given): one row per family in the table beside the enum, the started q-split kernels compiled by a unit
    of their own, and no copy of a kernel template for the start."""
    families = re.search(r"enum\s+KernelFamily\s*\{([^}]*)\}", _code("host_internal.h")).group(1).replace(" ", "").split(",")
    assert families[-1] == "KF_COUNT" and "KF_WIDE" in families[:-1] and len(set(families)) == len(families)
    n = len(families) - 1
    table = re.search(r"KERNEL_FAMILY\[KF_COUNT\]\s*=\s*\{(.*?)\};", _code("host_internal.h"), re.S).group(1)
    rows = re.findall(r'\{\s*"[\w -]*"\s*,\s*"(\w+)"\s*,\s*"([\w ]+)"\s*(?:,\s*(?:true|false)\s*)+(?:,\s*FamilyInfo::\w+\s*)+\}', table)
    assert len(rows) == n and rows[families.index("KF_WIDE")][0] == "chain_wide_kernel", rows
    assert "FAMILY[" not in _code("host_plugin.hip") and "plugin_kernel_name(" in _code("host_plugin.hip")       # (no table of its own)
    assert len(re.findall(r"\{[^{}]*\}", table)) == n, table                    # (no row of another shape)
    assert len({key for _, key in rows}) == n                                    # (the program keys tell the families apart)
    # the built-in models: one row of lookups per family, cold and started, for every model of the list
    row_k = re.search(r"#define ROW_K\(m\)(.*?)\n(?!\s)", _code("mcsas_hip.hip").replace("\\\n", " "), re.S).group(1)
    pairs = re.findall(r"\{\s*(\w+)##m\s*,\s*(\w+##m|nullptr)\s*\}", row_k)
    assert len(pairs) == n, row_k
    assert pairs[families.index("KF_WIDE")] == ("mcsas_wide_kernel_m", "mcsas_wide_kernel_given_m##m"), pairs
    assert re.search(r"BUILTIN\[MCSAS_MODEL_COUNT\]\[KF_COUNT\]\[2\]\s*=\s*\{\s*MCSAS_FOR_MODELS\(ROW_K\)\s*\}", _code("mcsas_hip.hip"))
    # one translation unit per model, and the lookup the host links against: the started instances of the shared table
    assert re.search(r"MCSAS_WIDE_LOOKUP\(\s*mcsas_wide_kernel_given_m\s*,\s*chain_wide_kernel\s*,\s*true\s*\)", _code("kern_wide_start.hip"))
    lookup = re.search(r"#define MCSAS_WIDE_LOOKUP\(LOOKUP, KERNEL, GIVEN\)(.*?)\n(?!\s)", _code("kern_lookup.h").replace("\\\n", " "), re.S).group(1)
    assert "KERNEL<MCSAS_M, 8, GIVEN>" in lookup and "CAT(LOOKUP, MCSAS_M)" in lookup
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "kern_wide_start_m$(m).o" in make and re.search(r"kern_wide_start_m%\.o:\s*kern_wide_start\.hip \$\(WIDE_HDRS\)", make)
    # the start is a template parameter, not a second template
    for name in sorted(os.listdir(CSRC)):
        assert "_start_kernel" not in open(os.path.join(CSRC, name)).read(), name


def test_every_included_text_is_embedded_for_the_plugin_compiler():
    """What a kernel header includes by name must be among the texts the run-time compiler is handed (Makefile: EMBED), and a
    dependency of the units that compile it."""
    make = open(os.path.join(CSRC, "Makefile")).read()
    embed = re.search(r"^EMBED :=(.*?)\n(?!\s)", make, re.S | re.M).group(1)
    embedded = set(re.findall(r"([\w.]+)=", embed))
    assert "chain_wide.h" in embedded
    todo, seen = ["chain_wave.h", "chain_wg.h", "chain_wide.h", "chain_pipe.h", "small_kernels.h", "plugin_model.h"], set()
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        assert name in embedded or name == "mcsas_hip.h", name
        path = os.path.join(CSRC, name)
        if os.path.exists(path):
            todo += [os.path.basename(x) for x in re.findall(r'#\s*include\s+"([\w./]+)"', _code(name))]
    incs = [x for x in seen if x.endswith(".inc")]
    assert "chain_wave_kernel.inc" in incs and "chain_body.inc" in incs
    wide_hdrs = re.search(r"^WIDE_HDRS :=(.*)$", make, re.M).group(1).split()
    assert set(re.findall(r'#\s*include\s+"([\w.]+\.inc)"', _code("chain_wide.h"))) <= set(wide_hdrs)

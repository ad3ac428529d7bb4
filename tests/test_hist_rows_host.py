"""CPU-side checks (no GPU) of histogram() on rows the caller fills on the device (include/mcsas_hip.h: mcsas_hip_histogram_rows_shape,
mcsas_hip_histogram_device_rows): the two symbols, the shape rule, every refusal made before a device is touched — in the sentences
of mcsas_hip_histogram where the refusal is its own —, the ValueErrors of the Python front and the routing of McSAS.histogram()."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import _lib, engine, series

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcsas_hip.h")
NEW = ("mcsas_hip_histogram_rows_shape", "mcsas_hip_histogram_device_rows")


def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    declared = set(re.findall(r"\b(mcsas_hip_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.mcsas_hip_abi_version() == _lib.ABI_VERSION == 5          # additive: the ABI version stays


def _shape(n_contrib, n_reps, nq):
    return engine.histogram_rows_shape(mcsas_amd.Sphere().setup(), np.linspace(1e8, 1e9, nq), (n_contrib, n_reps))


def test_shape_rule():
    assert _shape(60, 5, 100) == (60, 300, 100)
    # 256 MiB of rows of 16384 doubles are 2048 rows, less than one repetition: a round is never less than one
    assert _shape(4096, 50, 16384) == (4096, 4096, 16384)
    assert _shape(1, 3, 64) == (1, 3, 64)
    # the cap, rounded down to whole repetitions: 256 MiB / (100 * 8) = 335544 rows = 1118 repetitions of 300 and 144 rows
    assert _shape(300, 5000, 100) == (300, 1118 * 300, 100)
    st = engine.Settings(n_contrib=60, n_reps=5)
    assert engine.histogram_rows_shape(mcsas_amd.Sphere().setup(), np.linspace(1e8, 1e9, 100), st) == (60, 300, 100)
    lib = _lib.load()
    assert lib.mcsas_hip_histogram_rows_shape(None, None, None, None) == -1
    assert "problem is NULL" in lib.mcsas_hip_last_error().decode()
    prob = engine.HipProblem(mcsas_amd.Sphere().setup(), [1e8, 2e8], [1., 1.], [1., 1.], engine.Settings())
    assert lib.mcsas_hip_histogram_rows_shape(C.byref(prob.c), None, None, None) == 0        # (any of the three may be NULL)
    prob.c.n_reps = 0
    assert lib.mcsas_hip_histogram_rows_shape(C.byref(prob.c), None, None, None) == -1
    prob.c.n_reps = 1
    prob.c.struct_size += 8
    assert lib.mcsas_hip_histogram_rows_shape(C.byref(prob.c), None, None, None) == -1
    assert "ABI mismatch" in lib.mcsas_hip_last_error().decode()


# Runs in a process of its own with every device hidden: a call that passes all the checks made before a device is touched then ends
# with MCSAS_ENODEV (the control), so MCSAS_EINVAL shows that the refusal came first.  Nothing is ever read through the three
# buffer addresses.  `same`: the refusal is check_hist_set's — mcsas_hip_histogram of the same arguments (the built-in Sphere as the
# model) is asked too, and its sentence is expected behind the prefix.
_REFUSALS = r"""
import ctypes as C, json, sys
import numpy as np
import mcsas_amd
from mcsas_amd import _lib, engine

lib = _lib.load()
q = np.linspace(1e8, 1e9, 100)
edges = np.linspace(1e-9, 1e-7, 11)
out = {}

def call(tag, null=(), capacity=60, n_contrib=60, n_hist=1, same=False, spec=None, **change):
    setup = mcsas_amd.Sphere().setup()
    prob = engine.HipProblem(setup, q, np.ones(100), np.ones(100), engine.Settings(n_contrib=n_contrib, n_reps=3))
    keep = []
    for k, v in change.items():
        if k == "no_q":
            prob.c.q = None
        elif k == "smear":
            keep = [np.ones((100, v)), np.ones(v), np.ones(v)]
            prob.c.smear_nk = v
            prob.c.smear_locs, prob.c.smear_q_offset, prob.c.smear_weights = (_lib.as_dp(a) for a in keep)
        else:
            setattr(prob.c, k, v)
    contribs = np.full((n_contrib, 1, 3), 5e-8)
    arr = (_lib.HistogramSpec * 1)()
    a = arr[0]
    a.param_index, a.weighting, a.n_bin, a.lower, a.upper, a.edges = 0, 0, 10, 1e-9, 1e-7, _lib.as_dp(edges)
    for k, v in (spec or {}).items():
        setattr(a, k, v)
    sc, frac, res = np.zeros((2, 3)), np.zeros((8, n_contrib, 3)), np.zeros(3 * 10 * 3 + 5 * 3)
    cb = _lib.DeviceRowsCallback() if "rows_cb" in null else _lib.DeviceRowsCallback(lambda user, n: 0)
    specs_p = None if "specs" in null else arr
    sc_p = None if "scaling" in null else _lib.as_dp(sc)
    if same:
        rc = lib.mcsas_hip_histogram(C.byref(prob.c), _lib.as_dp(contribs), n_hist, specs_p, sc_p, _lib.as_dp(frac), _lib.as_dp(res))
        out[tag + ":builtin"] = [rc, lib.mcsas_hip_last_error().decode()]
    if "model_id" not in change:
        prob.c.model_id = engine.MODEL_HOST
    rc = lib.mcsas_hip_histogram_device_rows(None if "problem" in null else C.byref(prob.c),
                                             None if "contribs" in null else _lib.as_dp(contribs),
                                             None if "d_pset" in null else C.c_void_p(0x10000),
                                             None if "d_rows" in null else C.c_void_p(0x20000),
                                             None if "d_vws" in null else C.c_void_p(0x30000), capacity, cb, None, n_hist, specs_p, sc_p,
                                             None if "fractions" in null else _lib.as_dp(frac), None if "out" in null else _lib.as_dp(res))
    out[tag] = [rc, lib.mcsas_hip_last_error().decode()]

call("control")
call("control_no_fractions", null=("fractions",))
call("control_no_histograms", n_hist=0, null=("specs",))
call("control_unknown_model", model_id=12345)             # the model is the callback's business
for name in ("problem", "contribs", "d_pset", "d_rows", "d_vws", "rows_cb", "out"):
    call("null_" + name, null=(name,))
call("struct_size", struct_size=C.sizeof(_lib.Problem) - 8)
call("capacity", capacity=59)
call("capacity_0", capacity=0)
call("nq_0", nq=0)
call("n_reps_0", n_reps=0)
call("n_active_0", n_active=0, n_hist=0)
call("n_active_5", n_active=5, n_hist=0)
call("smear", smear=5)
call("smear_count_only", smear_nk=3)
call("null_scaling", null=("scaling",), same=True)
call("no_q", no_q=True, same=True)
call("null_specs", null=("specs",), same=True)
call("n_hist_neg", n_hist=-1, same=True)
call("too_many", n_contrib=4097, capacity=4097, same=True)
call("weighting", spec=dict(weighting=4), same=True)
call("param_index", spec=dict(param_index=1), same=True)
call("n_bin_neg", spec=dict(n_bin=-1), same=True)
call("n_bin_big", spec=dict(n_bin=(1 << 20) + 1), same=True)
call("no_edges", spec=dict(edges=None), same=True)

def front(tag, **kw):
    args = dict(model=mcsas_amd.Sphere().setup(), q=q, intensity=np.ones(100), sigma=np.ones(100), contribs=np.full((60, 1, 3), 5e-8),
                specs=[dict(param_index=0, yweight="vol", edges=edges, lower=1e-9, upper=1e-7)], row_fn=None)
    args.update(kw)
    try:
        engine.histogram_device_rows(**args)
        out[tag] = ["no error", ""]
    except Exception as e:
        out[tag] = [type(e).__name__, str(e)]

front("py_capacity", capacity=59)
front("py_contribs_2d", contribs=np.full((60, 3), 5e-8))
front("py_contribs_p", contribs=np.full((60, 2, 3), 5e-8))
front("py_yweight", specs=[dict(param_index=0, yweight="mass", edges=edges, lower=1e-9, upper=1e-7)])
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def refusals():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _REFUSALS], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("tag", ["control", "control_no_fractions", "control_no_histograms", "control_unknown_model"])
def test_the_control_calls_find_no_device(refusals, tag):
    assert refusals[tag][0] == -2, refusals[tag]                         # MCSAS_ENODEV: every check before the device passed


@pytest.mark.parametrize("tag, words", [
    ("null_problem", "problem is NULL"), ("null_contribs", "contribs is NULL"), ("null_d_pset", "d_pset is NULL"),
    ("null_d_rows", "d_rows is NULL"), ("null_d_vws", "d_vws is NULL"), ("null_rows_cb", "rows_cb is NULL"), ("null_out", "out is NULL"),
    ("struct_size", "ABI mismatch"), ("capacity", "capacity_rows 59 < 60"), ("capacity_0", "capacity_rows 0 < 60"),
    ("nq_0", "nq 0"), ("n_reps_0", "n_reps 0"), ("n_active_0", "n_active 0"), ("n_active_5", "n_active 5"),
    ("smear", "smearing table (smear_nk 5)"), ("smear_count_only", "smearing table (smear_nk 3)")])
def test_refused_before_a_device_is_touched(refusals, tag, words):
    rc, msg = refusals[tag]
    assert rc == -1, (tag, rc, msg)                                      # MCSAS_EINVAL, not MCSAS_ENODEV
    assert msg.startswith("histogram_device_rows: ") and words in msg, (tag, msg)


@pytest.mark.parametrize("tag, words", [
    ("null_scaling", "bad argument"), ("no_q", "bad argument"), ("null_specs", "bad argument"), ("n_hist_neg", "bad argument"),
    ("too_many", "n_contrib 4097 > 4096"), ("weighting", "histogram 0: param_index 0, weighting 4, n_bin 10"),
    ("param_index", "histogram 0: param_index 1"), ("n_bin_neg", "n_bin -1"), ("n_bin_big", "n_bin 1048577"), ("no_edges", "histogram 0")])
def test_what_the_histogram_call_refuses_is_refused_in_its_sentence(refusals, tag, words):
    rc, msg = refusals[tag]
    rc_builtin, msg_builtin = refusals[tag + ":builtin"]
    assert rc == rc_builtin == -1, (tag, rc, msg, rc_builtin, msg_builtin)
    assert words in msg_builtin, (tag, msg_builtin)
    assert msg == "histogram_device_rows: " + msg_builtin, (tag, msg, msg_builtin)


def test_python_front_refuses_before_a_tensor_is_made(refusals):
    assert refusals["py_capacity"][0] == "ValueError" and "capacity 59 < 60" in refusals["py_capacity"][1]
    assert refusals["py_contribs_2d"][0] == "ValueError" and "(60, 3)" in refusals["py_contribs_2d"][1]
    assert refusals["py_contribs_p"][0] == "ValueError" and "n_active = 1" in refusals["py_contribs_p"][1]
    assert refusals["py_yweight"][0] == "KeyError"


class BatchOnlySphere(mcsas_amd.SASModel):
    """A sphere that brings nothing but calcIntensityBatch."""
    shortName = "Sphere (torch batch only)"
    parameters = mcsas_amd.Sphere.parameters

    def __init__(self):
        super().__init__()
        self.radius.setActive(True)

    def calcIntensityBatch(self, q, pset, compensationExponent):
        raise AssertionError("not evaluated in these tests")


class NumpyOnlySphere(mcsas_amd.SASModel):
    parameters = mcsas_amd.Sphere.parameters

    def __init__(self):
        super().__init__()
        self.radius.setActive(True)

    def volume(self):
        return (np.pi * 4. / 3.) * self.radius()**3

    def formfactor(self, dataset):
        qr = self.getQ(dataset) * self.radius()
        return 3. * (np.sin(qr) - qr * np.cos(qr)) / (qr**3.)


class _Reached(Exception):
    pass


def _algo(model, n_contrib=8):
    q = np.logspace(8, 9.3, 40)
    algo = mcsas_amd.McSAS(seed=1)
    algo.numContribs.setValue(n_contrib); algo.numReps.setValue(3)
    algo.findBackground.setValue(False); algo.positiveBackground.setValue(True)
    algo.model = model
    model.radius.histograms().append(mcsas_amd.Histogram(model.radius, 1e-9, 1e-7, binCount=7, xscale='lin', yweight='num'))
    algo.data = mcsas_amd.SASData(q, 1.0 / q, 0.01 / q)
    algo.result = [dict(contribs=np.full((n_contrib, 1, 3), 5e-8))]
    return algo


def test_histogram_routes_a_batch_model_to_device_rows(monkeypatch):
    seen = []

    def device_rows(**kw):
        seen.append(kw)
        raise _Reached()

    def other(*a, **k):
        raise AssertionError("not the path of a calcIntensityBatch model")
    monkeypatch.setattr(engine, "histogram_device_rows", device_rows)
    for name in ("histogram_device", "histogram_prep", "bgfit"):
        monkeypatch.setattr(engine, name, other)
    algo = _algo(BatchOnlySphere())
    with pytest.raises(_Reached):
        algo.histogram()
    kw, = seen
    assert set(kw) == {"model", "q", "intensity", "sigma", "contribs", "specs", "row_fn", "find_background", "positive_background", "device"}
    assert kw["model"].model_id == engine.MODEL_HOST and callable(kw["row_fn"])
    assert kw["find_background"] is False and kw["positive_background"] is True and kw["device"] == -1
    assert kw["contribs"] is algo.result[0]["contribs"] and len(kw["specs"]) == 1 and kw["specs"][0]["yweight"] == "num"
    # the batched histogram pass of a series keeps leaving host models to histogram()
    assert not series._histograms_batchable(algo, engine)


def test_histogram_keeps_the_host_path_where_the_new_one_does_not_apply(monkeypatch):
    def device_rows(**kw):
        raise AssertionError("histogram_device_rows must not be reached")

    def bgfit(*a, **k):
        raise _Reached()
    monkeypatch.setattr(engine, "histogram_device_rows", device_rows)
    monkeypatch.setattr(engine, "bgfit", bgfit)
    # a numpy-only model has no device rows to hand over
    with pytest.raises(_Reached):
        _algo(NumpyOnlySphere()).histogram()
    # switched off on the object
    import mcsas_amd.mcsas as front
    monkeypatch.setattr(front, "batch_model_calc", lambda *a, **k: (_ for _ in ()).throw(_Reached()))
    algo = _algo(BatchOnlySphere())
    algo.deviceRowsHistogram = False
    with pytest.raises(_Reached):
        algo.histogram()
    # beyond the contributions a repetition stages in LDS
    with pytest.raises(_Reached):
        _algo(BatchOnlySphere(), n_contrib=engine.HISTOGRAM_MAX_CONTRIBS + 1).histogram()


def test_batch_model_histogram_refuses_data_whose_smearing_would_apply(monkeypatch):
    def device_rows(**kw):
        raise AssertionError("histogram_device_rows must not be reached")
    monkeypatch.setattr(engine, "histogram_device_rows", device_rows)
    from helpers import product_smearing

    class Smearable(BatchOnlySphere):
        canSmear = True
    algo = _algo(Smearable())
    q = algo.data.q
    algo.data, _ = product_smearing("trapezoid", False, 9, q, 1.0 / q, 0.01 / q, umbra=2e-3 * q.max(), penumbra=4e-3 * q.max())
    assert algo.data.smearArgs(algo.model) is not None
    with pytest.raises(NotImplementedError, match="smear"):
        algo.histogram()

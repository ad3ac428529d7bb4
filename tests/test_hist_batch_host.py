"""mcsas_hip_histogram_batch and mcsas_hip_histogram without a GPU: the declaration, the export, and every refusal — each before a
device is touched, the batch's naming the set it is about and otherwise the single call's word for word."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import _lib, engine

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "mcsas_hip.h")
EINVAL, ENODEV = -1, -2
DPP = C.POINTER(C.c_double)


def _call(n_contrib=6, n_reps=2, nq=12, n_bins=(4, 3), device=-1):
    """One valid set: a sphere, seeded contributions inside its range, a histogram per entry of n_bins."""
    rs = np.random.RandomState(n_contrib + 7 * nq)
    q = np.geomspace(1e8, 3e9, nq)
    m = mcsas_amd.Sphere()
    lo, hi = np.pi / q.max(), np.pi / q.min()
    m.radius.setActiveRange((lo, hi))
    contribs = rs.uniform(lo, hi, (n_contrib, 1, n_reps))
    specs = [dict(param_index=0, yweight="vol", edges=np.linspace(lo, hi, nb + 1), lower=lo, upper=hi) for nb in n_bins]
    return engine._HistogramCall(m.setup(), q, 1.0 + rs.rand(nq), 0.1 + rs.rand(nq), contribs, 0.6666666, specs, device=device)


def _run(calls, n_sets=None, null=None, patch=None):
    """(return code, last error) of the batch call over `calls`; `null`: the name of a table passed as NULL; `patch`: changes the
    tables before the call."""
    lib = _lib.load()
    n = len(calls)
    tables = dict(
        problems=(_lib.Problem * max(n, 1))(*[c.prob.c for c in calls]),
        contribs=(DPP * max(n, 1))(*[_lib.as_dp(c.contribs) for c in calls]),
        n_hist=(C.c_int32 * max(n, 1))(*[len(c.specs) for c in calls]),
        specs=(C.POINTER(_lib.HistogramSpec) * max(n, 1))(*[C.cast(c.arr, C.POINTER(_lib.HistogramSpec)) for c in calls]),
        scaling=(DPP * max(n, 1))(*[_lib.as_dp(c.sc) for c in calls]),
        fractions=(DPP * max(n, 1))(*[_lib.as_dp(c.frac) for c in calls]),
        out=(DPP * max(n, 1))(*[_lib.as_dp(c.out) for c in calls]))
    if null:
        tables[null] = None
    if patch:
        patch(tables)
    rc = lib.mcsas_hip_histogram_batch(n if n_sets is None else n_sets, tables["problems"], tables["contribs"], tables["n_hist"], tables["specs"],
                                       tables["scaling"], tables["fractions"], tables["out"])
    return rc, lib.mcsas_hip_last_error().decode()


def _run_single(call, null_contribs=False):
    """(return code, last error) of mcsas_hip_histogram over one set"""
    lib = _lib.load()
    rc = lib.mcsas_hip_histogram(C.byref(call.prob.c), None if null_contribs else _lib.as_dp(call.contribs), len(call.specs), call.arr,
                                 _lib.as_dp(call.sc), _lib.as_dp(call.frac), _lib.as_dp(call.out))
    return rc, lib.mcsas_hip_last_error().decode()


def _set(obj, name, value):
    setattr(obj, name, value)


# what makes a set unacceptable: (how the valid set of _call is spoilt, the single call's message)
REFUSALS = {
    "no contributions": (None, "bad argument"),
    "nq = 0": (lambda c: _set(c.prob.c, "nq", 0), "bad argument"),
    "n_contrib = 4097": (None, "mcsas_hip_histogram stages a repetition's contributions in LDS: n_contrib 4097 > 4096 (use mcsas_hip_histogram_prep)"),
    "weighting = 7": (lambda c: _set(c.arr[1], "weighting", 7), "histogram 1: param_index 0, weighting 7, n_bin 3"),
    "param_index = 1": (lambda c: _set(c.arr[1], "param_index", 1), "histogram 1: param_index 1, weighting 0, n_bin 3"),   # (one active parameter)
    "n_bin = -1": (lambda c: _set(c.arr[0], "n_bin", -1), "histogram 0: param_index 0, weighting 0, n_bin -1"),
    "no edges": (lambda c: _set(c.arr[0], "edges", DPP()), "histogram 0: param_index 0, weighting 0, n_bin 4"),
    "model_id = 77": (lambda c: _set(c.prob.c, "model_id", 77), "unknown model_id 77"),
    "smear_nk = 1": (lambda c: _set(c.prob.c, "smear_nk", 1), "smearing: smear_nk 1 (2..4096) needs locs, q_offset and weights"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_the_single_call_refuses_before_a_device_and_a_batch_of_one_says_the_same(case):
    """Every refusal of a set is MCSAS_EINVAL (never MCSAS_ENODEV: no device is looked for) with the single call's wording, and the
    same set as a batch of one is refused with the same code and "histogram_batch: set 0: " before the same sentence: one validator."""
    spoil, wording = REFUSALS[case]
    call = _call(n_contrib=4097, n_reps=1, nq=4, n_bins=()) if case == "n_contrib = 4097" else _call()
    if spoil:
        spoil(call)
    null = case == "no contributions"
    rc, msg = _run_single(call, null_contribs=null)
    assert rc == EINVAL, (rc, msg)
    assert msg == wording

    def no_contribs(tables):
        tables["contribs"][0] = DPP()
    brc, bmsg = _run([call], patch=no_contribs if null else None)
    assert brc == rc
    assert bmsg == "histogram_batch: set 0: " + msg


def test_header_declares_the_batch_call_at_abi_5_and_the_library_exports_it():
    text = open(HEADER).read()
    assert re.search(r"\bint\s+mcsas_hip_histogram_batch\s*\(\s*int32_t\s+n_sets\s*,\s*const\s+mcsas_problem\s*\*\s*problems", text)
    assert re.search(r"#define\s+MCSAS_ABI_VERSION\s+5\b", text)
    assert "mcsas_hip_histogram_batch" in _lib.SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "mcsas_hip_histogram_batch") and lib.mcsas_hip_abi_version() == 5


def test_an_empty_batch_is_ok_without_a_device():
    assert _run([])[0] == 0
    rc, msg = _run([], n_sets=-1)
    assert rc == EINVAL and "n_sets -1" in msg


@pytest.mark.parametrize("table", ["problems", "contribs", "n_hist", "specs", "scaling", "out"])
def test_a_null_table_is_refused(table):
    rc, msg = _run([_call(), _call()], null=table)
    assert rc == EINVAL and "NULL table" in msg


def test_refusals_name_the_set_and_the_histogram():
    # a per-set check of the single call: no contributions for set 1
    def no_contribs_for_set_1(tables):
        tables["contribs"][1] = DPP()
    rc, msg = _run([_call(), _call(), _call()], patch=no_contribs_for_set_1)
    assert rc == EINVAL and "set 1" in msg
    # a bad histogram record: set 2, histogram 1
    calls = [_call(), _call(), _call()]
    calls[2].arr[1].weighting = 7
    rc, msg = _run(calls)
    assert rc == EINVAL and "set 2" in msg and "histogram 1" in msg and "weighting 7" in msg
    calls[2].arr[1].weighting = 0
    calls[2].arr[1].param_index = 1                            # (one active parameter)
    rc, msg = _run(calls)
    assert rc == EINVAL and "set 2" in msg and "histogram 1" in msg
    # a model the library does not know: set 1
    calls = [_call(), _call()]
    calls[1].prob.c.model_id = 77
    rc, msg = _run(calls)
    assert rc == EINVAL and "set 1" in msg and "77" in msg
    # no data points: set 0
    calls = [_call(), _call()]
    calls[0].prob.c.nq = 0
    rc, msg = _run(calls)
    assert rc == EINVAL and "set 0" in msg


def test_more_than_4096_contributions_is_refused_for_its_set():
    rc, msg = _run([_call(), _call(), _call(n_contrib=4097, n_reps=1, nq=4, n_bins=())])
    assert rc == EINVAL and "set 2" in msg and "4096" in msg and "4097" in msg


def test_sets_on_different_devices_are_refused():
    rc, msg = _run([_call(device=0), _call(device=0), _call(device=1)])
    assert rc == EINVAL and "set 2" in msg and "device" in msg


def test_a_valid_batch_reaches_the_device_selection():
    """No GPU here: MCSAS_ENODEV says that validation passed and the call got as far as selecting a device; the single call answers
    the same for each of the sets.  engine.histogram_device_batch raises it; an empty list needs no device."""
    if _lib.load().mcsas_hip_device_count() > 0:
        pytest.skip("a GPU is present")
    calls = [_call(), _call(n_contrib=4096, n_reps=1, nq=4, n_bins=()), _call(n_bins=())]
    rc, msg = _run(calls)
    assert rc == ENODEV, msg
    assert _run(calls, null="fractions")[0] == ENODEV          # (fractions may be NULL)
    for call in calls:
        rc, msg = _run_single(call)
        assert rc == ENODEV, msg
    c = calls[0]
    with pytest.raises(_lib.McSASHipError) as e:
        engine.histogram_device_batch([dict(model=c.prob.model, q=c.prob.q, intensity=c.prob.I, sigma=c.prob.sigma, contribs=c.contribs,
                                            comp_exp=0.6666666, specs=c.specs)])
    assert e.value.code == ENODEV
    assert engine.histogram_device_batch([]) == []

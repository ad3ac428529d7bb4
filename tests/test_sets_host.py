"""One population fitted to several data sets (mcsas_hip_analyse_sets, engine.analyse_sets, mcsas_amd.DataSets): what can be checked
without a GPU — the float64 restatement tests/sets_exact.py against the oracle, the margin condition the GPU tests rest on, the
additive C ABI and its struct, every refusal (each made before a device is touched), and the plumbing of the front end."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import _lib, engine
from oracle import mcsas_oracle as O
from helpers import PythonOnlySphere, make_models
import sets_exact as SX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcsas_hip.h")
CSRC = os.path.join(ROOT, "mcsas_amd", "csrc")
MCSAS_EINVAL, MCSAS_ENODEV = -1, -2
FIELDS = ("struct_size", "n_sets", "scaling", "background", "chisq")
MARGIN = 1e-9


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", [n for n in SX.REPLAYED if n.startswith("s1_")])
def test_with_one_set_the_restatement_is_the_oracles_chain(name):
    c = SX.case(name)
    _, spec = make_models(c["tag"], c["lo"], c["hi"])
    q, I, sig = c["sets"][0]
    ref = O.mc_fit(spec, q, I, sig, [I.min(), I.max()], [q.min(), q.max()], c["st"], O.ReplayStream(c["replay"][0]), method="closed")
    got = SX.reference(name)
    assert (got.num_iter, got.num_moves) == (ref.num_iter, ref.num_moves) and ref.num_moves > 10
    np.testing.assert_array_equal(got.rset, ref.rset)
    np.testing.assert_allclose(got.conval, ref.conval, rtol=1e-12)         # (ft + (new - old) against (ft - old) + new)
    np.testing.assert_allclose([got.set_scaling[0], got.set_background[0]], [ref.scaling, ref.background], rtol=1e-9, atol=1e-300)
    np.testing.assert_allclose(got.fit, ref.fit, rtol=1e-9)


# Kholodenko's device row follows the oracle's QUADPACK integral only to 2e-8 relatively (test_kholodenko_active_ranges_vs_quadpack_500_sets),
# not to float64 rounding as every other model's row (test_model_calc_vs_reference_vectors).  The inputs carry 1 % uncertainties: a
# relative row error eps moves every residual (I - fit) / sigma by at most eps / 0.01, so X = sum of their squares by at most about
# 2 (eps / 0.01) sqrt(X Q) absolutely, 2 (eps / 0.01) / sqrt(chi²) relatively: 4e-6 at chi² >= 1.  A margin of 1e-5 lies above that,
# as long as the chain stays at chi² >= 1, which is asserted.
KHOLODENKO_MARGIN = 1e-5


def check_margin(name, c, ref):
    """What the GPU comparisons rest on, of a replayed input and the restatement's chain on it (also tests/test_sets_shared_host.py's)."""
    print(name, "min margin %.3e" % ref.min_margin, "steps", ref.num_iter, "moves", ref.num_moves, "attempts", ref.attempts)
    if c["st"].n_contrib == 1:                                                # the Monte-Carlo loop is skipped
        P = len(c["lo"])
        assert (ref.num_iter, ref.num_moves, ref.draws, ref.attempts) == (0, 0, P, 1) and ref.rset.shape == (1, P)
        return
    assert ref.num_moves >= 5
    if c["tag"] == "kholodenko":
        lowest = min([chi2 for _, chi2 in ref.trajectory] + [ref.conval])
        print(name, "lowest chi2", lowest)
        assert ref.min_margin >= KHOLODENKO_MARGIN and lowest >= 1.0
    else:
        assert ref.min_margin >= MARGIN


@pytest.mark.parametrize("name", SX.REPLAYED)
def test_no_decision_of_the_gpu_tests_inputs_is_a_near_tie(name):
    """|X_t - X| / X >= 1e-9 at every step of every replayed input of tests/test_sets_gpu.py and tests/test_sets_matrix_gpu.py (1e-5 for
    Kholodenko): then "the device takes the restatement's decisions" is a fair demand, and inputs changed later cannot quietly make
    it an unfair one."""
    check_margin(name, SX.case(name), SX.reference(name))


def test_the_generated_inputs_are_what_their_names_say():
    """One input per (model, slot count); per-set scales a factor >= 100 apart, different backgrounds, intDiv <= 12; the edges' settings."""
    assert len(SX.MATRIX) == 40 and len(set(SX.GENERATED)) == len(SX.GENERATED) == 53
    for name in SX.GENERATED:
        c = SX.case(name)
        tag, nqs, qpl = SX.generated_shape(name)
        assert tuple(len(s[0]) for s in c["sets"]) == nqs == c["set_nq"] and c["qpl"] == qpl
        assert sum(-(-n // 64) for n in nqs) in range(qpl // 2 + 1, qpl + 1)
        assert all(v <= 12 for k, v in c["fixed"].items() if k == "intDiv") and (tag in SX.INT_DIV) == ("intDiv" in c["fixed"])
        assert 8 <= c["st"].n_contrib <= 12 or name in SX.EDGES
        assert c["st"].conv_crit == 1e-12 and c["st"].max_retries == 0 and 40 <= c["st"].max_iter <= 80
    scales = SX.PER_SET_SCALES
    assert all(max(a, b) / min(a, b) >= 100. for i, a in enumerate(scales) for b in scales[i + 1:]) and len(set(SX.BACKGROUNDS)) == 4
    assert sorted(SX.case("ed_%s_n%d" % (t, n))["st"].n_contrib for t in ("sphere", "sphcs") for n in SX.EDGE_COUNTS) == sorted(2 * SX.EDGE_COUNTS)
    for t in ("sphere", "sphcs"):
        c = SX.case("ed_%s_min" % t)
        assert c["st"].start_from_min and min(c["lo"]) > 0
        ref = SX.reference("ed_%s_min" % t)
        assert ref.draws == len(c["lo"]) * ref.num_iter                      # the initial set costs no draws
    assert SX.case("ed_sphcs_gen12")["gen"] == (1, 2) and SX.case("ed_sphcs_gen30")["gen"] == (3, 0)
    c = SX.case("ed_ellcs_nobg")
    assert not c["st"].find_bg and len(c["lo"]) == 3 and (SX.reference("ed_ellcs_nobg").set_background == 0.).all()


def test_the_inputs_end_where_their_tests_say():
    crit, retry, odd = SX.reference("end_crit"), SX.reference("end_retry"), SX.reference("end_odd")
    st = SX.case("end_crit")["st"]
    assert crit.num_iter % 64 not in (0, 63) and crit.num_iter < st.max_iter and crit.conval <= st.conv_crit      # inside a batch of 64 proposals
    st = SX.case("end_retry")["st"]
    assert retry.attempts >= 2 and retry.conval <= st.conv_crit
    assert retry.draws == retry.attempts * st.n_contrib + (retry.attempts - 1) * st.max_iter + retry.num_iter   # (one active parameter)
    assert odd.num_iter == 100 and odd.num_iter % 64
    # the sets of the boundary cases are a factor 1000 apart in scale, and the fit finds that
    b2 = SX.reference("b2")
    np.testing.assert_allclose(b2.set_scaling[1] / b2.set_scaling[0], 1e3, rtol=0.05)


def test_a_chain_on_the_acceptance_inputs_converges_within_max_iterations():
    """The front-end test asks every repetition to converge to chi² <= 1 on two sets a factor 250 apart: the restatement does, within
    the default maxIterations, with both sets near 1 and the scales' ratio within 5 % of 250."""
    spec, sets = SX.quickstart_sets()
    st = O.Settings(n_contrib=100, n_reps=1, max_iter=100000, conv_crit=1.0, max_retries=0, comp_exp=0.6666666)
    ref = SX.sets_analyse(spec, sets, st, O.PhiloxStream(7, 0))
    print("steps", ref.num_iter, "chi2", ref.conval, ref.set_chisq, "scales", ref.set_scaling)
    assert ref.conval <= 1.0 and ref.num_iter < st.max_iter and (ref.set_chisq <= 1.5).all()
    assert abs(ref.set_scaling[1] / ref.set_scaling[0] / 250. - 1.) < 0.05


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_abi_is_extended_not_changed():
    text = open(HEADER).read()
    assert "mcsas_hip_analyse_sets" in set(re.findall(r"\b(mcsas_hip_[a-z_0-9]+)\s*\(", text)) and "mcsas_hip_analyse_sets" in _lib.SYMBOLS
    assert re.search(r"#define\s+MCSAS_ABI_VERSION\s+5\b", text) and _lib.ABI_VERSION == 5
    assert re.search(r"#define\s+MCSAS_MAX_SETS\s+4\b", text) and _lib.MAX_SETS == 4 and engine.MAX_SETS == 4
    assert "mcsas.py:354-404" in text and "backgroundscalingfit.py:112-139" in text
    lib = _lib.load()
    assert hasattr(lib, "mcsas_hip_analyse_sets") and lib.mcsas_hip_abi_version() == 5
    assert hasattr(_lib.load(tuning=True), "mcsas_hip_analyse_sets")


def test_sets_result_layout_matches_the_header(tmp_path):
    src = tmp_path / "sr.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(mcsas_sets_result));\n%s\nprintf("\\n"); return 0;}\n'
                   % (HEADER, "\n".join('printf(" %%zu", offsetof(mcsas_sets_result, %s));' % f for f in FIELDS)))
    subprocess.check_call(["gcc", "-o", str(tmp_path / "sr"), str(src)])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "sr")]).split()]
    assert [name for name, _ in _lib.SetsResult._fields_] == list(FIELDS)
    assert out == [C.sizeof(_lib.SetsResult)] + [getattr(_lib.SetsResult, f).offset for f in FIELDS]


def test_the_kernel_is_a_unit_of_its_own_and_leaves_the_shared_chain_text_alone():
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "kern_wave_sets_m$(m).o" in make and re.search(r"kern_wave_sets_m%\.o:\s*kern_wave_sets\.hip \$\(SETS_HDRS\)", make)
    assert "$(BUILD)/host_sets.o" in make
    unit = open(os.path.join(CSRC, "kern_wave_sets.hip")).read()
    for qpl in (1, 2, 4, 8, 16):
        assert "chain_sets_kernel<MCSAS_M, %d>" % qpl in unit
    text = open(os.path.join(CSRC, "chain_sets.h")).read()
    assert "chain_body.inc\"" not in text and "chain_wave_kernel.inc\"" not in text        # its own chain text, no hook
    for reused in ("Contrib<M>", "RowEval<M, QPL>", "make_qtables<M>", "draw_value", "DrawSource", "wave_sum3", "stop_requested", "ChainOut"):
        assert reused in text, reused


# ------------------------------------------------------------------------------------------------ refusals
def _request(nqs=(40, 50), **st_kw):
    """-> (problem, result, sets result, set_nq) of a valid request; the caller breaks one thing."""
    m, _ = make_models("sphere", [2e-9], [3e-7])
    nq = int(sum(nqs))
    q = np.concatenate([np.logspace(7, 9, n) for n in nqs]) if nq else np.zeros(0)
    st = engine.Settings(**{**dict(n_contrib=8, n_reps=2, max_iter=10), **st_kw})
    prob = engine.HipProblem(m.setup(), q, np.ones(nq), np.ones(nq), st)
    res = engine.SetsResults(8, 1, 2, list(nqs))
    return prob, res, np.ascontiguousarray(nqs, dtype=np.int32)


def _call(prob, res, set_nq, n_sets=None):
    lib = _lib.load()
    rc = lib.mcsas_hip_analyse_sets(C.byref(prob.c), len(set_nq) if n_sets is None else n_sets, set_nq.ctypes.data_as(C.POINTER(C.c_int32)),
                                    C.byref(res.c), C.byref(res.sets_c))
    return rc, lib.mcsas_hip_last_error().decode()


def test_a_valid_request_reaches_the_device():
    """The yardstick of "before a device is touched": on a machine without one, the request that nothing is wrong with is answered
    MCSAS_ENODEV — so an MCSAS_EINVAL below was decided ahead of the device.  (With a device the request runs.)"""
    rc, msg = _call(*_request())
    assert rc == (MCSAS_ENODEV if _lib.load().mcsas_hip_device_count() == 0 else 0), msg


REFUSALS = {
    "positive_background": (dict(positive_background=True), None, "positive_background"),
    "smearing": ({}, lambda p: setattr(p.c, "smear_nk", 5), "smearing (smear_nk 5)"),
    "device_list": ({}, lambda p: setattr(p.c, "n_devices", 2), "n_devices 2"),
    "plugin": ({}, lambda p: setattr(p.c, "model_id", engine.MODEL_PLUGIN0), "plug-in"),
    "host_model": ({}, lambda p: setattr(p.c, "model_id", engine.MODEL_HOST), "host model"),
    "no_active": ({}, lambda p: setattr(p.c, "n_active", 0), "n_active == 0"),
    "no_cache": (dict(cache_intensities=0), None, "cache_intensities == 0"),
    "workgroup": (dict(exec_mode=engine.EXEC_WORKGROUP), None, "MCSAS_EXEC_WORKGROUP"),
    "pipeline": (dict(exec_mode=engine.EXEC_PIPELINE), None, "MCSAS_EXEC_PIPELINE"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_what_is_out_of_scope_is_refused_before_a_device_is_touched(what):
    st_kw, spoil, words = REFUSALS[what]
    prob, res, set_nq = _request(**st_kw)
    if spoil:
        spoil(prob)
    rc, msg = _call(prob, res, set_nq)
    assert rc == MCSAS_EINVAL and words in msg and msg.startswith("analyse_sets:"), msg


def test_the_shape_of_the_sets_is_refused_before_a_device_is_touched():
    prob, res, set_nq = _request()
    for n in (0, 5):
        rc, msg = _call(prob, res, np.ascontiguousarray([18] * 5, dtype=np.int32), n_sets=n)
        assert rc == MCSAS_EINVAL and "n_sets %d (1..4)" % n in msg, msg
    rc, msg = _call(prob, res, np.ascontiguousarray([40, 49], dtype=np.int32))
    assert rc == MCSAS_EINVAL and "sum of set_nq 89 != nq 90" in msg, msg
    rc, msg = _call(prob, res, np.ascontiguousarray([88, 2], dtype=np.int32))
    assert rc == MCSAS_EINVAL and "set 1 has 2 points" in msg and "at least 3" in msg, msg
    # 16 slots of 64 entries hold the padded sets: 4 x 193 points are 772 points and 4 x 4 = 16 slots; one point more is a 17th slot
    prob, res, set_nq = _request(nqs=(193, 193, 193, 193))
    rc, msg = _call(prob, res, set_nq)
    assert rc == (MCSAS_ENODEV if _lib.load().mcsas_hip_device_count() == 0 else 0), msg
    prob, res, set_nq = _request(nqs=(257, 193, 193, 193))
    rc, msg = _call(prob, res, set_nq)
    assert rc == MCSAS_EINVAL and "17 padded slots" in msg and "1024" in msg, msg
    # the blocks themselves
    prob, res, set_nq = _request()
    res.sets_c.struct_size -= 8
    rc, msg = _call(prob, res, set_nq)
    assert rc == MCSAS_EINVAL and "mcsas_sets_result size" in msg, msg
    prob, res, set_nq = _request()
    res.sets_c.n_sets = 3
    rc, msg = _call(prob, res, set_nq)
    assert rc == MCSAS_EINVAL and "n_sets 3" in msg, msg
    lib = _lib.load()
    assert lib.mcsas_hip_analyse_sets(None, 2, None, None, None) == MCSAS_EINVAL and "null argument" in lib.mcsas_hip_last_error().decode()


class _NoLibrary(object):
    """engine refusals that must come before any library call"""
    def __init__(self, monkeypatch):
        def boom(*a, **k):
            raise AssertionError("the library was loaded")
        monkeypatch.setattr(_lib, "load", boom)


def test_engine_refusals_come_before_any_library_call(monkeypatch):
    _NoLibrary(monkeypatch)
    m, _ = make_models("sphere", [2e-9], [3e-7])
    sets = [(np.logspace(7, 9, 20), np.ones(20), np.ones(20))] * 2
    st = engine.Settings(n_contrib=8, n_reps=2, max_iter=10)
    host = m.setup(); host.model_id = engine.MODEL_HOST
    with pytest.raises(ValueError, match="host code"):
        engine.analyse_sets(host, sets, st)
    plug = m.setup(); plug.model_id = engine.MODEL_PLUGIN0 + 1
    with pytest.raises(ValueError, match="plug-in"):
        engine.analyse_sets(plug, sets, st)
    with pytest.raises(ValueError, match="device list"):
        engine.analyse_sets(m.setup(), sets, engine.Settings(n_contrib=8, n_reps=2, max_iter=10, devices=(0, 0)))
    with pytest.raises(ValueError, match="same length"):
        engine.analyse_sets(m.setup(), [(np.ones(4), np.ones(4), np.ones(3))], st)


# ------------------------------------------------------------------------------------------------ the front end
def _algo(monkeypatch=None, histogram_set=0):
    m, _ = make_models("sphere", [2e-9], [3e-7])
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, 2e-9, 3e-7, binCount=10, xscale='log', yweight='vol'))
    algo = mcsas_amd.McSAS(seed=3)
    algo.numContribs.setValue(6); algo.numReps.setValue(3)
    algo.model = m
    d0 = mcsas_amd.SASData(np.logspace(7, 8.5, 12), np.full(12, 5.), np.full(12, .1))
    d1 = mcsas_amd.SASData(np.logspace(7.5, 9, 20), np.full(20, 7.), np.full(20, .2))
    algo.data = mcsas_amd.DataSets([d0, d1], histogramSet=histogram_set)
    return algo, d0, d1


def test_data_sets_concatenate_their_members():
    algo, d0, d1 = _algo()
    ds = algo.data
    assert len(ds) == 2 and ds.count == 32 and ds.slices == [slice(0, 12), slice(12, 32)]
    np.testing.assert_array_equal(ds.q, np.concatenate([d0.q, d1.q]))
    np.testing.assert_array_equal(ds.f.binnedDataU[ds.slices[1]], d1.f.binnedDataU)
    assert ds.x0.limit == [1e7, 1e9] and ds.histogramMember() is d0 and ds.smearArgs(algo.model) is None
    assert [len(t[0]) for t in ds.triples()] == [12, 20]
    with pytest.raises(ValueError):
        mcsas_amd.DataSets([])
    ds.histogramSet = 2
    with pytest.raises(ValueError, match="histogramSet 2"):
        ds.histogramMember()


def test_analyse_runs_the_joint_fit_and_stores_the_sets(monkeypatch):
    """McSAS.analyse() with a DataSets, the engine call stubbed: its arguments, result[0] with its usual keys over all points, 'sets',
    and histogram() against the one member DataSets.histogramSet names, through the existing single-set path."""
    algo, d0, d1 = _algo(histogram_set=1)
    seen = {}

    def fake_sets(model, sets, st, replay=None, stop=None):
        seen.update(model=model, sets=sets, st=st, stop=stop)
        res = engine.SetsResults(st.n_contrib, model.n_active, st.n_reps, [len(s[0]) for s in sets])
        res.contribs[:] = 5e-8; res.converged[:] = 1
        res.fit[:] = np.arange(32)[:, None]
        res.set_scaling[:] = [[1., 2., 3.], [10., 20., 30.]]; res.set_background[:] = [[.1, .2, .3], [1., 1., 1.]]
        res.set_chisq[:] = [[.9, 1., 1.1], [.8, .7, .6]]
        res.scaling[:] = res.set_scaling[0]; res.background[:] = res.set_background[0]
        return res

    def fake_hist(**item):
        seen["hist"] = item
        raise _Stop()

    class _Stop(Exception):
        pass

    monkeypatch.setattr(engine, "analyse_sets", fake_sets)
    monkeypatch.setattr(engine, "histogram_device", fake_hist)
    monkeypatch.setattr(engine, "analyse", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the single-set call")))
    algo.analyse()
    assert [len(s[0]) for s in seen["sets"]] == [12, 20] and seen["st"].n_contrib == 6 and seen["stop"] is algo._stop
    r = algo.result[0]
    assert r["fitMeasValMean"].shape == (1, 32) and len(r["dataMean"]) == 32 and len(r["fitX0"]) == 32
    np.testing.assert_allclose(r["scaling"], (2., 1.))
    assert [s["slice"] for s in r["sets"]] == [slice(0, 12), slice(12, 32)]
    np.testing.assert_allclose(r["sets"][1]["scaling"], (20., 10.)); np.testing.assert_allclose(r["sets"][0]["background"], (.2, .1))
    np.testing.assert_array_equal(r["sets"][1]["chisq"], [.8, .7, .6])
    with pytest.raises(_Stop):
        algo.histogram()
    np.testing.assert_array_equal(seen["hist"]["q"], d1.q)                  # member 1 alone, and the DataSets is back in place
    np.testing.assert_array_equal(seen["hist"]["intensity"], d1.f.binnedData)
    assert isinstance(algo.data, mcsas_amd.DataSets)
    for kw in (dict(start=np.zeros((6, 1, 3))), dict(trace=4)):
        with pytest.raises(ValueError, match="joint fit"):
            algo.analyse(**kw)
    with pytest.raises(ValueError, match="no plan, batch or series"):
        mcsas_amd.run_series(algo, [algo.data, algo.data], batch=True)
    host = PythonOnlySphere(); host.radius.setActiveRange((2e-9, 3e-7))
    algo.model = host
    monkeypatch.undo()
    _NoLibrary(monkeypatch)
    with pytest.raises(ValueError, match="host code"):
        algo.analyse()

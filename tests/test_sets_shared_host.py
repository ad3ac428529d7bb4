"""Without a device: the shared-scale restatement and the joint histogram's restatement (tests/sets_shared_exact.py), the margin
condition the GPU comparisons of tests/test_sets_shared_gpu.py rest on, every refusal of mcsas_hip_analyse_sets_mode and
mcsas_hip_histogram_sets (each made before a device is touched), and the front end: DataSets' new arguments and where
McSAS.histogram() goes for each of them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import _lib, engine
from oracle import mcsas_oracle as O
from helpers import make_models
import hist_exact as H
import sets_exact as SX
import sets_shared_exact as SH

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcsas_hip.h")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcsas_amd", "csrc")
MCSAS_EINVAL, MCSAS_ENODEV = -1, -2


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", SH.REPLAYED)
def test_no_decision_of_the_gpu_tests_inputs_is_a_near_tie(name):
    """|X_t - X| / X >= 1e-9 at every step of every attempt (DESIGN §4.1e's margin condition): the device's roundings, nine digits
    below that, cannot turn a decision of the restatement."""
    ref = SH.reference(name)
    print(name, "steps", ref.num_iter, "moves", ref.num_moves, "attempts", ref.attempts, "smallest margin %.3g" % ref.min_margin)
    if name in SX.GENERATED:                                 # >= 5 moves; Kholodenko: 1e-5 at chi² >= 1 (test_sets_host.KHOLODENKO_MARGIN)
        from test_sets_host import check_margin
        check_margin(name, SH.case(name), ref)
    assert ref.min_margin >= 1e-9
    assert ref.num_moves > 3 or SH.case(name)["st"].n_contrib == 1
    assert len(set(ref.set_scaling)) == 1                    # one scale


def test_the_inputs_end_where_their_tests_say():
    odd, retry = SH.reference("sh_end_odd"), SH.reference("sh_end_retry")
    assert odd.num_iter == 100 and odd.conval > SH.case("sh_end_odd")["st"].conv_crit
    assert retry.attempts >= 2 and not retry.conval > SH.case("sh_end_retry")["st"].conv_crit


@pytest.mark.parametrize("name", ["s1_n5_bg", "s1_n70_nobg"])
def test_with_one_set_the_shared_restatement_is_the_per_set_one(name):
    c = SX.case(name)
    _, spec = make_models(c["tag"], c["lo"], c["hi"], **c["fixed"])
    a = SX.sets_mc_fit(spec, c["sets"], c["st"], O.ReplayStream(c["replay"][0]))
    b = SH.sets_mc_fit(spec, c["sets"], c["st"], O.ReplayStream(c["replay"][0]))
    assert (a.num_iter, a.num_moves, a.conval) == (b.num_iter, b.num_moves, b.conval)
    for f in ("rset", "fit", "set_chisq", "set_scaling", "set_background"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert SX._fit_sets is SH.SX_FIT_SETS                     # (the per-set solve is back in its place)


def test_the_shared_solve_is_the_least_squares_optimum():
    """(A, b_0, b_1) of the restatement against numpy's least squares on the stacked weighted system; never a better fit than a scale per set."""
    c = SH.case("sh2")
    sets = c["sets"]
    rng = np.random.RandomState(0)
    Cs = [I * (1 + 0.05 * rng.standard_normal(len(I))) / 2e4 for _, I, _ in sets]
    C_all = np.concatenate(Cs)
    slices = [slice(0, 37), slice(37, 137)]
    rs, sc = SH._fit_sets_shared(sets, slices, C_all, True)
    M = np.zeros((137, 3)); y = np.zeros(137)
    for s, sl in enumerate(slices):
        w = 1.0 / sets[s][2]
        M[sl, 0] = w * C_all[sl]; M[sl, 1 + s] = w; y[sl] = w * sets[s][1]
    sol = np.linalg.lstsq(M, y, rcond=None)[0]
    np.testing.assert_allclose([sc[0][0], sc[0][1], sc[1][1]], sol, rtol=1e-8)
    assert sc[0][0] == sc[1][0]
    np.testing.assert_allclose(rs.sum(), ((M @ sol - y) ** 2).sum(), rtol=1e-8)
    per = SH.SX_FIT_SETS(sets, slices, C_all, True)[0]
    assert rs.sum() >= per.sum()                              # fewer unknowns: never a better fit than a scale per set


# ------------------------------------------------------------------------------------------------ the joint histogram's restatement
@pytest.mark.parametrize("set_nq", SH.SET_SHAPES, ids=lambda s: "S%d" % len(s))
def test_the_histogram_restatement_on_host_rows(set_nq):
    """On rows no device made: the fit's bounds hold its float64 emulation in both modes; with one scale for every point and every set
    visible the limits and fractions are hist_exact's own; hiding a set can only raise a limit."""
    c = SH.hist_case(set_nq)
    S = len(set_nq)
    for shared in (False, True):
        set_A = np.zeros((S, c["R"]))
        for r in range(c["R"]):
            bd = SH.fit_sets_bounds(c, r, shared)
            emu = SH.emu_fit_sets(c, r, shared)
            for s in range(S):
                for k, name in enumerate("Ab"):
                    ratio = SH.F.within(emu[s][k], bd[s][k])
                    assert ratio <= 1.0, (shared, r, s, name, ratio)
                set_A[s, r] = emu[s][0]
        if shared:
            assert (set_A == set_A[0]).all()
            np.testing.assert_allclose(set_A[0, 0], SH.A_TRUE, rtol=0.02)
            fr = SH.fractions_bounds_sets(c, set_A[0], set_A, range(S))
            ref = H.fractions_bounds(c, set_A[0])
            for k in H.FRAC8:
                for i in range(c["N"]):
                    for r in range(c["R"]):
                        a, b = fr[k][i, r], ref[k][i, r]
                        assert (a == b) if H.special(a) else (a.v == b.v and a.e == b.e), (k, i, r)
            # the limit over all sets is the lowest of the limits each set gives alone, and not every time the same set's
            alone = [SH.fractions_bounds_sets(c, set_A[0], set_A, [s])["mv"] for s in range(S)]
            winners = set()
            for i in range(c["N"]):
                for r in range(c["R"]):
                    each = [a[i, r].v for a in alone]
                    assert fr["mv"][i, r].v == min(each), (i, r)
                    winners.add(each.index(min(each)))
            print("sets that give a limit:", sorted(winners))


# ------------------------------------------------------------------------------------------------ the C ABI and its refusals
def test_the_abi_is_extended_not_changed():
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(mcsas_hip_[a-z_0-9]+)\s*\(", text))
    for name in ("mcsas_hip_analyse_sets", "mcsas_hip_analyse_sets_mode", "mcsas_hip_histogram_sets"):
        assert name in declared and name in _lib.SYMBOLS
    assert re.search(r"#define\s+MCSAS_ABI_VERSION\s+5\b", text) and _lib.ABI_VERSION == 5
    assert re.search(r"#define\s+MCSAS_SETS_SCALE_PER_SET\s+0\b", text) and re.search(r"#define\s+MCSAS_SETS_SCALE_SHARED\s+1\b", text)
    assert _lib.SETS_SCALE == {"per_set": 0, "shared": 1}
    lib = _lib.load()
    assert hasattr(lib, "mcsas_hip_analyse_sets_mode") and hasattr(lib, "mcsas_hip_histogram_sets")
    assert hasattr(_lib.load(tuning=True), "mcsas_hip_histogram_sets")


def test_the_shared_kernels_are_a_unit_of_their_own():
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "kern_wave_sets_shared_m$(m).o" in make and re.search(r"kern_wave_sets_shared_m%\.o:\s*kern_wave_sets_shared\.hip \$\(SETS_HDRS\)", make)
    unit = open(os.path.join(CSRC, "kern_wave_sets_shared.hip")).read()
    for qpl in (1, 2, 4, 8, 16):
        assert "chain_sets_kernel<MCSAS_M, %d, true>" % qpl in unit
    text = open(os.path.join(CSRC, "chain_sets.h")).read()
    assert "template <int M, int QPL, bool SHARED = false>" in text and "chain_body.inc\"" not in text


def _request(nqs=(40, 50), **st_kw):
    m, _ = make_models("sphere", [2e-9], [3e-7])
    nq = int(sum(nqs))
    q = np.concatenate([np.logspace(7, 9, n) for n in nqs])
    st = engine.Settings(**{**dict(n_contrib=8, n_reps=2, max_iter=10), **st_kw})
    prob = engine.HipProblem(m.setup(), q, np.ones(nq), np.ones(nq), st)
    return prob, engine.SetsResults(8, 1, 2, list(nqs)), np.ascontiguousarray(nqs, dtype=np.int32)


def _analyse(prob, res, set_nq, mode):
    lib = _lib.load()
    rc = lib.mcsas_hip_analyse_sets_mode(C.byref(prob.c), len(set_nq), set_nq.ctypes.data_as(C.POINTER(C.c_int32)), mode, C.byref(res.c),
                                         C.byref(res.sets_c))
    return rc, lib.mcsas_hip_last_error().decode()


def test_analyse_sets_mode_refuses_an_unknown_mode_and_what_analyse_sets_refuses():
    reached = MCSAS_ENODEV if _lib.load().mcsas_hip_device_count() == 0 else 0
    for mode in (0, 1):
        rc, msg = _analyse(*_request(), mode)
        assert rc == reached, msg
    for mode in (-1, 2, 7):
        rc, msg = _analyse(*_request(), mode)
        assert rc == MCSAS_EINVAL and "unknown scale_mode %d" % mode in msg and msg.startswith("analyse_sets:"), msg
    rc, msg = _analyse(*_request(positive_background=True), 1)
    assert rc == MCSAS_EINVAL and "positive_background" in msg, msg
    prob, res, set_nq = _request()
    prob.c.reserved0 = 3
    rc, msg = _analyse(prob, res, set_nq, 1)
    assert rc == MCSAS_EINVAL and "reserved0" in msg, msg
    with pytest.raises(ValueError, match="scale 'both'"):
        engine.analyse_sets(make_models("sphere", [2e-9], [3e-7])[0].setup(), [(np.ones(4),) * 3], engine.Settings(), scale="both")


class _HistRequest(object):
    """a valid mcsas_hip_histogram_sets request on two sets of 40 and 50 points; the caller breaks one thing"""

    def __init__(self, nqs=(40, 50), **kw):
        m, _ = make_models("sphere", [2e-9], [3e-7])
        nq = int(sum(nqs))
        q = np.concatenate([np.logspace(7, 9, n) for n in nqs])
        contribs = np.full((8, 1, 2), 5e-8)
        specs = [dict(param_index=0, yweight="vol", edges=np.geomspace(2e-9, 3e-7, 6), lower=2e-9, upper=3e-7)]
        self.call = engine._HistogramCall(m.setup(), q, np.ones(nq), np.ones(nq), contribs, 0.5, specs, **kw)
        self.set_nq = np.ascontiguousarray(nqs, dtype=np.int32)
        self.A, self.b = np.zeros((len(nqs), 2)), np.zeros((len(nqs), 2))
        self.sr = _lib.SetsResult()
        self.sr.struct_size = C.sizeof(_lib.SetsResult)
        self.sr.n_sets = len(nqs)
        self.sr.scaling, self.sr.background = _lib.as_dp(self.A), _lib.as_dp(self.b)
        self.n_sets, self.mode, self.ref, self.visible = len(nqs), 0, 0, 3

    def run(self):
        lib, k = _lib.load(), self.call
        rc = lib.mcsas_hip_histogram_sets(C.byref(k.prob.c), _lib.as_dp(k.contribs), len(k.specs), k.arr, self.n_sets,
                                          self.set_nq.ctypes.data_as(C.POINTER(C.c_int32)), self.mode, self.ref, self.visible, _lib.as_dp(k.sc),
                                          _lib.as_dp(k.frac), _lib.as_dp(k.out), C.byref(self.sr))
        return rc, lib.mcsas_hip_last_error().decode()


def _spoil(**fields):
    def f(h):
        for k, v in fields.items():
            setattr(h, k, v)
    return f


def _spoil_problem(**fields):
    def f(h):
        for k, v in fields.items():
            setattr(h.call.prob.c, k, v)
    return f


HIST_REFUSALS = {
    "no_sets": (_spoil(n_sets=0), "n_sets 0 (1..4)"),
    "too_many_sets": (_spoil(n_sets=5), "n_sets 5 (1..4)"),
    "sum": (lambda h: h.set_nq.__setitem__(1, 49), "sum of set_nq 89 != nq 90"),
    "short_set": (lambda h: h.set_nq.__setitem__(slice(None), (88, 2)), "set 1 has 2 points"),
    "ref_set": (_spoil(ref=2), "ref_set 2: there are 2 sets"),
    "ref_set_negative": (_spoil(ref=-1), "ref_set -1"),
    "visible_empty": (_spoil(visible=0), "visible_sets is empty"),
    "visible_absent": (_spoil(visible=5), "names a set that is not there"),
    "mode": (_spoil(mode=2), "unknown scale_mode 2"),
    "positive_background": (_spoil_problem(positive_background=1), "positive_background"),
    "smearing": (_spoil_problem(smear_nk=5), "smearing (smear_nk 5)"),
    "plugin": (_spoil_problem(model_id=engine.MODEL_PLUGIN0), "plug-in"),
    "host_model": (_spoil_problem(model_id=engine.MODEL_HOST), "host model"),
    "too_many_contribs": (_spoil_problem(n_contrib=4097), "n_contrib 4097 > 4096"),      # (check_hist_set's)
    "bad_histogram": (lambda h: setattr(h.call.arr[0], "weighting", 9), "weighting 9"),  # (check_hist_set's)
}


def test_a_valid_histogram_request_reaches_the_device():
    rc, msg = _HistRequest().run()
    assert rc == (MCSAS_ENODEV if _lib.load().mcsas_hip_device_count() == 0 else 0), msg


@pytest.mark.parametrize("what", sorted(HIST_REFUSALS))
def test_histogram_sets_refuses_before_a_device_is_touched(what):
    spoil, words = HIST_REFUSALS[what]
    h = _HistRequest()
    spoil(h)
    rc, msg = h.run()
    assert rc == MCSAS_EINVAL and words in msg and msg.startswith("histogram_sets:"), msg


def test_engine_histogram_sets_refusals():
    m, _ = make_models("sphere", [2e-9], [3e-7])
    sets = [(np.logspace(7, 9, 20), np.ones(20), np.ones(20))] * 2
    contribs = np.full((8, 1, 2), 5e-8)
    spec = dict(param_index=0, yweight="vol", edges=np.geomspace(2e-9, 3e-7, 6), lower=2e-9, upper=3e-7)
    with pytest.raises(ValueError, match="scale 'x'"):
        engine.histogram_sets(m.setup(), sets, contribs, 0.5, [spec], scale="x")
    with pytest.raises(ValueError, match="partial intensities are not offered"):
        engine.histogram_sets(m.setup(), sets, contribs, 0.5, [dict(spec, partial="range")])
    with pytest.raises(_lib.McSASHipError, match="names a set that is not there"):
        engine.histogram_sets(m.setup(), sets, contribs, 0.5, [spec], visible=[2])


# ------------------------------------------------------------------------------------------------ the front end
def _algo(**sets_kw):
    m, _ = make_models("sphere", [2e-9], [3e-7])
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, 2e-9, 3e-7, binCount=10, xscale='log', yweight='vol'))
    algo = mcsas_amd.McSAS(seed=3)
    algo.numContribs.setValue(6); algo.numReps.setValue(3)
    algo.model = m
    d0 = mcsas_amd.SASData(np.logspace(7, 8.5, 12), np.full(12, 5.), np.full(12, .1))
    d1 = mcsas_amd.SASData(np.logspace(7.5, 9, 20), np.full(20, 7.), np.full(20, .2))
    algo.data = mcsas_amd.DataSets([d0, d1], **sets_kw)
    return algo, d0, d1


def test_data_sets_take_the_new_arguments():
    ds = _algo()[0].data
    assert (ds.histogramSet, ds.sharedScale, ds.scaleSet, ds.jointHistogram(), ds.visibleSets()) == (0, False, 0, False, [0])
    ds = _algo(histogramSet="all")[0].data
    assert ds.jointHistogram() and ds.visibleSets() == [0, 1] and not ds.sharedScale
    with pytest.raises(ValueError, match="all"):
        ds.histogramMember()
    ds = _algo(histogramSet=1, sharedScale=True, scaleSet=1)[0].data
    assert ds.jointHistogram() and ds.visibleSets() == [1] and ds.scaleSet == 1
    with pytest.raises(ValueError, match="histogramSet 'some'"):
        _algo(histogramSet="some")
    with pytest.raises(ValueError, match="scaleSet 2"):
        _algo(scaleSet=2)
    assert "divide" in mcsas_amd.DataSets.__doc__ and "k_s" in mcsas_amd.DataSets.__doc__


class _Stop(Exception):
    pass


def _fake_sets(seen):
    def fake(model, sets, st, replay=None, stop=None, **kw):
        seen["analyse"] = kw
        res = engine.SetsResults(st.n_contrib, model.n_active, st.n_reps, [len(s[0]) for s in sets])
        res.contribs[:] = 5e-8; res.converged[:] = 1
        return res
    return fake


DISPATCH = [                       # DataSets arguments -> (analyse_sets' extra arguments, the histogram call, its arguments)
    (dict(), {}, "histogram_device", None),
    (dict(histogramSet=1), {}, "histogram_device", None),
    (dict(histogramSet="all"), {}, "histogram_sets", dict(scale="per_set", ref_set=0, visible=[0, 1])),
    (dict(histogramSet="all", scaleSet=1), {}, "histogram_sets", dict(scale="per_set", ref_set=1, visible=[0, 1])),
    (dict(sharedScale=True), dict(scale="shared"), "histogram_sets", dict(scale="shared", ref_set=0, visible=[0])),
    (dict(sharedScale=True, histogramSet=1), dict(scale="shared"), "histogram_sets", dict(scale="shared", ref_set=0, visible=[1])),
    (dict(sharedScale=True, histogramSet="all"), dict(scale="shared"), "histogram_sets", dict(scale="shared", ref_set=0, visible=[0, 1])),
]


@pytest.mark.parametrize("sets_kw, analyse_kw, target, hist_kw", DISPATCH, ids=lambda v: None)
def test_where_histogram_goes(monkeypatch, sets_kw, analyse_kw, target, hist_kw):
    """The table of McSAS.histogram() on a DataSets, the engine calls stubbed: sharedScale False with an index is the single-member
    path with that member's data; everything else is engine.histogram_sets over all members, never the single-member call."""
    algo, d0, d1 = _algo(**sets_kw)
    seen = {}

    def fake_hist(*a, **kw):
        seen["hist"] = (a, kw)
        raise _Stop()

    def never(*a, **kw):
        raise AssertionError("the other histogram call")
    monkeypatch.setattr(engine, "analyse_sets", _fake_sets(seen))
    monkeypatch.setattr(engine, "histogram_device", fake_hist if target == "histogram_device" else never)
    monkeypatch.setattr(engine, "histogram_sets", fake_hist if target == "histogram_sets" else never)
    algo.analyse()
    assert seen["analyse"] == analyse_kw
    assert algo.result[0]["setsScale"] == ("shared" if sets_kw.get("sharedScale") else "per_set")
    assert sorted(algo.result[0]["sets"][0]) == ["background", "chisq", "scaling", "slice"]
    with pytest.raises(_Stop):
        algo.histogram()
    a, kw = seen["hist"]
    if target == "histogram_device":
        member = (d0, d1)[sets_kw.get("histogramSet", 0)]
        np.testing.assert_array_equal(kw["q"], member.q)
    else:
        assert [len(s[0]) for s in a[1]] == [12, 20] and a[2].shape == (6, 1, 3) and len(a[4]) == 1
        assert {k: (list(v) if k == "visible" else v) for k, v in kw.items() if k in hist_kw} == hist_kw
        assert kw["find_background"] is True or kw["find_background"] == algo.findBackground.value()
    assert isinstance(algo.data, mcsas_amd.DataSets)


def test_histogram_sets_results_are_taken_over(monkeypatch):
    """result[0]['scalingFactors'] is the reference pair, 'sets' gains nothing, the histograms are filled"""
    algo, d0, d1 = _algo(sharedScale=True, histogramSet="all")
    seen = {}
    monkeypatch.setattr(engine, "analyse_sets", _fake_sets(seen))

    def fake_hist(model, sets, contribs, comp_exp, specs, **kw):
        N, _, R = contribs.shape
        z = np.ones((N, R))
        nb = len(specs[0]["edges"]) - 1
        hist = dict(bins=np.ones((nb, R)), obs=np.ones((nb, R)), cdf=np.ones((nb, R)), moments=np.ones((5, R)))
        return np.array([[2.] * R, [.5] * R]), {k: (z, z) for k in ("vol", "num", "int", "surf")}, [hist], np.full((2, R), 2.), np.ones((2, R))
    monkeypatch.setattr(engine, "histogram_sets", fake_hist)
    algo.analyse()
    keys = sorted(algo.result[0]["sets"][0])
    algo.histogram()
    np.testing.assert_array_equal(algo.result[0]["scalingFactors"], [[2.] * 3, [.5] * 3])
    assert sorted(algo.result[0]["sets"][0]) == keys
    assert algo.model.radius.histograms()[0].bins.mean.shape == (10,)


@pytest.mark.parametrize("sets_kw", [dict(histogramSet="all"), dict(sharedScale=True)], ids=["all", "shared"])
def test_partial_intensities_and_too_many_contributions_raise(monkeypatch, sets_kw):
    algo, d0, d1 = _algo(**sets_kw)
    seen = {}
    monkeypatch.setattr(engine, "analyse_sets", _fake_sets(seen))
    for name in ("histogram_device", "histogram_sets", "histogram_prep"):
        monkeypatch.setattr(engine, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("a histogram call")))
    algo.analyse()
    with pytest.raises(ValueError, match="at most %d" % engine.HISTOGRAM_MAX_CONTRIBS):
        algo.histogram(np.full((engine.HISTOGRAM_MAX_CONTRIBS + 1, 1, 3), 5e-8))
    m = algo.model
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, 2e-9, 3e-7, binCount=4, xscale='log', yweight='vol', partialIntensity="range"))
    with pytest.raises(ValueError, match="partialIntensity"):
        algo.histogram()

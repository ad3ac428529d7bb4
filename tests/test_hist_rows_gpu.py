"""GPU tests of histogram() on rows the caller fills on the device (mcsas_hip_histogram_device_rows, csrc/host_hist.hip;
csrc/hist_kernels.h: hist_pset_kernel + hist_take_vws_kernel in front of the hist_* kernels of mcsas_hip_histogram).

Fed the rows, volumes, weights and surfaces of a BUILT-IN model (engine.model_calc: model_rows_kernel is hist_rows_body's text under
-ffp-contract=off) every array must be mcsas_hip_histogram's of that model bit for bit, however the repetitions are cut into rounds:
no tolerance.  A model typed in torch is compared with the host path McSAS.histogram() took for it before (batch_model_calc, one
engine.bgfit per repetition, the limits in numpy, _histogram_tail) on the same contributions at rtol 1e-9, atol 1e-300 — what the
project holds a torch model's histogram to against the built-in's (test_device_rows_gpu.py).  Largest relative difference seen
on one MI355X, over every array of every case (the tests print it per array): 0 — both paths see the same torch rows and keep
contribution order in every sum."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch                        # ahead of the library's first load: one HIP runtime in the process (engine._one_hip_runtime)
import mcsas_amd
from mcsas_amd import engine
from mcsas_amd import _lib
from mcsas_amd.scatteringmodels import batch_clip, batch_model_calc
from oracle import mcsas_oracle as O
from helpers import load, make_models
from test_device_rows_gpu import TorchSphere, TorchCoreShell

C_EXP = 0.6666666
RTOL, ATOL = 1e-9, 1e-300


def _equal(a, b):
    return np.array_equal(a, b, equal_nan=True)


def assert_same_triple(got, ref, what=""):
    (sc, fr, hs), (rsc, rfr, rhs) = got, ref
    assert _equal(sc, rsc), (what, "scaling")
    assert list(fr) == ["vol", "num", "int", "surf"] == list(rfr)
    for k in fr:
        assert _equal(fr[k][0], rfr[k][0]) and _equal(fr[k][1], rfr[k][1]), (what, "fractions", k)
    assert len(hs) == len(rhs)
    for h, (a, b) in enumerate(zip(hs, rhs)):
        for k in ("bins", "obs", "cdf", "moments"):
            assert a[k].shape == b[k].shape and _equal(a[k], b[k]), (what, "histogram", h, k)


def builtin_rows(setup, q, calls=None):
    """row_fn of engine.histogram_device_rows that hands over the built-in model's own rows, volumes, weights and surfaces."""
    def fn(pset):
        if calls is not None:
            calls.append(len(pset))
        _, v, w, s, rows = engine.model_calc(setup, q, pset.cpu().numpy(), C_EXP, want_rows=True)
        return rows, v, w, s
    return fn


def torch_rows(model, q):
    qd = []

    def fn(pset):
        if not qd:
            qd.append(torch.as_tensor(np.ascontiguousarray(q, dtype=np.float64), device=pset.device))
        return model.calcIntensityBatch(qd[0], batch_clip(model, pset), C_EXP)
    return fn


def _spec(pi, lo, hi, nb, xscale, yweight):
    edges = np.linspace(lo, hi, nb + 1) if xscale == "lin" else np.geomspace(lo, hi, nb + 1)
    return dict(param_index=pi, yweight=yweight, edges=edges, lower=lo, upper=hi)


@pytest.fixture(scope="module")
def sphere():
    """The built-in sphere's chains at 100 q x 60 contributions x 5 repetitions, four histograms, and mcsas_hip_histogram of them."""
    g = load("g4_sphere_q100_fixed.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    lo, hi = float(g["spec_lo"][0]), float(g["spec_hi"][0])
    m, _ = make_models("sphere", [lo], [hi], sld=float(g["spec_sld"]))
    setup = m.setup()
    st = engine.Settings(n_contrib=60, n_reps=5, max_iter=300, conv_crit=1e-9, max_retries=0, seed=21, comp_exp=C_EXP)
    contribs = engine.analyse(setup, q, I, sig, st).contribs
    span = hi - lo
    specs = [_spec(0, lo, hi, 20, "log", "vol"), _spec(0, lo, hi, 130, "lin", "num"),           # (130 bins: three passes of 64 lanes)
             _spec(0, lo + 0.2 * span, lo + 0.7 * span, 12, "lin", "surf"), _spec(0, lo, hi, 50, "log", "int")]
    ref = engine.histogram_device(setup, q, I, sig, contribs, C_EXP, specs)
    return dict(q=q, I=I, sig=sig, lo=lo, hi=hi, sld=float(g["spec_sld"]), setup=setup, contribs=contribs, specs=specs, ref=ref)


def test_built_in_rows_give_the_built_in_histogram_whatever_the_rounds(sphere):
    f = sphere
    assert engine.histogram_rows_shape(f["setup"], f["q"], (60, 5)) == (60, 300, 100)
    sc, fr, hs = f["ref"]
    assert np.isfinite(sc).all() and (sc[0] > 0).all()
    assert (hs[3]["bins"] == 0).any() and (hs[3]["bins"] != 0).any()                  # some of the 50 bins stay empty
    assert (hs[2]["moments"][0] < 1).all() and (hs[2]["bins"] != 0).any()             # the narrowed range leaves contributions out
    assert [h["bins"].shape for h in hs] == [(20, 5), (130, 5), (12, 5), (50, 5)]
    for capacity, rounds in ((None, [300]), (60, [60] * 5), (120, [120, 120, 60]), (299, [240, 60])):
        calls = []
        got = engine.histogram_device_rows(f["setup"], f["q"], f["I"], f["sig"], f["contribs"], f["specs"],
                                           builtin_rows(f["setup"], f["q"], calls), capacity=capacity)
        assert calls == rounds, (capacity, calls)
        assert_same_triple(got, f["ref"], capacity)


def _builtin_case(tag, lo, hi, nq, N, R, seed, fixed=None, **flags):
    rs = np.random.RandomState(seed)
    q = np.geomspace(1e8, 3e9, nq)
    m, spec = make_models(tag, lo, hi, **(fixed or {}))
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    contribs = rs.uniform(lo[None, :, None], hi[None, :, None], (N, len(lo), R))
    truth = rs.uniform(lo, hi, (20, len(lo)))
    It = O.model_calc(spec, q, truth, C_EXP)[0]
    It *= 1e3 / It.max()
    I = It * (1 + 0.02 * rs.standard_normal(nq)) + 0.5
    sig = 0.02 * It + 0.01
    last = len(lo) - 1
    specs = [_spec(0, lo[0], hi[0], 20, "log", "vol"), _spec(last, lo[last], hi[last], 9, "lin", "surf"),
             _spec(last, lo[last], hi[last], 70, "lin", "num"), _spec(0, lo[0], hi[0], 5, "log", "int")]
    return m, q, I, sig, contribs, specs, flags


@pytest.mark.parametrize("case", ["two_params_zero_surface", "two_params_1300_q", "no_background", "positive_background", "one_contribution",
                                  "64_q"])
def test_further_shapes_and_flags_with_built_in_rows(case):
    """Two active parameters (a core-shell sphere has no surface: every total of the surface weighting is zero and the ts == 0
    branch runs), 1300 q-points (six column blocks of 256), the fit's two flags, a single contribution, 64 q-points exactly."""
    cs = dict(tag="sphcs", lo=[2e-9, 5e-10], hi=[1e-7, 2e-8], N=40, R=3)
    sp = dict(tag="sphere", lo=[2e-9], hi=[1e-7], N=60, R=5)
    m, q, I, sig, contribs, specs, flags = _builtin_case(**{
        "two_params_zero_surface": dict(cs, nq=100, seed=1), "two_params_1300_q": dict(cs, nq=1300, seed=2),
        "no_background": dict(sp, nq=100, seed=3, find_background=False), "positive_background": dict(sp, nq=100, seed=4, positive_background=True),
        "one_contribution": dict(sp, nq=100, seed=5, N=1), "64_q": dict(sp, nq=64, seed=6)}[case])
    setup = m.setup()
    ref = engine.histogram_device(setup, q, I, sig, contribs, C_EXP, specs, **flags)
    N, R = contribs.shape[0], contribs.shape[2]
    calls = []
    got = engine.histogram_device_rows(setup, q, I, sig, contribs, specs, builtin_rows(setup, q, calls), capacity=max(N, 2 * N), **flags)
    assert calls == ([2 * N] * (R // 2) + [N] * (R % 2) if N > 0 else []), calls
    assert_same_triple(got, ref, case)
    sc, fr, hs = ref
    assert np.isfinite(sc).all()
    if case.startswith("two_params"):
        assert (fr["surf"][0] == 0).all() and (fr["vol"][0] != 0).all()               # ts == 0: nothing is divided
    if case == "no_background":
        assert (sc[1] == 0).all()
    if case == "positive_background":
        assert (sc[1] >= 0).all()


def _collect(algo):
    hists = [h for p in algo.model.activeParams() for h in p.histograms()]
    out = dict(scalingFactors=np.array(algo.result[0]["scalingFactors"]))
    for k, (frac, lim) in algo.fractions.items():
        out["frac_" + k], out["lim_" + k] = np.array(frac), np.array(lim)
    for i, h in enumerate(hists):
        out["bins%d" % i], out["cdf%d" % i], out["obs%d" % i] = h.bins.full.copy(), h.cdf.full.copy(), np.array(h.observability)
        out["moments%d" % i] = np.array(h.moments.fields)
    return out


def host_path(algo, contribs):
    """McSAS.histogram() of a calcIntensityBatch model as it was before the device path: the rows downloaded, the fit by one
    engine.bgfit call per repetition, the visibility limits in numpy, then _histogram_tail."""
    model, data = algo.model, algo.data
    N, P, R = contribs.shape
    sig = np.array(data.f.binnedDataU, dtype=float)
    sets = np.ascontiguousarray(np.moveaxis(contribs, 2, 0)).reshape(R * N, -1)
    _, v, w, s, rows = batch_model_calc(model, data, sets, algo.compensationExponent(), want_rows=True)
    v, w, s = (np.ascontiguousarray(a.reshape(R, N).T) for a in (v, w, s))
    rows = rows.reshape(R, N, -1)
    sc, mv = np.zeros((2, R)), np.zeros((N, R))
    for r in range(R):
        cum = np.cumsum(rows[r], axis=0)[-1]
        sc[:, r] = engine.bgfit(data.f.binnedData, sig, cum, algo.findBackground.value(), algo.positiveBackground.value(),
                                num_params=model.activeParamCount())[0]
        vf = w[:, r] * sc[0, r] / v[:, r]
        for ci in range(N):
            part = sc[0, r] * rows[r, ci]
            nz = part != 0.
            mv[ci, r] = (sig[nz] * vf[ci] / part[nz]).min()
    algo._histogram_tail(contribs, sc, v, w, s, mv)
    return _collect(algo)


def assert_close_to_host_path(new, old, what):
    worst = 0.
    assert set(new) == set(old)
    for k in sorted(new):
        a, b = new[k], old[k]
        assert a.shape == b.shape, (what, k)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(a - b) / np.abs(b)
        rel = rel[np.isfinite(rel)]
        if rel.size:
            worst = max(worst, float(rel.max()))
            print("%s %-16s largest relative difference %.3e" % (what, k, rel.max()))
    for k in sorted(new):
        np.testing.assert_allclose(new[k], old[k], rtol=RTOL, atol=ATOL, err_msg="%s %s" % (what, k))
    return worst


def test_torch_sphere_through_calc_against_the_host_path():
    """TorchSphere through McSAS.calc(): analyse() on device rows, histogram() on device rows; the stored histograms, fractions and
    scaling factors against the host path on the same contributions."""
    g = load("g4_sphere_q100_fixed.npz")
    lo, hi = float(g["spec_lo"][0]), float(g["spec_hi"][0])
    m = TorchSphere(); m.radius.setActiveRange((lo, hi)); m.sld.setValue(float(g["spec_sld"]))
    span = hi - lo
    for args in ((lo, hi, 20, "log", "vol"), (lo, hi, 130, "lin", "num"), (lo + 0.2 * span, lo + 0.7 * span, 12, "lin", "surf"),
                 (lo, hi, 50, "log", "int")):
        m.radius.histograms().append(mcsas_amd.Histogram(m.radius, args[0], args[1], binCount=args[2], xscale=args[3], yweight=args[4],
                                                         autoFollow=False))
    algo = mcsas_amd.McSAS(seed=3)
    algo.numContribs.setValue(60); algo.numReps.setValue(5); algo.maxIterations.setValue(300)
    algo.convergenceCriterion.setValue(1e-9); algo.showIncomplete.setValue(True)
    algo.maxRetries = mcsas_amd.mcsas._Setting("maxRetries", 0)
    algo.model = m
    algo.data = mcsas_amd.SASData(g["data_q"], g["data_I"], g["data_sigma"], f_limit=g["data_f_limit"])
    seen = []
    real = engine.histogram_device_rows

    def spy(**kw):
        seen.append(kw["contribs"].shape)
        return real(**kw)
    engine.histogram_device_rows = spy
    try:
        algo.calc()
    finally:
        engine.histogram_device_rows = real
    assert seen == [(60, 1, 5)] and len(algo.result) == 1
    new = _collect(algo)
    assert new["bins0"].shape == (20, 5) and new["bins1"].shape == (130, 5) and (new["bins1"] != 0).any()
    old = host_path(algo, algo.result[0]["contribs"])
    assert_close_to_host_path(new, old, "torch sphere 100 q x 60 x 5")


@pytest.mark.parametrize("nq, flags", [(100, {}), (1300, {}), (100, dict(findBackground=False)), (100, dict(positiveBackground=True))])
def test_torch_core_shell_against_the_host_path(nq, flags):
    """Two active parameters and no surface, 40 contributions x 3 repetitions, through McSAS.histogram(contribs)."""
    rs = np.random.RandomState(7)
    q = np.geomspace(1e8, 3e9, nq)
    lo, hi = [2e-9, 5e-10], [1e-7, 2e-8]
    m = TorchCoreShell()
    m.radius.setActiveRange((lo[0], hi[0])); m.t.setActiveRange((lo[1], hi[1]))
    _, spec = make_models("sphcs", lo, hi)
    It = O.model_calc(spec, q, rs.uniform(lo, hi, (20, 2)), C_EXP)[0]
    It *= 1e3 / It.max()
    I = It * (1 + 0.02 * rs.standard_normal(nq)) + 0.5
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo[0], hi[0], binCount=20, xscale="log", yweight="vol"))
    m.t.histograms().append(mcsas_amd.Histogram(m.t, lo[1], hi[1], binCount=9, xscale="lin", yweight="surf"))
    m.t.histograms().append(mcsas_amd.Histogram(m.t, lo[1], hi[1], binCount=70, xscale="lin", yweight="num"))
    algo = mcsas_amd.McSAS(seed=3)
    for name, value in flags.items():
        getattr(algo, name).setValue(value)
    algo.compensationExponent.setValue(C_EXP)
    algo.model = m
    algo.data = mcsas_amd.SASData(q, I, 0.02 * It + 0.01)
    contribs = rs.uniform(np.array(lo)[None, :, None], np.array(hi)[None, :, None], (40, 2, 3))
    algo.result = [dict(contribs=contribs)]
    algo.histogram()
    new = _collect(algo)
    assert (new["frac_surf"] == 0).all() and (new["frac_vol"] != 0).all() and np.isfinite(new["scalingFactors"]).all()
    if flags.get("findBackground") is False:
        assert (new["scalingFactors"][1] == 0).all()
    old = host_path(algo, contribs)
    assert_close_to_host_path(new, old, "torch core-shell %d q x 40 x 3 %r" % (nq, flags))


def test_failures_leave_the_next_call_intact(sphere):
    """An exception in row_fn comes back as itself, a callback that reports failure gives MCSAS_ECALLBACK, a host pointer handed
    over as d_rows gives MCSAS_EINVAL — and the call after each of them is the good result bit for bit: the staging blocks went
    back to the cache only after what was queued on them had run."""
    f = sphere
    args = (f["setup"], f["q"], f["I"], f["sig"], f["contribs"], f["specs"])
    good = builtin_rows(f["setup"], f["q"])
    calls = []

    def bad(pset):
        calls.append(len(pset))
        if len(calls) == 2:
            raise ZeroDivisionError("model failed")
        return good(pset)
    with pytest.raises(ZeroDivisionError, match="model failed"):
        engine.histogram_device_rows(*args, bad, capacity=120)
    assert calls == [120, 120]
    assert_same_triple(engine.histogram_device_rows(*args, good, capacity=120), f["ref"], "after an exception")

    lib = _lib.load()
    call = engine._HistogramCall(f["setup"], f["q"], f["I"], f["sig"], f["contribs"], 0.0, f["specs"])
    call.prob.c.model_id = engine.MODEL_HOST
    dev = torch.device("cuda", torch.cuda.current_device())
    pset = torch.zeros((300, 1), dtype=torch.float64, device=dev)
    rows = torch.zeros((300, 100), dtype=torch.float64, device=dev)
    vws = torch.ones((3, 300), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    entered = []

    def raw(d_rows, cb):
        return lib.mcsas_hip_histogram_device_rows(C.byref(call.prob.c), _lib.as_dp(call.contribs), C.c_void_p(pset.data_ptr()), d_rows,
                                                   C.c_void_p(vws.data_ptr()), 300, _lib.DeviceRowsCallback(cb), None, len(call.specs),
                                                   call.arr, _lib.as_dp(call.sc), _lib.as_dp(call.frac), _lib.as_dp(call.out))

    def failing(user, n):
        entered.append(n)
        return 1
    assert raw(C.c_void_p(rows.data_ptr()), failing) == -6                             # MCSAS_ECALLBACK
    assert entered == [300] and "rows callback returned 1" in lib.mcsas_hip_last_error().decode()
    # the parameter sets were laid out for the callback: row rl * 60 + c is contribution c of repetition rl
    np.testing.assert_array_equal(pset.cpu().numpy().reshape(5, 60), f["contribs"][:, 0, :].T)
    host_rows = np.zeros((300, 100))
    assert raw(C.c_void_p(host_rows.ctypes.data), failing) == -1                       # MCSAS_EINVAL
    assert "d_rows is not device memory" in lib.mcsas_hip_last_error().decode() and entered == [300]
    assert_same_triple(engine.histogram_device_rows(*args, good), f["ref"], "after the refusals")


# engine.histogram_device of the built-in sphere on the arrays of an .npz, every array of the result into another: run by a fresh
# process for the test below, and by the test itself
_PLAIN_CALL = """
import sys
import numpy as np
import mcsas_amd
from mcsas_amd import engine

def plain_call(g):
    lo, hi = float(g["lo"]), float(g["hi"])
    m = mcsas_amd.Sphere(); m.radius.setActiveRange((lo, hi))
    spec = dict(param_index=0, yweight="vol", edges=g["edges"], lower=lo, upper=hi)
    sc, fr, hs = engine.histogram_device(m.setup(), g["q"], g["I"], g["sig"], g["contribs"], float(g["c_exp"]), [spec])
    out = dict(scaling=sc, **{k: hs[0][k] for k in ("bins", "obs", "cdf", "moments")})
    for k, (frac, limit) in fr.items():
        out["frac_" + k], out["limit_" + k] = frac, limit
    return out

if __name__ == "__main__":
    np.savez(sys.argv[2], **plain_call(np.load(sys.argv[1])))
"""


def test_a_callback_failing_in_a_later_round_leaves_the_plain_call_intact(tmp_path):
    """8 contributions x 3 q x 3 repetitions with room for one repetition's rows: three rounds, and the callback reports failure in
    the second, with the first round's kernels and the second's parameter sets behind it.  The call is MCSAS_ECALLBACK, and
    mcsas_hip_histogram of the same sizes — the same staging blocks from the cache — then gives the bits a process that never saw
    the failure gives: the set's guard waited before the blocks went back."""
    N, nq, R = 8, 3, 3
    rs = np.random.RandomState(83)
    q = np.geomspace(1e8, 3e9, nq)
    lo, hi = np.pi / 3e9, np.pi / 1e8
    inputs = dict(q=q, I=1.0 + rs.rand(nq), sig=0.1 + rs.rand(nq), contribs=rs.uniform(lo, hi, (N, 1, R)), lo=lo, hi=hi,
                  edges=np.geomspace(lo, hi, 5), c_exp=C_EXP)
    np.savez(tmp_path / "in.npz", **inputs)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _PLAIN_CALL, str(tmp_path / "in.npz"), str(tmp_path / "fresh.npz")], cwd=root, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    fresh = np.load(tmp_path / "fresh.npz")
    assert np.isfinite(fresh["scaling"]).all() and (fresh["bins"] != 0).any()

    lib = _lib.load()
    m = mcsas_amd.Sphere(); m.radius.setActiveRange((lo, hi))
    spec = dict(param_index=0, yweight="vol", edges=inputs["edges"], lower=lo, upper=hi)
    call = engine._HistogramCall(m.setup(), q, inputs["I"], inputs["sig"], inputs["contribs"], 0.0, [spec])
    call.prob.c.model_id = engine.MODEL_HOST
    dev = torch.device("cuda", torch.cuda.current_device())
    pset = torch.zeros((N, 1), dtype=torch.float64, device=dev)
    rows = torch.ones((N, nq), dtype=torch.float64, device=dev)
    vws = torch.ones((3, N), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    entered = []

    def failing_second(user, n):
        entered.append(n)
        return 7 if len(entered) == 2 else 0
    rc = lib.mcsas_hip_histogram_device_rows(C.byref(call.prob.c), _lib.as_dp(call.contribs), C.c_void_p(pset.data_ptr()), C.c_void_p(rows.data_ptr()),
                                             C.c_void_p(vws.data_ptr()), N, _lib.DeviceRowsCallback(failing_second), None, len(call.specs),
                                             call.arr, _lib.as_dp(call.sc), _lib.as_dp(call.frac), _lib.as_dp(call.out))
    assert rc == -6 and entered == [N, N]                                              # MCSAS_ECALLBACK, in round 2 of 3
    assert "rows callback returned 7" in lib.mcsas_hip_last_error().decode()
    np.testing.assert_array_equal(pset.cpu().numpy()[:, 0], inputs["contribs"][:, 0, 1])    # (round 2's sets were laid out)

    scope = {"__name__": "plain_call"}
    exec(_PLAIN_CALL, scope)
    here = scope["plain_call"](inputs)
    assert sorted(here) == sorted(fresh.files)
    for k in here:
        assert _equal(here[k], fresh[k]), k

"""The partial intensities of histogram ranges and bins on the device (csrc/hist_partial_kernel.h; mcsas_hip_histogram_partial,
mcsas_hip_histogram_partial_device_rows) — tests/hist_partial_exact.py holds the cases, the exact values and the bounds.

  1. every case, its rows fed through engine.histogram_device_rows: intensity and bin_intensity equal the numpy form
     (parameter.partial_intensities) bit for bit and lie inside the exact bounds; scaling, fractions, bins, obs, cdf and moments
     are those of the call without `partial`, bit for bit;
  2. rounds of one repetition and a second call give the same bits;
  3. built-in models (sphere; cylinders with two active parameters; a slit-smeared sphere): a range, and a bin, holding every
     contribution give scaling[0][r] * model_calc(...) bit for bit; the bins of edges that span every value sum to the range curve;
  4. a built-in model written again as a plug-in gives its twin's bits;
  5. McSAS.histogram() on the quick-start data, for a torch model, for a model that exists only in Python, for more
     contributions or bins than the device call takes, and run_series(batch=True).

No assertion has a tolerance that is not derived: bits, the bounds of hist_partial_exact, the sum bound of test 3 (its docstring),
and for the torch model the agreement the project holds two evaluations of a torch model to (test_hist_rows_gpu.RTOL)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

try:                                # ahead of the library's first load: one HIP runtime in the process (engine._one_hip_runtime)
    import torch
    NO_TORCH = None if torch.cuda.is_available() else "torch cannot reach the device"
except Exception as e:              # noqa: BLE001
    NO_TORCH = "torch cannot reach the device: %s" % e

import hist_exact as H
import hist_partial_exact as X
import mcsas_amd
from exact import U, gamma
from mcsas_amd import engine, series
from mcsas_amd.parameter import partial_intensities
from mcsas_amd.scatteringmodels import batch_model_calc, host_model_calc
from helpers import load, make_models, plugin_twin, PythonOnlySphere, _quickstart_algo

CASES = {c["name"]: c for c in X.cases()}
_SETUP = {}


def _setup(c):
    tag = "sphcs" if c["P"] == 2 else "sphere"              # (explicit rows: the model only names the sizes)
    if tag not in _SETUP:
        _SETUP[tag] = make_models(tag, H.PAR_LO[:c["P"]], H.PAR_HI[:c["P"]])[0].setup()
    return _SETUP[tag]


def handed_rows(c):
    """row_fn that hands the case's arrays over a round at a time (hist_exact's order); the sets it is shown are the case's"""
    N, P, nrep, nq = c["N"], c["P"], c["R"], c["nq"]
    rows = c["rows"].reshape(nrep * N, nq)
    v, w, s = (np.ascontiguousarray(c[k].T).reshape(-1) for k in "vws")
    pset_all = np.ascontiguousarray(c["contribs"].transpose(2, 0, 1)).reshape(nrep * N, P)
    pos = [0]

    def fn(pset):
        a, n = pos[0], len(pset)
        pos[0] += n
        assert np.array_equal(pset.cpu().numpy(), pset_all[a:a + n], equal_nan=True)
        return tuple(torch.from_numpy(np.ascontiguousarray(x[a:a + n])) for x in (rows, v, w, s))
    return fn


def fed(name, partial="case", capacity=None):
    if NO_TORCH:
        pytest.skip(NO_TORCH)
    c = X.host_case(CASES[name])
    return engine.histogram_device_rows(_setup(c), c["q"], c["I"], c["sigma"], c["contribs"], c["specs"], handed_rows(c),
                                        find_background=c["find_bg"], capacity=capacity, partial=list(c["want"]) if partial == "case" else partial)


def curves(c, hs):
    """{h: (intensity, bin_intensity or None)} of the histograms that asked; the others carry neither key"""
    out = {}
    for h, (res, w) in enumerate(zip(hs, c["want"])):
        assert ("intensity" in res) == (w >= 1) and ("bin_intensity" in res) == (w == 2), (c["name"], h, sorted(res))
        if w:
            out[h] = (res["intensity"], res.get("bin_intensity"))
    return out


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def same_triple(a, b, what):
    (sc, fr, hs), (rsc, rfr, rhs) = a, b
    assert X.same_bits(sc, rsc), (what, "scaling")
    for k in H.WEIGHTS:
        assert _eq(fr[k][0], rfr[k][0]) and _eq(fr[k][1], rfr[k][1]), (what, "fractions", k)
    assert len(hs) == len(rhs)
    for h, (x, y) in enumerate(zip(hs, rhs)):
        for k in ("bins", "obs", "cdf", "moments"):
            assert _eq(x[k], y[k]), (what, "histogram", h, k)


def same_curves(a, b, what):
    assert sorted(a) == sorted(b)
    for h in a:
        for x, y in zip(a[h], b[h]):
            assert (x is None) == (y is None) and (x is None or X.same_bits(x, y)), (what, h)


# ------------------------------------------------------------------------------------------------- 1. rows of the test's choosing
@pytest.mark.parametrize("name", sorted(CASES))
def test_fed_rows_give_the_numpy_forms_bits_inside_the_exact_bounds(name):
    c = X.host_case(CASES[name])
    got = fed(name)
    A = got[0][0]
    assert np.isfinite(A).all() and (A > 0).all() and (A < 0.5).all(), A
    mine = curves(c, got[2])
    for h, sp, w in X.wanted(c):
        assert mine[h][0].shape == (c["nq"], c["R"]) and (w != 2 or mine[h][1].shape == (X.n_bins(sp), c["nq"], c["R"]))
    same_curves(mine, X.numpy_partial(c, A), name)
    ref, _ = X.exact_partial(c, A)
    bad, worst = [], {}
    X.look_partial(bad, worst, c, mine, ref)
    for k, v in sorted(H.summarise(worst).items()):
        print("%s  %-8s  largest error / bound %.3g" % (name, k, v))
    assert not bad, "\n".join(bad[:40])
    same_triple(got, fed(name, partial=None), name)             # everything else: the call without a request


@pytest.mark.parametrize("name", ["placed", "n64", "n130"])
def test_rounds_and_a_second_call_give_the_same_bits(name):
    c = X.host_case(CASES[name])
    first = fed(name)
    for what, again in (("a repetition a round", fed(name, capacity=c["N"])), ("second call", fed(name))):
        same_triple(again, first, (name, what))
        same_curves(curves(c, again[2]), curves(c, first[2]), (name, what))


# ------------------------------------------------------------------------------------------------- 3. anchors on built-in models
def _anchor_items():
    from test_hist_batch_gpu import model_groups_batch
    items = model_groups_batch()[0]
    return {"sphere": items[0], "cylinders": items[1], "smeared_sphere": items[3]}


@pytest.mark.parametrize("name", ["sphere", "cylinders", "smeared_sphere"])
def test_everything_selected_is_the_scaled_model_curve_and_bins_sum_to_the_range(name):
    """A range holding every contribution, and one bin holding every contribution, sum the rows model_calc sums, in the same
    order: scaling[0][r] * cumInt bit for bit.  Bins whose edges span every value partition the contributions: with S_b the
    exact sum of bin b's rows and S = sum_b S_b, every bin curve is within gamma(m_b) <= gamma(N) of A S_b and the range curve
    within gamma(N) of A S (hist_partial_exact: m roundings, non-negative rows), so
        |sum_b bin_b - range| <= gamma(N) sum_b A S_b + gamma(N) A S,  A S_b <= bin_b / (1 - gamma(N)),  A S <= range / (1 - gamma(N));
    the sum over the bins is math.fsum's, exact and rounded once: + u |sum|."""
    it = dict(_anchor_items()[name])
    contribs, N = it["contribs"], it["contribs"].shape[0]
    P = contribs.shape[1]
    specs = []
    for p in range(P):
        lo, hi = 0.5 * contribs[:, p, :].min(), 2.0 * contribs[:, p, :].max()
        specs += [dict(param_index=p, yweight="vol", edges=np.array([lo, hi]), lower=lo, upper=hi),
                  dict(param_index=p, yweight="num", edges=np.geomspace(lo, hi, 14), lower=lo, upper=hi)]
    it["specs"] = specs
    sc, fr, hs = engine.histogram_device(partial=[2] * len(specs), **it)
    same_triple((sc, fr, hs), engine.histogram_device(**it), name)
    g = gamma(N)
    for r in range(contribs.shape[2]):
        cum = engine.model_calc(it["model"], it["q"], contribs[:, :, r], it["comp_exp"], smear=it["smear"])[0]
        assert (cum > 0).all()
        whole = sc[0][r] * cum
        for h in hs:
            assert X.same_bits(h["intensity"][:, r], whole), (name, r)
        for h in hs[0::2]:
            assert X.same_bits(h["bin_intensity"][0, :, r], whole), (name, r)
        for h in hs[1::2]:
            for k in range(len(cum)):
                total = math.fsum(h["bin_intensity"][:, k, r])
                bound = g * total / (1 - g) + g * whole[k] / (1 - g) + U * total
                assert abs(total - whole[k]) <= bound, (name, r, k, total, whole[k], bound)


# ------------------------------------------------------------------------------------------------- 4. a plug-in twin
def test_a_plug_in_twin_gives_the_built_in_models_bits():
    """the core-shell sphere typed again as HIP text, operation for operation (helpers.PLUGIN_SOURCES; test_parity_gpu holds its
    rows to the built-in's bits): its rows come through the same hist_rows kernel family, the curves are the twin's"""
    from test_hist_batch_gpu import _item
    lo, hi = H.PAR_LO, H.PAR_HI
    m, _ = make_models("sphcs", lo, hi)
    it = _item(m.setup(), lo, hi, 65, 40, 3, [(0, 12, "log", "vol", 1.0), (1, 7, "lin", "num", 0.5), (1, 3, "log", "int", 1.0)], 31)
    twin = plugin_twin(make_models("sphcs", lo, hi)[0], "sphcs").setup()
    assert twin.model_id >= engine.MODEL_PLUGIN0
    want = [2, 1, 2]
    a = engine.histogram_device(partial=want, **it)
    b = engine.histogram_device(partial=want, **{**it, "model": twin})
    same_triple(b, a, "twin")
    assert (a[2][0]["bin_intensity"] > 0).any()
    for x, y in zip(a[2], b[2]):
        assert sorted(x) == sorted(y)
        for k in ("intensity", "bin_intensity"):
            assert (k not in x) or X.same_bits(x[k], y[k]), k


# ------------------------------------------------------------------------------------------------- 5. the front end
def _collect(algo):
    hists = [h for p in algo.model.activeParams() for h in p.histograms()]
    out = dict(scalingFactors=np.array(algo.result[0]["scalingFactors"]))
    for k, (frac, lim) in algo.fractions.items():
        out["frac_" + k], out["lim_" + k] = np.array(frac), np.array(lim)
    for i, h in enumerate(hists):
        out["bins%d" % i], out["cdf%d" % i], out["obs%d" % i] = h.bins.full.copy(), h.cdf.full.copy(), np.array(h.observability)
        out["moments%d" % i] = np.array(h.moments.fields)
    return out


def _numpy_curves(h, rows_of, contribs, scale, pi=0):
    """the numpy form of histogram h over every repetition, rows_of(r) -> rows [N][nq]"""
    out = [partial_intensities(rows_of(r), contribs[:, pi, r], scale[r], min(h.xrange), max(h.xrange), h.xLowerEdge, h.partialIntensity == "bins")
           for r in range(contribs.shape[2])]
    rng = np.stack([o[0] for o in out], axis=1)
    return rng, (np.stack([o[1] for o in out], axis=2) if h.partialIntensity == "bins" else None)


def _check_against(h, rng, bins, same):
    assert h.intensity.full.shape == rng.shape and same(h.intensity.full, rng)
    R = rng.shape[1]
    assert same(h.moments.intensity[0], rng.mean(axis=1)) and same(h.moments.intensity[1], rng.std(axis=1, ddof=1 if R > 1 else 0))
    if bins is None:
        assert h.binIntensity is None
    else:
        assert h.binIntensity.full.shape == bins.shape and same(h.binIntensity.full, bins)
        assert h.binIntensity.mean.shape == bins.shape[:2] and h.binIntensity.std.shape == bins.shape[:2]


def test_mcsas_calc_on_the_quick_start_data_fills_both_kinds():
    g = load("g13_quickstart.npz")
    reps = 3
    algo, m = _quickstart_algo(g, reps, 5)
    lo, hi = float(g["lo"]), float(g["hi"])
    hs = m.radius.histograms()
    hs.append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=20, xscale="log", yweight="vol", partialIntensity="bins"))
    hs.append(mcsas_amd.Histogram(m.radius, 2 * lo, 0.25 * hi, binCount=8, xscale="lin", yweight="num", autoFollow=False, partialIntensity="range"))
    hs.append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=257, xscale="log", yweight="vol", partialIntensity="bins"))   # (numpy: > 256 bins)
    algo.calc()
    assert len(algo.result) == 1
    contribs, scale = algo.result[0]["contribs"], algo.result[0]["scalingFactors"][0]
    nq = algo.data.count
    assert hs[0].intensity is None and hs[0].binIntensity is None and hs[0].moments.intensity is None
    assert hs[1].intensity.full.shape == (nq, reps) and hs[1].binIntensity.full.shape == (20, nq, reps)
    assert hs[2].intensity.full.shape == (nq, reps) and hs[2].binIntensity is None and hs[3].binIntensity.full.shape == (257, nq, reps)
    assert hs[1].moments.intensity[0].shape == (nq,) and hs[1].moments.intensity[1].shape == (nq,)
    setup, c = m.setup(), algo.compensationExponent()
    rows = [engine.model_calc(setup, algo.data.q, contribs[:, :, r], c, want_rows=True)[4] for r in range(reps)]
    for h in hs[1:]:
        _check_against(h, *_numpy_curves(h, lambda r: rows[r], contribs, scale), same=X.same_bits)
    assert (hs[2].intensity.full <= hs[1].intensity.full).all() and (hs[2].intensity.full < hs[1].intensity.full).any()   # the narrower range
    with_request = _collect(algo)
    kept = [(h.intensity.full.copy(), h.partialIntensity) for h in hs[1:]]
    for h in hs:
        h.partialIntensity = None
    algo.histogram()
    without = _collect(algo)
    assert set(with_request) == set(without) and all(_eq(with_request[k], without[k]) for k in without)
    assert all(h.intensity is None and h.binIntensity is None and h.moments.intensity is None for h in hs)
    # one repetition: ddof 0 (utils/parameter.py:150-152), the standard deviation is 0, not NaN
    hs[2].partialIntensity = "range"
    algo.histogram(np.ascontiguousarray(contribs[:, :, :1]))
    assert X.same_bits(hs[2].intensity.full[:, 0], kept[1][0][:, 0]) and not hs[2].moments.intensity[1].any()


def _algo_with_result(m, q, I, sig, contribs):
    algo = mcsas_amd.McSAS(seed=1)
    algo.model = m
    algo.data = mcsas_amd.SASData(q, I, sig)
    algo.result = [dict(contribs=contribs)]
    return algo


def test_a_torch_model_goes_through_the_device_rows_route():
    if NO_TORCH:
        pytest.skip(NO_TORCH)
    from test_device_rows_gpu import TorchSphere
    from test_hist_rows_gpu import RTOL, ATOL
    g = load("g4_sphere_q100_fixed.npz")
    lo, hi = float(g["spec_lo"][0]), float(g["spec_hi"][0])
    m = TorchSphere(); m.radius.setActiveRange((lo, hi)); m.sld.setValue(float(g["spec_sld"]))
    hs = m.radius.histograms()
    hs.append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=12, xscale="log", yweight="vol", partialIntensity="bins"))
    hs.append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=300, xscale="lin", yweight="num", partialIntensity="bins"))   # (numpy: > 256 bins)
    contribs = np.random.RandomState(3).uniform(lo, hi, (40, 1, 3))
    algo = _algo_with_result(m, g["data_q"], g["data_I"], g["data_sigma"], contribs)
    calls = []
    real = engine.histogram_device_rows
    engine.histogram_device_rows = lambda *a, **kw: calls.append([sp.get("partial") for sp in kw["specs"]]) or real(*a, **kw)
    try:
        algo.histogram()
    finally:
        engine.histogram_device_rows = real
    assert calls == [["bins", None]]                            # the device took the first, numpy the second
    scale = algo.result[0]["scalingFactors"][0]
    rows = [batch_model_calc(m, algo.data, np.ascontiguousarray(contribs[:, :, r]), algo.compensationExponent(), want_rows=True)[4].reshape(40, -1)
            for r in range(3)]
    close = lambda a, b: np.allclose(a, b, rtol=RTOL, atol=ATOL)
    for h in hs:
        _check_against(h, *_numpy_curves(h, lambda r: rows[r], contribs, scale), same=close)


def test_a_python_only_model_uses_the_rows_it_holds():
    g = load("g4_sphere_q100_fixed.npz")
    lo, hi = float(g["spec_lo"][0]), float(g["spec_hi"][0])
    m = PythonOnlySphere(); m.radius.setActiveRange((lo, hi)); m.sld.setValue(float(g["spec_sld"]))
    h = mcsas_amd.Histogram(m.radius, lo, hi, binCount=9, xscale="log", yweight="vol", partialIntensity="bins")
    m.radius.histograms().append(h)
    contribs = np.random.RandomState(4).uniform(lo, hi, (30, 1, 2))
    algo = _algo_with_result(m, g["data_q"], g["data_I"], g["data_sigma"], contribs)
    algo.histogram()
    scale = algo.result[0]["scalingFactors"][0]
    rows = [host_model_calc(m, algo.data, contribs[:, :, r], algo.compensationExponent(), want_rows=True)[4] for r in range(2)]
    _check_against(h, *_numpy_curves(h, lambda r: rows[r], contribs, scale), same=X.same_bits)


def test_4097_contributions_go_through_the_host_route():
    q = np.geomspace(1e8, 3e9, 20)
    lo, hi = 2e-9, 1e-7
    m, _ = make_models("sphere", [lo], [hi])
    h = mcsas_amd.Histogram(m.radius, lo, hi, binCount=5, xscale="log", yweight="vol", partialIntensity="bins")
    m.radius.histograms().append(h)
    contribs = np.random.RandomState(5).uniform(1.01 * lo, 0.99 * hi, (4097, 1, 2))
    I = 1.0 / (1.0 + (q / 5e8) ** 4) + 1e-3
    algo = _algo_with_result(m, q, I, 0.02 * I, contribs)
    assert contribs.shape[0] > engine.HISTOGRAM_MAX_CONTRIBS
    algo.histogram()
    scale = algo.result[0]["scalingFactors"][0]
    setup, c = m.setup(), algo.compensationExponent()
    calc = [engine.model_calc(setup, algo.data.q, contribs[:, :, r], c, want_rows=True) for r in range(2)]
    _check_against(h, *_numpy_curves(h, lambda r: calc[r][4], contribs, scale), same=X.same_bits)
    for r in range(2):                                          # the range holds everybody: the scaled model curve
        assert X.same_bits(h.intensity.full[:, r], scale[r] * calc[r][0])


def test_a_series_with_a_request_takes_each_sets_own_call():
    from test_hist2d_gpu import _front_end
    algo, m, datasets, replays = _front_end()
    h1 = m.radius.histograms()[0]
    h1.partialIntensity = "bins"
    assert not series._histograms_batchable(algo, engine)
    alone = []
    for data, rep in zip(datasets, replays):
        algo.data = data
        algo.calc(replay=rep)
        assert h1.intensity.full.shape == (data.count, 3) and h1.binIntensity.full.shape == (6, data.count, 3)
        alone.append(dict(rng=h1.intensity.full.copy(), bins=h1.binIntensity.full.copy(), fields=h1.moments.fields, mean=h1.moments.intensity[0].copy()))
    results, ser = mcsas_amd.run_series(algo, datasets, keys=["a", "b"], replays=replays, batch=True)
    assert all(r is not None for r in results)
    uid = [k for k in ser if len(k) == 4][0]
    assert [fl for _, fl in ser[uid]] == [a["fields"] for a in alone]
    assert X.same_bits(h1.intensity.full, alone[1]["rng"]) and X.same_bits(h1.binIntensity.full, alone[1]["bins"])
    assert X.same_bits(h1.moments.intensity[0], alone[1]["mean"])
    h1.partialIntensity = None
    assert series._histograms_batchable(algo, engine)

"""mcsas_hip_histogram_batch on the device: every array of every set is the one mcsas_hip_histogram returns for that set alone, bit
for bit — whatever else is in the batch, in whatever order, however the batch is cut into chunks.  Contributions are seeded draws
inside the model's ranges (no Monte-Carlo run but in the last two tests); "equal" is numpy.array_equal(..., equal_nan=True)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mcsas_amd
from mcsas_amd import engine
from helpers import load, make_models, FakeData, plugin_twin, product_smearing

C_EXP = 0.6666666


def _synthetic(nq):
    from bench import synthetic_data
    return synthetic_data(nq)


def _edges(lo, hi, nb, xscale):
    return np.linspace(lo, hi, nb + 1) if xscale == "lin" else np.geomspace(lo, hi, nb + 1)


def _spec(pi, lo, hi, nb, xscale, yweight):
    return dict(param_index=pi, yweight=yweight, edges=_edges(lo, hi, nb, xscale), lower=lo, upper=hi)


def _item(setup, lo, hi, nq, N, R, hists, seed, data=None, smear=None, **flags):
    """One set: `hists` = (parameter, bins, xscale, weighting, share of the active range) each."""
    q, I, sig = _synthetic(nq) if data is None else data
    rs = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    contribs = rs.uniform(lo[None, :, None], hi[None, :, None], (N, len(lo), R))
    specs = [_spec(pi, lo[pi], lo[pi] + share * (hi[pi] - lo[pi]), nb, xs, yw) for pi, nb, xs, yw, share in hists]
    return dict(model=setup, q=q, intensity=I, sigma=sig, contribs=contribs, comp_exp=C_EXP, specs=specs, smear=smear, **flags)


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


def _singles(items):
    return [engine.histogram_device(**it) for it in items]


@functools.lru_cache(maxsize=None)
def mixed_sphere_batch():
    """Test 1's sets and each one's single-call result: one and two lane passes over contributions and bins, blocks that leave
    because another set is larger, the first N whose 3N doubles exceed 64 KB of LDS, and the cap."""
    q = _synthetic(130)[0]
    lo, hi = [np.pi / q.max()], [np.pi / q.min()]
    m = mcsas_amd.Sphere(); m.radius.setActiveRange((lo[0], hi[0]))
    s = m.setup()
    items = [
        _item(s, lo, hi, 37, 5, 1, [], 1),
        _item(s, lo, hi, 64, 70, 3, [(0, 1, "lin", "vol", 1.0), (0, 64, "log", "num", 1.0), (0, 65, "lin", "int", 1.0)], 2, find_background=False),
        _item(s, lo, hi, 130, 1, 7, [(0, 130, "lin", "surf", 0.5)], 3, positive_background=True),
        _item(s, lo, hi, 8, 2731, 1, [(0, 10, "log", "vol", 1.0)], 4),
        _item(s, lo, hi, 8, 4096, 2, [(0, 70, "log", "num", 1.0), (0, 3, "lin", "surf", 1.0)], 5),
    ]
    return items, _singles(items)


@functools.lru_cache(maxsize=None)
def model_groups_batch():
    """Test 2's sets (100 q x 40 x 3 each) and each one's single-call result: three built-in models and a slit-smeared sphere."""
    from test_parity_gpu import RANDOM_RANGES
    items = []
    for seed, tag in enumerate(("sphere", "cyl_aspect", "ellcs")):
        lo, hi = RANDOM_RANGES[tag]
        m, _ = make_models(tag, lo, hi, **({"intDiv": 20.} if tag != "sphere" else {}))
        last = len(lo) - 1
        items.append(_item(m.setup(), lo, hi, 100, 40, 3, [(0, 50, "log", "vol", 1.0), (last, 12, "lin", "surf", 1.0), (last, 7, "log", "int", 0.5)], 10 + seed))
    g = load("g7_smearing.npz"); pre = "trapz_slit_"
    q = g[pre + "q"]
    q = np.geomspace(q.min(), q.max(), 100)
    rs = np.random.RandomState(20)
    I = 1.0 / (1.0 + (q / q[30]) ** 4) + 1e-3
    I = I * (1 + 0.02 * rs.standard_normal(100))
    d, _ = product_smearing("trapezoid", False, 25, q, I, 0.02 * I, umbra=float(g[pre + "umbra"]), penumbra=float(g[pre + "penumbra"]))
    m = mcsas_amd.Sphere(); m.radius.setActiveRange((np.pi / q.max(), np.pi / q.min()))
    smear = d.smearArgs(m)
    assert smear is not None
    items.append(_item(m.setup(d), [np.pi / q.max()], [np.pi / q.min()], 100, 40, 3, [(0, 30, "log", "vol", 1.0), (0, 9, "lin", "num", 1.0)], 13,
                       data=(q, I, 0.02 * I), smear=smear))
    refs = _singles(items)
    unsmeared = engine.histogram_device(**{**items[3], "smear": None})
    assert not _equal(unsmeared[0], refs[3][0])                # (the smearing is in the numbers)
    return items, refs


def test_mixed_shapes_in_one_batch():
    items, refs = mixed_sphere_batch()
    got = engine.histogram_device_batch(items)
    assert len(got) == len(items)
    for i, (g, r) in enumerate(zip(got, refs)):
        assert_same_triple(g, r, i)
    assert [len(g[2]) for g in got] == [0, 3, 1, 1, 2]
    assert got[1][2][2]["bins"].shape == (65, 3) and got[2][2][0]["moments"].shape == (5, 7) and got[4][1]["vol"][0].shape == (4096, 2)
    assert (got[1][2][0]["bins"] != 0).all() and (got[4][2][0]["bins"] != 0).any()    # (something was counted)
    assert (got[2][2][0]["bins"] != 0).any()                                          # (the sphere has a surface)


def test_several_model_groups_in_one_batch():
    items, refs = model_groups_batch()
    got = engine.histogram_device_batch(items)
    for i, (g, r) in enumerate(zip(got, refs)):
        assert_same_triple(g, r, i)
    # cylinders and ellipsoids have no surface(): that weighting is all zero, its variance 0 / 0 — a NaN, as in the single call
    for i in (1, 2):
        assert (got[i][2][1]["bins"] == 0).all() and np.isnan(got[i][2][1]["moments"][2]).all() and (got[i][2][0]["bins"] != 0).any()
    # a tuple in histogram_device's argument order is an item as well
    names = ("model", "q", "intensity", "sigma", "contribs", "comp_exp", "specs")
    assert_same_triple(engine.histogram_device_batch([tuple(items[1][k] for k in names)])[0], refs[1])


def test_order_and_company_do_not_matter():
    items, refs = mixed_sphere_batch()
    for i, g in zip(reversed(range(len(items))), engine.histogram_device_batch(items[::-1])):
        assert_same_triple(g, refs[i], ("reversed", i))
    for i, g in zip((3, 1), engine.histogram_device_batch([items[3], items[1]])):
        assert_same_triple(g, refs[i], ("subset", i))


@pytest.mark.parametrize("which,mb,how", [
    ("groups", "0.1", "every set (96 000 B of rows) a chunk of its own"),
    ("groups", "0.2", "two sets share a chunk"),
    ("groups", "0.05", "a set exceeds the budget alone: the single-set path"),
    ("mixed", "0.3", "the first four sets (291 064 B) share a chunk, the last (524 288 B) exceeds the budget alone"),
    ("mixed", "0", "no budget at all"),
])
def test_chunks_give_the_same_arrays(monkeypatch, which, mb, how):
    items, refs = model_groups_batch() if which == "groups" else mixed_sphere_batch()
    whole = engine.histogram_device_batch(items)
    monkeypatch.setenv("MCSAS_HIP_HIST_BATCH_MB", mb)
    cut = engine.histogram_device_batch(items)
    for i, (g, w, r) in enumerate(zip(cut, whole, refs)):
        assert_same_triple(g, w, (how, i))
        assert_same_triple(g, r, (how, i, "single"))


def test_a_plugin_set_between_two_built_in_sets():
    items, refs = mixed_sphere_batch()
    q, I, sig = _synthetic(60)
    lo, hi = [1e-9, 1e-9], [1e-7, 1e-7]
    m, _ = make_models("gausschain", lo, hi)
    twin = engine.histogram_device(**_item(m.setup(), lo, hi, 60, 33, 2, [(0, 20, "log", "vol", 1.0), (1, 5, "lin", "num", 1.0)], 30))
    plugin_twin(m, "gausschain")
    setup = m.setup(FakeData(q))
    assert setup.model_id >= engine.MODEL_PLUGIN0
    mid = _item(setup, lo, hi, 60, 33, 2, [(0, 20, "log", "vol", 1.0), (1, 5, "lin", "num", 1.0)], 30)
    ref = engine.histogram_device(**mid)
    got = engine.histogram_device_batch([items[1], mid, items[2]])
    assert_same_triple(got[0], refs[1], 0)
    assert_same_triple(got[1], ref, "plug-in")
    assert_same_triple(got[1], twin, "plug-in against its built-in twin")
    assert_same_triple(got[2], refs[2], 2)


def test_a_set_between_two_others_matches_the_reference():
    """The reference's quick-start result (its contributions: tests/golden/g45_analyse.npz) histogrammed in the middle of a batch,
    against the reference's bins, CDF, observability and moments at the tolerances of
    test_parity_gpu.test_calc_converges_and_histogram_matches_reference."""
    g = load("g45_analyse.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    lo, hi = float(g["A_lo"]), float(g["A_hi"])
    m, _ = make_models("sphere", [lo], [hi])
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=20, xscale='log', yweight='vol'))
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=12, xscale='lin', yweight='num'))
    algo = mcsas_amd.McSAS.factory()()
    algo.numContribs.setValue(150); algo.numReps.setValue(3); algo.convergenceCriterion.setValue(5.0)
    algo.model = m
    algo.data = mcsas_amd.SASData(q, I, sig, f_limit=g["data_f_limit"])
    algo.result = [dict(contribs=np.array(g["A_contribs"]))]
    items, refs = mixed_sphere_batch()
    got = engine.histogram_device_batch([items[1], algo._histogram_item(), items[2]])
    assert_same_triple(got[0], refs[1]); assert_same_triple(got[2], refs[2])
    algo._histogram_from_device(got[1])
    for hi_, h in enumerate(m.radius.histograms()):
        p = "A_h%d_" % hi_
        np.testing.assert_allclose(h.xLowerEdge, g[p + "edges"], rtol=1e-15)
        np.testing.assert_allclose(h.bins.full, g[p + "bins_full"], rtol=1e-6, atol=1e-300)
        np.testing.assert_allclose(h.bins.mean, g[p + "bins_mean"], rtol=1e-6, atol=1e-300)
        np.testing.assert_allclose(h.bins.std, g[p + "bins_std"], rtol=1e-5, atol=1e-300)
        np.testing.assert_allclose(h.cdf.mean, g[p + "cdf_mean"], rtol=1e-6)
        np.testing.assert_allclose(h.observability, g[p + "obs"], rtol=1e-6)
        np.testing.assert_allclose(np.array(h.moments.fields)[0::2], g[p + "moments"][0::2], rtol=1e-6)


def _series_run(**kw):
    """Five seeded data sets of 40 q x 20 contributions x 3 repetitions x 200 steps, two histograms on the radius.  Uncertainties of
    five times the intensity put every chain below the criterion (a model of nothing but background has a reduced chi-squared of
    1/25); data set 2 has noisy intensities with uncertainties of 1e-5 of them, which no chain reaches: with showIncomplete off it
    stores nothing."""
    q, I, _ = _synthetic(40)
    rs = np.random.RandomState(4)
    datasets = []
    for k in range(5):
        Ik = I * (1.0 + 0.3 * k) * (1 + 0.01 * rs.standard_normal(40))
        datasets.append(mcsas_amd.SASData(q, Ik, (1e-5 if k == 2 else 5.0) * Ik))
    lo, hi = np.pi / q.max(), np.pi / q.min()
    m = mcsas_amd.Sphere(); m.radius.setActiveRange((lo, hi))
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=12, xscale='log', yweight='vol'))
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, 0.5 * hi, binCount=70, xscale='lin', yweight='num'))
    algo = mcsas_amd.McSAS(seed=21)
    algo.numContribs.setValue(20); algo.numReps.setValue(3); algo.maxIterations.setValue(200)
    algo.convergenceCriterion.setValue(5.0); algo.maxRetries.setValue(0); algo.showIncomplete.setValue(False)
    algo.model = m
    results, series = mcsas_amd.run_series(algo, datasets, keys=[10., 11., 12., 13., 14.], **kw)
    state = dict(result=algo.result[0], fractions=algo.fractions, data=algo.data is datasets[-1])
    return results, series, state


def _assert_same_series(a, b, what):
    (ra, sa, ta), (rb, sb, tb) = a, b
    assert [r is None for r in ra] == [r is None for r in rb] == [False, False, True, False, False], what
    for x, y in zip(ra, rb):
        if x is None:
            continue
        assert list(x) == list(y), what
        assert "scalingFactors" in x
        for k in x:
            if k != "times":                                  # (wall-clock seconds of the chains)
                assert _equal(np.asarray(x[k], dtype=float), np.asarray(y[k], dtype=float)), (what, k)
    assert list(sa) == list(sb) and len(sa) == 2, what
    for uid in sa:
        assert [k for k, _ in sa[uid]] == [k for k, _ in sb[uid]] == [10., 11., 13., 14.], what
        for (_, ma), (_, mb) in zip(sa[uid], sb[uid]):
            assert _equal(np.array(ma, dtype=float), np.array(mb, dtype=float)), (what, uid)
    assert ta["data"] and tb["data"]
    for k in ta["fractions"]:
        assert _equal(ta["fractions"][k][0], tb["fractions"][k][0]) and _equal(ta["fractions"][k][1], tb["fractions"][k][1]), (what, k)
    assert _equal(ta["result"]["contribs"], ra[-1]["contribs"]) and _equal(tb["result"]["contribs"], rb[-1]["contribs"])


def test_run_series_with_batched_histograms_equals_the_call_per_data_set():
    sequential = _series_run()
    for kw in (dict(batch=True), dict(overlap=True)):
        per_set = _series_run(batch_histograms=False, **kw)
        batched = _series_run(batch_histograms=True, **kw)
        _assert_same_series(batched, per_set, kw)
        _assert_same_series(batched, sequential, (kw, "sequential"))
        _assert_same_series(_series_run(**kw), per_set, (kw, "default"))


@pytest.mark.parametrize("find_background,positive_background", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("nq", [1, 63, 65])
@pytest.mark.parametrize("N", [7, 8, 9])
def test_histogram_prep_equals_the_device_histogram(N, nq, find_background, positive_background):
    """mcsas_hip_histogram_prep and mcsas_hip_histogram take a repetition's summed intensity, its scale fit and its visibility limits
    through the same kernels: the scaling and the limits are the same bits.  N around the eight-at-a-time column sum (its tail, an
    exact fill, one over), nq around the 64 lanes of the q loops; three repetitions.  Radii inside pi / q and positive uncertainties:
    no limit is a NaN, which would be equal to anything here — but for a single point fitted with a background, where scale and
    background are 0 / 0 by construction and only the equality is asserted."""
    R = 3
    q = np.geomspace(1e8, 3e9, nq)
    lo, hi = np.pi / 3e9, np.pi / 1e8
    m = mcsas_amd.Sphere(); m.radius.setActiveRange((lo, hi))
    rs = np.random.RandomState(100 * N + nq)
    I, sig = 1.0 + rs.rand(nq), 0.1 + rs.rand(nq)
    contribs = rs.uniform(lo, hi, (N, 1, R))
    flags = dict(find_background=find_background, positive_background=positive_background)
    prep = engine.histogram_prep(m.setup(), q, I, sig, contribs, C_EXP, **flags)
    scaling, fractions, hists = engine.histogram_device(m.setup(), q, I, sig, contribs, C_EXP, [], **flags)
    assert prep[0].shape == (2, R) and prep[4].shape == (N, R) and hists == []
    if nq > 1 or not find_background:
        assert not np.isnan(prep[0]).any() and not np.isnan(prep[4]).any()
    np.testing.assert_array_equal(prep[0], scaling)
    np.testing.assert_array_equal(prep[4], fractions["vol"][1])


def test_histogram_prep_with_a_smearing_table_equals_the_device_histogram():
    """The same with a smearing table, which both calls hand to the device in the one place that makes the set there: 9
    contributions (one over the eight-at-a-time column sum), 65 q (one over the 64 lanes), 3 smearing points, 2 repetitions.  The
    table is a slit's, locs = sqrt(q² + offset²), typed in here; it is in the numbers, and scaling and limits are the same bits."""
    import types
    N, nq, R = 9, 65, 2
    q = np.geomspace(1e8, 3e9, nq)
    lo, hi = np.pi / 3e9, np.pi / 1e8
    m = mcsas_amd.Sphere(); m.radius.setActiveRange((lo, hi))
    rs = np.random.RandomState(965)
    I, sig = 1.0 + rs.rand(nq), 0.1 + rs.rand(nq)
    contribs = rs.uniform(lo, hi, (N, 1, R))
    offset = np.array([0., 4e7, 8e7])
    smear = types.SimpleNamespace(locs=np.sqrt(q[:, None] ** 2 + offset[None, :] ** 2), q_offset=offset, weights=np.array([1., 0.7, 0.2]))
    prep = engine.histogram_prep(m.setup(), q, I, sig, contribs, C_EXP, smear=smear)
    scaling, fractions, hists = engine.histogram_device(m.setup(), q, I, sig, contribs, C_EXP, [], smear=smear)
    assert prep[0].shape == (2, R) and prep[4].shape == (N, R) and hists == []
    assert np.isfinite(prep[0]).all() and not np.isnan(prep[4]).any()
    np.testing.assert_array_equal(prep[0], scaling)
    np.testing.assert_array_equal(prep[4], fractions["vol"][1])
    plain = engine.histogram_prep(m.setup(), q, I, sig, contribs, C_EXP)
    assert (plain[0][0] != prep[0][0]).all() and (plain[4] != prep[4]).any()

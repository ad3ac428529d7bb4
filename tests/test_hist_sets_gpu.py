"""The histogram of a joint fit on the device (mcsas_hip_histogram_sets; csrc/hist_kernels.h: hist_fit_sets_kernel,
hist_obs_sets_kernel) against mcsas_hip_histogram where the two must agree bit for bit, and against the exact restatement
tests/sets_shared_exact.py with the bounds derived there and in tests/hist_exact.py / tests/fit_exact.py.  No assertion has a tolerance
that is not such a bound; which contribution is in which bin and where NaN, +-inf and an exact 0 stand are compared by equality.
Shapes: 12 contributions x 3 repetitions, sets of (37, 100) and (64, 3, 63, 130) points, a `vol` histogram of 7 bins and a `num` one
of 70 (more than one pass of 64)."""
import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import engine
from helpers import make_models
import fit_exact as F
import hist_exact as H
import sets_exact as SX
import sets_shared_exact as SH

pytestmark = pytest.mark.gpu

_CASES = {}


def _setup():
    return make_models("sphere", H.PAR_LO[:1], H.PAR_HI[:1])[0].setup()


def ready(set_nq):
    """the case with the device's own rows (model_calc's, as tests/test_hist_exact_gpu.py takes them), made once"""
    if set_nq not in _CASES:
        setup = _setup()

        def rows_fn(q, pset):
            _, v, w, s, rows = engine.model_calc(setup, q, pset, H.C_EXP, want_rows=True)
            return rows, v, w, s
        _CASES[set_nq] = SH.hist_case(set_nq, rows_fn)
    return _CASES[set_nq]


def _triples(c, members=None):
    off = c["off"]
    return [(c["q"][off[s]:off[s + 1]], c["I"][off[s]:off[s + 1]], c["sigma"][off[s]:off[s + 1]])
            for s in (range(len(off) - 1) if members is None else members)]


def _sets_call(c, **kw):
    return engine.histogram_sets(_setup(), _triples(c), c["contribs"], H.C_EXP, c["specs"], find_background=c["find_bg"], device=0, **kw)


def _single_call(c, q, I, sigma):
    return engine.histogram_device(_setup(), q, I, sigma, c["contribs"], H.C_EXP, c["specs"], find_background=c["find_bg"], device=0)


def _same(a, b, what, scaling=True):
    (sc, fr, hs), (rsc, rfr, rhs) = a[:3], b[:3]
    eq = lambda x, y: x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
    assert eq(sc, rsc), (what, "scaling")
    for k in H.WEIGHTS:
        assert eq(fr[k][0], rfr[k][0]) and eq(fr[k][1], rfr[k][1]), (what, "fractions", k)
    assert len(hs) == len(rhs)
    for h, (x, y) in enumerate(zip(hs, rhs)):
        for k in ("bins", "obs", "cdf", "moments"):
            assert eq(x[k], y[k]), (what, "histogram", h, k)


@pytest.mark.parametrize("scale", ("per_set", "shared"))
def test_one_set_is_mcsas_hip_histogram_bit_for_bit(scale):
    c = ready(SH.SET_SHAPES[0])
    one = engine.histogram_sets(_setup(), [(c["q"], c["I"], c["sigma"])], c["contribs"], H.C_EXP, c["specs"], find_background=c["find_bg"],
                                device=0, scale=scale)
    ref = _single_call(c, c["q"], c["I"], c["sigma"])
    _same(one, ref, scale)
    assert np.array_equal(one[3][0], ref[0][0]) and np.array_equal(one[4][0], ref[0][1])
    assert np.isfinite(ref[0]).all() and (ref[0][0] > 0).all()


@pytest.mark.parametrize("set_nq", SH.SET_SHAPES, ids=lambda s: "S%d" % len(s))
def test_per_set_mode_seen_by_one_member_is_that_members_histogram(set_nq):
    """visible_sets = bit ref_set: scaling, fractions and histograms are mcsas_hip_histogram's on that member alone, and every
    member's own fit comes back beside them"""
    c = ready(set_nq)
    for s in range(len(set_nq)):
        got = _sets_call(c, scale="per_set", ref_set=s, visible=[s])
        ref = _single_call(c, *_triples(c, [s])[0])
        _same(got, ref, (set_nq, s))
        assert np.array_equal(got[3][s], ref[0][0]) and np.array_equal(got[4][s], ref[0][1])
        if s:
            assert np.array_equal(got[3], first[3]) and np.array_equal(got[4], first[4])
        first = got


def _report(what, worst, bad):
    for k, v in sorted(worst.items()):
        print("%s  %-10s  largest error / bound %.3g" % (what, k, v))
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("scale", ("per_set", "shared"))
@pytest.mark.parametrize("set_nq", SH.SET_SHAPES, ids=lambda s: "S%d" % len(s))
def test_all_sets_visible_against_exact(set_nq, scale):
    """every set's scale and background inside the bounds of the exact fit (per set: the closed form on the set's own points; shared:
    the (1 + S)-unknown closed form), then limits, fractions, bins, observability, CDF and moments inside hist_exact's bounds at the
    call's own scales, each point's product taken with its own set's scale"""
    c = ready(set_nq)
    S, ref_set = len(set_nq), len(set_nq) - 1
    got = _sets_call(c, scale=scale, ref_set=ref_set)
    sc, set_A, set_b = got[0], got[3], got[4]
    assert np.array_equal(sc[0], set_A[ref_set]) and np.array_equal(sc[1], set_b[ref_set])
    assert np.isfinite(set_A).all() and (set_A > 0).all() and (set_A < 0.5).all(), set_A
    if scale == "shared":
        assert (set_A == set_A[0]).all()
    bad, worst = [], {}
    for r in range(c["R"]):
        bd = SH.fit_sets_bounds(c, r, scale == "shared")
        for s in range(S):
            for name, g, ref in (("scaling", set_A[s, r], bd[s][0]), ("background", set_b[s, r], bd[s][1])):
                ratio = F.within(g, ref)
                worst[name] = max(worst.get(name, 0.0), ratio)
                if not ratio <= 1.0:
                    bad.append("set %d rep %d %s: got %.17g, exact %.17g, error %.3g of its bound %.3g" % (s, r, name, g, float(ref.v), ratio, ref.e))
    _report("%s fit" % scale, worst, bad)
    bad, worst = [], {}
    H.look_triple(bad, worst, c, got[:3], bounds=SH.all_bounds_sets(c, sc[0], set_A, range(S)))
    _report("%s histogram" % scale, H.summarise(worst), bad)


def test_a_size_only_the_second_member_shows_is_visible_with_all():
    """Eleven spheres of 30 nm and one of 1 nm, seen at q up to 1e8 (member 0: the small sphere is a millionth of the curve) and at
    5e8 .. 3e9 (member 1: the large ones have fallen as q^-4, the small one is a tenth of the curve and more); 1 % uncertainties.  The
    small sphere's volume fraction lies above its visibility limit where member 1's points are looked at, and below it as member 0
    alone sees it — the single-member path, and histogram_sets told to look at member 0 only."""
    setup = make_models("sphere", [5e-10], [1e-7])[0].setup()
    contribs = np.full((12, 1, 1), 3e-8)
    contribs[11, 0, 0] = 1e-9
    qs = (np.geomspace(1e7, 1e8, 30), np.geomspace(5e8, 3e9, 40))
    sets = []
    for q, bg in zip(qs, (0.0, 0.0)):
        cum = engine.model_calc(setup, q, np.ascontiguousarray(contribs[:, :, 0]), H.C_EXP)[0]
        I = 1e-3 * cum + bg
        sets.append((q, I, 0.01 * I))
    spec = [dict(param_index=0, yweight="vol", edges=np.geomspace(5e-10, 1e-7, 8), lower=5e-10, upper=1e-7)]
    everyone = engine.histogram_sets(setup, sets, contribs, H.C_EXP, spec, device=0, scale="shared", visible=None)
    member0 = engine.histogram_sets(setup, sets, contribs, H.C_EXP, spec, device=0, scale="shared", visible=[0])
    alone = engine.histogram_device(setup, *sets[0], contribs, H.C_EXP, spec, device=0)
    for name, (sc, fr, hs) in (("all", everyone[:3]), ("member 0 of the joint call", member0[:3]), ("member 0 alone", alone)):
        vf, mv = fr["vol"][0][11, 0], fr["vol"][1][11, 0]
        print("%-28s  vf %.4g  limit %.4g" % (name, vf, mv))
        assert (vf > mv) == (name == "all"), name
        assert fr["vol"][0][0, 0] > fr["vol"][1][0, 0]                        # (a large sphere is visible to everyone)


def test_through_the_front_end_shared_scale_all_members():
    """The quick-start population on two overlapping q ranges on ONE scale, different backgrounds: every repetition converges, the
    members report one scaling, and the `vol` histogram's total is the sum of the volume fractions."""
    spec, sets = SX.quickstart_sets()
    (q0, I0, s0), (q1, I1, s1) = sets
    sets = [(q0, I0, s0), (q1, (I1 - 30.) / 250. + 0.05, s1 / 250.)]                 # (equal scales: member 1 brought to member 0's)
    lo, hi = np.pi / 1e9, np.pi / 1e7
    m, _ = make_models("sphere", [lo], [hi])
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=30, xscale='log', yweight='vol'))
    algo = mcsas_amd.McSAS(seed=11, device=0)
    algo.numContribs.setValue(100); algo.numReps.setValue(4); algo.convergenceCriterion.setValue(1.0)
    algo.model = m
    algo.data = mcsas_amd.DataSets([mcsas_amd.SASData(*s) for s in sets], sharedScale=True, histogramSet="all")
    algo.calc()
    r, d = algo.result[0], algo.details
    print("chi2", d.chisq, "per set", d.set_chisq, "scales", d.set_scaling, "steps", d.num_iter, "attempts", d.attempts)
    assert (d.converged == 1).all() and (d.chisq <= 1.0).all()
    assert (d.set_scaling == d.set_scaling[0]).all() and r["setsScale"] == "shared"
    assert r["sets"][0]["scaling"] == r["sets"][1]["scaling"]
    np.testing.assert_allclose(r["scalingFactors"][0], d.set_scaling[0], rtol=1e-6)
    h = m.radius.histograms()[0]
    vf = algo.fractions["vol"][0]
    assert h.bins.mean.shape == (30,) and np.isfinite(h.bins.mean).all()
    np.testing.assert_allclose(h.bins.mean.sum(), vf.sum(axis=0).mean(), rtol=1e-12)

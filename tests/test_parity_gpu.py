"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the committed
golden vectors.  Tolerances (fp64 path):
  * form factors / intensities: 1e-9 relative (device sincos/j1 vs numpy/scipy differ in the last
    ulps; the sphere's sin x - x cos x cancellation amplifies that to ~1e-12 at small q·R)
  * accept/reject decisions, iteration and move counts, parameter sets: exact
  * chi-squared, scaling: 1e-7 relative (north_star asks for 1e-5)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mcsas_amd
from mcsas_amd import engine
from mcsas_amd import _lib
from oracle import mcsas_oracle as O
from helpers import load, make_models, traj_setup, FakeData, SMEAR_CASES, product_smearing, oracle_smearing, traj_smearing
from helpers import PythonOnlySphere, PythonOnlyCoreShell, _quickstart_algo    # noqa: F401 (other modules take them from here too)


@pytest.mark.parametrize("tag", ["sphere", "cyl_aspect", "cyl_length", "ellcs", "kholodenko", "elliso", "sphcs",
                                 "gausschain", "lmasphere"])
def test_model_calc_vs_reference_vectors(tag):
    g = load("g12_models.npz")
    m, spec = make_models(tag)
    q, pset, c = g[tag + "_q"], g[tag + "_pset"], float(g["comp_exp"])
    cum, v, w, s, rows = engine.model_calc(m.setup(), q, pset, c, want_rows=True)
    # Kholodenko: the reference itself integrates to QUADPACK epsrel 1e-10
    rt = 2e-9 if tag == "kholodenko" else 1e-9
    if tag == "lmasphere":
        # the reference's structure-factor expression (lmadensesphere.py:79-85) cancels catastrophically at
        # small 2qR_h (terms ~A^-5 that sum to O(1)): its own value carries ~1e-7 noise there, so an ulp of
        # difference in sin/cos moves the result by that much
        rt = 1e-6
    np.testing.assert_allclose(rows, g[tag + "_rows"], rtol=rt)
    np.testing.assert_allclose(cum, g[tag + "_cumInt"], rtol=rt)
    np.testing.assert_allclose(v, g[tag + "_vset"], rtol=1e-13)
    np.testing.assert_allclose(w, g[tag + "_wset"], rtol=1e-12)
    np.testing.assert_allclose(s, g[tag + "_sset"], rtol=1e-13)
    # class-level API: ScatteringModel.calc -> SASModelData
    class D: pass
    d = D(); d.q = q
    md = m.calc(d, pset, c)
    np.testing.assert_allclose(md.chisqrInt, g[tag + "_cumInt"], rtol=rt)
    assert md.numParams == m.activeParamCount()


def test_radially_isotropic_cylinders_plugin_vs_reference_vectors():
    """mcsas_amd.CylindersRadiallyIsotropic (models/cylindersradiallyisotropic.py, shipped as a run-time plug-in with an orientation
    loop in its form factor) against the reference's own formfactor / calc vectors (G18); a reference-shaped object of that class
    name flattens to the same plug-in (setup_from_model: SHIPPED_PLUGINS)."""
    g = load("g18_cylradiso_models.npz")
    m, spec = make_models("cylradiso", aspect=float(g["aspect"]), sld=float(g["sld"]), psiAngleDivisions=float(g["divisions"]))
    setup = m.setup()
    assert setup.model_id >= engine.MODEL_PLUGIN0
    q, pset, c = g["q"], g["pset"], float(g["comp_exp"])
    cum, v, w, s, rows = engine.model_calc(setup, q, pset, c, want_rows=True)
    np.testing.assert_allclose(rows, g["rows"], rtol=1e-9)
    np.testing.assert_allclose(cum, g["cumInt"], rtol=1e-9)
    np.testing.assert_allclose(v, g["vset"], rtol=1e-13)
    np.testing.assert_allclose(w, g["wset"], rtol=1e-12)
    np.testing.assert_allclose(s, g["sset"], rtol=1e-13)
    twin = type("CylindersRadiallyIsotropic", (mcsas_amd.SASModel,), {"parameters": mcsas_amd.CylindersRadiallyIsotropic.parameters})()
    for p_ours, p_twin in zip(m.params(), twin.params()):
        p_twin.setValue(p_ours())
        if hasattr(p_ours, "setActive"):
            p_twin.setActive(p_ours.isActive()); p_twin.setActiveRange(p_ours.activeRange())
    assert not hasattr(twin, "hipSource")
    assert mcsas_amd.setup_from_model(twin).model_id == setup.model_id          # the same text, compiled once


def test_bgfit_vs_reference():
    g = load("g3_bgfit.npz")
    I, sig = g["I"], g["sigma"]
    for C, (ci, fb, pb), lm in zip(g["C"], g["flags"], g["lm"]):
        sc, cv, ag = engine.bgfit(I, sig, C, bool(fb), bool(pb), 1)
        np.testing.assert_allclose(cv, lm[2], rtol=1e-10)
        np.testing.assert_allclose(sc[0], lm[0], rtol=1e-6)
        np.testing.assert_allclose(ag, lm[3], rtol=1e-6)
    sc, cv, ag = engine.bgfit(g["neg_I"], g["neg_sigma"], g["neg_C"], True, True, 1)
    assert sc[1] == 0.0
    np.testing.assert_allclose(cv, g["neg_pos"][2], rtol=1e-6)


TRAJ = ["g4_sphere_q100_fixed.npz", "g4_sphere_q100_converge.npz", "g4_sphere_q512_fixed.npz",
        "g4_sphere_q100_nobg.npz", "g4_sphere_q100_posbg.npz", "g4_sphere_q100_frommin.npz",
        "g4_cyl_q40.npz", "g4_ellcs_q40.npz", "g4_kho_q24.npz", "g4_elliso_q40.npz", "g4_sphcs_q40.npz",
        "g4_gausschain_q40.npz", "g4_lmasphere_q40.npz",
        # round 2: reference replays at the BASELINE shapes of configs 3 and 4 (512 q x 400 cylinders, 2000 steps;
        # 1024 q x 1000 core-shell ellipsoids, 1500 steps), a 64 q x 64 x 300-step Kholodenko chain on the
        # reference's worm data file, and config 5 AS NAMED (that file at 512 q x 600 contributions, 300 steps)
        "g9_cyl_q512.npz", "g9_ellcs_q1024.npz", "g9_kho_q64.npz", "g9_kho_q512.npz",
        # round 3: config 2's shape (512 q x 400) over long budgets — 25 000 fixed steps (62 sweeps over the contributions) and a
        # chain that the reference ends by convergence (criterion 2, 5509 steps)
        "g14_sphere_q512_long.npz", "g14_sphere_q512_converge.npz",
        # round 4: chains the reference ENDS BY CONVERGENCE (criterion 1) for models with an orientation integral (cylinders 6228
        # steps, core-shell ellipsoids 1887 steps; 100 q x 200 contributions) and with positiveBackground (sphere, criterion 2, 5768 steps)
        "g17_cyl_q100_converge.npz", "g17_ellcs_q100_converge.npz", "g17_sphere_q100_posbg_converge.npz",
        # round 4: radially isotropic cylinders — no built-in kernel, the shipped model class hands its form factor to the library
        # as HIP text (mcsas_amd.CylindersRadiallyIsotropic.hipSource, rows with an integral): every mode compiled at run time
        "g18_cylradiso_q40.npz",
        # round 5: config 5 AS NAMED over 1300 steps = more than two sweeps over its 600 contributions (every contribution is proposed
        # again after it may have been replaced: the eager slot swap of an accepted row is read back at the named shape)
        "g9_kho_q512_long.npz"]


@pytest.mark.parametrize("name", TRAJ)
@pytest.mark.parametrize("cache,waves", [(1, 1), (0, 1), (1, 8), (1, 3), (1, -3)])
def test_replay_trajectories_vs_reference(name, cache, waves):
    """The uniform stream the reference consumed, replayed on the GPU, gives the reference's
    accept/reject trajectory: same iteration count, same number of moves, same final parameter
    set, chi-squared within 1e-7."""
    import os
    from helpers import G as golden
    if not os.path.exists(os.path.join(golden, name)):
        pytest.skip("fixture %s not generated yet" % name)
    if name.startswith("g9_") and (cache, waves) == (0, 1):
        pytest.skip("re-evaluating `old` every step at the full shapes is covered by the small replays")
    g, m, spec, st, ost = traj_setup(name)
    st.cache_intensities = cache
    if waves == -3:                      # whole-chip pipeline
        st.exec_mode, st.waves_per_chain = engine.EXEC_PIPELINE, 0
    else:
        st.waves_per_chain = waves
    if waves > 1 and 2 * (waves - 1) > st.n_contrib:
        pytest.skip("window does not fit 2K <= N")
    try:
        res = engine.analyse(m.setup(FakeData(g["data_q"])), g["data_q"], g["data_I"], g["data_sigma"], st,
                             replay=g["stream"][None, :])
    except mcsas_amd._lib.McSASHipError as e:
        # one workgroup per chain keeps its window's d rows in LDS: at 1024 q eight waves do not fit and say so
        assert e.code == -1 and waves > 1 and len(g["data_q"]) > 512
        pytest.skip("workgroup kernel refuses this shape: " + str(e))
    assert res.num_iter[0] == int(g["res_num_iter"])
    assert res.num_moves[0] == int(g["res_num_moves"])
    np.testing.assert_allclose(res.contribs[:, :, 0], g["res_rset"], rtol=1e-12)
    rtol = 1e-5 if "posbg" in name else 1e-7
    minpack_gave_up = name == "g17_sphere_q100_posbg_converge.npz"      # (its last fit hit maxfev: tests/test_oracle_golden.py)
    if minpack_gave_up:
        assert float(g["res_conval"]) * (1 - 1e-2) < res.chisq[0] <= float(g["res_conval"]) * (1 + 1e-9)
    else:
        np.testing.assert_allclose(res.chisq[0], float(g["res_conval"]), rtol=rtol)
    if "posbg" in name:
        # (the reference's MINPACK stalls next to the |b| kink of positiveBackground — its chi² is 1e-6 above the minimum; against
        # the closed-form minimiser of the same residual, replayed by the oracle, there is no such slack)
        ref = O.mc_fit(spec, g["data_q"], g["data_I"], g["data_sigma"], g["data_f_limit"], g["data_x0_limit"], ost,
                       O.ReplayStream(g["stream"]), method="closed")
        assert ref.num_moves == res.num_moves[0]
        np.testing.assert_allclose(res.chisq[0], ref.conval, rtol=1e-9)
        if minpack_gave_up:
            np.testing.assert_allclose(res.fit[:, 0], ref.fit, rtol=1e-9)
            np.testing.assert_allclose(res.scaling[0], ref.scaling, rtol=1e-9)
            return
    # (atol: scale * model + background crosses zero on the worm data file, whose intensity spans 9 decades)
    np.testing.assert_allclose(res.fit[:, 0], g["res_fit"], rtol=1e-6, atol=1e-12 * np.abs(g["res_fit"]).max())
    np.testing.assert_allclose(res.scaling[0], float(g["res_scaling"]), rtol=1e-6)
    assert res.draws[0] == (0 if st.start_from_minimum else ost.n_contrib * spec.n_active) + res.num_iter[0] * spec.n_active


@pytest.mark.parametrize("waves", [1, 8, -3])
def test_positive_background_chain_that_only_minpack_follows(waves):
    """g17_..._posbg_minpack (see tests/test_oracle_golden.py): the reference's MINPACK decides accepted move 584 of this chain by
    stopping 1e-6 above the minimum next to the |b| kink.  The kernels minimise in closed form: on the same stream (continued) they
    are the closed-form oracle decision for decision, to convergence."""
    g, m, spec, st, ost = traj_setup("g17_sphere_q100_posbg_minpack.npz")
    if waves == -3:
        st.exec_mode = engine.EXEC_PIPELINE
    else:
        st.waves_per_chain = waves
    longer = np.concatenate([g["stream"], np.random.RandomState(1).random_sample(20000)])
    ref = O.mc_fit(spec, g["data_q"], g["data_I"], g["data_sigma"], g["data_f_limit"], g["data_x0_limit"], ost,
                   O.ReplayStream(longer), method="closed")
    res = engine.analyse(m.setup(FakeData(g["data_q"])), g["data_q"], g["data_I"], g["data_sigma"], st, replay=longer[None, :])
    assert res.num_iter[0] == ref.num_iter and res.num_moves[0] == ref.num_moves and res.converged[0] == 1
    np.testing.assert_allclose(res.contribs[:, :, 0], ref.rset, rtol=1e-12)
    np.testing.assert_allclose(res.chisq[0], ref.conval, rtol=1e-9)
    assert res.num_iter[0] != int(g["res_num_iter"])          # (documented: not the reference's count)


@pytest.mark.parametrize("waves", [1, 8, -3])
def test_analyse_reps_retries_and_result_dict(waves):
    """McSAS.analyse with 2 reps x 3 attempts (maxRetries=2, showIncomplete) against the reference
    run; each rep replays its own slice of the reference's single global stream."""
    g = load("g45_analyse.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    m, spec = make_models("sphere", [float(g["A_lo"])], [float(g["A_hi"])])
    ost = O.Settings(n_contrib=50, n_reps=2, max_iter=60, conv_crit=1e-9, max_retries=2, show_incomplete=True)
    _, info = O.analyse(spec, q, I, sig, g["data_f_limit"], g["data_x0_limit"], ost,
                        O.ReplayStream(g["B_stream"]), method="closed")
    L = max(i["end"] - i["start"] for i in info) + 8
    replay = np.stack([np.resize(g["B_stream"][i["start"]:], L) for i in info])
    algo = mcsas_amd.McSAS.factory()()
    algo.wavesPerChain = max(waves, 0)
    algo.execMode = engine.EXEC_PIPELINE if waves == -3 else 0
    algo.numContribs.setValue(50); algo.numReps.setValue(2); algo.maxIterations.setValue(60)
    algo.convergenceCriterion.setValue(1e-9); algo.maxRetries.setValue(2); algo.showIncomplete.setValue(True)
    algo.model = m
    algo.data = mcsas_amd.SASData(q, I, sig, f_limit=g["data_f_limit"])
    algo.result = []
    algo.analyse(replay=replay)
    res = algo.result[0]
    assert list(algo.details.attempts) == [3, 3]
    assert list(algo.details.draws) == [i["end"] - i["start"] for i in info]
    np.testing.assert_allclose(res["contribs"], g["B_contribs"], rtol=1e-12)
    np.testing.assert_allclose(res["fitMeasValMean"], g["B_fitMean"], rtol=1e-6)
    np.testing.assert_allclose(res["fitMeasValStd"], g["B_fitStd"], rtol=1e-4, atol=1e-9 * g["B_fitMean"].max())
    np.testing.assert_allclose(res["scaling"], g["B_scaling"], rtol=1e-6)
    assert res["numIter"] == float(g["B_numIter"])
    assert len(m.radius.activeValues()) == 2
    # not converged and showIncomplete off -> no result, like mcsas.py:227-230
    algo.showIncomplete.setValue(False); algo.result = []
    algo.analyse(replay=replay)
    assert algo.result == []


def test_calc_converges_and_histogram_matches_reference():
    """Whole McSAS.calc() on the reference's quick-start data: 3 reps to chi² <= 5, then the
    size-distribution histogram (bins, CDF, observability, moments) against the reference's."""
    g = load("g45_analyse.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    lo, hi = float(g["A_lo"]), float(g["A_hi"])
    m, spec = make_models("sphere", [lo], [hi])
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=20, xscale='log', yweight='vol'))
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=12, xscale='lin', yweight='num'))
    ost = O.Settings(n_contrib=150, n_reps=3, max_iter=100000, conv_crit=5.0)
    _, info = O.analyse(spec, q, I, sig, g["data_f_limit"], g["data_x0_limit"], ost,
                        O.ReplayStream(g["A_stream"]), method="closed")
    L = max(i["end"] - i["start"] for i in info) + 8
    replay = np.stack([np.resize(g["A_stream"][i["start"]:], L) for i in info])
    algo = mcsas_amd.McSAS.factory()()
    algo.numContribs.setValue(150); algo.numReps.setValue(3); algo.convergenceCriterion.setValue(5.0)
    algo.model = m
    algo.data = mcsas_amd.SASData(q, I, sig, f_limit=g["data_f_limit"])
    algo.result = []; algo.stop = False
    algo.analyse(replay=replay)
    res = algo.result[0]
    np.testing.assert_allclose(res["contribs"], g["A_contribs"], rtol=1e-12)
    assert res["numIter"] == float(g["A_numIter"])
    np.testing.assert_allclose(res["fitMeasValMean"], g["A_fitMean"], rtol=1e-6)
    np.testing.assert_allclose(res["scaling"], g["A_scaling"], rtol=1e-6)
    np.testing.assert_allclose(res["background"], g["A_background"], rtol=1e-4)
    assert (algo.details.chisq <= 5.0).all()
    algo.histogram()
    for hi_, h in enumerate(m.radius.histograms()):
        p = "A_h%d_" % hi_
        np.testing.assert_allclose(h.xLowerEdge, g[p + "edges"], rtol=1e-15)
        np.testing.assert_allclose(h.bins.full, g[p + "bins_full"], rtol=1e-6, atol=1e-300)
        np.testing.assert_allclose(h.bins.mean, g[p + "bins_mean"], rtol=1e-6, atol=1e-300)
        np.testing.assert_allclose(h.bins.std, g[p + "bins_std"], rtol=1e-5, atol=1e-300)
        np.testing.assert_allclose(h.cdf.mean, g[p + "cdf_mean"], rtol=1e-6)
        np.testing.assert_allclose(h.observability, g[p + "obs"], rtol=1e-6)
        np.testing.assert_allclose(np.array(h.moments.fields)[0::2], g[p + "moments"][0::2], rtol=1e-6)


def test_quickstart_acceptance_free_running():
    """The reference's published workload, end to end and free-running (doc/source/quickstart.rst:66-107): Sphere on
    quickstartdemo1.csv, 300 contributions, criterion 1, one 50-bin log histogram — here 50 repetitions with the device's
    Philox stream against the reference's own 10-repetition run (fixture g13, oracle/make_golden.py gen_quickstart):
    every repetition reaches chi² <= 1, the volume-weighted histogram agrees bin by bin within the two runs' standard
    errors, and the three populations of the document's ground truth (quickstart.rst:195-199: Gaussians at 8, 40 and
    100 nm) come out as three separate modes."""
    g = load("g13_quickstart.npz")
    algo, m = _quickstart_algo(g, 50, 77)
    algo.calc()
    res = algo.result[0]
    assert res["contribs"].shape == (300, 1, 50)
    assert (algo.details.chisq <= 1.0).all() and (algo.details.converged == 1).all()
    h = m.radius.histograms()[0]
    np.testing.assert_allclose(h.xLowerEdge, g["h_edges"], rtol=1e-14)
    ours, ours_se = np.asarray(h.bins.mean), np.asarray(h.bins.std) / np.sqrt(50.)
    ref, ref_se = g["h_bins_mean"], g["h_bins_std"] / np.sqrt(10.)
    se = np.sqrt(ours_se**2 + ref_se**2) + 0.01 * ref.max()
    z = (ours - ref) / se
    assert np.abs(z).max() < 5.0 and np.sqrt(np.mean(z**2)) < 2.0, z
    # the same mean number of iterations within a factor (the stream differs, the statistics do not)
    assert 0.6 < res["numIter"] / float(g["numIter"]) < 1.6
    # total volume fraction and volume-weighted mean radius (Moments.fields[0], [2]) within 2 %
    mo = np.asarray(h.moments.fields, dtype=float)
    np.testing.assert_allclose(mo[[0, 2]], g["h_moments"][[0, 2]], rtol=0.02)
    # three modes: local maxima of the smoothed histogram next to 8+, 40+ and 100 nm (volume weighting on a log axis
    # moves a Gaussian's mode up: the reference's own histogram peaks at 10.9, 47.6 and 99.5 nm)
    x = np.asarray(g["h_mean"])
    sm = np.convolve(ours, [0.25, 0.5, 0.25], mode="same")
    peaks = [x[i] for i in range(1, 49) if sm[i] > sm[i - 1] and sm[i] >= sm[i + 1] and sm[i] > 0.05 * sm.max()]
    assert len(peaks) == 3, peaks
    for got, want in zip(peaks, (1.09e-8, 4.76e-8, 9.95e-8)):
        assert abs(np.log(got / want)) < 0.2, peaks
    # the fit itself: mean over the repetitions against the reference's mean curve
    np.testing.assert_allclose(res["fitMeasValMean"], g["fitMean"], rtol=0.02)




def _heavy_free_setup(tag):
    g = load("g16_%s_free.npz" % tag)
    model = str(g["spec_model"])
    extra = {}
    if model == "cyl_aspect":
        extra = dict(sld=float(g["spec_sld"]), intDiv=float(g["spec_int_div"]))
    if model == "ellcs":
        extra = dict(eta_c=float(g["spec_eta_c"]), eta_s=float(g["spec_eta_s"]), eta_sol=float(g["spec_eta_sol"]),
                     intDiv=float(g["spec_int_div"]))
    m, spec = make_models(model, g["spec_lo"], g["spec_hi"], [int(x) for x in g["spec_gen"]], **extra)
    return g, m, spec


@pytest.mark.parametrize("tag,reps", [("cyl", 24), ("ellcs", 24), ("kho", 12), ("kho32", 24)])
def test_heavy_models_free_running_vs_the_reference_calc(tag, reps):
    """McSAS.calc() end to end and free-running for the models with an orientation / contour integral (mcsas.py:191-285 +
    :445-615), against the reference's own free run of the same workload (fixtures g16_*, oracle/make_golden.py
    gen_free_running_heavy: cylinders and core-shell ellipsoids 100 q x 200 contributions x 8 repetitions to criterion 1 on curves
    of their own model, the worm-like chain on testdata/sasfit_kho-1-10-1000.dat 64 bins x 64 contributions x 3 repetitions to
    criterion 12 ("kho", round 4: three reference repetitions, loose thresholds) and 32 bins x 48 contributions x 12 repetitions to
    criterion 8 ("kho32", round 5: at the cylinders' thresholds)):
    every repetition here reaches the criterion, the mean number of iterations is the reference's within a factor, and every
    configured histogram (one per active parameter) agrees bin by bin within the two runs' standard errors; total volume fraction
    and the distribution mean (Moments.fields[0], [2]) within a few per cent."""
    import os
    from helpers import G as golden
    if not os.path.exists(os.path.join(golden, "g16_%s_free.npz" % tag)):
        pytest.skip("fixture g16_%s_free.npz not generated (the worm-like chain takes the reference hours)" % tag)
    g, m, _ = _heavy_free_setup(tag)
    crit, ref_reps = float(g["crit"]), int(g["reps"])
    hists = []
    for k in range(int(g["n_hist"])):
        pre = "h%d_" % k
        p = getattr(m, str(g[pre + "param"]))
        h = mcsas_amd.Histogram(p, float(g[pre + "lo"]), float(g[pre + "hi"]), binCount=int(g[pre + "nbin"]),
                                xscale=str(g[pre + "xscale"]), yweight=str(g[pre + "yweight"]))
        p.histograms().append(h)
        hists.append((pre, h))
    algo = mcsas_amd.McSAS(seed=77)
    algo.numContribs.setValue(int(g["n_contrib"])); algo.numReps.setValue(reps)
    algo.convergenceCriterion.setValue(crit); algo.maxIterations.setValue(float(g["max_iter"]))
    algo.model = m
    algo.data = mcsas_amd.SASData(g["data_q"], g["data_I"], g["data_sigma"], f_limit=g["data_f_limit"])
    algo.calc()
    res = algo.result[0]
    assert res["contribs"].shape == (int(g["n_contrib"]), len(g["spec_lo"]), reps)
    assert (algo.details.chisq <= crit).all() and (algo.details.converged == 1).all()
    assert 0.5 < res["numIter"] / float(g["numIter"]) < 2.0
    for pre, h in hists:
        np.testing.assert_allclose(h.xLowerEdge, g[pre + "edges"], rtol=1e-14)
        ours, ours_se = np.asarray(h.bins.mean), np.asarray(h.bins.std) / np.sqrt(float(reps))
        ref, ref_se = g[pre + "bins_mean"], g[pre + "bins_std"] / np.sqrt(float(ref_reps))
        se = np.sqrt(ours_se**2 + ref_se**2) + 0.01 * ref.max()
        z = (ours - ref) / se
        # (the numpy oracle run free on the device's Philox streams — which the kernels reproduce chain for chain — gives
        # |z| <= 0.93, rms 0.52 for the cylinders, tools/g16_calibration.py)
        assert np.abs(z).max() < 5.0 and np.sqrt(np.mean(z**2)) < 2.0, (pre, z)
        mo = np.asarray(h.moments.fields, dtype=float)
        np.testing.assert_allclose(mo[[0, 2]], g[pre + "moments"][[0, 2]], rtol=0.05 if tag != "kho" else 0.25)
    # the mean fitted curve within 5 %; the three-repetition worm fixture ("kho") alone gets three standard errors of the two means
    # on top (in the form-factor minima the reference's own three repetitions spread by 19 %, and its fit sits four sigma off the data)
    fit_se = np.sqrt(np.asarray(res["fitMeasValStd"])**2 / reps + g["fitStd"]**2 / ref_reps)
    allow = 3. * fit_se if tag == "kho" else 0.
    assert (np.abs(res["fitMeasValMean"] - g["fitMean"]) <= 0.05 * np.abs(g["fitMean"]) + allow).all()


@pytest.mark.parametrize("mode", [engine.EXEC_PIPELINE, engine.EXEC_WAVE, engine.EXEC_WORKGROUP])
def test_device_list_shards_repetitions_like_one_device(mode):
    """mcsas_problem.n_devices / devices (the repetition loop of mcsas.py:214-262 over several GPUs, inside the C ABI): the
    same device listed two and three times stands in for two and three GPUs on this one-GPU box — every block runs from
    its own host thread with its own plan and stream, concurrently — and every array of the result is bit for bit what
    one device computes for all repetitions (chain id = global repetition index; the pipeline's window geometry does
    not depend on how many chains share a launch)."""
    g = load("g4_sphere_q100_fixed.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    m, _ = make_models("sphere", g["spec_lo"], g["spec_hi"])
    st = engine.Settings(n_contrib=200, n_reps=7, max_iter=3000, conv_crit=0.5, max_retries=1, seed=11, rep_offset=2, exec_mode=mode)
    one = engine.analyse(m.setup(), q, I, sig, st)
    assert len(set(one.num_moves.tolist())) > 3
    for devs in ((0, 0), (0, 0, 0), (0,) * 9):
        st2 = engine.Settings(**{**st.__dict__, "devices": devs})
        many = engine.analyse(m.setup(), q, I, sig, st2)
        for name in ("contribs", "fit", "chisq", "scaling", "background", "num_iter", "num_moves", "attempts", "converged", "draws"):
            np.testing.assert_array_equal(getattr(many, name), getattr(one, name), err_msg="%s with %d devices" % (name, len(devs)))
    # a replayed stream is split along with the repetitions
    replay = np.stack([g["stream"][k:k + 1720] for k in (0, 50, 100, 150, 200)])
    st3 = engine.Settings(n_contrib=200, n_reps=5, max_iter=1500, conv_crit=1e-9, max_retries=0, exec_mode=mode)
    a = engine.analyse(m.setup(), q, I, sig, st3, replay=replay)
    b = engine.analyse(m.setup(), q, I, sig, engine.Settings(**{**st3.__dict__, "devices": (0, 0)}), replay=replay)
    np.testing.assert_array_equal(a.contribs, b.contribs); np.testing.assert_array_equal(a.num_moves, b.num_moves)
    # a device that does not exist fails the whole call, loudly
    with pytest.raises(mcsas_amd._lib.McSASHipError) as e:
        engine.analyse(m.setup(), q, I, sig, engine.Settings(**{**st.__dict__, "devices": (0, 99)}))
    assert e.value.code == -2


def test_mcsas_front_end_takes_a_device_list():
    g = load("g13_quickstart.npz")
    out = []
    for dev in (0, [0, 0, 0]):
        lo, hi = float(g["lo"]), float(g["hi"])
        m, _ = make_models("sphere", [lo], [hi])
        m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=20, xscale='log', yweight='vol'))
        algo = mcsas_amd.McSAS(seed=3, device=dev, execMode=engine.EXEC_PIPELINE)
        algo.numContribs.setValue(100); algo.numReps.setValue(5); algo.convergenceCriterion.setValue(20.0)
        algo.model = m
        algo.data = mcsas_amd.SASData(g["data_q"], g["data_I"], g["data_sigma"], f_limit=g["data_f_limit"])
        algo.calc()
        out.append((algo.result[0]["contribs"].copy(), np.asarray(m.radius.histograms()[0].bins.mean).copy()))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])



def test_mcsas_front_end_device_list_with_an_integral_model_in_auto_mode():
    """mcsas_amd.McSAS(device=[0, 0]) for a model whose rows cost an integral, MCSAS_EXEC_AUTO (it picks the row-queue pipeline on
    every block): the repetition loop of mcsas.py:214-262 split over two plans on two host threads inside the C ABI gives the arrays of
    one device bit for bit (chain id = global repetition index; the window follows each plan's contribution, chain and CU counts —
    pipe_layout.h: pipe_geometry — and nothing a chain decides depends on it), histogram included."""
    g = load("g16_cyl_free.npz")
    out = []
    for dev in (0, [0, 0]):
        m, _ = make_models("cyl_aspect", g["spec_lo"], g["spec_hi"], [int(x) for x in g["spec_gen"]], sld=float(g["spec_sld"]),
                           intDiv=float(g["spec_int_div"]))
        m.radius.histograms().append(mcsas_amd.Histogram(m.radius, float(g["spec_lo"][0]), float(g["spec_hi"][0]), binCount=12,
                                                         xscale='log', yweight='vol'))
        algo = mcsas_amd.McSAS(seed=5, device=dev)
        algo.numContribs.setValue(96); algo.numReps.setValue(7); algo.convergenceCriterion.setValue(3.0)
        algo.maxIterations.setValue(4000)
        algo.model = m
        algo.data = mcsas_amd.SASData(g["data_q"], g["data_I"], g["data_sigma"], f_limit=g["data_f_limit"])
        algo.calc()
        assert algo.result, "calc() gave no result"
        out.append((algo.result[0]["contribs"].copy(), np.asarray(algo.result[0]["fitMeasValMean"]).copy(),
                    np.asarray(m.radius.histograms()[0].bins.mean).copy(), algo.details.num_iter.copy()))
    assert len(set(out[0][3].tolist())) > 2                    # (chains end at different steps)
    for a, b in zip(out[0], out[1]):
        np.testing.assert_array_equal(a, b)


def test_python_only_model_replays_the_reference_through_host_rows():
    """A ScatteringModel that exists only as Python (the reference's plug-in contract as it stands: scatteringmodel.py:16-58,
    sasmodel.py:37-79) runs through McSAS.calc(): the library draws the proposals, calls back into the model's own calcIntensity
    for the rows of a window (mcsas_hip_analyse_host_rows) and takes every decision on the device.  Fed the uniform stream the
    reference consumed (g4_sphere_q100_fixed), it reproduces the reference's chain: iterations, accepted moves, parameter set exact,
    chi² 1e-9 — and equals the built-in sphere kernel run on the same stream; histogram() works on the result."""
    g, m_builtin, spec, st, ost = traj_setup("g4_sphere_q100_fixed.npz")
    assert mcsas_amd.scatteringmodels.is_host_model(PythonOnlySphere())
    out = {}
    for tag, cls in (("python", PythonOnlySphere), ("builtin", mcsas_amd.Sphere)):
        m = cls()
        lo, hi = float(g["spec_lo"][0]), float(g["spec_hi"][0])
        m.radius.setActiveRange((lo, hi)); m.sld.setValue(float(g["spec_sld"]))
        m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=20, xscale='log', yweight='vol'))
        algo = mcsas_amd.McSAS(seed=1)
        algo.numContribs.setValue(st.n_contrib); algo.numReps.setValue(1); algo.maxIterations.setValue(st.max_iter)
        algo.convergenceCriterion.setValue(st.conv_crit); algo.compensationExponent.setValue(st.comp_exp); algo.showIncomplete.setValue(True)
        algo.maxRetries = mcsas_amd.mcsas._Setting("maxRetries", 0)
        algo.hostRowWindow = 37                                   # (a window that does not divide the budget)
        algo.model = m
        algo.data = mcsas_amd.SASData(g["data_q"], g["data_I"], g["data_sigma"], f_limit=g["data_f_limit"])
        algo.calc(replay=g["stream"][None, :])
        d = algo.details
        out[tag] = (algo.result[0]["contribs"].copy(), d.chisq.copy(), np.asarray(m.radius.histograms()[0].bins.mean).copy())
        assert d.num_iter[0] == int(g["res_num_iter"]) and d.num_moves[0] == int(g["res_num_moves"]), tag
        np.testing.assert_allclose(algo.result[0]["contribs"][:, :, 0], g["res_rset"], rtol=1e-15)
        np.testing.assert_allclose(d.chisq[0], float(g["res_conval"]), rtol=1e-9)
        np.testing.assert_allclose(algo.result[0]["fitMeasValMean"][0], g["res_fit"], rtol=1e-6)
    np.testing.assert_array_equal(out["python"][0], out["builtin"][0])
    np.testing.assert_allclose(out["python"][1], out["builtin"][1], rtol=1e-12)
    np.testing.assert_allclose(out["python"][2], out["builtin"][2], rtol=1e-9, atol=1e-300)


def test_python_only_model_free_running_retries_and_stop():
    """Host rows, free-running: several chains with a criterion some reach within the budget and some only in a later attempt
    (the retry loop of mcsas.py:220-246 is followed between windows, the random stream goes on where the attempt stopped), against
    the numpy oracle on the same Philox streams; and McSAS.stop raised by the model's own callback ends every chain where it is."""
    g = load("g4_sphere_q100_fixed.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    lo, hi = float(g["spec_lo"][0]), float(g["spec_hi"][0])
    m = PythonOnlySphere(); m.radius.setActiveRange((lo, hi)); m.sld.setValue(float(g["spec_sld"]))
    _, spec = make_models("sphere", [lo], [hi], sld=float(g["spec_sld"]))
    data = mcsas_amd.SASData(q, I, sig, f_limit=g["data_f_limit"])
    st = engine.Settings(n_contrib=60, n_reps=5, max_iter=400, conv_crit=350.0, max_retries=2, seed=77, rep_offset=3)
    setup = m.setup(data)

    def rows(pset):
        return mcsas_amd.scatteringmodels.host_model_calc(m, data, pset, st.comp_exp, want_rows=True)[4]
    res = engine.analyse_host_rows(setup, q, I, sig, st, rows, window=50)
    ost = O.Settings(n_contrib=60, n_reps=1, max_iter=400, conv_crit=350.0, max_retries=2)
    attempts = []
    for r in range(5):
        stream = O.PhiloxStream(77, 3 + r)
        for att in range(3):
            ref = O.mc_fit(spec, q, I, sig, g["data_f_limit"], g["data_x0_limit"], ost, stream, method="closed")
            if ref.conval <= 350.0:
                break
        attempts.append(att + 1)
        assert res.attempts[r] == att + 1 and res.num_iter[r] == ref.num_iter and res.num_moves[r] == ref.num_moves, r
        assert res.draws[r] == stream.pos
        np.testing.assert_allclose(res.contribs[:, :, r], ref.rset, rtol=1e-13)
        np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-9)
    assert sorted(set(attempts)) == [1, 2, 3] and res.converged.sum() == 4      # (one chain misses the criterion in all three attempts)
    # stop: raised inside the third callback
    import ctypes
    stop = ctypes.c_int32(0)
    calls = []

    def rows_then_stop(pset):
        calls.append(len(pset))
        if len(calls) == 3:
            stop.value = 1
        return rows(pset)
    st2 = engine.Settings(n_contrib=60, n_reps=4, max_iter=100000, conv_crit=0.0, max_retries=0, seed=5)
    res2 = engine.analyse_host_rows(setup, q, I, sig, st2, rows_then_stop, stop=stop, window=40)
    assert len(calls) == 3 and (res2.num_iter == 80).all() and (res2.converged == 0).all() and np.isfinite(res2.chisq).all()
    # a callback that raises: the exception comes back to the caller, nothing hangs
    def bad(pset):
        raise ZeroDivisionError("model failed")
    with pytest.raises(ZeroDivisionError):
        engine.analyse_host_rows(setup, q, I, sig, st2, bad)


def test_python_only_model_flags_and_stream_end():
    """Host rows with the settings that change mcFit's set-up and fit — startFromMinimum (mcsas.py:310-315: no draws for the initial
    set), no background, positiveBackground — against the numpy oracle on the same replayed stream; and a replay stream that is too
    short is reported (MCSAS_ESTREAM), as by every other entry point — in both directions: reported if and only if a step the
    chain took needed a draw behind the stream's end, not for what was drawn ahead for a window the chain left early
    (tests/test_chain_end_gpu.py pins that for every entry point)."""
    g = load("g4_sphere_q100_fixed.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    lo, hi = float(g["spec_lo"][0]), float(g["spec_hi"][0])
    _, spec = make_models("sphere", [lo], [hi], sld=float(g["spec_sld"]))
    stream = g["stream"][:60 + 300 + 4]
    for flags in (dict(start_from_minimum=True), dict(find_background=False), dict(positive_background=True)):
        m = PythonOnlySphere(); m.radius.setActiveRange((lo, hi)); m.sld.setValue(float(g["spec_sld"]))
        data = mcsas_amd.SASData(q, I, sig, f_limit=g["data_f_limit"])
        st = engine.Settings(n_contrib=60, n_reps=1, max_iter=300, conv_crit=1e-9, max_retries=0, **flags)
        rows = lambda pset: mcsas_amd.scatteringmodels.host_model_calc(m, data, pset, st.comp_exp, want_rows=True)[4]
        res = engine.analyse_host_rows(m.setup(data), q, I, sig, st, rows, replay=stream[None, :], window=64)
        ost = O.Settings(n_contrib=60, n_reps=1, max_iter=300, conv_crit=1e-9, find_bg=st.find_background, pos_bg=st.positive_background,
                         start_from_min=st.start_from_minimum)
        ref = O.mc_fit(spec, q, I, sig, g["data_f_limit"], g["data_x0_limit"], ost, O.ReplayStream(stream), method="closed")
        assert res.num_iter[0] == ref.num_iter == 300 and res.num_moves[0] == ref.num_moves, flags
        assert res.draws[0] == (300 if st.start_from_minimum else 360)
        np.testing.assert_allclose(res.contribs[:, :, 0], ref.rset, rtol=1e-13)
        np.testing.assert_allclose(res.chisq[0], ref.conval, rtol=1e-9)
        np.testing.assert_allclose([res.scaling[0], res.background[0]], [ref.scaling, ref.background], rtol=1e-8, atol=1e-300)
    with pytest.raises(_lib.McSASHipError) as e:
        engine.analyse_host_rows(m.setup(data), q, I, sig, engine.Settings(n_contrib=60, n_reps=1, max_iter=300, conv_crit=1e-9, max_retries=0),
                                 rows, replay=stream[None, :200], window=64)
    assert e.value.code == -5                                   # MCSAS_ESTREAM


def test_python_only_model_two_parameters_more_than_1024_q():
    """Host rows with two active parameters (exponential generators), 1300 q-points (q slots beyond a wavefront's 1024) and a
    model that declares more parameters than the C ABI carries: free-running chains follow the numpy oracle of the same model
    (oracle: models/sphericalcoreshell.py restated) on the device's Philox streams, retries included."""
    q = np.logspace(7, np.log10(3e9), 1300)
    rs = np.random.RandomState(5)
    m = PythonOnlyCoreShell()
    lo, hi = [2e-9, 5e-10], [1e-7, 2e-8]
    m.radius.setActiveRange((lo[0], hi[0])); m.t.setActiveRange((lo[1], hi[1]))
    assert len(m.params()) == 11 and mcsas_amd.scatteringmodels.is_host_model(m)
    _, spec = make_models("sphcs", lo, hi)
    truth = np.stack([rs.uniform(5e-9, 5e-8, 30), rs.uniform(1e-9, 1e-8, 30)], axis=1)
    It = O.model_calc(spec, q, truth, 0.6666666)[0]
    It *= 1e3 / It.max()
    sig = 0.02 * It
    I = It * (1 + 0.02 * rs.normal(size=len(q)))
    data = mcsas_amd.SASData(q, I, sig)
    st = engine.Settings(n_contrib=40, n_reps=3, max_iter=150, conv_crit=1e-9, max_retries=1, seed=9)
    rows = lambda pset: mcsas_amd.scatteringmodels.host_model_calc(m, data, pset, st.comp_exp, want_rows=True)[4]
    res = engine.analyse_host_rows(m.setup(data), q, I, sig, st, rows, window=33)
    ost = O.Settings(n_contrib=40, n_reps=1, max_iter=150, conv_crit=1e-9, max_retries=1)
    for r in range(3):
        stream = O.PhiloxStream(9, r)
        for att in range(2):
            ref = O.mc_fit(spec, q, I, sig, [I.min(), I.max()], [q.min(), q.max()], ost, stream, method="closed")
        assert res.attempts[r] == 2 and res.num_iter[r] == ref.num_iter == 150 and res.num_moves[r] == ref.num_moves, r
        assert res.draws[r] == stream.pos
        np.testing.assert_allclose(res.contribs[:, :, r], ref.rset, rtol=1e-12)
        np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-9)
        np.testing.assert_allclose(res.fit[:, r], ref.fit, rtol=1e-9)


@pytest.mark.parametrize("waves", [1, 8, 5, -3])
def test_free_running_philox_matches_oracle(waves):
    """Free-running chains (device Philox) follow the oracle run with the same counter-based stream:
    identical decisions, parameter sets and iteration counts for every rep."""
    g = load("g4_sphere_q100_fixed.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    m, spec = make_models("sphere", g["spec_lo"], g["spec_hi"])
    st = engine.Settings(n_contrib=80, n_reps=4, max_iter=500, conv_crit=1e-9, max_retries=0, seed=20250101, rep_offset=3,
                         waves_per_chain=max(waves, 0), exec_mode=engine.EXEC_PIPELINE if waves == -3 else 0)
    res = engine.analyse(m.setup(), q, I, sig, st)
    ost = O.Settings(n_contrib=80, n_reps=1, max_iter=500, conv_crit=1e-9)
    for r in range(4):
        ref = O.mc_fit(spec, q, I, sig, g["data_f_limit"], g["data_x0_limit"], ost,
                       O.PhiloxStream(20250101, 3 + r), method="closed")
        assert res.num_moves[r] == ref.num_moves
        np.testing.assert_allclose(res.contribs[:, :, r], ref.rset, rtol=1e-12)
        np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-7)
    assert len(set(res.num_moves.tolist())) > 1 or len(set(np.round(res.chisq, 6).tolist())) > 1


@pytest.mark.parametrize("waves", [1, 8, -3])
def test_full_size_properties_config2(waves):
    """BASELINE config 2 shape (512 q x 400 contribs x 50 reps), fixed budget: size-independent
    properties — chi² decreases monotonically with the step budget on the same seed, reported chi²
    equals a direct evaluation of the reported fit, and contributions stay inside the range."""
    g = load("g4_sphere_q512_fixed.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    m, _ = make_models("sphere", g["spec_lo"], g["spec_hi"])
    chis = []
    for steps in (200, 2000):
        st = engine.Settings(n_contrib=400, n_reps=50, max_iter=steps, conv_crit=0.0, max_retries=0, seed=7,
                             waves_per_chain=max(waves, 0), exec_mode=engine.EXEC_PIPELINE if waves == -3 else 0)
        res = engine.analyse(m.setup(), q, I, sig, st)
        assert (res.num_iter == steps).all()
        direct = (((I[:, None] - res.fit) / sig[:, None])**2).sum(axis=0) / len(q)
        np.testing.assert_allclose(res.chisq, direct, rtol=1e-9)
        assert (res.contribs >= g["spec_lo"][0]).all() and (res.contribs <= g["spec_hi"][0]).all()
        chis.append(res.chisq.copy())
    assert (chis[1] < chis[0]).all()


def test_stop_flag_ends_the_run():
    import ctypes
    g = load("g4_sphere_q100_fixed.npz")
    m, _ = make_models("sphere", g["spec_lo"], g["spec_hi"])
    stop = ctypes.c_int32(1)          # already set: chains must leave at their first poll
    st = engine.Settings(n_contrib=100, n_reps=2, max_iter=10**9, conv_crit=0.0, max_retries=0, seed=1)
    res = engine.analyse(m.setup(), g["data_q"], g["data_I"], g["data_sigma"], st, stop=stop)
    assert (res.num_iter == 0).all() and (res.converged == 0).all()


def test_errors_are_reported_not_swallowed():
    g = load("g4_sphere_q100_fixed.npz")
    m, _ = make_models("sphere", g["spec_lo"], g["spec_hi"])
    st = engine.Settings(n_contrib=100, n_reps=1, max_iter=50, conv_crit=0.0, max_retries=0)
    with pytest.raises(mcsas_amd._lib.McSASHipError) as e:      # replay stream too short
        engine.analyse(m.setup(), g["data_q"], g["data_I"], g["data_sigma"], st, replay=g["stream"][None, :120])
    assert e.value.code == -5
    bad = m.setup(); bad.model_id = 17
    with pytest.raises(mcsas_amd._lib.McSASHipError):
        engine.analyse(bad, g["data_q"], g["data_I"], g["data_sigma"], st)


@pytest.mark.parametrize("R", [2, 10, 20, 50, 100])
def test_sasfit_sphere_known_answers_on_gpu(R, golden_dir):
    """The reference's own golden vectors (sphere.py:68-75, testRelErr 1e-4 on the mean relative
    error of (V·F)²) through the HIP path: compensationExponent 1 makes F²·V^(2c) = (V·F)²."""
    import os
    d = np.loadtxt(os.path.join(golden_dir, "ref_testdata", "sasfit_sphere-%d-1.dat" % R))
    q, Iref = d[:, 0], d[:, 1]
    m, _ = make_models("sphere")
    cum, v, w, s = engine.model_calc(m.setup(), q, [[float(R)]], 1.0)
    assert np.mean(np.abs((Iref - cum) / Iref)) < 1e-4


def test_sasfit_kholodenko_known_answer_on_gpu(golden_dir):
    """kholodenko.py:98-102: testVolExp = 0 (intensity = F²), default testRelErr 1e-5, all 501 rows."""
    import os
    d = np.loadtxt(os.path.join(golden_dir, "ref_testdata", "sasfit_kho-1-10-1000.dat"))
    q, Iref = d[:, 0], d[:, 1]
    m, _ = make_models("kholodenko")
    cum, v, w, s = engine.model_calc(m.setup(), q, [[1.0, 10.0, 1000.0]], 0.0)
    assert np.mean(np.abs((Iref - cum) / Iref)) < 1e-5


def _synthetic(nq):
    from bench import synthetic_data
    return synthetic_data(nq)


FULL = {
    # BASELINE.json configs 3-5 at their full q x contribution sizes; repetitions and step budgets cut so
    # the GPU suite stays short (the form factors of these models cost 100-1000x a sphere's)
    "cfg3_cylinders": dict(tag="cyl_aspect", nq=512, n=400, lo=[1e-9, 0.5], hi=[1e-7, 20.0], reps=6, steps=(40, 160)),
    "cfg4_ellipsoid": dict(tag="ellcs", nq=1024, n=1000, lo=[1e-9, 2e-9, 2e-10], hi=[1e-7, 2e-7, 1e-8], reps=4, steps=(30, 120)),
    "cfg5_kholodenko": dict(tag="kholodenko", nq=512, n=600, lo=None, hi=None, reps=3, steps=(16, 48)),
}


@pytest.mark.parametrize("name", list(FULL))
def test_full_size_properties_other_configs(name):
    """Size-independent properties at the full BASELINE shapes: (1) the three execution modes (wavefront
    / workgroup / whole-chip pipeline) give IDENTICAL chains, (2) chi² never increases with the step
    budget on the same stream, (3) the reported chi² equals a direct evaluation of the reported fit,
    (4) parameters stay inside their generator ranges."""
    c = FULL[name]
    q, I, sig = _synthetic(c["nq"])
    m, _ = make_models(c["tag"], c["lo"], c["hi"])
    setup = m.setup()
    prev = None
    for steps in c["steps"]:
        res = {}
        for mode in (engine.EXEC_PIPELINE, engine.EXEC_WAVE, engine.EXEC_WORKGROUP):
            if mode != engine.EXEC_PIPELINE and steps != c["steps"][0]:
                continue                                  # cross-mode identity on the short budget only
            st = engine.Settings(n_contrib=c["n"], n_reps=c["reps"], max_iter=steps, conv_crit=0.0, max_retries=0,
                                 seed=11, exec_mode=mode)
            try:
                res[mode] = engine.analyse(setup, q, I, sig, st)
            except mcsas_amd._lib.McSASHipError as e:
                if mode == engine.EXEC_PIPELINE:
                    raise
                assert e.code == -1                       # a mode that does not fit this shape says so
        r = res[engine.EXEC_PIPELINE]
        for mode, o in res.items():
            np.testing.assert_array_equal(o.num_moves, r.num_moves)
            np.testing.assert_array_equal(o.contribs, r.contribs)
            np.testing.assert_allclose(o.chisq, r.chisq, rtol=1e-9)
        assert (r.num_iter == steps).all()
        direct = (((I[:, None] - r.fit) / sig[:, None])**2).sum(axis=0) / len(q)
        np.testing.assert_allclose(r.chisq, direct, rtol=1e-9)
        for col in range(setup.n_active):
            assert (r.contribs[:, col, :] >= setup.gen_lo[col]).all() and (r.contribs[:, col, :] <= setup.gen_hi[col]).all()
        if prev is not None:
            assert (r.chisq <= prev * (1 + 1e-12)).all()
        prev = r.chisq.copy()


EDGE = [  # (nq, n_contrib, max_iter, reps)
    (64, 40, 130, 3), (65, 33, 97, 2), (7, 16, 50, 2), (130, 2, 40, 2), (512, 1, 10, 2), (100, 50, 0, 2),
    (300, 200, 700, 5), (1024, 64, 90, 2),
    # more than 1024 q-points (un-binned data files, nBin = 0: the reference takes any data.count, mcsas.py:210): one
    # workgroup per chain with the q-points split over its waves (chain_wide.h: exec_mode 2 and what auto picks), or — up to
    # 4096 — one wavefront per chain with 32 / 64 q slots per lane (exec_mode 1); the pipeline refuses these shapes
    (1500, 40, 120, 2), (2048, 33, 70, 2), (3000, 24, 50, 1), (4096, 20, 40, 1),
    # ... and beyond 4096 (16 / 32 q slots per lane in the q-split kernel), up to 16384
    (5000, 20, 40, 2), (9000, 16, 24, 1), (16384, 16, 12, 1),
]


@pytest.mark.parametrize("nq,n,steps,reps", EDGE)
def test_edge_shapes_all_modes_agree_with_oracle(nq, n, steps, reps):
    """Ragged q counts (padding lanes), tiny contribution counts (window does not fit -> that mode
    must refuse, not misbehave), a single contribution (no loop, mcsas.py:354), zero iterations: every
    execution mode that accepts the shape gives the oracle's chains."""
    q, I, sig = _synthetic(nq)
    m, spec = make_models("sphere", [np.pi / q.max()], [np.pi / q.min()])
    ost = O.Settings(n_contrib=n, n_reps=1, max_iter=steps, conv_crit=1e-9)
    ref = [O.mc_fit(spec, q, I, sig, [I.min(), I.max()], [q.min(), q.max()], ost, O.PhiloxStream(5, r), method="closed")
           for r in range(reps)]
    ran = 0
    for mode in (engine.EXEC_WAVE, engine.EXEC_WORKGROUP, engine.EXEC_PIPELINE, engine.EXEC_AUTO):
        st = engine.Settings(n_contrib=n, n_reps=reps, max_iter=steps, conv_crit=1e-9, max_retries=0, seed=5, exec_mode=mode)
        try:
            res = engine.analyse(m.setup(), q, I, sig, st)
        except mcsas_amd._lib.McSASHipError as e:
            assert e.code == -1 and (mode in (engine.EXEC_WORKGROUP, engine.EXEC_PIPELINE) or (mode == engine.EXEC_WAVE and nq > 4096))
            assert not (mode == engine.EXEC_WORKGROUP and nq > 1024)          # the q-split kernel takes every wide shape
            continue
        ran += 1
        if nq > 1024 and mode in (engine.EXEC_WORKGROUP, engine.EXEC_AUTO):
            info = engine.Plan(m.setup(), q, I, sig, st).info
            assert info["exec_mode"] == "workgroup" and info["q_per_lane"] * 64 * info["waves_per_chain"] >= nq
        for r in range(reps):
            assert res.num_iter[r] == ref[r].num_iter and res.num_moves[r] == ref[r].num_moves
            np.testing.assert_allclose(res.contribs[:, :, r], ref[r].rset, rtol=1e-12)
            np.testing.assert_allclose(res.chisq[r], ref[r].conval, rtol=1e-7)
            np.testing.assert_allclose(res.fit[:, r], ref[r].fit, rtol=1e-7)
    assert ran >= 2                                    # auto always runs, and wavefront or q-split workgroup mode


@pytest.mark.parametrize("case", ["si_units", "huge_counts", "tiny_volumes"])
def test_extreme_unit_scalings_all_modes_agree_with_oracle(case):
    """The decision of a step compares products of fit sums (num² den' > num'² den): their exponent range is what the data's and the
    model's units make it.  Intensities in SI-like units (1e-30), detector counts of 1e+40 with matching uncertainties, and
    sub-nanometre spheres with compensationExponent 1 (volume^2 weights of 1e-59) under large uncertainties: every execution mode
    still takes the oracle's decisions — nothing underflows to "0 > 0 is never accepted"."""
    q, I, sig = _synthetic(100)
    lo, hi, comp = np.pi / q.max(), np.pi / q.min(), 0.6666666
    if case == "si_units":
        I, sig = I * 1e-30, sig * 1e-30
    elif case == "huge_counts":
        I, sig = I * 1e40, sig * 1e40
    else:
        q = q * 10.0; lo, hi, comp = 1e-10, 1e-9, 1.0
        sig = sig * 1e6
    m, spec = make_models("sphere", [lo], [hi])
    n, steps, reps = 60, 600, 3
    ost = O.Settings(n_contrib=n, n_reps=1, max_iter=steps, conv_crit=1e-9, comp_exp=comp)
    ref = [O.mc_fit(spec, q, I, sig, [I.min(), I.max()], [q.min(), q.max()], ost, O.PhiloxStream(5, r), method="closed")
           for r in range(reps)]
    assert all(r.num_moves > 20 for r in ref)
    for mode in (engine.EXEC_WAVE, engine.EXEC_WORKGROUP, engine.EXEC_PIPELINE):
        st = engine.Settings(n_contrib=n, n_reps=reps, max_iter=steps, conv_crit=1e-9, max_retries=0, seed=5, exec_mode=mode, comp_exp=comp)
        res = engine.analyse(m.setup(), q, I, sig, st)
        for r in range(reps):
            assert res.num_iter[r] == ref[r].num_iter and res.num_moves[r] == ref[r].num_moves, (mode, r)
            np.testing.assert_allclose(res.contribs[:, :, r], ref[r].rset, rtol=1e-12)
            np.testing.assert_allclose(res.chisq[r], ref[r].conval, rtol=1e-7)


@pytest.mark.parametrize("mode", [engine.EXEC_WAVE, engine.EXEC_WORKGROUP, engine.EXEC_PIPELINE])
def test_stop_word_is_honoured_in_every_mode(mode):
    import ctypes
    g = load("g4_sphere_q100_fixed.npz")
    m, _ = make_models("sphere", g["spec_lo"], g["spec_hi"])
    stop = ctypes.c_int32(1)
    st = engine.Settings(n_contrib=100, n_reps=3, max_iter=10**9, conv_crit=0.0, max_retries=3, seed=1, exec_mode=mode)
    res = engine.analyse(m.setup(), g["data_q"], g["data_I"], g["data_sigma"], st, stop=stop)
    assert (res.converged == 0).all() and (res.attempts == 1).all()
    assert (res.num_iter < 10**6).all()               # left at the first poll, not after the budget


@pytest.mark.parametrize("mode", [engine.EXEC_PIPELINE, engine.EXEC_WAVE])
def test_stop_word_set_while_chains_with_an_integral_are_running(mode):
    """McSAS.stop (mcsas.py:357) raised from another thread 30 ms into a run of cylinder chains with a budget of 1e6 steps (a few
    seconds of work at most, so a stop that is not seen still ends): the row-queue pipeline forwards the word with the next ticks,
    the wavefront kernel reads it through its relay — every chain leaves early, not converged, without another attempt."""
    import ctypes, threading, time
    q, I, sig = _synthetic(128)
    m, _ = make_models("cyl_aspect", *RANDOM_RANGES["cyl_aspect"], intDiv=20.)
    budget = 10**6
    warm = engine.Settings(n_contrib=64, n_reps=6, max_iter=64, conv_crit=0.0, max_retries=0, seed=3, exec_mode=mode)
    engine.analyse(m.setup(), q, I, sig, warm)                # (library, plan memory and kernels warm: the timer below is about the run)
    stop = ctypes.c_int32(0)
    st = engine.Settings(n_contrib=64, n_reps=6, max_iter=budget, conv_crit=0.0, max_retries=2, seed=3, exec_mode=mode)
    timer = threading.Timer(0.03, lambda: setattr(stop, "value", 1))
    t0 = time.perf_counter()
    timer.start()
    res = engine.analyse(m.setup(), q, I, sig, st, stop=stop)
    wall = time.perf_counter() - t0
    timer.cancel()
    assert (res.num_iter < budget).all() and (res.num_iter > 0).all(), (res.num_iter, wall)
    assert (res.converged == 0).all() and (res.attempts == 1).all()          # (stopped: no retry, mcsas.py:240-245)


def test_many_reps_in_pipeline_and_replay_overflow_reporting():
    g = load("g4_sphere_q100_fixed.npz")
    m, _ = make_models("sphere", g["spec_lo"], g["spec_hi"])
    st = engine.Settings(n_contrib=64, n_reps=300, max_iter=200, conv_crit=0.0, max_retries=0, seed=3,
                         exec_mode=engine.EXEC_PIPELINE)
    a = engine.analyse(m.setup(), g["data_q"], g["data_I"], g["data_sigma"], st)
    st.exec_mode = engine.EXEC_WAVE
    b = engine.analyse(m.setup(), g["data_q"], g["data_I"], g["data_sigma"], st)
    np.testing.assert_array_equal(a.contribs, b.contribs)
    np.testing.assert_array_equal(a.num_moves, b.num_moves)
    for mode in (engine.EXEC_WORKGROUP, engine.EXEC_PIPELINE):
        st2 = engine.Settings(n_contrib=100, n_reps=1, max_iter=50, conv_crit=0.0, max_retries=0, exec_mode=mode)
        with pytest.raises(mcsas_amd._lib.McSASHipError) as e:
            engine.analyse(m.setup(), g["data_q"], g["data_I"], g["data_sigma"], st2, replay=g["stream"][None, :120])
        assert e.value.code == -5


# ----------------------------------------------------------------------------- beam-profile smearing (§8 f3)
@pytest.mark.parametrize("tag,kind,two_d", SMEAR_CASES)
def test_smeared_intensities_vs_reference(tag, kind, two_d):
    """2 trapz(F(locs)^2 w weights, x = qOffset) (sasmodel.py:56-73) evaluated by the kernels against the
    reference's values for Sphere and LMADenseSphere; a model without canSmear ignores the configuration."""
    g = load("g7_smearing.npz"); pre = tag + "_"
    q = g[pre + "q"]
    widths = {k: float(g[pre + k]) for k in ("umbra", "penumbra", "variance") if pre + k in g}
    d, args = product_smearing(kind, two_d, int(g[pre + "n_steps"]), q, **widths)
    m, _ = make_models("sphere", [1e-10], [1e-6])
    cum, v, w, s, rows = engine.model_calc(m.setup(), q, g[pre + "sphere_radii"][:, None], 0.6666666, want_rows=True, smear=args)
    np.testing.assert_allclose(rows, g[pre + "sphere_it"], rtol=1e-9)
    md = m.calc(d, g[pre + "sphere_pset"], 0.6666666)            # the plugin-API call, smearing taken from data.config
    np.testing.assert_allclose(md.cumInt, g[pre + "sphere_cum"], rtol=1e-9)
    mf, sld = g[pre + "lma_fixed"]
    ml, _ = make_models("lmasphere", [1e-10, 0.001], [1e-6, 0.9], mf=float(mf), sld=float(sld))
    rows = engine.model_calc(ml.setup(), q, g[pre + "lma_params"], 0.6666666, want_rows=True, smear=args)[4]
    # LMA: the reference's structure-factor expression cancels catastrophically at small q*R (see
    # test_model_calc_vs_reference_vectors); pinhole offsets put evaluation points next to q = 0, where
    # the last ulp of sin/cos decides the 4th digit of single terms of the integrand
    rel = np.abs(rows / g[pre + "lma_it"] - 1.)
    assert np.median(rel) < 1e-9 and rel.max() < (2e-3 if two_d else 1e-6)
    mg, gspec = make_models("gausschain")
    row = np.array([[gspec.values[i] for i in gspec.active]])
    rows = engine.model_calc(mg.setup(), q, row, 0.6666666, want_rows=True, smear=args)[4]
    np.testing.assert_allclose(rows[0], g[pre + "gauss_chain_it"], rtol=1e-9)


@pytest.mark.parametrize("cache,waves", [(1, 1), (0, 1), (1, 8), (1, -3)])
def test_smeared_trajectory_vs_reference(cache, waves):
    g, m, spec, st, ost = traj_setup("g7_sphere_q100_smeared.npz")
    _, psm = traj_smearing(g)
    st.cache_intensities = cache
    if waves == -3:
        st.exec_mode, st.waves_per_chain = engine.EXEC_PIPELINE, 0
    else:
        st.waves_per_chain = waves
    res = engine.analyse(m.setup(FakeData(g["data_q"])), g["data_q"], g["data_I"], g["data_sigma"], st,
                         replay=g["stream"][None, :], smear=psm)
    assert res.num_iter[0] == int(g["res_num_iter"])
    assert res.num_moves[0] == int(g["res_num_moves"])
    np.testing.assert_allclose(res.contribs[:, :, 0], g["res_rset"], rtol=1e-12)
    np.testing.assert_allclose(res.chisq[0], float(g["res_conval"]), rtol=1e-7)
    np.testing.assert_allclose(res.fit[:, 0], g["res_fit"], rtol=1e-6)


def test_mcsas_mirror_with_smearing_matches_oracle():
    """McSAS.calc() end to end (analyse + histogram) on slit-smeared data configured through
    data.config.smearing, free-running Philox chains, against the oracle with the same streams."""
    g = load("g7_smearing.npz"); pre = "trapz_slit_"
    q = g[pre + "q"]
    widths = dict(umbra=float(g[pre + "umbra"]), penumbra=float(g[pre + "penumbra"]))
    osm = oracle_smearing("trapezoid", False, 25, q, **widths)
    ospec = O.ModelSpec.make("sphere", ["radius"], [np.pi / q.max()], [np.pi / q.min()]); ospec.smear = osm
    rs = np.random.RandomState(3)
    truth = rs.uniform(5e-9, 6e-8, 40)[:, None]
    I = O.model_calc(ospec, q, truth, 0.6666666)[0]
    sig = 0.02 * I
    I = I * (1 + 0.02 * rs.standard_normal(len(q)))
    d, _ = product_smearing("trapezoid", False, 25, q, I, sig, **widths)
    m = mcsas_amd.Sphere(); m.radius.setActiveRange((np.pi / q.max(), np.pi / q.min()))
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, np.pi / q.max(), np.pi / q.min(), binCount=10, xscale='log', yweight='vol'))
    st = engine.Settings(n_contrib=80, n_reps=3, max_iter=1500, conv_crit=1e-9, max_retries=0, seed=77)
    res = engine.analyse(m.setup(d), q, I, sig, st, smear=d.smearArgs(m))
    ost = O.Settings(n_contrib=80, n_reps=3, max_iter=1500, conv_crit=1e-9, max_retries=0)
    for r in range(3):
        ref = O.mc_fit(ospec, q, I, sig, d.f.limit, d.x0.limit, ost, O.PhiloxStream(77, r), method="closed")
        assert res.num_moves[r] == ref.num_moves
        np.testing.assert_allclose(res.contribs[:, :, r], ref.rset, rtol=1e-12)
        np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-7)
    # the algorithm object picks the configuration up from data.config by itself (maxRetries >= 1 there,
    # mcsasparameters.json: compare with the library called with the same settings)
    algo = mcsas_amd.McSAS(seed=77)
    algo.numContribs.setValue(80); algo.numReps.setValue(3); algo.maxIterations.setValue(1500)
    algo.convergenceCriterion.setValue(1e-9); algo.maxRetries.setValue(1); algo.showIncomplete.setValue(True)
    algo.model, algo.data = m, d
    algo.calc()
    st.max_retries = 1
    res1 = engine.analyse(m.setup(d), q, I, sig, st, smear=d.smearArgs(m))
    np.testing.assert_array_equal(algo.result[0]["contribs"], res1.contribs)
    unsmeared = engine.analyse(m.setup(d), q, I, sig, st)
    assert not np.array_equal(unsmeared.contribs, res1.contribs)
    # histogram(): fractions and observability from smeared model intensities (mcsas.py:549-604)
    h = m.radius.histograms()[0]
    fr, _ = O.fractions(ospec, q, I, sig, d.f.limit, ost, res1.contribs, method="closed")
    np.testing.assert_allclose(algo.fractions["vol"][0], fr["vol"][0], rtol=1e-6)
    np.testing.assert_allclose(algo.fractions["vol"][1], fr["vol"][1], rtol=1e-6)
    assert np.isfinite(h.bins.mean).all() and np.isfinite(h.observability).all()


# ----------------------------------------------------------------------------- input preparation (§8 f4)
@pytest.mark.parametrize("tag", ["demo", "dense"])
def test_uncertainty_floor_and_rebin_vs_reference(tag):
    """mcsas_hip_prepare_uncertainty / mcsas_hip_rebin against the reference's DataObj._prepareUncertainty /
    _reBin outputs.  Bin membership, single-point bins and the floor are exact; means and standard errors
    are sums in a different order than numpy's pairwise ones: 1e-13."""
    g = load("g8_input_prep.npz")
    fu = engine.prepare_uncertainty(g[tag + "_raw_f"], g[tag + "_raw_fu"], float(g[tag + "_fu_min"]))
    np.testing.assert_array_equal(fu, g[tag + "_si_fu"])
    np.testing.assert_array_equal(engine.prepare_uncertainty(g[tag + "_raw_f"], None, 0.05), 0.05 * g[tag + "_raw_f"])
    xb, fb, ub = engine.rebin(g[tag + "_san_x"], g[tag + "_san_f"], g[tag + "_san_fu"], int(g[tag + "_nbin"]))
    assert len(xb) == len(g[tag + "_bin_x"])
    np.testing.assert_allclose(xb, g[tag + "_bin_x"], rtol=1e-13)
    np.testing.assert_allclose(fb, g[tag + "_bin_f"], rtol=1e-13)
    fin = np.isfinite(g[tag + "_bin_fu"])
    np.testing.assert_array_equal(np.isfinite(ub), fin)
    np.testing.assert_allclose(ub[fin], g[tag + "_bin_fu"][fin], rtol=1e-12)
    single = np.array([np.sum((g[tag + "_san_x"] == v)) == 1 for v in xb])      # bins of one point are copies
    np.testing.assert_array_equal(xb[single], g[tag + "_bin_x"][single])


def test_fromraw_and_series_driver():
    """SASData.fromRaw (floor + mask + rebin on the GPU) feeding McSAS through run_series: every data set of
    the series gets its own result and one entry per histogram in the series table (gui/calc.py:331-349)."""
    g = load("g8_input_prep.npz")
    d = mcsas_amd.SASData.fromRaw(g["dense_san_x"], g["dense_san_f"], g["dense_san_fu"], nBin=60, fuMin=0.0)
    np.testing.assert_allclose(d.q, g["dense_bin_x"], rtol=1e-13)
    np.testing.assert_allclose(d.f.binnedData, g["dense_bin_f"], rtol=1e-13)
    assert d.f.limit == [float(g["dense_san_f"].min()), float(g["dense_san_f"].max())]
    q = np.logspace(7.3, 9.2, 300)
    datasets = []
    for radius in (1.0e-8, 2.5e-8):
        _, spec = make_models("sphere", [1e-10], [1e-6])
        I = O.calc_intensity(spec, q, [radius], 0.6666666)[0]
        I = I / I.max() + 1e-3                                  # the curve two decades above a flat background
        datasets.append(mcsas_amd.SASData.fromRaw(q, I, None, nBin=50, fuMin=0.02))
    rel = datasets[0].f.binnedDataU / datasets[0].f.binnedData      # the 2 % floor where the curve is smooth, the bin's own scatter
    assert datasets[0].count <= 50 and np.allclose(rel[:10], 0.02, rtol=0.05) and (rel > 0.015).all()   # where it oscillates
    m = mcsas_amd.Sphere(); m.radius.setActiveRange((2e-9, 1e-7))
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, 2e-9, 1e-7, binCount=12, xscale='log', yweight='vol'))
    algo = mcsas_amd.McSAS(seed=5)
    algo.numContribs.setValue(60); algo.numReps.setValue(4); algo.maxIterations.setValue(4000)
    algo.convergenceCriterion.setValue(50.0); algo.showIncomplete.setValue(True)
    algo.model = m
    results, series = mcsas_amd.run_series(algo, datasets, keys=[10.0, 25.0])
    assert len(results) == 2 and all(r is not None for r in results)
    (uid, rows), = series.items()
    assert uid == ("radius", 2e-9, 1e-7, "vol") and [k for k, _ in rows] == [10.0, 25.0]
    means = [fields[2] for _, fields in rows]                 # Moments.fields: (total, totalStd, mean, ...)
    # (a curve that drowns in the background converges at the initial set and both series entries come out identical: the
    # data sets must really be fitted) — the volume-weighted mean radius tracks the sphere radius of each data set
    assert all(r["numIter"] > 100 for r in results)
    assert 0.7e-8 < means[0] < 1.5e-8 and 2.0e-8 < means[1] < 3.2e-8, means


def test_kholodenko_regimes_vs_quadpack():
    """The worm-like chain form factor across its regimes against the oracle's QUADPACK evaluation
    (models/kholodenko.py:32-49, epsrel 1e-10): contour shorter than the closed-form split (x < 2), x of
    a few hundred, q l_k/3 far below, around (panel fallback, |e| < 0.05) and far above 1."""
    rs = np.random.RandomState(9)
    m, spec = make_models("kholodenko", [1e-10, 1e-9, 1e-9], [1e-7, 1e-6, 1e-4])
    for lk, lc in ((2e-8, 1e-8), (3e-8, 2.5e-8), (1e-8, 6e-8), (2e-8, 1.5e-6), (5e-8, 4e-7)):
        ratio = 3.0 / lk
        q = np.sort(np.concatenate([ratio * 10 ** rs.uniform(-2.5, 1.7, 24), ratio * (1 + rs.uniform(-2e-3, 2e-3, 6)),
                                    [ratio, ratio * (1 - 1e-9), ratio * (1 + 1e-9)]]))
        row = np.array([[2e-9, lk, lc]])
        ref = O.calc_intensity(spec, q, row[0], 0.6666666)[0]
        got = engine.model_calc(m.setup(), q, row, 0.6666666, want_rows=True)[4][0]
        np.testing.assert_allclose(got, ref, rtol=2e-9)


def test_kholodenko_active_ranges_vs_quadpack_500_sets():
    """The worm-like chain form factor over the model's whole preset active range (models/kholodenko.py:57-71: radius 1-5 nm,
    Kuhn length 10-50 nm, contour length 100-1000 nm; the box's corners and edges included) against the oracle's QUADPACK
    evaluation (models/kholodenko.py:32-49, epsrel 1e-10): 500 seeded parameter sets x 32 q on the q range of the reference's
    worm data file, relative difference <= 2e-9 everywhere."""
    rs = np.random.RandomState(2025)
    lo, hi = np.array([1e-9, 1e-8, 1e-7]), np.array([5e-9, 5e-8, 1e-6])
    sets = lo + (hi - lo) * rs.uniform(size=(500, 3))
    corners = np.array([[(lo, hi)[(c >> k) & 1][k] for k in range(3)] for c in range(8)])
    sets[:8] = corners
    for k in range(3):                                        # edge mid-points: one coordinate free, the others at a bound
        for c in range(4):
            e = np.array([(lo, hi)[(c >> j) & 1][(k + 1 + j) % 3] for j in range(2)])
            row = np.empty(3); row[k] = 0.5 * (lo[k] + hi[k]); row[(k + 1) % 3] = e[0]; row[(k + 2) % 3] = e[1]
            sets[8 + 4 * k + c] = row
    m, spec = make_models("kholodenko", lo, hi)
    g = load("g9_kho_q512.npz")
    qlo, qhi = g["data_q"].min(), g["data_q"].max()
    beyond = []
    for i in range(0, 500, 50):
        q = np.sort(qlo * (qhi / qlo) ** rs.uniform(size=32))
        got = engine.model_calc(m.setup(), q, sets[i:i + 50], 0.6666666, want_rows=True)[4]
        for j in range(50):
            ref = O.calc_intensity(spec, q, sets[i + j], 0.6666666)[0]
            rel = np.abs(got[j] / ref - 1)
            np.testing.assert_allclose(got[j], ref, rtol=2e-8, err_msg="set %d %r" % (i + j, sets[i + j]))
            beyond += [(i + j, float(q[k]), float(got[j][k])) for k in np.nonzero(rel > 2e-9)[0]]
    # QUADPACK at epsrel 1e-10 is itself off by a few 1e-9 at a handful of the 16 000 points (deep in the oscillating tail,
    # five decades below the forward intensity; first seen at set 140, q = 6.24e9 1/m: +2.66e-9).  Every point where the
    # two disagree by more than 2e-9 is settled against a 30-digit evaluation of the same integral: the kernel is the one
    # that is right, to 1e-10.
    assert len(beyond) <= 16, len(beyond)
    for idx, qq, val in beyond:
        np.testing.assert_allclose(val, _kholodenko_mp(qq, sets[idx], 0.6666666), rtol=1e-10, err_msg="set %d q %g" % (idx, qq))


def _kholodenko_mp(q, row, comp_exp):
    """models/kholodenko.py:16-94 in 30-digit arithmetic (mpmath): intensity F^2 V^(2c) of one worm at one q."""
    import mpmath as mp
    mp.mp.dps = 30
    r, lk, lc = [mp.mpf(float(v)) for v in row]
    q = mp.mpf(float(q))
    x = 3 * lc / lk
    if q > 3 / lk:
        F = mp.sqrt(q * q * lk * lk / 9 - 1)
        f = lambda z: mp.sin(F * z) / (F * mp.sinh(z)) if z != 0 else mp.mpf(1)
    else:
        e = mp.sqrt(1 - q * q * lk * lk / 9)
        f = (lambda z: mp.sinh(e * z) / (e * mp.sinh(z)) if z != 0 else mp.mpf(1)) if e != 0 else (lambda z: z / mp.sinh(z) if z != 0 else mp.mpf(1))
    pts = sorted(set([mp.mpf(0)] + [mp.mpf(k) for k in (1, 2, 4, 8, 16, 32, 64, 128) if k < x] + [x]))
    p0 = mp.quad(lambda z: f(z) * (2 / x) * (1 - z / x), pts, maxdegree=10)
    u = q * r
    pcs = 2 * mp.besselj(1, u) / u
    vol = mp.pi * lc * r * r
    return float(p0 * pcs * pcs * vol ** (2 * mp.mpf(comp_exp)))


def test_cylinders_at_the_ends_of_the_aspect_range():
    """Isotropic cylinders at aspect 1e-3 and 1e3, the ends of the parameter's value range (models/cylindersisotropic.py:31-36),
    and radii from 0.1 nm (its lower bound) to 100 nm: needles and discs against the oracle's trapezoid over scipy's j1."""
    m, spec = make_models("cyl_aspect", [1e-10, 1e-3], [1e-7, 1e3])
    q = np.logspace(7, np.log10(3e9), 48)
    rows = np.array([[r, asp] for r in (1e-10, 1e-9, 7.3e-9, 4e-8, 1e-7) for asp in (1e-3, 3.3e-2, 1.0, 47.0, 1e3)])
    got = engine.model_calc(m.setup(FakeData(q)), q, rows, 0.6666666, want_rows=True)[4]
    for j, row in enumerate(rows):
        ref = O.calc_intensity(spec, q, row, 0.6666666)[0]
        np.testing.assert_allclose(got[j], ref, rtol=1e-9, atol=1e-14 * ref.max(), err_msg=repr(row))


def test_lazy_rows_equal_eager_rows_over_a_long_free_run():
    """The lazy row cache's premise — a contribution row evaluated again for the cache (one q per thread, intensity_fast)
    has the bits of the row evaluated as a proposal (eight q per lane interleaved, intensity_fast_n) — over a long
    free-running run at config 2's shape: 50 repetitions x 20 000 steps with the device's Philox stream, default (lazy) on
    the release library against the eager variant of the measurement build (every `new` row stored, row slots swapped on
    acceptance; same Gram grouping, so the two must agree to the last bit), and against equal row shares of a SIMD's two
    producer waves (arithmetic does not depend on which wave evaluates a row)."""
    from bench import synthetic_data
    q, I, sig = synthetic_data(512)
    m = mcsas_amd.Sphere(); m.radius.setActiveRange((np.pi / q.max(), np.pi / q.min()))
    runs = []
    for flags in (0, 1 << 16, 3 << 19):
        st = engine.Settings(n_contrib=400, n_reps=50, max_iter=20000, conv_crit=0.0, max_retries=0, seed=99,
                             exec_mode=engine.EXEC_PIPELINE, debug_flags=flags)
        runs.append(engine.analyse(m.setup(), q, I, sig, st))
    assert runs[0].num_moves.min() > 800
    for other in runs[1:]:
        np.testing.assert_array_equal(other.contribs, runs[0].contribs)
        np.testing.assert_array_equal(other.num_moves, runs[0].num_moves)
        np.testing.assert_array_equal(other.chisq, runs[0].chisq)
        np.testing.assert_array_equal(other.fit, runs[0].fit)



RANDOM_RANGES = {   # generator ranges per model tag (SI)
    "sphere": ([2e-9], [3e-7]), "cyl_aspect": ([1e-9, 0.5], [1e-7, 20.0]), "cyl_length": ([1e-9, 5e-9], [1e-7, 5e-7]),
    "ellcs": ([1e-9, 2e-9, 2e-10], [1e-7, 2e-7, 1e-8]), "kholodenko": ([1e-9, 1e-8, 1e-7], [5e-9, 5e-8, 1e-6]),
    "elliso": ([1e-9, 0.3], [1e-7, 8.0]), "sphcs": ([1e-9, 5e-10], [1e-7, 2e-8]), "gausschain": ([1e-9, 1e-9], [1e-7, 1e-7]),
    "lmasphere": ([2e-9, 0.01], [2e-7, 0.4]),
}


@pytest.mark.parametrize("case", range(18))
def test_random_configurations_all_modes_identical(case):
    """Seeded sweep over model, q count, contribution count, repetitions, step budget, convergence criterion,
    retries and the three fit flags: the execution modes that accept a configuration walk identical chains
    (parameter sets, iteration / move / draw / attempt counts: exact); the chi², scale, background and fit
    reported at the end are re-summed once per mode in its own lane order: 1e-12."""
    rs = np.random.RandomState(1000 + case)
    tag = list(RANDOM_RANGES)[case % len(RANDOM_RANGES)]
    heavy = tag in ("cyl_aspect", "cyl_length", "ellcs", "kholodenko", "elliso")
    nq = int(rs.choice([5, 33, 64, 100, 257] if heavy else [5, 33, 64, 100, 257, 512, 700]))
    n = int(rs.choice([16, 24, 50, 130] if heavy else [16, 24, 50, 130, 300, 400]))
    reps = int(rs.randint(1, 5))
    steps = int(rs.randint(1, 4 * n))
    lo, hi = RANDOM_RANGES[tag]
    m, spec = make_models(tag, lo, hi)
    q = np.sort(10 ** rs.uniform(7.2, 9.3, nq))
    truth = np.array([10 ** rs.uniform(np.log10(a), np.log10(b), 12) for a, b in zip(lo, hi)]).T
    I = O.model_calc(spec, q, truth, 0.6666666)[0]
    I = I * (1 + 0.03 * rs.standard_normal(nq)) + 0.02 * I.mean()
    sig = 0.03 * np.abs(I) + 1e-3 * np.abs(I).mean()
    kw = dict(find_background=bool(rs.randint(2)), positive_background=bool(rs.randint(2)),
              start_from_minimum=bool(rs.randint(4) == 0), max_retries=int(rs.randint(0, 3)),
              conv_crit=float(rs.choice([1e-9, 5.0, 200.0])))
    outs = []
    for mode in (engine.EXEC_WAVE, engine.EXEC_WORKGROUP, engine.EXEC_PIPELINE):
        st = engine.Settings(n_contrib=n, n_reps=reps, max_iter=steps, seed=77 + case, exec_mode=mode, **kw)
        try:
            outs.append((mode, engine.analyse(m.setup(FakeData(q)), q, I, sig, st)))
        except mcsas_amd._lib.McSASHipError as e:
            assert e.code == -1 and mode != engine.EXEC_WAVE
    assert len(outs) >= 2
    ref = outs[0][1]
    assert np.isfinite(ref.chisq).all() and (ref.num_iter <= steps).all()
    for mode, res in outs[1:]:
        for f in ("contribs", "num_iter", "num_moves", "attempts", "converged", "draws"):
            np.testing.assert_array_equal(getattr(res, f), getattr(ref, f), err_msg="%s differs in mode %d (%s nq=%d n=%d)" % (f, mode, tag, nq, n))
        for f in ("chisq", "scaling", "fit"):
            np.testing.assert_allclose(getattr(res, f), getattr(ref, f), rtol=1e-12, err_msg="%s differs in mode %d (%s nq=%d n=%d)" % (f, mode, tag, nq, n))
        np.testing.assert_allclose(res.background, ref.background, rtol=1e-9, atol=1e-12 * np.abs(I).max())


def test_histogram_prep_equals_the_per_call_entry_points():
    """mcsas_hip_histogram_prep (all repetitions in one call) against model_calc + bgfit + observability
    called per repetition, and against the oracle's fractions (mcsas.py:549-594)."""
    g = load("g45_analyse.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    lo, hi = float(g["A_lo"]), float(g["A_hi"])
    m, spec = make_models("sphere", [lo], [hi])
    contribs = g["A_contribs"]
    N, P, R = contribs.shape
    sc, v, w, s, mv = engine.histogram_prep(m.setup(), q, I, sig, contribs, 0.6666666)
    for r in range(R):
        cum, v1, w1, s1 = engine.model_calc(m.setup(), q, contribs[:, :, r], 0.6666666)
        sc1, _, _ = engine.bgfit(I, sig, cum, True, False, 1)
        np.testing.assert_allclose(sc[:, r], sc1, rtol=1e-12)
        np.testing.assert_array_equal(v[:, r], v1); np.testing.assert_array_equal(w[:, r], w1); np.testing.assert_array_equal(s[:, r], s1)
    vf = w * sc[0][None, :] / v
    mv1 = engine.observability(m.setup(), q, sig, contribs, sc[0], vf, 0.6666666)
    np.testing.assert_allclose(mv, mv1, rtol=1e-9)
    ost = O.Settings(n_contrib=N, n_reps=R, max_iter=1, conv_crit=5.0)
    frac, oscal = O.fractions(spec, q, I, sig, g["data_f_limit"], ost, contribs, method="closed")
    np.testing.assert_allclose(sc, oscal, rtol=1e-7)
    np.testing.assert_allclose(vf, frac["vol"][0], rtol=1e-7)
    np.testing.assert_allclose(mv, frac["vol"][1], rtol=1e-7)


@pytest.mark.parametrize("tag", ["sphere", "cyl_aspect", "ellcs"])
def test_device_histogram_equals_the_two_step_host_path(tag):
    """mcsas_hip_histogram (fractions, bins, CDF, observability, moments of every repetition on the device, ordered sums) against
    mcsas_hip_histogram_prep + the numpy half of McSAS.histogram(): the same numbers, bit for bit, for every weighting, linear and
    logarithmic bins, more than 64 bins, bins nobody falls into, a range narrower than the parameter's."""
    q, I, sig = _synthetic(100)
    lo, hi = RANDOM_RANGES[tag]
    m, _ = make_models(tag, lo, hi, **({"intDiv": 20.} if tag != "sphere" else {}))
    ap = m.activeParams()
    decl = [(0, 50, 'log', 'vol', 1.0), (0, 130, 'lin', 'num', 1.0), (len(ap) - 1, 7, 'log', 'int', 0.5), (len(ap) - 1, 12, 'lin', 'surf', 1.0)]
    for pi, nb, xs, yw, shrink in decl:
        p = ap[pi]
        a, b = p.activeRange()
        p.histograms().append(mcsas_amd.Histogram(p, a, a + shrink * (b - a), binCount=nb, xscale=xs, yweight=yw, autoFollow=False))
    algo = mcsas_amd.McSAS(seed=3)
    algo.numContribs.setValue(90); algo.numReps.setValue(7); algo.maxIterations.setValue(600); algo.convergenceCriterion.setValue(1e-9)
    algo.showIncomplete.setValue(True); algo.model = m
    algo.data = mcsas_amd.SASData(q, I, sig)
    algo.result = []; algo.stop = False
    algo.analyse()

    def snapshot():
        out = []
        for p in ap:
            for h in p.histograms():
                out.append(dict(bins=np.array(h.bins.full), bm=np.array(h.bins.mean), bs=np.array(h.bins.std), cdf=np.array(h.cdf.full),
                                obs=np.array(h.observability), mom=np.array(h.moments.fields, dtype=float), edges=np.array(h.xLowerEdge)))
        fr = {k: (np.array(v[0]), np.array(v[1])) for k, v in algo.fractions.items()}
        return out, fr, np.array(algo.result[0]['scalingFactors'])

    algo.histogram()
    dev, dfr, dsc = snapshot()
    cap = engine.HISTOGRAM_MAX_CONTRIBS
    engine.HISTOGRAM_MAX_CONTRIBS = 0                          # force the two-step path
    try:
        algo.histogram()
    finally:
        engine.HISTOGRAM_MAX_CONTRIBS = cap
    host, hfr, hsc = snapshot()
    np.testing.assert_array_equal(dsc, hsc)
    for k in hfr:
        np.testing.assert_array_equal(dfr[k][0], hfr[k][0], err_msg=k)
        np.testing.assert_array_equal(dfr[k][1], hfr[k][1], err_msg=k)
    assert len(dev) == 4
    for d, h in zip(dev, host):
        for k in d:
            np.testing.assert_array_equal(d[k], h[k], err_msg=k)
    assert sum(d["bins"].sum() > 0 for d in dev) >= 3          # (the surface weighting of a model without surface() is all zero)


def test_auto_mode_for_rows_with_an_integral():
    """MCSAS_EXEC_AUTO for models whose rows cost an integral (round 4 sweep, tools/sweep_heavy_modes2.sh, profiles/r04_heavy_modes.txt):
    the pipeline at every chain count — BASELINE's totals of configs 3 and 4 on one GPU (200 / 400 chains) included; where its
    geometry does not fit (fewer than 16 contributions; nor does the workgroup mode's then) one wavefront per chain."""
    q, I, sig = _synthetic(128)
    m, _ = make_models("cyl_aspect", *RANDOM_RANGES["cyl_aspect"], intDiv=20.)
    for ncontrib, reps, want in ((64, 13, "pipeline"), (64, 200, "pipeline"), (64, 400, "pipeline"), (64, 2048, "pipeline"),
                                 (12, 13, "wave"), (12, 2048, "wave")):
        st = engine.Settings(n_contrib=ncontrib, n_reps=reps, max_iter=50, conv_crit=0.0, max_retries=0, seed=1)
        plan = engine.Plan(m.setup(), q, I, sig, st)
        if engine.device_count() and plan.info["exec_mode"] != want:
            import torch
            assert torch.cuda.get_device_properties(0).multi_processor_count != 256, (ncontrib, reps, plan.info)   # (thresholds scale with the CU count)
        plan.close()


def test_auto_mode_never_picks_a_mode_whose_working_set_does_not_fit():
    """MCSAS_EXEC_AUTO: 9000 chains of config 4's shape (1000 contributions x 1024 q) would need 147 GB of row
    cache plus window buffers in pipeline mode — more than half of the free memory — so AUTO runs them one wavefront per chain
    (which needs no window buffers and can do without its cache), the way it did before the row queue; the pipeline asked for BY NAME is still refused with MCSAS_ENOMEM."""
    try:                                                        # (sized for the MI355X's 288 GB; torch is only asked, never needed)
        import torch
        if torch.cuda.mem_get_info(0)[0] > 290e9:
            pytest.skip("device with more memory than the case is sized for")
    except RuntimeError:
        pass
    q, I, sig = _synthetic(1024)
    m, _ = make_models("ellcs", [1e-9, 2e-9, 2e-10], [1e-7, 2e-7, 1e-8])
    st = engine.Settings(n_contrib=1000, n_reps=9000, max_iter=10, conv_crit=0.0, max_retries=0, seed=1)
    plan = engine.Plan(m.setup(), q, I, sig, st)
    assert plan.info["exec_mode"] == "wave", plan.info         # (its own 74 GB row cache is optional: kept when half the free memory holds it)
    plan.close()
    with pytest.raises(_lib.McSASHipError) as e:
        engine.Plan(m.setup(), q, I, sig, engine.Settings(**{**st.__dict__, "exec_mode": engine.EXEC_PIPELINE}))
    assert e.value.code == -4                                   # MCSAS_ENOMEM
    engine.release_cached_memory()


def test_uncertainty_floor_special_values():
    """_prepareUncertainty's corner cases (dataobj/dataobj.py:204-227): the floor wins over smaller and over
    zero uncertainties, non-finite results become +inf, negative intensities give a negative floor that the
    given uncertainty beats."""
    I = np.array([10.0, 10.0, 10.0, -4.0, 5.0, np.inf, 2.0])
    su = np.array([0.01, 5.0, 0.0, 0.3, np.nan, 1.0, np.inf])
    got = engine.prepare_uncertainty(I, su, 0.1)
    ref = O.prepare_uncertainty(I, su, 0.1)
    np.testing.assert_array_equal(got, ref)
    assert got[0] == 1.0 and got[1] == 5.0 and got[2] == 1.0 and got[3] == 0.3 and np.isinf(got[4:]).all()


# ----------------------------------------------------------------------------- round 2: row edges
@pytest.mark.parametrize("mode", [engine.EXEC_WAVE, engine.EXEC_WORKGROUP, engine.EXEC_PIPELINE])
def test_exponential2_and_3_generators_on_device(mode):
    """RandomExponential2 / RandomExponential3 (numbergenerator.py:181-189) through the device-side gen_transform:
    (1) the initial parameter set drawn from a replayed uniform stream equals the reference's own transform of the
    same uniforms (g6_generators.npz) scaled into the active range; (2) free-running chains with those generators
    follow the oracle."""
    g = load("g6_generators.npz")
    u = g["u"]
    lo, hi = [2e-9, 3e-9], [9e-8, 4e-7]
    m, spec = make_models("gausschain", lo, hi, [2, 3])
    N = 32
    q, I, sig = _synthetic(100)
    st = engine.Settings(n_contrib=N, n_reps=1, max_iter=0, conv_crit=0.0, max_retries=0, exec_mode=mode)
    res = engine.analyse(m.setup(), q, I, sig, st, replay=np.concatenate([u, u])[None, :])
    want = np.stack([g["exp2"][:N] * (hi[0] - lo[0]) + lo[0], g["exp3"][N:2 * N] * (hi[1] - lo[1]) + lo[1]], axis=1)
    np.testing.assert_allclose(res.contribs[:, :, 0], want, rtol=4e-16)       # device pow against numpy's: one ulp
    assert res.num_iter[0] == 0 and res.draws[0] == 2 * N
    st = engine.Settings(n_contrib=N, n_reps=3, max_iter=150, conv_crit=1e-9, max_retries=0, seed=99, exec_mode=mode)
    res = engine.analyse(m.setup(), q, I, sig, st)
    ost = O.Settings(n_contrib=N, n_reps=1, max_iter=150, conv_crit=1e-9)
    for r in range(3):
        ref = O.mc_fit(spec, q, I, sig, [I.min(), I.max()], [q.min(), q.max()], ost, O.PhiloxStream(99, r), method="closed")
        assert res.num_moves[r] == ref.num_moves and res.num_iter[r] == ref.num_iter
        np.testing.assert_allclose(res.contribs[:, :, r], ref.rset, rtol=1e-12)
        np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-7)


def test_config5_as_named_full_size_properties():
    """BASELINE config 5 as named — the Kholodenko fit on testdata/sasfit_kho-1-10-1000.dat at 512 q x 600
    contributions — with the per-GPU share of its 100 repetitions (13): the three execution modes walk identical
    chains, chi² never increases with the budget, the reported chi² is the chi² of the reported fit, parameters stay
    inside the model's default active ranges.  (The reference's own 300-step chain on this data is replayed in
    test_replay_trajectories_vs_reference[g9_kho_q512].)"""
    from bench import kholodenko_file_data
    q, I, sig = kholodenko_file_data()
    assert len(q) == 512
    m, _ = make_models("kholodenko")
    setup = m.setup()
    prev = None
    for steps in (24, 96, 700):
        res = {}
        for mode in (engine.EXEC_PIPELINE, engine.EXEC_WAVE, engine.EXEC_WORKGROUP):
            if mode != engine.EXEC_PIPELINE and steps != 24:
                continue
            st = engine.Settings(n_contrib=600, n_reps=13, max_iter=steps, conv_crit=0.0, max_retries=0, seed=5, exec_mode=mode)
            res[mode] = engine.analyse(setup, q, I, sig, st)
        r = res[engine.EXEC_PIPELINE]
        for mode, o in res.items():
            np.testing.assert_array_equal(o.num_moves, r.num_moves)
            np.testing.assert_array_equal(o.contribs, r.contribs)
            np.testing.assert_allclose(o.chisq, r.chisq, rtol=1e-9)
        assert (r.num_iter == steps).all()
        direct = (((I[:, None] - r.fit) / sig[:, None])**2).sum(axis=0) / len(q)
        np.testing.assert_allclose(r.chisq, direct, rtol=1e-9)
        for col in range(3):
            assert (r.contribs[:, col, :] >= setup.gen_lo[col]).all() and (r.contribs[:, col, :] <= setup.gen_hi[col]).all()
        if prev is not None:
            assert (r.chisq <= prev * (1 + 1e-12)).all()
        prev = r.chisq.copy()


def test_no_active_parameter_returns_the_model_intensity():
    """mcsas.py:198-201, 238-239, 322-323: with no active fit parameter analyse() runs one repetition of one
    contribution and mcFit hands back the model intensity at the fixed parameter values (conval -1, scaling 1,
    background 0); the result dict has contribs of shape (1, 0, 1) and histogram() has nothing to do."""
    q, I, sig = _synthetic(100)
    m = mcsas_amd.Sphere()
    m.radius.setValue(2.5e-8)
    m.radius.setActive(False)
    assert m.activeParamCount() == 0
    algo = mcsas_amd.McSAS(seed=1)
    algo.model = m
    algo.data = mcsas_amd.SASData(q, I, sig)
    algo.calc()
    res = algo.result[0]
    assert res["contribs"].shape == (1, 0, 1)
    _, spec = make_models("sphere")
    want = O.calc_intensity(spec, q, [2.5e-8], algo.compensationExponent())[0]
    np.testing.assert_allclose(res["fitMeasValMean"][0], want, rtol=1e-9)
    np.testing.assert_array_equal(res["fitMeasValStd"], 0.0)
    assert res["scaling"] == (1.0, 0.0) and res["background"] == (0.0, 0.0) and res["numIter"] == 0.0
    assert algo.details.chisq[0] == -1.0
    # the library entry point with n_active = 0 directly, and a plan (which needs something to fit) refusing it
    st = engine.Settings(n_contrib=300, n_reps=10)
    r = engine.analyse(m.setup(), q, I, sig, engine.Settings(n_contrib=1, n_reps=1))
    np.testing.assert_allclose(r.fit[:, 0], want, rtol=1e-9)
    with pytest.raises(mcsas_amd._lib.McSASHipError):
        engine.Plan(m.setup(), q, I, sig, st)


def test_more_than_16384_q_points_is_refused_loudly():
    q, I, sig = _synthetic(16385)
    m, _ = make_models("sphere", [np.pi / q.max()], [np.pi / q.min()])
    st = engine.Settings(n_contrib=20, n_reps=1, max_iter=10, conv_crit=0.0, max_retries=0)
    with pytest.raises(mcsas_amd._lib.McSASHipError) as e:
        engine.analyse(m.setup(), q, I, sig, st)
    assert e.value.code == -1 and "16384" in str(e.value)


def test_pipeline_tuning_variants_replay_the_reference():
    """The pipeline's alternative layouts, selected by the tuning bits of the diagnostic word and kept for measurements,
    replay the reference's 512 q x 400 contribution chain like the default does: `new` rows stored eagerly and row slots
    swapped on acceptance instead of stale rows evaluated again (bit 16), Gram operands from HBM/L2 instead of the LDS copy
    of the sub-window (bit 18), other sub-window sizes (bits 12-15), rows per producer wave (bits 8-11) and row shares of the two waves of a SIMD (bits 19-20).  (Their Gram
    blocks are summed in different groupings, so two free-running chains may take different turns at a numerically tied
    step — replacing one negligible sphere by another moves chi² by less than its rounding error — which is why every
    variant is compared with the reference, not with the default layout.)"""
    for flags in (1 << 16, 1 << 18, (1 << 16) | (1 << 18), 2 << 12, 1 << 12, (1 << 12) | (1 << 16), 8 << 8, 4 << 8, (2 << 8) | (1 << 18), 3 << 8,
                  1 << 19, 2 << 19, (6 << 8) | (2 << 19), (2 << 12) | (6 << 8)):
        g, m, spec, st, ost = traj_setup("g4_sphere_q512_fixed.npz")
        st.exec_mode, st.debug_flags = engine.EXEC_PIPELINE, flags
        res = engine.analyse(m.setup(FakeData(g["data_q"])), g["data_q"], g["data_I"], g["data_sigma"], st, replay=g["stream"][None, :])
        assert res.num_iter[0] == int(g["res_num_iter"]) and res.num_moves[0] == int(g["res_num_moves"]), flags
        np.testing.assert_allclose(res.contribs[:, :, 0], g["res_rset"], rtol=1e-12)
        np.testing.assert_allclose(res.chisq[0], float(g["res_conval"]), rtol=1e-7)
    # the other models without an integral (their stale rows are re-evaluated too), eager and lazy, against their reference replays
    for name, flags in [(n, f) for n in ("g4_sphcs_q40.npz", "g4_gausschain_q40.npz", "g4_lmasphere_q40.npz", "g7_sphere_q100_smeared.npz") for f in (0, 1 << 16)]:
        g, m, spec, st, ost = traj_setup(name)
        _, psm = traj_smearing(g)
        st.exec_mode, st.debug_flags = engine.EXEC_PIPELINE, flags
        res = engine.analyse(m.setup(FakeData(g["data_q"])), g["data_q"], g["data_I"], g["data_sigma"], st, replay=g["stream"][None, :], smear=psm)
        assert res.num_moves[0] == int(g["res_num_moves"]), name
        np.testing.assert_allclose(res.contribs[:, :, 0], g["res_rset"], rtol=1e-12)


def test_pipeline_geometry_follows_the_chain_count():
    """The pipeline's window is chosen with the chain count and the CU count in hand (pipe_layout.h: pipe_geometry):
    rows without an integral get more, smaller producer blocks per chain while every block still has a CU of its own
    (the window stays 192 steps at 512 q x 400 contributions: 3 / 4 / 6 rows per producer wave), rows with an integral
    the number of producer blocks that gives the most steps per round of CUs.  Pinned here on a 256-CU MI355X."""
    import mcsas_amd
    import torch
    from bench import synthetic_data
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the expected windows are those of a 256-CU device (the library reads the CU count at run time)")
    q, I, sig = synthetic_data(512)
    m = mcsas_amd.Sphere()
    m.radius.setActiveRange((np.pi / q.max(), np.pi / q.min()))
    for reps in (1, 28, 36, 50, 100):
        st = engine.Settings(n_contrib=400, n_reps=reps, max_iter=100, conv_crit=0.0, max_retries=0, seed=1, exec_mode=engine.EXEC_PIPELINE)
        plan = engine.Plan(m.setup(), q, I, sig, st)
        assert plan.info["exec_mode"] == "pipeline" and plan.info["window"] == 192, (reps, plan.info)
        plan.close()
    # Kholodenko, 600 contributions, rows that cost an integral: the window is as long as 2 Kb <= N allows (296 steps; the cap is one
    # step per thread of a workgroup, 512) whatever the chain count — the chain's producer waves pull its rows from a queue (round 4)
    g = load("g9_kho_q512.npz")
    mk, _ = make_models("kholodenko", g["spec_lo"], g["spec_hi"])
    for reps, window in ((13, 296), (50, 296), (300, 296)):
        st = engine.Settings(n_contrib=600, n_reps=reps, max_iter=10, conv_crit=0.0, max_retries=0, seed=1, exec_mode=engine.EXEC_PIPELINE)
        plan = engine.Plan(mk.setup(FakeData(g["data_q"])), g["data_q"], g["data_I"], g["data_sigma"], st)
        assert plan.info["window"] == window, (reps, plan.info)
        plan.close()


# ------------------------------------------------------------------------------ run-time model plug-ins
@pytest.mark.parametrize("tag,name", [("gausschain", "g4_gausschain_q40.npz"), ("sphcs", "g4_sphcs_q40.npz")])
def test_plugin_model_replays_the_reference_and_equals_its_built_in_twin(tag, name):
    """A model that reaches the library as HIP source text (mcsas_hip_plugin_compile) runs the same kernels as the built-in
    ones, in every execution mode: written operation for operation like its built-in twin it replays the reference's trajectory
    and is bit-identical to the twin — chain results, ScatteringModel.calc, the histogram preparation and the visibility limits
    alike."""
    from helpers import plugin_twin
    g, m, spec, st, ost = traj_setup(name)
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    modes = [(engine.EXEC_WAVE, 1, 1), (engine.EXEC_WAVE, 1, 0), (engine.EXEC_WORKGROUP, 8, 1), (engine.EXEC_PIPELINE, 0, 1)]
    refs = []
    for mode, waves, cache in modes:
        st.exec_mode, st.waves_per_chain, st.cache_intensities = mode, waves, cache
        refs.append(engine.analyse(m.setup(FakeData(q)), q, I, sig, st, replay=g["stream"][None, :]))
    ref = refs[0]
    pset = np.array(ref.contribs[:, :, 0])
    calc_ref = engine.model_calc(m.setup(), q, pset, st.comp_exp, want_rows=True)
    prep_ref = engine.histogram_prep(m.setup(), q, I, sig, ref.contribs, st.comp_exp, st.find_background, st.positive_background)
    sc, v, w = prep_ref[0], prep_ref[1], prep_ref[2]
    vf = w * sc[0][None, :] / v
    obs_ref = engine.observability(m.setup(), q, sig, ref.contribs, sc[0], vf, st.comp_exp)
    plugin_twin(m, tag)
    setup = m.setup(FakeData(q))
    assert setup.model_id >= engine.MODEL_PLUGIN0
    for (mode, waves, cache), twin in zip(modes, refs):
        st.exec_mode, st.waves_per_chain, st.cache_intensities = mode, waves, cache
        res = engine.analyse(setup, q, I, sig, st, replay=g["stream"][None, :])
        assert res.num_iter[0] == int(g["res_num_iter"]) and res.num_moves[0] == int(g["res_num_moves"])
        np.testing.assert_allclose(res.contribs[:, :, 0], g["res_rset"], rtol=1e-12)
        np.testing.assert_allclose(res.chisq[0], float(g["res_conval"]), rtol=1e-7)
        assert np.array_equal(res.contribs, twin.contribs) and np.array_equal(res.fit, twin.fit) and res.chisq[0] == twin.chisq[0], (mode, waves, cache)
    for a, b in zip(engine.model_calc(setup, q, pset, st.comp_exp, want_rows=True), calc_ref):
        assert np.array_equal(a, b)
    for a, b in zip(engine.histogram_prep(setup, q, I, sig, ref.contribs, st.comp_exp, st.find_background, st.positive_background), prep_ref):
        assert np.array_equal(a, b)
    assert np.array_equal(engine.observability(setup, q, sig, ref.contribs, sc[0], vf, st.comp_exp), obs_ref)
    # more than 1024 q-points: the q-split workgroup kernel, compiled for the plug-in like the others (what auto picks); one
    # wavefront per chain is refused for a plug-in there, not silently replaced
    qw, Iw, sw = _synthetic(1500)
    stw = engine.Settings(n_contrib=24, n_reps=2, max_iter=60, conv_crit=1e-9, max_retries=0, seed=3)
    wide = engine.analyse(setup, qw, Iw, sw, stw)
    m2, _ = make_models(tag, g["spec_lo"], g["spec_hi"], [int(x) for x in g["spec_gen"]])
    for p_, p2 in zip(m.params(), m2.params()):
        p2.setValue(p_())
    twin = engine.analyse(m2.setup(), qw, Iw, sw, stw)
    assert twin.num_moves.sum() > 0 and np.array_equal(wide.contribs, twin.contribs) and np.array_equal(wide.fit, twin.fit)
    with pytest.raises(mcsas_amd._lib.McSASHipError) as e:
        engine.analyse(setup, qw, Iw, sw, engine.Settings(**{**stw.__dict__, "exec_mode": engine.EXEC_WAVE}))
    assert e.value.code == -1


def test_plugin_model_through_the_mcsas_front_end():
    """McSAS.calc() — analyse() + histogram() — with a model class of the user's own (`hipSource`), free-running: the same seed
    gives the same result dictionary as the built-in twin."""
    from helpers import plugin_twin
    out = []
    for as_plugin in (False, True):
        m, _ = make_models("gausschain", [1e-9, 5e-8], [3e-8, 2e-7], [1, 0])
        if as_plugin:
            plugin_twin(m, "gausschain")
        rng = np.random.default_rng(5)
        q = np.geomspace(1e8, 4e9, 60)
        pset = np.column_stack([rng.uniform(2e-9, 2e-8, 30), rng.uniform(6e-8, 1.5e-7, 30)])
        base = m.calc(q, pset, 0.6666666).chisqrInt
        I = base / base.max() + 1e-3
        sig = 0.02 * I
        algo = mcsas_amd.McSAS.factory()()
        algo.numContribs.setValue(40); algo.numReps.setValue(4); algo.maxIterations.setValue(3000)
        algo.convergenceCriterion.setValue(1e-3); algo.maxRetries.setValue(0); algo.showIncomplete.setValue(True)
        algo.seed = 11
        algo.model = m
        algo.data = mcsas_amd.SASData(q, I, sig)
        algo.calc()
        out.append(algo.result[0])
        assert engine.Plan(m.setup(), q, I, sig, algo._settings(40, 4)).info["exec_mode"] == "pipeline"   # what auto picks for 4 chains
    a, b = out
    assert np.array_equal(a["contribs"], b["contribs"]) and np.array_equal(a["fitMeasValMean"], b["fitMeasValMean"])
    assert np.array_equal(a["scalingFactors"], b["scalingFactors"])


@pytest.mark.parametrize("tag", ["cyl_aspect", "kholodenko", "lmasphere"])
def test_wide_q_workgroup_kernel_with_integral_models_and_smearing_matches_the_wave_kernel(tag):
    """More than 1024 q-points with rows that cost an orientation / contour integral (per-wave row tables in the q-split
    workgroup) and with beam-profile smearing: the same chains as one wavefront per chain — the sums are put together in another
    order, so decisions and parameter sets must agree and chi-squared to rounding."""
    nq = {"cyl_aspect": 1300, "kholodenko": 1100, "lmasphere": 1500}[tag]
    q, I, sig = _synthetic(nq)
    lo, hi = RANDOM_RANGES[tag]
    kw = {"intDiv": 20.} if tag == "cyl_aspect" else {}
    m, spec = make_models(tag, lo, hi, **kw)
    smear = None
    if tag == "lmasphere":
        d, _ = product_smearing("trapezoid", False, 15, q, I, sig, umbra=2e-3 * q.max(), penumbra=4e-3 * q.max())
        smear = d.smearArgs(m)
    out = {}
    for mode in (engine.EXEC_WAVE, engine.EXEC_WORKGROUP):
        st = engine.Settings(n_contrib=24, n_reps=3, max_iter=60, conv_crit=1e-9, max_retries=0, seed=9, exec_mode=mode)
        out[mode] = engine.analyse(m.setup(), q, I, sig, st, smear=smear)
    a, b = out[engine.EXEC_WAVE], out[engine.EXEC_WORKGROUP]
    assert (a.num_iter == 60).all() and np.array_equal(a.num_moves, b.num_moves) and a.num_moves.sum() > 0
    np.testing.assert_array_equal(a.contribs, b.contribs)
    np.testing.assert_allclose(a.chisq, b.chisq, rtol=1e-10)
    np.testing.assert_allclose(a.fit, b.fit, rtol=1e-10)


def test_run_series_replays_the_reference_series():
    """mcsas_amd.run_series against the reference's own series run (fixture g15, oracle/make_golden.py gen_series: the same
    algorithm and model objects, calc() on two data sets drawing from one global stream, the series table of
    gui/calc.py:331-349): each data set's repetitions replay their slices of the reference's stream and every entry of the
    table — (series key, histogram moments) per (parameter, range, weighting) — comes out as the reference's."""
    g = load("g15_series.npz")
    lo, hi = float(g["lo"]), float(g["hi"])
    m, spec = make_models("sphere", [lo], [hi])
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=16, xscale='log', yweight='vol'))
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, 0.5 * hi, binCount=8, xscale='lin', yweight='num'))
    ost = O.Settings(n_contrib=60, n_reps=2, max_iter=200, conv_crit=1e-9, max_retries=1, show_incomplete=True)
    stream = O.ReplayStream(g["stream"])
    datasets, replays = [], []
    for i in range(2):
        pre = "d%d_" % i
        _, info = O.analyse(spec, g[pre + "q"], g[pre + "I"], g[pre + "sigma"], g[pre + "f_limit"], g[pre + "x0_limit"], ost,
                            stream, method="closed")
        L = max(x["end"] - x["start"] for x in info) + 8
        replays.append(np.stack([np.resize(g["stream"][x["start"]:], L) for x in info]))
        datasets.append(mcsas_amd.SASData(g[pre + "q"], g[pre + "I"], g[pre + "sigma"], f_limit=g[pre + "f_limit"]))
    algo = mcsas_amd.McSAS.factory()()
    algo.numContribs.setValue(60); algo.numReps.setValue(2); algo.maxIterations.setValue(200)
    algo.convergenceCriterion.setValue(1e-9); algo.maxRetries.setValue(0); algo.showIncomplete.setValue(True)
    assert algo.maxRetries() == 1                        # clipped into its valueRange like the reference's (mcsasparameters.json:71-74)
    algo.model = m
    results, series = mcsas_amd.run_series(algo, datasets, keys=list(g["keys"]), replays=replays)
    for i, res in enumerate(results):
        pre = "d%d_" % i
        np.testing.assert_allclose(res["contribs"], g[pre + "contribs"], rtol=1e-12)
        assert res["numIter"] == float(g[pre + "numIter"])
        np.testing.assert_allclose(res["scaling"], g[pre + "scaling"], rtol=1e-6)
    assert len(series) == 2
    for j, (uid, rows) in enumerate(series.items()):
        assert uid[0] == "radius" and uid[3] == str(g["s%d_weight" % j])
        np.testing.assert_allclose(uid[1:3], g["s%d_uid" % j], rtol=1e-15)
        assert [r[0] for r in rows] == list(g["s%d_keys" % j])
        got = np.array([r[1] for r in rows], dtype=float)
        # (value, uncertainty) pairs of mean / variance / skew / kurtosis: the values are sums over all contributions; their
        # uncertainties are standard deviations over TWO repetitions of nearly equal numbers
        np.testing.assert_allclose(got[:, 0::2], g["s%d_moments" % j][:, 0::2], rtol=1e-6)
        want = g["s%d_moments" % j]
        for r in range(want.shape[0]):
            for c in range(1, want.shape[1], 2):
                np.testing.assert_allclose(got[r, c], want[r, c], rtol=1e-4, atol=1e-9 * abs(want[r, c - 1]))


def test_bench_workload_at_full_budget_equals_the_c_oracle_chain_by_chain():
    """bench.py's headline workload exactly as it is timed — synthetic 512 q x 400 contributions x 50 repetitions x 20 000
    steps, pipeline mode, Philox streams — against the plain-C oracle (oracle/c) run on the same counter-based streams: every
    chain takes the same decisions over its full budget (move counts, final parameter sets: exact; chi-squared 1e-7)."""
    from oracle import c_oracle
    q, I, sig = _synthetic(512)
    lo, hi = np.pi / q.max(), np.pi / q.min()
    m, _ = make_models("sphere", [lo], [hi])
    st = engine.Settings(n_contrib=400, n_reps=50, max_iter=20000, conv_crit=0.0, max_retries=0, seed=1000, exec_mode=engine.EXEC_PIPELINE)
    res = engine.analyse(m.setup(), q, I, sig, st)
    ref = c_oracle.analyse_sphere(q, I, sig, lo, hi, 400, 50, 20000, 0.0, seed=1000, threads=min(16, os.cpu_count() or 1))
    assert (res.num_iter == 20000).all() and (ref.num_iter == 20000).all()
    np.testing.assert_array_equal(res.num_moves, ref.num_moves)
    np.testing.assert_allclose(res.contribs, ref.contribs, rtol=1e-12)
    np.testing.assert_allclose(res.chisq, ref.chisq, rtol=1e-7)
    assert 900 < res.num_moves.mean() < 1600            # (~6 % of the steps are accepted)


@pytest.mark.parametrize("config,tag,lo,hi,steps", [
    (3, "cyl_aspect", [1e-9, 0.5], [1e-7, 20.0], 4000),
    (4, "ellcs", [1e-9, 2e-9, 2e-10], [1e-7, 2e-7, 1e-8], 3000)])
def test_bench_workloads_of_configs_3_and_4_equal_the_c_oracle_chain_by_chain(config, tag, lo, hi, steps):
    """BASELINE configs 3 and 4 AS bench.py TIMES THEM — its ground-truth curve of the model under test (512 q / 1024 q), 400 / 1000
    contributions, the per-GPU share of the repetitions (25 / 50), row-queue pipeline with helping blocks, Philox streams — over ten
    sweeps (4000 steps) / three sweeps (3000 steps) against the plain-C oracle (oracle/c: models/cylindersisotropic.py:50-101,
    ellipsoidalcoreshell.py:59-97 restated with libm and Cephes' J1, pinned on the CPU against the reference's own chains) on the
    same counter-based streams: every chain takes the same decisions (move counts and parameter sets exact, chi-squared 1e-7)."""
    from oracle import c_oracle
    import bench
    wl = bench.workload(config, 0)
    _, spec = make_models(tag, lo, hi)
    setup = wl["model"].setup()
    assert list(setup.gen_lo) == list(spec.lo) and list(setup.gen_hi) == list(spec.hi) and tuple(setup.gen_kind) == tuple(spec.gen)
    np.testing.assert_array_equal(setup.params, spec.values)
    st = engine.Settings(n_contrib=wl["n"], n_reps=wl["reps_gpu"], max_iter=steps, conv_crit=0.0, max_retries=0, seed=1000,
                         exec_mode=engine.EXEC_PIPELINE)
    plan = engine.Plan(setup, wl["q"], wl["I"], wl["sigma"], st)
    assert plan.info["exec_mode"] == "pipeline"
    plan.launch(); res = plan.fetch(); plan.close()
    ref = c_oracle.analyse(spec, wl["q"], wl["I"], wl["sigma"], wl["n"], wl["reps_gpu"], steps, 0.0, seed=1000,
                           threads=min(16, os.cpu_count() or 1))
    assert (res.num_iter == steps).all() and (ref.num_iter == steps).all()
    np.testing.assert_array_equal(res.num_moves, ref.num_moves)
    np.testing.assert_allclose(res.contribs, ref.contribs, rtol=1e-12)
    np.testing.assert_allclose(res.chisq, ref.chisq, rtol=1e-7)
    assert res.num_moves.min() > 50


def test_many_chains_as_timed_sampled_against_the_c_oracle():
    """The kernel north_star describes, at the size bench.py's `many_chains` times it — 8192 chains x 20 000 steps, one wavefront per
    chain (chain_wave_kernel<0, 8, true>) — with 32 of the chains (four blocks of eight, first / middle / last) against the plain-C
    oracle on the same Philox streams (chain id = repetition index): same move counts, parameter sets, chi-squared."""
    from oracle import c_oracle
    q, I, sig = _synthetic(512)
    lo, hi = np.pi / q.max(), np.pi / q.min()
    m, _ = make_models("sphere", [lo], [hi])
    st = engine.Settings(n_contrib=400, n_reps=8192, max_iter=20000, conv_crit=0.0, max_retries=0, seed=20250101, exec_mode=engine.EXEC_WAVE)
    res = engine.analyse(m.setup(), q, I, sig, st)
    assert (res.num_iter == 20000).all()
    for first in (0, 2731, 5000, 8184):
        ref = c_oracle.analyse_sphere(q, I, sig, lo, hi, 400, 8, 20000, 0.0, seed=20250101, rep_offset=first, threads=8)
        sl = slice(first, first + 8)
        np.testing.assert_array_equal(res.num_moves[sl], ref.num_moves)
        np.testing.assert_allclose(res.contribs[:, :, sl], ref.contribs, rtol=1e-12)
        np.testing.assert_allclose(res.chisq[sl], ref.chisq, rtol=1e-7)


@pytest.mark.parametrize("tag", ["cyl_aspect", "kholodenko", "ellcs"])
def test_rows_with_an_integral_give_the_same_chain_whatever_the_chain_count(tag):
    """Pipeline mode, rows that cost an integral: the producer blocks per chain follow the number of chains in the launch, and which
    wave evaluates which row is decided at run time (the chain's waves pull rows from a queue) — nothing a chain decides may depend
    on either (the window is fixed by the contribution count, 8-step Gram blocks taken by the scan block, running sums re-derived
    every 64 steps of the attempt, chi²·Q carried across windows exactly).  24 repetitions in one launch, in two launches of 12 and
    in launches of 5: bit for bit the same arrays — which is what makes a device list (mcsas_problem.devices) reproduce one device
    for these models too — and the same again when the launch is simply repeated."""
    q, I, sig = _synthetic(128)
    lo, hi = RANDOM_RANGES[tag]
    kw = {"intDiv": 20.} if tag in ("cyl_aspect", "ellcs") else {}
    m, _ = make_models(tag, lo, hi, **kw)
    st = engine.Settings(n_contrib=400, n_reps=24, max_iter=900, conv_crit=1e-9, max_retries=0, seed=21, exec_mode=engine.EXEC_PIPELINE)
    one = engine.analyse(m.setup(), q, I, sig, st)
    windows = [engine.Plan(m.setup(), q, I, sig, engine.Settings(**{**st.__dict__, "n_reps": r})).info["window"] for r in (24, 12, 5)]
    # 2 Kb <= N = 400, a multiple of 8 — and since round 5 the window follows the chain count where a tick is only a few rounds of rows
    # (24 chains x 200 rows on 2048 wave slots are 2.3 rounds: 168 steps = 2 rounds; 12 and 5 chains: the longest): the arrays must not care
    assert all(w % 8 == 0 and 100 <= w <= 200 for w in windows) and windows[2] == 200
    assert one.num_moves.min() > 0 and len(set(one.num_moves.tolist())) > 3
    again = engine.analyse(m.setup(), q, I, sig, st)
    for name in ("contribs", "fit", "chisq", "num_iter", "num_moves"):
        np.testing.assert_array_equal(getattr(again, name), getattr(one, name), err_msg=name + " (same launch repeated)")
    for devs in ((0, 0), (0,) * 5):
        many = engine.analyse(m.setup(), q, I, sig, engine.Settings(**{**st.__dict__, "devices": devs}))
        for name in ("contribs", "fit", "chisq", "scaling", "background", "num_iter", "num_moves"):
            np.testing.assert_array_equal(getattr(many, name), getattr(one, name), err_msg="%s with %d blocks" % (name, len(devs)))


@pytest.mark.parametrize("tag,nq,N,R,steps", [("cyl_aspect", 100, 48, 7, 120), ("ellcs", 100, 48, 7, 120), ("kholodenko", 40, 32, 5, 60)])
def test_rows_with_an_integral_retries_and_uneven_chain_ends_follow_the_oracle(tag, nq, N, R, steps):
    """McSAS.analyse's retry loop (mcsas.py:220-246) for models whose rows cost an integral, in the pipeline's row-queue kernels:
    seven (five) free-running chains, up to three attempts of 120 (60) steps each, with a criterion that about half of the first
    attempts reach — so chains converge in different windows, fail and start again from a new initial set (pulled from the chain's
    initialisation queue), or give up, while the producer blocks of the chains that are through join the queues of the others.
    Every chain against the oracle walking the same Philox stream attempt after attempt: attempts, iterations and moves of the
    last attempt, draws, parameter sets exact; chi² 1e-7.  The wavefront mode must give the same arrays."""
    q, I, sig = _synthetic(nq)
    lo, hi = RANDOM_RANGES[tag]
    kw = {"intDiv": 20.} if tag in ("cyl_aspect", "ellcs") else {}
    m, spec = make_models(tag, lo, hi, **kw)
    retries, seed = 2, 4242
    lim = ([I.min(), I.max()], [q.min(), q.max()])
    # criterion: the median chi² the first attempts end at with none
    first = [O.mc_fit(spec, q, I, sig, lim[0], lim[1], O.Settings(n_contrib=N, n_reps=1, max_iter=steps, conv_crit=0.0),
                      O.PhiloxStream(seed, r), method="closed").conval for r in range(R)]
    crit = float(np.median(first)) * 1.001                    # (the median IS one chain's final chi²: no tie with its last step)
    ost = O.Settings(n_contrib=N, n_reps=1, max_iter=steps, conv_crit=crit)
    refs = []
    for r in range(R):
        stream, att = O.PhiloxStream(seed, r), 0
        while True:
            ref = O.mc_fit(spec, q, I, sig, lim[0], lim[1], ost, stream, method="closed")
            att += 1
            if ref.conval <= crit or att > retries:
                break
        refs.append((att, ref))
    assert len({a for a, _ in refs}) > 1 and any(ref.conval <= crit for _, ref in refs)
    out = {}
    for mode in (engine.EXEC_PIPELINE, engine.EXEC_WAVE):
        st = engine.Settings(n_contrib=N, n_reps=R, max_iter=steps, conv_crit=crit, max_retries=retries, seed=seed, exec_mode=mode)
        res = out[mode] = engine.analyse(m.setup(), q, I, sig, st)
        for r, (att, ref) in enumerate(refs):
            assert res.attempts[r] == att and res.num_iter[r] == ref.num_iter and res.num_moves[r] == ref.num_moves, (mode, r)
            assert res.converged[r] == (1 if ref.conval <= crit else 0)
            np.testing.assert_allclose(res.contribs[:, :, r], ref.rset, rtol=1e-12)
            np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-7)
    for name in ("contribs", "num_iter", "num_moves", "draws", "attempts", "converged"):
        np.testing.assert_array_equal(getattr(out[engine.EXEC_PIPELINE], name), getattr(out[engine.EXEC_WAVE], name), err_msg=name)


def test_row_queue_window_at_its_cap_of_512_steps():
    """Rows with an integral, more than 1024 contributions: the window is capped at one proposal per thread of a workgroup (512
    steps, 64 sub-windows) — core-shell ellipsoids, 1100 contributions, three chains over 1300 steps (two full windows and a part of
    a third, a sweep over the contributions and a fifth) give the wavefront mode's arrays."""
    q, I, sig = _synthetic(64)
    lo, hi = RANDOM_RANGES["ellcs"]
    m, _ = make_models("ellcs", lo, hi, intDiv=12.)
    out = {}
    for mode in (engine.EXEC_PIPELINE, engine.EXEC_WAVE):
        st = engine.Settings(n_contrib=1100, n_reps=3, max_iter=1300, conv_crit=1e-9, max_retries=0, seed=5, exec_mode=mode)
        plan = engine.Plan(m.setup(), q, I, sig, st)
        if mode == engine.EXEC_PIPELINE:
            assert plan.info["exec_mode"] == "pipeline" and plan.info["window"] == 512
        plan.launch(); out[mode] = plan.fetch(); plan.close()
    for name in ("contribs", "num_iter", "num_moves", "draws"):
        np.testing.assert_array_equal(getattr(out[engine.EXEC_PIPELINE], name), getattr(out[engine.EXEC_WAVE], name), err_msg=name)
    assert out[engine.EXEC_PIPELINE].num_moves.min() > 20


def test_plugin_model_with_an_integral_runs_the_row_queue_kernels():
    """A plug-in that declares `#define MCSAS_PLUGIN_ROW_CLASS 1` (its form factor loops over orientations: isotropic ellipsoids,
    models/ellipsoidsisotropic.py:51-81, written the plain way) is spread over the chip like the built-in models with an
    integral — `pipe_tick_kernel<MCSAS_MODEL_PLUGIN, QPL, true>` compiled at run time, rows pulled from the chain's queue, blocks
    helping each other.  Its intensities equal the oracle's (1e-9), its free-running chains are the same arrays in the pipeline,
    wavefront and workgroup modes, and they follow the oracle on the same Philox streams decision for decision."""
    from helpers import plugin_twin
    lo, hi = RANDOM_RANGES["elliso"]
    m, spec = make_models("elliso", lo, hi, intDiv=24.)
    plugin_twin(m, "elliso")
    setup = m.setup()
    assert setup.model_id >= engine.MODEL_PLUGIN0
    q, I, sig = _synthetic(100)
    rs = np.random.RandomState(3)
    pars = np.stack([10 ** rs.uniform(np.log10(a), np.log10(b), 9) for a, b in zip(lo, hi)], axis=1)
    cum, v, w, s_, rows = engine.model_calc(setup, q, pars, 0.6666666, want_rows=True)
    ref_it, ref_v = O.model_calc(spec, q, pars, 0.6666666)[:2]
    np.testing.assert_allclose(cum, ref_it, rtol=1e-9)
    np.testing.assert_allclose(v, ref_v, rtol=1e-12)
    N, R, steps, seed = 48, 5, 150, 808
    out = {}
    for mode in (engine.EXEC_PIPELINE, engine.EXEC_WAVE, engine.EXEC_WORKGROUP):
        st = engine.Settings(n_contrib=N, n_reps=R, max_iter=steps, conv_crit=1e-9, max_retries=0, seed=seed, exec_mode=mode)
        plan = engine.Plan(setup, q, I, sig, st)
        assert plan.info["exec_mode"] == {engine.EXEC_PIPELINE: "pipeline", engine.EXEC_WAVE: "wave", engine.EXEC_WORKGROUP: "workgroup"}[mode]
        if mode == engine.EXEC_PIPELINE:
            assert plan.info["window"] == 24                   # 2 Kb <= N: the row-queue geometry (8-step sub-windows)
        plan.launch(); out[mode] = plan.fetch(); plan.close()
    for mode in (engine.EXEC_WAVE, engine.EXEC_WORKGROUP):
        for name in ("contribs", "num_iter", "num_moves", "draws"):
            np.testing.assert_array_equal(getattr(out[mode], name), getattr(out[engine.EXEC_PIPELINE], name), err_msg=name)
    ost = O.Settings(n_contrib=N, n_reps=1, max_iter=steps, conv_crit=1e-9)
    res = out[engine.EXEC_PIPELINE]
    for r in range(R):
        ref = O.mc_fit(spec, q, I, sig, [I.min(), I.max()], [q.min(), q.max()], ost, O.PhiloxStream(seed, r), method="closed")
        assert res.num_moves[r] == ref.num_moves and res.num_iter[r] == ref.num_iter
        np.testing.assert_allclose(res.contribs[:, :, r], ref.rset, rtol=1e-12)
        np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-7)
    assert res.num_moves.min() > 5


def test_plugin_model_with_can_smear_matches_the_reference_smeared_intensities():
    """A plug-in that declares canSmear (`#define MCSAS_PLUGIN_CAN_SMEAR 1`, plus `canSmear = True` on the model class) is
    smeared like the built-in models: the reference's smeared sphere intensities (fixture g7, slit and pinhole trapezoid,
    Gaussian) through a sphere written as plug-in text, and a short smeared chain equal in wave and pipeline mode."""
    from helpers import plugin_twin
    g = load("g7_smearing.npz")
    for tag, kind, two_d in SMEAR_CASES:
        pre = tag + "_"
        q = g[pre + "q"]
        widths = {k: float(g[pre + k]) for k in ("umbra", "penumbra", "variance") if pre + k in g}
        d, args = product_smearing(kind, two_d, int(g[pre + "n_steps"]), q, **widths)
        m, _ = make_models("sphere", [1e-10], [1e-6])
        plugin_twin(m, "sphere")
        assert m.canSmear and m.setup().model_id >= engine.MODEL_PLUGIN0
        cum, v, w, s, rows = engine.model_calc(m.setup(), q, g[pre + "sphere_radii"][:, None], 0.6666666, want_rows=True, smear=d.smearArgs(m))
        np.testing.assert_allclose(rows, g[pre + "sphere_it"], rtol=1e-9)
    q, I, sig = _synthetic(100)
    d, _ = product_smearing("trapezoid", False, 15, q, I, sig, umbra=2e-3 * q.max(), penumbra=4e-3 * q.max())
    m, _ = make_models("sphere", [np.pi / q.max()], [np.pi / q.min()])
    plugin_twin(m, "sphere")
    out = []
    for mode in (engine.EXEC_WAVE, engine.EXEC_PIPELINE):
        st = engine.Settings(n_contrib=40, n_reps=3, max_iter=300, conv_crit=1e-9, max_retries=0, seed=4, exec_mode=mode)
        out.append(engine.analyse(m.setup(), q, I, sig, st, smear=d.smearArgs(m)))
    assert out[0].num_moves.sum() > 0 and np.array_equal(out[0].num_moves, out[1].num_moves)
    np.testing.assert_array_equal(out[0].contribs, out[1].contribs)
    unsmeared = engine.analyse(m.setup(), q, I, sig, engine.Settings(n_contrib=40, n_reps=3, max_iter=300, conv_crit=1e-9, max_retries=0, seed=4, exec_mode=engine.EXEC_WAVE))
    assert not np.array_equal(unsmeared.contribs, out[0].contribs)


@pytest.mark.parametrize("mode", [engine.EXEC_PIPELINE, engine.EXEC_WAVE, engine.EXEC_WORKGROUP])
def test_result_slots_keep_two_analyses_apart(mode):
    """mcsas_hip_plan_launch_slot / _fetch_slot: two analyses queued back to back on one stream into the plan's two result
    slots (one set of workspaces) come back exactly as when each is run alone — also when slot 0 is launched again before
    slot 1 has been fetched."""
    g = load("g4_sphere_q100_fixed.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    m, _ = make_models("sphere", g["spec_lo"], g["spec_hi"])
    st = engine.Settings(n_contrib=200, n_reps=6, max_iter=2500, conv_crit=0.5, max_retries=1, seed=1, exec_mode=mode)
    alone = {}
    for seed in (11, 12, 13):
        alone[seed] = engine.analyse(m.setup(), q, I, sig, engine.Settings(**{**st.__dict__, "seed": seed}))
    pl = engine.Plan(m.setup(), q, I, sig, st)
    pl.reseed(11); pl.launch(slot=0)
    pl.reseed(12); pl.launch(slot=1)
    a = pl.fetch(slot=0)
    pl.reseed(13); pl.launch(slot=0)
    b = pl.fetch(slot=1)
    c = pl.fetch(slot=0)
    for got, seed in ((a, 11), (b, 12), (c, 13)):
        for name in ("contribs", "fit", "chisq", "num_iter", "num_moves", "attempts", "converged"):
            np.testing.assert_array_equal(getattr(got, name), getattr(alone[seed], name), err_msg="%s seed %d" % (name, seed))
    with pytest.raises(mcsas_amd._lib.McSASHipError):
        pl.launch(slot=2)


def test_analyse_many_and_overlapped_series_equal_one_after_the_other():
    """engine.analyse_many — a plan per problem, the plans going round two streams, analyses side by side on the chip — returns what
    analyse() returns for each problem (different models, shapes and modes in one list); run_series(overlap=True) gives the same
    results and the same series table as the data sets one after the other."""
    probs = []
    for nq, tag, n, reps, steps, mode in ((100, "sphere", 120, 5, 900, engine.EXEC_AUTO), (257, "gausschain", 60, 3, 400, engine.EXEC_WAVE),
                                          (64, "cyl_aspect", 48, 4, 150, engine.EXEC_PIPELINE), (1500, "sphere", 40, 2, 120, engine.EXEC_AUTO),
                                          (100, "sphere", 120, 5, 900, engine.EXEC_WORKGROUP)):
        q, I, sig = _synthetic(nq)
        lo, hi = RANDOM_RANGES[tag]
        m, _ = make_models(tag, lo, hi, **({"intDiv": 20.} if tag == "cyl_aspect" else {}))
        st = engine.Settings(n_contrib=n, n_reps=reps, max_iter=steps, conv_crit=1e-9, max_retries=0, seed=31 + nq, exec_mode=mode)
        probs.append((m.setup(), q, I, sig, st))
    many = engine.analyse_many(probs)
    for pr, got in zip(probs, many):
        one = engine.analyse(*pr)
        for name in ("contribs", "fit", "chisq", "num_iter", "num_moves"):
            np.testing.assert_array_equal(getattr(got, name), getattr(one, name), err_msg=name)
    # the series driver
    out = []
    for overlap in (False, True):
        datasets = []
        for k, scale in enumerate((1.0, 0.6, 1.7)):
            q, I, sig = _synthetic(100)
            datasets.append(mcsas_amd.SASData(q, I * scale + k * 1e-3 * I.max(), sig * scale))
        q = datasets[0].q
        m = mcsas_amd.Sphere(); m.radius.setActiveRange((np.pi / q.max(), np.pi / q.min()))
        m.radius.histograms().append(mcsas_amd.Histogram(m.radius, np.pi / q.max(), np.pi / q.min(), binCount=12, xscale='log', yweight='vol'))
        algo = mcsas_amd.McSAS(seed=9)
        algo.numContribs.setValue(80); algo.numReps.setValue(4); algo.maxIterations.setValue(1500)
        algo.convergenceCriterion.setValue(1e-9); algo.maxRetries.setValue(1); algo.showIncomplete.setValue(True)
        algo.model = m
        out.append(mcsas_amd.run_series(algo, datasets, keys=[1.0, 2.0, 3.0], overlap=overlap))
    (ra, sa), (rb, sb) = out
    for a, b in zip(ra, rb):
        assert np.array_equal(a["contribs"], b["contribs"]) and np.array_equal(a["fitMeasValMean"], b["fitMeasValMean"])
    assert list(sa) == list(sb)
    for uid in sa:
        for (ka, ma), (kb, mb) in zip(sa[uid], sb[uid]):
            assert ka == kb and np.array_equal(np.array(ma, dtype=float), np.array(mb, dtype=float))
    # what a plan cannot do is run through mcsas_hip_analyse at its place in the sequence: a model with parameters but none active
    # (one contribution, nothing to fit: mcsas.py:198-199) and a device list; a stopped series says "stop pressed"
    q, I, sig = _synthetic(100)
    fixed = mcsas_amd.Sphere(); fixed.radius.setValue(2.5e-8); fixed.radius.setActive(False)
    mixed = [(fixed.setup(), q, I, sig, engine.Settings(n_contrib=1, n_reps=1)), probs[0],
             (probs[0][0], q, I, sig, engine.Settings(n_contrib=120, n_reps=5, max_iter=900, conv_crit=1e-9, max_retries=0, seed=131, devices=(0, 0)))]
    got = engine.analyse_many(mixed)
    for pr, g_ in zip(mixed, got):
        one = engine.analyse(*pr)
        for name in ("contribs", "fit", "chisq", "num_iter"):
            np.testing.assert_array_equal(getattr(g_, name), getattr(one, name), err_msg=name)
    outs = []
    for overlap in (False, True):
        algo = mcsas_amd.McSAS(seed=9)
        algo.model = fixed
        outs.append(mcsas_amd.run_series(algo, [mcsas_amd.SASData(q, I, sig), mcsas_amd.SASData(q, 2 * I, sig)], overlap=overlap)[0])
    for a, b in zip(*outs):
        assert a["contribs"].shape == (1, 0, 1) and np.array_equal(a["fitMeasValMean"], b["fitMeasValMean"])


def test_bench_collective_path_runs_on_rccl(tmp_path):
    """bench.py as a fresh child process under torch.distributed.run (one rank: this box has one GPU) with MCSAS_BENCH_FORCE_DIST=1:
    init_process_group("nccl", device_id=...), the packed all-gather of the results on the device (mcsas_amd/dist.py
    gather_results) and the all-reduce of the timings have executed on RCCL; the gathered arrays are the rank's own results."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dump = os.path.join(str(tmp_path), "forced.npz")
    env = dict(os.environ, MCSAS_BENCH_FORCE_DIST="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MCSAS_BENCH_DRY", "MCSAS_BENCH_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--launches-per-step", "2",
           "--mc-steps", "2000", "--no-cpu-baseline", "--no-convergence-run", "--no-configs", "--no-series", "--dump", dump]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["config"]["ranks_seen"] == 1 and line["value"] > 1e6
    gm = line["gather_ms"]
    assert gm["backend"] == "nccl" and gm["ranks"] == 1 and gm["first"] > 0 and gm["steady"] > 0
    a = np.load(dump)
    assert a["contribs"].shape == (50, 400, 1) and a["fit"].shape == (50, 512) and np.isfinite(a["chisq"]).all()
    assert (a["chisq"] > 0).all() and (a["contribs"] > 0).all()


def test_bench_named_totals_go_through_rccl(tmp_path):
    """bench.py's named totals of configs 3-5 (200 / 400 / 100 repetitions sharded over the ranks: what `--gpus 8` reports per config)
    with the process group on RCCL (one rank, MCSAS_BENCH_FORCE_DIST=1): every rank's block runs between barriers and the timings
    meet in the MAX / SUM all-reduces on the device — executed on hardware here, at world size 1."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MCSAS_BENCH_FORCE_DIST="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MCSAS_BENCH_DRY", "MCSAS_BENCH_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--launches-per-step", "2",
           "--mc-steps", "2000", "--no-cpu-baseline", "--no-convergence-run", "--no-series", "--no-many-chains", "--totals-only", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["gather_ms"]["backend"] == "nccl"
    for k, total in (("3", 200), ("4", 400), ("5", 100)):
        c = line["configs"][k]
        assert c["reps_total"] == c["reps_rank0"] == total and c["ranks_seen"] == 1 and c["scaling"] == "strong"
        assert c["value"] > 1e6 and c["exec_mode"] == "pipeline" and c["mc_steps"] == 2 * total * {"3": 10000, "4": 15000, "5": 10000}[k]

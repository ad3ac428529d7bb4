"""Several analyses in one wavefront-per-chain launch (mcsas_hip_analyse_batch / mcsas_hip_plan_launch_batch, engine.analyse_batch,
run_series(batch=True)): every data set's result is IDENTICAL to its own analysis in MCSAS_EXEC_WAVE, whatever else is in the batch."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mcsas_amd
from mcsas_amd import engine, _lib
from oracle import mcsas_oracle as O
from helpers import load, make_models, product_smearing
from chain_cases import RANGES, _alone, _same, _synthetic

HEAVY = {"cyl_aspect", "ellcs", "kholodenko", "elliso"}        # rows with an integral: fewer contributions and steps


def _problems(tag):
    """3-4 data sets of one model: two q-slot classes (100 and 200 q: two groups), different active ranges, seeds, repetition
    counts (1 / 3 / 7), the row cache on and off; for the sphere a smeared data set, for every model one data set with retries
    that are taken (a criterion no chain reaches)."""
    lo, hi = RANGES[tag]
    n, steps = (24, 120) if tag in HEAVY else (60, 700)
    out = []
    for k, (nq, reps, cache, shrink, retries) in enumerate(((100, 3, 1, 1.0, 0), (200, 1, 0, 0.5, 0), (100, 7, 0, 0.8, 2), (200, 3, 1, 1.0, 0))):
        if tag in HEAVY and k == 3:
            continue
        q, I, sig = _synthetic(nq)
        m, _ = make_models(tag, lo, [l + shrink * (h - l) for l, h in zip(lo, hi)], **({"intDiv": 12.} if tag == "cyl_aspect" else {}))
        crit = 0.0 if retries else 1e-9
        st = engine.Settings(n_contrib=n, n_reps=reps, max_iter=steps, conv_crit=crit, max_retries=retries, seed=101 + 7 * k,
                             cache_intensities=cache, exec_mode=engine.EXEC_AUTO)
        smear = None
        if tag == "sphere" and k == 1:
            d, smear = product_smearing("trapezoid", False, 9, q, I, sig, umbra=2e-3 * q.max(), penumbra=4e-3 * q.max())
        out.append(dict(model=m.setup(), q=q, intensity=I, sigma=sig, st=st, smear=smear))
    return out


@pytest.mark.parametrize("tag", list(RANGES))
def test_batch_equals_each_problem_alone(tag):
    probs = _problems(tag)
    got = engine.analyse_batch(probs)
    ones = [_alone(pr) for pr in probs]
    for i, (g, one) in enumerate(zip(got, ones)):
        _same(g, one, (tag, i))
    assert sum(int(g.num_moves.sum()) for g in got) > 0
    retried = [g for pr, g in zip(probs, got) if pr["st"].max_retries]
    assert retried and all((g.attempts == 3).all() for g in retried)          # (conv_crit 0: every retry is taken)
    # independence: reversed, and a subset
    rev = engine.analyse_batch(probs[::-1])
    for g, one in zip(rev[::-1], ones):
        _same(g, one, (tag, "reversed"))
    sub = engine.analyse_batch([probs[2], probs[0]])
    _same(sub[0], ones[2], (tag, "subset")); _same(sub[1], ones[0], (tag, "subset"))


def test_resident_plans_launched_as_a_batch_and_reseeded():
    """engine.launch_batch on resident plans: each plan's fetch, total steps and a reseed between launches as for its own launch."""
    probs = _problems("sphere")
    plans = [engine.Plan(pr["model"], pr["q"], pr["intensity"], pr["sigma"], engine.Settings(**{**pr["st"].__dict__, "exec_mode": engine.EXEC_WAVE}),
                         smear=pr["smear"]) for pr in probs]
    try:
        for seed in (0, 5):
            for k, pl in enumerate(plans):
                pl.reseed(probs[k]["st"].seed + seed)
            engine.launch_batch(plans)
            for k, pl in enumerate(plans):
                got = pl.fetch()
                one = _alone(dict(probs[k], st=engine.Settings(**{**probs[k]["st"].__dict__, "seed": probs[k]["st"].seed + seed})))
                _same(got, one, ("plan", seed, k))
                assert pl.total_steps >= int(one.num_iter.sum()) > 0
                assert pl.last_ms > 0
    finally:
        for pl in plans:
            pl.close()


def test_reference_series_through_the_batch():
    """Fixture g15 (the reference's own series run, 100 and 64 q: two groups) through run_series(batch=True): as
    test_run_series_replays_the_reference_series asks of the one-after-another run."""
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
    algo.model = m
    results, series = mcsas_amd.run_series(algo, datasets, keys=list(g["keys"]), replays=replays, batch=True)
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
        np.testing.assert_allclose(got[:, 0::2], g["s%d_moments" % j][:, 0::2], rtol=1e-6)
        want = g["s%d_moments" % j]
        for r in range(want.shape[0]):
            for c in range(1, want.shape[1], 2):
                np.testing.assert_allclose(got[r, c], want[r, c], rtol=1e-4, atol=1e-9 * abs(want[r, c - 1]))


def test_plugin_model_in_a_batch_equals_its_wave_analysis():
    """The shipped run-time plug-in (CylindersRadiallyIsotropic, hipSource) gets the batch kernel through the run-time compiler."""
    m, _ = make_models("cylradiso", [2e-9, 1.0], [5e-8, 40.0])
    probs = []
    for k, (nq, reps) in enumerate(((40, 2), (100, 3))):
        q, I, sig = _synthetic(nq)
        setup = m.setup(mcsas_amd.SASData(q, I, sig))
        assert setup.model_id >= engine.MODEL_PLUGIN0
        probs.append(dict(model=setup, q=q, intensity=I, sigma=sig,
                          st=engine.Settings(n_contrib=16, n_reps=reps, max_iter=60, conv_crit=1e-9, max_retries=0, seed=7 + k)))
    got = engine.analyse_batch(probs)
    for i, pr in enumerate(probs):
        _same(got[i], _alone(pr), ("plugin", i))
    assert sum(int(g.num_moves.sum()) for g in got) > 0


def test_config2_shape_sampled_against_the_c_oracle():
    """Shape (b) of tools/bench_series_batch.py (512 q x 400 contributions x 50 repetitions x 160 data sets) at a reduced step budget:
    16 chains from different data sets against the plain-C oracle on the same Philox streams, chain by chain."""
    from oracle import c_oracle
    import bench
    q, I, sig = _synthetic(512)
    lo, hi = np.pi / q.max(), np.pi / q.min()
    m, _ = make_models("sphere", [lo], [hi])
    rng = np.random.default_rng(5)
    probs = []
    for d in range(160):
        Id = I * (1.0 + 0.05 * rng.standard_normal(len(q)))
        probs.append(dict(model=m.setup(), q=q, intensity=Id, sigma=sig,
                          st=engine.Settings(n_contrib=400, n_reps=50, max_iter=600, conv_crit=0.0, max_retries=0, seed=1000 + d)))
    got = engine.analyse_batch(probs)
    assert all((g.num_iter == 600).all() for g in got)
    for d, r in ((0, 0), (17, 49), (40, 3), (63, 25), (80, 11), (99, 0), (120, 42), (159, 49), (5, 7), (33, 33), (71, 1),
                 (88, 48), (101, 20), (133, 9), (147, 30), (152, 14)):
        ref = c_oracle.analyse_sphere(q, probs[d]["intensity"], sig, lo, hi, 400, 1, 600, 0.0, seed=1000 + d, rep_offset=r, threads=1)
        assert got[d].num_moves[r] == ref.num_moves[0], (d, r)
        np.testing.assert_allclose(got[d].contribs[:, :, r], ref.contribs[:, :, 0], rtol=1e-12)
        np.testing.assert_allclose(got[d].chisq[r], ref.chisq[0], rtol=1e-7)


def test_stop_word_set_before_the_launch_ends_every_chain():
    g = load("g4_sphere_q100_fixed.npz")
    m, _ = make_models("sphere", g["spec_lo"], g["spec_hi"])
    stop = ctypes.c_int32(1)
    probs = []
    for k, nq in enumerate((100, 200, 100)):
        q, I, sig = _synthetic(nq)
        probs.append(dict(model=m.setup(), q=q, intensity=I, sigma=sig, stop=stop,
                          st=engine.Settings(n_contrib=100, n_reps=2 + k, max_iter=10**9, conv_crit=0.0, max_retries=0, seed=1 + k)))
    for res in engine.analyse_batch(probs):
        assert (res.num_iter == 0).all() and (res.converged == 0).all()


class _PythonOnlySphere(mcsas_amd.SASModel):
    shortName = "Sphere (Python only, batch test)"
    canSmear = True
    parameters = mcsas_amd.Sphere.parameters

    def __init__(self):
        super().__init__()
        self.radius.setActive(True)

    def surface(self):
        return 4. * np.pi * self.radius() * self.radius()

    def volume(self):
        return (np.pi * 4. / 3.) * self.radius()**3

    def absVolume(self):
        return self.volume() * self.sld()**2

    def formfactor(self, dataset):
        qr = self.getQ(dataset) * self.radius()
        return 3. * (np.sin(qr) - qr * np.cos(qr)) / (qr**3.)


def test_errors_and_mixed_lists():
    lib = _lib.load()
    q, I, sig = _synthetic(100)
    m, _ = make_models("sphere", *RANGES["sphere"])
    st = engine.Settings(n_contrib=40, n_reps=2, max_iter=200, conv_crit=1e-9, max_retries=0, seed=3)

    def plan(mode=engine.EXEC_WAVE, stop=None):
        return engine.Plan(m.setup(), q, I, sig, engine.Settings(**{**st.__dict__, "exec_mode": mode}), stop=stop)

    def rc_of(plans, n=None):
        hs = (ctypes.c_void_p * max(len(plans), 1))(*[p.h.value for p in plans])
        return lib.mcsas_hip_plan_launch_batch(hs, len(plans) if n is None else n, None)

    a, b = plan(), plan(engine.EXEC_PIPELINE)
    s1, s2 = ctypes.c_int32(0), ctypes.c_int32(0)
    c, d = plan(stop=s1), plan(stop=s2)
    try:
        for plans, n, words in (([a, b], None, "exec_mode"), ([c, d], None, "stop"), ([a], 0, "n >= 1"), ([a, a], None, "again")):
            assert rc_of(plans, n) == -1
            assert words in lib.mcsas_hip_last_error().decode(), words
        with pytest.raises(_lib.McSASHipError) as e:
            engine.launch_batch([a, b])
        assert e.value.code == -1
        engine.launch_batch([a])                                             # a valid batch still runs afterwards
        _same(a.fetch(), _alone(dict(model=m.setup(), q=q, intensity=I, sigma=sig, st=st)))
    finally:
        for p in (a, b, c, d):
            p.close()
    # the one-shot form refuses what a batch cannot run, before anything is launched
    for bad in (dict(exec_mode=engine.EXEC_PIPELINE), dict(exec_mode=engine.EXEC_WORKGROUP)):
        with pytest.raises(_lib.McSASHipError) as e:
            engine.analyse_batch([(m.setup(), q, I, sig, st), (m.setup(), q, I, sig, engine.Settings(**{**st.__dict__, **bad}))])
        assert e.value.code == -1
    # no active parameter: answered at its place as analyse() answers it
    fixed = mcsas_amd.Sphere(); fixed.radius.setValue(2.5e-8); fixed.radius.setActive(False)
    mixed = [(m.setup(), q, I, sig, st), (fixed.setup(), q, I, sig, engine.Settings(n_contrib=1, n_reps=1)),
             (m.setup(), q, I, sig, engine.Settings(**{**st.__dict__, "seed": 4}))]
    got = engine.analyse_batch(mixed)
    for pr, g_ in zip(mixed, got):
        one = engine.analyse(*pr[:4], engine.Settings(**{**pr[4].__dict__, "exec_mode": engine.EXEC_WAVE}))
        for name in ("contribs", "fit", "chisq", "num_iter", "scaling"):
            np.testing.assert_array_equal(getattr(g_, name), getattr(one, name), err_msg=name)
    # a Python-only model: ValueError before any launch; run_series(batch=True) falls back to the data sets one after the other
    py = _PythonOnlySphere(); py.radius.setActiveRange(tuple(x[0] for x in RANGES["sphere"]))
    data = mcsas_amd.SASData(q, I, sig)
    with pytest.raises(ValueError):
        engine.analyse_batch([(m.setup(), q, I, sig, st), (py.setup(data), q, I, sig, st)])
    outs = []
    for batch in (False, True):
        algo = mcsas_amd.McSAS(seed=9)
        algo.numContribs.setValue(30); algo.numReps.setValue(2); algo.maxIterations.setValue(200)
        algo.convergenceCriterion.setValue(1e-9); algo.maxRetries.setValue(0); algo.showIncomplete.setValue(True)
        algo.model = py
        outs.append(mcsas_amd.run_series(algo, [mcsas_amd.SASData(q, I, sig), mcsas_amd.SASData(q, 2 * I, sig)], batch=batch)[0])
    for a_, b_ in zip(*outs):
        assert np.array_equal(a_["contribs"], b_["contribs"]) and np.array_equal(a_["fitMeasValMean"], b_["fitMeasValMean"])

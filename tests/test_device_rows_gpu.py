"""GPU tests of the chains whose rows the caller produces ON THE DEVICE (mcsas_hip_analyse_device_rows, csrc/chain_feed.h:
feed_draw_kernel + feed_rows_kernel): models typed in torch against the reference's replayed chain, the numpy oracle, the built-in
kernels and the host-rows entry point with the numpy twins of tests/test_parity_gpu.py.  Tolerances are those of the host-rows
tests there: decisions, counters and draws exact; parameter sets 1e-13 (exact where the proposals are the device's own); chi² 1e-9."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch                        # ahead of the library's first load: one HIP runtime in the process (engine._one_hip_runtime)
import mcsas_amd
from mcsas_amd import engine
from mcsas_amd import _lib
from mcsas_amd.scatteringmodels import batch_clip, host_model_calc
from oracle import mcsas_oracle as O
from helpers import load, make_models, traj_setup
from test_parity_gpu import PythonOnlySphere, PythonOnlyCoreShell


class TorchSphere(mcsas_amd.SASModel):
    """PythonOnlySphere (models/sphere.py:12-63) typed in torch: declarations + the batch form of calcIntensity, nothing else."""
    shortName = "Sphere (torch)"
    canSmear = True
    parameters = mcsas_amd.Sphere.parameters

    def __init__(self):
        super().__init__()
        self.radius.setActive(True)

    def calcIntensityBatch(self, q, pset, compensationExponent):
        import torch
        r = pset[:, 0]
        vol = (np.pi * 4. / 3.) * r**3
        v = vol * self.sld()**2
        w = vol ** (2 * compensationExponent)
        s = 4. * np.pi * r * r
        qr = q[None, :] * r[:, None]
        ff = 3. * (torch.sin(qr) - qr * torch.cos(qr)) / (qr**3)
        return ff**2 * w[:, None], v, w, s


class TorchCoreShell(mcsas_amd.SASModel):
    """PythonOnlyCoreShell (models/sphericalcoreshell.py:14-77) typed in torch; two active parameters, exponential generators."""
    shortName = "Core-shell sphere (torch)"
    parameters = PythonOnlyCoreShell.parameters

    def __init__(self):
        super().__init__()
        self.radius.setActive(True); self.t.setActive(True)

    def calcIntensityBatch(self, q, pset, compensationExponent):
        import torch
        r, rt = pset[:, 0], pset[:, 0] + pset[:, 1]

        def k(rr, d_eta):
            qr = q[None, :] * rr[:, None]
            return d_eta * 3 * (torch.sin(qr) - qr * torch.cos(qr)) / (qr)**3
        vc = 4. / 3 * np.pi * r**3
        vt = 4. / 3 * np.pi * rt**3
        ff = k(rt, self.eta_s() - self.eta_sol()) - (vc / vt)[:, None] * k(r, self.eta_s() - self.eta_c())
        w = vt ** (2 * compensationExponent)
        return ff**2 * w[:, None], vt, w, torch.zeros_like(vt)


def torch_rows(model, q, c):
    """row_fn of engine.analyse_device_rows for a batch model: fills the rows view in place."""
    qd = []

    def fn(pset, out):
        import torch
        if not qd:
            qd.append(torch.as_tensor(np.ascontiguousarray(q, dtype=np.float64), device=pset.device))
        out.copy_(model.calcIntensityBatch(qd[0], batch_clip(model, pset), c)[0])
    return fn


def numpy_rows(model, data, c):
    return lambda pset: host_model_calc(model, data, pset, c, want_rows=True)[4]


def same_chains(a, b, exact_sets=True):
    for f in ("num_iter", "num_moves", "attempts", "draws", "converged"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    if exact_sets:
        np.testing.assert_array_equal(a.contribs, b.contribs)
    else:
        np.testing.assert_allclose(a.contribs, b.contribs, rtol=1e-13)
    np.testing.assert_allclose(a.chisq, b.chisq, rtol=1e-9)
    np.testing.assert_allclose(a.fit, b.fit, rtol=1e-9)


def sphere_pair(g, cls=TorchSphere):
    lo, hi = float(g["spec_lo"][0]), float(g["spec_hi"][0])
    m = cls(); m.radius.setActiveRange((lo, hi)); m.sld.setValue(float(g["spec_sld"]))
    _, spec = make_models("sphere", [lo], [hi], sld=float(g["spec_sld"]))
    return m, spec


def test_torch_model_replays_the_reference_through_device_rows():
    """A ScatteringModel that brings only calcIntensityBatch runs through McSAS.calc(): proposals generated on the device, the rows
    of a round by the model's torch lines, every decision on the device.  Fed the uniform stream the reference consumed it
    reproduces the reference's chain and equals the built-in sphere kernel on the same stream; histogram() works on the result.
    100 q-points: rows of 128 doubles with 28 padding columns; a window of 37 does not divide the budget."""
    g, m_builtin, spec, st, ost = traj_setup("g4_sphere_q100_fixed.npz")
    assert mcsas_amd.scatteringmodels.is_host_model(TorchSphere())
    out = {}
    for tag, cls in (("torch", TorchSphere), ("builtin", mcsas_amd.Sphere)):
        m = cls()
        lo, hi = float(g["spec_lo"][0]), float(g["spec_hi"][0])
        m.radius.setActiveRange((lo, hi)); m.sld.setValue(float(g["spec_sld"]))
        m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=20, xscale='log', yweight='vol'))
        algo = mcsas_amd.McSAS(seed=1)
        algo.numContribs.setValue(st.n_contrib); algo.numReps.setValue(1); algo.maxIterations.setValue(st.max_iter)
        algo.convergenceCriterion.setValue(st.conv_crit); algo.compensationExponent.setValue(st.comp_exp); algo.showIncomplete.setValue(True)
        algo.maxRetries = mcsas_amd.mcsas._Setting("maxRetries", 0)
        algo.hostRowWindow = 37
        algo.model = m
        algo.data = mcsas_amd.SASData(g["data_q"], g["data_I"], g["data_sigma"], f_limit=g["data_f_limit"])
        algo.calc(replay=g["stream"][None, :])
        d = algo.details
        out[tag] = (algo.result[0]["contribs"].copy(), d.chisq.copy(), np.asarray(m.radius.histograms()[0].bins.mean).copy())
        assert d.num_iter[0] == int(g["res_num_iter"]) and d.num_moves[0] == int(g["res_num_moves"]), tag
        np.testing.assert_allclose(algo.result[0]["contribs"][:, :, 0], g["res_rset"], rtol=1e-15)
        np.testing.assert_allclose(d.chisq[0], float(g["res_conval"]), rtol=1e-9)
    np.testing.assert_array_equal(out["torch"][0], out["builtin"][0])
    np.testing.assert_allclose(out["torch"][2], out["builtin"][2], rtol=1e-9, atol=1e-300)


FREE = dict(n_contrib=60, n_reps=5, max_iter=400, conv_crit=350.0, max_retries=2, seed=77, rep_offset=3)


@pytest.fixture(scope="module")
def free_run():
    """The free-running workload of test_python_only_model_free_running_retries_and_stop through the engine, capacity = useful_rows."""
    g = load("g4_sphere_q100_fixed.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    m, spec = sphere_pair(g)
    data = mcsas_amd.SASData(q, I, sig, f_limit=g["data_f_limit"])
    st = engine.Settings(**FREE)
    setup = m.setup(data)
    shape = engine.device_rows_shape(setup, q, st, 50)
    assert shape == (60, 300, 128)
    res = engine.analyse_device_rows(setup, q, I, sig, st, torch_rows(m, q, st.comp_exp), window=50, capacity=shape[1])
    return dict(g=g, q=q, I=I, sig=sig, m=m, spec=spec, data=data, st=st, setup=setup, res=res)


def test_free_running_retries_rounds_stop_and_a_raising_callback(free_run):
    """Several chains with a criterion some reach within the budget and some only in a later attempt, against the numpy oracle on
    the same Philox streams; one chain per round (capacity = min_rows) gives the same results as all chains per round; McSAS.stop
    raised inside the third callback ends every chain where it is; an exception in row_fn comes back to the caller."""
    f = free_run
    g, q, I, sig, st, res = f["g"], f["q"], f["I"], f["sig"], f["st"], f["res"]
    ost = O.Settings(n_contrib=60, n_reps=1, max_iter=400, conv_crit=350.0, max_retries=2)
    attempts = []
    for r in range(5):
        stream = O.PhiloxStream(77, 3 + r)
        for att in range(3):
            ref = O.mc_fit(f["spec"], q, I, sig, g["data_f_limit"], g["data_x0_limit"], ost, stream, method="closed")
            if ref.conval <= 350.0:
                break
        attempts.append(att + 1)
        assert res.attempts[r] == att + 1 and res.num_iter[r] == ref.num_iter and res.num_moves[r] == ref.num_moves, r
        assert res.draws[r] == stream.pos
        np.testing.assert_allclose(res.contribs[:, :, r], ref.rset, rtol=1e-13)
        np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-9)
    assert sorted(set(attempts)) == [1, 2, 3] and res.converged.sum() == 4
    # one chain per round: many rounds, the same chains
    rounds = []
    fill = torch_rows(f["m"], q, st.comp_exp)

    def counted(pset, out):
        rounds.append(len(pset))
        return fill(pset, out)
    one = engine.analyse_device_rows(f["setup"], q, I, sig, st, counted, window=50, capacity=60)
    assert max(rounds) <= 60 and len(rounds) >= 2 * int(res.attempts.sum())      # (an initial set and at least one window per attempt)
    same_chains(one, res)
    np.testing.assert_array_equal(one.chisq, res.chisq)
    np.testing.assert_array_equal(one.fit, res.fit)
    # stop: raised inside the third callback
    stop = C.c_int32(0)
    calls = []

    def rows_then_stop(pset, out):
        calls.append(len(pset))
        if len(calls) == 3:
            stop.value = 1
        return fill(pset, out)
    st2 = engine.Settings(n_contrib=60, n_reps=4, max_iter=100000, conv_crit=0.0, max_retries=0, seed=5)
    res2 = engine.analyse_device_rows(f["setup"], q, I, sig, st2, rows_then_stop, stop=stop, window=40)
    assert calls == [240, 160, 160] and (res2.num_iter == 80).all() and (res2.converged == 0).all() and np.isfinite(res2.chisq).all()

    def bad(pset, out):
        raise ZeroDivisionError("model failed")
    with pytest.raises(ZeroDivisionError):
        engine.analyse_device_rows(f["setup"], q, I, sig, st2, bad)


def test_proposals_are_the_wave_kernels_with_exponential_generators():
    """Two active parameters with RandomExponential generators, 1300 q-points (rows of 1344 doubles): the proposals come from the
    device's own draw source and generator transform, so the accepted sets are bit for bit those of the built-in core-shell kernel
    run one wavefront per chain on the same seed — which the host-rows path, whose pow is the host's, cannot promise."""
    q = np.logspace(7, np.log10(3e9), 1300)
    rs = np.random.RandomState(5)
    m = TorchCoreShell()
    lo, hi = [2e-9, 5e-10], [1e-7, 2e-8]
    m.radius.setActiveRange((lo[0], hi[0])); m.t.setActiveRange((lo[1], hi[1]))
    assert len(m.params()) == 11 and mcsas_amd.scatteringmodels.is_host_model(m)
    builtin, spec = make_models("sphcs", lo, hi)
    truth = np.stack([rs.uniform(5e-9, 5e-8, 30), rs.uniform(1e-9, 1e-8, 30)], axis=1)
    It = O.model_calc(spec, q, truth, 0.6666666)[0]
    It *= 1e3 / It.max()
    sig = 0.02 * It
    I = It * (1 + 0.02 * rs.normal(size=len(q)))
    data = mcsas_amd.SASData(q, I, sig)
    st = engine.Settings(n_contrib=40, n_reps=3, max_iter=150, conv_crit=1e-9, max_retries=1, seed=9)
    setup = m.setup(data)
    assert tuple(setup.gen_kind) == (engine.GEN_EXP1, engine.GEN_EXP1) == tuple(builtin.setup(data).gen_kind)
    assert engine.device_rows_shape(setup, q, st, 33) == (40, 120, 1344)
    res = engine.analyse_device_rows(setup, q, I, sig, st, torch_rows(m, q, st.comp_exp), window=33)
    ref = engine.analyse(builtin.setup(data), q, I, sig, replace(st, exec_mode=engine.EXEC_WAVE))
    assert (res.attempts == 2).all() and (res.num_iter == 150).all() and (res.num_moves > 0).all()
    same_chains(res, ref)


MID_WINDOW_CRITERION = 2000.0       # the replayed chain of 60 contributions passes it at step 158 (the oracle below): 30 steps into a window of 64


def test_flags_and_stream_end():
    """startFromMinimum (no draws for the initial set), no background, positiveBackground against the numpy oracle on the same
    replayed stream; a replay stream is exhausted if and only if a step the chain TOOK needed a draw behind its end — also for a
    chain that converges in the middle of a window whose proposals were drawn ahead."""
    g = load("g4_sphere_q100_fixed.npz")
    q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
    m, spec = sphere_pair(g)
    data = mcsas_amd.SASData(q, I, sig, f_limit=g["data_f_limit"])
    fill = torch_rows(m, q, 0.6666666)
    stream = g["stream"][:60 + 300 + 4]
    for flags in (dict(start_from_minimum=True), dict(find_background=False), dict(positive_background=True)):
        st = engine.Settings(n_contrib=60, n_reps=1, max_iter=300, conv_crit=1e-9, max_retries=0, **flags)
        res = engine.analyse_device_rows(m.setup(data), q, I, sig, st, fill, replay=stream[None, :], window=64)
        ost = O.Settings(n_contrib=60, n_reps=1, max_iter=300, conv_crit=1e-9, find_bg=st.find_background, pos_bg=st.positive_background,
                         start_from_min=st.start_from_minimum)
        ref = O.mc_fit(spec, q, I, sig, g["data_f_limit"], g["data_x0_limit"], ost, O.ReplayStream(stream), method="closed")
        assert res.num_iter[0] == ref.num_iter == 300 and res.num_moves[0] == ref.num_moves, flags
        assert res.draws[0] == (300 if st.start_from_minimum else 360)
        np.testing.assert_allclose(res.contribs[:, :, 0], ref.rset, rtol=1e-13)
        np.testing.assert_allclose(res.chisq[0], ref.conval, rtol=1e-9)
        np.testing.assert_allclose([res.scaling[0], res.background[0]], [ref.scaling, ref.background], rtol=1e-8, atol=1e-300)
    # the chain that runs out its budget consumed 360 draws: one short is reported, exactly as long is not
    st = engine.Settings(n_contrib=60, n_reps=1, max_iter=300, conv_crit=1e-9, max_retries=0)
    with pytest.raises(_lib.McSASHipError) as e:
        engine.analyse_device_rows(m.setup(data), q, I, sig, st, fill, replay=stream[None, :359], window=64)
    assert e.value.code == -5                                   # MCSAS_ESTREAM
    res = engine.analyse_device_rows(m.setup(data), q, I, sig, st, fill, replay=stream[None, :360], window=64)
    assert res.draws[0] == 360 and res.num_iter[0] == 300
    # a chain that converges mid-window: the proposals of the rest of its window were drawn behind the stream's end, none was used
    st = replace(st, conv_crit=MID_WINDOW_CRITERION)
    ost = O.Settings(n_contrib=60, n_reps=1, max_iter=300, conv_crit=MID_WINDOW_CRITERION)
    ref = O.mc_fit(spec, q, I, sig, g["data_f_limit"], g["data_x0_limit"], ost, O.ReplayStream(stream), method="closed")
    k = ref.num_iter
    assert 0 < k < 300 and k % 64 not in (0, 63)
    res = engine.analyse_device_rows(m.setup(data), q, I, sig, st, fill, replay=stream[None, :60 + k], window=64)
    assert res.num_iter[0] == k and res.draws[0] == 60 + k and res.converged[0] == 1 and res.num_moves[0] == ref.num_moves
    with pytest.raises(_lib.McSASHipError) as e:
        engine.analyse_device_rows(m.setup(data), q, I, sig, st, fill, replay=stream[None, :60 + k - 1], window=64)
    assert e.value.code == -5


def test_the_padding_is_the_librarys(free_run):
    """The library called directly with a rows tensor full of NaN: it zeroes the buffer itself, the callback writes the nq = 100
    real columns only, and the 28 padding columns of every row stay out of the sums — the results are those of the engine path."""
    import torch
    f = free_run
    q, st = f["q"], f["st"]
    lib = _lib.load()
    prob = engine.HipProblem(f["setup"], q, f["I"], f["sig"], st)
    prob.c.model_id = engine.MODEL_HOST
    res = engine.ChainResults(st.n_contrib, 1, st.n_reps, 100)
    lo, hi, stride = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    assert lib.mcsas_hip_device_rows_shape(C.byref(prob.c), 50, C.byref(lo), C.byref(hi), C.byref(stride)) == 0
    assert (lo.value, hi.value, stride.value) == (60, 300, 128)
    dev = torch.device("cuda", torch.cuda.current_device())
    pset = torch.full((hi.value, 1), float("nan"), dtype=torch.float64, device=dev)
    rows = torch.full((hi.value, stride.value), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    qd = torch.as_tensor(q, device=dev)
    errors = []

    def cb(user, n):
        try:
            rows[:n, :100] = f["m"].calcIntensityBatch(qd, batch_clip(f["m"], pset[:n]), st.comp_exp)[0]
            torch.cuda.synchronize()
            return 0
        except BaseException as e:
            errors.append(e)
            return 1
    rc = lib.mcsas_hip_analyse_device_rows(C.byref(prob.c), C.c_void_p(pset.data_ptr()), C.c_void_p(rows.data_ptr()), hi.value,
                                           _lib.DeviceRowsCallback(cb), None, 50, C.byref(res.c))
    assert not errors and rc == 0, (errors, lib.mcsas_hip_last_error())
    assert np.isfinite(res.chisq).all() and np.isfinite(res.fit).all() and np.isfinite(res.contribs).all()
    assert bool((rows[:, 100:] == 0).all())                     # (the padding is still the library's zeros)
    for name in ("contribs", "fit", "chisq", "scaling", "background", "num_iter", "num_moves", "attempts", "converged", "draws"):
        np.testing.assert_array_equal(getattr(res, name), getattr(f["res"], name), err_msg=name)


@pytest.mark.parametrize("nq, n_contrib", [(64, 60), (100, 1)])
def test_no_padding_and_a_chain_that_cannot_step(nq, n_contrib):
    """64 q-points exactly (rows without padding) and one contribution (a chain that cannot step: mcsas.py:354 never enters the
    loop): answered as mcsas_hip_analyse_host_rows answers them with the numpy twin of the model."""
    g = load("g4_sphere_q100_fixed.npz")
    q, I, sig = g["data_q"][:nq], g["data_I"][:nq], g["data_sigma"][:nq]
    mt, _ = sphere_pair(g)
    mn, _ = sphere_pair(g, PythonOnlySphere)
    data = mcsas_amd.SASData(q, I, sig)
    st = engine.Settings(n_contrib=n_contrib, n_reps=3, max_iter=200, conv_crit=1e-9, max_retries=1, seed=11)
    assert engine.device_rows_shape(mt.setup(data), q, st, 48) == (max(n_contrib, 48), 3 * max(n_contrib, 48), (nq + 63) // 64 * 64)
    res = engine.analyse_device_rows(mt.setup(data), q, I, sig, st, torch_rows(mt, q, st.comp_exp), window=48)
    ref = engine.analyse_host_rows(mn.setup(data), q, I, sig, st, numpy_rows(mn, data, st.comp_exp), window=48)
    assert (ref.attempts == 2).all() and (ref.num_iter == (0 if n_contrib == 1 else 200)).all()
    same_chains(res, ref)                                       # (a uniform generator: the host's proposals are the device's)
    np.testing.assert_allclose([res.scaling, res.background], [ref.scaling, ref.background], rtol=1e-8, atol=1e-300)

"""Where a replayed random stream ends, in every execution path.

A chain is over the moment it converges, runs out of steps, is stopped or runs out of replayed random numbers; every execution
path but one wavefront per chain draws and evaluates proposals AHEAD of that moment (a window of the pipeline, of the workgroup
kernel's producer waves, 64 proposals of the wave and q-split kernels, `window` steps of the host-rows entry point).  The contract:

  * a replay stream is exhausted (MCSAS_ESTREAM) if and only if a step the chain TOOK — or the initial set of an attempt it made —
    needed a draw at an index >= replay_len;
  * no draw the chain did not consume reaches a result.

Part A runs chains that end in the middle of a window on a stream exactly as long as they consumed (MCSAS_OK, the oracle's chain),
on the long stream (the same arrays, bit for bit) and on a stream one draw short (MCSAS_ESTREAM), in every path.  Part B: rows with
an integral give the same arrays whatever window the pipeline speculates in (the MCSAS_HIP_PIPE_KB knob, the few-chains rule).

Every choice made with the oracle on the CPU (seeds, criteria, the attempts and draws they give) is asserted on the oracle's own
output where the workload is built, so that a change of the oracle cannot turn a mid-window end into an end-of-budget one unnoticed."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mcsas_amd
from mcsas_amd import engine, _lib
from oracle import mcsas_oracle as O
from helpers import load, make_models, traj_setup, FakeData, GEN_CLS
from test_parity_gpu import PythonOnlySphere, RANDOM_RANGES, _synthetic

FIELDS = ("contribs", "fit", "chisq", "scaling", "background", "num_iter", "num_moves", "attempts", "converged", "draws")
MCSAS_ESTREAM = -5

# execution paths: (id, settings that select it the way the existing tests do, entry point)
PATHS = {
    "wave": dict(kw=dict(waves_per_chain=1, cache_intensities=1)),
    "wave_nocache": dict(kw=dict(waves_per_chain=1, cache_intensities=0)),
    "wg8": dict(kw=dict(waves_per_chain=8, cache_intensities=1)),
    "wg3": dict(kw=dict(waves_per_chain=3, cache_intensities=1)),
    "pipe": dict(kw=dict(exec_mode=engine.EXEC_PIPELINE)),              # sphere: no row queue
    "pipe_rowq": dict(kw=dict(exec_mode=engine.EXEC_PIPELINE)),         # a model with an integral: row queue
    "wide": dict(kw=dict(exec_mode=engine.EXEC_WORKGROUP)),             # nq > 1024: the q-split workgroup kernel
    "batch": dict(kw=dict(exec_mode=engine.EXEC_AUTO)),
    "host37": dict(kw={}, window=37),
    "host64": dict(kw={}, window=64),
}
SPHERE_PATHS = ("wave", "wave_nocache", "wg8", "wg3", "pipe", "batch", "host37", "host64")


def _oracle_chain(spec, q, I, sig, f_limit, x0_limit, ost, stream, retries):
    """McSAS.analyse's retry loop for one chain -> dict(attempts, iters per attempt, draws after each attempt, last ChainResult)."""
    iters, pos = [], []
    while True:
        ref = O.mc_fit(spec, q, I, sig, f_limit, x0_limit, ost, stream, method="closed")
        iters.append(ref.num_iter); pos.append(stream.pos)
        if ref.conval <= ost.conv_crit or len(iters) > retries:
            break
    return dict(attempts=len(iters), iters=iters, pos=pos, ref=ref, converged=int(ref.conval <= ost.conv_crit))


@functools.lru_cache(maxsize=None)
def _workload(name):
    """One workload of Part A, its oracle chains computed once and shared: dict(setup, q, I, sig, st, replay [R][L], chains,
    draws [R], draws_first [R] (what the first attempt alone consumes: the one-draw-short run has no retries), g (fixture or None),
    host (-> (setup, rows callback) of the same model typed as Python, sphere only))."""
    wl = dict(g=None, host=None)
    if name in ("a1_sphere", "a1_cyl"):
        # A1: chains the reference ENDED BY CONVERGENCE, replayed; one chain each
        g, m, spec, st, ost = traj_setup("g4_sphere_q100_converge.npz" if name == "a1_sphere" else "g17_cyl_q100_converge.npz")
        q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
        ch = _oracle_chain(spec, q, I, sig, g["data_f_limit"], g["data_x0_limit"], ost, O.ReplayStream(g["stream"]), 0)
        N, P, it = ost.n_contrib, spec.n_active, ch["ref"].num_iter
        assert it == int(g["res_num_iter"]) == (7827 if name == "a1_sphere" else 6228) and ch["ref"].num_moves == int(g["res_num_moves"])
        assert ch["converged"] and it < ost.max_iter                         # ended by convergence, not by the budget
        assert ch["pos"][-1] == P * (N + it) == len(g["stream"]) - 8           # (the recorded stream has eight spare draws)
        wl.update(setup=m.setup(FakeData(q)), q=q, I=I, sig=sig, st=st, replay=np.array(g["stream"][None, :]), chains=[ch], g=g, spec=spec)
        if name == "a1_sphere":
            def host():
                hm = PythonOnlySphere()
                hm.radius.setActiveRange((float(g["spec_lo"][0]), float(g["spec_hi"][0]))); hm.sld.setValue(float(g["spec_sld"]))
                hm.radius.setGenerator(GEN_CLS[int(g["spec_gen"][0])])
                data = mcsas_amd.SASData(q, I, sig, f_limit=g["data_f_limit"])
                return hm.setup(data), lambda pset: mcsas_amd.scatteringmodels.host_model_calc(hm, data, pset, st.comp_exp, want_rows=True)[4]
            wl["host"] = host
    elif name in ("a2_sphere", "a2_cyl", "a2_sphere_one", "a2_cyl_one"):
        # A2: five chains with different ends and retries in one launch; the Philox draws written out as a replay array.  The array
        # is rectangular, as long as the longest consumption, so only the chain that consumes most sees it END; `_one` is the chain
        # of the five that converges in its THIRD attempt, alone on a row exactly as long as it consumed: the array ends behind a
        # mid-window convergence that two retry hand-overs (and two further initial sets) precede.
        seed, first, R, N, steps, retries = 77, 3, 5, 60, 400, 2
        if name.startswith("a2_sphere"):
            g = load("g4_sphere_q100_fixed.npz")
            q, I, sig = g["data_q"], g["data_I"], g["data_sigma"]
            lo, hi = [float(g["spec_lo"][0])], [float(g["spec_hi"][0])]
            m, spec = make_models("sphere", lo, hi, sld=float(g["spec_sld"]))
            lim, crit = (g["data_f_limit"], g["data_x0_limit"]), 350.0
            expect = dict(attempts=[3, 2, 1, 3, 1], converged=[1, 1, 1, 0, 1], one=0)

            def host():
                hm = PythonOnlySphere(); hm.radius.setActiveRange((lo[0], hi[0])); hm.sld.setValue(float(g["spec_sld"]))
                data = mcsas_amd.SASData(q, I, sig, f_limit=g["data_f_limit"])
                return hm.setup(data), lambda pset: mcsas_amd.scatteringmodels.host_model_calc(hm, data, pset, 0.6666666, want_rows=True)[4]
            wl["host"] = host
        else:
            q, I, sig = _synthetic(40)
            m, spec = make_models("cyl_aspect", *RANDOM_RANGES["cyl_aspect"], intDiv=20.)
            lim, crit = ([I.min(), I.max()], [q.min(), q.max()]), 5900.0
            # (chosen with the oracle: chain 1 converges in its third attempt, at step 369; the others in their first)
            expect = dict(attempts=[1, 3, 1, 1, 1], converged=[1, 1, 1, 1, 1], one=1)
        if name.endswith("_one"):
            first, R = first + expect["one"], 1
            expect = dict(attempts=[3], converged=[1])
        ost = O.Settings(n_contrib=N, n_reps=1, max_iter=steps, conv_crit=crit, max_retries=retries)
        chains = [_oracle_chain(spec, q, I, sig, lim[0], lim[1], ost, O.PhiloxStream(seed, first + r), retries) for r in range(R)]
        assert [c["attempts"] for c in chains] == expect["attempts"] and [c["converged"] for c in chains] == expect["converged"]
        assert len({c["attempts"] for c in chains}) >= 2 or name.endswith("_one")
        if name.endswith("_one"):
            assert chains[0]["iters"][:2] == [steps, steps] and chains[0]["iters"][2] < steps     # third attempt ends by convergence
        L = max(c["pos"][-1] for c in chains)
        replay = np.stack([O.philox_uniform(seed, first + r, np.arange(L, dtype=np.uint64)) for r in range(R)])
        st = engine.Settings(n_contrib=N, n_reps=R, max_iter=steps, conv_crit=crit, max_retries=retries)
        wl.update(setup=m.setup(), q=q, I=I, sig=sig, st=st, replay=replay, chains=chains, spec=spec)
    elif name == "a3":
        # A3: the q-split kernel (more than 1024 q-points), two chains that converge inside their second batch of 64 proposals
        q, I, sig = _synthetic(1500)
        m, spec = make_models("sphere", [np.pi / q.max()], [np.pi / q.min()])
        seed, R, N, steps, crit = 5, 2, 40, 120, 320.0
        ost = O.Settings(n_contrib=N, n_reps=1, max_iter=steps, conv_crit=crit, max_retries=0)
        chains = [_oracle_chain(spec, q, I, sig, [I.min(), I.max()], [q.min(), q.max()], ost, O.PhiloxStream(seed, r), 0) for r in range(R)]
        assert [c["iters"] for c in chains] == [[81], [104]] and all(c["converged"] for c in chains)      # (before step 120, both)
        L = max(c["pos"][-1] for c in chains)
        replay = np.stack([O.philox_uniform(seed, r, np.arange(L, dtype=np.uint64)) for r in range(R)])
        st = engine.Settings(n_contrib=N, n_reps=R, max_iter=steps, conv_crit=crit, max_retries=0)
        wl.update(setup=m.setup(), q=q, I=I, sig=sig, st=st, replay=replay, chains=chains, spec=spec)
    else:
        raise KeyError(name)
    P, N = wl["spec"].n_active, wl["st"].n_contrib
    wl["draws"] = np.array([c["pos"][-1] for c in wl["chains"]], dtype=np.int64)
    wl["draws_first"] = np.array([c["pos"][0] for c in wl["chains"]], dtype=np.int64)
    for c in wl["chains"]:                                                  # N·P per attempt plus P per step
        assert c["pos"][-1] == P * (N * c["attempts"] + sum(c["iters"]))
    wl["replay"].setflags(write=False)
    return wl


def _mid_window(wl, window):
    """Every attempt that ends before the budget does (by convergence) ends INSIDE a window of `window` steps: the path has drawn
    proposals the chain never took.  (Behind the budget nothing is drawn, in any path.)"""
    early = [n for c in wl["chains"] for n in c["iters"] if n < wl["st"].max_iter]
    assert early and all(n % window != 0 for n in early), (early, window)


def _exact_fit(wl):
    """The replay array cut to the longest consumption; what a shorter chain did not consume replaced by OTHER uniforms in [0, 1)."""
    draws = wl["draws"]
    out = np.array(wl["replay"][:, :int(draws.max())])
    for r, d in enumerate(draws):
        u = out[r, d:]
        v = np.minimum(1.0 - u, np.nextafter(1.0, 0.0))
        v[v == u] = 0.25
        assert ((v >= 0.0) & (v < 1.0) & (v != u)).all()
        out[r, d:] = v
    return out


def _run(wl, path, replay, **over):
    """The workload on `replay` through execution path `path` -> ChainResults (raises McSASHipError as the entry points do)."""
    sel = PATHS[path]
    st = engine.Settings(**{**wl["st"].__dict__, **sel["kw"], **over})
    if path.startswith("host"):
        setup, rows = wl["host"]()
        return engine.analyse_host_rows(setup, wl["q"], wl["I"], wl["sig"], st, rows, replay=replay, window=sel["window"])
    if path == "batch":
        # beside it in the launch: a free-running data set of another shape (the batch's second group)
        q2, I2, sig2 = _synthetic(64)
        m2, _ = make_models("sphere", [np.pi / q2.max()], [np.pi / q2.min()])
        other = dict(model=m2.setup(), q=q2, intensity=I2, sigma=sig2,
                     st=engine.Settings(n_contrib=40, n_reps=2, max_iter=100, conv_crit=1e-9, max_retries=0, seed=1))
        return engine.analyse_batch([other, dict(model=wl["setup"], q=wl["q"], intensity=wl["I"], sigma=wl["sig"], st=st, replay=replay)])[1]
    return engine.analyse(wl["setup"], wl["q"], wl["I"], wl["sig"], st, replay=replay)


def _window_of(wl, path):
    """Steps the path draws ahead: the library's own answer for the pipeline and the workgroup kernel, 64 for the others — and
    the check that the settings select the path they are meant to (Plan.info: the mode the library chose)."""
    if path.startswith("host"):
        assert wl["host"]()[0].model_id == engine.MODEL_HOST
        return PATHS[path]["window"]
    # (the batch entry point runs a problem as MCSAS_EXEC_WAVE does: the plan of that mode stands for it)
    kw = dict(exec_mode=engine.EXEC_WAVE) if path == "batch" else PATHS[path]["kw"]
    plan = engine.Plan(wl["setup"], wl["q"], wl["I"], wl["sig"], engine.Settings(**{**wl["st"].__dict__, **kw}), replay=wl["replay"])
    info = plan.info
    plan.close()
    nq = len(wl["q"])
    if path in ("wg8", "wg3", "pipe", "pipe_rowq"):
        assert info["exec_mode"] == ("pipeline" if path.startswith("pipe") else "workgroup") and info["window"] > 1, info
        assert nq <= 1024 and (path not in ("wg8", "wg3") or info["waves_per_chain"] == int(path[2:])), info
        return info["window"]
    if path == "wide":                                                      # the q-split kernel: the q-points over the workgroup's waves
        assert nq > 1024 and info["exec_mode"] == "workgroup" and info["waves_per_chain"] > 1, info
        assert info["q_per_lane"] * 64 * info["waves_per_chain"] >= nq, info
    else:
        assert info["exec_mode"] == "wave" and info["cached_rows"] == (path != "wave_nocache"), info
    return 64


def _check_against_oracle(wl, res):
    for r, c in enumerate(wl["chains"]):
        ref = c["ref"]
        got = (res.num_iter[r], res.num_moves[r], res.attempts[r], res.converged[r], res.draws[r])
        print("chain %d: iter, moves, attempts, converged, draws = %s; oracle %s" % (r, got, (ref.num_iter, ref.num_moves, c["attempts"], c["converged"], c["pos"][-1])))
        assert got == (ref.num_iter, ref.num_moves, c["attempts"], c["converged"], c["pos"][-1]), r
        np.testing.assert_allclose(res.contribs[:, :, r], ref.rset, rtol=1e-12)
        np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-7)
    g = wl["g"]
    if g is not None:                                                      # the reference's own record of the chain (A1)
        assert res.num_iter[0] == int(g["res_num_iter"]) and res.num_moves[0] == int(g["res_num_moves"])
        np.testing.assert_allclose(res.contribs[:, :, 0], g["res_rset"], rtol=1e-12)
        np.testing.assert_allclose(res.chisq[0], float(g["res_conval"]), rtol=1e-7)
        np.testing.assert_allclose(res.fit[:, 0], g["res_fit"], rtol=1e-6, atol=1e-12 * np.abs(g["res_fit"]).max())
        np.testing.assert_allclose(res.scaling[0], float(g["res_scaling"]), rtol=1e-6)


def _same_arrays(a, b, what):
    for name in FIELDS:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg="%s: %s" % (what, name))


A_CASES = ([("a1_sphere", p) for p in SPHERE_PATHS] + [("a1_cyl", "pipe_rowq"), ("a1_cyl", "wave")]
           + [("a2_sphere", p) for p in SPHERE_PATHS] + [("a2_cyl", "pipe_rowq"), ("a2_cyl", "wave")]
           + [("a2_sphere_one", p) for p in SPHERE_PATHS] + [("a2_cyl_one", "pipe_rowq"), ("a2_cyl_one", "wave")] + [("a3", "wide")])


@pytest.mark.parametrize("name,path", A_CASES)
def test_stream_exactly_as_long_as_the_chain_consumed(name, path):
    """(1) On a replay array cut to the longest consumption — what the shorter chains left over replaced by other uniforms — every
    path returns MCSAS_OK and the oracle's chains: iterations, moves, attempts, converged, draws exact, contributions 1e-12, chi²
    1e-7 (A1: the reference's recorded results too).  (2) The same path on the long, untouched stream returns the same arrays bit
    for bit: no draw a chain did not consume reaches a result.  Every attempt ends inside a window of the path, so proposals WERE
    drawn from behind the consumed end.  a1_sphere through host37 / host64 is ADVICE.md round 5's case: mcsas_hip_analyse_host_rows
    on stream[:draws] — MCSAS_ESTREAM before this test existed (overflow was latched when a window was drawn, not when a step was taken).
    Which cases show what: a FALSE overflow report can only come from a row that ends where its chain stopped — A1, A3's longer
    chain and the `_one` cases (a convergence in a third attempt: the retry hand-over and the initial sets' overflow words are on the
    way).  In the five-chain A2 arrays (rectangular, as long as the longest consumption) the row that ends is a chain's that ran to
    the budget in every attempt (a2_sphere) or chain 1's (a2_cyl, asserted by `_one`); their other chains, with overwritten
    left-overs, show that unconsumed draws reach no result."""
    wl = _workload(name)
    _mid_window(wl, _window_of(wl, path))
    fit = _run(wl, path, _exact_fit(wl))                                    # (raises on MCSAS_ESTREAM)
    _check_against_oracle(wl, fit)
    _same_arrays(fit, _run(wl, path, wl["replay"]), "exact fit vs. long stream")


@pytest.mark.parametrize("name,path", A_CASES)
def test_stream_one_draw_short_is_reported(name, path):
    """(3) One draw fewer than the longest chain consumes (no retries: what the first attempts consume): the step that needed it was
    taken — on 0.5 in the draw's place —, so every path reports MCSAS_ESTREAM.  (The chain that lost its draw may go on, on 0.5
    for every further draw, to the end of the budget: the budget of this run ends 100 steps behind the longest first attempt.)
    The draw that is lost belongs to a step in the MIDDLE of a window in A1 and A3 (the converging step); in every A2 case the
    longest first attempt ends at the budget of 400 steps, so there it is the last step of the budget that is taken on 0.5."""
    wl = _workload(name)
    short = np.array(wl["replay"][:, :int(wl["draws_first"].max()) - 1])
    budget = min(wl["st"].max_iter, max(c["iters"][0] for c in wl["chains"]) + 100)
    with pytest.raises(_lib.McSASHipError) as e:
        _run(wl, path, short, max_retries=0, max_iter=budget)
    assert e.value.code == MCSAS_ESTREAM


# ----------------------------------------------------------------------------- Part B: the window a chain was speculated in
B_SHAPE = dict(nq=40, N=64, steps=192, seed=31)          # 3 x 64 steps: every contribution is proposed again after it may have been replaced
# criteria some chains reach within the budget, chosen with the oracle, and the step each of the five chains then ends at (192: never
# reached) — asserted on the oracle's output in _b_oracle.  All five chains are walked by the oracle, once per module run
# (a Kholodenko row costs the numpy oracle 27 ms: 35 s without a criterion, 25 s with it; the cylinders' five take a second).
B_CRIT = {"cyl_aspect": 6300.0, "kholodenko": 5450.0}
B_ENDS = {"cyl_aspect": [192, 65, 47, 99, 192], "kholodenko": [93, 159, 149, 192, 138]}


def _b_setup(tag):
    q, I, sig = _synthetic(B_SHAPE["nq"])
    m, spec = make_models(tag, *RANDOM_RANGES[tag], **({"intDiv": 20.} if tag == "cyl_aspect" else {}))
    return q, I, sig, m.setup(), spec


@functools.lru_cache(maxsize=None)
def _b_oracle(tag, crit):
    q, I, sig, _, spec = _b_setup(tag)
    ost = O.Settings(n_contrib=B_SHAPE["N"], n_reps=1, max_iter=B_SHAPE["steps"], conv_crit=crit, max_retries=0)
    chains = {r: _oracle_chain(spec, q, I, sig, [I.min(), I.max()], [q.min(), q.max()], ost, O.PhiloxStream(B_SHAPE["seed"], r), 0)
              for r in range(5)}
    if crit == 0.0:
        assert all(c["iters"] == [B_SHAPE["steps"]] and c["ref"].num_moves > 20 for c in chains.values())
    else:
        ends = [chains[r]["iters"][0] for r in range(5)]
        assert ends == B_ENDS[tag], ends
        assert [chains[r]["converged"] for r in range(5)] == [int(n < B_SHAPE["steps"]) for n in ends]
        early = [n for n in ends if n < B_SHAPE["steps"]]
        assert 0 < len(early) < 5 and all(n % 8 != 0 for n in early)       # some reach it, each inside a window of 8 (so of 16, 24 and 32) steps
    return chains


def _b_run(tag, crit, reps, monkeypatch, kb=None):
    q, I, sig, setup, _ = _b_setup(tag)
    if kb is None:
        monkeypatch.delenv("MCSAS_HIP_PIPE_KB", raising=False)
    else:
        monkeypatch.setenv("MCSAS_HIP_PIPE_KB", str(kb))
    st = engine.Settings(n_contrib=B_SHAPE["N"], n_reps=reps, max_iter=B_SHAPE["steps"], conv_crit=crit, max_retries=0,
                         seed=B_SHAPE["seed"], rep_offset=0, exec_mode=engine.EXEC_PIPELINE)
    plan = engine.Plan(setup, q, I, sig, st)
    try:
        info = plan.info
        plan.launch()
        return info, plan.fetch()
    finally:
        plan.close()


@pytest.mark.parametrize("with_crit", [False, True])
@pytest.mark.parametrize("tag", ["cyl_aspect", "kholodenko"])
def test_rows_with_an_integral_do_not_depend_on_the_window_knob(tag, with_crit, monkeypatch):
    """B1: the same five chains in windows of 32 (the default at 64 contributions), 8 and 16 steps (MCSAS_HIP_PIPE_KB, read at plan
    creation): every returned array bit for bit the same, and the default run is the oracle's chain on the same Philox streams."""
    crit = B_CRIT[tag] if with_crit else 0.0
    out = {}
    for kb, window in ((None, 32), (8, 8), (16, 16)):
        info, out[kb] = _b_run(tag, crit, 5, monkeypatch, kb)
        assert info["exec_mode"] == "pipeline" and info["window"] == window, (kb, info)
    for kb in (8, 16):
        _same_arrays(out[kb], out[None], "window %d vs. 32" % kb)
    res = out[None]
    for r, c in _b_oracle(tag, crit).items():
        ref = c["ref"]
        assert (res.num_iter[r], res.num_moves[r], res.attempts[r], res.converged[r], res.draws[r]) == \
               (ref.num_iter, ref.num_moves, 1, c["converged"], c["pos"][-1]), r
        np.testing.assert_allclose(res.contribs[:, :, r], ref.rset, rtol=1e-12)
        np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-7)


@pytest.mark.parametrize("with_crit", [False, True])
@pytest.mark.parametrize("tag", ["cyl_aspect", "kholodenko"])
def test_rows_with_an_integral_do_not_depend_on_the_few_chains_rule(tag, with_crit, monkeypatch):
    """B2: on a 256-CU device 129 to 255 chains of 64 contributions make 2 to 4 rounds of rows per tick and the few-chains rule of
    pipe_geometry shortens the window (160 chains: 24 steps instead of 32).  Chains 0-7 of such a launch equal chains 0-7 run alone,
    bit for bit — what the split over a device list relies on, whose shards have different chain counts."""
    import torch
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the chain counts that enter the few-chains rule are those of a 256-CU device (the library reads the CU count at run time)")
    crit = B_CRIT[tag] if with_crit else 0.0
    info_many, many = _b_run(tag, crit, 160, monkeypatch)
    info_few, few = _b_run(tag, crit, 8, monkeypatch)
    assert info_many["exec_mode"] == info_few["exec_mode"] == "pipeline" and info_many["window"] != info_few["window"], (info_many, info_few)
    for name in FIELDS:
        a = getattr(many, name)
        np.testing.assert_array_equal(a[..., :8], getattr(few, name), err_msg=name)
    assert few.num_moves.min() > 0


@pytest.mark.parametrize("name", ["a1_cyl", "a2_cyl"])
def test_short_window_on_an_exactly_fitting_stream(name, monkeypatch):
    """B3: Part A's exactly fitting stream through the row-queue pipeline in windows of 8 steps: MCSAS_OK, the oracle's chains, and
    the arrays of the long stream bit for bit."""
    wl = _workload(name)
    monkeypatch.setenv("MCSAS_HIP_PIPE_KB", "8")
    assert _window_of(wl, "pipe_rowq") == 8
    _mid_window(wl, 8)
    fit = _run(wl, "pipe_rowq", _exact_fit(wl))
    _check_against_oracle(wl, fit)
    _same_arrays(fit, _run(wl, "pipe_rowq", wl["replay"]), "exact fit vs. long stream, window 8")

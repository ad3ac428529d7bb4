"""Shared by the test modules of given starts, traces and batches (test_*start*.py, test_*trace*.py, test_batch_*.py), on the device
and on the host: the workloads and their oracle chains, the checkers, and the host-side helpers.  A plain module like helpers.py:
nothing in here is collected.

The reference of a started chain is the oracle's own mc_fit, unchanged: while it runs, generate_parameters is replaced so that its
FIRST call returns a copy of the start set (the rset of mcsas.py:317) and every later call — the per-step draws, the fresh sets of
retry attempts — goes to the real function (_oracle_from).  For a trace, bgfit_calc is wrapped as well and records its conval call
by call (_oracle_traced).  Workloads are computed once, shared among the modules, and read-only."""
import ctypes as C
import functools
import os
import re

import numpy as np

import mcsas_amd
from mcsas_amd import _lib, engine
from oracle import mcsas_oracle as O
from helpers import make_models

MCSAS_OK, MCSAS_EINVAL, MCSAS_ENODEV, MCSAS_ESTREAM = 0, -1, -2, -5
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mcsas_amd", "csrc")
WG = engine.EXEC_WORKGROUP

FIELDS = ("contribs", "fit", "chisq", "scaling", "background", "num_iter", "num_moves", "attempts", "converged", "draws")
RANGES = {
    "sphere": ([2e-9], [3e-7]), "cyl_aspect": ([1e-9, 0.5], [1e-7, 20.0]), "ellcs": ([1e-9, 2e-9, 2e-10], [1e-7, 2e-7, 1e-8]),
    "kholodenko": ([1e-9, 1e-8, 1e-7], [5e-9, 5e-8, 1e-6]), "elliso": ([1e-9, 0.3], [1e-7, 8.0]), "sphcs": ([1e-9, 5e-10], [1e-7, 2e-8]),
    "gausschain": ([1e-9, 1e-9], [1e-7, 1e-7]), "lmasphere": ([2e-9, 0.01], [2e-7, 0.4]),
}
SEED, REP_OFFSET, R = 5, 3, 3
K = 200           # trace capacity: above the moves of every chain below (asserted)

# name: model, q-points, contributions, steps of the started run, steps of the cold run the start comes from, criterion (chosen with
# the oracle so that chains end mid-run), fixed model parameters
SHAPES = {
    "sphere100": ("sphere", 100, 60, 700, 150, 50.0, {}),
    "sphere200": ("sphere", 200, 60, 700, 150, 50.0, {}),
    "cyl100": ("cyl_aspect", 100, 24, 120, 40, 7000.0, {"intDiv": 12.}),
    "sphere1500": ("sphere", 1500, 16, 64, 20, 450.0, {}),          # 32 q slots per lane: a cache-only class
    # the q-split kernel's (test_wide_*_gpu.py)
    "sphere1025": ("sphere", 1025, 16, 64, 20, 440.0, {}),
    "sphere4097": ("sphere", 4097, 16, 64, 20, 440.0, {}),
    "sphere8193": ("sphere", 8193, 12, 64, 20, 460.0, {}),          # one chain of the three runs to its budget
}
# the wave kernels' cases: (name, cache_intensities)
CASES = [("sphere100", 1), ("sphere100", 0), ("sphere200", 1), ("sphere200", 0), ("cyl100", 1), ("sphere1500", -1)]
# the q-split kernel's cases: name -> q slots per lane, waves per chain
GEOMETRY = {"sphere1500": (8, 3), "sphere1025": (8, 3), "sphere4097": (16, 5), "sphere8193": (32, 5)}
# criterion of the COLD run of each shape, chosen with the oracle so that chains end mid-run, at different steps.  sphere8193: one
# chain of the three runs to its budget
COLD_CRIT = {"sphere100": 60.0, "sphere200": 70.0, "cyl100": 7000.0, "sphere1500": 500.0,
             "sphere1025": 420.0, "sphere4097": 420.0, "sphere8193": 430.0}


# ----------------------------------------------------------------------------- data, and results bit for bit
def _synthetic(nq):
    from bench import synthetic_data
    return synthetic_data(nq)


def _same(got, one, what=""):
    for name in FIELDS:
        assert np.array_equal(getattr(got, name), getattr(one, name)), (what, name)


def _alone(pr):
    st = engine.Settings(**{**pr["st"].__dict__, "exec_mode": engine.EXEC_WAVE})
    return engine.analyse(pr["model"], pr["q"], pr["intensity"], pr["sigma"], st, pr.get("replay"), pr.get("stop"), pr.get("smear"))


# ----------------------------------------------------------------------------- started chains against the oracle
def _oracle_from(spec, q, I, sig, ost, start, stream, retries):
    """The retry loop of tests/test_chain_end_gpu.py::_oracle_chain with the first initial set given."""
    real, calls = O.generate_parameters, [0]

    def given_first(spec_, stream_, count=1):
        calls[0] += 1
        if calls[0] == 1:
            assert count == start.shape[0]
            return np.array(start, dtype=float)
        return real(spec_, stream_, count)

    lim = ([I.min(), I.max()], [q.min(), q.max()])
    iters, pos = [], []
    O.generate_parameters = given_first
    try:
        while True:
            ref = O.mc_fit(spec, q, I, sig, lim[0], lim[1], ost, stream, method="closed")
            iters.append(ref.num_iter); pos.append(stream.pos)
            if ref.conval <= ost.conv_crit or len(iters) > retries:
                break
    finally:
        O.generate_parameters = real
    assert calls[0] == 1 + sum(iters) + (len(iters) - 1)          # the start, one call per step, one per fresh set
    return dict(attempts=len(iters), iters=iters, pos=pos, ref=ref, converged=int(ref.conval <= ost.conv_crit))


@functools.lru_cache(maxsize=None)
def _workload(name):
    """The start (a short cold run of the oracle: a realistic mid-fit state, one column per repetition, stored in columns 1..3 of
    a five-column array) and the oracle's started chains on the Philox streams of chains REP_OFFSET + r — the same numbers serve
    the replayed and the free-running run.  Computed once, shared, read-only."""
    tag, nq, N, steps, steps0, crit, fixed = SHAPES[name]
    q, I, sig = _synthetic(nq)
    m, spec = make_models(tag, *RANGES[tag], **fixed)
    lim = ([I.min(), I.max()], [q.min(), q.max()])
    cold = O.Settings(n_contrib=N, n_reps=1, max_iter=steps0, conv_crit=1e-9, max_retries=0)
    start = np.zeros((N, spec.n_active, 5))
    start[:, :, 0] = start[:, :, 4] = np.nan                                 # (columns a correct rep_first never reads)
    for r in range(R):
        start[:, :, 1 + r] = O.mc_fit(spec, q, I, sig, lim[0], lim[1], cold, O.PhiloxStream(11, r), method="closed").rset
    ost = O.Settings(n_contrib=N, n_reps=1, max_iter=steps, conv_crit=crit, max_retries=0)
    chains = [_oracle_from(spec, q, I, sig, ost, start[:, :, 1 + r], O.PhiloxStream(SEED, REP_OFFSET + r, pos=0), 0) for r in range(R)]
    P = spec.n_active
    for c in chains:
        assert c["attempts"] == 1 and c["pos"][-1] == P * c["iters"][0]         # no uniforms for the initial set
        assert c["ref"].num_moves > 0
    early = [c["iters"][0] for c in chains if c["iters"][0] < steps]
    assert early and all(c["converged"] for c in chains if c["iters"][0] < steps)   # a mid-run end that is not the budget
    assert len({c["iters"][0] for c in chains}) > 1
    L = max(c["pos"][-1] for c in chains)
    replay = np.stack([O.philox_uniform(SEED, REP_OFFSET + r, np.arange(L, dtype=np.uint64)) for r in range(R)])
    for r, c in enumerate(chains):                                             # what a chain did not consume: OTHER uniforms
        u = replay[r, c["pos"][-1]:]
        replay[r, c["pos"][-1]:] = np.where(u < 0.5, u + 0.25, u - 0.25)
    st = engine.Settings(n_contrib=N, n_reps=R, max_iter=steps, conv_crit=crit, max_retries=0, seed=SEED, rep_offset=REP_OFFSET)
    for a in (start, replay):
        a.setflags(write=False)
    return dict(setup=m.setup(), spec=spec, q=q, I=I, sig=sig, st=st, start=start, chains=chains, replay=replay)


def _check_against_oracle(chains, res, P):
    """The comparison of tests/test_chain_end_gpu.py::_check_against_oracle, fit and scaling included."""
    for r, c in enumerate(chains):
        ref = c["ref"]
        got = (res.num_iter[r], res.num_moves[r], res.attempts[r], res.converged[r], res.draws[r])
        print("chain %d: iter, moves, attempts, converged, draws = %s; oracle %s"
              % (r, got, (ref.num_iter, ref.num_moves, c["attempts"], c["converged"], c["pos"][-1])))
        assert got == (ref.num_iter, ref.num_moves, c["attempts"], c["converged"], c["pos"][-1]), r
        np.testing.assert_allclose(res.contribs[:, :, r], ref.rset, rtol=1e-12)
        np.testing.assert_allclose(res.chisq[r], ref.conval, rtol=1e-7)
        np.testing.assert_allclose(res.fit[:, r], ref.fit, rtol=1e-6, atol=1e-12 * np.abs(ref.fit).max())
        np.testing.assert_allclose(res.scaling[r], ref.scaling, rtol=1e-6)


@functools.lru_cache(maxsize=None)
def _wave_retry_workload():
    """A start the chain cannot bring to the criterion within its budget (every contribution at one small radius), two retries.
    Seed and criterion chosen with the oracle: chains 0 and 2 converge in their second attempt, chain 1 in none of its three."""
    nq, N, steps, crit, seed = 100, 40, 300, 90.0, 3
    q, I, sig = _synthetic(nq)
    m, spec = make_models("sphere", *RANGES["sphere"])
    start = np.full((N, 1, R), 2e-9) * np.array([1.0, 1.5, 2.0])[None, None, :]
    ost = O.Settings(n_contrib=N, n_reps=1, max_iter=steps, conv_crit=crit, max_retries=2)
    chains = [_oracle_from(spec, q, I, sig, ost, start[:, :, r], O.PhiloxStream(seed, REP_OFFSET + r, pos=0), 2) for r in range(R)]
    assert [c["attempts"] for c in chains] == [2, 3, 2] and [c["converged"] for c in chains] == [1, 0, 1]
    for c in chains:                                                            # the started attempt ran to its budget, a retry WAS taken
        assert c["iters"][0] == steps and c["pos"][0] == steps                  # ... and the start cost no draws
        assert c["pos"][-1] == sum(c["iters"]) + N * (c["attempts"] - 1)        # N * P for each later initial set
    assert chains[0]["iters"][1] < steps and chains[2]["iters"][1] < steps      # converged mid-run in the later attempt
    st = engine.Settings(n_contrib=N, n_reps=R, max_iter=steps, conv_crit=crit, max_retries=2, seed=seed, rep_offset=REP_OFFSET)
    start.setflags(write=False)
    return dict(setup=m.setup(), spec=spec, q=q, I=I, sig=sig, st=st, start=start, chains=chains)


@functools.lru_cache(maxsize=None)
def _wide_retry_workload():
    """1025 q-points, every contribution of a start at one large radius, a budget of 24 steps: no started attempt reaches the
    criterion, two retries.  Seed and criterion chosen with the oracle: chains 0 and 1 converge mid-run in their third attempt
    (at 0.99 and 0.96 of the criterion), chain 2 in none."""
    nq, N, steps, crit, seed = 1025, 16, 24, 1000.0, 4
    q, I, sig = _synthetic(nq)
    m, spec = make_models("sphere", *RANGES["sphere"])
    start = np.full((N, 1, R), 1.5e-7) * np.array([1.0, 1.5, 2.0])[None, None, :]
    ost = O.Settings(n_contrib=N, n_reps=1, max_iter=steps, conv_crit=crit, max_retries=2)
    chains = [_oracle_from(spec, q, I, sig, ost, start[:, :, r], O.PhiloxStream(seed, REP_OFFSET + r, pos=0), 2) for r in range(R)]
    assert [c["attempts"] for c in chains] == [3, 3, 3] and [c["converged"] for c in chains] == [1, 1, 0]
    for c in chains:                                                            # the started attempt ran to its budget, retries WERE taken
        assert c["iters"][0] == steps and c["pos"][0] == steps                  # ... and the start cost no draws
        assert c["pos"][-1] == sum(c["iters"]) + N * (c["attempts"] - 1)        # N * P for each later initial set
    assert chains[0]["iters"][2] < steps and chains[1]["iters"][2] < steps
    st = engine.Settings(n_contrib=N, n_reps=R, max_iter=steps, conv_crit=crit, max_retries=2, seed=seed, rep_offset=REP_OFFSET, exec_mode=WG)
    start.setflags(write=False)
    return dict(setup=m.setup(), spec=spec, q=q, I=I, sig=sig, st=st, start=start, chains=chains)


# ----------------------------------------------------------------------------- traced chains against the oracle
def _oracle_traced(spec, q, I, sig, ost, stream, start=None, retries=0):
    """The retry loop of _oracle_from (start: the first initial set given, or None for a cold chain) with every attempt's proposals
    and convals recorded — the second bgfit_calc call of an attempt is the chi² of the initial set (mcsas.py:343), call 2 + s belongs
    to step s (mcsas.py:376); ref.accepted names the steps of the moves.  The trace is the last attempt's."""
    real_gen, real_fit = O.generate_parameters, O.bgfit_calc
    calls, props, convals = [0], [], []

    def gen(spec_, stream_, count=1):
        calls[0] += 1
        if calls[0] == 1 and start is not None:
            assert count == start.shape[0]
            return np.array(start, dtype=float)
        out = real_gen(spec_, stream_, count)
        if count == 1:
            props.append(out[0].copy())
        return out

    def fit(*a, **k):
        out = real_fit(*a, **k)
        convals.append(float(out[1]))
        return out

    lim = ([I.min(), I.max()], [q.min(), q.max()])
    iters, pos = [], []
    O.generate_parameters, O.bgfit_calc = gen, fit
    try:
        while True:
            del props[:], convals[:]
            ref = O.mc_fit(spec, q, I, sig, lim[0], lim[1], ost, stream, method="closed")
            iters.append(ref.num_iter); pos.append(stream.pos)
            if ref.conval <= ost.conv_crit or len(iters) > retries:
                break
    finally:
        O.generate_parameters, O.bgfit_calc = real_gen, real_fit
    assert len(props) == ref.num_iter and len(convals) == 3 + ref.num_iter and len(ref.accepted) == ref.num_moves
    trace = dict(chisq0=convals[1], step=np.array(ref.accepted, dtype=np.int64),
                 chisq=np.array([convals[2 + s] for s in ref.accepted]),
                 values=np.array([props[s] for s in ref.accepted]).reshape(ref.num_moves, spec.n_active))
    return dict(attempts=len(iters), iters=iters, pos=pos, ref=ref, converged=int(ref.conval <= ost.conv_crit), trace=trace)


def _assert_chains_are_worth_tracing(chains, steps):
    assert all(3 < c["ref"].num_moves < K for c in chains), [c["ref"].num_moves for c in chains]
    assert len({c["iters"][-1] for c in chains}) > 1                            # chains end at different steps
    assert any(c["iters"][-1] < steps and c["converged"] for c in chains)       # ... one of them mid-run, by convergence


@functools.lru_cache(maxsize=None)
def _traced_workload(name, started):
    """The workload of _workload(name) with the oracle's traces: started from its start, or cold (the chain's own
    initial set, a criterion of its own).  The chains run on the Philox streams of chains REP_OFFSET + r; `replay` holds the same
    numbers.  Computed once, shared, read-only."""
    wl = _workload(name)
    tag, nq, N, steps, steps0, crit, fixed = SHAPES[name]
    spec, q, I, sig = wl["spec"], wl["q"], wl["I"], wl["sig"]
    if not started:
        crit = COLD_CRIT[name]
    ost = O.Settings(n_contrib=N, n_reps=1, max_iter=steps, conv_crit=crit, max_retries=0)
    chains = [_oracle_traced(spec, q, I, sig, ost, O.PhiloxStream(SEED, REP_OFFSET + r, pos=0),
                             start=wl["start"][:, :, 1 + r] if started else None) for r in range(R)]
    _assert_chains_are_worth_tracing(chains, steps)
    if started:
        assert [c["iters"] for c in chains] == [c["iters"] for c in wl["chains"]]
    L = max(c["pos"][-1] for c in chains)
    replay = np.stack([O.philox_uniform(SEED, REP_OFFSET + r, np.arange(L, dtype=np.uint64)) for r in range(R)])
    replay.setflags(write=False)
    st = engine.Settings(**{**wl["st"].__dict__, "conv_crit": crit})
    return dict(wl, st=st, chains=chains, replay=replay, start=wl["start"][:, :, 1:1 + R] if started else None)


def _check_trace(chains, tr, capacity):
    """The trace against the oracle's, and what holds of any trace: steps rise, chi² falls from chisq0 on, sentinels behind.
    Tolerances are those of _check_against_oracle: steps and counts exact, values rtol 1e-12, chi² rtol 1e-7."""
    assert tr.step.shape == (capacity, len(chains)) and tr.chisq.shape == tr.step.shape and tr.values.shape[::2] == tr.step.shape
    for r, c in enumerate(chains):
        ref, t = c["ref"], c["trace"]
        n = min(ref.num_moves, capacity)
        print("chain %d: count %d (oracle %d), chisq0 %.17g (oracle %.17g), last kept chisq %.17g (oracle %.17g)"
              % (r, tr.count[r], ref.num_moves, tr.chisq0[r], t["chisq0"], tr.chisq[n - 1, r], t["chisq"][n - 1]))
        assert tr.count[r] == ref.num_moves
        assert np.array_equal(tr.step[:n, r], t["step"][:n])
        np.testing.assert_allclose(tr.values[:n, :, r], t["values"][:n], rtol=1e-12)
        np.testing.assert_allclose(tr.chisq[:n, r], t["chisq"][:n], rtol=1e-7)
        np.testing.assert_allclose(tr.chisq0[r], t["chisq0"], rtol=1e-7)
        assert (np.diff(tr.step[:n, r]) > 0).all() and (np.diff(tr.chisq[:n, r]) < 0).all() and tr.chisq[0, r] < tr.chisq0[r]
        assert (tr.step[n:, r] == -1).all() and np.isnan(tr.chisq[n:, r]).all() and np.isnan(tr.values[n:, :, r]).all()


def _same_trace(a, b, what=""):
    for f in ("count", "chisq0", "step", "chisq", "values"):
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=f != "count" and f != "step"), (what, f)


def _guarded_trace(capacity, P, n_reps, guard=64):
    """A mcsas_trace whose arrays sit inside larger ones filled with sentinels: (the block, the larger arrays by field)."""
    sizes = dict(count=n_reps, chisq0=n_reps, step=capacity * n_reps, chisq=capacity * n_reps, values=capacity * P * n_reps)
    big = {f: (np.full(n + 2 * guard, -77, dtype=np.int64) if f in ("count", "step") else np.full(n + 2 * guard, -77.5)) for f, n in sizes.items()}
    t = _lib.Trace()
    t.struct_size, t.capacity = C.sizeof(_lib.Trace), capacity
    for f, a in big.items():
        setattr(t, f, a[guard:].ctypes.data_as(C.POINTER(C.c_int64 if a.dtype == np.int64 else C.c_double)))
    return t, big, {f: (guard, n) for f, n in sizes.items()}


# ----------------------------------------------------------------------------- the host side: what is refused before a device is touched
def _data(nq=40):
    q = np.linspace(1e8, 2e9, nq)
    I = 1.0 / (1.0 + (q * 2e-9) ** 4)
    return q, I, 0.02 * I


def _problem(nq=40, N=8, R=2, **over):
    q, I, sig = _data(nq)
    m, _ = make_models("sphere", [2e-9], [3e-7])
    st = engine.Settings(**{**dict(n_contrib=N, n_reps=R, max_iter=10, conv_crit=1e-9, max_retries=0), **over})
    prob = engine.HipProblem(m.setup(), q, I, sig, st)
    res = engine.ChainResults(N, 1, R, nq)
    return prob, res


def _from(prob, start, res):
    lib = _lib.load()
    rc = lib.mcsas_hip_analyse_from(C.byref(prob.c), None if start is None else _lib.as_dp(start), C.byref(res.c))
    return rc, lib.mcsas_hip_last_error().decode()


def _traced(prob, res, tr, start=None):
    lib = _lib.load()
    rc = lib.mcsas_hip_analyse_traced(C.byref(prob.c), None if start is None else _lib.as_dp(start), C.byref(res.c),
                                      None if tr is None else C.byref(tr.c))
    return rc, lib.mcsas_hip_last_error().decode()


class _NoLibrary(object):
    """_lib.load replaced for the duration: a refusal made in Python must come before the library is needed."""
    def __init__(self, monkeypatch):
        def load(*a, **k):
            raise AssertionError("the library was asked for before the argument check")
        monkeypatch.setattr(_lib, "load", load)


class _LibraryReached(Exception):
    pass


def _stub_library(monkeypatch):
    """_lib.load replaced for the duration: reaching it means every check made in Python has passed."""
    def load(*a, **k):
        raise _LibraryReached()
    monkeypatch.setattr(_lib, "load", load)


def _algo_40q(**kw):
    q, I, sig = _data()
    algo = mcsas_amd.McSAS.factory()(seed=1, **kw)
    algo.numContribs.setValue(8); algo.numReps.setValue(3); algo.maxIterations.setValue(10)
    algo.model, _ = make_models("sphere", [2e-9], [3e-7])
    algo.data = mcsas_amd.SASData(q, I, sig)
    return algo


def _algo_nq(nq, **kw):
    q, I, sig = _data(nq)
    algo = mcsas_amd.McSAS.factory()(seed=1, **kw)
    algo.numContribs.setValue(8); algo.numReps.setValue(3); algo.maxIterations.setValue(10)
    algo.model, _ = make_models("sphere", [2e-9], [3e-7])
    algo.data = mcsas_amd.SASData(q, I, sig)
    return algo


def _code(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())

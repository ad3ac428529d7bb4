"""The instance matrix of the two chain families that come cold, started and traced, for tests/test_instances_gpu.py (device),
tests/test_instances_host.py (what those tests rest on) and oracle/make_instance_chains.py (Kholodenko's recorded chains).  A plain
module like chain_cases.py: nothing in here is collected.

One wavefront per chain (csrc/chain_wave.h; kern_lookup.h: MCSAS_WAVE_LOOKUP): 8 built-in models x 12 (q slots per lane, row cache)
pairs, each as chain_wave_kernel / chain_wave_trace_kernel / chain_wave_batch_kernel<.., GIVEN = false | true>: 576 instances.  The
q-split workgroup (csrc/chain_wide.h; MCSAS_WIDE_LOOKUP): 8 models x 8 / 16 / 32 slots, cold, started, traced cold, traced started: 96.
What selects an instance: the model, the number of q-points (slots per lane, and for the q-split kernel the waves per chain),
cache_intensities, exec_mode, and whether the plan has a start, a trace, or is launched in a batch.

Data is bench.synthetic_data(nq); models, ranges and intDiv are sets_exact's (MATRIX_MODELS, model_range).  Every (model, nq) has two
oracle chains per repetition, both chain_cases._oracle_traced's: the cold chain, and the continued chain, started from the cold
chain's final set on a stream of its own (the calc(start=result) use).  Every step's chi² is recorded on the way (bgfit_calc is
wrapped around _oracle_traced, which wraps it in turn): a chain's margin is the smallest |chi²_step - chi²_best| / chi²_best, which
test_instances_host.py holds above what the device's rounding can reach."""
import functools
import hashlib
import os
import types

import numpy as np

from oracle import mcsas_oracle as O
import sets_exact as SX

MODELS = SX.MATRIX_MODELS
R, REP_OFFSET = 2, 5
N_CONTRIB, STEPS = 12, 64
KHOLODENKO_N = 6                    # its oracle row is a QUADPACK integral per point: 6 contributions, 16 to 24 steps
CRIT = 1e-12                        # never reached: chains run to their budget (where a loop ends: tests/test_chain_end_gpu.py)
CAPACITY = 80                       # trace capacity: above the budget, so above the moves of every chain
MIN_MOVES = 3
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instance_chains_kholodenko.npz")

# ------------------------------------------------------------------------------------------------ the shapes
WAVE_QPL = (1, 2, 4, 8, 16, 32, 64)
WIDE_QPL = (8, 16, 32)


def wave_nq(qpl):
    """The last q slot of the instance holds real points and padding: 37, 101, 229, 485, 997, 2021, 4069."""
    return 64 * (qpl - 1) + 37


# (model, slots, cache_intensities): the row cache on and off up to 16 slots, cached rows only at 32 and 64 (kern_lookup.h)
WAVE = tuple((tag, qpl, cache) for tag in MODELS for qpl in WAVE_QPL for cache in ((1, 0) if qpl <= 16 else (1,)))
# slots -> shape name -> (q-points, waves per chain).  A: the full waves use every slot, the tail wave holds one point; B: 8 waves, the
# last slot of the last wave partly filled
WIDE_SHAPES = {8: {"A": (1025, 3), "B": (4069, 8)}, 16: {"A": (4097, 5), "B": (8165, 8)}, 32: {"A": (8193, 5), "B": (16357, 8)}}
# (model, slots, shape name); Kholodenko runs A only (0.6 ms per point and oracle row)
WIDE = tuple((tag, qpl, shape) for tag in MODELS for qpl in WIDE_QPL for shape in ("A", "B") if not (tag == "kholodenko" and shape == "B"))


def wide_nq(qpl, shape):
    return WIDE_SHAPES[qpl][shape][0]


# every (model, q-points) with oracle chains; 4069 points serve the wave kernel at 64 slots and the q-split kernel at 8
ENTRIES = tuple(sorted({(tag, wave_nq(qpl)) for tag, qpl, _ in WAVE} | {(tag, wide_nq(qpl, shape)) for tag, qpl, shape in WIDE},
                       key=lambda e: (MODELS.index(e[0]), e[1])))
KHOLODENKO_NQ = tuple(nq for tag, nq in ENTRIES if tag == "kholodenko")

# ------------------------------------------------------------------------------------------------ seeds and budgets
# (seed of the cold chains, seed of the continued chains); the streams are Philox (seed, REP_OFFSET + r).  The default, and per
# (model, q-points) another pair where the default gives the oracle a chain under MIN_MOVES moves, a margin under its bound, equal
# repetitions, or (Kholodenko) a chi² under 1 — chosen on the CPU from the oracle alone (oracle/make_instance_chains.py --search
# prints every candidate's figures), as sets_exact.GENERATED_SEED is; tests/test_instances_host.py prints every entry's.
DEFAULT_SEEDS = (41, 42)
SEEDS = {("lmasphere", 37): (43, 44), ("lmasphere", 101): (45, 46)}        # (the default: a continued chain of 2 moves)
SEEDS.update({("kholodenko", nq): (43, 44) for nq in (37, 101, 229, 485, 997, 2021, 4069, 1025, 4097, 8193)})   # (the default: 0 to 2)
# Kholodenko's steps (16 to 24), the same for the cold and the continued chain
KHOLODENKO_STEPS = {nq: 24 for nq in (37, 101, 229, 485, 997, 2021, 4069, 1025, 4097, 8193)}


def seeds(tag, nq):
    return SEEDS.get((tag, nq), DEFAULT_SEEDS)


def budget(tag, nq):
    """-> (contributions, steps)"""
    return (KHOLODENKO_N, KHOLODENKO_STEPS[nq]) if tag == "kholodenko" else (N_CONTRIB, STEPS)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def data(nq):
    from bench import synthetic_data
    q, I, sig = synthetic_data(nq)
    for a in (q, I, sig):
        a.setflags(write=False)
    return q, I, sig


def models(tag):
    """-> (product model, oracle spec)"""
    from helpers import make_models
    lo, hi, fixed = SX.model_range(tag)
    return make_models(tag, lo, hi, **fixed)


def oracle_settings(tag, nq):
    n, steps = budget(tag, nq)
    return O.Settings(n_contrib=n, n_reps=1, max_iter=steps, conv_crit=CRIT, max_retries=0)


def engine_settings(tag, nq, exec_mode, cache=-1, continued=False, n_reps=R, first=0):
    """The device's settings of an entry's cold or continued chains: repetitions first .. first + n_reps - 1 of the R."""
    from mcsas_amd import engine
    n, steps = budget(tag, nq)
    return engine.Settings(n_contrib=n, n_reps=n_reps, max_iter=steps, conv_crit=CRIT, max_retries=0, seed=seeds(tag, nq)[int(continued)],
                           rep_offset=REP_OFFSET + first, cache_intensities=cache, exec_mode=exec_mode)


def digest(tag, nq, r, start, seed):
    """SHA-256 over what a chain is computed from: q, I, sigma, the start (none for a cold chain), the settings, the model's ranges and
    fixed parameters, the seed and the chain's number."""
    q, I, sig = data(nq)
    lo, hi, fixed = SX.model_range(tag)
    n, steps = budget(tag, nq)
    h = hashlib.sha256()
    for a in (q, I, sig, np.zeros(0) if start is None else start, lo, hi, [n, steps, CRIT, O.Settings().comp_exp],
              [float(v) for _, v in sorted(fixed.items())], [seed, REP_OFFSET + r]):
        a = np.ascontiguousarray(a, dtype=np.float64)
        h.update(np.int64(a.size).tobytes()); h.update(a.tobytes())
    h.update(tag.encode())
    return np.frombuffer(h.digest(), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ oracle chains
def recorded_chain(spec, q, I, sig, ost, stream, start=None):
    """chain_cases._oracle_traced, unchanged, with every bgfit_calc result recorded around it: call 1 is the chi² of the initial set,
    call 2 + s that of step s (mcsas.py:343, :376), accepted iff below the best so far (mcsas.py:379).  Adds to its dict: margin,
    lowest (chi²), step_chisq."""
    from chain_cases import _oracle_traced
    real, seen = O.bgfit_calc, []

    def fit(*a, **k):
        out = real(*a, **k)
        seen.append(float(out[1]))
        return out

    O.bgfit_calc = fit
    try:
        c = _oracle_traced(spec, q, I, sig, ost, stream, start=start)
    finally:
        O.bgfit_calc = real
    steps = c["ref"].num_iter
    assert c["attempts"] == 1 and len(seen) == 3 + steps
    best, margin, moves = seen[1], np.inf, 0
    for x in seen[2:2 + steps]:
        margin = min(margin, abs(x - best) / best)
        if x < best:
            best, moves = x, moves + 1
    assert moves == c["ref"].num_moves
    c.update(margin=float(margin), lowest=float(best), step_chisq=np.array(seen[2:2 + steps]))
    return c


def compute_chains(tag, nq, seed_pair=None):
    """-> dict(cold=[chain] * R, cont=[chain] * R) from the oracle, live."""
    q, I, sig = data(nq)
    _, spec = models(tag)
    ost = oracle_settings(tag, nq)
    s_cold, s_cont = seed_pair or seeds(tag, nq)
    cold = [recorded_chain(spec, q, I, sig, ost, O.PhiloxStream(s_cold, REP_OFFSET + r, pos=0)) for r in range(R)]
    cont = [recorded_chain(spec, q, I, sig, ost, O.PhiloxStream(s_cont, REP_OFFSET + r, pos=0), start=cold[r]["ref"].rset) for r in range(R)]
    return dict(cold=cold, cont=cont)


FIXTURE_FIELDS = ("index", "rset", "numbers", "counts", "trace_step", "trace_chisq", "trace_values", "digest")


def pack_chains(by_nq):
    """{nq: compute_chains("kholodenko", nq)} -> the fixture's arrays, numbers only; one row per chain, in the order of `index`
    (q-points, 0 cold / 1 continued, repetition).  numbers: chi², scale, background, chisq0, margin, lowest chi²; counts: steps, moves,
    draws.  Traces are padded to the largest budget with -1 / NaN.  The fit is not stored."""
    P, T = 3, max(KHOLODENKO_STEPS.values())
    rows = [(nq, k, r) for nq in sorted(by_nq) for k in (0, 1) for r in range(R)]
    out = dict(index=np.array(rows, dtype=np.int64), rset=np.zeros((len(rows), KHOLODENKO_N, P)), numbers=np.zeros((len(rows), 6)),
               counts=np.zeros((len(rows), 3), dtype=np.int64), trace_step=np.full((len(rows), T), -1, dtype=np.int64),
               trace_chisq=np.full((len(rows), T), np.nan), trace_values=np.full((len(rows), T, P), np.nan),
               digest=np.zeros((len(rows), 32), dtype=np.uint8))
    for i, (nq, k, r) in enumerate(rows):
        both = by_nq[nq]
        c = both["cont" if k else "cold"][r]
        ref, t, n = c["ref"], c["trace"], c["ref"].num_moves
        out["rset"][i] = ref.rset
        out["numbers"][i] = (ref.conval, ref.scaling, ref.background, t["chisq0"], c["margin"], c["lowest"])
        out["counts"][i] = (ref.num_iter, ref.num_moves, c["pos"][-1])
        out["trace_step"][i, :n], out["trace_chisq"][i, :n], out["trace_values"][i, :n] = t["step"], t["chisq"], t["values"]
        out["digest"][i] = digest("kholodenko", nq, r, both["cold"][r]["ref"].rset if k else None, seeds("kholodenko", nq)[k])
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE, allow_pickle=False) as g:
        return {f: g[f] for f in FIXTURE_FIELDS}


def unpack_chains(nq):
    """Kholodenko's recorded chains at `nq` points in compute_chains' form; ref.fit is None."""
    g = fixture()
    out = dict(cold=[], cont=[])
    for i, (n, k, r) in enumerate(g["index"]):
        if n != nq:
            continue
        steps, moves, draws = (int(x) for x in g["counts"][i])
        conval, scaling, background, chisq0, margin, lowest = (float(x) for x in g["numbers"][i])
        ref = types.SimpleNamespace(rset=g["rset"][i], fit=None, conval=conval, num_iter=steps, num_moves=moves, scaling=scaling,
                                    background=background, accepted=[int(s) for s in g["trace_step"][i, :moves]])
        trace = dict(chisq0=chisq0, step=g["trace_step"][i, :moves], chisq=g["trace_chisq"][i, :moves], values=g["trace_values"][i, :moves])
        out["cont" if k else "cold"].append(dict(attempts=1, iters=[steps], pos=[draws], ref=ref, converged=0, trace=trace, margin=margin,
                                                  lowest=lowest, digest=g["digest"][i]))
    assert len(out["cold"]) == len(out["cont"]) == R, nq
    return out


@functools.lru_cache(maxsize=None)
def chains(tag, nq):
    """The oracle chains of a matrix entry, computed once and shared (the cache-on and cache-off tests, the wave and the q-split test
    at 4069 points); Kholodenko's are the recorded ones."""
    assert (tag, nq) in ENTRIES
    return unpack_chains(nq) if tag == "kholodenko" else compute_chains(tag, nq)


def start_array(both):
    """The continued chains' starts in columns 1..R of an R + 2 column array, NaN in the columns a correct rep_first never reads."""
    n, P = both["cold"][0]["ref"].rset.shape
    start = np.full((n, P, R + 2), np.nan)
    for r in range(R):
        start[:, :, 1 + r] = both["cold"][r]["ref"].rset
    start.setflags(write=False)
    return start

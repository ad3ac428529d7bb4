"""The joint fit of several data sets with one population (include/mcsas_hip.h: mcsas_hip_analyse_sets; csrc/chain_sets.h), restated in
float64 from the oracle's parts: one set of contributions, one running intensity over the points of all sets, and at every fit a
closed-form scale and background per set (O.bgfit_closed on the set's own points).  X = chi² Q is the sum of the sets' residual
sums at those optima; a step is accepted iff X_t < X (mcsas.py:379), convergence and max_iter use X / Q.  Also here: the inputs of
tests/test_sets_gpu.py, so that tests/test_sets_host.py can hold them to the margin condition those tests rest on."""
import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import mcsas_oracle as O


@dataclass
class SetsFit:
    rset: np.ndarray
    fit: np.ndarray                    # all points, each with its own set's scale and background
    conval: float                      # direct residual sum over all points / Q
    set_chisq: np.ndarray              # per set: its residual sum / Q_s
    set_scaling: np.ndarray
    set_background: np.ndarray
    num_iter: int
    num_moves: int
    attempts: int = 1
    draws: int = 0
    min_margin: float = np.inf         # min over the steps of |X_t - X| / X
    trajectory: list = field(default_factory=list)   # (step, conval) after every accepted move


def _fit_sets(sets, slices, C, find_bg):
    """-> (residual sum of every set at its own optimum, [(A, b)])"""
    rs, sc = [], []
    for (q, I, sigma), sl in zip(sets, slices):
        err = np.array(sigma, dtype=float); err[err == 0.0] = 1.
        A, b = O.bgfit_closed(I, err, C[sl], find_bg, False)
        rs.append(sum(((I - (C[sl] * A + b)) / err)**2)); sc.append((A, b))
    return np.array(rs), sc


def sets_mc_fit(spec, sets, st, stream):
    """One attempt: McSAS.mcFit (mcsas.py:287-439) judged by all sets."""
    sets = [tuple(np.asarray(v, dtype=float) for v in s) for s in sets]
    edges = np.concatenate([[0], np.cumsum([len(s[0]) for s in sets])])
    slices = [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]
    q = np.concatenate([s[0] for s in sets]); Q = len(q); N = st.n_contrib
    if st.start_from_min:
        rset = np.tile(np.where(np.minimum(spec.lo, spec.hi) == 0, np.pi / q.max(), np.minimum(spec.lo, spec.hi)) * .5, (N, 1))
    else:
        rset = O.generate_parameters(spec, stream, N)
    rows = np.empty((N, Q)); ft = np.zeros(Q)
    for i in range(N):
        rows[i] = O.calc_intensity(spec, q, rset[i], st.comp_exp)[0]
        ft += rows[i]
    X = _fit_sets(sets, slices, ft, st.find_bg)[0].sum()
    conval = X / Q
    num_iter = num_moves = ri = 0
    out = SetsFit(rset, None, 0., None, None, None, 0, 0)
    while N > 1 and conval > st.conv_crit and num_iter < st.max_iter:
        rt = O.generate_parameters(spec, stream, 1)
        new = O.calc_intensity(spec, q, rt[0], st.comp_exp)[0]
        test = ft + (new - rows[ri])
        Xt = _fit_sets(sets, slices, test, st.find_bg)[0].sum()
        out.min_margin = min(out.min_margin, abs(Xt - X) / X)
        if Xt < X:
            rset[ri], rows[ri], ft, X, conval = rt[0], new, test, Xt, Xt / Q
            out.trajectory.append((num_iter, conval))
            num_moves += 1
        ri = (ri + 1) % N
        num_iter += 1
    rs, sc = _fit_sets(sets, slices, ft, st.find_bg)
    out.fit = np.concatenate([ft[sl] * A + b for sl, (A, b) in zip(slices, sc)])
    out.conval = float(rs.sum() / Q)
    out.set_chisq = rs / np.array([len(s[0]) for s in sets], dtype=float)
    out.set_scaling = np.array([A for A, _ in sc]); out.set_background = np.array([b for _, b in sc])
    out.num_iter, out.num_moves = num_iter, num_moves
    return out


def sets_analyse(spec, sets, st, stream):
    """The retry loop of McSAS.analyse (mcsas.py:220-246) around sets_mc_fit for one repetition: attempts go on in the stream."""
    margin, res = np.inf, None
    for attempt in range(st.max_retries + 1):
        res = sets_mc_fit(spec, sets, st, stream)
        margin = min(margin, res.min_margin)
        res.attempts = attempt + 1
        if not res.conval > st.conv_crit:
            break
    res.min_margin, res.draws = margin, stream.pos
    return res


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests
LO, HI = 2e-8, 1.5e-7           # sphere radius range (narrow: a proposal that changes nothing visible makes a near-tie)


def population_sets(tag, nqs, scales, backgrounds, seed, lo=None, hi=None, **fixed):
    """Data sets that are ONE population (40 contributions drawn from the model's generators; its intensity is 1 at q = 1e7) seen
    through scales[s] and backgrounds[s] on a q range of its own, with 1 % noise and 1 % uncertainties.  -> [(q, I, sigma)]"""
    from helpers import make_models
    _, spec = make_models(tag, lo, hi, **fixed)
    rng = np.random.RandomState(seed)
    pop = O.generate_parameters(spec, O.ReplayStream(rng.uniform(size=40 * spec.n_active)), 40)
    sets = []
    norm = O.model_calc(spec, np.array([1e7]), pop, 0.6666666)[0][0]
    for s, (n, A, b) in enumerate(zip(nqs, scales, backgrounds)):
        q = np.logspace(7.0 + 0.1 * s, 8.3 + 0.05 * s, n)
        I = A * O.model_calc(spec, q, pop, 0.6666666)[0] / norm + b
        I = I * (1. + 0.01 * rng.standard_normal(n))
        sets.append((q, I, 0.01 * np.abs(I)))
    return sets


# ------------------------------------------------------------------------------------------------ the instance matrix and the chain text's edges
# chain_sets_kernel<M, QPL, SHARED> exists for 8 built-in models x 5 slot counts x 2 scale modes; one generated input per (model, QPL),
# seen by both modes (tests/sets_shared_exact.py builds the shared twin from the same recipe), and a family of inputs at the edges of the
# chain text.  The shapes are the smallest that still select the instance and use its last slot.
MATRIX_MODELS = ("sphere", "cyl_aspect", "ellcs", "kholodenko", "elliso", "sphcs", "gausschain", "lmasphere")
MATRIX_SHAPES = {
    1: (50,),                      # S = 1
    2: (30, 64),                   # slots 1 + 1: a set of exactly 64 points
    4: (37, 100),                  # slots 1 + 2 of 4: one slot is all padding
    8: (65, 3, 128, 70),           # slots 2 + 1 + 2 + 2 = 7 of 8: a 3-point set, a set that ends on a slot edge
    16: (300, 64, 385, 129),       # slots 5 + 1 + 7 + 3 = 16: bit 15 of end_mask, no padding slot
}
# Kholodenko's oracle row is a QUADPACK integral per point: 12 slots (1 + 2 + 3 + 6, 524 real points) still select the 16-slot instance
KHOLODENKO_16 = (3, 70, 130, 321)
INT_DIV = {"cyl_aspect": 12, "ellcs": 12, "elliso": 12}          # (the models that have an orientation integral)
# GaussianChain over chain_cases.RANGES (rg and bp both 1e-9 .. 1e-7) makes proposals that change nothing visible at these q: margins of
# 3.6e-10 to 1.8e-8.  rg from 1e-8 on keeps q rg >= 0.1 at every point, bp within a factor 10 keeps every contribution visible.
GAUSSCHAIN_RANGE = ([1e-8, 1e-8], [1e-7, 1e-7])
PER_SET_SCALES = (2e3, 2e6, 2e1, 4e8)                          # every pair a factor >= 100 apart
SHARED_SCALE = 2e4
BACKGROUNDS = (0.5, 90., 0., 7.)
# the replay seed of a generated input where the default (1) gives the restatement fewer than 5 moves in its short Kholodenko chain or
# takes it below chi² = 1 (where the Kholodenko margin's derivation ends): (name, shared) -> seed, chosen on the CPU from the
# restatement alone (tests/test_sets_host.py, tests/test_sets_shared_host.py print every margin)
GENERATED_SEED = {("mx_kholodenko_q2", False): 6, ("mx_kholodenko_q2", True): 3, ("mx_kholodenko_q8", False): 2,
                  ("mx_kholodenko_q16", False): 2}


def matrix_name(tag, qpl):
    return "mx_%s_q%d" % (tag, qpl)


def matrix_shape(tag, qpl):
    return KHOLODENKO_16 if (tag, qpl) == ("kholodenko", 16) else MATRIX_SHAPES[qpl]


def model_range(tag):
    from chain_cases import RANGES
    lo, hi = GAUSSCHAIN_RANGE if tag == "gausschain" else RANGES[tag]
    return list(lo), list(hi), ({"intDiv": INT_DIV[tag]} if tag in INT_DIV else {})


MATRIX = tuple(matrix_name(tag, qpl) for tag in MATRIX_MODELS for qpl in sorted(MATRIX_SHAPES))
EDGE_COUNTS = (1, 64, 65, 128)      # N == 1 skips the Monte-Carlo loop, 64 fills the initial wave exactly, 65 and 128 are the neighbours
# name -> (model, set_nq, what differs from the matrix's chain)
EDGES = {}
for _tag, _nqs in (("sphere", MATRIX_SHAPES[4]), ("sphcs", MATRIX_SHAPES[2])):
    for _n in EDGE_COUNTS:
        EDGES["ed_%s_n%d" % (_tag, _n)] = (_tag, _nqs, dict(n_contrib=_n))
    EDGES["ed_%s_min" % _tag] = (_tag, _nqs, dict(start_from_min=True))             # (both lower bounds are non-zero)
EDGES["ed_sphcs_gen12"] = ("sphcs", MATRIX_SHAPES[2], dict(gen=(1, 2)))
EDGES["ed_sphcs_gen30"] = ("sphcs", MATRIX_SHAPES[2], dict(gen=(3, 0)))
EDGES["ed_ellcs_nobg"] = ("ellcs", MATRIX_SHAPES[2], dict(find_bg=False))           # three active parameters
GENERATED = MATRIX + tuple(EDGES)


def generated_shape(name):
    """-> (model, set_nq, the slot count QPL of the instance the input is to select) of a generated input, without building it"""
    if name in EDGES:
        tag, nqs, _ = EDGES[name]
        return tag, nqs, {v: k for k, v in MATRIX_SHAPES.items()}[nqs]
    if name not in MATRIX:
        raise KeyError(name)
    tag, qpl = name[3:].rsplit("_q", 1)
    return tag, matrix_shape(tag, int(qpl)), int(qpl)


def generated_case(name, shared):
    """The generated input `name` for one scale mode -> case()'s dict plus set_nq, qpl, gen.  Per set: scales a factor >= 100 apart;
    shared: equal scales; both: different backgrounds.  12 contributions and 80 steps (Kholodenko: 8 and 60, at 16 slots 8 and 40, to
    keep its QUADPACK reference under 10 s), criterion 1e-12, no retry."""
    from helpers import make_models
    kw = dict(n_contrib=12, n_reps=1, max_iter=80, conv_crit=1e-12, max_retries=0)
    tag, nqs, qpl = generated_shape(name)
    gen = None
    if name in EDGES:
        diff = dict(EDGES[name][2])
        gen = diff.pop("gen", None)
        kw.update(diff)
    elif tag == "kholodenko":
        kw.update(n_contrib=8, max_iter=40 if qpl == 16 else 60)
    lo, hi, fixed = model_range(tag)
    S = len(nqs)
    scales = (SHARED_SCALE,) * S if shared else PER_SET_SCALES[:S]
    pop_seed = 300 + sum(map(ord, name)) % 97 + (50 if shared else 0)
    sets = population_sets(tag, nqs, scales, BACKGROUNDS[:S], pop_seed, lo, hi, **fixed)
    _, spec = make_models(tag, lo, hi, gen, **fixed)
    st = O.Settings(comp_exp=0.6666666, **kw)
    ndraw = (st.n_contrib + st.max_iter) * spec.n_active + 8
    seed = GENERATED_SEED.get((name, shared), 1)
    replay = np.random.RandomState(3000 + 1000 * seed + (500 if shared else 0) + sum(map(ord, name))).uniform(size=(1, ndraw))
    return dict(tag=tag, lo=lo, hi=hi, fixed=fixed, gen=gen, sets=sets, st=st, replay=replay, set_nq=tuple(nqs), qpl=qpl)


def case_models(c):
    """-> (product model, oracle spec) of a case() dict"""
    from helpers import make_models
    return make_models(c["tag"], c["lo"], c["hi"], c.get("gen"), **c["fixed"])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(tag, lo, hi, fixed, sets, st (O.Settings), replay [R][len]) of the named input."""
    from helpers import make_models
    if name in GENERATED:
        return generated_case(name, shared=False)
    tag, lo, hi, fixed = "sphere", [LO], [HI], {}
    kw = dict(n_contrib=20, n_reps=1, max_iter=300, conv_crit=1e-12, max_retries=0)
    if name.startswith("s1_"):                              # one set of 65 points: two slots, one nearly empty
        _, n, bg = name.split("_")
        sets = population_sets(tag, (65,), (3e4,), (2.,), 11, lo, hi)
        kw.update(n_contrib=int(n[1:]), find_bg=bg == "bg")
    elif name == "b2":                                      # slots 1 + 2 of 4: one slot is all padding
        sets = population_sets(tag, (37, 100), (2e3, 2e6), (0.5, 90.), 12, lo, hi)
    elif name == "b4":                                      # slots 1 + 1 + 1 + 3 of 8
        sets = population_sets(tag, (64, 3, 63, 130), (2e3, 2e6, 5e4, 2e5), (0.5, 90., 0., 7.), 13, lo, hi)
    elif name == "cyl":                                     # a row with an integral, two active parameters
        tag, lo, hi, fixed = "cyl_aspect", [2e-8, 0.5], [1e-7, 5.0], dict(intDiv=30)
        sets = population_sets(tag, (20, 70), (1e3, 4e5), (0.2, 30.), 14, lo, hi, **fixed)
        kw.update(n_contrib=8, max_iter=150)
    elif name in ("end_crit", "end_retry", "end_odd"):      # where the loop ends, on the inputs of b2
        sets = case("b2")["sets"]
        if name == "end_odd":
            kw.update(max_iter=100)                          # not a multiple of 64
        elif name == "end_retry":
            kw.update(max_iter=70, max_retries=2)            # the criterion below is set from the attempts' own ends
    else:
        raise KeyError(name)
    _, spec = make_models(tag, lo, hi, **fixed)
    st = O.Settings(comp_exp=0.6666666, **kw)
    P = spec.n_active
    ndraw = (st.max_retries + 1) * (st.n_contrib + st.max_iter) * P + 8
    replay = np.random.RandomState(1000 + sum(map(ord, name))).uniform(size=(1, ndraw))
    if name == "end_crit":
        # the criterion is reached inside a batch of 64 proposals: just above the chi² the chain has after the accepted move nearest to step 100
        traj = sets_mc_fit(spec, sets, st, O.ReplayStream(replay[0])).trajectory
        step, conval = min(traj, key=lambda t: abs(t[0] - 100))
        st.conv_crit = conval * (1. + 1e-6)
    elif name == "end_retry":
        # the first attempt ends unconverged at max_iter, a later one converges: the criterion lies between their best chi²
        stream = O.ReplayStream(replay[0])
        ends = [sets_mc_fit(spec, sets, st, stream).conval for _ in range(st.max_retries + 1)]
        later = min(ends[1:])
        assert later < ends[0], "end_retry: pick a stream whose later attempt ends lower (%r)" % (ends,)
        st.conv_crit = float(np.sqrt(later * ends[0]))
    return dict(tag=tag, lo=lo, hi=hi, fixed=fixed, sets=sets, st=st, replay=replay)


REPLAYED = ("s1_n5_bg", "s1_n5_nobg", "s1_n70_bg", "s1_n70_nobg", "b2", "b4", "cyl", "end_crit", "end_retry", "end_odd") + GENERATED


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's result on case(name), computed once."""
    c = case(name)
    _, spec = case_models(c)
    return sets_analyse(spec, c["sets"], c["st"], O.ReplayStream(c["replay"][0]))


def quickstart_sets(seed=5):
    """The quick-start tri-modal sphere population (radii 8 / 40 / 100 nm, widths 3 / 10 / 10 nm) on two overlapping q ranges of 50
    points: scales 1 and 250 (of a curve that is 1e4 at q = 1e7), backgrounds 0.2 and 30, 1 % noise."""
    from helpers import make_models
    _, spec = make_models("sphere", [np.pi / 1e9], [np.pi / 1e7])
    rng = np.random.RandomState(seed)
    radii = np.abs(np.concatenate([rng.normal(8e-9, 3e-9, 120), rng.normal(40e-9, 10e-9, 40), rng.normal(100e-9, 10e-9, 12)])) + 1e-9
    sets = []
    norm = O.model_calc(spec, np.array([1e7]), radii[:, None], 0.6666666)[0][0] / 1e4
    for q, A, b in ((np.logspace(7, 8.5, 50), 1., 0.2), (np.logspace(7.6, 9, 50), 250., 30.)):
        I = A * O.model_calc(spec, q, radii[:, None], 0.6666666)[0] / norm + b
        I = I * (1. + 0.01 * rng.standard_normal(len(q)))
        sets.append((q, I, 0.01 * np.abs(I)))
    return spec, sets

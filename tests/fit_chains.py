"""Shared by test_fit_exact_host.py and test_fit_exact_gpu.py: chains set down next to a good fit at any relative uncertainty u, their
oracle chains, and the bound of every step.  A plain module like helpers.py: nothing in here is collected.

Data: 16 sphere radii (the truth) inside a band of relative width delta around 10 nm, I = A0 sum rows(truth) + b0 + sigma xi,
sigma = u (A0 sum rows + b0); the start is the truth with every radius moved by a fraction of the band; the active range is the
band, so every proposal is a radius of the band.  The chains run CHAIN_STEPS replayed Philox steps to their budget (the criterion is
far below any chi-squared they reach: where a loop ends is test_chain_end_gpu.py's subject, not this one's).

What the chain's summed intensity ft is off by against the rows model_calc gives for the same set (input_error):
  - the two evaluators: a chain row is Contrib<SPHERE>::intensity_fast, model_calc's is ::intensity (sphere_row_gap);
  - the chain's own additions: N - 1 for the initial set (chain_body.inc `ft[j] += it[j]`, the first onto 0.0), two per accepted
    move (`test[j] = ft[j] + (inew[j] - test[j])`), each at most u times the largest ft of the history at that q (rows are >= 0);
    a row that leaves takes with it exactly the double that came (the cache, or the same evaluation again);
  - the reference's own ordered sum of N rows: (N + 1) u C."""
import functools

import numpy as np

import fit_exact as F
from exact import ABS_SINCOS, U, ULP_SINCOS
from mcsas_amd import engine
from oracle import mcsas_oracle as O
from helpers import make_models

N, REPS, CHAIN_STEPS, CAPACITY = 16, 3, 200, 200
SEED, REP_OFFSET = 5, 3
R0 = 1e-8
CRIT = 1e-9
# name: q-points, q slots per lane, waves per chain, execution mode
GEOMETRY = {"wave65": (65, 2, 1, engine.EXEC_WAVE), "wave200": (200, 4, 1, engine.EXEC_WAVE), "wave1500": (1500, 32, 1, engine.EXEC_WAVE),
            "wide1025": (1025, 8, 3, engine.EXEC_WORKGROUP)}
VARIANTS = {"free": (True, False), "nobg": (False, False), "posbg": (True, True)}


def sphere_row_gap(q, r, w):
    """Bound on |Contrib<SPHERE>::intensity_fast - ::intensity| of one row (models.h), both at the double x = q r, from the bounds
    test_formfactor_exact.py holds each of them to (sphere_hot_f, sphere_f), in doubles:
      g = fma(-x, cos x, sin x): |x| e_c + e_s + u |g| with sincos_fast's e = 1.6 ulp + 2e-26 on each
      ::intensity       div_fast(3. * g, x * x * x): 3 g one rounding, x^3 two, div_fast 2 u           -> 3 e_g / x^3 + 5 u |F|
      ::intensity_fast  (3. * g) * (q3inv * invr3): 3 g one rounding, q3inv invr3 within 10.1 u of x^-3, the product one
                                                                                                         -> 3 e_g / x^3 + 12.1 u |F|
      row = f * f * w: two roundings on (|F| + e_F)^2 w, and 2 |F| e_F + e_F^2 of f's error"""
    x = np.asarray(q, dtype=float) * float(r)
    s, c = np.sin(x), np.cos(x)
    es, ec = 2 * ULP_SINCOS * U * np.abs(s) + ABS_SINCOS, 2 * ULP_SINCOS * U * np.abs(c) + ABS_SINCOS
    g = np.abs(s - x * c)
    eg = np.abs(x) * ec + es + U * g
    g = g + eg
    x3 = x * x * x
    Fm = 3 * g / x3
    gap = 0.0
    for k in (5.0, 12.1):
        eF = (3 * eg / x3 + k * U * Fm) * (1 + 16 * U)
        gap = gap + w * (2 * Fm * eF + eF * eF) + 2 * U * w * (Fm + eF) ** 2
    return gap


def ordered_sum(rows):
    c = np.zeros(rows.shape[1])
    for row in rows:
        c = c + row
    return c


def input_error(rows, gaps, moves):
    """The states of a chain and what its ft is off by (module docstring).  rows, gaps: [N][nq] of the start set; moves: (index, row,
    gap) per accepted move -> [(C, eC)] for the start and after every move."""
    rows, gaps = np.array(rows, dtype=float), np.array(gaps, dtype=float)
    n = len(rows)
    C = ordered_sum(rows)
    M = C.copy()
    out = [(C, (n + 1) * U * C + (n - 1) * U * M + gaps.sum(axis=0))]
    for m, (i, row, gap) in enumerate(moves):
        rows[i], gaps[i] = row, gap
        C = ordered_sum(rows)
        M = np.maximum(M, C)
        out.append((C, (n + 1) * U * C + (n - 1 + 2 * (m + 1)) * U * M + gaps.sum(axis=0)))
    return out


# ------------------------------------------------------------------------------------------------- workloads and their oracle chains
def _oracle_steps(spec, q, I, sig, ost, stream, start):
    """tests/chain_cases.py::_oracle_traced with the model intensity and the chi-squared of EVERY bgfit_calc call kept: call 1 is the
    initial set's (mcsas.py:343), call 2 + s step s's candidate (mcsas.py:376)."""
    real_gen, real_fit = O.generate_parameters, O.bgfit_calc
    calls, props, fits, initial = [0], [], [], []

    def gen(spec_, stream_, count=1):
        calls[0] += 1
        if calls[0] == 1:                                           # the initial set: the start given, or (start None) the chain's own
            out = np.array(start, dtype=float) if start is not None else real_gen(spec_, stream_, count)
            assert count == len(out)
            initial.append(out.copy())
            return out
        out = real_gen(spec_, stream_, count)
        props.append(out[0].copy())
        return out

    def fit(I_, s_, C_, *a, **k):
        out = real_fit(I_, s_, C_, *a, **k)
        fits.append((np.array(C_, dtype=float), float(out[1])))
        return out

    O.generate_parameters, O.bgfit_calc = gen, fit
    try:
        ref = O.mc_fit(spec, q, I, sig, [I.min(), I.max()], [q.min(), q.max()], ost, stream, method="closed")
    finally:
        O.generate_parameters, O.bgfit_calc = real_gen, real_fit
    assert len(props) == ref.num_iter and len(fits) == 3 + ref.num_iter
    return dict(ref=ref, props=np.array(props).reshape(ref.num_iter, -1), fits=fits, pos=stream.pos, initial=initial[0])


@functools.lru_cache(maxsize=None)
def workload(geometry, u, variant, delta, frac, seed, n=N, steps=CHAIN_STEPS, cold=False):
    """Data, start and oracle chains (module docstring); cold: the chains draw their own initial set from the band instead.
    Computed once, shared, read-only."""
    N = n
    nq, slots, waves, mode = GEOMETRY[geometry] if isinstance(geometry, str) else geometry
    find_bg, pos_bg = VARIANTS[variant]
    q = np.logspace(8.0, 9.3, nq)
    lo, hi = R0 * (1 - delta / 2), R0 * (1 + delta / 2)
    m, spec = make_models("sphere", [lo], [hi])
    rs = np.random.RandomState(seed)
    truth = lo + (hi - lo) * rs.rand(N)
    ost = O.Settings(n_contrib=N, n_reps=1, max_iter=steps, conv_crit=CRIT, max_retries=0, find_bg=find_bg, pos_bg=pos_bg)
    C = ordered_sum(np.array([O.calc_intensity(spec, q, [r], ost.comp_exp)[0] for r in truth]))
    A0 = 1.0 / C.max()
    b0 = 1e-3 if variant == "free" else 0.0
    I0 = A0 * C + b0
    sig = u * I0
    I = I0 + sig * rs.standard_normal(nq)
    start = np.zeros((N, 1, REPS))
    for r in range(REPS):
        start[:, 0, r] = np.clip(truth + frac * (hi - lo) * (rs.rand(N) - 0.5), lo, hi)
    chains = [_oracle_steps(spec, q, I, sig, ost, O.PhiloxStream(SEED, REP_OFFSET + r, pos=0), None if cold else start[:, :, r])
              for r in range(REPS)]
    L = max(c["pos"] for c in chains)
    replay = np.stack([O.philox_uniform(SEED, REP_OFFSET + r, np.arange(L, dtype=np.uint64)) for r in range(REPS)])
    st = engine.Settings(n_contrib=N, n_reps=REPS, max_iter=steps, conv_crit=CRIT, max_retries=0, seed=SEED, rep_offset=REP_OFFSET,
                         find_background=find_bg, positive_background=pos_bg, exec_mode=mode)
    for a in (start, replay, I, sig, q):
        a.setflags(write=False)
    return dict(model=m, spec=spec, q=q, I=I, sig=sig, st=st, ost=ost, start=None if cold else start, replay=replay, chains=chains,
                slots=slots, waves=waves, find_bg=find_bg, pos_bg=pos_bg, u=u, band=(lo, hi))


def oracle_margins(wl):
    """Conditions (i)-(iii) of a workload, with the oracle alone: per chain chisq0, the number of moves, and the smallest
    margin / bound over its steps, margin = |chi2_t - chi2| / chi2 of the oracle, bound = the derived bound of that comparison
    (fit_exact.decision_bound, magnitudes from doubles; a candidate in the other positive-background branch than the current
    state: the two in-loop bounds, S no longer being common).  A step whose free b lies within its bound of 0 (positive background
    only) has no defined branch and is left out."""
    spec, q, I, sig, ost = wl["spec"], wl["q"], wl["I"], wl["sig"], wl["ost"]
    fb, pb, sl, wv = wl["find_bg"], wl["pos_bg"], wl["slots"], wl["waves"]
    out = []
    for ch, c in enumerate(wl["chains"]):
        ref, fits, props = c["ref"], c["fits"], c["props"]
        rows, gaps = [], []
        for r in c["initial"][:, 0]:
            it, _, w, _ = O.calc_intensity(spec, q, [r], ost.comp_exp)
            rows.append(it); gaps.append(sphere_row_gap(q, r, w))
        rows, gaps = np.array(rows), np.array(gaps)
        n = len(rows)
        M = ordered_sum(rows)
        moves, chi2 = 0, fits[1][1]

        def bounds(Cv, eC):
            x = F.approx_fit(I, sig, Cv, fb, pb)
            return x, F.chain_bounds(x, I, sig, Cv, fb, eC, sl, wv)

        def err_of(Cv, extra_moves, Mv, gsum):
            return (n + 1) * U * Cv + (n - 1 + 2 * (moves + extra_moves)) * U * Mv + gsum

        xc, bc = bounds(fits[1][0], err_of(fits[1][0], 0, M, gaps.sum(axis=0)))
        worst, undefined = np.inf, 0
        for s in range(ref.num_iter):
            Ct, chi2_t = fits[2 + s]
            i = s % n
            _, _, w, _ = O.calc_intensity(spec, q, props[s], ost.comp_exp)
            gnew = sphere_row_gap(q, props[s][0], w)
            Mt = np.maximum(M, Ct)
            xt, bt = bounds(Ct, err_of(Ct, 1, Mt, gaps.sum(axis=0) - gaps[i] + gnew))
            if pb and not (F.branch_is_defined(xt, bt) and F.branch_is_defined(xc, bc)):
                undefined += 1
            else:
                if xt["clamp"] == xc["clamp"]:
                    bound = F.decision_bound(bt["expl"], bc["expl"], xc["X"], xc["n"])
                else:
                    bound = bt["inloop"].e + bc["inloop"].e
                worst = min(worst, abs(chi2_t - chi2) / bound)
            if chi2_t < chi2:
                assert s in ref.accepted
                gaps[i], M, moves, chi2, xc, bc = gnew, Mt, moves + 1, chi2_t, xt, bt
        assert moves == ref.num_moves
        out.append(dict(chisq0=fits[1][1], moves=ref.num_moves, margin_over_bound=worst, undefined=undefined,
                        bound_rel=bc["inloop"].e / chi2, decision_rel=None))
    return out


def oracle_trace(c):
    """the oracle's trace of a chain: steps, chi-squared after each accepted move, the accepted values"""
    ref = c["ref"]
    return dict(chisq0=c["fits"][1][1], step=np.array(ref.accepted, dtype=np.int64),
                chisq=np.array([c["fits"][2 + s][1] for s in ref.accepted]), values=np.array([c["props"][s] for s in ref.accepted]))


def history_max(wl, ch):
    """the largest summed intensity per q over the history of the oracle's chain `ch` (its initial set and every accepted state):
    what a rounding of the chain's running ft is at most u times of"""
    c = wl["chains"][ch]
    M = c["fits"][1][0].copy()
    for s in c["ref"].accepted:
        M = np.maximum(M, c["fits"][2 + s][0])
    return M


# ------------------------------------------------------------------------------------------------- the chosen workloads
# (geometry, u, variant): (delta, fraction of the band the start is moved by, seed, decisions asserted).  Chosen with the oracle
# (oracle_margins) so that (i) every chisq0 lies in 1 .. 100, (ii) every chain accepts at least three moves, (iii) at every step
# the oracle's margin is at least ten times the derived bound of the comparison; test_fit_exact_host.py re-checks all three.
# delta = 30 u: a proposal then changes the intensity by about as much as the noise.  At u = 1e-6 none of the seeds 0 .. 19 meets
# (iii) in any geometry — the largest margin / bound over a seed's steps stays below 1, the bound of the in-loop chi-squared itself
# being 6 % (65 q) to 50 % (1500 q) of it: those rungs keep their chi-squared assertions and assert no decision.
CHOSEN = {
    ("wave65", 1e-2, "free"): (0.3, 0.3, 0, True), ("wave200", 1e-2, "free"): (0.3, 0.3, 0, True),
    ("wave1500", 1e-2, "free"): (0.3, 0.3, 0, True), ("wide1025", 1e-2, "free"): (0.3, 0.3, 0, True),
    ("wave65", 1e-4, "free"): (3e-3, 0.3, 0, True), ("wave200", 1e-4, "free"): (3e-3, 0.3, 2, True),
    ("wave1500", 1e-4, "free"): (3e-3, 0.3, 6, True), ("wide1025", 1e-4, "free"): (3e-3, 0.3, 1, True),
    ("wave65", 1e-6, "free"): (3e-5, 0.3, 0, False), ("wave200", 1e-6, "free"): (3e-5, 0.3, 0, False),
    ("wave1500", 1e-6, "free"): (3e-5, 0.3, 0, False), ("wide1025", 1e-6, "free"): (3e-5, 0.3, 2, False),
    ("wave65", 1e-2, "nobg"): (0.3, 0.3, 0, True), ("wave200", 1e-2, "nobg"): (0.3, 0.3, 1, True),
    ("wave1500", 1e-2, "nobg"): (0.3, 0.3, 0, True), ("wide1025", 1e-2, "nobg"): (0.3, 0.3, 0, True),
    ("wave65", 1e-2, "posbg"): (0.3, 0.3, 0, True), ("wave200", 1e-2, "posbg"): (0.3, 0.3, 1, True),
    ("wave1500", 1e-2, "posbg"): (0.3, 0.3, 0, True), ("wide1025", 1e-2, "posbg"): (0.3, 0.3, 0, True),
}


def chosen(key):
    delta, frac, seed, _ = CHOSEN[key]
    return workload(key[0], key[1], key[2], delta, frac, seed)


# the final fit of the modes that take neither a start nor a trace: cold chains in the band, 24 contributions, 150 steps, 1 % data
FINAL_N, FINAL_STEPS = 24, 150
FINAL_GEOMETRY = {65: (65, 2, 1, engine.EXEC_AUTO), 200: (200, 4, 1, engine.EXEC_AUTO)}


def final_workload(nq):
    return workload(FINAL_GEOMETRY[nq], 1e-2, "free", 0.3, 0.3, 0, n=FINAL_N, steps=FINAL_STEPS, cold=True)

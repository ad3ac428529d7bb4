"""The joint fit of several data sets with ONE scale for all of them (include/mcsas_hip.h: mcsas_hip_analyse_sets_mode with
MCSAS_SETS_SCALE_SHARED; csrc/chain_sets.h) and the histogram of a joint fit (mcsas_hip_histogram_sets; csrc/hist_kernels.h:
hist_fit_sets_kernel, hist_obs_sets_kernel), restated from the parts the other restatements are made of.  A plain module like
sets_exact.py: nothing in here is collected, nothing is fitted to a device's output.

The chain is tests/sets_exact.py's sets_mc_fit / sets_analyse with _fit_sets replaced by the shared solve, in float64 from
O.bgfit_closed's ingredients (the weighted sums of each set): with num_s = SIC - SI SC / Sw and den_s = SCC - SC² / Sw of set s (SIC and
SCC themselves without a background), A = sum num_s / sum den_s, b_s = (SI - A SC) / Sw, and X the direct residual sum at (A, b_s).
With one set the solve is sets_exact's own (O.bgfit_closed), as the kernel takes set_fit's operations there.

The histogram: the scale of every set is an input (the call's own output, as hist_exact.py takes A), held on its own by
fit_sets_bounds — the per-set closed form as fit_exact.py holds hist_fit_cum_kernel, the shared one operation for operation from the
same bounded sums — and fractions_bounds_sets is hist_exact.fractions_bounds with the limit taken over the points of the visible sets,
each point's product formed with its own set's scale: still five roundings (`w * A_ref / v` two, `A_s * row[k]` one,
`(sigma[k] * vf) / scaled` two), around sigma w A_ref / (v A_s row)."""
import contextlib
import functools
import math
from fractions import Fraction

import numpy as np

import fit_exact as F
import hist_exact as H
import sets_exact as SX
from exact import R, U, fma, gamma
from oracle import mcsas_oracle as O


# ------------------------------------------------------------------------------------------------ the chain
def _fit_sets_shared(sets, slices, C, find_bg):
    """-> (residual sum of every set at the shared optimum, [(A, b_s)])"""
    if len(sets) == 1:
        return SX_FIT_SETS(sets, slices, C, find_bg)
    parts = []
    for (q, I, sigma), sl in zip(sets, slices):
        err = np.array(sigma, dtype=float); err[err == 0.0] = 1.
        w = 1.0 / (err * err)
        c = C[sl]
        sw, swc, swcc, swi, swic = w.sum(), (w * c).sum(), (w * c * c).sum(), (w * I).sum(), (w * I * c).sum()
        num, den = (swic - swi * swc / sw, swcc - swc * swc / sw) if find_bg else (swic, swcc)
        parts.append((num, den, sw, swc, swi, err))
    A = sum(p[0] for p in parts) / sum(p[1] for p in parts)
    rs, sc = [], []
    for (q, I, sigma), sl, (num, den, sw, swc, swi, err) in zip(sets, slices, parts):
        b = (swi - A * swc) / sw if find_bg else 0.0
        rs.append(sum(((I - (C[sl] * A + b)) / err)**2)); sc.append((A, b))
    return np.array(rs), sc


SX_FIT_SETS = SX._fit_sets


@contextlib.contextmanager
def _shared_solve():
    SX._fit_sets = _fit_sets_shared
    try:
        yield
    finally:
        SX._fit_sets = SX_FIT_SETS


def sets_mc_fit(spec, sets, st, stream):
    with _shared_solve():
        return SX.sets_mc_fit(spec, sets, st, stream)


def sets_analyse(spec, sets, st, stream):
    with _shared_solve():
        return SX.sets_analyse(spec, sets, st, stream)


# the replay seeds, chosen on the CPU so that the restatement alone keeps |X_t - X| / X >= 1e-9 at every step (tests/test_sets_shared_host.py)
REPLAY_SEED = dict(sh2=1, sh4=1, sh_cyl=1, sh_nobg=1, sh_end_odd=1, sh_end_retry=3)
# ... and the shared twins of sets_exact's generated inputs (the instance matrix, the chain text's edges): the same names
REPLAYED = tuple(REPLAY_SEED) + SX.GENERATED


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(tag, lo, hi, fixed, sets, st (O.Settings), replay [1][len]) of the named input: one population seen through EQUAL scales
    and different backgrounds (sets_exact.population_sets)."""
    from helpers import make_models
    if name in SX.GENERATED:
        return SX.generated_case(name, shared=True)
    tag, lo, hi, fixed = "sphere", [SX.LO], [SX.HI], {}
    kw = dict(n_contrib=20, n_reps=1, max_iter=300, conv_crit=1e-12, max_retries=0)
    if name == "sh4":                                       # slots 1 + 1 + 1 + 3 of 8
        sets = SX.population_sets(tag, (64, 3, 63, 130), (2e4,) * 4, (0.5, 90., 0., 7.), 23, lo, hi)
    elif name == "sh_cyl":
        tag, lo, hi, fixed = "cyl_aspect", [2e-8, 0.5], [1e-7, 5.0], dict(intDiv=30)
        sets = SX.population_sets(tag, (20, 70), (1e4, 1e4), (0.2, 30.), 24, lo, hi, **fixed)
        kw.update(n_contrib=8, max_iter=150)
    elif name == "sh2":                                     # slots 1 + 2 of 4: one slot is all padding
        sets = SX.population_sets(tag, (37, 100), (2e4, 2e4), (0.5, 40.), 22, lo, hi)
    elif name in ("sh_nobg", "sh_end_odd", "sh_end_retry"):
        sets = case("sh2")["sets"]
        if name == "sh_nobg":
            kw.update(find_bg=False)
        elif name == "sh_end_odd":
            kw.update(max_iter=100)                          # not a multiple of 64
        else:
            kw.update(max_iter=70, max_retries=2)            # the criterion below is set from the attempts' own ends
    else:
        raise KeyError(name)
    _, spec = make_models(tag, lo, hi, **fixed)
    st = O.Settings(comp_exp=0.6666666, **kw)
    P = spec.n_active
    ndraw = (st.max_retries + 1) * (st.n_contrib + st.max_iter) * P + 8
    replay = np.random.RandomState(2000 + 100 * REPLAY_SEED[name] + sum(map(ord, name))).uniform(size=(1, ndraw))
    if name == "sh_end_retry":
        # the first attempt ends unconverged at max_iter, a later one converges: the criterion lies between their best chi²
        stream = O.ReplayStream(replay[0])
        ends = [sets_mc_fit(spec, sets, st, stream).conval for _ in range(st.max_retries + 1)]
        later = min(ends[1:])
        assert later < ends[0], "sh_end_retry: pick a stream whose later attempt ends lower (%r)" % (ends,)
        st.conv_crit = float(np.sqrt(later * ends[0]))
    return dict(tag=tag, lo=lo, hi=hi, fixed=fixed, sets=sets, st=st, replay=replay)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The shared restatement's result on case(name), computed once."""
    c = case(name)
    _, spec = SX.case_models(c)
    return sets_analyse(spec, c["sets"], c["st"], O.ReplayStream(c["replay"][0]))


# ------------------------------------------------------------------------------------------------ the histogram of a joint fit
SET_SHAPES = ((37, 100), (64, 3, 63, 130))
HIST_N, HIST_R = 12, 3
A_TRUE = 1e-3


def offsets(set_nq):
    return np.concatenate([[0], np.cumsum(set_nq)]).astype(int)


def hist_case(set_nq, rows_fn=None, seed=41):
    """12 sphere contributions x 3 repetitions on len(set_nq) q ranges, a `vol` histogram of 7 bins and a `num` one of 70 (more than one
    pass of 64); data: repetition 0's summed rows times ONE scale on a background of its own per set, 2 % uncertainties.
    rows_fn(q, pset[N][P]) -> (rows, v, w, s): the device's model_calc, or hist_exact.fake_rows where there is none."""
    nq = int(sum(set_nq))
    c = H._case("sets_%d" % len(set_nq), HIST_N, HIST_R, nq, [H.spec(0, "vol", 7, "log"), H.spec(0, "num", 70, "lin")], seed, P=1,
                builtin="sphere")
    c["q"] = np.concatenate([np.geomspace(1e8 * 1.5 ** s, 2e9 * 1.2 ** s, n) for s, n in enumerate(set_nq)])
    c["set_nq"] = tuple(int(n) for n in set_nq)
    H.finish(c, lambda pset: (rows_fn or H.fake_rows)(c["q"], pset))
    cum = c["rows"][0].sum(axis=0)
    k = np.arange(nq)
    off = offsets(set_nq)
    bg = np.concatenate([np.full(n, 0.02 * (1 + 3 * s) * A_TRUE * cum.mean()) for s, n in enumerate(set_nq)])
    c["I"] = A_TRUE * cum * (1.0 + 0.01 * np.cos(1.7 * k)) + bg
    c["sigma"] = 0.02 * c["I"] * (1.0 + 0.5 * np.sin(0.9 * k) ** 2)
    c["off"] = off
    return c


def cum_of(c, r):
    """hist_colsum_body: the rows of a repetition added in contribution order"""
    cum = np.zeros(c["nq"])
    for i in range(c["N"]):
        cum = cum + c["rows"][r, i]
    return cum


@F.exactly
def fit_sets_bounds(c, r, shared):
    """hist_fit_sets_kernel for repetition r -> [(A, b)] per set as exact.R.  The six sums of each set are hist_fit_cum_body's on the set's
    own points (fit_exact.sums_bgfit; the input error of cum: the (N + 1) u C of an ordered sum of N positive rows).  Per set (and
    with one set): solve_fit, fit_exact.bgfit_bounds.  Shared: `num = fma(-(si / sw), sc, sic); den = fma(-(sc * (1.0 / sw)), sc, scc);
    Num += num; Den += den` (the first onto 0.0 exact), `A = Num / Den`, `b = (si - A * sc) / sw`."""
    off, find_bg = c["off"], c["find_bg"]
    C = cum_of(c, r)
    S = len(off) - 1
    out, parts = [], []
    for s in range(S):
        sl = slice(off[s], off[s + 1])
        I, sg, Cs = c["I"][sl], c["sigma"][sl], C[sl]
        eC = (c["N"] + 1) * U * Cs
        x = F.exact_fit(I, sg, Cs, find_bg, False)
        if not shared or S == 1:
            bd = F.bgfit_bounds(x, I, sg, Cs, find_bg, 1, eC=eC)
            out.append((bd["A"], bd["b"]))
        else:
            parts.append(F.sums_bgfit(x, I, sg, Cs, eC))
    if parts:
        Num = Den = None
        for p in parts:
            num, den = p["SIC"], p["SCC"]
            if find_bg:
                num = fma(-(p["SI"] / p["Sw"]), p["SC"], p["SIC"])
                den = fma(-(p["SC"] * (1.0 / p["Sw"])), p["SC"], p["SCC"])
            Num = num if Num is None else Num + num
            Den = den if Den is None else Den + den
        A = Num / Den
        out = [(A, (p["SI"] - A * p["SC"]) / p["Sw"] if find_bg else R(0)) for p in parts]
    return out


def point_scales(c, set_A, r):
    """the scale of each point's own set, [nq]"""
    return np.concatenate([np.full(n, float(set_A[s][r])) for s, n in enumerate(c["set_nq"])])


def visible_points(c, visible):
    return np.concatenate([np.full(n, s in visible, dtype=bool) for s, n in enumerate(c["set_nq"])])


def limit_bound_sets(sigma, row, v, w, A_ref, A_pt, vis):
    """hist_obs_sets_kernel for one (c, r): min over the kept points k of the visible sets of (sigma[k] vf) / (A_s(k) row[k]) with
    vf = w A_ref / v, +inf where none is kept (hist_exact.limit_bound with the per-point scale)"""
    with np.errstate(under="ignore"):
        keep = vis & (np.asarray(A_pt, dtype=np.float64) * np.asarray(row, dtype=np.float64) != 0.0)
    if not keep.any():
        return math.inf
    if v == 0.0 or not math.isfinite(w * A_ref / v if v else math.inf):
        with np.errstate(all="ignore"):
            vf = np.float64(w) * np.float64(A_ref) / np.float64(v)
            best = float(np.fmin.reduce((sigma[keep] * vf) / (A_pt[keep] * row[keep]), initial=np.inf))
        assert not math.isfinite(best)
        return best
    f = Fraction(float(w)) * Fraction(float(A_ref)) / Fraction(float(v))
    return H.min_within([Fraction(float(s)) * f / (Fraction(float(a)) * Fraction(float(x)))
                         for s, a, x in zip(sigma[keep], A_pt[keep], row[keep])], gamma(H.LIMIT_ROUNDINGS))


@F.exactly
def fractions_bounds_sets(c, A_ref, set_A, visible):
    """hist_exact.fractions_bounds with hist_obs_sets_kernel's limits: A_ref[R] the reference scale, set_A[S][R] every set's"""
    N, nrep = c["N"], c["R"]
    vis = visible_points(c, visible)
    out = {k: np.empty((N, nrep), dtype=object) for k in H.FRAC8}
    for r in range(nrep):
        Ar = R(float(A_ref[r]))
        A_pt = point_scales(c, set_A, r)
        for i in range(N):
            v, w, s = R(c["v"][i, r]), R(c["w"][i, r]), R(c["s"][i, r])
            vf = H.div(H.mul(w, Ar), v)
            nf = H.div(vf, v)
            m = limit_bound_sets(c["sigma"], c["rows"][r, i], c["v"][i, r], c["w"][i, r], float(A_ref[r]), A_pt, vis)
            mn = H.div(m, v)
            vals = dict(vf=vf, nf=nf, qf=H.mul(vf, v), sf=H.mul(nf, s), mv=m, mn=mn, mq=H.mul(H.mul(mn, m), m), ms=H.mul(mn, s))
            for k in H.FRAC8:
                out[k][i, r] = vals[k]
        for f, m in (("nf", "mn"), ("qf", "mq"), ("sf", "ms")):
            t = H.seq(out[f][:, r])
            if not H.is_zero(t):
                for i in range(N):
                    out[f][i, r] = H.div(out[f][i, r], t)
                    out[m][i, r] = H.div(out[m][i, r], t)
    return out


def all_bounds_sets(c, A_ref, set_A, visible):
    """-> (fractions, [histogram][repetition] of hist_exact.histogram_bounds), hist_exact.look_triple's `bounds`"""
    fr = fractions_bounds_sets(c, A_ref, set_A, visible)
    return fr, [[H.histogram_bounds(c, fr, sp, r) for r in range(c["R"])] for sp in c["specs"]]


def emu_fit_sets(c, r, shared):
    """hist_fit_sets_kernel in numpy doubles, the lane order folded into plain sums (a magnitude check for the host test) -> [(A, b)]"""
    off, find_bg = c["off"], c["find_bg"]
    C = cum_of(c, r)
    sets = [(None, c["I"][off[s]:off[s + 1]], c["sigma"][off[s]:off[s + 1]]) for s in range(len(off) - 1)]
    slices = [slice(off[s], off[s + 1]) for s in range(len(off) - 1)]
    fit = _fit_sets_shared if shared else SX_FIT_SETS
    return fit(sets, slices, C, find_bg)[1]

"""Shared by test_fit_exact_host.py and test_fit_exact_gpu.py: the scale / background fit and the chi-squared of a Monte-Carlo step
(csrc/chain_common.h solve_fit, the centred test of chain_body.inc, host_calls.hip bgfit_kernel) as
  - exact values (mpmath, 60 digits) of the discrete operation at the doubles given,
  - bounds derived from the kernels' operation order (tests/exact.py: R, V, reduced_sum), and
  - numpy fp64 emulations of the same order (lane i & 63, slot i >> 6, the tree of wave_sum3),
and the cases of the one-call fits.  A plain module like helpers.py: nothing in here is collected.

Every bound is a count of rounded operations read off the source, propagated by the rules of exact.py; the line a count was read
from stands next to it.  Nothing is fitted to a device's output."""
from fractions import Fraction

import mpmath as mp
import numpy as np

from exact import R, U, V, fma, gamma, reduced_sum, slots_of, sum_roundings, sum_roundings_sequential

DPS = 60
exactly = mp.workdps(DPS)          # decorator: mpmath arithmetic of the function at 60 digits, whatever the importing module set


# ------------------------------------------------------------------------------------------------- exact values
def approx_fit(I, sigma, C, find_bg, pos_bg):
    """exact_fit's record from doubles (products rounded, sums by fs, the fit in doubles): MAGNITUDES for a bound where no
    exact value is compared with anything — the bound of every step of a chain (fit_chains.py), a thousand times cheaper."""
    fs = lambda v: float(np.sum(v))                             # (pairwise: a magnitude needs no more)
    I, C = np.asarray(I, dtype=float), np.asarray(C, dtype=float)
    e = np.where(np.asarray(sigma, dtype=float) == 0.0, 1.0, np.asarray(sigma, dtype=float))
    w = 1.0 / (e * e)
    n = len(I)
    s = dict(Sw=fs(w), SI=fs(w * I), SII=fs(w * I * I), SC=fs(w * C), SCC=fs(w * C * C),
             SIC=fs(w * I * C), Ss2=fs(e * e))
    b_free, clamp = None, False
    if find_bg:
        Cm, Im = s["SC"] / s["Sw"], s["SI"] / s["Sw"]                # centred: the doubles keep their digits
        A = fs(w * (I - Im) * (C - Cm)) / fs(w * (C - Cm) ** 2)
        b = b_free = Im - A * Cm
        clamp = bool(pos_bg) and b < 0
    if not find_bg or clamp:
        A, b = s["SIC"] / s["SCC"], 0.0
    r = I - A * C - b
    X = fs(w * r * r)
    Sx = fs(w * (I - s["SI"] / s["Sw"]) ** 2) if (find_bg and not clamp) else s["SII"]
    out = {k: mp.mpf(v) for k, v in s.items()}
    out.update(n=n, A=mp.mpf(A), b=mp.mpf(b), b_free=None if b_free is None else mp.mpf(b_free), clamp=clamp, X=mp.mpf(X),
               chi2=mp.mpf(X / n), r2=mp.mpf(fs(r * r)), expl=mp.mpf(Sx - X), agofs=None, absr=np.abs(r))
    return out


@exactly
def exact_fit(I, sigma, C, find_bg, pos_bg, num_params=1):
    """The weighted sums, the minimiser of sum ((I - A C - b) / e)^2 and the chi-squared there, at the doubles given, e = sigma
    with 0 -> 1 (backgroundscalingfit.py:117).  b_free is the background of the free optimum (None without one): its sign
    decides the positive-background branch."""
    I, C = [mp.mpf(float(x)) for x in I], [mp.mpf(float(x)) for x in C]
    e = [mp.mpf(1) if float(s) == 0.0 else mp.mpf(float(s)) for s in sigma]
    w = [1 / (x * x) for x in e]
    n = len(I)
    s = dict(Sw=mp.fsum(w), SI=mp.fsum(w[i] * I[i] for i in range(n)), SII=mp.fsum(w[i] * I[i] * I[i] for i in range(n)),
             SC=mp.fsum(w[i] * C[i] for i in range(n)), SCC=mp.fsum(w[i] * C[i] * C[i] for i in range(n)),
             SIC=mp.fsum(w[i] * I[i] * C[i] for i in range(n)), Ss2=mp.fsum(x * x for x in e))
    b_free, clamp = None, False
    if find_bg:
        det = s["Sw"] * s["SCC"] - s["SC"] ** 2
        A = (s["Sw"] * s["SIC"] - s["SI"] * s["SC"]) / det
        b = b_free = (s["SI"] - A * s["SC"]) / s["Sw"]
        clamp = bool(pos_bg) and b < 0
    if not find_bg or clamp:
        A, b = s["SIC"] / s["SCC"], mp.mpf(0)
    r = [I[i] - A * C[i] - b for i in range(n)]
    X = mp.fsum(w[i] * r[i] * r[i] for i in range(n))
    r2 = mp.fsum(x * x for x in r)
    centred = find_bg and not clamp
    Sx = s["SII"] - s["SI"] ** 2 / s["Sw"] if centred else s["SII"]
    return dict(s, n=n, A=A, b=b, b_free=b_free, clamp=clamp, X=X, chi2=X / n, r2=r2, expl=Sx - X,
                agofs=r2 / s["Ss2"] * (mp.mpf(n) / (n - num_params)) if n != num_params else None, absr=np.array([abs(float(x)) for x in r]))


# ------------------------------------------------------------------------------------------------- derived bounds
def _weights(sigma):
    """e e (one rounding) and w = 1.0 / (e e) (one more) as the kernels and the host make them:
    host_calls.hip `double w = 1.0 / (e * e);`, host_internal.h `double wi = 1.0 / (e * e);`"""
    e = np.where(np.asarray(sigma, dtype=float) == 0.0, 1.0, np.asarray(sigma, dtype=float))
    ee = V(e) * V(e)
    return e, ee, 1.0 / ee


@exactly
def sums_bgfit(x, I, sigma, C, eC=0.0):
    """The six sums of bgfit_kernel / hist_fit_cum_body as R, terms in the source's order (-ffp-contract=off: every product
    rounded): `sw += w; si += w * I[k]; sii += w * I[k] * I[k]; sc += w * C[k]; scc += w * C[k] * C[k]; sic += w * I[k] * C[k];
    ss2 += e * e`; each through sum_roundings(slots) additions.  eC: bound on the error of C per point (an input error)."""
    _, ee, w = _weights(sigma)
    Iv, Cv = V(I), V(C, eC)
    k = sum_roundings(slots_of(len(I)))
    return dict(Sw=reduced_sum(x["Sw"], w, k), SI=reduced_sum(x["SI"], w * Iv, k), SII=reduced_sum(x["SII"], (w * Iv) * Iv, k),
                SC=reduced_sum(x["SC"], w * Cv, k), SCC=reduced_sum(x["SCC"], (w * Cv) * Cv, k),
                SIC=reduced_sum(x["SIC"], (w * Iv) * Cv, k), Ss2=reduced_sum(x["Ss2"], ee, k))


@exactly
def sums_chain(x, I, sigma, C, eC=0.0, slots=None, waves=1):
    """The sums a chain kernel works with.  Sw, SI, SII come from the host (host_internal.h WeighedData: `Sw += wi; SI += wi * I;
    SII += wi * I * I` in order: nq - 1 additions), as do w and wI = fl(w I).  The three sums of a step, chain_body.inc:
    `double wt = CHAIN_W(j) * test[j]; s1 += wt; s2 = fma(wt, test[j], s2); s3 = fma(CHAIN_WI(j), test[j], s3);` — wt rounded, the
    two products inside fma not — through sum_roundings(slots, waves)."""
    _, ee, w = _weights(sigma)
    Iv, Cv = V(I), V(C, eC)
    n = len(I)
    kh = sum_roundings_sequential(n)
    k = sum_roundings(slots if slots is not None else slots_of(n), waves)
    wI = w * Iv
    wt = w * Cv
    return dict(Sw=reduced_sum(x["Sw"], w, kh), SI=reduced_sum(x["SI"], wI, kh), SII=reduced_sum(x["SII"], wI * Iv, kh),
                SC=reduced_sum(x["SC"], wt, k), SCC=reduced_sum(x["SCC"], wt.times(Cv, rounded=False), k),
                SIC=reduced_sum(x["SIC"], wI.times(Cv, rounded=False), k))


def _twice(a):
    return R(2 * a.v, 2 * a.e)          # 2. * x is exact


@exactly
def solve_fit_R(s, n, find_bg, clamp):
    """chain_common.h solve_fit, operation for operation, on sums with bounds: -> (A, b, chi2, free b).
        det = Sw * SCC - SC * SC;  A = (Sw * SIC - SI * SC) / det;  b = (SI - A * SC) / Sw;           (3, 4 and 3 roundings)
        [b < 0 and pos_bg, or no background:  A = SIC / SCC;  b = 0]                                   (1 rounding)
        q2 = SII - 2. * A * SIC - 2. * b * SI + A * A * SCC + 2. * A * b * SC + b * b * Sw;           (13 roundings; 2. * x exact)
        chi2 = q2 / (double)nq                                                                         (1 rounding)
    `clamp` says which branch the exact fit takes; a case whose free b lies within its bound of 0 has no defined branch."""
    Sw, SI, SII, SC, SCC, SIC = (s[k] for k in ("Sw", "SI", "SII", "SC", "SCC", "SIC"))
    bf = None
    if find_bg:
        det = Sw * SCC - SC * SC
        A = (Sw * SIC - SI * SC) / det
        b = bf = (SI - A * SC) / Sw
    if not find_bg or clamp:
        A, b = SIC / SCC, R(0)
    q2 = SII - _twice(A) * SIC - _twice(b) * SI + (A * A) * SCC + (_twice(A) * b) * SC + (b * b) * Sw
    return A, b, q2 / R(n), bf


@exactly
def centred_R(s, n, centred):
    """The chi-squared of a step as chain_body.inc takes it (and chain_wg.h, pipe_scan.h, chain_feed.h after it):
        invSw = 1.0 / Sw, SIoSw = SI / Sw, Scen = SII - SI * SI / Sw                                   (1, 1 and 3 roundings)
        numc = fma(-SIoSw, s1, s3), denc = fma(-(s1 * invSw), s1, s2)                                  (1 and 2 roundings)
        X = S - num * num / den;  chi2 = X / nqd                                                       (3 and 1 roundings)
    with S = Scen, num = numc, den = denc when a background is fitted and not clamped (`centred`), else S = SII, num = s3, den = s2.
    -> (chi2, explained = num num / den, S): S is one double for the whole chain, so its error is common to every chi2 of the
    chain and absent from the comparison of two of them (decision_bound)."""
    Sw, SI, SII, s1, s2, s3 = (s[k] for k in ("Sw", "SI", "SII", "SC", "SCC", "SIC"))
    if centred:
        invSw, SIoSw = 1.0 / Sw, SI / Sw
        S = SII - (SI * SI) / Sw
        num, den = fma(-SIoSw, s1, s3), fma(-(s1 * invSw), s1, s2)
    else:
        S, num, den = SII, s3, s2
    expl = (num * num) / den
    return (S - expl) / R(n), expl, S


def decision_bound(expl_t, expl_cur, X_cur, n):
    """Bound on the error of chi2_t - chi2 as the comparison `num * num > (S - X) * den` (chain_body.inc) sees it, both states in
    the same branch: the two explained sums' own errors (centred_R; the division of the left side stands for the product of the
    right), and on the right `X = S - num * num / den` (one rounding of X when the current state was accepted), `S - X` (one of
    the difference, which is the explained sum) and `(S - X) * den` (one of the product): u |X| + 2 u explained."""
    return (expl_t.e + expl_cur.e + U * abs(float(X_cur)) + 2 * U * abs(float(expl_cur.v))) / n


@exactly
def residual_R(x, I, sigma, C, A, b, kind, eC=0.0, slots=None, waves=1):
    """The residual chi-squared at the COMPUTED scale and background (bounds A.e, b.e) against the exact chi-squared at the exact
    optimum, and bgfit's aGoFs numerator sum r^2 -> (chi2, r2) as R.
      r = I - (C * A + b): three roundings, u |C A| + u |C A + b| + u |r|, and |A| eC of the input       (rho)
      the fit's own error d = C dA + db enters chi2 only in second order — sum w r C = 0 and sum w r = 0 at the optimum (with a
      clamped or absent background db = 0 and the first alone is needed) — as sum w d^2 <= (|dA| sqrt(SCC) + |db| sqrt(Sw))^2;
      so sum w r^2 is off by at most Q + 2 sum w (|r| + |d|) rho + sum w rho^2.  sum r^2 (no weights: nothing vanishes) is off by
      2 sum |r| (|d| + rho) + sum (|d| + rho)^2.
      bgfit_kernel: `rs += (r / e) * (r / e); r2 += r * r;`  three roundings / one per term; chain_body.inc: `rs += CHAIN_W(j) * r * r;`
      two, and w's own two (_weights); then the sum's path, then `/ nq` (one)."""
    e, ee, w = _weights(sigma)
    n = len(I)
    I, C = np.asarray(I, dtype=float), np.asarray(C, dtype=float)
    Av, bv = abs(float(A.v)), abs(float(b.v))
    absr = x["absr"]
    wx = 1.0 / (e * e)
    rho = U * np.abs(C) * Av + U * (np.abs(C) * Av + bv) + U * absr + Av * eC
    d = (np.abs(C) + eC) * A.e + b.e
    Q = (A.e * float(mp.sqrt(x["SCC"])) + b.e * float(mp.sqrt(x["Sw"]))) ** 2
    dX = Q + 2 * np.sum(wx * (absr + d) * rho) + np.sum(wx * rho * rho)
    k = sum_roundings(slots if slots is not None else slots_of(n), waves)
    per_term = gamma(3) if kind == "bgfit" else gamma(2) + float(np.max(w.e / w.a))
    Xf = float(x["X"])
    chi2 = R(x["X"], dX + ((1 + per_term) * (1 + gamma(k)) - 1) * (Xf + dX)) / R(n)
    dd = d + rho
    d2 = 2 * np.sum(absr * dd) + np.sum(dd * dd)
    r2 = R(x["r2"], d2 + ((1 + gamma(1)) * (1 + gamma(k)) - 1) * (float(x["r2"]) + d2))
    return chi2, r2


@exactly
def bgfit_bounds(x, I, sigma, C, find_bg, num_params, eC=0.0):
    """What bgfit_kernel writes, as R: out[0] = A, out[1] = b, out[2] = rs / nq, out[3] = r2 / ss2 * ((double)nq / (double)(nq -
    num_params)) (two divisions and a product on top of the sums); and the free b with its bound."""
    s = sums_bgfit(x, I, sigma, C, eC)
    A, b, _, bf = solve_fit_R(s, x["n"], find_bg, x["clamp"])
    chi2, r2 = residual_R(x, I, sigma, C, A, b, "bgfit", eC)
    n = x["n"]
    agofs = (r2 / s["Ss2"]) * (R(n) / R(n - num_params)) if n > num_params else None
    return dict(A=A, b=b, chi2=chi2, agofs=agofs, b_free=bf)


@exactly
def within(got, ref):
    """|got - exact| / bound (<= 1: inside)."""
    err = float(abs(mp.mpf(float(got)) - ref.v))
    if err == 0.0:
        return 0.0
    return err / ref.e if ref.e > 0 else np.inf


# ------------------------------------------------------------------------------------------------- emulations, numpy fp64
def fma64(a, b, c):
    """fma(a, b, c) of doubles: the exact a b + c rounded once."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def tree(v):
    """device_util.h wave_sum3 over 64 lane values: xor 1, xor 2, half-mirror, mirror, row_bcast15, row_bcast31 — six pairwise levels
    (an addition commutes, so the neighbour's order within a pair does not matter)."""
    v = np.asarray(v, dtype=np.float64)
    assert v.shape[-1] == 64
    for _ in range(6):
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def layout(x, slots, waves=1):
    """x[i] at [wave][slot][lane], i = 64 (slots wave + slot) + lane (one wave: lane i & 63, slot i >> 6), zeros behind"""
    out = np.zeros(64 * slots * waves)
    out[:len(x)] = x
    return out.reshape(waves, slots, 64)


def lane_sum(t, dtype=np.float64):
    """terms [wave][slot][lane] -> the kernel's sum: slots in order per lane, the tree, the waves in order"""
    acc = np.zeros((t.shape[0], 64), dtype=dtype)
    for j in range(t.shape[1]):
        acc = acc + t[:, j, :].astype(dtype)
    tot = 0.0
    for v in tree(acc.astype(np.float64)):
        tot = tot + float(v)
    return tot


def lane_sum_fma(x, y):
    """s = fma(x, y, s) per lane over the slots, then as lane_sum"""
    acc = np.zeros((x.shape[0], 64))
    for j in range(x.shape[1]):
        for wv in range(x.shape[0]):
            for l in range(64):
                if x[wv, j, l] != 0.0 and y[wv, j, l] != 0.0:
                    acc[wv, l] = fma64(x[wv, j, l], y[wv, j, l], acc[wv, l])
    tot = 0.0
    for v in tree(acc):
        tot = tot + float(v)
    return tot


def emu_solve_fit(Sw, SI, SII, SC, SCC, SIC, n, find_bg, pos_bg):
    """chain_common.h solve_fit in Python doubles"""
    if find_bg:
        det = Sw * SCC - SC * SC
        A = (Sw * SIC - SI * SC) / det
        b = (SI - A * SC) / Sw
        if pos_bg and b < 0.:
            A, b = SIC / SCC, 0.
    else:
        A, b = SIC / SCC, 0.
    q2 = SII - 2. * A * SIC - 2. * b * SI + A * A * SCC + 2. * A * b * SC + b * b * Sw
    return A, b, q2 / float(n)


def emu_bgfit(I, sigma, C, find_bg, pos_bg, num_params=1, mutate=None):
    """host_calls.hip bgfit_kernel -> out[0..3].  mutate: "f32" (scc accumulated in float32), "w32" (w = (1 / e)^2 in float32),
    "drop" (the last slot of lane 0 left out of every sum)."""
    I, C = np.asarray(I, dtype=float), np.asarray(C, dtype=float)
    n, sl = len(I), slots_of(len(I))
    e = np.where(np.asarray(sigma, dtype=float) == 0.0, 1.0, np.asarray(sigma, dtype=float))
    w = 1.0 / (e * e)
    if mutate == "w32":
        w = ((np.float32(1.0) / e.astype(np.float32)) ** 2).astype(np.float64)
    keep = np.ones(n)
    if mutate == "drop":
        keep[64 * (sl - 1)] = 0.0
    L = lambda t: layout(t * keep, sl)
    sw, si, sii = lane_sum(L(w)), lane_sum(L(w * I)), lane_sum(L(w * I * I))
    sc, sic = lane_sum(L(w * C)), lane_sum(L(w * I * C))
    scc = lane_sum(L(w * C * C), np.float32 if mutate == "f32" else np.float64)
    ss2 = lane_sum(L(e * e))
    A, b, _ = emu_solve_fit(sw, si, sii, sc, scc, sic, n, find_bg, pos_bg)
    r = I - (C * A + b)
    rs, r2 = lane_sum(L((r / e) * (r / e))), lane_sum(L(r * r))
    return np.array([A, b, rs / n, r2 / ss2 * (float(n) / float(n - num_params)) if n != num_params else np.nan])


def emu_chain(I, sigma, C, find_bg, pos_bg, slots=None, waves=1, mutate=None):
    """What a chain kernel computes of a state with summed intensity C (chain_body.inc), in its order: -> dict(chisq0: solve_fit's
    expansion; A, b; inloop: the centred X / nq; expl: num num / den; final: the residual chi-squared at A, b).
    mutate: "f32" (s2 accumulated in float32), "uncentred" (the expansion where the step has the centred form: inloop and expl are
    taken from solve_fit's q2), "drop" (lane 0's last slot left out), "w32" (w = (1 / e)^2 in float32)."""
    I, C = np.asarray(I, dtype=float), np.asarray(C, dtype=float)
    n = len(I)
    sl = slots if slots is not None else slots_of(n)
    e = np.where(np.asarray(sigma, dtype=float) == 0.0, 1.0, np.asarray(sigma, dtype=float))
    w = 1.0 / (e * e)
    if mutate == "w32":
        w = ((np.float32(1.0) / e.astype(np.float32)) ** 2).astype(np.float64)
    wI = w * I
    Sw = SI = SII = 0.0
    for i in range(n):                                            # host_internal.h WeighedData
        Sw += w[i]; SI += w[i] * I[i]; SII += w[i] * I[i] * I[i]
    Sw, SI, SII = float(Sw), float(SI), float(SII)
    keep = np.ones(n)
    if mutate == "drop":
        keep[64 * (slots_of(n) - 1)] = 0.0
    Lw, LwI, LC = layout(w * keep, sl, waves), layout(wI * keep, sl, waves), layout(C, sl, waves)
    wt = Lw * LC
    s1 = lane_sum(wt)
    s2 = lane_sum(wt * LC, np.float32) if mutate == "f32" else lane_sum_fma(wt, LC)
    s3 = lane_sum_fma(LwI, LC)
    A, b, chisq0 = emu_solve_fit(Sw, SI, SII, s1, s2, s3, n, find_bg, pos_bg)
    nqd, invSw, SIoSw, Scen = float(n), 1.0 / Sw, SI / Sw, SII - SI * SI / Sw
    S, num, den = SII, s3, s2
    if find_bg:
        numc, denc = fma64(-SIoSw, s1, s3), fma64(-(s1 * invSw), s1, s2)
        neg_b = pos_bg and fma64(SI, denc, -(numc * s1)) < 0.
        if not neg_b:
            S, num, den = Scen, numc, denc
    expl = num * num / den
    X = S - expl
    if mutate == "uncentred":
        X = chisq0 * nqd
        expl = S - X
    r = I - (C * A + b)
    final = lane_sum(layout(w * keep * r * r, sl, waves)) / nqd
    return dict(chisq0=chisq0, A=A, b=b, inloop=X / nqd, expl=expl, final=final)


@exactly
def chain_bounds(x, I, sigma, C, find_bg, eC=0.0, slots=None, waves=1):
    """The bounds of what emu_chain returns (and a chain kernel records), as R, from the exact fit x = exact_fit(...)."""
    s = sums_chain(x, I, sigma, C, eC, slots, waves)
    A, b, chisq0, bf = solve_fit_R(s, x["n"], find_bg, x["clamp"])
    inloop, expl, S = centred_R(s, x["n"], find_bg and not x["clamp"])
    chisq0 = R(x["chi2"], chisq0.e)                                # (the expansion's value IS the chi-squared at the optimum)
    inloop = R(x["chi2"], inloop.e)
    final, _ = residual_R(x, I, sigma, C, A, b, "chain", eC, slots, waves)
    return dict(A=A, b=b, chisq0=chisq0, inloop=inloop, expl=R(x["expl"], expl.e), final=final, b_free=bf, S=S)


# ------------------------------------------------------------------------------------------------- the cases of the one-call fits
NQS = (2, 3, 63, 64, 65, 127, 129, 1000)
FLAGS = ((True, False, "free"), (False, False, "nobg"), (True, True, "clamped"), (True, True, "posb"))
LADDER = (tuple(("u%g" % u, u, None) for u in (1e-2, 1e-4, 1e-6)) + tuple(("flat%g" % eps, 1e-2, eps) for eps in (1.0, 1e-3, 1e-6))
          + (("bg1000", 1e-6, None),))
# (the last rung: a background a thousand times the signal under the curve itself — the data are flat, the model is not: the one
# regime in which centring the sums buys anything, see test_fit_exact_host.py::test_degraded_emulations_fall_outside)
SI_I, SI_C = 3e-28, 7e-43          # intensities of 1e-30 .. 1e-25 (SI units), model intensities far below


def shape(nq):
    """a smooth curve over two decades, no zeros (so that sigma = u I stays away from 0): a Guinier-Porod-like fall plus a floor"""
    xq = np.logspace(-1, np.log10(8.0), nq) if nq > 1 else np.array([1.0])
    return 1.0 / (1.0 + xq * xq) ** 2 + 0.01


def fit_case(nq, flags, rung, si_units, zeros=False, seed=0):
    """-> dict(I, sigma, C, find_bg, pos_bg): I = A0 C + b0 + sigma xi, sigma = u (A0 C + b0); the rung's C is the curve itself or
    the nearly flat c0 (1 + eps curve).  b0 < 0 for "clamped" (the free optimum has b < 0), > 0 for "free" and "posb", 0 for "nobg".
    zeros: sigma = 0 exactly at lanes 0 and 63 and in the last, partial slot (the last point): they become 1."""
    find_bg, pos_bg, name = flags
    _, u, eps = rung
    rs = np.random.RandomState(1000 * nq + 10 * FLAGS.index(flags) + LADDER.index(rung) + 7 * seed)
    C = shape(nq)
    if eps is not None:
        C = 0.37 * (1.0 + eps * C)
    A0 = 2.3
    b0 = {"free": 0.02, "nobg": 0.0, "clamped": -0.004, "posb": 0.02}[name] * A0
    if eps is not None and name == "clamped":
        b0 = -0.2 * A0
    if rung[0] == "bg1000" and name in ("free", "posb"):
        b0 = 1000.0 * A0
    I0 = A0 * C + b0
    sigma = u * I0
    for _ in range(40):                                          # (1,1): noise under which the free b has the sign the case is named for
        I = I0 + sigma * rs.standard_normal(nq)
        if not pos_bg:
            break
        w = 1.0 / (sigma * sigma)
        bf = emu_solve_fit(w.sum(), (w * I).sum(), (w * I * I).sum(), (w * C).sum(), (w * C * C).sum(), (w * I * C).sum(), nq, True, False)[1]
        if (bf < 0) == (name == "clamped"):
            break
    if zeros:
        sigma = sigma.copy()
        for i in (0, 63, nq - 1):
            if i < nq:
                sigma[i] = 0.0
    if si_units:
        I, sigma, C = I * SI_I, sigma * SI_I, C * SI_C
    return dict(I=np.ascontiguousarray(I), sigma=np.ascontiguousarray(sigma), C=np.ascontiguousarray(C), find_bg=find_bg, pos_bg=pos_bg,
                name="nq%d-%s-%s-%s%s" % (nq, name, rung[0], "SI" if si_units else "one", "-zeros" if zeros else ""), kind=name)


def fit_cases(nq):
    """every flag set x every rung of both ladders at this q-count, order-one and SI units alternating so that each (flag set, rung)
    meets both across the q-counts; zero uncertainties on the first rung of each flag set, in both units"""
    out = []
    for fi, flags in enumerate(FLAGS):
        for ri, rung in enumerate(LADDER):
            out.append(fit_case(nq, flags, rung, si_units=(NQS.index(nq) + fi + ri) % 2 == 1))
        out.append(fit_case(nq, flags, LADDER[0], si_units=False, zeros=True))
        if nq >= 63:          # (in SI units a point of uncertainty 1 weighs 1e-60 of the others: below 63 q too few points would be left)
            out.append(fit_case(nq, flags, LADDER[0], si_units=True, zeros=True))
    return out


def single_point_cases():
    """nq = 1 without a background (with one the determinant is 0 and the reference refuses)"""
    return [fit_case(1, FLAGS[1], LADDER[0], si_units=s) for s in (False, True)]


def branch_is_defined(x, bounds):
    """the exact free b is further from 0 than the bound on the computed one: the positive-background branch is the exact fit's"""
    return x["b_free"] is None or abs(float(x["b_free"])) > bounds["b_free"].e

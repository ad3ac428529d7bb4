"""Shared by test_hist_exact_host.py and test_hist_exact_gpu.py: what McSAS.histogram() reads off a set of contributions (visibility
limits, fractions, bins, observability, cumulative distribution, moments: csrc/hist_kernels.h hist_obs_body, hist_fractions_body,
hist_bins_body), engine.observability (csrc/small_kernels.h observability_kernel; both limits are its visibility_limit) and the
re-binning of raw data (csrc/host_calls.hip rebin_kernel) as
  - the cases,
  - exact values (fractions.Fraction and mpmath, 60 digits) of the discrete operation at the doubles the kernel is given,
  - bounds derived from the kernels' operation order (tests/exact.py: R, V, gamma, reduced_sum), the line a count was read from next
    to it, and
  - numpy fp64 emulations of the same order, with the degradations test_hist_exact_host.py holds the bounds against.
A plain module like helpers.py: nothing in here is collected.  Nothing is fitted to a device's output.

What is not a number with a bound is compared by equality: which contribution is in which bin or mask, which product is zero, which
bins the re-binning keeps, and where NaN, +-inf and an exact 0 stand.  A value that IEEE arithmetic makes non-finite is a plain float
here (a "special"), everything else an exact.R; an operation with a special operand has an exact IEEE result, which is again special
or an exact 0 (x / inf), never a number that would need a bound (mul, div, add, sub below).  A decision of the kernel on a computed
value (`tn != 0.`, `(tot * sg) != 0.`, `scaled != 0.`) is defined where the exact value is 0 with a bound of 0, or further from 0 than
its bound; the cases are made so that every decision is defined, and Undefined is raised where one is not.

The scale A of a repetition is an input here: the caller takes it from the call's own output (hist_fit_cum_kernel is held by
test_fit_exact_gpu.py), or from fit_exact's emulation where there is no device.

Read off the source, where a summary of these kernels might say otherwise: hist_bins_body's membership is `x >= elo && x < ehi &&
x < last` (last = the last edge) — with ascending edges the third condition follows from the second, and the cases' edges ascend;
the reference takes a bin's observability as numpy's pairwise .mean(), the kernel as the ordered sum over the count, which the
bound here follows; `mq` is `mnc * m * m`, that is (mn mv) mv."""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

from exact import R, V, gamma, reduced_sum, slots_of, sum_roundings
from fit_exact import emu_bgfit, exactly, tree

WEIGHTS = ("vol", "num", "int", "surf")
FRAC8 = ("vf", "nf", "qf", "sf", "mv", "mn", "mq", "ms")          # frac8 = [vf nf qf sf | mv mn mq ms][N][R] (hist_kernels.h: hist_fractions_body)
C_EXP = 0.6666666


class Undefined(AssertionError):
    """a decision of the kernel whose exact counterpart lies within the bound of the value it is taken on"""


# ------------------------------------------------------------------------------------------------- R or special
def special(x):
    return isinstance(x, float)


def _fl(x):
    return x if special(x) else float(x.v)


def is_zero(x):
    """the kernel's `x == 0.` on the double it has computed, decided from the exact value and its bound (NaN, inf: not zero)"""
    if special(x):
        return x == 0.0
    if x.v == 0 and x.e == 0.0:
        return True
    if abs(float(x.v)) > x.e:
        return False
    raise Undefined("exact %s lies within its bound %.3g of zero" % (mp.nstr(x.v, 8), x.e))


def _ieee(op, a, b):
    """an operation with a non-finite operand, or a division by an exact zero: IEEE's own result, exact"""
    for x in (a, b):
        if not special(x):
            is_zero(x)                                            # (raises where the operand's sign or zero-ness is not the double's)
    with np.errstate(all="ignore"):
        r = float(op(np.float64(_fl(a)), np.float64(_fl(b))))
    assert r == 0.0 or not math.isfinite(r), (a, b, r)
    return R(0) if r == 0.0 else r


def mul(a, b):
    return _ieee(np.multiply, a, b) if special(a) or special(b) else a * b


def add(a, b):
    return _ieee(np.add, a, b) if special(a) or special(b) else a + b


def sub(a, b):
    return _ieee(np.subtract, a, b) if special(a) or special(b) else a - b


def div(a, b):
    return _ieee(np.divide, a, b) if special(a) or special(b) or is_zero(b) else a / b


def sqrt_abs(a):
    """sqrt(fabs(a))"""
    if special(a):
        return abs(a)                                             # (inf -> inf, nan -> nan)
    return R(abs(a.v), a.e).sqrt()


def seq(xs):
    """`t = 0.; for (...) t += x` over xs in order: the first addition, onto 0.0, is exact"""
    t = None
    for x in xs:
        t = x if t is None else add(t, x)
    return R(0) if t is None else t


@exactly
def min_within(exact_candidates, delta):
    """The minimum of computed values each within relative `delta` of its exact value is within `delta` of the exact minimum: if
    candidate j is the computed minimum and i the exact one, c^_j <= c^_i <= (1 + delta) c_i and c^_j >= (1 - delta) c_j >=
    (1 - delta) c_i.  (Positive candidates; the order in which fmin and wave_min take them does not matter.)"""
    m = min(exact_candidates)
    assert m > 0
    m = mp.mpf(m.numerator) / m.denominator
    return R(m, delta * float(m))


# ------------------------------------------------------------------------------------------------- exact values and bounds: histogram
LIMIT_ROUNDINGS = 5
# hist_obs_body: `vf = wset * A / vset` (two roundings), then visibility_limit (small_kernels.h) with intensity(k) = row[k]: per q
# `scaled = A * intensity(k)` (one), `(sigma[k] * vf) / scaled` (two): a quotient of products, five factors (1 + d) in all, within
# gamma(5) of sigma vf / (A row) = sigma w / (v row): A cancels.
OBS_ROUNDINGS = 3
# observability_kernel: vf is the caller's double, intensity(k) the model's row: `scaled = A * intensity(k)`, `(sigma[k] * vf) / scaled`: three


def scaled_classes(A, row):
    """`scaled = A * row[k]` as the kernel forms it, one IEEE product of two known doubles: which points `scaled != 0.` keeps"""
    with np.errstate(under="ignore"):
        return np.float64(A) * np.asarray(row, dtype=np.float64) != 0.0


def limit_bound(sigma, row, v, w, A):
    """hist_obs_body for one (c, r): min over the kept k of (sigma[k] vf) / (A row[k]), +inf where none is kept"""
    keep = scaled_classes(A, row)
    if not keep.any():
        return math.inf
    if v == 0.0 or not math.isfinite(w * A / v if v else math.inf):
        with np.errstate(all="ignore"):                           # vf is inf (or NaN): every candidate is, and fmin leaves +inf
            vf = np.float64(w) * np.float64(A) / np.float64(v)
            best = float(np.fmin.reduce((sigma[keep] * vf) / (np.float64(A) * row[keep]), initial=np.inf))
        assert not math.isfinite(best)
        return best
    wv = Fraction(float(w)) / Fraction(float(v))
    return min_within([Fraction(float(s)) * wv / Fraction(float(x)) for s, x in zip(sigma[keep], row[keep])], gamma(LIMIT_ROUNDINGS))


def obs_bound(sigma, row, vf, A):
    """observability_kernel for one (c, r): the same minimum with the caller's vf"""
    keep = scaled_classes(A, row)
    if not keep.any():
        return math.inf
    f = Fraction(float(vf)) / Fraction(float(A))
    return min_within([Fraction(float(s)) * f / Fraction(float(x)) for s, x in zip(sigma[keep], row[keep])], gamma(OBS_ROUNDINGS))


@exactly
def fractions_bounds(c, A):
    """hist_obs_body and hist_fractions_body -> {name: [N][R] of R or special}, the source's lines:
        vfc = w * A / v;  nfc = vfc / v;  mnc = m / v;  qf = vfc * v;  sf = nfc * s;  mq = mnc * m * m;  ms = mnc * s
        t += src[c R + r] over c in order, for nf, qf, sf;  where a total is not 0: nf /= tn, mn /= tn; qf /= tq, mq /= tq; ..."""
    N, nrep = c["N"], c["R"]
    out = {k: np.empty((N, nrep), dtype=object) for k in FRAC8}
    for r in range(nrep):
        Ar = R(float(A[r]))
        for i in range(N):
            v, w, s = R(c["v"][i, r]), R(c["w"][i, r]), R(c["s"][i, r])
            vf = div(mul(w, Ar), v)
            nf = div(vf, v)
            m = limit_bound(c["sigma"], c["rows"][r, i], c["v"][i, r], c["w"][i, r], float(A[r]))
            mn = div(m, v)
            vals = dict(vf=vf, nf=nf, qf=mul(vf, v), sf=mul(nf, s), mv=m, mn=mn, mq=mul(mul(mn, m), m), ms=mul(mn, s))
            for k in FRAC8:
                out[k][i, r] = vals[k]
        for f, m in (("nf", "mn"), ("qf", "mq"), ("sf", "ms")):
            t = seq(out[f][:, r])
            if not is_zero(t):
                for i in range(N):
                    out[f][i, r] = div(out[f][i, r], t)
                    out[m][i, r] = div(out[m][i, r], t)
    return out


def bin_members(x, edges):
    """[n_bin][N] masks: elo <= x < ehi (and x < the last edge), on the doubles themselves"""
    e = np.asarray(edges, dtype=np.float64)
    return [(x >= e[b]) & (x < e[b + 1]) & (x < e[-1]) for b in range(len(e) - 1)]


def moments_mask(x, lo, hi):
    return (x > lo) & (x < hi)


def is_pow2(x):
    return x > 0 and math.frexp(x)[0] == 0.5


@exactly
def histogram_bounds(c, fr, sp, r):
    """hist_bins_body for one (histogram, repetition) -> dict(bins, obs, cdf: lists over the bins; moments: five) of R or special,
    and counts (per bin), n_in (inside the moments mask).  Lines of the source:
        sb += lf[c]; so += ll[c]; cnt += 1. over the members in order;  bins = sb != sb ? 0 : sb;  obs = cnt > 0 ? so / cnt : 0
        run += bins[b]; cdf[b] = run; top = fmax(top, run);  cdf[b] = top == 0 ? 0 : cdf[b] / top
        tot += lf;  m1 += x * lf;  if (tot != 0) m1 /= tot;  d = x - m1;  v2 += (d * d) * lf;  var = v2 / tot;  sg = sqrt(fabs(var))
        ok3 = any && (tot * sg) != 0;  d2 = d * d;  acc += (d2 * d) * lf | (d2 * d2) * lf;  sg2 = sg * sg;
        val = ok3 ? acc / (tot * (sg2 * sg | sg2 * sg2)) : 0;  nobody inside: all five are 0."""
    wi = WEIGHTS.index(sp["yweight"])
    x = np.ascontiguousarray(c["contribs"][:, sp["param_index"], r])
    lf, ll = fr[FRAC8[wi]][:, r], fr[FRAC8[4 + wi]][:, r]
    bins, obs, counts = [], [], []
    for m in bin_members(x, sp["edges"]):
        idx = np.flatnonzero(m)
        sb = seq(lf[i] for i in idx)
        bins.append(R(0) if special(sb) and sb != sb else sb)
        obs.append(div(seq(ll[i] for i in idx), R(len(idx))) if len(idx) else R(0))
        counts.append(len(idx))
    run, runs = None, []
    for b in bins:
        assert special(b) or b.v >= 0                              # (fractions are not negative: the running sum does not fall, its
        run = b if run is None else add(run, b)                    # maximum is its last value)
        runs.append(run)
    top = runs[-1] if runs else R(0)
    cdf = [R(0) if is_zero(top) else div(q, top) for q in runs]
    idx = np.flatnonzero(moments_mask(x, sp["lower"], sp["upper"]))
    if not len(idx):
        mom = [R(0)] * 5
    else:
        xs = [R(float(x[i])) for i in idx]
        fs = [lf[i] for i in idx]
        tot = seq(fs)
        m1 = seq(mul(a, f) for a, f in zip(xs, fs))
        if not is_zero(tot):
            if len(idx) == 1 and not special(tot):
                # x f / f with x a power of two: product and quotient are exact, m1 is x bit for bit, d = 0 and var = 0; any other
                # x leaves m1 an ulp from x at times and skew = +-1: a case with one contribution inside places a power of two
                if not is_pow2(float(x[idx[0]])):
                    raise Undefined("one contribution inside the range, and its value is no power of two")
                m1 = xs[0]
            else:
                m1 = div(m1, tot)
        if len(idx) == 1 and not special(tot) and not is_zero(tot):
            d = [R(0)]
        else:
            d = [sub(a, m1) for a in xs]
        d2 = [mul(a, a) for a in d]
        var = div(seq(mul(a, f) for a, f in zip(d2, fs)), tot)
        sg = sqrt_abs(var)
        sg2 = mul(sg, sg)
        mom = [tot, m1, var]
        if is_zero(mul(tot, sg)):
            mom += [R(0), R(0)]
        else:
            a3 = seq(mul(mul(q, a), f) for q, a, f in zip(d2, d, fs))
            a4 = seq(mul(mul(q, q), f) for q, f in zip(d2, fs))
            mom += [div(a3, mul(tot, mul(sg2, sg))), div(a4, mul(tot, mul(sg2, sg2)))]
    return dict(bins=bins, obs=obs, cdf=cdf, moments=mom, counts=counts, n_in=len(idx))


def all_bounds(c, A):
    """-> (fractions, [histogram][repetition] of histogram_bounds)"""
    fr = fractions_bounds(c, A)
    return fr, [[histogram_bounds(c, fr, sp, r) for r in range(c["R"])] for sp in c["specs"]]


# ------------------------------------------------------------------------------------------------- comparing
def klass(x):
    """nan / +inf / -inf / 0 / number"""
    x = float(x)
    return "nan" if x != x else ("+inf" if x == math.inf else ("-inf" if x == -math.inf else ("0" if x == 0.0 else "number")))


@exactly
def look(bad, worst, case, name, got, ref):
    """got against ref: a special or an exact 0 by equality, a number by its bound; worst[name] = largest error / bound"""
    got = float(got)
    if special(ref) or (ref.v == 0 and ref.e == 0.0):
        want = klass(ref if special(ref) else 0.0)
        if klass(got) != want:
            bad.append("%s %s: got %r where %s stands" % (case, name, got, want))
        return
    if klass(got) not in ("number", "0"):
        bad.append("%s %s: got %r, exact %.17g" % (case, name, got, float(ref.v)))
        return
    err = float(abs(mp.mpf(got) - ref.v))
    r = 0.0 if err == 0.0 else (err / ref.e if ref.e > 0 else math.inf)
    worst[name] = max(worst.get(name, 0.0), r)
    if not r <= 1.0:
        bad.append("%s %s: got %.17g, exact %.17g, error %.3g of its bound %.3g" % (case, name, got, float(ref.v), r, ref.e))


def look_triple(bad, worst, c, got, bounds=None):
    """engine.histogram_device's triple (scaling, fractions, histograms) of case c against the bounds at the triple's own scale
    (or `bounds`, all_bounds' result at that scale, where it is at hand)"""
    sc, frd, hs = got
    fr, hb = bounds if bounds is not None else all_bounds(c, sc[0])
    for wi, wname in enumerate(WEIGHTS):
        for j, k in ((0, FRAC8[wi]), (1, FRAC8[4 + wi])):
            for i in range(c["N"]):
                for r in range(c["R"]):
                    look(bad, worst, c["name"], "%s [%d, %d]" % (k, i, r), frd[wname][j][i, r], fr[k][i, r])
    assert len(hs) == len(c["specs"])
    for h, sp in enumerate(c["specs"]):
        for r in range(c["R"]):
            ref = hb[h][r]
            for k in ("bins", "obs", "cdf", "moments"):
                assert hs[h][k].shape == (len(ref[k]), c["R"])
                for b, q in enumerate(ref[k]):
                    look(bad, worst, c["name"], "hist %d %s [%d, %d]" % (h, k, b, r), hs[h][k][b, r], q)
    return fr, hb


def summarise(worst):
    """{quantity: largest error / bound}, the indices folded away"""
    out = {}
    for k, v in worst.items():
        words = k.split(" [")[0].split()
        q = words[-1] if words[0] == "hist" else words[0]
        out[q] = max(out.get(q, 0.0), v)
    return out


# ------------------------------------------------------------------------------------------------- emulation, numpy fp64: histogram
def _seq(xs, dtype=np.float64):
    t = dtype(0.0)
    for x in xs:
        t = dtype(t + dtype(x))
    return np.float64(t)


def emu_histogram(c, A, mutate=None):
    """The kernels' order in doubles -> engine.histogram_device's triple.  mutate: "upper_le" (upper bin edge taken as <=),
    "moments_le" (moments mask not strict), "obs_N" (observability divided by N), "bin32" (a bin accumulated in float32),
    "q_drop" (the last q-point left out of the visibility minimum), "mq_short" (mq = mn mv)."""
    N, nrep = c["N"], c["R"]
    A = np.asarray(A, dtype=np.float64)
    f8 = {k: np.zeros((N, nrep)) for k in FRAC8}
    with np.errstate(all="ignore"):
        for r in range(nrep):
            v, w, s = c["v"][:, r], c["w"][:, r], c["s"][:, r]
            m = np.full(N, np.inf)
            vf = w * A[r] / v
            for i in range(N):
                row = c["rows"][r, i]
                scaled = A[r] * row
                keep = scaled != 0.0
                if mutate == "q_drop":
                    keep[-1] = False
                if keep.any():
                    m[i] = np.fmin.reduce((c["sigma"][keep] * vf[i]) / scaled[keep], initial=np.inf)
            nf, mn = vf / v, m / v
            f8["vf"][:, r], f8["nf"][:, r], f8["qf"][:, r], f8["sf"][:, r] = vf, nf, vf * v, nf * s
            f8["mv"][:, r], f8["mn"][:, r], f8["ms"][:, r] = m, mn, mn * s
            f8["mq"][:, r] = mn * m if mutate == "mq_short" else mn * m * m
            for f, l in (("nf", "mn"), ("qf", "mq"), ("sf", "ms")):
                t = _seq(f8[f][:, r])
                if t != 0.0:
                    f8[f][:, r] /= t; f8[l][:, r] /= t
        hists = []
        for sp in c["specs"]:
            wi = WEIGHTS.index(sp["yweight"])
            e = np.asarray(sp["edges"], dtype=np.float64)
            nb = len(e) - 1
            h = dict(bins=np.zeros((nb, nrep)), obs=np.zeros((nb, nrep)), cdf=np.zeros((nb, nrep)), moments=np.zeros((5, nrep)))
            for r in range(nrep):
                x = c["contribs"][:, sp["param_index"], r]
                lf, ll = f8[FRAC8[wi]][:, r], f8[FRAC8[4 + wi]][:, r]
                for b in range(nb):
                    hi = (x <= e[b + 1]) if mutate == "upper_le" else (x < e[b + 1])
                    idx = np.flatnonzero((x >= e[b]) & hi & (x < e[-1]))
                    sb = _seq(lf[idx], np.float32 if mutate == "bin32" else np.float64)
                    h["bins"][b, r] = 0.0 if sb != sb else sb
                    h["obs"][b, r] = _seq(ll[idx]) / (N if mutate == "obs_N" else len(idx)) if len(idx) else 0.0
                run, top = np.float64(0.0), -np.inf
                for b in range(nb):
                    run = run + h["bins"][b, r]; h["cdf"][b, r] = run; top = np.fmax(top, run)
                h["cdf"][:, r] = 0.0 if top == 0.0 else h["cdf"][:, r] / top
                ok = (x >= sp["lower"]) & (x <= sp["upper"]) if mutate == "moments_le" else (x > sp["lower"]) & (x < sp["upper"])
                idx = np.flatnonzero(ok)
                if len(idx):
                    xs, fs = x[idx], lf[idx]
                    tot, m1 = _seq(fs), _seq(xs * fs)
                    if tot != 0.0:
                        m1 = m1 / tot
                    d = xs - m1
                    var = _seq((d * d) * fs) / tot
                    sg = np.sqrt(np.abs(var))
                    sg2, d2 = sg * sg, d * d
                    ok3 = (tot * sg) != 0.0
                    sk = _seq((d2 * d) * fs) / (tot * (sg2 * sg)) if ok3 else 0.0
                    ku = _seq((d2 * d2) * fs) / (tot * (sg2 * sg2)) if ok3 else 0.0
                    h["moments"][:, r] = tot, m1, var, sk, ku
            hists.append(h)
    fractions = {wn: (f8[FRAC8[i]], f8[FRAC8[4 + i]]) for i, wn in enumerate(WEIGHTS)}
    return np.vstack([A, np.zeros(nrep)]), fractions, hists


def reference_lines(c, A):
    """What the reference's own lines give in numpy doubles under np.errstate, in its words and its order (mcsas.py:561-604: the
    fractions, their totals by the builtin sum(), the limits; utils/parameter.py:441-479: a bin by sum() over its mask, NaN to 0,
    the observability by .mean(), the running sum over its maximum; :84-122: the moments over the strict range) -> the triple.
    It says where NaN, +-inf and 0 stand when an input is 0; where it would raise (the .min() of no point at all) the value is the
    +inf hist_obs_body documents."""
    N, nrep = c["N"], c["R"]
    f8 = {k: np.zeros((N, nrep)) for k in FRAC8}
    hists = []
    with np.errstate(all="ignore"):
        for ri in range(nrep):
            vset, sset = c["v"][:, ri], c["s"][:, ri]
            vol = c["w"][:, ri] * A[ri] / vset
            num = vol / vset
            sqr = vol * vset
            surf = num * sset
            tot_num, tot_sqr, tot_surf = sum(num), sum(sqr), sum(surf)
            req = np.zeros((4, N))
            for ci in range(N):
                weighted = c["sigma"] * vol[ci]
                partial = A[ri] * c["rows"][ri, ci]
                ind = partial != 0.
                req[0, ci] = (weighted[ind] / partial[ind]).min() if ind.any() else np.inf
                req[1, ci] = req[0, ci] / vset[ci]
                req[2, ci] = req[1, ci] * req[0, ci] * req[0, ci]
                req[3, ci] = req[1, ci] * sset[ci]
            if 0 != tot_num:
                num = num / tot_num; req[1] /= tot_num
            if 0 != tot_sqr:
                sqr = sqr / tot_sqr; req[2] /= tot_sqr
            if 0 != tot_surf:
                surf = surf / tot_surf; req[3] /= tot_surf
            for k, a in zip(FRAC8, (vol, num, sqr, surf, req[0], req[1], req[2], req[3])):
                f8[k][:, ri] = a
        for sp in c["specs"]:
            wi = WEIGHTS.index(sp["yweight"])
            e = sp["edges"]
            nb = len(e) - 1
            h = dict(bins=np.zeros((nb, nrep)), obs=np.zeros((nb, nrep)), cdf=np.zeros((nb, nrep)), moments=np.zeros((5, nrep)))
            for ri in range(nrep):
                par = c["contribs"][:, sp["param_index"], ri]
                fraction, min_req = f8[FRAC8[wi]][:, ri], f8[FRAC8[4 + wi]][:, ri]
                for bi in range(nb):
                    mask = (par >= e[bi]) & (par < e[bi + 1])
                    val = sum(fraction[mask])
                    h["bins"][bi, ri] = 0. if np.isnan(val) else val
                    h["obs"][bi, ri] = min_req[mask].mean() if any(mask) else 0.
                cdf = np.zeros(nb)
                cdf[0] = h["bins"][0, ri]
                for i in range(1, nb):
                    cdf[i] = cdf[i - 1] + h["bins"][i, ri]
                h["cdf"][:, ri] = 0. if cdf.max() == 0.0 else cdf / cdf.max()
                valid = (par > sp["lower"]) & (par < sp["upper"])
                if not any(valid):
                    continue
                rset, frac = par[valid], fraction[valid]
                val = sum(frac)
                mu = sum(rset * frac)
                if 0 != sum(frac):
                    mu /= sum(frac)
                var = sum((rset - mu) ** 2 * frac) / sum(frac)
                sigma = np.sqrt(abs(var))
                skw = krt = 0.
                if not (sum(frac) * sigma) == 0.0:
                    skw = sum((rset - mu) ** 3 * frac) / (sum(frac) * sigma ** 3)
                    krt = sum((rset - mu) ** 4 * frac) / (sum(frac) * sigma ** 4)
                h["moments"][:, ri] = val, mu, var, skw, krt
            hists.append(h)
    return np.vstack([A, np.zeros(nrep)]), {wn: (f8[FRAC8[i]], f8[FRAC8[4 + i]]) for i, wn in enumerate(WEIGHTS)}, hists


def classes_differ(c, got, bounds, what):
    """-> where a triple and the exact reference disagree on nan / +inf / -inf / 0 / number"""
    sc, frd, hs = got
    fr, hb = bounds
    out = []
    for wi, wn in enumerate(WEIGHTS):
        for j, k in ((0, FRAC8[wi]), (1, FRAC8[4 + wi])):
            for i in range(c["N"]):
                for r in range(c["R"]):
                    if klass(frd[wn][j][i, r]) != klass(_fl(fr[k][i, r])):
                        out.append("%s %s %s [%d, %d]: %r, exact %s" % (c["name"], what, k, i, r, frd[wn][j][i, r], klass(_fl(fr[k][i, r]))))
    for h in range(len(c["specs"])):
        for r in range(c["R"]):
            for k in ("bins", "obs", "cdf", "moments"):
                for b, q in enumerate(hb[h][r][k]):
                    if klass(hs[h][k][b, r]) != klass(_fl(q)):
                        out.append("%s %s hist %d %s [%d, %d]: %r, exact %s" % (c["name"], what, h, k, b, r, hs[h][k][b, r], klass(_fl(q))))
    return out


def emu_scaling(c):
    """a scale per repetition where there is no device: the fit's emulation (fit_exact.emu_bgfit) against the ordered column sum"""
    A = np.zeros(c["R"])
    for r in range(c["R"]):
        cum = np.zeros(c["nq"])
        for i in range(c["N"]):
            cum = cum + c["rows"][r, i]
        A[r] = emu_bgfit(c["I"], c["sigma"], cum, c["find_bg"], False)[0]
    return A


# ------------------------------------------------------------------------------------------------- the histogram cases
PAR_LO, PAR_HI = np.array([2e-9, 5e-10]), np.array([1e-7, 2e-8])
A0 = 1e-3
TINY = 5e-324                       # the smallest subnormal: times a scale below 1/2 it rounds to exactly 0


def edges_of(lo, hi, nb, xscale):
    return np.linspace(lo, hi, nb + 1) if xscale == "lin" else np.geomspace(lo, hi, nb + 1)


def spec(pi, yweight, nb, xscale, lo=None, hi=None):
    lo = float(PAR_LO[pi] if lo is None else lo); hi = float(PAR_HI[pi] if hi is None else hi)
    return dict(param_index=pi, yweight=yweight, edges=edges_of(lo, hi, nb, xscale), lower=lo, upper=hi)


def fake_rows(q, pset):
    """plausible positive doubles for the rows, volumes, weights and surfaces of a sphere-like model: the arithmetic after the rows is
    a function of these doubles whatever made them (on the device the built-in cases take model_calc's instead)"""
    r = pset[:, 0] + (pset[:, 1] if pset.shape[1] > 1 else 0.0)
    v = 4.1887902 * r ** 3
    w = v ** -C_EXP
    s = 12.566371 * r * r
    x = q[None, :] * r[:, None]
    rows = (w * v * v)[:, None] * (1.0 / (1.0 + x * x / 5.0) ** 2 + 1e-4 * (1.0 + np.cos(x)))
    return rows, v, w, s


def finish(c, rows_fn):
    """rows [R][N][nq], v, w, s [N][R] of the case's contributions from rows_fn(pset[N][P]) -> (rows, v, w, s), then the case's own
    changes to them, then data a thousandth of repetition 0's summed rows (so that the scale is near 1e-3) on a small background"""
    N, nrep, nq = c["N"], c["R"], c["nq"]
    c["rows"] = np.zeros((nrep, N, nq))
    for k in "vws":
        c[k] = np.zeros((N, nrep))
    for r in range(nrep):
        rows, v, w, s = rows_fn(np.ascontiguousarray(c["contribs"][:, :, r]))
        c["rows"][r], c["v"][:, r], c["w"][:, r], c["s"][:, r] = rows, v, w, s
    if "edit" in c:
        c["edit"](c)
    cum = c["rows"][0].sum(axis=0)
    k = np.arange(nq)
    c["I"] = A0 * cum * (1.0 + 0.01 * np.cos(1.7 * k)) + (0.02 * A0 * cum.mean() if c["find_bg"] else 0.0)
    c["sigma"] = 0.02 * c["I"] * (1.0 + 0.5 * np.sin(0.9 * k) ** 2)
    return c


def _case(name, N, nrep, nq, specs, seed, P=2, builtin=None, edit=None, place=None):
    rs = np.random.RandomState(seed)
    contribs = rs.uniform(PAR_LO[None, :P, None], PAR_HI[None, :P, None], (N, P, nrep))
    c = dict(name=name, N=N, P=P, R=nrep, nq=nq, q=np.geomspace(1e8, 3e9, nq) if nq > 1 else np.array([3e8]), specs=specs,
             contribs=contribs, find_bg=nq > 1, builtin=builtin, claims={})
    if place:
        place(c)
    if edit:
        c["edit"] = edit
    return c


NARROW = (2.0 ** -27, 2.0 ** -25)         # 7.45e-9 .. 2.98e-8 in param 0; 2^-26 lies inside


def _place_edges(c):
    """repetition 0: contributions on the first, an inner and the last edge of histogram 0 (the first and last are its lower and
    upper too), and on the lower and upper of the narrow histogram 2; repetition 1: nobody inside the narrow range; repetition 2:
    exactly one, 2^-26"""
    e = c["specs"][0]["edges"]
    x = c["contribs"][:, 0, :]
    x[0, 0], x[1, 0], x[2, 0] = e[0], e[3], e[-1]
    x[3, 0], x[4, 0] = NARROW
    x[:, 1] = np.where((x[:, 1] >= NARROW[0]) & (x[:, 1] <= NARROW[1]), x[:, 1] + NARROW[1], x[:, 1])
    x[:, 2] = np.where((x[:, 2] >= NARROW[0]) & (x[:, 2] <= NARROW[1]), x[:, 2] + NARROW[1], x[:, 2])
    x[5, 2] = 2.0 ** -26
    c["claims"] = dict(first_edge=(0, 0, 0, 0), inner_edge=(0, 1, 0, 3), last_edge=(0, 2, 0), lower=(2, 3, 0), upper=(2, 4, 0),
                       nobody=(2, 1), one=(2, 2, 5), empty_bin=(1, 0))


def _place_one(c):
    """a single contribution is the one inside every range: powers of two (histogram_bounds)"""
    c["contribs"][0, :, 0] = 2.0 ** -26, 2.0 ** -28


def _edit_zero_surface(c):
    c["s"][:] = 0.0
    c["claims"]["zero_total"] = "surf"


def _edit_zero_volume(c):
    c["v"][2, 1] = 0.0
    c["claims"]["zero_volume"] = (2, 1)


def _edit_rows(c):
    """contribution 0: every point exactly 0; 1: every point the smallest subnormal, whose product with the scale underflows to
    exactly 0; 2: exact zeros at the even points; 3: subnormals at the first 32 points; the others as they are"""
    rows = c["rows"]
    rows[:, 0, :] = 0.0
    rows[:, 1, :] = TINY
    rows[:, 2, 0::2] = 0.0
    rows[:, 3, :32] = TINY
    c["claims"]["row_classes"] = {0: "zero", 1: "underflow", 2: "zero at even points", 3: "underflow at the first 32"}


def _edit_last_q(c):
    """the smallest contribution of repetition 0 made a million times stronger at the last q-point: that point gives its visibility
    minimum"""
    i = int(np.argmin(c["v"][:, 0]))
    c["rows"][:, i, -1] *= 1e6
    c["claims"]["min_at_last_q"] = i


def hist_cases():
    """Explicit rows (two active parameters; driven through engine.histogram_device_rows with a row_fn that hands these arrays over)
    and built-in ones (the sphere's and the core-shell sphere's own rows: every entry point).  N in {1, 7, 63, 64, 65, 129, 2731},
    bins in {1, 63, 64, 65, 130}, R in {1, 3}, q in {1, 63, 64, 65, 130}; N = 63, 64, 65 each with 63, 64 and 65 bins."""
    three = lambda: [spec(0, "vol", 63, "lin"), spec(0, "num", 64, "log"), spec(1, "int", 65, "lin"), spec(1, "surf", 8, "log")]
    out = [
        _case("one", 1, 1, 1, [spec(0, "vol", 1, "lin"), spec(1, "num", 1, "log")], 1, place=_place_one),
        _case("placed", 7, 3, 63, [spec(0, "vol", 8, "lin"), spec(0, "num", 130, "log"), spec(0, "int", 8, "lin", *NARROW),
                                   spec(1, "surf", 1, "log"), spec(1, "vol", 8, "lin", 4e-9, 1.2e-8), spec(0, "surf", 63, "lin")],
              2, place=_place_edges),
        _case("zero_surface", 7, 1, 1, [spec(0, "surf", 8, "lin"), spec(1, "vol", 8, "log")], 3, edit=_edit_zero_surface),
        _case("zero_volume", 7, 3, 63, [spec(0, w, 8, "lin") for w in WEIGHTS] + [spec(1, "num", 8, "log")], 4, edit=_edit_zero_volume),
        _case("row_classes", 7, 1, 64, [spec(0, "vol", 8, "lin"), spec(1, "num", 8, "log")], 5, edit=_edit_rows),
        _case("n63", 63, 1, 64, three(), 6),
        _case("n64", 64, 3, 65, three(), 7, edit=_edit_last_q),
        _case("n65", 65, 1, 130, three() + [spec(0, "int", 130, "log")], 8),
        _case("n129", 129, 3, 1, [spec(0, "num", 1, "lin"), spec(1, "vol", 130, "lin")], 9),
        _case("n2731", 2731, 1, 1, [spec(0, "vol", 8, "lin")], 10),           # 3 N doubles of LDS: 65544 bytes, the first above 64 KB
    ]
    return out + builtin_cases()


def builtin_cases():
    return [
        _case("sphere_7", 7, 3, 63, [spec(0, "vol", 8, "log"), spec(0, "num", 65, "lin")], 11, P=1, builtin="sphere"),
        _case("sphere_65", 65, 1, 130, [spec(0, "int", 64, "lin"), spec(0, "surf", 1, "lin"), spec(0, "vol", 130, "log", 1e-8, 5e-8)],
              12, P=1, builtin="sphere"),
        _case("coreshell_64", 64, 3, 65, [spec(0, "vol", 63, "lin"), spec(1, "num", 8, "log"), spec(1, "surf", 8, "lin")], 13,
              builtin="sphcs"),
    ]


def host_case(c):
    """the case with rows no device made (built-in cases too: their device rows are model_calc's)"""
    return finish(c, lambda pset: fake_rows(c["q"], pset))


# ------------------------------------------------------------------------------------------------- re-binning
def rebin_edges(x, n_bin):
    """engine.rebin's own expression"""
    return np.logspace(np.log10(x.min()), np.log10(x.max() + np.diff(x)[-1] / 100.), n_bin + 1)


def rebin_members(x, edges):
    return [np.flatnonzero((x >= edges[b]) & (x < edges[b + 1])) for b in range(len(edges) - 1)]


@exactly
def rebin_bounds(x, f, fu, n_bin):
    """rebin_kernel and the host loop behind it -> the kept bins in order, each dict(bin, count, x, f, fu) of R or special.
    One point: its three doubles (R with a bound of 0).  More: point i is in lane i & 63, a lane adds its members in order
    (`sx += xi; sf += f[i]; su2 += fu[i] * fu[i]`: at most slots - 1 rounded additions, the product rounded), wave_sum adds the lanes
    in six levels: exact.sum_roundings(slots); `xb = sx / cnt; mf = sf / cnt`; second pass `dlt = f[i] - mf; ss += dlt * dlt` through
    the same path; `sem = sqrt(ss / (cnt - 1.)) / sqrt(cnt), prop = sqrt(su2 / cnt)`; ub = fmax(sem, prop), NaN if either is: the
    maximum of two values within their bounds is within the larger bound of the exact maximum.  A bin whose mean is NaN is dropped."""
    edges = rebin_edges(x, n_bin)
    k = sum_roundings(slots_of(len(x)))
    out = []
    for b, idx in enumerate(rebin_members(x, edges)):
        cnt = len(idx)
        if cnt == 0 or np.isnan(f[idx]).any():
            continue
        if cnt == 1:
            i = idx[0]
            out.append(dict(bin=b, count=1, x=R(float(x[i])), f=R(float(f[i])), fu=float(fu[i]) if fu[i] != fu[i] else R(float(fu[i]))))
            continue
        xs, fs, us = ([mp.mpf(float(a)) for a in arr[idx]] for arr in (x, f, fu))
        sx = reduced_sum(mp.fsum(xs), V(x[idx]), k)
        sf = reduced_sum(mp.fsum(fs), V(f[idx]), k)
        mf = sf / R(cnt)
        d = [R(a) - mf for a in fs]
        t = [a * a for a in d]
        ss = reduced_sum(mp.fsum(a.v for a in t), V([float(a.v) for a in t], [a.e for a in t]), k)
        sem = (ss / R(cnt - 1)).sqrt() / R(cnt).sqrt()
        ub, wins = math.nan, "nan"
        if not np.isnan(fu[idx]).any():
            su2 = reduced_sum(mp.fsum(a * a for a in us), V(fu[idx]) * V(fu[idx]), k)
            prop = (su2 / R(cnt)).sqrt()
            ub = R(max(sem.v, prop.v), max(sem.e, prop.e))
            wins = "scatter" if sem.v - sem.e > prop.v + prop.e else ("propagated" if prop.v - prop.e > sem.v + sem.e else "close")
        out.append(dict(bin=b, count=cnt, x=sx / R(cnt), f=mf, fu=ub, wins=wins))
    return out


def emu_rebin(x, f, fu, n_bin, mutate=None):
    """rebin_kernel in numpy doubles, lane by lane -> (x, f, fu) of the kept bins.  mutate: "drop" (lane 0's last slot left out),
    "ddof0" (standard error with the count in place of the count less one)."""
    n = len(x)
    edges = rebin_edges(x, n_bin)
    live = np.ones(n, dtype=bool)
    if mutate == "drop":
        live[64 * (slots_of(n) - 1)] = False
    xo, fo, uo = [], [], []

    def lanes(terms, idx):
        acc = np.zeros(64)
        for t, i in zip(terms, idx):
            acc[i & 63] = acc[i & 63] + t
        return float(tree(acc))
    with np.errstate(all="ignore"):
        for b in range(n_bin):
            idx = np.flatnonzero((x >= edges[b]) & (x < edges[b + 1]) & live)
            cnt = float(len(idx))
            if cnt == 0:
                continue
            if cnt == 1:
                xb, fb, ub = x[idx[0]], f[idx[0]], fu[idx[0]]
            else:
                sx, sf, su2 = lanes(x[idx], idx), lanes(f[idx], idx), lanes(fu[idx] * fu[idx], idx)
                xb, fb = sx / cnt, sf / cnt
                dl = f[idx] - fb
                ss = lanes(dl * dl, idx)
                sem = np.sqrt(ss / (cnt if mutate == "ddof0" else cnt - 1.)) / np.sqrt(cnt)
                prop = np.sqrt(su2 / cnt)
                ub = np.nan if (sem != sem or prop != prop) else max(sem, prop)
            if fb == fb:
                xo.append(xb); fo.append(fb); uo.append(ub)
    return np.array(xo), np.array(fo), np.array(uo)


def look_rebin(bad, worst, name, got, ref):
    """engine.rebin's (x, f, fu) against rebin_bounds: the number of bins, then every kept bin"""
    xb, fb, ub = got
    if not (len(xb) == len(fb) == len(ub) == len(ref)):
        bad.append("%s: %d bins kept, %d expected (bins %s)" % (name, len(xb), len(ref), [q["bin"] for q in ref]))
        return
    for j, q in enumerate(ref):
        for k, g in (("x", xb[j]), ("f", fb[j]), ("fu", ub[j])):
            look(bad, worst, name, "%s [bin %d, %d points]" % (k, q["bin"], q["count"]), g, q[k])


def rebin_cases():
    """n in {2, 63, 64, 65, 200}: x ascending over a decade and a half with a cluster of 70 points in one bin at n = 200, f a smooth
    fall with a relative scatter of 1e-3 against uncertainties of 1e-2 f (the propagated uncertainty wins) or of 1e-6 f (the scatter
    wins), a run of equal f, a point moved onto an inner edge, NaN in f and in fu.  -> dicts(name, x, f, fu, n_bin, claims)"""
    out = []
    for n, n_bin in ((2, 3), (63, 40), (64, 100), (65, 20), (65, 7), (200, 12)):
        rs = np.random.RandomState(100 + n + n_bin)
        x = np.geomspace(1e8, 3e9, n)
        if n == 200:
            x[60:130] = np.linspace(x[60], x[60] * 1.02, 70)                # more than 64 points in one bin
        f = 1e3 / (1.0 + (x / 5e8) ** 2) * (1.0 + 1e-3 * rs.standard_normal(n))
        fu = (1e-2 if n_bin % 2 == 0 else 1e-6) * f
        claims = {}
        if n >= 63:
            e = rebin_edges(x, n_bin)
            for j in range(n // 2, n - 2):                                   # the first point from the middle on with an edge between it
                b = int(np.searchsorted(e, x[j], side="right"))              # and the next point is moved onto that edge
                if b < n_bin and e[b] < x[j + 1]:
                    x[j] = e[b]
                    claims["on_edge"] = (j, b)
                    break
            assert np.array_equal(rebin_edges(x, n_bin), e)
        if n == 200:
            e = rebin_edges(x, n_bin)
            f[(x >= e[np.searchsorted(e, x[60], side="right") - 1]) & (x < e[np.searchsorted(e, x[60], side="right")])] = f[60]   # a bin of equal f
            fu[140] = np.nan; f[170] = np.nan
            claims.update(equal=60, nan_fu=140, nan_f=170)
        if n == 65 and n_bin == 20:
            fu[10] = np.nan; f[40] = np.nan
            claims.update(nan_fu=10, nan_f=40)
        out.append(dict(name="n%d-%dbins" % (n, n_bin), x=x, f=f, fu=fu, n_bin=n_bin, claims=claims))
    return out

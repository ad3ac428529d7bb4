"""Shared by test_hist2d_host.py and test_hist2d_gpu.py: the joint histogram of two parameters (csrc/hist2d_kernel.h hist2d_body,
include/mcsas_hip.h mcsas_hip_histogram2d; parameter.Histogram2D.calc is its numpy form) as
  - the cases: contributions, fractions and limits of the test's own choosing, no model behind them,
  - exact values (mpmath, 60 digits) of the discrete operation at those doubles,
  - bounds derived from the kernel's operation order with exact.R through hist_exact's seq / mul / div / sub / sqrt_abs, and
  - a numpy fp64 emulation of the same order with the degradations test_hist2d_host.py holds the bounds against.
A plain module like helpers.py: nothing in here is collected.  Nothing is fitted to a device's output.

The roundings, read off hist2d_body:
    sb[k] += lf[c]; so[k] += ll[c]; cnt[k] += 1   over a cell's members in contribution order, onto 0.: m members, m - 1 roundings
    bins = sb != sb ? 0 : sb;  obs = cnt > 0 ? so / cnt : 0                                          one more for obs
    acc += ok ? f | x * f | y * f : 0.            tot, then mx and my, each `/= tot` unless tot == 0
    dx = x - mx; dy = y - my;  acc += ok ? (dx * dx | dy * dy | dx * dy) * f : 0.;  acc / tot        vxx, vyy, cxy
    den = sqrt(fabs(vxx)) * sqrt(fabs(vyy));  rho = den != 0 ? cxy / den : 0;  nobody inside: all seven are 0
so a moment's bound is the running error of dx, dy carried through the products, the ordered sum and the quotients (exact.R).
Which contribution is in which cell or mask, an empty cell's 0, the NaN -> 0 of a cell, the 0 of an empty selection and where NaN
and inf stand are compared by equality (hist_exact.look).  A decision on a computed value (`tot != 0.`, `den != 0.`) must be defined:
hist_exact.is_zero raises Undefined where the exact value lies within its bound of zero, and the cases are made so that none does."""
import math

import numpy as np

import hist_exact as H
from exact import R
from fit_exact import exactly
from mcsas_amd.parameter import FitParameter, Histogram2D

WEIGHTS = H.WEIGHTS
MOMENTS = ("total", "meanX", "meanY", "varianceX", "varianceY", "covariance", "correlation")
WAVE = 64


def _val(x):
    """a double of the case as hist_exact takes it: exact.R, or the float itself where it is not finite"""
    x = float(x)
    return R(x) if math.isfinite(x) else x


def columns(edges, x):
    """#{k : e[k] <= x} - 1 per value, on the doubles themselves (a NaN: no comparison holds, -1)"""
    e = np.asarray(edges, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (e[None, :] <= np.asarray(x, dtype=np.float64)[:, None]).sum(axis=1) - 1


def cells_of(sp, x, y):
    """flat cell i ny + j per contribution, -1 for a non-member"""
    nx, ny = len(sp["edges_x"]) - 1, len(sp["edges_y"]) - 1
    i, j = columns(sp["edges_x"], x), columns(sp["edges_y"], y)
    return np.where((i >= 0) & (i < nx) & (j >= 0) & (j < ny), i * ny + j, -1)


def moments_mask(sp, x, y):
    with np.errstate(invalid="ignore"):
        return (x > sp["lower_x"]) & (x < sp["upper_x"]) & (y > sp["lower_y"]) & (y < sp["upper_y"])


# ------------------------------------------------------------------------------------------------- exact values and bounds
@exactly
def bounds(c, sp, r):
    """hist2d_body for one (histogram, repetition) -> dict(bins, obs: [nx ny] lists, moments: seven) of R or special, counts per cell
    and n_in, the contributions inside the moments' mask"""
    wi = WEIGHTS.index(sp["yweight"])
    x, y = c["contribs"][:, sp["param_x"], r], c["contribs"][:, sp["param_y"], r]
    f, lim = c["frac8"][wi][:, r], c["frac8"][4 + wi][:, r]
    nx, ny = len(sp["edges_x"]) - 1, len(sp["edges_y"]) - 1
    cell = cells_of(sp, x, y)
    bins, obs, counts = [], [], []
    for k in range(nx * ny):
        idx = np.flatnonzero(cell == k)
        sb = H.seq(_val(f[i]) for i in idx)
        bins.append(R(0) if H.special(sb) and sb != sb else sb)
        obs.append(H.div(H.seq(_val(lim[i]) for i in idx), R(len(idx))) if len(idx) else R(0))
        counts.append(len(idx))
    idx = np.flatnonzero(moments_mask(sp, x, y))
    if not len(idx):
        mom = [R(0)] * 7
    else:
        xs, ys, fs = [_val(x[i]) for i in idx], [_val(y[i]) for i in idx], [_val(f[i]) for i in idx]
        tot = H.seq(fs)
        one = len(idx) == 1 and not H.special(tot) and not H.is_zero(tot)
        if one:
            # x f / f with x a power of two: product and quotient are exact, the mean is x bit for bit and the deviation 0 (as in
            # hist_exact.histogram_bounds): a case with one contribution inside places powers of two
            if not (H.is_pow2(float(x[idx[0]])) and H.is_pow2(float(y[idx[0]]))):
                raise H.Undefined("one contribution inside the ranges, and its values are no powers of two")
            mx, my, dx, dy = xs[0], ys[0], [R(0)], [R(0)]
        else:
            mx, my = H.seq(H.mul(a, w) for a, w in zip(xs, fs)), H.seq(H.mul(a, w) for a, w in zip(ys, fs))
            if not H.is_zero(tot):
                mx, my = H.div(mx, tot), H.div(my, tot)
            dx, dy = [H.sub(a, mx) for a in xs], [H.sub(a, my) for a in ys]
        vxx = H.div(H.seq(H.mul(H.mul(a, a), w) for a, w in zip(dx, fs)), tot)
        vyy = H.div(H.seq(H.mul(H.mul(a, a), w) for a, w in zip(dy, fs)), tot)
        cxy = H.div(H.seq(H.mul(H.mul(a, b), w) for a, b, w in zip(dx, dy, fs)), tot)
        den = H.mul(H.sqrt_abs(vxx), H.sqrt_abs(vyy))
        rho = R(0) if H.is_zero(den) else H.div(cxy, den)
        mom = [tot, mx, my, vxx, vyy, cxy, rho]
    return dict(bins=bins, obs=obs, moments=mom, counts=counts, n_in=len(idx))


def all_bounds(c):
    """[histogram][repetition] of bounds(), worked out once per case and kept with it"""
    if "bounds" not in c:
        c["bounds"] = [[bounds(c, sp, r) for r in range(c["R"])] for sp in c["specs"]]
    return c["bounds"]


def look_hists(bad, worst, c, hists, what=("bins", "obs", "moments")):
    """engine.histogram2d_device's list (or emu's) of case c against its bounds: numbers inside them, classes by equality"""
    ref = all_bounds(c)
    assert len(hists) == len(c["specs"])
    for h, sp in enumerate(c["specs"]):
        nx, ny = len(sp["edges_x"]) - 1, len(sp["edges_y"]) - 1
        for k, shape in (("bins", (nx, ny, c["R"])), ("obs", (nx, ny, c["R"])), ("moments", (7, c["R"]))):
            assert hists[h][k].shape == shape, (c["name"], h, k, hists[h][k].shape, shape)
        for r in range(c["R"]):
            for k in what:
                got = hists[h][k][..., r].reshape(-1)
                for b, q in enumerate(ref[h][r][k]):
                    H.look(bad, worst, c["name"], "hist %d %s [%d, %d]" % (h, k, b, r), got[b], q)
    return ref


# ------------------------------------------------------------------------------------------------- emulation, numpy fp64
MUTATIONS = ("upper_le_y", "edges_swapped", "obs_N", "cell32", "share_dropped", "moments_le", "cov_dxdx")


def emu(c, mutate=None):
    """hist2d_body's order in doubles -> engine.histogram2d_device's list.  mutate: "upper_le_y" (the upper edge of a y column taken
    as <=), "edges_swapped" (x looked up in the y edges and y in the x edges), "obs_N" (the limits' sum over N instead of the count),
    "cell32" (a cell summed in float32), "share_dropped" (the last contribution of lane 0's share, c = 64 (N - 1) // 64, never
    staged), "moments_le" (the moments' mask not strict), "cov_dxdx" (the covariance from dx dx)."""
    N, nrep = c["N"], c["R"]
    out = []
    with np.errstate(all="ignore"):
        for sp in c["specs"]:
            wi = WEIGHTS.index(sp["yweight"])
            ex, ey = np.asarray(sp["edges_x"], dtype=np.float64), np.asarray(sp["edges_y"], dtype=np.float64)
            nx, ny = len(ex) - 1, len(ey) - 1
            h = dict(bins=np.zeros((nx, ny, nrep)), obs=np.zeros((nx, ny, nrep)), moments=np.zeros((7, nrep)))
            for r in range(nrep):
                x, y = c["contribs"][:, sp["param_x"], r], c["contribs"][:, sp["param_y"], r]
                f, lim = c["frac8"][wi][:, r], c["frac8"][4 + wi][:, r]
                if mutate == "edges_swapped":
                    i, j = columns(ey, x), columns(ex, y)
                else:
                    i, j = columns(ex, x), columns(ey, y)
                if mutate == "upper_le_y" and ny:
                    # column j holds ey[j] <= y <= ey[j + 1]: a value on an inner or the last edge stays in the column below it
                    j = np.where((j >= 1) & (j <= ny) & (y == ey[np.clip(j, 0, ny)]), j - 1, j)
                cell = np.where((i >= 0) & (i < nx) & (j >= 0) & (j < ny), i * ny + j, -1)
                if mutate == "share_dropped":
                    cell[WAVE * ((N - 1) // WAVE)] = -1
                for k in range(nx * ny):
                    idx = np.flatnonzero(cell == k)
                    sb = H._seq(f[idx], np.float32 if mutate == "cell32" else np.float64)
                    h["bins"][k // ny, k % ny, r] = 0.0 if sb != sb else sb
                    h["obs"][k // ny, k % ny, r] = H._seq(lim[idx]) / (N if mutate == "obs_N" else len(idx)) if len(idx) else 0.0
                if mutate == "moments_le":
                    ok = (x >= sp["lower_x"]) & (x <= sp["upper_x"]) & (y >= sp["lower_y"]) & (y <= sp["upper_y"])
                else:
                    ok = moments_mask(sp, x, y)
                idx = np.flatnonzero(ok)
                if len(idx):
                    xs, ys, fs = x[idx], y[idx], f[idx]
                    tot, mx, my = H._seq(fs), H._seq(xs * fs), H._seq(ys * fs)
                    if tot != 0.0:
                        mx, my = mx / tot, my / tot
                    dx, dy = xs - mx, ys - my
                    vxx, vyy = H._seq((dx * dx) * fs) / tot, H._seq((dy * dy) * fs) / tot
                    cxy = H._seq(((dx * dx) if mutate == "cov_dxdx" else (dx * dy)) * fs) / tot
                    den = np.sqrt(np.abs(vxx)) * np.sqrt(np.abs(vyy))
                    h["moments"][:, r] = tot, mx, my, vxx, vyy, cxy, (cxy / den if den != 0.0 else 0.0)
            out.append(h)
    return out


# ------------------------------------------------------------------------------------------------- Histogram2D.calc on a case's edges
class GivenEdges(Histogram2D):
    """Histogram2D with the edges of a case's record in place of linspace / logspace of its ranges (a pair of equal neighbouring
    edges, ranges narrower than the edges): calc's method is what the tests hold, whatever formed the edges"""

    def __init__(self, sp):
        wide = [FitParameter(n, 1.0, valueRange=(-1e300, 1e300)) for n in ("x", "y")]
        super().__init__(wide[0], wide[1], (sp["lower_x"], sp["upper_x"]), (sp["lower_y"], sp["upper_y"]),
                         binCount=(len(sp["edges_x"]) - 1, len(sp["edges_y"]) - 1), yweight=sp["yweight"], autoFollow=False)
        self._given = (np.asarray(sp["edges_x"], dtype=np.float64), np.asarray(sp["edges_y"], dtype=np.float64))

    def _setEdges(self):
        self.xLowerEdge, self.yLowerEdge = self._given


def fractions_dict(frac8):
    return {w: (frac8[i], frac8[4 + i]) for i, w in enumerate(WEIGHTS)}


def calc_hists(c):
    """Histogram2D.calc of every histogram of the case -> engine.histogram2d_device's list"""
    fr = fractions_dict(c["frac8"])
    out = []
    for sp in c["specs"]:
        h = GivenEdges(sp)
        h.calc(c["contribs"], sp["param_x"], sp["param_y"], fr)
        out.append(dict(bins=h.bins.full, obs=h.obs, moments=h.moments.full))
    return out


# ------------------------------------------------------------------------------------------------- the cases
X_LO, X_HI = 2e-9, 1e-7                   # the range of the x column's values and of most x edges
Y_LO, Y_HI = 5e-10, 2e-8


def edges_of(lo, hi, n, scale):
    return np.linspace(lo, hi, n + 1) if scale == "lin" else np.geomspace(lo, hi, n + 1)


def spec(px, py, yweight, nx, ny, scale_x="lin", scale_y="log", ex=None, ey=None, rx=None, ry=None):
    """a histogram's record; the moments' ranges are the edges' ends unless rx / ry give others"""
    ex = edges_of(X_LO, X_HI, nx, scale_x) if ex is None else np.asarray(ex, dtype=np.float64)
    ey = edges_of(Y_LO, Y_HI, ny, scale_y) if ey is None else np.asarray(ey, dtype=np.float64)
    rx = (float(ex[0]), float(ex[-1])) if rx is None else rx
    ry = (float(ey[0]), float(ey[-1])) if ry is None else ry
    return dict(param_x=px, param_y=py, yweight=yweight, edges_x=ex, edges_y=ey, lower_x=rx[0], upper_x=rx[1], lower_y=ry[0], upper_y=ry[1])


def _case(name, N, nrep, P, px, py, specs, seed, place=None):
    """contributions uniform inside (X_LO, X_HI) in column px and (Y_LO, Y_HI) in column py (any third column: its own numbers, read
    by nobody), fractions and limits positive doubles of no model; then the case's placements"""
    rs = np.random.RandomState(seed)
    contribs = rs.uniform(1.0, 2.0, (N, P, nrep))
    contribs[:, px, :] = rs.uniform(X_LO, X_HI, (N, nrep))
    contribs[:, py, :] = rs.uniform(Y_LO, Y_HI, (N, nrep))
    frac8 = np.concatenate([rs.uniform(0.01, 1.0, (4, N, nrep)) / N, rs.uniform(1e-4, 1e-2, (4, N, nrep))])
    c = dict(name=name, N=N, R=nrep, P=P, px=px, py=py, specs=specs, contribs=contribs, frac8=frac8, claims={})
    if place:
        place(c)
    return c


def _place_one(c):
    """the one contribution: powers of two inside every range (bounds())"""
    c["contribs"][0, c["px"], 0], c["contribs"][0, c["py"], 0] = 2.0 ** -26, 2.0 ** -28


RANGE_X, RANGE_Y = (1.25e-8, 7.5e-8), (1.5e-9, 1.25e-8)       # the narrower moments' ranges of "placed" histogram 2


def _place_edges(c):
    """repetition 0, per axis: contributions exactly on the first edge, an inner edge and the last edge of histogram 0, on the lower
    and the upper of histogram 2's narrower ranges, and a pair of duplicates (equal in x and in y).  Histogram 1 has a pair of
    equal neighbouring edges on each axis: the column between them holds nobody"""
    x, y = c["contribs"][:, c["px"], :], c["contribs"][:, c["py"], :]
    ex, ey = c["specs"][0]["edges_x"], c["specs"][0]["edges_y"]
    x[0, 0], x[1, 0], x[2, 0] = ex[0], ex[3], ex[-1]
    y[3, 0], y[4, 0], y[5, 0] = ey[0], ey[2], ey[-1]
    x[6, 0], x[7, 0] = RANGE_X
    y[8, 0], y[9, 0] = RANGE_Y
    x[10, 0] = x[11, 0] = 3.3e-8
    y[10, 0] = y[11, 0] = 7.7e-9
    c["claims"] = dict(first_x=0, inner_x=(1, 3), last_x=2, first_y=3, inner_y=(4, 2), last_y=5, lower_x=6, upper_x=7, lower_y=8, upper_y=9,
                       duplicates=(10, 11))


def _place_own_cells(c):
    """histogram 0 (64 x 64): contribution n in cell (n, 7 n mod 64), a cell of its own, in every repetition; histogram 2 (1 x 1)
    takes all N in its one cell"""
    ex, ey = c["specs"][0]["edges_x"], c["specs"][0]["edges_y"]
    n = np.arange(c["N"])
    c["contribs"][:, c["px"], :] = (0.5 * (ex[n] + ex[n + 1]))[:, None]
    c["contribs"][:, c["py"], :] = np.sqrt(ey[(7 * n) % 64] * ey[(7 * n) % 64 + 1])[:, None]
    c["claims"] = dict(own_cell=0, one_cell=2)


def _place_congruent(c):
    """histogram 0 (64 x 64): every y in column 5, so that every member's flat cell is 5 mod 64 and lane 5 owns them all; the x
    values stay random, several contributions share a cell"""
    ey = c["specs"][0]["edges_y"]
    rs = np.random.RandomState(77)
    c["contribs"][:, c["py"], :] = rs.uniform(ey[5] * 1.001, ey[6] * 0.999, (c["N"], c["R"]))
    c["claims"] = dict(congruent=(0, 5))


def _place_nan_inf(c):
    """the 'num' fraction of contribution 3 is NaN in repetition 1 (its cell of histogram 1 is stored as 0, the moments of that
    repetition are NaN), the 'num' limit of contribution 4 is +inf in repetition 0 (its cell's observability is +inf)"""
    c["frac8"][1][3, 1] = np.nan
    c["frac8"][5][4, 0] = np.inf
    c["claims"] = dict(nan_fraction=(1, 3, 1), inf_limit=(1, 4, 0), no_member=0)


def cases():
    """N in {1, 63, 64, 65, 130, 4096}; cells 1 x 1, 1 x 7, 7 x 1, 3 x 130, 63 x 65, 64 x 64, 0 x 5; R in {1, 3}; P 2 and 3 with
    (param_x, param_y) = (2, 0); all four weightings; three histograms of different sizes per call."""
    dup_x = [X_LO, 2e-8, 2e-8, 6e-8, X_HI]                     # a pair of equal neighbouring edges: column 1 is empty
    dup_y = [Y_LO, 4e-9, 4e-9, Y_HI]
    far = ([1.0, 2.0], [3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0])   # edges and ranges no value reaches: no member, nobody inside
    return [
        _case("n1", 1, 1, 2, 0, 1, [spec(0, 1, "vol", 1, 1), spec(0, 1, "num", 0, 5), spec(0, 1, "int", 1, 7)], 1, place=_place_one),
        _case("placed", 63, 3, 3, 2, 0, [spec(2, 0, "vol", 7, 4), spec(2, 0, "surf", 4, 3, ex=dup_x, ey=dup_y),
                                         spec(2, 0, "int", 7, 1, scale_x="log", rx=RANGE_X, ry=RANGE_Y)], 2, place=_place_edges),
        _case("own_cells", 64, 3, 2, 0, 1, [spec(0, 1, "vol", 64, 64), spec(0, 1, "num", 63, 65, scale_x="log"), spec(0, 1, "surf", 1, 1)],
              3, place=_place_own_cells),
        _case("congruent", 65, 3, 2, 0, 1, [spec(0, 1, "int", 64, 64), spec(1, 0, "vol", 3, 130, ex=edges_of(Y_LO, Y_HI, 3, "lin"),
                                                                          ey=edges_of(X_LO, X_HI, 130, "log")),
                                            spec(0, 0, "num", 7, 1, ey=[X_LO, X_HI])], 4, place=_place_congruent),
        _case("nan_inf", 130, 3, 3, 2, 0, [spec(2, 0, "vol", 1, 7, ex=far[0], ey=far[1]), spec(2, 0, "num", 3, 130),
                                           spec(2, 0, "surf", 0, 5)], 5, place=_place_nan_inf),
        _case("cap", 4096, 1, 2, 0, 1, [spec(0, 1, "vol", 1, 1), spec(0, 1, "num", 64, 64), spec(0, 1, "surf", 0, 5)], 6),
    ]


def swapped(sp):
    """the record with x and y exchanged"""
    return dict(param_x=sp["param_y"], param_y=sp["param_x"], yweight=sp["yweight"], edges_x=sp["edges_y"], edges_y=sp["edges_x"],
                lower_x=sp["lower_y"], upper_x=sp["upper_y"], lower_y=sp["lower_x"], upper_y=sp["upper_x"])


SWAP_ROWS = (0, 2, 1, 4, 3, 5, 6)          # total, mean y, mean x, variance y, variance x, covariance, correlation

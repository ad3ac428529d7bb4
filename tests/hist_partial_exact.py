"""Shared by test_hist_partial_host.py and test_hist_partial_gpu.py: the partial intensities of histogram ranges and bins
(csrc/hist_partial_kernel.h hist_partial_body; mcsas_amd/parameter.py partial_intensities) as
  - the cases: rows of the test's own choosing (hist_exact.fake_rows and edits of them), so that every curve is a function of
    known doubles, fed to the device through engine.histogram_device_rows,
  - exact rational sums of the selected rows (integers over a common power of two) times the scale, with the bound derived below,
  - the numpy form over a case, and
  - an fp64 emulation of the kernel's loop, a contribution at a time, with the degradations test_hist_partial_host.py wants caught.
A plain module like helpers.py: nothing in here is collected.  Nothing is fitted to a device's output.

The bound.  A curve value is `acc = 0.; acc += row[c][k]` over the m selected contributions in order, then `A * acc`
(hist_partial_body: `in_range += v`, `mine[64 b] += v`, `A * in_range`, `A * mine[64 b]`; -ffp-contract=off, no fused product).
The first addition, onto 0.0, is exact: m - 1 rounded additions and one rounded product, m roundings; the rows are not negative,
so nothing cancels and every partial sum is below the whole: |got - A S| <= gamma(m) A S (exact.gamma).  An addition of doubles
cannot underflow inexactly, the product can: where A S lies below the normal range its rounding error is half the smallest
subnormal at the most, 2^-1075, whatever its size — added to the bound.  m = 0: A * 0.0, an exact zero, compared by class.

Which contribution is in which bin or range is compared by equality, on the doubles themselves (hist_exact.bin_members,
hist_exact.moments_mask): a value on edges[b] is in bin b, on the last edge in none, on lower or upper outside the range, NaN nowhere."""
import math

import mpmath as mp
import numpy as np

import hist_exact as H
from exact import R, gamma
from fit_exact import exactly
from mcsas_amd.parameter import partial_intensities

HALF_SUBNORMAL = 2.0 ** -1075
SHIFT = 1140                          # every double is an integer over 2^SHIFT (the smallest subnormal is 2^-1074, a mantissa has 53 bits)
MUTATIONS = ("range_le", "upper_le", "scale_per_term", "acc32", "q_drop", "reverse")


# ------------------------------------------------------------------------------------------------- the cases
def _edit_nan(c):
    """a NaN parameter value in column 0 of repetition 0, set after the rows were made: it is in no bin and in no range"""
    c["contribs"][6, 0, 0] = np.nan
    c["claims"]["nan"] = (6, 0, 0)


def _case(name, N, nrep, nq, specs, want, seed, P=2, edit=None, place=None):
    c = H._case(name, N, nrep, nq, specs, seed, P=P, edit=edit, place=place)
    c["want"] = tuple(want)
    return c


def cases():
    """N in {1, 63, 64, 65, 130, 4096}, q in {1, 63, 64, 65, 130}, bins in {0, 1, 3, 64, 65, 256}, R in {1, 3}, one and two
    parameter columns with histograms on the second; "placed": three histograms wanting (2, 0, 1), contributions on the first, an
    inner and the last edge and on lower and upper (hist_exact._place_edges), a NaN value, a range holding nobody (the narrow one,
    repetition 1); "one" and "n64": a bin holding everything; "row_classes": rows of exact zeros and subnormals."""
    S = H.spec
    return [
        _case("one", 1, 1, 1, [S(0, "vol", 1, "lin")], (2,), 21, P=1),
        _case("placed", 65, 3, 63, [S(0, "vol", 8, "lin"), S(0, "num", 130, "log"), S(0, "int", 8, "lin", *H.NARROW)], (2, 0, 1), 22,
              place=H._place_edges, edit=_edit_nan),
        _case("row_classes", 7, 1, 64, [S(1, "num", 3, "log"), S(0, "vol", 0, "lin")], (2, 2), 23, edit=H._edit_rows),
        _case("n63", 63, 1, 64, [S(0, "vol", 64, "lin"), S(1, "num", 65, "log")], (2, 2), 24),
        _case("n64", 64, 3, 65, [S(0, "vol", 1, "lin"), S(1, "int", 3, "lin")], (2, 1), 25),
        _case("n65", 65, 1, 130, [S(0, "vol", 256, "log"), S(0, "num", 65, "lin")], (2, 2), 26, P=1),
        _case("n130", 130, 3, 1, [S(1, "vol", 64, "lin"), S(0, "surf", 3, "log"), S(0, "vol", 8, "lin", 1e-8, 5e-8)], (2, 0, 1), 27),
        _case("n4096", 4096, 1, 65, [S(0, "vol", 256, "lin")], (2,), 28, P=1),       # the LDS cap: 256 bins, 4096 contributions
    ]


def host_case(c):
    return H.host_case(c) if "rows" not in c else c


def wanted(c):
    """[(h, spec, want)] of the histograms that ask, in order"""
    return [(h, sp, w) for h, (sp, w) in enumerate(zip(c["specs"], c["want"])) if w]


def n_bins(sp):
    return len(sp["edges"]) - 1


# ------------------------------------------------------------------------------------------------- the numpy form over a case
def numpy_partial(c, A, form=partial_intensities):
    """{h: (range [nq][R], bin [n_bin][nq][R] or None)} by `form` (parameter.partial_intensities) a repetition at a time"""
    out = {}
    for h, sp, w in wanted(c):
        rng = np.zeros((c["nq"], c["R"]))
        bins = np.zeros((n_bins(sp), c["nq"], c["R"])) if w == 2 else None
        for r in range(c["R"]):
            a, b = form(c["rows"][r], c["contribs"][:, sp["param_index"], r], A[r], sp["lower"], sp["upper"], sp["edges"], w == 2)
            rng[:, r] = a
            if w == 2:
                bins[:, :, r] = b
        out[h] = (rng, bins)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def differing(x, y):
    """whether two numpy_partial-shaped results differ in a bit anywhere"""
    for h in x:
        for a, b in zip(x[h], y[h]):
            if a is not None and not same_bits(a, b):
                return True
    return False


# ------------------------------------------------------------------------------------------------- exact values and bounds
def _as_int(x):
    """the double x >= 0 as an integer over 2^SHIFT"""
    m, e = math.frexp(x)
    return int(m * 9007199254740992.0) << (e - 53 + SHIFT)


_INT = np.frompyfunc(_as_int, 1, 1)


@exactly
def exact_partial(c, A):
    """{h: (range [nq][R], bin [n_bin][nq][R] or None)} of exact.R (an exact 0 where nobody is selected), and the member counts
    {h: (in range [R], per bin [n_bin][R])}"""
    assert (c["rows"] >= 0).all()
    ints = [_INT(c["rows"][r]) for r in range(c["R"])]
    two = mp.mpf(2) ** SHIFT

    def curve(r, mask):
        m = int(mask.sum())
        if m == 0:
            return [R(0)] * c["nq"], 0
        tot = ints[r][mask].sum(axis=0)
        a = mp.mpf(float(A[r]))
        out = []
        for k in range(c["nq"]):
            v = mp.mpf(int(tot[k])) / two * a
            out.append(R(v, gamma(m) * abs(float(v)) + HALF_SUBNORMAL))
        return out, m
    vals, counts = {}, {}
    for h, sp, w in wanted(c):
        rng = np.empty((c["nq"], c["R"]), dtype=object)
        bins = np.empty((n_bins(sp), c["nq"], c["R"]), dtype=object) if w == 2 else None
        n_in, n_bin = np.zeros(c["R"], dtype=int), np.zeros((n_bins(sp), c["R"]), dtype=int)
        for r in range(c["R"]):
            x = np.ascontiguousarray(c["contribs"][:, sp["param_index"], r])
            rng[:, r], n_in[r] = curve(r, H.moments_mask(x, sp["lower"], sp["upper"]))
            if w == 2:
                for b, m in enumerate(H.bin_members(x, sp["edges"])):
                    bins[b, :, r], n_bin[b, r] = curve(r, m)
        vals[h], counts[h] = (rng, bins), (n_in, n_bin)
    return vals, counts


def look_partial(bad, worst, c, got, ref):
    """got {h: (range, bin)} against exact_partial's values: every value inside its bound, exact zeros by class"""
    assert sorted(got) == sorted(ref)
    for h in ref:
        for name, g, e in zip(("range", "bin"), got[h], ref[h]):
            if e is None:
                assert g is None
                continue
            assert g.shape == e.shape, (c["name"], h, name, g.shape, e.shape)
            for idx in np.ndindex(*e.shape):
                H.look(bad, worst, c["name"], "hist %d %s [%s]" % (h, name, ", ".join(map(str, idx))), g[idx], e[idx])


# ------------------------------------------------------------------------------------------------- emulation of the kernel's loop
def emu_partial(c, A, mutate=None):
    """hist_partial_body in numpy doubles, a contribution at a time in the kernel's order (all q-points of a row at once: a lane
    per q-point) -> numpy_partial's shape.  mutate: "range_le" (range mask not strict), "upper_le" (a bin's upper edge taken as
    <=), "scale_per_term" (A times every row instead of once at the end), "acc32" (float32 accumulators), "q_drop" (the last
    q-point of a tile's remainder of one left out: nq = 64 j + 1), "reverse" (contributions from the last to the first)."""
    dt = np.float32 if mutate == "acc32" else np.float64
    out = {}
    with np.errstate(all="ignore"):
        for h, sp, w in wanted(c):
            e = np.asarray(sp["edges"], dtype=np.float64)
            nb = len(e) - 1
            rng = np.zeros((c["nq"], c["R"]))
            bins = np.zeros((nb, c["nq"], c["R"])) if w == 2 else None
            for r in range(c["R"]):
                a = np.float64(A[r])
                x = c["contribs"][:, sp["param_index"], r]
                acc_r = np.zeros(c["nq"], dtype=dt)
                acc_b = np.zeros((nb, c["nq"]), dtype=dt)
                order = range(c["N"] - 1, -1, -1) if mutate == "reverse" else range(c["N"])
                for i in order:
                    row = c["rows"][r, i] * a if mutate == "scale_per_term" else c["rows"][r, i]
                    xi = x[i]
                    if (sp["lower"] <= xi <= sp["upper"]) if mutate == "range_le" else (sp["lower"] < xi < sp["upper"]):
                        acc_r = (acc_r + row.astype(dt)).astype(dt)
                    if w == 2:
                        for b in range(nb):
                            hi = xi <= e[b + 1] if mutate == "upper_le" else xi < e[b + 1]
                            if xi >= e[b] and hi and xi < e[-1]:
                                acc_b[b] = (acc_b[b] + row.astype(dt)).astype(dt)
                                break
                one = np.float64(1.0)
                rng[:, r] = (one if mutate == "scale_per_term" else a) * acc_r.astype(np.float64)
                if w == 2:
                    bins[:, :, r] = (one if mutate == "scale_per_term" else a) * acc_b.astype(np.float64)
                if mutate == "q_drop" and c["nq"] % 64 == 1:
                    rng[-1, r] = 0.0
                    if w == 2:
                        bins[:, -1, r] = 0.0
            out[h] = (rng, bins)
    return out

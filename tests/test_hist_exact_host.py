"""What McSAS.histogram() reads off a set of contributions, engine.observability and the re-binning, without a device: numpy fp64
emulations of the kernels' order (tests/hist_exact.py) against the EXACT value of the same discrete operation and the bound derived
from the operation order (tests/exact.py).  Pinned here:

  (a) every emulation lies inside its bound on every case the device module uses (test_hist_exact_gpu.py takes the same cases and the
      same bounds; the built-in models' cases with stand-in rows, since the arithmetic after the rows is a function of the doubles
      handed over) — a bound that misses an operation of the source fails here, where no device can be blamed;
  (b) the discrete claims of the cases hold for the exact reference alone: each placed value is in the bin or mask its case says,
      each product with the scale is the zero / non-zero class it says, the re-binning keeps the bins it says;
  (c) the bounds are not vacuous: eight degraded emulations each fall outside a bound, or break an equality, on some case;
  (d) the slack, bound / observed error of the emulation, is printed per quantity.

No tolerance here is anything but a bound computed by hist_exact.py."""
import math
from fractions import Fraction

import numpy as np
import pytest

import hist_exact as H

_CASES = {}


def case(name):
    """the finished host case and its scale and bounds, made once"""
    if not _CASES:
        for c in H.hist_cases():
            _CASES[c["name"]] = dict(c=H.host_case(c))
    e = _CASES[name]
    if "A" not in e:
        e["A"] = H.emu_scaling(e["c"])
        e["bounds"] = H.all_bounds(e["c"], e["A"])
    return e["c"], e["A"], e["bounds"]


NAMES = [c["name"] for c in H.hist_cases()]


def _slack(what, worst):
    for k, v in sorted(H.summarise(worst).items()):
        print("%s  %-8s  bound / error %s" % (what, k, "%.3g" % (1.0 / v) if v > 0 else "inf (exact)"))


# ------------------------------------------------------------------------------------------------- (a), (d)
@pytest.mark.parametrize("name", NAMES)
def test_histogram_emulation_inside_its_bounds(name):
    c, A, bounds = case(name)
    assert (A > 0).all() and np.isfinite(A).all() and (A < 0.5).all()            # (below 1/2: the smallest subnormal times A is 0)
    bad, worst = [], {}
    H.look_triple(bad, worst, c, H.emu_histogram(c, A), bounds)
    _slack(name, worst)
    assert not bad, "\n".join(bad[:40])


def test_sizes_the_cases_cover():
    cs = H.hist_cases()
    assert {c["N"] for c in cs} >= {1, 7, 63, 64, 65, 129, 2731}
    assert {c["R"] for c in cs} == {1, 3}
    assert {c["nq"] for c in cs} >= {1, 63, 64, 65, 130}
    bins = lambda c: {len(sp["edges"]) - 1 for sp in c["specs"]}
    assert set().union(*[bins(c) for c in cs]) >= {1, 63, 64, 65, 130}
    for N in (63, 64, 65):
        assert set().union(*[bins(c) for c in cs if c["N"] == N]) >= {63, 64, 65}
    big = [c for c in cs if c["N"] == 2731][0]
    assert 3 * 8 * 2730 <= 65536 < 3 * 8 * 2731 and len(big["specs"]) == 1 and bins(big) == {8}
    explicit = [c for c in cs if not c["builtin"]]
    assert all(c["P"] == 2 for c in explicit)
    assert {sp["yweight"] for c in explicit for sp in c["specs"]} == set(H.WEIGHTS)
    assert {sp["param_index"] for c in explicit for sp in c["specs"]} == {0, 1}
    for c in cs:
        for sp in c["specs"]:
            e = sp["edges"]
            assert (np.diff(e) > 0).all() and e[0] == sp["lower"] and e[-1] == sp["upper"]


# ------------------------------------------------------------------------------------------------- (b)
def test_placed_values_are_where_the_case_says():
    c, A, (fr, hb) = case("placed")
    cl = c["claims"]
    x = c["contribs"]
    h, i, r, b = cl["first_edge"]
    sp = c["specs"][h]
    assert x[i, sp["param_index"], r] == sp["edges"][0] and H.bin_members(x[:, sp["param_index"], r], sp["edges"])[b][i] and b == 0
    h, i, r, b = cl["inner_edge"]
    sp = c["specs"][h]
    m = H.bin_members(x[:, sp["param_index"], r], sp["edges"])
    assert x[i, sp["param_index"], r] == sp["edges"][b] and 0 < b < len(m) and m[b][i] and not m[b - 1][i]
    h, i, r = cl["last_edge"]
    sp = c["specs"][h]
    assert x[i, sp["param_index"], r] == sp["edges"][-1] and not any(mm[i] for mm in H.bin_members(x[:, sp["param_index"], r], sp["edges"]))
    for key in ("lower", "upper"):
        h, i, r = cl[key]
        sp = c["specs"][h]
        assert x[i, sp["param_index"], r] == sp[key] and not H.moments_mask(x[:, sp["param_index"], r], sp["lower"], sp["upper"])[i]
    assert c["specs"][cl["lower"][0]]["lower"] > H.PAR_LO[0] and c["specs"][cl["upper"][0]]["upper"] < H.PAR_HI[0]      # a narrower range
    h, r = cl["nobody"]
    ref = hb[h][r]
    assert ref["n_in"] == 0 and sum(ref["counts"]) == 0
    assert all(q.v == 0 and q.e == 0 for k in ("bins", "obs", "cdf", "moments") for q in ref[k])
    h, r, i = cl["one"]
    ref = hb[h][r]
    sp = c["specs"][h]
    assert ref["n_in"] == 1 and H.moments_mask(x[:, sp["param_index"], r], sp["lower"], sp["upper"])[i] and H.is_pow2(x[i, sp["param_index"], r])
    assert float(ref["moments"][0].v) > 0 and float(ref["moments"][1].v) == x[i, sp["param_index"], r]
    assert all(q.v == 0 and q.e == 0 for q in ref["moments"][2:])
    h, r = cl["empty_bin"]
    assert 0 in hb[h][r]["counts"] and max(hb[h][r]["counts"]) > 0


def test_zero_total_and_zero_volume():
    c, A, (fr, hb) = case("zero_surface")
    assert (c["s"] == 0).all()
    assert all(q.v == 0 and q.e == 0 for q in fr["sf"].ravel())                   # exact zeros, no division
    ref = hb[0][0]                                                                # the surface-weighted histogram
    assert all(q.v == 0 and q.e == 0 for q in ref["bins"] + ref["cdf"]) and ref["n_in"] > 1
    assert [H.klass(H._fl(q)) for q in ref["moments"]] == ["0", "0", "nan", "nan", "nan"]        # 0 / 0 and what follows from it
    c, A, (fr, hb) = case("zero_volume")
    i, r = c["claims"]["zero_volume"]
    assert c["v"][i, r] == 0 and (np.delete(c["v"][:, r], i) > 0).all()
    assert fr["vf"][i, r] == math.inf and fr["mv"][i, r] == math.inf and fr["qf"][i, r] != fr["qf"][i, r]
    kl = {k: [H.klass(H._fl(q)) for q in fr[k][:, r]] for k in H.FRAC8}
    assert set(kl["qf"]) == {"nan"} and set(kl["mq"]) == {"nan"}                  # inf 0 = NaN in the total
    assert kl["nf"].count("nan") == 1 and kl["nf"].count("0") == c["N"] - 1       # inf / inf, and x / inf
    assert kl["vf"].count("number") == c["N"] - 1
    h_num = [h for h, sp in enumerate(c["specs"]) if sp["yweight"] == "num" and sp["param_index"] == 0][0]
    b = [b for b, n in enumerate(hb[h_num][r]["counts"]) if n and H.bin_members(c["contribs"][:, 0, r], c["specs"][h_num]["edges"])[b][i]]
    assert len(b) == 1 and hb[h_num][r]["bins"][b[0]].v == 0                      # the NaN sum became 0
    for rr in (0, 2):                                                             # the other repetitions are whole
        assert all(not H.special(q) for k in H.FRAC8 for q in fr[k][:, rr])


def test_products_with_the_scale_are_the_class_the_case_says():
    c, A, (fr, hb) = case("row_classes")
    rows = c["rows"][0]
    a = Fraction(float(A[0]))
    half_tiny = Fraction(1, 2 ** 1075)
    for i in range(c["N"]):
        exact = [a * Fraction(float(x)) for x in rows[i]]
        kept = H.scaled_classes(A[0], rows[i])
        for k, p in enumerate(exact):
            cls = "zero" if p == 0 else ("underflow" if p <= half_tiny else ("normal" if p > Fraction(1, 2 ** 900) else "neither"))
            assert cls != "neither" and kept[k] == (cls == "normal"), (i, k, cls)
    cls = lambda i: [("zero" if x == 0 else ("underflow" if x == H.TINY else "normal")) for x in rows[i]]
    assert set(cls(0)) == {"zero"} and set(cls(1)) == {"underflow"}
    assert set(cls(2)[0::2]) == {"zero"} and set(cls(2)[1::2]) == {"normal"}
    assert set(cls(3)[:32]) == {"underflow"} and set(cls(3)[32:]) == {"normal"}
    assert all(set(cls(i)) == {"normal"} for i in range(4, c["N"]))
    assert fr["mv"][0, 0] == math.inf and fr["mv"][1, 0] == math.inf              # an empty minimum: +inf (visibility_limit's `best = __builtin_inf()`)
    assert all(not H.special(fr["mv"][i, 0]) for i in range(2, c["N"]))
    c, A, _ = case("n64")
    i = c["claims"]["min_at_last_q"]
    cand = [Fraction(float(s)) / Fraction(float(x)) for s, x in zip(c["sigma"], c["rows"][0, i])]
    assert c["nq"] == 65 and cand.index(min(cand)) == 64


def test_specials_stand_where_the_reference_lines_put_them():
    """NaN, +-inf and exact 0 of the exact reference (IEEE's rules applied to the kernel's operations) are those of a plain numpy
    transcription of the reference's lines, on every case; the cases made for it do hold each kind"""
    kinds = {}
    for name in NAMES:
        c, A, bounds = case(name)
        got = H.reference_lines(c, A)
        bad = H.classes_differ(c, got, bounds, "reference lines")
        assert not bad, "\n".join(bad[:20])
        flat = np.concatenate([a.ravel() for pair in got[1].values() for a in pair] + [h[k].ravel() for h in got[2] for k in h])
        kinds[name] = {H.klass(v) for v in flat}
    print(kinds)
    assert kinds["zero_volume"] >= {"nan", "+inf", "0", "number"} and kinds["zero_surface"] >= {"nan", "0", "number"}
    assert kinds["row_classes"] >= {"+inf", "number"} and "nan" not in kinds["row_classes"]
    assert all("-inf" not in k for k in kinds.values())
    assert all(kinds[n] <= {"0", "number"} for n in NAMES if n not in ("zero_volume", "zero_surface", "row_classes"))


def test_no_intermediate_leaves_the_normal_range():
    """the relative bounds (gamma) count roundings of normal numbers: every finite non-zero value of the emulation is one"""
    for name in NAMES:
        c, A, _ = case(name)
        sc, fr, hs = H.emu_histogram(c, A)
        for arr in [a for pair in fr.values() for a in pair] + [h[k] for h in hs for k in h]:
            v = np.abs(arr[np.isfinite(arr) & (arr != 0)])
            assert not len(v) or (v.min() > 1e-290 and v.max() < 1e290), name


# ------------------------------------------------------------------------------------------------- observability_kernel
@pytest.mark.parametrize("name", [c["name"] for c in H.builtin_cases()])
def test_observability_emulation_inside_its_bound(name):
    c, A, _ = case(name)
    vf = c["w"] * A[None, :] / c["v"]
    bad, worst = [], {}
    for r in range(c["R"]):
        for i in range(c["N"]):
            got = np.fmin.reduce((c["sigma"] * vf[i, r]) / (A[r] * c["rows"][r, i]), initial=np.inf)
            H.look(bad, worst, name, "limit [%d, %d]" % (i, r), got, H.obs_bound(c["sigma"], c["rows"][r, i], vf[i, r], A[r]))
    _slack(name, worst)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------- re-binning
REBIN = {c["name"]: c for c in H.rebin_cases()}


@pytest.mark.parametrize("name", sorted(REBIN))
def test_rebin_emulation_inside_its_bounds(name):
    c = REBIN[name]
    ref = H.rebin_bounds(c["x"], c["f"], c["fu"], c["n_bin"])
    bad, worst = [], {}
    H.look_rebin(bad, worst, name, H.emu_rebin(c["x"], c["f"], c["fu"], c["n_bin"]), ref)
    _slack(name, worst)
    assert not bad, "\n".join(bad)


def test_rebin_cases_hold_what_they_claim():
    seen = set()
    assert sorted({len(c["x"]) for c in REBIN.values()}) == [2, 63, 64, 65, 200]
    for name, c in REBIN.items():
        x, f, fu, nb = c["x"], c["f"], c["fu"], c["n_bin"]
        edges = H.rebin_edges(x, nb)
        members = H.rebin_members(x, edges)
        counts = [len(m) for m in members]
        ref = H.rebin_bounds(x, f, fu, nb)
        assert sum(counts) == len(x) and len(x) - 1 in members[-1]                # the widening keeps the last point
        dropped = [b for b, m in enumerate(members) if len(m) and np.isnan(f[m]).any()]
        assert [q["bin"] for q in ref] == [b for b, n in enumerate(counts) if n and b not in dropped]
        seen |= {"empty"} if 0 in counts else set()
        seen |= {"two"} if 2 in counts else set()
        seen |= {"over 64"} if max(counts) > 64 else set()
        seen |= {"single, lane %s" % ("0" if m[0] % 64 == 0 else ">= 1") for m in members if len(m) == 1}
        seen |= {q["wins"] for q in ref if q["count"] > 1}
        cl = c["claims"]
        if "on_edge" in cl:
            j, b = cl["on_edge"]
            assert x[j] == edges[b] and j in members[b] and 0 < b < nb
            seen.add("on an inner edge")
        if "nan_fu" in cl:
            b = [b for b, m in enumerate(members) if cl["nan_fu"] in m][0]
            q = [q for q in ref if q["bin"] == b][0]
            assert q["fu"] != q["fu"] and not H.special(q["f"])                   # kept, its uncertainty NaN
            seen.add("nan fu")
        if "nan_f" in cl:
            b = [b for b, m in enumerate(members) if cl["nan_f"] in m][0]
            assert b in dropped
            seen.add("nan f, %s" % ("one point" if counts[b] == 1 else "several"))
        if "equal" in cl:
            b = [b for b, m in enumerate(members) if cl["equal"] in m][0]
            q = [q for q in ref if q["bin"] == b][0]
            assert counts[b] > 64 and len(set(f[members[b]])) == 1 and q["wins"] == "propagated"
            seen.add("equal f")
    print(sorted(seen))
    assert seen >= {"empty", "two", "over 64", "single, lane >= 1", "scatter", "propagated", "nan", "on an inner edge", "nan fu", "equal f"}
    assert any(s.startswith("nan f,") for s in seen)


# ------------------------------------------------------------------------------------------------- (c)
MUTATIONS = {"upper_le": "placed", "moments_le": "placed", "obs_N": "placed", "bin32": "placed", "q_drop": "n64", "mq_short": "placed"}


@pytest.mark.parametrize("mutate", sorted(MUTATIONS))
def test_degraded_histogram_emulations_fall_outside(mutate):
    c, A, bounds = case(MUTATIONS[mutate])
    bad = []
    H.look_triple(bad, {}, c, H.emu_histogram(c, A, mutate), bounds)
    print("%s: %d values outside, e.g.\n  %s" % (mutate, len(bad), "\n  ".join(bad[:4])))
    assert bad, "the mutation %r passes every bound and every equality" % mutate


@pytest.mark.parametrize("mutate,name", [("drop", "n65-20bins"), ("drop", "n65-7bins"), ("ddof0", "n65-7bins")])
def test_degraded_rebin_emulations_fall_outside(mutate, name):
    c = REBIN[name]
    bad = []
    H.look_rebin(bad, {}, name, H.emu_rebin(c["x"], c["f"], c["fu"], c["n_bin"], mutate), H.rebin_bounds(c["x"], c["f"], c["fu"], c["n_bin"]))
    print("%s on %s: %s" % (mutate, name, "; ".join(bad[:3])))
    assert bad, "the mutation %r passes every bound and every equality" % mutate

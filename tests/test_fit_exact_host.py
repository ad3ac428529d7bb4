"""The scale / background fit and the chi-squared of a step, without a device: numpy fp64 emulations of the kernels' formulas in the
kernels' order (tests/fit_exact.py) against the EXACT value of the same discrete operation (mpmath, 60 digits) and the bound derived
from the operation order (tests/exact.py).  Three things are pinned here:

  (a) every emulation lies inside its bound on every case the device modules use (test_fit_exact_gpu.py takes the same cases and the
      same bounds) — a bound that misses an operation of the source fails here, where no device can be blamed;
  (b) the bounds are not vacuous: four degraded emulations (a sum accumulated in float32, the uncentred expansion where the step has
      centred sums, a lane's last slot dropped at 65 q, w = (1 / sigma)^2 in float32) each fall OUTSIDE a bound on some case;
  (c) the slack, bound / observed error of the emulation, is printed per quantity; its maximum is quoted in DESIGN §2.

The comparison of two states of one chain (decision_bound) is checked on a pair of model intensities a proposal apart."""
import numpy as np
import pytest

import fit_chains as FC
import fit_exact as F


def _pair(c):
    """a second state of the same chain: the model intensity with one of 16 equal contributions replaced by one 3 % larger in radius
    — here simply a smooth relative change of a few parts in a thousand over q"""
    n = len(c["C"])
    t = np.linspace(0.0, 1.0, n) if n > 1 else np.zeros(1)
    return c["C"] * (1.0 + 4e-3 * np.cos(5.0 * t) / 16.0)


def _check_case(c, slack, mutate=None, geometry=(None, 1)):
    """the emulations of one case against their bounds -> the names of the quantities outside; slack[name] = largest bound / error"""
    out = []
    I, sg, C, fb, pb = c["I"], c["sigma"], c["C"], c["find_bg"], c["pos_bg"]
    x = F.exact_fit(I, sg, C, fb, pb)

    def look(name, got, ref):
        r = F.within(got, ref)
        if not r <= 1.0:
            out.append("%s %s: %.3g of its bound (bound %.3g, exact %.6g)" % (c["name"], name, r, ref.e, float(ref.v)))
        elif r > 0:
            lo, hi = slack.get(name, (np.inf, 0.0))
            slack[name] = (min(lo, 1.0 / r), max(hi, 1.0 / r))
            mine.append(1.0 / r)

    mine = []
    if geometry == (None, 1) and mutate != "uncentred":
        for p in (1, 4):
            if len(I) == p:
                continue
            xb = x if p == 1 else F.exact_fit(I, sg, C, fb, pb, p)
            bd = F.bgfit_bounds(xb, I, sg, C, fb, p)
            if mutate is None and pb:                             # (1,1): the sign of the free b, checked with the exact fit
                assert F.branch_is_defined(xb, bd), c["name"]
                assert (xb["b_free"] < 0) == (c["kind"] == "clamped") == xb["clamp"], c["name"]
            got = F.emu_bgfit(I, sg, C, fb, pb, p, mutate)
            look("bgfit A", got[0], bd["A"]); look("bgfit b", got[1], bd["b"]); look("bgfit chi2", got[2], bd["chi2"])
            if len(I) > p:
                look("bgfit aGoFs", got[3], bd["agofs"])
    if len(I) < 2:
        return out
    sl, wv = geometry
    bd = F.chain_bounds(x, I, sg, C, fb, 0.0, sl, wv)
    got = F.emu_chain(I, sg, C, fb, pb, sl, wv, mutate)
    for k, name in (("A", "chain A"), ("b", "chain b"), ("chisq0", "chisq0"), ("inloop", "in-loop chi2"), ("final", "final chi2")):
        look(name, got[k], bd[k])
    # the comparison of two states: the explained sums' difference against the exact one, S (one double per chain) cancelling
    Ct = _pair(c)
    xt = F.exact_fit(I, sg, Ct, fb, pb) if len(I) < 1000 else None          # (a thousand fma's in rational arithmetic: once is enough)
    if xt is not None and xt["clamp"] == x["clamp"]:
        bt = F.chain_bounds(xt, I, sg, Ct, fb, 0.0, sl, wv)
        gt = F.emu_chain(I, sg, Ct, fb, pb, sl, wv, mutate)
        n = x["n"]
        ref = F.R(0, 0)
        with F.exactly:
            ref = F.R((xt["expl"] - x["expl"]) / n, F.decision_bound(bt["expl"], bd["expl"], x["X"], n))
        look("chi2 - chi2_t", (gt["expl"] - got["expl"]) / n, ref)
    if mutate is None and mine:
        print("%-34s bound / error of its quantities: %.3g .. %.3g" % (c["name"], min(mine), max(mine)))
    return out


@pytest.mark.parametrize("nq", F.NQS)
def test_emulations_inside_their_bounds(nq):
    """(a), (c): bgfit_kernel's four outputs and a chain's chisq0 / in-loop / final chi-squared, scale and background, and the
    difference of two states, on every case of the one-call fits at this q-count"""
    slack, bad = {}, []
    cases = F.fit_cases(nq) + (F.single_point_cases() if nq == F.NQS[0] else [])
    for c in cases:
        bad += _check_case(c, slack)
    for k in sorted(slack):
        print("nq %4d  %-14s  bound / error %.3g .. %.3g" % ((nq, k) + slack[k]))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("nq,slots,waves", [(65, 2, 1), (200, 4, 1), (1500, 32, 1), (1025, 8, 3)])
def test_chain_geometries_inside_their_bounds(nq, slots, waves):
    """(a) at the q-counts and layouts of the chain kernels the device module runs: the wave kernel's 2, 4 and 32 slots, the
    q-split kernel's 8 slots x 3 waves (the last wave holding one real point)"""
    slack, bad = {}, []
    for flags in F.FLAGS[:3]:
        for rung in F.LADDER[:3]:
            bad += _check_case(F.fit_case(nq, flags, rung, si_units=False), slack, geometry=(slots, waves))
    for k in sorted(slack):
        print("nq %4d (%d slots, %d waves)  %-14s  bound / error %.3g .. %.3g" % ((nq, slots, waves, k) + slack[k]))
    assert not bad, "\n".join(bad)


MUTATIONS = ("f32", "uncentred", "drop", "w32")


@pytest.mark.parametrize("mutate", MUTATIONS)
def test_degraded_emulations_fall_outside(mutate):
    """(b): the bounds would notice a sum in float32, the uncentred expansion in the step, a dropped slot at 65 q, float32 weights"""
    caught = []
    nqs = (65,) if mutate == "drop" else (65, 129)
    for nq in nqs:
        for flags in F.FLAGS[:2]:
            for rung in F.LADDER:
                caught += _check_case(F.fit_case(nq, flags, rung, si_units=False), {}, mutate)
    print("%s: %d quantities outside their bounds, e.g.\n  %s" % (mutate, len(caught), "\n  ".join(caught[:6])))
    assert caught, "the mutation %r passes every bound: the bounds are too wide to be worth anything" % mutate


@pytest.mark.parametrize("key", sorted(FC.CHOSEN), ids=lambda k: "%s-u%g-%s" % k)
def test_chosen_chains_meet_their_conditions(key):
    """The workloads test_fit_exact_gpu.py sets down next to a good fit, with the oracle alone: (i) chisq0 in 1 .. 100, (ii) at least
    three accepted moves, (iii) every step's margin at least ten times the derived bound of its comparison — where decisions are
    asserted; at u = 1e-6 they are not (fit_chains.CHOSEN) and the margin found is printed.  And (a) on these cases: the emulation of
    the chain's order on the oracle's own states (chain 0: the start, the first three accepted ones and the last) inside the bounds."""
    wl = FC.chosen(key)
    decisions = FC.CHOSEN[key][3]
    om = FC.oracle_margins(wl)
    for r, o in enumerate(om):
        print("%s chain %d: chisq0 %.4g, %d moves, smallest margin / bound %.3g (%d steps without a defined branch), "
              "bound of the in-loop chi2 %.3g of it" % (key, r, o["chisq0"], o["moves"], o["margin_over_bound"], o["undefined"], o["bound_rel"]))
        assert 1.0 <= o["chisq0"] <= 100.0 and o["moves"] >= 3
        assert wl["chains"][r]["ref"].num_iter == FC.CHAIN_STEPS
        if decisions:
            assert o["margin_over_bound"] >= 10.0
    if not decisions:
        assert key[1] == 1e-6 and min(o["margin_over_bound"] for o in om) < 10.0
    c = wl["chains"][0]
    I, sg, fb, pb, sl, wv = wl["I"], wl["sig"], wl["find_bg"], wl["pos_bg"], wl["slots"], wl["waves"]
    slack, bad = {}, []
    for k, s in enumerate([None] + list(c["ref"].accepted)[:3] + list(c["ref"].accepted)[-1:]):
        C = c["fits"][1][0] if s is None else c["fits"][2 + s][0]
        x = F.exact_fit(I, sg, C, fb, pb)
        bd = F.chain_bounds(x, I, sg, C, fb, 0.0, sl, wv)
        got = F.emu_chain(I, sg, C, fb, pb, sl, wv)
        for name in ("chisq0", "inloop", "final", "A", "b"):
            r = F.within(got[name], bd[name])
            if not r <= 1.0:
                bad.append("%s state %d %s: %.3g of its bound" % (key, k, name, r))
            elif r > 0:
                lo, hi = slack.get(name, (np.inf, 0.0))
                slack[name] = (min(lo, 1.0 / r), max(hi, 1.0 / r))
    for k in sorted(slack):
        print("%s  %-8s bound / error %.3g .. %.3g" % ((key, k) + slack[k]))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("nq", sorted(FC.FINAL_GEOMETRY))
def test_cold_chains_of_the_final_fit_cases(nq):
    """the cold chains whose final fit the device module checks in the modes without a start: they move, run to their budget, and
    the oracle takes every decision with ten times its derived bound to spare (the device module asserts the oracle's final set)"""
    wl = FC.final_workload(nq)
    for c, o in zip(wl["chains"], FC.oracle_margins(wl)):
        print("nq %d: chisq0 %.4g, %d moves, smallest margin / bound %.3g" % (nq, o["chisq0"], o["moves"], o["margin_over_bound"]))
        assert c["ref"].num_iter == FC.FINAL_STEPS and c["ref"].num_moves >= 3 and c["pos"] == FC.FINAL_N + FC.FINAL_STEPS
        assert o["margin_over_bound"] >= 10.0

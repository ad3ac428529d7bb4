"""The scale / background fit and the chi-squared on the device against exact values, each inside the bound derived for it from the
kernel's operation order (tests/fit_exact.py, tests/exact.py; the same cases and bounds hold the numpy emulations in
test_fit_exact_host.py, so a device value outside a bound its emulation keeps is the kernel's).  No assertion here has a tolerance
that is not such a bound; the only comparisons by equality are steps, counts and recorded values against the oracle, on chains whose
every decision the oracle makes with ten times the bound to spare (test_fit_exact_host.py re-checks that).

  1. engine.bgfit (bgfit_kernel): A, b, the residual chi-squared and aGoFs (num_params 1 and 4), 2 .. 1000 q, every flag set, both
     conditioning ladders, SI and order-one units, exact zeros among the uncertainties;
  2. engine.histogram_prep (hist_fit_cum_kernel: the same solve_fit on a path of its own) against model_calc's summed intensity;
  3. the chi-squared of given starts and of every accepted move of the wave and q-split kernels (analyse(start=, trace=));
  4. the final fit of the modes that take neither."""
import numpy as np
import pytest

import fit_chains as FC
import fit_exact as F
from exact import U
from mcsas_amd import engine
from helpers import make_models

pytestmark = pytest.mark.gpu


def _look(bad, worst, case, name, got, ref):
    r = F.within(got, ref)
    worst[name] = max(worst.get(name, 0.0), r)
    if not r <= 1.0:
        bad.append("%s %s: got %.17g, exact %.17g, error %.3g of its bound %.3g" % (case, name, got, float(ref.v), r, ref.e))


def _report(what, worst, bad):
    for k in sorted(worst):
        print("%s  %-12s  largest error / bound %.3g" % (what, k, worst[k]))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------- 1. bgfit
@pytest.mark.parametrize("nq", F.NQS)
def test_bgfit_against_exact(nq):
    """bgfit_kernel's A, b, residual chi-squared and aGoFs inside their derived bounds on every case of this q-count (and, at the
    smallest, the single point without a background)"""
    bad, worst = [], {}
    for c in F.fit_cases(nq) + (F.single_point_cases() if nq == F.NQS[0] else []):
        I, sg, C, fb, pb = c["I"], c["sigma"], c["C"], c["find_bg"], c["pos_bg"]
        for p in (1, 4):
            x = F.exact_fit(I, sg, C, fb, pb, p)
            bd = F.bgfit_bounds(x, I, sg, C, fb, p)
            sc, conval, agofs = engine.bgfit(I, sg, C, fb, pb, p)
            _look(bad, worst, c["name"], "A", sc[0], bd["A"]); _look(bad, worst, c["name"], "b", sc[1], bd["b"])
            _look(bad, worst, c["name"], "chi2", conval, bd["chi2"])
            if len(I) > p:
                _look(bad, worst, c["name"], "aGoFs p=%d" % p, agofs, bd["agofs"])
    _report("bgfit nq %d" % nq, worst, bad)


# ------------------------------------------------------------------------------------------------- 2. histogram_prep's scaling rows
HIST_N, HIST_R = 5, 3
HIST_RADII = np.array([4e-9, 7e-9, 1.1e-8, 1.9e-8, 3.1e-8])


def _hist_sets():
    """[N][1][R]: repetition 0 the radii the data are made of, 1 and 2 a few parts in a thousand away from them"""
    out = np.zeros((HIST_N, 1, HIST_R))
    for r in range(HIST_R):
        out[:, 0, r] = HIST_RADII * (1.0 + 2e-3 * r * np.cos(np.arange(HIST_N)))
    return out


@pytest.mark.parametrize("nq", (1,) + F.NQS)
def test_histogram_prep_scaling_against_exact(nq):
    """hist_fit_cum_kernel's scale and background per repetition inside the bounds of the exact fit against model_calc's cum of the
    same sets (input error: the (N + 1) u C of an ordered sum of N positive rows), over the u ladder, the flag sets and both units"""
    m, _ = make_models("sphere", [2e-9], [3e-7])
    setup = m.setup()
    q = np.logspace(8.0, 9.3, nq) if nq > 1 else np.array([3e8])
    sets = _hist_sets()
    comp = 0.5
    cums = [engine.model_calc(setup, q, np.ascontiguousarray(sets[:, :, r]), comp)[0] for r in range(HIST_R)]
    bad, worst = [], {}
    for fi, flags in enumerate(F.FLAGS):
        find_bg, pos_bg, kind = flags
        if nq == 1 and find_bg:
            continue
        for ui, u in enumerate((1e-2, 1e-4, 1e-6)):
            si_units = (fi + ui + nq) % 2 == 1
            C0 = cums[0]
            A0 = (3e-28 if si_units else 1.0) / C0.max()
            b0 = {"free": 0.02, "nobg": 0.0, "clamped": -0.3, "posb": 0.02}[kind] * A0 * C0.min()
            I0 = A0 * C0 + b0
            sg = u * I0
            I = I0 + sg * np.random.RandomState(31 * nq + 7 * fi + ui).standard_normal(nq)
            sc = engine.histogram_prep(setup, q, I, sg, sets, comp, find_background=find_bg, positive_background=pos_bg)[0]
            for r in range(HIST_R):
                C = cums[r]
                x = F.exact_fit(I, sg, C, find_bg, pos_bg)
                bd = F.bgfit_bounds(x, I, sg, C, find_bg, 1, eC=(HIST_N + 1) * U * C)
                name = "nq%d-%s-u%g-%s rep %d" % (nq, kind, u, "SI" if si_units else "one", r)
                if pos_bg:
                    assert F.branch_is_defined(x, bd), name
                _look(bad, worst, name, "scaling", sc[0, r], bd["A"]); _look(bad, worst, name, "background", sc[1, r], bd["b"])
    _report("histogram_prep nq %d" % nq, worst, bad)


# ------------------------------------------------------------------------------------------------- 3. the chi-squared of a step
def _device_rows(setup, q, radii, comp_exp):
    """model_calc's rows of these radii and, per row, the bound on what the chain's own evaluator may differ by"""
    _, _, w, _, rows = engine.model_calc(setup, q, np.ascontiguousarray(np.asarray(radii, dtype=float)[:, None]), comp_exp, want_rows=True)
    gaps = np.array([FC.sphere_row_gap(q, r, wi) for r, wi in zip(radii, w)])
    return rows, gaps


@pytest.mark.parametrize("key", sorted(FC.CHOSEN), ids=lambda k: "%s-u%g-%s" % k)
def test_chain_chisq_against_exact(key):
    """analyse(start=, trace=): chisq0 (solve_fit's expansion) and the chi-squared after every accepted move (the centred X / nq) inside
    the derived bound of the exact chi-squared at the exact optimum of the recorded set, its rows from model_calc; the final chisq
    (residual form), scaling and background inside theirs; and, where the oracle decides every step with ten times the bound to
    spare (fit_chains.CHOSEN), steps, counts and recorded values equal to the oracle's."""
    wl = FC.chosen(key)
    decisions = FC.CHOSEN[key][3]
    setup, q, I, sg, st = wl["model"].setup(), wl["q"], wl["I"], wl["sig"], wl["st"]
    fb, pb, sl, wv = wl["find_bg"], wl["pos_bg"], wl["slots"], wl["waves"]
    n = st.n_contrib
    res = engine.analyse(setup, q, I, sg, st, replay=wl["replay"], start=np.array(wl["start"]), trace=FC.CAPACITY)
    tr = res.trace
    bad, worst = [], {}
    for r in range(FC.REPS):
        cnt = int(tr.count[r])
        print("%s chain %d: %d steps, %d moves (oracle %d), chisq0 %.17g, last chi2 %.17g, final %.17g"
              % (key, r, res.num_iter[r], cnt, wl["chains"][r]["ref"].num_moves, tr.chisq0[r], tr.chisq[max(cnt - 1, 0), r], res.chisq[r]))
        assert res.num_iter[r] == FC.CHAIN_STEPS and res.num_moves[r] == cnt and 0 <= cnt <= FC.CAPACITY
        radii = np.concatenate([wl["start"][:, 0, r], tr.values[:cnt, 0, r]])
        rows, gaps = _device_rows(setup, q, radii, st.comp_exp)
        states = FC.input_error(rows[:n], gaps[:n], [(int(tr.step[m, r]) % n, rows[n + m], gaps[n + m]) for m in range(cnt)])
        assert np.array_equal(np.sort(res.contribs[:, 0, r]), np.sort(_final_set(wl["start"][:, 0, r], tr, r, cnt, n)))
        for m, (C, eC) in enumerate(states):
            x = F.exact_fit(I, sg, C, fb, pb)
            bd = F.chain_bounds(x, I, sg, C, fb, eC, sl, wv)
            name = "%s chain %d state %d" % (key, r, m)
            if pb:
                assert F.branch_is_defined(x, bd), name
            if m == 0:
                _look(bad, worst, name, "chisq0", tr.chisq0[r], bd["chisq0"])
            else:
                _look(bad, worst, name, "in-loop chi2", tr.chisq[m - 1, r], bd["inloop"])
        _look(bad, worst, name, "final chisq", res.chisq[r], bd["final"])
        _look(bad, worst, name, "scaling", res.scaling[r], bd["A"]); _look(bad, worst, name, "background", res.background[r], bd["b"])
        print("%s chain %d: bound of the last in-loop chi2 %.3g of it" % (key, r, bd["inloop"].e / float(x["chi2"])))
        if decisions:
            t = FC.oracle_trace(wl["chains"][r])
            assert cnt == len(t["step"]) and np.array_equal(tr.step[:cnt, r], t["step"]), name
            assert np.array_equal(tr.values[:cnt, :, r], t["values"]), name
            assert np.array_equal(res.contribs[:, :, r], wl["chains"][r]["ref"].rset), name
    _report("%s-u%g-%s" % key, worst, bad)


def _final_set(start, tr, r, cnt, n):
    out = np.array(start, dtype=float)
    for m in range(cnt):
        out[int(tr.step[m, r]) % n] = tr.values[m, 0, r]
    return out


# ------------------------------------------------------------------------------------------------- 4. the final fit of the other modes
def _host_rows(wl):
    """the numpy twin of the sphere (helpers.PythonOnlySphere) in the workload's band: (setup, rows callback)"""
    import mcsas_amd
    from helpers import PythonOnlySphere
    hm = PythonOnlySphere()
    hm.radius.setActiveRange(wl["band"])
    data = mcsas_amd.SASData(wl["q"], wl["I"], wl["sig"])
    comp = wl["st"].comp_exp
    return hm.setup(data), lambda pset: mcsas_amd.scatteringmodels.host_model_calc(hm, data, pset, comp, want_rows=True)[4]


@pytest.mark.parametrize("mode", ("workgroup", "pipeline", "host_rows"))
@pytest.mark.parametrize("nq", sorted(FC.FINAL_GEOMETRY))
def test_final_fit_against_exact(nq, mode):
    """The workgroup-window kernel, the pipeline and analyse_host_rows, cold on replayed streams: chisq, scaling and background of the
    returned sets inside the derived bounds of the exact fit against the rows of those sets (model_calc's; the caller's own for
    analyse_host_rows, whose chain sums exactly the rows it was given).  The history that bounds the running sum's roundings is the
    oracle's chain, whose final set the returned one must equal."""
    wl = FC.final_workload(nq)
    q, I, sg, fb, pb, sl, wv = wl["q"], wl["I"], wl["sig"], wl["find_bg"], wl["pos_bg"], wl["slots"], wl["waves"]
    n = FC.FINAL_N
    if mode == "host_rows":
        setup, rows_fn = _host_rows(wl)
        res = engine.analyse_host_rows(setup, q, I, sg, wl["st"], rows_fn, replay=wl["replay"])
    else:
        setup = wl["model"].setup()
        st = engine.Settings(**{**wl["st"].__dict__, "exec_mode": engine.EXEC_WORKGROUP if mode == "workgroup" else engine.EXEC_PIPELINE})
        res = engine.analyse(setup, q, I, sg, st, replay=wl["replay"])
    bad, worst = [], {}
    for r in range(FC.REPS):
        ref = wl["chains"][r]["ref"]
        print("%s nq %d chain %d: %d steps, %d moves (oracle %d), chisq %.17g (oracle %.17g)"
              % (mode, nq, r, res.num_iter[r], res.num_moves[r], ref.num_moves, res.chisq[r], ref.conval))
        assert res.num_iter[r] == FC.FINAL_STEPS and res.num_moves[r] == ref.num_moves
        assert np.array_equal(res.contribs[:, :, r], ref.rset)
        radii = res.contribs[:, 0, r]
        if mode == "host_rows":
            rows, gaps = rows_fn(np.ascontiguousarray(radii[:, None])), np.zeros((n, nq))
        else:
            rows, gaps = _device_rows(setup, q, radii, wl["st"].comp_exp)
        C = FC.ordered_sum(rows)
        M = np.maximum(FC.history_max(wl, r), C) + gaps.sum(axis=0)          # (the oracle's rows are off the device's by no more than these)
        eC = (n + 1) * U * C + (n - 1 + 2 * ref.num_moves) * U * M + gaps.sum(axis=0)
        x = F.exact_fit(I, sg, C, fb, pb)
        bd = F.chain_bounds(x, I, sg, C, fb, eC, sl, wv)
        name = "%s nq %d chain %d" % (mode, nq, r)
        _look(bad, worst, name, "chisq", res.chisq[r], bd["final"])
        _look(bad, worst, name, "scaling", res.scaling[r], bd["A"]); _look(bad, worst, name, "background", res.background[r], bd["b"])
    _report("%s nq %d" % (mode, nq), worst, bad)

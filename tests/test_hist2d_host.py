"""The joint histogram of two parameters without a device: parameter.Histogram2D.calc — the numpy form of mcsas_hip_histogram2d and
the product's path beyond 4096 contributions or cells — against exact values inside the bounds derived from the kernel's operation
order (tests/hist2d_exact.py); degraded emulations that must each fall outside those bounds; the ctypes record against the header;
every refusal of the entry point, made before a device is touched; and McSAS.histogram()'s host path with and without a configured
Histogram2D.  No assertion on a number has a tolerance that is not such a bound."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hist2d_exact as X
import hist_exact as H
import mcsas_amd
from helpers import PythonOnlyCoreShell
from mcsas_amd import _lib, engine
from mcsas_amd.parameter import FitParameter, Histogram, Histogram2D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcsas_hip.h")
CASES = {c["name"]: c for c in X.cases()}
OK, EINVAL, ENODEV = 0, -1, -2


def _report(what, worst, bad):
    for k, v in sorted(H.summarise(worst).items()):
        print("%s  %-8s  largest error / bound %.3g" % (what, k, v))
    assert not bad, "\n".join(bad[:40])


# ------------------------------------------------------------------------------------------------- Histogram2D.calc against exact values
@pytest.mark.parametrize("name", sorted(CASES))
def test_calc_and_emulation_inside_the_bounds(name):
    """Histogram2D.calc and the fp64 emulation of hist2d_body's order inside every bound, classes by equality; their bins and
    observabilities are the same bits (both are ordered sums)"""
    c = CASES[name]
    got, emu = X.calc_hists(c), X.emu(c)
    for what, hs in (("calc", got), ("emu", emu)):
        bad, worst = [], {}
        X.look_hists(bad, worst, c, hs)
        _report("%s %s" % (name, what), worst, bad)
    for h, (a, b) in enumerate(zip(got, emu)):
        for k in ("bins", "obs"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (name, h, k)


def test_the_cases_place_what_they_claim():
    """membership on the doubles themselves: edges, duplicates, the empty column, cells of one's own, one owner lane, nobody"""
    c = CASES["placed"]
    sp0, sp1, sp2 = c["specs"]
    x, y = c["contribs"][:, c["px"], 0], c["contribs"][:, c["py"], 0]
    cl = c["claims"]
    i, j = X.columns(sp0["edges_x"], x), X.columns(sp0["edges_y"], y)
    assert i[cl["first_x"]] == 0 and i[cl["inner_x"][0]] == cl["inner_x"][1] and i[cl["last_x"]] == len(sp0["edges_x"]) - 1
    assert j[cl["first_y"]] == 0 and j[cl["inner_y"][0]] == cl["inner_y"][1] and j[cl["last_y"]] == len(sp0["edges_y"]) - 1
    cell = X.cells_of(sp0, x, y)
    assert cell[cl["last_x"]] == -1 and cell[cl["last_y"]] == -1 and cell[cl["first_x"]] >= 0 and cell[cl["first_y"]] >= 0
    assert cell[cl["duplicates"][0]] == cell[cl["duplicates"][1]] >= 0
    m0, m2 = X.moments_mask(sp0, x, y), X.moments_mask(sp2, x, y)
    assert not m0[cl["first_x"]] and not m0[cl["last_x"]] and not m0[cl["first_y"]] and not m0[cl["last_y"]]
    assert not any(m2[cl[k]] for k in ("lower_x", "upper_x", "lower_y", "upper_y")) and m2.sum() > 2
    assert (X.columns(sp1["edges_x"], x) != 1).all() and (X.columns(sp1["edges_y"], y) != 1).all()      # the empty columns
    c = CASES["own_cells"]
    for r in range(c["R"]):
        cell = X.cells_of(c["specs"][0], c["contribs"][:, 0, r], c["contribs"][:, 1, r])
        assert len(set(cell)) == c["N"] and (cell >= 0).all()
        assert (X.cells_of(c["specs"][2], c["contribs"][:, 0, r], c["contribs"][:, 1, r]) == 0).all()
    c = CASES["congruent"]
    cell = X.cells_of(c["specs"][0], c["contribs"][:, 0, 0], c["contribs"][:, 1, 0])
    assert (cell >= 0).all() and (cell % 64 == 5).all() and len(set(cell)) < c["N"]
    c = CASES["nan_inf"]
    assert (X.cells_of(c["specs"][0], c["contribs"][:, 2, 0], c["contribs"][:, 0, 0]) == -1).all()
    ref = X.all_bounds(c)
    assert all(ref[0][r]["n_in"] == 0 for r in range(c["R"])) and all(q.v == 0 and q.e == 0 for q in ref[0][0]["moments"])
    assert all(isinstance(q, float) and q != q for q in ref[1][1]["moments"])                            # NaN goes on
    assert any(isinstance(q, float) and q == np.inf for q in ref[1][0]["obs"])
    c = CASES["cap"]
    assert ref is not None and X.all_bounds(c)[0][0]["counts"] == [c["N"]]


@pytest.mark.parametrize("mutate", X.MUTATIONS)
def test_a_degraded_emulation_falls_outside_the_bounds(mutate):
    """each of: the y axis' upper edge taken as <=, the axes' edges swapped, the observability over N, a cell summed in float32,
    the last contribution of a lane's share dropped (N = 65), the moments' mask not strict, the covariance from dx dx"""
    names = ["congruent"] if mutate == "share_dropped" else ["placed", "congruent", "own_cells"]
    bad = []
    for name in names:
        X.look_hists(bad, {}, CASES[name], X.emu(CASES[name], mutate))
    print("%s: %d values outside; first: %s" % (mutate, len(bad), bad[:1]))
    assert bad, mutate


# ------------------------------------------------------------------------------------------------- Histogram2D, the object
def _params():
    a = FitParameter("a", 1e-8, valueRange=(1e-10, 1e-6)); b = FitParameter("b", 10.0, valueRange=(0.5, 100.0))
    a.setActive(True); b.setActive(True)
    return a, b


def test_histogram2d_ranges_scales_edges_and_results():
    a, b = _params()
    h = Histogram2D(a, b, (1e-12, 5e-8), (200.0, 1.0), binCount=(5, 3), scaleX="lin", scaleY="nonsense", yweight="also nonsense")
    assert h.xrange == (1e-10, 5e-8) and h.yrange == (1.0, 100.0)                  # clipped into the value ranges, ordered
    assert h.scaleX == "lin" and h.scaleY == "log" and h.yweight == "vol"           # the fall-backs of Histogram
    a.setActiveRange((2e-9, 4e-8)); b.setActiveRange((2.0, 50.0))                   # autoFollow
    assert h.xrange == (2e-9, 4e-8) and h.yrange == (2.0, 50.0)
    fixed = Histogram2D(a, b, (3e-9, 3e-8), (3.0, 30.0), autoFollow=False)
    a.setActiveRange((2e-9, 5e-8))
    assert fixed.xrange == (3e-9, 3e-8) and fixed.binCount == (20, 20) and h.xrange == (2e-9, 5e-8)
    one_x, one_y = Histogram(a, 2e-9, 5e-8, binCount=5, xscale="lin"), Histogram(b, 2.0, 50.0, binCount=3, xscale="log")
    one_x._setXLowerEdge(); one_y._setXLowerEdge()
    spec = h.deviceSpec(0, 1)
    assert np.array_equal(spec["edges_x"], one_x.xLowerEdge) and np.array_equal(spec["edges_y"], one_y.xLowerEdge)
    assert (spec["lower_x"], spec["upper_x"], spec["lower_y"], spec["upper_y"], spec["yweight"]) == (2e-9, 5e-8, 2.0, 50.0, "vol")
    rs = np.random.RandomState(5)
    N, nrep = 40, 3
    contribs = np.stack([rs.uniform(2e-9, 5e-8, (N, nrep)), rs.uniform(2.0, 50.0, (N, nrep))], axis=1)
    f8 = rs.uniform(0.1, 1.0, (8, N, nrep))
    f8[4, :, 1] = np.inf                                                            # repetition 1: no finite limit anywhere
    h.calc(contribs, 0, 1, X.fractions_dict(f8))
    assert h.bins.full.shape == (5, 3, nrep) and h.bins.mean.shape == (5, 3) and h.observability.shape == (5, 3)
    assert np.array_equal(h.bins.mean, h.bins.full.mean(axis=2)) and np.array_equal(h.bins.std, h.bins.full.std(axis=2, ddof=1))
    best = np.where(np.isfinite(h.obs), h.obs, -np.inf).max(axis=2)
    assert np.array_equal(h.observability, np.where(np.isfinite(best), best, 0.0)) and (h.observability < np.inf).all()
    assert len(h.moments.fields) == 14 and h.moments.fields[:2] == h.moments.total and h.moments.fields[12:] == h.moments.correlation
    assert h.moments.total == (h.moments.full[0].mean(), h.moments.full[0].std(ddof=1))
    same = Histogram2D(a, b, h.xrange, h.yrange, binCount=(5, 3), scaleX="lin", autoFollow=False)
    same.setFromDevice(dict(bins=h.bins.full, obs=h.obs, moments=h.moments.full))
    assert np.array_equal(same.observability, h.observability) and same.moments.fields == h.moments.fields
    single = Histogram2D(a, b, h.xrange, h.yrange, binCount=(2, 2), autoFollow=False)
    single.calc(contribs[:, :, :1], 0, 1, X.fractions_dict(f8[:, :, :1]))
    assert (single.bins.std == 0).all() and single.moments.total[1] == 0.0          # one repetition: ddof 0


# ------------------------------------------------------------------------------------------------- the C ABI
def test_histogram2d_struct_layout_matches_header(tmp_path):
    names = [n for n, _ in _lib.Histogram2dSpec._fields_]
    src = tmp_path / "sz2d.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(mcsas_histogram2d_spec));\n%s\n'
                   'printf("\\n"); return 0;}\n' % (HEADER, "\n".join('printf(" %%zu", offsetof(mcsas_histogram2d_spec, %s));' % n for n in names)))
    exe = tmp_path / "sz2d"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(_lib.Histogram2dSpec)
    assert out[1:] == [getattr(_lib.Histogram2dSpec, n).offset for n in names]


def _record(**kw):
    """a valid record (2 x 3 cells over columns 0 and 1) with the given fields replaced; the edges stay alive with it"""
    ex, ey = np.array([0.0, 1.0, 2.0]), np.array([0.0, 1.0, 1.0, 3.0])             # (equal neighbours: allowed)
    d = dict(param_x=0, param_y=1, weighting=0, n_bin_x=2, n_bin_y=3, reserved=0, lower_x=0.0, upper_x=2.0, lower_y=0.0, upper_y=3.0,
             edges_x=ex, edges_y=ey)
    d.update(kw)
    keep = [d["edges_x"], d["edges_y"]]
    rec = _lib.Histogram2dSpec()
    for k, v in d.items():
        setattr(rec, k, (None if v is None else _lib.as_dp(v)) if k.startswith("edges") else v)
    return rec, keep


def _call(records, N=4, P=2, nrep=2, n_hist=None, contribs=True, fractions=True, specs=True, out=True):
    lib = _lib.load()
    arr = (_lib.Histogram2dSpec * max(len(records), 1))(*[r for r, _ in records])
    c, f, o = np.ones((max(N, 1), max(P, 1), max(nrep, 1))), np.ones((8, max(N, 1), max(nrep, 1))), np.zeros(32768)
    rc = lib.mcsas_hip_histogram2d(N, P, nrep, _lib.as_dp(c) if contribs else None, _lib.as_dp(f) if fractions else None,
                                   len(records) if n_hist is None else n_hist, arr if specs else None, _lib.as_dp(o) if out else None, -1)
    return rc, lib.mcsas_hip_last_error().decode()


BAD_RECORDS = dict(
    reserved=dict(reserved=1), weighting_low=dict(weighting=-1), weighting_high=dict(weighting=4), param_x_high=dict(param_x=2),
    param_y_low=dict(param_y=-1), bins_negative=dict(n_bin_x=-1), cells_4097=dict(n_bin_x=4097, n_bin_y=1, edges_x=np.arange(4098.0), edges_y=np.arange(2.0)),
    cells_65x64=dict(n_bin_x=65, n_bin_y=64, edges_x=np.arange(66.0), edges_y=np.arange(65.0)), edges_x_null=dict(edges_x=None),
    edges_y_null=dict(edges_y=None), edges_nan=dict(edges_x=np.array([0.0, np.nan, 2.0])), edges_inf=dict(edges_y=np.array([0.0, 1.0, 2.0, np.inf])),
    edges_fall=dict(edges_x=np.array([0.0, 2.0, 1.0])), edges_y_fall=dict(edges_y=np.array([0.0, 1.0, 0.5, 3.0])))


@pytest.mark.parametrize("name", sorted(BAD_RECORDS))
def test_a_bad_record_is_refused_by_its_index_before_a_device_is_touched(name):
    rc, msg = _call([_record(), _record(**BAD_RECORDS[name])])
    assert rc == EINVAL and "histogram 1" in msg, (rc, msg)


def test_bad_sizes_and_tables_are_refused_and_good_calls_go_on():
    good = [_record(), _record(n_bin_x=0, edges_x=None)]                            # (an axis without bins does not read its edges)
    for kw in (dict(n_hist=-1), dict(contribs=False), dict(fractions=False), dict(specs=False), dict(out=False), dict(N=0), dict(N=4097),
               dict(P=0), dict(nrep=0)):
        rc, msg = _call(good, **kw)
        assert rc == EINVAL and "histogram2d" in msg, (kw, rc, msg)
    assert _call(good, n_hist=0)[0] == OK
    assert _call([], n_hist=0, contribs=False, fractions=False, specs=False, out=False)[0] == OK
    have = _lib.load().mcsas_hip_device_count() > 0
    for recs in (good, [_record(n_bin_x=64, n_bin_y=64, edges_x=np.arange(65.0), edges_y=np.arange(65.0))]):
        rc, msg = _call(recs, N=4096)
        assert rc == (OK if have else ENODEV), (rc, msg)
    if not have:
        with pytest.raises(_lib.McSASHipError) as e:
            engine.histogram2d_device(np.ones((4, 2, 2)), np.ones((8, 4, 2)), [dict(param_x=0, param_y=1, yweight="vol", edges_x=[0.0, 2.0],
                                                                                    edges_y=[0.0, 2.0], lower_x=0, upper_x=2, lower_y=0, upper_y=2)])
        assert e.value.code == ENODEV
    assert engine.histogram2d_device(np.ones((4, 2, 2)), np.ones((8, 4, 2)), []) == []
    assert engine.HISTOGRAM2D_MAX_CELLS == 4096 and mcsas_amd.Histogram2D is Histogram2D


# ------------------------------------------------------------------------------------------------- McSAS.histogram(), the host path
def _host_algo(n2d):
    """a Python-only model (two active parameters) with one 1-D histogram per parameter, fixed arrays for _histogram_tail, and
    n2d joint histograms of more than 4096 cells: they run in numpy, no device is asked"""
    m = PythonOnlyCoreShell()
    m.radius.setActiveRange((2e-9, 1e-7)); m.t.setActiveRange((5e-10, 2e-8))
    m.radius.histograms().append(Histogram(m.radius, 2e-9, 1e-7, binCount=9, xscale="log", yweight="vol"))
    m.t.histograms().append(Histogram(m.t, 5e-10, 2e-8, binCount=7, xscale="lin", yweight="num"))
    algo = mcsas_amd.McSAS.factory()()
    algo.model = m
    rs = np.random.RandomState(9)
    N, nrep = 33, 3
    contribs = np.stack([rs.uniform(2e-9, 1e-7, (N, nrep)), rs.uniform(5e-10, 2e-8, (N, nrep))], axis=1)
    arrays = dict(scalingFactors=np.vstack([rs.uniform(1e-3, 2e-3, nrep), np.zeros(nrep)]), vsets=rs.uniform(1e-24, 1e-21, (N, nrep)),
                  wsets=rs.uniform(1e14, 1e16, (N, nrep)), ssets=rs.uniform(1e-16, 1e-14, (N, nrep)), mv=rs.uniform(1e-4, 1e-2, (N, nrep)))
    algo.result = [dict(contribs=contribs)]
    for k in range(n2d):
        algo.histograms2d.append(Histogram2D(m.radius, m.t, (2e-9, 1e-7), (5e-10, 2e-8), binCount=(65, 64), yweight=("vol", "int")[k % 2]))
    return algo, m, contribs, arrays


def _snapshot(algo, m):
    out = dict(sc=algo.result[0]["scalingFactors"].copy())
    for w, (f, lim) in algo.fractions.items():
        out["f_" + w], out["l_" + w] = f.copy(), lim.copy()
    for p in (m.radius, m.t):
        for h in p.histograms():
            out.update({p.name() + "_bins": h.bins.full.copy(), p.name() + "_cdf": h.cdf.full.copy(), p.name() + "_obs": h.observability.copy(),
                        p.name() + "_mom": np.array(h.moments.fields)})
    return out


def test_histogram_host_path_is_unchanged_by_the_joint_histograms(monkeypatch):
    """_histogram_tail with an empty histograms2d: nothing new runs (neither engine.histogram2d_device nor Histogram2D.calc is
    entered) and result, fractions and the 1-D histograms are what the restated lines of the tail and Histogram.calc give; with
    joint histograms configured the same arrays, bit for bit, and the joint ones filled by Histogram2D.calc"""
    def never(*a, **k):
        raise AssertionError("a joint histogram ran with none configured")
    algo, m, contribs, arr = _host_algo(0)
    assert algo.histograms2d == []
    with monkeypatch.context() as mp:
        mp.setattr(engine, "histogram2d_device", never); mp.setattr(Histogram2D, "calc", never)
        algo._histogram_tail(contribs, **arr)
    plain = _snapshot(algo, m)
    # the tail's own lines (mcsas.py:561-604) restated, and fresh 1-D histograms on them
    A, v, w, s, mv = arr["scalingFactors"][0], arr["vsets"], arr["wsets"], arr["ssets"], arr["mv"]
    vf = w * A[None, :] / v; nf = vf / v; qf = vf * v; sf = nf * s; mn = mv / v; mq = mn * mv * mv; ms = mn * s
    for f, lim in ((nf, mn), (qf, mq), (sf, ms)):
        tot = np.cumsum(f, axis=0)[-1]
        f /= tot; lim /= tot
    want = dict(vol=(vf, mv), num=(nf, mn), int=(qf, mq), surf=(sf, ms))
    for k in want:
        assert np.array_equal(plain["f_" + k], want[k][0]) and np.array_equal(plain["l_" + k], want[k][1]), k
    fresh = Histogram(m.radius, 2e-9, 1e-7, binCount=9, xscale="log", yweight="vol")
    fresh.calc(contribs, 0, want)
    assert np.array_equal(plain["radius_bins"], fresh.bins.full) and np.array_equal(plain["radius_mom"], np.array(fresh.moments.fields))
    # with two joint histograms (65 x 64 cells: beyond the device call, so they run here)
    algo2, m2, contribs2, arr2 = _host_algo(2)
    with monkeypatch.context() as mp:
        mp.setattr(engine, "histogram2d_device", never)
        algo2._histogram_tail(contribs2, **arr2)
    both = _snapshot(algo2, m2)
    assert sorted(both) == sorted(plain)
    for k in plain:
        assert np.array_equal(plain[k], both[k], equal_nan=True), k
    for h, wname in zip(algo2.histograms2d, ("vol", "int")):
        assert h.bins.full.shape == (65, 64, 3) and h.observability.shape == (65, 64)
        direct = Histogram2D(m2.radius, m2.t, h.xrange, h.yrange, binCount=(65, 64), yweight=wname, autoFollow=False)
        direct.calc(contribs2, 0, 1, algo2.fractions)
        assert np.array_equal(h.bins.full, direct.bins.full) and h.moments.fields == direct.moments.fields
        assert (np.count_nonzero(h.bins.full, axis=(0, 1)) > 0).all()


def test_a_joint_histogram_of_an_inactive_parameter_is_refused_by_name():
    algo, m, contribs, arr = _host_algo(0)
    m.t.setActive(False)
    algo.histograms2d.append(Histogram2D(m.radius, m.t, (2e-9, 1e-7), (5e-10, 2e-8), binCount=(65, 64)))
    with pytest.raises(ValueError, match="'t'"):
        algo._histogram_tail(contribs[:, :1, :], **arr)

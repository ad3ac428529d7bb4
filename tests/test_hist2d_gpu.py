"""The joint histogram of two parameters on the device (csrc/hist2d_kernel.h hist2d_body through engine.histogram2d_device) against
exact values, each inside the bound derived for it from the kernel's operation order (tests/hist2d_exact.py; the same cases and
bounds hold parameter.Histogram2D.calc and the emulation in test_hist2d_host.py, so a device value outside a bound they keep is the
kernel's).  No assertion here has a tolerance that is not such a bound; membership, empty cells, the NaN -> 0 of a cell, the 0 of an
empty selection and where NaN and inf stand are compared by equality.

  1. every case (N 1, 63, 64, 65, 130, 4096; cells 1 x 1 ... 64 x 64 and 0 x 5; R 1 and 3; P 2 and 3; three histograms a call):
     inside the bounds; the bits of Histogram2D.calc for bins and observability; the transposed bits with x and y exchanged; the
     same bits from a second call;
  2. the 1-D anchor: a built-in two-parameter case through engine.histogram_device, its fractions fed back with one y column
     that holds every value: bins, observability, total, mean and variance are the 1-D kernel's bit for bit;
  3. the front end: McSAS.calc() on cylinders (radius, length) with a replayed short chain and run_series(batch=True)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hist2d_exact as X
import hist_exact as H
import mcsas_amd
from exact import gamma
from helpers import make_models
from mcsas_amd import engine

CASES = {c["name"]: c for c in X.cases()}
_FIRST = {}


def _device(c, specs=None):
    return engine.histogram2d_device(c["contribs"], c["frac8"], c["specs"] if specs is None else specs)


def first_call(name):
    if name not in _FIRST:
        _FIRST[name] = _device(CASES[name])
    return _FIRST[name]


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _report(what, worst, bad):
    for k, v in sorted(H.summarise(worst).items()):
        print("%s  %-8s  largest error / bound %.3g" % (what, k, v))
    assert not bad, "\n".join(bad[:40])


# ------------------------------------------------------------------------------------------------- 1. the cases
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_inside_the_bounds(name):
    bad, worst = [], {}
    X.look_hists(bad, worst, CASES[name], first_call(name))
    _report(name, worst, bad)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_bins_are_histogram2d_calc_bit_for_bit(name):
    """both are ordered sums over a cell's members: the same bits; the moments are held by the bounds"""
    for h, (dev, host) in enumerate(zip(first_call(name), X.calc_hists(CASES[name]))):
        for k in ("bins", "obs"):
            assert _eq(dev[k], host[k]), (name, h, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_exchanging_x_and_y_transposes_the_result(name):
    c = CASES[name]
    for h, (a, b) in enumerate(zip(first_call(name), _device(c, [X.swapped(sp) for sp in c["specs"]]))):
        for k in ("bins", "obs"):
            assert _eq(b[k], a[k].transpose(1, 0, 2)), (name, h, k)
        assert _eq(b["moments"], a["moments"][list(X.SWAP_ROWS)]), (name, h, a["moments"], b["moments"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_second_call_gives_the_same_bits(name):
    """(the staging and device blocks come back from the cache: nothing of the call before may show)"""
    a = first_call(name)
    other = sorted(CASES)[(sorted(CASES).index(name) + 1) % len(CASES)]
    first_call(other)                                           # another shape in between, into the same cached blocks
    b = _device(CASES[name])
    for h, (x, y) in enumerate(zip(a, b)):
        for k in ("bins", "obs", "moments"):
            assert _eq(x[k], y[k]), (name, h, k)


def test_fractions_as_mcsas_holds_them():
    c = CASES["placed"]
    got = engine.histogram2d_device(c["contribs"], X.fractions_dict(c["frac8"]), c["specs"])
    for x, y in zip(first_call("placed"), got):
        assert all(_eq(x[k], y[k]) for k in ("bins", "obs", "moments"))


# ------------------------------------------------------------------------------------------------- 2. the 1-D anchor
def test_one_y_column_gives_the_one_dimensional_kernels_bits():
    """coreshell_64 of hist_exact.builtin_cases() (64 contributions, 3 repetitions; volume, number and — all zero for this model —
    surface weighting) through engine.histogram_device; its fractions with n_bin_y = 1, y edges and a y range that hold every
    value: bins[:, 0, :], obs[:, 0, :] and total, mean x, variance x are the 1-D arrays bit for bit"""
    c = [k for k in H.builtin_cases() if k["name"] == "coreshell_64"][0]
    setup = make_models(c["builtin"], H.PAR_LO[:c["P"]], H.PAR_HI[:c["P"]])[0].setup()

    def rows_fn(pset):
        _, v, w, s, rows = engine.model_calc(setup, c["q"], pset, H.C_EXP, want_rows=True)
        return rows, v, w, s
    H.finish(c, rows_fn)
    sc, fractions, one = engine.histogram_device(model=setup, q=c["q"], intensity=c["I"], sigma=c["sigma"], contribs=c["contribs"],
                                                 comp_exp=H.C_EXP, specs=c["specs"], find_background=c["find_bg"])
    assert (c["contribs"] > 0.0).all() and (c["contribs"] < 1.0).all()
    specs = [dict(param_x=sp["param_index"], param_y=1 - sp["param_index"], yweight=sp["yweight"], edges_x=sp["edges"], edges_y=[0.0, 1.0],
                  lower_x=sp["lower"], upper_x=sp["upper"], lower_y=0.0, upper_y=1.0) for sp in c["specs"]]
    two = engine.histogram2d_device(c["contribs"], fractions, specs)
    assert len(two) == len(one) == 3
    for h, (a, b) in enumerate(zip(one, two)):
        assert b["bins"].shape[1] == 1
        assert _eq(b["bins"][:, 0, :], a["bins"]) and _eq(b["obs"][:, 0, :], a["obs"]), h
        assert _eq(b["moments"][[0, 1, 3]], a["moments"][:3]), (h, a["moments"][:3], b["moments"][[0, 1, 3]])
    assert (one[0]["bins"] > 0).any() and np.isfinite(one[0]["moments"][:3]).all()


# ------------------------------------------------------------------------------------------------- 3. the front end
N_CONTRIB, N_REPS, MAX_ITER = 40, 3, 100
LO, HI = (2e-9, 5e-9), (4e-8, 2e-7)                            # radius, length


def _front_end():
    from bench import synthetic_data
    m, _ = make_models("cyl_length", [LO[0], LO[1]], [HI[0], HI[1]], intDiv=20.)
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, LO[0], HI[0], binCount=6, xscale="log", yweight="vol"))
    algo = mcsas_amd.McSAS(seed=3, execMode=engine.EXEC_WAVE)        # (the mode run_series(batch=True) runs: the same chains)
    algo.numContribs.setValue(N_CONTRIB); algo.numReps.setValue(N_REPS); algo.maxIterations.setValue(MAX_ITER)
    algo.convergenceCriterion.setValue(1e-9); algo.maxRetries.setValue(0); algo.showIncomplete.setValue(True)
    algo.model = m
    algo.histograms2d.append(mcsas_amd.Histogram2D(m.radius, m.length, (LO[0], HI[0]), (LO[1], HI[1]), binCount=(6, 5), yweight="vol"))
    datasets, replays = [], []
    for k, nq in enumerate((64, 48)):
        q, I, sig = synthetic_data(nq)
        datasets.append(mcsas_amd.SASData(q, I * (1.0 + 0.1 * k), sig))
        replays.append(np.random.RandomState(20 + k).uniform(size=(N_REPS, 8 * (2 * N_CONTRIB + 4 * MAX_ITER))))
    return algo, m, datasets, replays


def _cell_sum_bound(member_masks, f):
    """sum over the cells of gamma(m - 1) S: what the ordered sums of a histogram's cells are off by, in all (m members, S their sum)"""
    return sum(gamma(max(int(mask.sum()) - 1, 0)) * math.fsum(f[mask]) for mask in member_masks)


def test_mcsas_calc_fills_the_joint_histogram_and_the_series_carries_it():
    algo, m, datasets, replays = _front_end()
    h2, h1 = algo.histograms2d[0], m.radius.histograms()[0]
    alone = []
    for data, rep in zip(datasets, replays):
        algo.data = data
        algo.calc(replay=rep)
        assert len(algo.result) == 1
        contribs, (f, lim) = algo.result[0]["contribs"], algo.fractions["vol"]
        assert h2.bins.full.shape == (6, 5, N_REPS) and h2.observability.shape == (6, 5)
        sp = h2.deviceSpec(0, 1)
        c = dict(name="cylinders", N=N_CONTRIB, R=N_REPS, contribs=contribs, frac8=engine.fractions_array(algo.fractions), specs=[sp])
        bad, worst = [], {}
        ref = X.look_hists(bad, worst, c, [dict(bins=h2.bins.full, obs=h2.obs, moments=h2.moments.full)])
        _report("cylinders", worst, bad)
        for r in range(N_REPS):
            x, y = contribs[:, 0, r], contribs[:, 1, r]
            cell = X.cells_of(sp, x, y)
            col = H.bin_members(x, h1.xLowerEdge)
            # the same contributions are in a cell and in a bin (the lengths all lie inside the y edges), so the two histograms sum
            # the same fractions; each is off by no more than its own ordered sums
            assert np.array_equal(cell >= 0, np.any(col, axis=0)) and (cell >= 0).sum() > 1
            bound = _cell_sum_bound([cell == k for k in range(30)], f[:, r]) + _cell_sum_bound(col, f[:, r])
            d = abs(math.fsum(h2.bins.full[:, :, r].ravel()) - math.fsum(h1.bins.full[:, r]))
            print("repetition %d: 2-D and 1-D sums differ by %.3g, bound %.3g" % (r, d, bound))
            assert d <= bound
            rho, rr = h2.moments.full[6, r], ref[0][r]["moments"][6]
            assert -1.0 <= float(rr.v) <= 1.0 and -1.0 - rr.e <= rho <= 1.0 + rr.e, (rho, rr.e)
        alone.append(dict(bins=h2.bins.full.copy(), obs=h2.obs.copy(), fields=h2.moments.fields, one=h1.moments.fields))
    results, series = mcsas_amd.run_series(algo, datasets, keys=["a", "b"], replays=replays, batch=True)
    uid = ("radius", "length") + tuple(h2.xrange) + tuple(h2.yrange) + ("vol",)
    assert uid in series and len(series) == 2 and all(r is not None for r in results)
    assert [k for k, _ in series[uid]] == ["a", "b"]
    for i, (key, fields) in enumerate(series[uid]):
        assert fields == alone[i]["fields"], (i, fields, alone[i]["fields"])
    assert [fl for _, fl in series[("radius", LO[0], HI[0], "vol")]] == [a["one"] for a in alone]
    assert _eq(h2.bins.full, alone[1]["bins"]) and _eq(h2.obs, alone[1]["obs"])      # (the object holds the last data set's arrays)
    m.length.setActive(False)
    with pytest.raises(ValueError, match="'length'"):
        algo._histograms2d_calc()

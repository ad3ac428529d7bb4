"""What McSAS.histogram() reads off a set of contributions on the device — visibility limits, fractions, bins, observability,
cumulative distribution, moments (csrc/hist_kernels.h hist_obs_body, hist_fractions_body, hist_bins_body) — engine.observability and
the re-binning (csrc/host_calls.hip rebin_kernel) against exact values, each inside the bound derived for it from the kernel's
operation order (tests/hist_exact.py, tests/exact.py; the same cases and bounds hold the numpy emulations in
test_hist_exact_host.py, so a device value outside a bound its emulation keeps is the kernel's).  No assertion here has a tolerance
that is not such a bound; which contribution is in which bin, which bins are kept and where NaN, +-inf and an exact 0 stand are
compared by equality.

  1. engine.histogram_device_rows on rows, volumes, weights and surfaces of the test's own choosing (exact zeros, products with the
     scale that underflow, a zero volume, zero surfaces), the scale taken from the call's own output;
  2. for the built-in models' cases engine.histogram_device, engine.histogram_device_batch (all of them in one batch, in both
     orders) and rounds of one repetition: the same bits, so the bounds hold for every entry point;
  3. engine.observability on the built-in cases;
  4. engine.rebin.

Without a device torch can reach, 1. skips (its only way in is a torch tensor); the built-in cases are then held to their bounds
through engine.histogram_device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

try:                                # ahead of the library's first load: one HIP runtime in the process (engine._one_hip_runtime)
    import torch
    NO_TORCH = None if torch.cuda.is_available() else "torch cannot reach the device"
except Exception as e:              # noqa: BLE001
    NO_TORCH = "torch cannot reach the device: %s" % e

import hist_exact as H
from mcsas_amd import engine
from helpers import make_models

HIST = {c["name"]: c for c in H.hist_cases()}
BUILTIN = [c["name"] for c in H.builtin_cases()]
_DONE = {}


def _setup(c):
    tag = c["builtin"] or "sphcs"                     # (explicit rows: any model of two active parameters names the sizes)
    return make_models(tag, H.PAR_LO[:c["P"]], H.PAR_HI[:c["P"]])[0].setup()


def ready(name):
    """the case with its rows (a built-in case: model_calc's), its setup, and what the entry points gave for it so far"""
    if name not in _DONE:
        c = HIST[name]
        setup = _setup(c)
        if c["builtin"]:
            def rows_fn(pset):
                _, v, w, s, rows = engine.model_calc(setup, c["q"], pset, H.C_EXP, want_rows=True)
                return rows, v, w, s
            H.finish(c, rows_fn)
        else:
            H.host_case(c)
        _DONE[name] = dict(c=c, setup=setup)
    return _DONE[name]


def handed_rows(c):
    """row_fn that hands the case's arrays over, a round at a time in the order the library asks (row rl N + i = contribution i of
    repetition r0 + rl), as torch tensors made from numpy arrays; the parameter sets it is shown are the case's"""
    N, P, nrep, nq = c["N"], c["P"], c["R"], c["nq"]
    rows = c["rows"].reshape(nrep * N, nq)
    v, w, s = (np.ascontiguousarray(c[k].T).reshape(-1) for k in "vws")
    pset_all = np.ascontiguousarray(c["contribs"].transpose(2, 0, 1)).reshape(nrep * N, P)
    pos = [0]

    def fn(pset):
        a, n = pos[0], len(pset)
        pos[0] += n
        assert np.array_equal(pset.cpu().numpy(), pset_all[a:a + n])
        return tuple(torch.from_numpy(np.ascontiguousarray(x[a:a + n])) for x in (rows, v, w, s))
    return fn


def device_rows(name, capacity=None):
    e = ready(name)
    c = e["c"]
    return engine.histogram_device_rows(e["setup"], c["q"], c["I"], c["sigma"], c["contribs"], c["specs"], handed_rows(c),
                                        find_background=c["find_bg"], capacity=capacity)


def _report(what, worst, bad):
    for k, v in sorted(H.summarise(worst).items()):
        print("%s  %-8s  largest error / bound %.3g" % (what, k, v))
    assert not bad, "\n".join(bad[:40])


def _same(a, b, what):
    (sc, fr, hs), (rsc, rfr, rhs) = a, b
    eq = lambda x, y: x.shape == y.shape and np.array_equal(x, y, equal_nan=True)
    assert eq(sc, rsc), (what, "scaling")
    for k in H.WEIGHTS:
        assert eq(fr[k][0], rfr[k][0]) and eq(fr[k][1], rfr[k][1]), (what, "fractions", k)
    assert len(hs) == len(rhs)
    for h, (x, y) in enumerate(zip(hs, rhs)):
        for k in ("bins", "obs", "cdf", "moments"):
            assert eq(x[k], y[k]), (what, "histogram", h, k)


# ------------------------------------------------------------------------------------------------- 1. rows of the test's choosing
@pytest.mark.parametrize("name", sorted(HIST))
def test_device_rows_against_exact(name):
    """fractions, limits, bins, observability, CDF and moments of every case inside their bounds at the call's own scale; specials
    and exact zeros where the exact reference has them"""
    if NO_TORCH:
        pytest.skip(NO_TORCH)
    got = device_rows(name)
    ready(name)["rows_result"] = got
    A = got[0][0]
    assert np.isfinite(A).all() and (A > 0).all() and (A < 0.5).all(), A
    bad, worst = [], {}
    H.look_triple(bad, worst, HIST[name], got)
    _report(name, worst, bad)


# ------------------------------------------------------------------------------------------------- 2. the other entry points
def _item(name):
    e = ready(name)
    c = e["c"]
    return dict(model=e["setup"], q=c["q"], intensity=c["I"], sigma=c["sigma"], contribs=c["contribs"], comp_exp=H.C_EXP, specs=c["specs"],
                find_background=c["find_bg"])


@pytest.mark.parametrize("name", BUILTIN)
def test_histogram_device_against_exact_and_device_rows(name):
    """engine.histogram_device of a built-in case inside the bounds, and the same bits as histogram_device_rows on model_calc's
    rows of it, in one round and in rounds of one repetition"""
    it = _item(name)
    got = engine.histogram_device(**it)
    ready(name)["device_result"] = got
    bad, worst = [], {}
    H.look_triple(bad, worst, HIST[name], got)
    _report(name, worst, bad)
    if not NO_TORCH:
        _same(device_rows(name), got, (name, "one round"))
        _same(device_rows(name, capacity=HIST[name]["N"]), got, (name, "a repetition a round"))


@pytest.mark.parametrize("order", (1, -1))
def test_batch_gives_the_same_bits(order):
    """all built-in cases in one batch — different N, q count and histogram count share the launches, blocks beyond a set's own
    extent return early — in both orders: engine.histogram_device's bits"""
    names = BUILTIN[::order]
    got = engine.histogram_device_batch([_item(n) for n in names])
    for n, g in zip(names, got):
        ref = ready(n).get("device_result") or engine.histogram_device(**_item(n))
        _same(g, ref, (n, order))


# ------------------------------------------------------------------------------------------------- 3. engine.observability
@pytest.mark.parametrize("name", BUILTIN)
def test_observability_against_exact(name):
    """observability_kernel evaluates the model itself; its minimum against the exact one over model_calc's rows of the same sets,
    with the volume fractions as handed in"""
    e = ready(name)
    c = e["c"]
    A = (ready(name).get("device_result") or engine.histogram_device(**_item(name)))[0][0]
    vf = c["w"] * A[None, :] / c["v"]
    got = engine.observability(e["setup"], c["q"], c["sigma"], c["contribs"], A, vf, H.C_EXP)
    bad, worst = [], {}
    for r in range(c["R"]):
        for i in range(c["N"]):
            H.look(bad, worst, name, "limit [%d, %d]" % (i, r), got[i, r], H.obs_bound(c["sigma"], c["rows"][r, i], vf[i, r], A[r]))
    _report(name, worst, bad)


# ------------------------------------------------------------------------------------------------- 4. engine.rebin
@pytest.mark.parametrize("c", H.rebin_cases(), ids=lambda c: c["name"])
def test_rebin_against_exact(c):
    """the number of bins and which are kept, single-point bins bit for bit, x, f and fu inside their bounds, NaN uncertainties
    where expected"""
    ref = H.rebin_bounds(c["x"], c["f"], c["fu"], c["n_bin"])
    bad, worst = [], {}
    H.look_rebin(bad, worst, c["name"], engine.rebin(c["x"], c["f"], c["fu"], c["n_bin"]), ref)
    _report(c["name"], worst, bad)

"""The partial intensities of histogram ranges and bins without a device (tests/hist_partial_exact.py):
  - parameter.partial_intensities, the numpy form of csrc/hist_partial_kernel.h, against exact rational sums, every value inside
    the bound derived from the operation count (m - 1 additions and one product: gamma(m), the rows being non-negative);
  - membership by equality: a value on an edge, on lower, on upper, a NaN;
  - the emulation of the kernel's loop gives the numpy form's bits, and each degradation of it leaves them on at least one case;
  - every refusal of mcsas_hip_histogram_partial and mcsas_hip_histogram_partial_device_rows, asked of the library before a device
    is selected: MCSAS_EINVAL with its own sentence naming the histogram; the plain call's refusals come through unchanged;
  - the Python layers: Histogram(partialIntensity=...), the `partial` argument of the engine calls and the layout they unpack."""
import ctypes as C

import numpy as np
import pytest

import hist_exact as H
import hist_partial_exact as X
from mcsas_amd import _lib, engine
from mcsas_amd.parameter import FitParameter, Histogram, partial_intensities
from helpers import make_models

CASES = {c["name"]: c for c in X.cases()}
OK, EINVAL, ENODEV = 0, -1, -2
_A = {}


def ready(name):
    c = X.host_case(CASES[name])
    if name not in _A:
        _A[name] = H.emu_scaling(c)
    return c, _A[name]


# ------------------------------------------------------------------------------------------------- the numpy form
@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_form_inside_the_exact_bounds(name):
    c, A = ready(name)
    assert np.isfinite(A).all() and (A > 0).all()
    got = X.numpy_partial(c, A)
    ref, counts = X.exact_partial(c, A)
    bad, worst = [], {}
    X.look_partial(bad, worst, c, got, ref)
    for k, v in sorted(H.summarise(worst).items()):
        print("%s  %-8s  largest error / bound %.3g" % (name, k, v))
    assert not bad, "\n".join(bad[:40])
    for h, sp, w in X.wanted(c):                              # shapes, and A * 0.0 where nobody is selected
        rng, bins = got[h]
        assert rng.shape == (c["nq"], c["R"]) and (bins is None) == (w != 2)
        n_in, n_bin = counts[h]
        for r in range(c["R"]):
            if n_in[r] == 0:
                assert not rng[:, r].any()
            if w == 2:
                assert bins.shape == (X.n_bins(sp), c["nq"], c["R"])
                assert not bins[n_bin[:, r] == 0, :, r].any()


def test_membership_is_the_moments_and_the_bins_rule():
    """on the first edge: in bin 0; on an inner edge: in the bin that begins there; on the last edge: in no bin; on lower, on
    upper: outside the range; NaN: nowhere; a range holding nobody; a bin holding everybody — on single rows of ones, so that a
    curve counts the members"""
    c, _ = ready("placed")
    cl = c["claims"]
    e = c["specs"][0]["edges"]
    x = c["contribs"][:, 0, 0]
    ones = np.ones((c["N"], 2))
    rng, bins = partial_intensities(ones, x, 1.0, e[0], e[-1], e, True)
    members = H.bin_members(x, e)
    assert np.array_equal(bins[:, 0], [m.sum() for m in members]) and rng[0] == H.moments_mask(x, e[0], e[-1]).sum()
    h, i, r, b = cl["first_edge"]
    assert x[i] == e[0] and members[0][i]
    h, i, r, b = cl["inner_edge"]
    assert x[i] == e[b] and members[b][i] and not members[b - 1][i]
    h, i, r = cl["last_edge"]
    assert x[i] == e[-1] and not any(m[i] for m in members)
    nan_i = cl["nan"][0]
    assert np.isnan(x[nan_i]) and not any(m[nan_i] for m in members)
    one = lambda i: partial_intensities(ones[i:i + 1], x[i:i + 1], 1.0, *H.NARROW)[0][0]
    assert one(cl["lower"][1]) == 0.0 and one(cl["upper"][1]) == 0.0 and one(nan_i) == 0.0     # strict on both sides
    assert x[cl["lower"][1]] == H.NARROW[0] and x[cl["upper"][1]] == H.NARROW[1]
    h, r = cl["nobody"]
    assert not X.numpy_partial(c, np.ones(3))[h][0][:, r].any()                                 # the narrow range, repetition 1
    c64, A = ready("n64")
    got = X.numpy_partial(c64, A)
    assert X.same_bits(got[0][1][0], got[0][0])                                                # one bin holding everybody = the range


def test_empty_selection_and_non_finite_rows():
    rows = np.array([[1.0, np.inf, 2.0], [3.0, 1.0, np.nan]])
    rng, bins = partial_intensities(rows, np.array([1.0, 2.0]), 0.5, 0.0, 3.0, [0.0, 1.5, 3.0], True)
    assert np.array_equal(rng, [2.0, np.inf, np.nan], equal_nan=True)
    assert np.array_equal(bins, [[0.5, np.inf, 1.0], [1.5, 0.5, np.nan]], equal_nan=True)
    rng, bins = partial_intensities(rows, np.array([1.0, 2.0]), -2.0, 5.0, 6.0, [5.0, 6.0], True)
    assert np.array_equal(rng, -2.0 * np.zeros(3)) and np.signbit(rng).all() and np.signbit(bins).all()   # A * 0.0
    rng, bins = partial_intensities(np.zeros((0, 3)), np.zeros(0), 2.0, 0.0, 1.0)
    assert np.array_equal(rng, np.zeros(3)) and bins is None


# ------------------------------------------------------------------------------------------------- emulation and degradations
@pytest.mark.parametrize("name", sorted(set(CASES) - {"n4096"}))
def test_the_kernel_loop_emulation_gives_the_numpy_forms_bits(name):
    c, A = ready(name)
    assert not X.differing(X.emu_partial(c, A), X.numpy_partial(c, A))


DEGRADED_ON = dict(range_le="placed", upper_le="placed", scale_per_term="n63", acc32="n63", q_drop="n64", reverse="n63")


@pytest.mark.parametrize("mutate", X.MUTATIONS)
def test_a_degraded_emulation_leaves_the_numpy_forms_bits(mutate):
    c, A = ready(DEGRADED_ON[mutate])
    assert X.differing(X.emu_partial(c, A, mutate), X.numpy_partial(c, A)), mutate


# ------------------------------------------------------------------------------------------------- refusals, no device
def _call(want=(2, 1), partial=True, specs=None, N=5, device_rows=False, plain=False, n_hist=None, want_null=False, nq=4, nrep=2):
    """mcsas_hip_histogram_partial (or _device_rows, or the plain call) -> (rc, message)"""
    lib = _lib.load()
    model = make_models("sphere", H.PAR_LO[:1], H.PAR_HI[:1])[0].setup()
    if specs is None:
        specs = [dict(param_index=0, yweight="vol", edges=np.linspace(2e-9, 1e-7, 4), lower=2e-9, upper=1e-7) for _ in want]
    q = np.geomspace(1e8, 3e9, nq)
    contribs = np.full((N, 1, nrep), 1e-8)
    call = engine._HistogramCall(model, q, np.ones(nq), np.ones(nq), contribs, 0.5, specs)
    if device_rows:
        call.prob.c.model_id = engine.MODEL_HOST
    w = (C.c_int32 * max(len(want), 1))(*want)
    part = np.zeros(1 << 16)
    args = [C.byref(call.prob.c), _lib.as_dp(call.contribs)]
    cb = _lib.DeviceRowsCallback(lambda user, n: 0)
    if device_rows:
        args += [C.c_void_p(64), C.c_void_p(64), C.c_void_p(64), N * nrep, cb, None]
    args += [len(specs) if n_hist is None else n_hist, call.arr]
    if not plain:
        args += [None if want_null else w]
    args += [_lib.as_dp(call.sc), _lib.as_dp(call.frac), _lib.as_dp(call.out)]
    if not plain:
        args += [_lib.as_dp(part) if partial else None]
    fn = {(False, False): lib.mcsas_hip_histogram_partial, (True, False): lib.mcsas_hip_histogram_partial_device_rows,
          (False, True): lib.mcsas_hip_histogram, (True, True): lib.mcsas_hip_histogram_device_rows}[(device_rows, plain)]
    rc = fn(*args)
    return rc, lib.mcsas_hip_last_error().decode()


def _spec(nb=3, edges=None):
    return dict(param_index=0, yweight="vol", edges=np.linspace(2e-9, 1e-7, nb + 1) if edges is None else np.asarray(edges, dtype=float),
                lower=2e-9, upper=1e-7)


REFUSALS = dict(
    want_null=(dict(want_null=True), "want is NULL"),
    want_negative=(dict(want=(1, -1)), "histogram 1: want -1"),
    want_three=(dict(want=(0, 3)), "histogram 1: want 3"),
    partial_null=(dict(want=(0, 1), partial=False), "histogram 1 wants curves (want 1), but partial is NULL"),
    bins_257=(dict(want=(1, 2), specs=[_spec(), _spec(257)]), "histogram 1: the bin curves keep every bin's running sums in LDS: n_bin 257 > 256"),
    edges_nan=(dict(want=(0, 2), specs=[_spec(), _spec(edges=[1e-9, np.nan, 1e-7])]), "histogram 1: bin curves need edges that are finite and non-decreasing"),
    edges_inf=(dict(want=(0, 2), specs=[_spec(), _spec(edges=[1e-9, 1e-8, np.inf])]), "histogram 1: bin curves need edges that are finite and non-decreasing"),
    edges_fall=(dict(want=(0, 2), specs=[_spec(), _spec(edges=[1e-9, 1e-7, 1e-8])]), "histogram 1: bin curves need edges that are finite and non-decreasing"),
    too_large=(dict(want=(1, 2), specs=[_spec(), _spec(256)], nq=4096, nrep=512, N=1), "histogram 1: the curves wanted up to here take"),
)


@pytest.mark.parametrize("device_rows", (False, True), ids=("model", "device_rows"))
@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_a_refusal_names_the_histogram_before_a_device_is_selected(name, device_rows):
    kw, sentence = REFUSALS[name]
    rc, msg = _call(device_rows=device_rows, **kw)
    assert rc == EINVAL and msg.startswith("histogram_partial: ") and sentence in msg, (rc, msg)


@pytest.mark.parametrize("device_rows", (False, True), ids=("model", "device_rows"))
def test_what_passes_and_what_the_plain_call_refuses(device_rows):
    have = _lib.load().mcsas_hip_device_count() > 0
    go_on = (OK,) if have and not device_rows else ((EINVAL,) if have else (ENODEV,))   # (device_rows: the dummy buffers are refused once a device is there)
    for kw in (dict(want=(2, 1)), dict(want=(0, 0), partial=False), dict(want=(1, 2), specs=[_spec(300), _spec(256)]),
               dict(want=(1, 0), specs=[_spec(edges=[1e-7, 1e-8, np.nan]), _spec(edges=[1e-7, 1e-8, np.nan])])):
        rc, msg = _call(device_rows=device_rows, **kw)
        assert rc in go_on and (rc == OK or "histogram_partial" not in msg), (kw, rc, msg)     # (a call that succeeds leaves the last message alone)
    # the plain call's refusals, in its own words, from both forms
    for kw in (dict(N=4097), dict(specs=[_spec(), dict(_spec(), param_index=1)], want=(1, 1)), dict(n_hist=-1)):
        plain, partial = _call(device_rows=device_rows, plain=True, **kw), _call(device_rows=device_rows, **kw)
        assert plain[0] == partial[0] == EINVAL and plain[1] == partial[1] and "histogram_partial" not in partial[1], (kw, plain, partial)
    assert _call(device_rows=device_rows, want=(), specs=[], want_null=True, partial=False)[0] in go_on     # nothing to want: the plain call


# ------------------------------------------------------------------------------------------------- the Python layers
def test_histogram_takes_partialIntensity_and_says_so_in_its_spec():
    p = FitParameter("radius", 1e-8, valueRange=(0., 1.), activeRange=(1e-9, 1e-7))
    with pytest.raises(ValueError, match="partialIntensity"):
        Histogram(p, 1e-9, 1e-7, partialIntensity="x")
    h = Histogram(p, 1e-9, 1e-7, binCount=5)
    assert h.partialIntensity is None and "partial" not in h.deviceSpec(0) and h.intensity is None and h.binIntensity is None
    assert Histogram(p, 1e-9, 1e-7, binCount=5, partialIntensity="range").deviceSpec(0)["partial"] == "range"
    assert Histogram(p, 1e-9, 1e-7, binCount=256, partialIntensity="bins").deviceSpec(0)["partial"] == "bins"
    big = Histogram(p, 1e-9, 1e-7, binCount=257, partialIntensity="bins")
    assert "partial" not in big.deviceSpec(0) and not big.partialOnDevice()        # (McSAS.histogram() takes it in numpy)
    assert engine.HISTOGRAM_PARTIAL_MAX_BINS == 256
    rng = np.arange(12.0).reshape(4, 3)
    h.moments = type("M", (), {})()
    h.setIntensity(rng, np.arange(60.0).reshape(5, 4, 3))
    assert np.array_equal(h.intensity.full, rng) and np.array_equal(h.moments.intensity[0], rng.mean(axis=1))
    assert np.array_equal(h.moments.intensity[1], rng.std(axis=1, ddof=1))          # utils/parameter.py:150-154
    assert h.binIntensity.full.shape == (5, 4, 3) and h.binIntensity.mean.shape == (5, 4) and h.binIntensity.std.shape == (5, 4)
    h.setIntensity(rng[:, :1])
    assert np.array_equal(h.moments.intensity[1], np.zeros(4)) and h.binIntensity is None     # one repetition: ddof 0


def test_the_engine_call_lays_the_curves_out_in_order():
    model = make_models("sphere", H.PAR_LO[:1], H.PAR_HI[:1])[0].setup()
    specs = [_spec(3), _spec(2), dict(_spec(4), partial="range")]
    mk = lambda **kw: engine._HistogramCall(model, np.geomspace(1e8, 3e9, 5), np.ones(5), np.ones(5), np.full((6, 1, 2), 1e-8), 0.5, specs, **kw)
    assert mk(partial=None).want.tolist() == [0, 0, 1] and mk(partial=[0, 0, 0]).want is None
    call = mk(partial=["bins", 0, 1])
    assert call.want.tolist() == [2, 0, 1] and call.partial.size == 5 * 2 * (1 + 3) + 5 * 2
    call.partial[:] = np.arange(call.partial.size)
    hs = call.unpack()[2]
    assert np.array_equal(hs[0]["intensity"], np.arange(10.0).reshape(5, 2))
    assert np.array_equal(hs[0]["bin_intensity"], 10 + np.arange(30.0).reshape(3, 5, 2))
    assert "intensity" not in hs[1] and "bin_intensity" not in hs[2]
    assert np.array_equal(hs[2]["intensity"], 40 + np.arange(10.0).reshape(5, 2))
    for bad in ([1, 2], [1, 2, "x"], [True, 0, 0]):
        with pytest.raises(ValueError, match="partial"):
            mk(partial=bad)
    with pytest.raises(ValueError, match="no partial"):
        engine.histogram_device_batch([dict(model=model, q=np.geomspace(1e8, 3e9, 5), intensity=np.ones(5), sigma=np.ones(5),
                                            contribs=np.full((6, 1, 2), 1e-8), comp_exp=0.5, specs=specs)])

"""Accuracy of mcsas_amd/csrc/fastmath.h (the fp64 sincos / J1 / division the form-factor kernels use instead of
the device libm), measured on a HOST build of the same header: tests/native/fastmath_host.cpp compiled with g++
(-mfma so that fma() is the single-rounding instruction the GPU executes, -ffp-contract=off so that nothing else
is fused).  References: x87 extended precision (64-bit significand) for sin / cos / division / rsqrt, scipy's
Cephes J1 for the Bessel function.  The bounds asserted here are the ones fastmath.h states.

What does NOT carry over from the host: the hardware reciprocal / reciprocal-square-root seeds of div_fast and
rsqrt_fast (v_rcp_f64, v_rsq_f64) are replaced by float-precision stand-ins.  div_fast's two Newton steps and residual
correction make its result independent of the seed: the device gives the host's bits.  rsqrt_fast's single correction
does not: the device result differs from the host build's in the last bit for about a fifth of the arguments (and so
does j1_core above x = 5, which calls it); both stay within the bounds above.  tests/test_fastmath_device.py runs every
function here on the device and checks both statements."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "fastmath_host.cpp")
dp = C.POINTER(C.c_double)


def P(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fastmath") / "libfastmath_host.so")
    cmd = ["g++", "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-o", out, SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("host build of fastmath.h failed (no FMA on this CPU?): " + r.stderr[-300:])
    L = C.CDLL(out)
    if L.fm_long_double_digits() < 64:
        pytest.skip("long double is not extended precision on this host")
    return L


def ulp_of(ref):
    return np.spacing(np.abs(ref))


def sincos(lib, fn, x):
    s, c = np.empty_like(x), np.empty_like(x)
    getattr(lib, fn)(len(x), P(x), P(s), P(c))
    return s, c


def ref_sincos(lib, x):
    a, b, c, d = (np.empty_like(x) for _ in range(4))
    lib.fm_ref_sincos(len(x), P(x), P(a), P(b), P(c), P(d))
    return a, b, c, d


def point_sets():
    rs = np.random.RandomState(1)
    k = np.arange(1, 667000, dtype=float)                      # k pi/2 < 2^20
    near = k * (np.pi / 2)
    return {
        "uniform": rs.uniform(-2.0**20, 2.0**20, 1500000),
        "log": 10 ** rs.uniform(-8, np.log10(2.0**20 * 0.999999), 1500000),
        "small": rs.uniform(-4, 4, 500000),
        "tiny": np.concatenate([[0.0, 1e-300, -1e-300, 5e-324], 10 ** rs.uniform(-300, -8, 1000)]),
        # the doubles next to multiples of pi/2, where the reduced argument is smallest
        "near_kpi2": np.concatenate([near, np.nextafter(near, np.inf), np.nextafter(near, -np.inf)]),
        "handoff": np.nextafter(2.0**20, 0) - np.arange(0, 2000) * 2.0**-32,
    }


@pytest.mark.parametrize("name", list(point_sets()))
def test_sincos_fast_relative_error(lib, name):
    """sincos_fast, |x| < 2^20: three-term Cody-Waite + fdlibm kernels: <= 1.6 ulp everywhere (0.8 ulp of the
    kernels + the rounding of the reduced argument), including next to multiples of pi/2."""
    x = np.ascontiguousarray(point_sets()[name])
    sh, sl, ch, cl = ref_sincos(lib, x)
    s, c = sincos(lib, "fm_sincos_fast", x)
    es, ec = np.abs((s - sh) - sl), np.abs((c - ch) - cl)
    assert (es / ulp_of(sh)).max() <= 1.6 and (ec / ulp_of(ch)).max() <= 1.6
    assert es.max() <= 1.8e-16 and ec.max() <= 1.8e-16


@pytest.mark.parametrize("name", list(point_sets()))
def test_sincos_core_absolute_error(lib, name):
    """sincos_core (branch-free, two-term reduction, what the row kernels call when q r < 2^20): ABSOLUTE error
    <= 1.8e-16 everywhere and <= 1.6 ulp away from multiples of pi/2; next to them (|value| < 1e-9) the dropped
    third reduction term (< 2e-27) shows as a relative error, the absolute error there is <= 2e-26."""
    x = np.ascontiguousarray(point_sets()[name])
    sh, sl, ch, cl = ref_sincos(lib, x)
    s, c = sincos(lib, "fm_sincos_core", x)
    es, ec = np.abs((s - sh) - sl), np.abs((c - ch) - cl)
    assert es.max() <= 1.8e-16 and ec.max() <= 1.8e-16
    big_s, big_c = np.abs(sh) > 1e-9, np.abs(ch) > 1e-9
    assert (es[big_s] / ulp_of(sh[big_s])).max() <= 1.6 and (ec[big_c] / ulp_of(ch[big_c])).max() <= 1.6
    if (~big_s).any():
        assert es[~big_s].max() <= 2e-26
    if (~big_c).any():
        assert ec[~big_c].max() <= 2e-26


def test_sincos_large_arguments_take_libm(lib):
    """|x| >= 2^20 (and NaN / Inf) leave the fast path: libm on the host, ocml on the device."""
    x = np.array([2.0**20, -2.0**20, 3.0e9, 1e15, 1e300])
    s, c = sincos(lib, "fm_sincos_fast", x)
    np.testing.assert_allclose(s, np.sin(x), rtol=0, atol=2.3e-16)
    np.testing.assert_allclose(c, np.cos(x), rtol=0, atol=2.3e-16)
    s, c = sincos(lib, "fm_sincos_fast", np.array([np.nan, np.inf]))
    assert np.isnan(s).all() and np.isnan(c).all()


def test_j1_against_scipy(lib):
    """j1_fast / j1_core are the Cephes rationals behind scipy.special.j1 re-associated to one division per branch:
    5e-16 absolute against scipy over (0, 2^20), both branches and the x = 5 seam; j1_fast is odd."""
    from scipy.special import j1
    rs = np.random.RandomState(2)
    x = np.concatenate([rs.uniform(0, 5, 400000), rs.uniform(5, 60, 400000), 10 ** rs.uniform(-6, 6, 400000),
                        np.nextafter(5.0, 0) - np.arange(100) * 1e-15, 5.0 + np.arange(100) * 1e-15,
                        [3.8317059702075125, 7.015586669815619, 1e-12, 1048575.9]])
    x = np.ascontiguousarray(x[(x > 0) & (x < 2.0**20)])
    ref = j1(x)
    for fn in ("fm_j1_fast", "fm_j1_core"):
        y = np.empty_like(x)
        getattr(lib, fn)(len(x), P(x), P(y))
        assert np.abs(y - ref).max() <= 5e-16, fn
        rel = np.abs(y - ref)[np.abs(ref) > 1e-3] / np.abs(ref)[np.abs(ref) > 1e-3]
        assert rel.max() <= 3e-13, fn                       # relative: limited by the zeros of J1, as scipy's own
    xm = np.ascontiguousarray(-x[:1000])
    y = np.empty_like(xm)
    lib.fm_j1_fast(len(xm), P(xm), P(y))
    yp = np.empty_like(xm)
    xp = np.ascontiguousarray(x[:1000])
    lib.fm_j1_fast(len(xp), P(xp), P(yp))
    np.testing.assert_array_equal(y, -yp)


def test_div_and_rsqrt(lib):
    """div_fast: <= 1 ulp for normal-range operands; rsqrt_fast: <= 1.5 ulp.  (Operand range of the sweep: what
    the host stand-in for the hardware seed — a float — can hold; the kernels divide by x^3 and by polynomial
    denominators of x = q r in 1e-4 .. 1e6.)"""
    rs = np.random.RandomState(3)
    a = np.ascontiguousarray(rs.uniform(-1, 1, 1000000) * 10 ** rs.uniform(-100, 100, 1000000))
    b = np.ascontiguousarray(rs.uniform(0.5, 1, 1000000) * 10 ** rs.uniform(-30, 30, 1000000) * rs.choice([-1, 1], 1000000))
    y, hi, lo = np.empty_like(a), np.empty_like(a), np.empty_like(a)
    lib.fm_div_fast(len(a), P(a), P(b), P(y))
    lib.fm_ref_div(len(a), P(a), P(b), P(hi), P(lo))
    assert (np.abs((y - hi) - lo) / ulp_of(hi)).max() <= 1.0
    x = np.ascontiguousarray(10 ** rs.uniform(-30, 30, 1000000))
    lib.fm_rsqrt_fast(len(x), P(x), P(y))
    lib.fm_ref_rsqrt(len(x), P(x), P(hi), P(lo))
    assert (np.abs((y - hi) - lo) / ulp_of(hi)).max() <= 1.5


def test_expm1_neg_fast(lib):
    """expm1_neg_fast (x <= 0; the Kholodenko quadrature's one transcendental per point besides sincos): <= 2 ulp
    against x87 expm1l from -1e-300 down to -60, including the arguments next to the k ln2 / 2 seams and the tiny
    ones where exp(x) - 1 would cancel."""
    rs = np.random.RandomState(4)
    seams = (np.arange(1, 80) * 0.5 * np.log(2.0))
    x = -np.concatenate([rs.uniform(0, 2.5, 600000), 10 ** rs.uniform(-300, 0, 200000), rs.uniform(2, 60, 200000),
                         seams, np.nextafter(seams, 0), np.nextafter(seams, 100), [0.0, 1e-320, 745.0, 800.0]])
    x = np.ascontiguousarray(x)
    y, hi, lo = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    lib.fm_expm1_neg_fast(len(x), P(x), P(y))
    lib.fm_ref_expm1(len(x), P(x), P(hi), P(lo))
    err = np.abs((y - hi) - lo) / np.maximum(ulp_of(hi), 5e-324)
    assert err.max() <= 2.0, (err.max(), x[np.argmax(err)])


# ------------------------------------------------------------------------------------------ sin x - x cos x, _n, split J1
EPS = 2.0**-52                      # ulp(v) <= EPS |v| for every normal double v


def tan_x_zeros(ks=None):
    """The positive roots of tan x = x (the zeros of sin x - x cos x, i.e. of the sphere's form factor), one per
    k in `ks`, x_k in (k pi, k pi + pi/2), to the nearest double (mpmath, 40 digits), each with its two neighbours."""
    import mpmath as mp
    if ks is None:
        ks = np.unique(np.concatenate([np.arange(1, 201), np.logspace(np.log10(201), np.log10(330000), 100).astype(int)]))
    with mp.workdps(40):
        roots = []
        for k in ks:
            a = mp.mpf(int(k)) * mp.pi + mp.pi / 2 - mp.mpf(1) / (int(k) * mp.pi + mp.pi / 2)  # 1st-order asymptote
            roots.append(float(mp.findroot(lambda t: mp.sin(t) - t * mp.cos(t), a)))
    r = np.array(roots)
    return np.concatenate([r, np.nextafter(r, np.inf), np.nextafter(r, 0)])


def smxc_mp(x, dps=40):
    """sin x - x cos x of the doubles x, in `dps`-digit arithmetic, rounded to double."""
    import mpmath as mp
    with mp.workdps(dps):
        return np.array([float(mp.sin(mp.mpf(v)) - mp.mpf(v) * mp.cos(mp.mpf(v))) for v in x])


def smxc_bound(x, value):
    """What fma(-x, cos x, sin x) may be off by, with sin x, cos x from sincos_core (the documented equivalent of
    sin_minus_xcos): each of s, c carries <= 1.6 ulp <= 1.6 EPS |.| of its own value, or 2e-26 absolute where that value
    is < 1e-9 (the dropped third reduction term); the fma multiplies c's error by |x| and rounds once, so
      |err| <= 1.6 EPS (|x cos x| + |sin x|) + 2e-26 (1 + |x|) + ulp(value) / 2.
    It scales with the magnitude of the two TERMS, not with their difference: that is the cancellation at small x and
    next to the zeros, which the kernel shares with the reference's own expression."""
    ax = np.abs(x)
    return 1.6 * EPS * (ax * np.abs(np.cos(x)) + np.abs(np.sin(x))) + 2e-26 * (1 + ax) + 0.5 * np.spacing(np.abs(value))


def fm1(lib, fn, x):
    y = np.empty_like(x)
    getattr(lib, fn)(len(x), P(x), P(y))
    return y


def smxc_point_sets():
    s = point_sets()
    s.pop("handoff")                                             # (callers keep q x below 2^20: no libm branch here)
    s["handoff"] = np.nextafter(2.0**20, 0) - np.arange(1, 2000) * 2.0**-32
    s["tan_zeros"] = tan_x_zeros()
    return s


@pytest.mark.parametrize("name", list(smxc_point_sets()))
def test_sin_minus_xcos_is_the_fma_of_sincos_core(lib, name):
    """sin_minus_xcos equals fma(-x, cos x, sin x) taken from sincos_core bit for bit; sin_minus_xcos_abs equals it up
    to the sign (fastmath.h: fma(-x, -c, -s) == -fma(-x, c, s)), so its square is the same double."""
    x = np.ascontiguousarray(smxc_point_sets()[name])
    ref = fm1(lib, "fm_sin_minus_xcos_via_core", x)
    signed = fm1(lib, "fm_sin_minus_xcos", x)
    absv = fm1(lib, "fm_sin_minus_xcos_abs", x)
    np.testing.assert_array_equal(signed, ref)
    np.testing.assert_array_equal(np.abs(absv), np.abs(ref))
    np.testing.assert_array_equal(absv * absv, ref * ref)


@pytest.mark.parametrize("name", list(smxc_point_sets()))
def test_sin_minus_xcos_within_its_bound(lib, name):
    """sin_minus_xcos / _abs against x87 (whose own error, ~3 2^-64 (|sin x| + |x cos x|), is 2^-12 of the bound and
    is added to it) within smxc_bound; on the sets where the difference cancels (tiny / small x, the zeros of
    tan x = x) also against mpmath at 40 digits."""
    x = np.ascontiguousarray(smxc_point_sets()[name])
    hi, lo = np.empty_like(x), np.empty_like(x)
    lib.fm_ref_sin_minus_xcos(len(x), P(x), P(hi), P(lo))
    signed = fm1(lib, "fm_sin_minus_xcos", x)
    absv = fm1(lib, "fm_sin_minus_xcos_abs", x)
    b = smxc_bound(x, hi) + 4 * 2.0**-64 * (np.abs(x * np.cos(x)) + np.abs(np.sin(x)))
    err = np.abs((signed - hi) - lo)
    assert (err / b).max() <= 1.0, (name, (err / b).max(), x[np.argmax(err / b)])
    erra = np.abs((np.abs(absv) - np.abs(hi)) - np.sign(hi) * lo)
    assert (erra / b).max() <= 1.0, (name, (erra / b).max())
    if name in ("tiny", "tan_zeros", "small"):
        xs = np.ascontiguousarray(x if name != "small" else x[np.abs(x) < 0.1][:3000])
        ex = smxc_mp(xs)
        got = fm1(lib, "fm_sin_minus_xcos", xs)
        r = np.abs(got - ex) / smxc_bound(xs, ex)
        assert r.max() <= 1.0, (name, r.max(), xs[np.argmax(r)])


def test_sin_minus_xcos_small_argument_regime(lib):
    """The cancellation at small x, stated: for 1e-6 <= x <= 0.1 the value is x^3/3 (1 - x^2/10 + ...) while the bound
    is ~3.2 EPS x — the RELATIVE error may reach ~10 EPS / x^2, and the evaluation is asked to stay inside that, not to beat
    it; at x = 1 and beyond the terms and the difference are of one size and the error is a few ulp of the value."""
    x = np.ascontiguousarray(np.logspace(-6, -1, 400))
    ex = smxc_mp(x)
    got = fm1(lib, "fm_sin_minus_xcos", x)
    assert (np.abs(got - ex) / smxc_bound(x, ex)).max() <= 1.0
    x = np.ascontiguousarray(np.linspace(1.0, 4.0, 400))
    ex = smxc_mp(x)
    got = fm1(lib, "fm_sin_minus_xcos", x)
    assert (np.abs(got - ex) / np.spacing(np.abs(ex))).max() <= 8.0   # terms <= 4x the value here: 1.6 * 2 * 4 / 2 + 1/2


def _pad8(x):
    return np.ascontiguousarray(np.concatenate([x, np.full((-len(x)) % 8, 1.0)]))


@pytest.mark.parametrize("name", list(smxc_point_sets()))
def test_n_variants_are_bit_identical_to_the_scalar_forms(lib, name):
    """sincos_poly_n / sincos_core_n / sin_minus_xcos_abs_n at N = 4 and 8 equal sincos_poly / sincos_core /
    sin_minus_xcos_abs per element, bit for bit (fastmath.h: same operations in the same order per element)."""
    x = _pad8(smxc_point_sets()[name])
    n = len(x)
    s0, c0, q0 = np.empty_like(x), np.empty_like(x), np.empty(n, dtype=np.int32)
    lib.fm_sincos_poly(n, P(x), P(s0), P(c0), q0.ctypes.data_as(C.POINTER(C.c_int)))
    sn0, cs0 = sincos(lib, "fm_sincos_core", x)
    g0 = fm1(lib, "fm_sin_minus_xcos_abs", x)
    for N in (4, 8):
        s, c, q = np.empty_like(x), np.empty_like(x), np.empty(n, dtype=np.int32)
        getattr(lib, "fm_sincos_poly_n%d" % N)(n, P(x), P(s), P(c), q.ctypes.data_as(C.POINTER(C.c_int)))
        np.testing.assert_array_equal(s.view(np.int64), s0.view(np.int64))
        np.testing.assert_array_equal(c.view(np.int64), c0.view(np.int64))
        np.testing.assert_array_equal(q, q0)
        sn, cs = sincos(lib, "fm_sincos_core_n%d" % N, x)
        np.testing.assert_array_equal(sn.view(np.int64), sn0.view(np.int64))
        np.testing.assert_array_equal(cs.view(np.int64), cs0.view(np.int64))
        g = fm1(lib, "fm_sin_minus_xcos_abs_n%d" % N, x)
        np.testing.assert_array_equal(g.view(np.int64), g0.view(np.int64))


def j1_points():
    rs = np.random.RandomState(2)
    x = np.concatenate([rs.uniform(0, 5, 200000), rs.uniform(5, 60, 200000), 10 ** rs.uniform(-6, 6, 200000),
                        np.nextafter(5.0, 0) - np.arange(100) * 1e-15, 5.0 + np.arange(100) * 1e-15, [5.0],
                        [3.8317059702075125, 7.015586669815619, 1e-12, 1048575.9]])
    return np.ascontiguousarray(x[(x > 0) & (x < 2.0**20)])


def test_split_j1_ranges_are_j1_core(lib):
    """j1_core_small (x <= 5) and j1_core_large (x > 5) are j1_core's two branches bit for bit — the interleaved
    cylinder loop calls them directly when a whole group of arguments is on one side of x = 5."""
    x = j1_points()
    core = fm1(lib, "fm_j1_core", x)
    sm, lg = x <= 5.0, x > 5.0
    ys = fm1(lib, "fm_j1_core_small", np.ascontiguousarray(x[sm]))
    yl = fm1(lib, "fm_j1_core_large", np.ascontiguousarray(x[lg]))
    np.testing.assert_array_equal(ys.view(np.int64), core[sm].view(np.int64))
    np.testing.assert_array_equal(yl.view(np.int64), core[lg].view(np.int64))
    from scipy.special import j1
    assert np.abs(ys - j1(x[sm])).max() <= 5e-16 and np.abs(yl - j1(x[lg])).max() <= 5e-16


def hard_division_cases(n=20000, seed=7):
    """Operand pairs (a, b) whose quotient lies within 2^-54 ulp of the midpoint between two doubles, on either side:
    b an odd 53-bit integer, c = (2m + 1) the midpoint's numerator with b c = -+1 (mod 2^54) (b is odd, so c = -+b^-1 mod 2^54),
    a = (b c +- 1) / 2^54 — an integer below 2^53, so a double — and a / b = c / 2^54 +- 1 / (b 2^54); scaled by powers of two.
    Only a division whose reciprocal carries a relative error far below 2^-54 rounds all of them correctly."""
    rs = np.random.RandomState(seed)
    M = 1 << 54
    A, B = [], []
    while len(A) < n:
        b = int(rs.randint(1 << 20, 1 << 31)) << 22 | int(rs.randint(0, 1 << 22)) | 1
        if not (1 << 52) <= b < (1 << 53):
            continue
        s = 1 if len(A) % 2 else -1
        c = (-s * pow(b, -1, M)) % M
        if not (1 << 53) <= c < M:
            continue
        a, r = divmod(b * c + s, M)
        assert r == 0 and a < (1 << 53)
        A.append(float(a)); B.append(float(b))
    ea, eb = rs.randint(-60, 60, n), rs.randint(-60, 60, n)
    return np.ascontiguousarray(np.ldexp(A, ea)), np.ascontiguousarray(np.ldexp(B, eb))


def test_div_fast_rounds_hard_quotients_correctly(lib):
    """div_fast = reciprocal seed, two Newton steps, q = a y, residual r = fma(-b, q, a), fma(r, y, q): the last step puts
    q + (a/b - q)(1 - d) with d the reciprocal's relative error, so it rounds like a/b unless a/b lies within about
    |a/b - q| d of a midpoint.  After two steps d <= ~(2^-24)^4 (host stand-in seed; the device seed is better): far below
    the 2^-54 ulp of hard_division_cases, so every one of them comes out correctly rounded (= numpy's IEEE a / b)."""
    a, b = hard_division_cases()
    y = np.empty_like(a)
    lib.fm_div_fast(len(a), P(a), P(b), P(y))
    np.testing.assert_array_equal(y, a / b)

"""mcsas_amd/csrc/fastmath.h as the DEVICE executes it, at the ulp level.

tests/test_fastmath.py measures a g++ build of the header; here the same functions run on the GPU, compiled with the library's
own flags (-O3 -ffp-contract=off, gfx950) through the run-time plug-in path: a probe model (FastmathProbe below) whose
absVolume() and surface() return one device evaluation each.  Contrib<PLUGIN>::prepare stores the two unchanged as vset / sset
and engine.model_calc returns them per parameter row, so every row is one exact device result on each of two channels
(volume() is 1: w = 1; every value range is the widest a parameter has, +-1e200, so the clip of full_params never bites).

Row = (a, selector, b, c):
  0  sincos_fast(a)                      -> sin, cos
  1  sincos_core(a)                      -> sin, cos
  2  sin_minus_xcos_abs(a), sin_minus_xcos(a)
  3  j1_fast(a), j1_core(a, b = 1/a)
  4  j1_core_small(a), j1_core_large(a, b = 1/a)
  5  div_fast(a, b), rsqrt_fast(a)
  6  expm1_neg_fast(a), sincos_poly(a)'s quadrant
  7  the _n variants (sincos_poly_n, sincos_core_n, sin_minus_xcos_abs_n) at N = 4 / 8 on a + i b, i < N, against the scalar
     forms per element, in the probe: the number of elements whose bits differ
  8  Contrib<SPHERE> prepared from a local ModelArgs (radius a, compensation exponent 0: w = 1): intensity_fast(q = b,
     q3inv = c) and intensity(b) — the hot path and the model_calc path (used by tests/test_formfactor_exact.py)
  9  the same Contrib, compensation exponent c: intensity_fast_n<4> / <8> at q_i = b (1 + i / 16) against intensity_fast per
     element (q3inv_i = 1 / (q_i q_i q_i), the library's table, mcsas_hip.hip): the number of elements whose bits differ

Functions without a hardware seed (the sincos and sin_minus_xcos families, expm1_neg_fast) must give the host build's bits.
div_fast / rsqrt_fast / j1_* start from v_rcp_f64 / v_rsq_f64 on the device: they are held to the bounds fastmath.h states.
div_fast's result does not depend on the seed (device bits == host bits, asserted); rsqrt_fast's single correction step does
not remove the seed's last bits (about a fifth of its results, and of j1_core's above x = 5, differ from the host build's in
the last place; asserted only to stay within the bounds)."""
import ctypes as C

import numpy as np
import pytest

from test_fastmath import (lib, P, point_sets, ref_sincos, ulp_of, fm1, smxc_point_sets, smxc_bound, tan_x_zeros, j1_points,  # noqa: F401
                           hard_division_cases)

pytestmark = pytest.mark.gpu

PROBE_SOURCE = r"""
// tests/test_fastmath_device.py: one device evaluation of a fastmath.h function per parameter row, on two channels
#define MCSAS_PLUGIN_ROW_CLASS 0
__device__ static inline bool mcsas_probe_same(double x, double y) { return __double_as_longlong(x) == __double_as_longlong(y); }
template <int N>
__device__ static double mcsas_probe_n(double a, double b) {
    double x[N], s[N], c[N], sn[N], cs[N], g[N];
    int q[N];
    for (int i = 0; i < N; ++i) x[i] = a + (double)i * b;
    mcsas::sincos_poly_n<N>(x, s, c, q);
    mcsas::sincos_core_n<N>(x, sn, cs);
    mcsas::sin_minus_xcos_abs_n<N>(x, g);
    int bad = 0;
    for (int i = 0; i < N; ++i) {
        double s1, c1, sn1, cs1;
        int q1;
        mcsas::sincos_poly(x[i], &s1, &c1, &q1);
        mcsas::sincos_core(x[i], &sn1, &cs1);
        const double g1 = mcsas::sin_minus_xcos_abs(x[i]);
        bad += !(mcsas_probe_same(s[i], s1) && mcsas_probe_same(c[i], c1) && q[i] == q1 && mcsas_probe_same(sn[i], sn1)
                 && mcsas_probe_same(cs[i], cs1) && mcsas_probe_same(g[i], g1));
    }
    return (double)bad;
}
__device__ static mcsas::Contrib<MCSAS_MODEL_SPHERE> mcsas_probe_sphere(double r, double qmax, double comp_exp) {
    mcsas::ModelArgs m = {};
    m.model_id = MCSAS_MODEL_SPHERE; m.n_active = 1;
    for (int i = 0; i < MCSAS_MAX_ACTIVE; ++i) { m.active_index[i] = i == 0 ? 0 : -1; m.clip_lo[i] = 0.; m.clip_hi[i] = 1e200; }
    m.params[0] = r; m.params[1] = 1.;
    m.comp_exp = comp_exp; m.int_div = 1; m.qmax = qmax;
    const double row[MCSAS_MAX_ACTIVE] = {r, 0., 0., 0.};
    mcsas::Contrib<MCSAS_MODEL_SPHERE> c;
    c.prepare(m, row);
    return c;
}
template <int N>
__device__ static double mcsas_probe_sphere_n(double r, double q0, double comp_exp) {
    double q[N], q3[N], o[N];
    for (int i = 0; i < N; ++i) { q[i] = q0 * (1. + (double)i * 0.0625); q3[i] = 1.0 / (q[i] * q[i] * q[i]); }
    const mcsas::Contrib<MCSAS_MODEL_SPHERE> c = mcsas_probe_sphere(r, q[N - 1], comp_exp);
    c.template intensity_fast_n<N>(q, q3, o);
    int bad = 0;
    for (int i = 0; i < N; ++i) bad += !mcsas_probe_same(o[i], c.intensity_fast(q[i], q3[i]));
    return (double)bad;
}
__device__ static void mcsas_probe(const double *p, double *u, double *v) {
    const double a = p[0], b = p[2], c = p[3];
    *u = 0.; *v = 0.;
    switch ((int)p[1]) {
        case 0: mcsas::sincos_fast(a, u, v); break;
        case 1: mcsas::sincos_core(a, u, v); break;
        case 2: *u = mcsas::sin_minus_xcos_abs(a); *v = mcsas::sin_minus_xcos(a); break;
        case 3: *u = mcsas::j1_fast(a); *v = mcsas::j1_core(a, b); break;
        case 4: *u = mcsas::j1_core_small(a); *v = mcsas::j1_core_large(a, b); break;
        case 5: *u = mcsas::div_fast(a, b); *v = mcsas::rsqrt_fast(a); break;
        case 6: { double s, cc; int q; mcsas::sincos_poly(a, &s, &cc, &q); *u = mcsas::expm1_neg_fast(a); *v = (double)q; break; }
        case 7: *u = mcsas_probe_n<4>(a, b); *v = mcsas_probe_n<8>(a, b); break;
        case 8: { const mcsas::Contrib<MCSAS_MODEL_SPHERE> s = mcsas_probe_sphere(a, b, 0.); *u = s.intensity_fast(b, c); *v = s.intensity(b, nullptr); break; }
        case 9: *u = mcsas_probe_sphere_n<4>(a, b, c); *v = mcsas_probe_sphere_n<8>(a, b, c); break;
        default: *u = *v = __longlong_as_double(0x7ff8dead00000000ll);
    }
}
__device__ double mcsas_plugin_volume(const double *p) { return 1.; }
__device__ double mcsas_plugin_absvolume(const double *p) { double u, v; mcsas_probe(p, &u, &v); return u; }
__device__ double mcsas_plugin_surface(const double *p) { double u, v; mcsas_probe(p, &u, &v); return v; }
__device__ double mcsas_plugin_formfactor(double q, const double *p) { return 0.; }
"""

SINCOS_FAST, SINCOS_CORE, SMXC, J1, J1_SPLIT, DIV_RSQRT, EXPM1_Q, N_VARIANTS, SPHERE, SPHERE_N = range(10)


def probe_model():
    from mcsas_amd.scatteringmodels import SASModel, _fp

    class FastmathProbe(SASModel):
        """Not a scattering model: the device probe of this module (see its docstring)."""
        shortName = "fastmath probe"
        model_id = None
        hipSource = PROBE_SOURCE
        parameters = tuple(_fp(n, 0., valueRange=(-np.inf, np.inf), activeRange=(-1., 1.)) for n in ("a", "sel", "b", "c"))

        def __init__(self):
            super().__init__()
            for p in self.params():
                p.setActive(True)

    return FastmathProbe()


@pytest.fixture(scope="module")
def probe():
    """run(selector, a, b=0, c=0) -> the two channels, one device evaluation per element (one compile for everything)."""
    from mcsas_amd import engine
    setup = probe_model().setup()
    assert setup.model_id >= engine.MODEL_PLUGIN0 and setup.n_active == 4
    assert (setup.clip_lo <= -1e200).all() and (setup.clip_hi >= 1e200).all()
    q = np.array([1.0])

    def run(sel, a, b=0.0, c=0.0):
        a = np.asarray(a, dtype=float)
        rows = np.stack(np.broadcast_arrays(a, float(sel), np.asarray(b, dtype=float), np.asarray(c, dtype=float)), axis=1)
        assert np.isfinite(rows).all() and (np.abs(rows) < 1e200).all()     # inside the clip: the probe sees the values as given
        _, u, w, v = engine.model_calc(setup, q, np.ascontiguousarray(rows), 0.6666666)
        assert (w == 1.0).all()
        return u, v
    return run


def bitdiff(x, y):
    return int((np.ascontiguousarray(x).view(np.int64) != np.ascontiguousarray(y).view(np.int64)).sum())


def host2(lib, fn, *args):
    args = [np.ascontiguousarray(a, dtype=float) for a in args]
    y = np.empty_like(args[0])
    getattr(lib, fn)(len(y), *[P(a) for a in args], P(y))
    return y


@pytest.mark.parametrize("name", list(point_sets()))
def test_device_sincos_is_the_host_build_and_within_its_bounds(lib, probe, name):
    """sincos_fast / sincos_core on the device: the host build's bits (no hardware seed in them), hence the host's bounds —
    re-asserted against x87 here: <= 1.6 ulp / 1.8e-16 (fast); 1.8e-16 absolute, 1.6 ulp where |value| > 1e-9 (core)."""
    x = np.ascontiguousarray(point_sets()[name])
    sh, sl, ch, cl = ref_sincos(lib, x)
    for sel, fn in ((SINCOS_FAST, "fm_sincos_fast"), (SINCOS_CORE, "fm_sincos_core")):
        s, c = probe(sel, x)
        hs, hc = np.empty_like(x), np.empty_like(x)
        getattr(lib, fn)(len(x), P(x), P(hs), P(hc))
        assert bitdiff(s, hs) == 0 and bitdiff(c, hc) == 0, fn
        es, ec = np.abs((s - sh) - sl), np.abs((c - ch) - cl)
        assert es.max() <= 1.8e-16 and ec.max() <= 1.8e-16, fn
        big_s, big_c = np.abs(sh) > 1e-9, np.abs(ch) > 1e-9
        assert (es[big_s] / ulp_of(sh[big_s])).max() <= 1.6 and (ec[big_c] / ulp_of(ch[big_c])).max() <= 1.6, fn
        if sel == SINCOS_FAST:
            assert (es / ulp_of(sh)).max() <= 1.6 and (ec / ulp_of(ch)).max() <= 1.6
        else:
            assert np.all(es[~big_s] <= 2e-26) and np.all(ec[~big_c] <= 2e-26)


@pytest.mark.parametrize("name", list(smxc_point_sets()))
def test_device_sin_minus_xcos_is_the_host_build_and_within_its_bound(lib, probe, name):
    """sin_minus_xcos_abs / sin_minus_xcos on the device: the host build's bits, within smxc_bound of x87's value (and of
    mpmath's on the zeros of tan x = x); sincos_poly's quadrant is the host's."""
    x = np.ascontiguousarray(smxc_point_sets()[name])
    ga, gs = probe(SMXC, x)
    assert bitdiff(ga, fm1(lib, "fm_sin_minus_xcos_abs", x)) == 0
    assert bitdiff(gs, fm1(lib, "fm_sin_minus_xcos", x)) == 0
    hi, lo = np.empty_like(x), np.empty_like(x)
    lib.fm_ref_sin_minus_xcos(len(x), P(x), P(hi), P(lo))
    b = smxc_bound(x, hi) + 4 * 2.0**-64 * (np.abs(x * np.cos(x)) + np.abs(np.sin(x)))
    assert (np.abs((gs - hi) - lo) / b).max() <= 1.0
    assert (np.abs((np.abs(ga) - np.abs(hi)) - np.sign(hi) * lo) / b).max() <= 1.0
    _, q = probe(EXPM1_Q, x)
    s0, c0, q0 = np.empty_like(x), np.empty_like(x), np.empty(len(x), dtype=np.int32)
    lib.fm_sincos_poly(len(x), P(x), P(s0), P(c0), q0.ctypes.data_as(C.POINTER(C.c_int)))
    np.testing.assert_array_equal(q, q0.astype(float))


@pytest.mark.parametrize("name", list(smxc_point_sets()))
def test_device_n_variants_are_bit_identical_to_the_scalar_forms(probe, name):
    """sincos_poly_n / sincos_core_n / sin_minus_xcos_abs_n at N = 4 and 8, evaluated next to the scalar forms IN the device
    probe: no element of any output differs in a bit (the slots a + i b, b = -0.7 sign(a), cross quadrants)."""
    x = np.ascontiguousarray(smxc_point_sets()[name])
    n4, n8 = probe(N_VARIANTS, x, -0.7 * np.sign(x))
    assert n4.max() == 0 and n8.max() == 0, (int((n4 > 0).sum()), int((n8 > 0).sum()))


def test_device_j1_within_its_bound_and_seed_independent(lib, probe):
    """j1_fast / j1_core / the split ranges on the device: <= 5e-16 absolute against scipy's Cephes j1 (fastmath.h); the split
    ranges are j1_core's two branches bit for bit.  Where only div_fast carries a hardware seed (j1_fast; j1_core for x <= 5)
    the device bits are the host build's; above x = 5 j1_core's rsqrt_fast makes some last bits the seed's (counted, not
    asserted: see the module docstring)."""
    from scipy.special import j1
    x = j1_points()
    inv = 1.0 / x
    ref = j1(x)
    yf, yc = probe(J1, x, inv)
    ys, yl = probe(J1_SPLIT, x, inv)
    for y in (yf, yc):
        assert np.abs(y - ref).max() <= 5e-16
    sm, lg = x <= 5.0, x > 5.0
    assert bitdiff(ys[sm], yc[sm]) == 0 and bitdiff(yl[lg], yc[lg]) == 0
    assert bitdiff(yf, fm1(lib, "fm_j1_fast", x)) == 0
    hc = fm1(lib, "fm_j1_core", x)
    assert bitdiff(yc[sm], hc[sm]) == 0
    print("j1_core: device bits != host bits at %d of %d arguments above 5" % (bitdiff(yc[lg], hc[lg]), int(lg.sum())))


def div_operands(wide):
    rs = np.random.RandomState(3)
    n = 1000000
    a = rs.uniform(-1, 1, n) * 10 ** rs.uniform(-100, 100, n)
    e = 150 if wide else 30                                  # wide: the device seed's range; else what a float seed holds
    b = rs.uniform(0.5, 1, n) * 10 ** rs.uniform(-e, e, n) * rs.choice([-1, 1], n)
    x = 10 ** rs.uniform(-(6 * e // 5), 6 * e // 5, n)
    return np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(x)


@pytest.mark.parametrize("wide", [False, True], ids=["float_range", "wide"])
def test_device_div_and_rsqrt(lib, probe, wide):
    """div_fast <= 1 ulp, rsqrt_fast <= 1.5 ulp against x87 over normal-range operands (the host test's ranges, and the
    wider ones only the device seed covers: divisors 1e-150 .. 1e150, rsqrt arguments 1e-180 .. 1e180); on the host's
    ranges div_fast gives the host build's bits (its Newton-refined result does not depend on the seed); rsqrt_fast's does, in
    the last place, for some arguments: counted and printed, not asserted."""
    a, b, x = div_operands(wide)
    y, _ = probe(DIV_RSQRT, a, b)
    _, r = probe(DIV_RSQRT, x)
    hi, lo = np.empty_like(a), np.empty_like(a)
    lib.fm_ref_div(len(a), P(a), P(b), P(hi), P(lo))
    assert (np.abs((y - hi) - lo) / ulp_of(hi)).max() <= 1.0
    lib.fm_ref_rsqrt(len(x), P(x), P(hi), P(lo))
    assert (np.abs((r - hi) - lo) / ulp_of(hi)).max() <= 1.5
    if not wide:
        assert bitdiff(y, host2(lib, "fm_div_fast", a, b)) == 0
        print("rsqrt_fast: device bits != host bits at %d of %d arguments" % (bitdiff(r, fm1(lib, "fm_rsqrt_fast", x)), len(x)))


def test_device_div_fast_rounds_hard_quotients_correctly(probe):
    """div_fast on the device over hard_division_cases (quotients within 2^-54 ulp of a midpoint): correctly rounded, every one
    (tests/test_fastmath.py: after two Newton steps the reciprocal's error is far below what could move such a quotient across
    its midpoint)."""
    a, b = hard_division_cases()
    y, _ = probe(DIV_RSQRT, a, b)
    np.testing.assert_array_equal(y, a / b)


def test_device_expm1_neg_fast(lib, probe):
    """expm1_neg_fast on the device: the host build's bits, <= 2 ulp against x87 expm1l, over the host test's arguments
    (0 .. -60, the k ln2 / 2 seams and their neighbours, tiny arguments, -745 and -800)."""
    rs = np.random.RandomState(4)
    seams = np.arange(1, 80) * 0.5 * np.log(2.0)
    x = -np.concatenate([rs.uniform(0, 2.5, 600000), 10 ** rs.uniform(-300, 0, 200000), rs.uniform(2, 60, 200000),
                         seams, np.nextafter(seams, 0), np.nextafter(seams, 100), [0.0, 1e-320, 745.0, 800.0]])
    x = np.ascontiguousarray(x)
    y, _ = probe(EXPM1_Q, x)
    assert bitdiff(y, fm1(lib, "fm_expm1_neg_fast", x)) == 0
    hi, lo = np.empty_like(x), np.empty_like(x)
    lib.fm_ref_expm1(len(x), P(x), P(hi), P(lo))
    assert (np.abs((y - hi) - lo) / np.maximum(ulp_of(hi), 5e-324)).max() <= 2.0


def sphere_pairs():
    """(r, q) pairs of the sphere's hot path: q r from 1e-4 to just below 2^20 (log-spaced, r 0.1 nm .. 10 um), the doubles
    next to the zeros of tan x = x, and the largest doubles below 2^20."""
    rs = np.random.RandomState(5)
    n = 4000
    r = 10 ** rs.uniform(-10, -5, n)
    x = 10 ** rs.uniform(-4, np.log10(2.0**20 * 0.99), n)
    zr = tan_x_zeros(np.unique(np.logspace(0, np.log10(300000), 60).astype(int)))
    rz = 10 ** rs.uniform(-9, -6, len(zr))
    hr = 10 ** rs.uniform(-9, -6, 200)
    hx = np.nextafter(2.0**20, 0) * (1 - np.arange(200) * 2.0**-40)
    # q chosen so that the double product q * r is the wanted x (or its neighbour): q = x / r
    r = np.concatenate([r, rz, hr])
    q = np.concatenate([x, zr, hx]) / r
    keep = q * r < 2.0**20
    return np.ascontiguousarray(r[keep]), np.ascontiguousarray(q[keep])


def test_device_sphere_intensity_fast_n_is_intensity_fast(probe):
    """The lazy row cache's premise on its own: Contrib<SPHERE>::intensity_fast_n<4> / <8> give intensity_fast's bits for
    every element (q_i = q (1 + i/16), q3inv_i the library's 1 / (q q q)), at w = 1 (c = 0) and w != 1 (c = 2/3)."""
    r, q = sphere_pairs()
    keep = q * 1.5 * r < 2.0**20
    r, q = r[keep], q[keep]
    for c in (0.0, 0.6666666):
        n4, n8 = probe(SPHERE_N, r, q, c)
        assert n4.max() == 0 and n8.max() == 0, (c, int((n4 > 0).sum()), int((n8 > 0).sum()))

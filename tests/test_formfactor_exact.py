"""Form-factor rows of the device against exact references of the same discrete operation.

The reference's models evaluate closed formulas (and, for the orientation- or contour-averaged ones, a fixed quadrature) in
doubles; the kernels evaluate the same expressions in another order with fastmath.h.  Here both are held to the EXACT value of
that discrete operation — the formula at the doubles the reference feeds it (q r rounded, the quadrature nodes numpy.linspace
makes), evaluated in 40-digit mpmath — and each device row must lie within a bound DERIVED from the kernel's operation order by
a running error analysis (class R of tests/exact.py): every value carries the exact (mpmath) result and a bound on what a double evaluation in the
kernel's order may be off by,

    a +- b: e_a + e_b + u|a +- b|            a b: |a| e_b + |b| e_a + e_a e_b + u|a b|         u = 2^-53 (one rounding)
    a / b: (e_a + |a/b| e_b) / (|b| - e_b) + u|a/b|    (div_fast: 2u, its <= 1 ulp)          fma: one rounding of the sum
    sqrt a: e_a / (sqrt a + sqrt(a - e_a)) + u sqrt a
    sin, cos (fastmath.h sincos_fast / _core, |x| < 2^20): |f'| e_x + 1.6 ulp + 2e-26;  libm (|x| >= 2^20, and the tables'
      sin / cos): 2 ulp;  j1_fast: |J1'| e_x (|J1'| <= 1) + 5e-16;  expm1, pow (device libm): 2 ulp

so a bound is the stated fastmath error plus one rounding per operation, propagated through the formula's own condition: the
sphere's sin x - x cos x, for one, carries an absolute error of order u |x cos x|, not u |sin x - x cos x|.  The kernel is not
asked to beat the reference's formula (the replays depend on evaluating the same expression), only to stay inside what that
formula allows.  The intensities are taken at compensation exponent 0 (w = volume^0 = 1), so a row is F^2 itself."""
import mpmath as mp
import numpy as np
import pytest

import mcsas_amd
from mcsas_amd import engine
from helpers import FakeData
from exact import R, U, check, div_fast, fma, j1, libm1, sincos
from test_fastmath import tan_x_zeros

pytestmark = pytest.mark.gpu

mp.mp.dps = 40


def rows_of(model, q, pset):
    q = np.ascontiguousarray(q, dtype=float)
    return engine.model_calc(model.setup(FakeData(q)), q, np.ascontiguousarray(pset, dtype=float), 0.0, want_rows=True)[4]


# ------------------------------------------------------------------------------------------------- the closed-form models

def sphere_f(x):
    """models.h Sphere::intensity: div_fast(3 fma(-x, cos x, sin x), x x x) at the double x = q r."""
    x = R(x)
    s, c = sincos(x)
    return div_fast(3.0 * fma(-x, c, s), (x * x) * x)


def sphere_hot_f(q, r):
    """Sphere::intensity_fast: (3 sin_minus_xcos_abs(x)) (q3inv invr3) at x = fl(q r); |sin_minus_xcos_abs| carries the error
    of fma(-x, cos x, sin x) (fastmath.h).  q3inv invr3 against 1 / x^3: 3 roundings in the library's q3inv = 1 / (q q q),
    3 in invr3 = 1 / (r r r), 1 in their product, and x^-3 = (q r)^-3 (1 + d)^-3 with |d| <= u: 10 u (+ second order)."""
    x = R(float(np.float64(q) * np.float64(r)))
    s, c = sincos(x)
    g = fma(-x, c, s)
    g = R(abs(g.v), g.e)
    k = R(1 / x.v**3, 10.1 * U / abs(float(x.v))**3)
    return (3.0 * g) * k


def sq(f):
    return f * f


def sphere_radii():
    return (1e-10, 1e-9, 3.3e-8, 1e-6)        # 1 nm and 1000 nm: the ends of Sphere's preset active range


def x_grid():
    """q r from 1e-4 to 1e9 (through the 2^20 hand-off to the libm branch), the doubles around 2^20, and next to the zeros of
    tan x = x (the zeros of the form factor)."""
    return np.concatenate([np.logspace(-4, 9, 60), np.nextafter(2.0**20, 0) * (1 - np.arange(4) * 2.0**-50),
                           2.0**20 * (1 + np.arange(3) * 2.0**-52), tan_x_zeros(np.array([1, 2, 7, 40, 333, 5000, 300000]))])


def test_sphere_rows_against_exact():
    """Sphere rows (model_calc: Contrib::intensity, sincos_fast + div_fast, libm beyond q r = 2^20) within the derived bound."""
    m = mcsas_amd.Sphere()
    worst = 0.0
    for r in sphere_radii():
        q = x_grid() / r
        got = rows_of(m, q, [[r]])[0]
        worst = max(worst, check(got, [sq(sphere_f(float(qq * r))) for qq in q], "sphere r=%g" % r))
    print("sphere: worst error / bound %.3g" % worst)


def test_sphere_hot_path_against_exact():
    """Contrib<SPHERE>::intensity_fast (every chain mode's row) and intensity (model_calc's), through the device probe of
    tests/test_fastmath_device.py, within their derived bounds, q r from 1e-4 to just below 2^20 and next to the zeros."""
    from test_fastmath_device import probe_model, sphere_pairs, SPHERE
    setup = probe_model().setup()
    r, q = sphere_pairs()
    pick = np.random.RandomState(6).choice(len(r), 1500, replace=False)
    r, q = r[pick], q[pick]
    q3 = 1.0 / (q * q * q)                                      # mcsas_hip.hip: hq3[i] = 1.0 / (hq[i] * hq[i] * hq[i])
    rows = np.stack([r, np.full_like(r, SPHERE), q, q3], axis=1)
    _, fast, _, slow = engine.model_calc(setup, np.array([1.0]), np.ascontiguousarray(rows), 0.0)
    wf = check(fast, [sq(sphere_hot_f(qq, rr)) for qq, rr in zip(q, r)], "intensity_fast")
    ws = check(slow, [sq(sphere_f(float(qq * rr))) for qq, rr in zip(q, r)], "intensity")
    print("sphere intensity_fast: worst error / bound %.3g; intensity %.3g (%d points)" % (wf, ws, len(r)))


def test_spherical_core_shell_rows_against_exact():
    """Core-shell sphere (models.h SPH_CS::intensity) at the ends of its preset active range (core radius 0.1 nm .. 1 um)
    and shell thicknesses from its range, within the derived bound."""
    m = mcsas_amd.SphericalCoreShell()
    m.t.setActive(True)
    eta_c, eta_s, eta_sol = (float(p()) for p in m.params()[2:5])
    worst = 0.0
    for r, t in ((1e-10, 1e-10), (1e-10, 1e-6), (1e-6, 1e-10), (1e-6, 1e-6), (5e-9, 2e-9)):
        rt = r + t
        q = np.logspace(-4, 8, 50) / rt
        got = rows_of(m, q, [[r, t]])[0]
        ref = []
        for qq in q:
            xs, xc = R(float(qq * rt)), R(float(qq * r))
            vc = R(4. / 3) * np.pi * ((R(r) * r) * r)
            vt = R(4. / 3) * np.pi * ((R(rt) * rt) * rt)
            vr = vc / vt
            ds, dc = R(eta_s) - eta_sol, R(eta_s) - eta_c
            sn, cs = sincos(xs)
            ks = div_fast((ds * 3.0) * (sn - xs * cs), (xs * xs) * xs)
            sn, cs = sincos(xc)
            kc = div_fast((dc * 3.0) * (sn - xc * cs), (xc * xc) * xc)
            ref.append(sq(ks - vr * kc))
        worst = max(worst, check(got, ref, "core-shell r=%g t=%g" % (r, t)))
    print("spherical core-shell: worst error / bound %.3g" % worst)


def test_gaussian_chain_rows_against_exact():
    """Gaussian chain (GAUSS_CHAIN::intensity: sqrt(2) sqrt(expm1(-u) + u) / u beta, u = (q rg)^2) at the ends of the preset
    active ranges of rg, bp, etas and k, q rg from 1e-4 to 1e4, within the derived bound (expm1(-u) + u cancels at small u)."""
    m = mcsas_amd.GaussianChain()
    for p in m.params():
        p.setActive(True)
    worst = 0.0
    for rg, bp, etas, k in ((1e-9, 1e-10, 1e19, 0.1), (1e-7, 1e-6, 1e21, 10.), (1e-9, 1e-6, 1e21, 0.1), (3e-8, 1e-7, 1e20, 1.)):
        q = np.logspace(-4, 4, 40) / rg
        got = rows_of(m, q, [[rg, bp, etas, k]])[0]
        ref = []
        for qq in q:
            x = R(float(qq * rg))
            u = x * x
            vol = R(k) * (R(rg) * rg)
            beta = R(bp) - vol * etas
            f = (R(float(np.sqrt(2.))) * (libm1(mp.expm1, -u) + u).sqrt()) / u
            ref.append(sq(f * beta))
        worst = max(worst, check(got, ref, "gaussian chain %r" % ((rg, bp, etas, k),)))
    print("gaussian chain: worst error / bound %.3g" % worst)


def test_lma_dense_sphere_rows_against_exact():
    """LMA dense spheres (LMA_SPHERE::intensity: sphere form factor times the Percus-Yevick S(q)) at volume fractions from the
    ends of the parameter's range, mf = -1 (auto: pow) and a fixed standoff, within the derived bound.  G(A) of S cancels
    like 1/A^5 at small A: the bound there is the formula's, as wide as it must be."""
    m = mcsas_amd.LMADenseSphere()
    m.volFrac.setActive(True)
    worst = 0.0
    for r, mu, mf in ((1e-9, 1e-5, -1.0), (1e-9, 0.3, -1.0), (2e-8, 0.55, 1.2), (1e-7, 0.05, -1.0)):
        m.mf.setValue(mf)
        q = np.logspace(-2, 6, 40) / r
        got = rows_of(m, q, [[r, mu]])[0]
        ref = []
        M = R(mu)
        mfr = (libm1(lambda t: t ** mp.mpf(1. / 3), R(0.634) / M)) if mf == -1.0 else R(mf)
        rh = mfr * r
        om = (((1. - M) * (1. - M)) * (1. - M)) * (1. - M)
        al = ((1. + 2. * M) * (1. + 2. * M)) / om
        be = (((-6. * M) * (1. + M / 2.)) * (1. + M / 2.)) / om
        ga = (M * al) / 2.
        for qq in q:
            x = R(float(qq * r))
            sn, cs = sincos(x)
            f = div_fast(3. * (sn - x * cs), (x * x) * x)
            A = R(2. * qq) * rh
            sn, cs = sincos(A)
            A2 = A * A
            A3, A4 = A2 * A, A2 * A2
            A5 = A4 * A
            G = (al * (sn - A * cs)) / A2 \
                + (be * ((((2. * A) * sn) + (2. - A2) * cs) - 2.)) / A3 \
                + (ga * ((-1. * A4) * cs + 4. * ((((3. * A2 - 6.) * cs) + (A3 - 6. * A) * sn) + 6.))) / A5
            S = 1. / (1. + ((24. * M) * G) / A)
            ref.append(sq(((f * f) * S).sqrt()))
        worst = max(worst, check(got, ref, "lma r=%g mu=%g mf=%g" % (r, mu, mf)))
    print("lma dense sphere: worst error / bound %.3g" % worst)


# ------------------------------------------------------------------------------- the orientation / contour-averaged models

def test_cylinder_rows_against_exact():
    """Isotropic cylinders (CYL_ISO::intensity: trapezoid over numpy.linspace(0, 1, intDiv) with the analytic end columns) at
    the radius / aspect ends of test_cylinders_at_the_ends_of_the_aspect_range, intDiv = 100, the sum taken exactly over the
    same nodes; a modest point set (mpmath is slow)."""
    m = mcsas_amd.CylindersIsotropic()
    m.aspect.setActive(True)
    K = 100
    step = 1.0 / (K - 1)
    xk = np.arange(K) * step
    xk[-1] = 1.0
    xk[0] = xk[-1] = 0.5
    sk = np.sqrt(1. - xk * xk)                                  # fill_table: the same doubles
    q = np.logspace(7, np.log10(3e9), 6)
    worst = 0.0
    for r, asp in ((1e-10, 1e-3), (1e-10, 1e3), (1e-7, 1e-3), (1e-7, 1e3), (7.3e-9, 1.0)):
        got = rows_of(m, q, [[r, asp]])[0]
        hl = float(np.float64(r) * asp)
        ref = []
        for qq in q:
            qr, qh = R(float(qq * r)), R(float(qq * hl))
            f0 = 0.5 * (j1(qr) / qr)
            sq_, _ = sincos(qh)
            fl = sq_ / qh
            prev, acc = f0 * f0, R(0.0)
            for k in range(1, K - 1):
                qrs = R(qq) * float(np.float64(r) * sk[k])
                qlx = R(qq) * float((2. * hl) * xk[k])
                sl, _ = sincos(qlx * 0.5)
                f = (j1(qrs) * sl) / (qrs * qlx)
                cur = f * f
                acc = acc + (cur + prev)
                prev = cur
            acc = acc + (fl * fl + prev)
            ff = (16. * ((acc * step) * 0.5)).sqrt()
            ref.append(ff * ff)
        worst = max(worst, check(got, ref, "cylinder r=%g aspect=%g" % (r, asp)))
    print("cylinders: worst error / bound %.3g" % worst)


def test_isotropic_ellipsoid_rows_against_exact():
    """Isotropic ellipsoids (ELL_ISO::intensity: mean over alpha = numpy.linspace(0, pi/2, intDiv) of F_sphere(q R(alpha))^2
    sin(alpha)) at the aspect ends, intDiv = 100, the sum taken exactly over the same nodes (the table's sin / cos are the device
    libm's: 2 ulp each)."""
    m = mcsas_amd.EllipsoidsIsotropic()
    m.aspect.setActive(True)
    K = 100
    step = (np.pi / 2.) / (K - 1)
    al = np.arange(K) * step
    al[-1] = np.pi / 2.
    tabs = [sincos(R(float(a)), libm=True) for a in al]
    t0 = [s * s for s, _ in tabs]
    t1 = [c * c for _, c in tabs]
    q = np.logspace(7, np.log10(3e9), 6)
    worst = 0.0
    for ra, asp in ((1e-10, 1e-3), (1e-10, 1e3), (1e-6, 1e-3), (1e-7, 1e3), (4e-9, 2.5)):
        got = rows_of(m, q, [[ra, asp]])[0]
        rc = float(np.float64(ra) * asp)
        ra2, rc2 = R(ra) * ra, R(rc) * rc
        invK = 1.0 / R(float(K))
        ref = []
        for qq in q:
            acc = R(0.0)
            for k in range(K):
                x = R(qq) * (ra2 * t0[k] + rc2 * t1[k]).sqrt()
                sn, cs = sincos(x)
                f = div_fast(3. * (sn - x * cs), (x * x) * x)
                acc = acc + (f * f) * tabs[k][0]
            ff = (acc * invK).sqrt()
            ref.append(ff * ff)
        worst = max(worst, check(got, ref, "ellipsoid a=%g aspect=%g" % (ra, asp)))
    print("isotropic ellipsoids: worst error / bound %.3g" % worst)


def test_core_shell_ellipsoid_rows_against_exact():
    """Core-shell ellipsoids (ELL_CS::intensity: mean over mu = numpy.linspace(0, 1, intDiv) of the squared core + shell
    amplitude) at the ends of the preset active ranges of a, b and t, intDiv = 100, summed exactly over the same nodes."""
    m = mcsas_amd.EllipsoidalCoreShell()
    m.b.setActive(True)
    m.t.setActive(True)
    eta_c, eta_s, eta_sol = (float(p()) for p in m.params()[3:6])
    K = 100
    step = 1.0 / (K - 1)
    mu = np.arange(K) * step
    mu[-1] = 1.0
    m2, n2 = mu * mu, 1. - mu * mu
    q = np.logspace(7, np.log10(3e9), 5)
    worst = 0.0
    for a, b, t in ((1e-10, 1e-9, 1e-10), (1e-6, 1e-5, 1e-6), (1e-10, 1e-5, 1e-10), (2e-9, 3e-8, 1e-9)):
        got = rows_of(m, q, [[a, b, t]])[0]
        A, B, T = R(a), R(b), R(t)
        vc = ((R(4. / 3) * np.pi) * A) * (B * B)
        vt = ((R(4. / 3) * np.pi) * (A + T)) * ((B + T) * (B + T))
        c1 = (R(eta_c) - eta_s) * (vc / vt)
        c2 = (R(eta_s) - eta_sol) * 1.
        a2, b2, at2, bt2 = A * A, B * B, (A + T) * (A + T), (B + T) * (B + T)
        invK = 1.0 / R(float(K))
        ref = []
        for qq in q:
            acc = R(0.0)
            for k in range(K):
                xc = R(qq) * (a2 * float(m2[k]) + b2 * float(n2[k])).sqrt()
                xt = R(qq) * (at2 * float(m2[k]) + bt2 * float(n2[k])).sqrt()
                sc, cc = sincos(xc)
                st, ct = sincos(xt)
                jc = div_fast(sc - xc * cc, xc * xc)
                jt = div_fast(st - xt * ct, xt * xt)
                f = c1 * div_fast(3. * jc, xc) + c2 * div_fast(3. * jt, xt)
                acc = acc + f * f
            ff = (acc * invK).sqrt()
            ref.append(ff * ff)
        worst = max(worst, check(got, ref, "core-shell ellipsoid %r" % ((a, b, t),)))
    print("core-shell ellipsoids: worst error / bound %.3g" % worst)

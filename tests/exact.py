"""Exact values with derived error bounds: shared by the modules that hold device arithmetic to the EXACT value of the discrete
operation it performs (test_formfactor_exact.py; test_fit_exact_host.py, test_fit_exact_gpu.py through fit_exact.py;
test_hist_exact_host.py, test_hist_exact_gpu.py through hist_exact.py).  A plain module like helpers.py: nothing in here is
collected.

A value of class R carries the exact (mpmath) result and a bound on what a double evaluation in the kernel's order may be off by
(a running error analysis):

    a +- b: e_a + e_b + u|a +- b|            a b: |a| e_b + |b| e_a + e_a e_b + u|a b|         u = 2^-53 (one rounding)
    a / b: (e_a + |a/b| e_b) / (|b| - e_b) + u|a/b|    (div_fast: 2u, its <= 1 ulp)          fma: one rounding of the sum
    sqrt a: e_a / (sqrt a + sqrt(a - e_a)) + u sqrt a
    sin, cos (fastmath.h sincos_fast / _core, |x| < 2^20): |f'| e_x + 1.6 ulp + 2e-26;  libm (|x| >= 2^20, and the tables'
      sin / cos): 2 ulp;  j1_fast: |J1'| e_x (|J1'| <= 1) + 5e-16;  expm1, pow (device libm): 2 ulp

so a bound is the stated fastmath error plus one rounding per operation, propagated through the formula's own condition.  The
library is compiled with -ffp-contract=off (csrc/Makefile): a multiply-add is fused only where the source says fma(), and the
number of roundings of an expression is the number of its operations in the source.

The sums over q (reduced_sum) follow the kernels' order, DESIGN §3: q-point i of a wave lives in lane i & 63, slot i >> 6; a lane
adds its slots one after the other, the 64 lane totals are added pairwise in six levels (device_util.h wave_sum3), and the q-split
kernel adds the totals of its waves in wave order (chain_wide.h wide_sum3).  Class V is R for a whole vector of terms at once:
magnitudes and bounds as numpy doubles (a term of these sums is a product of data, it does not cancel), the exact sum of the
terms being taken separately in mpmath."""
import math

import mpmath as mp
import numpy as np

U = 2.0**-53
ULP_SINCOS, ABS_SINCOS, ULP_LIBM, ABS_J1 = 1.6, 2e-26, 2.0, 5e-16
WAVE = 64


class R:
    """An exact value (mpmath) and a bound on the error of its double evaluation in the kernel's order (module docstring)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = mp.mpf(v), float(e)

    @staticmethod
    def _r(v):
        return U * abs(float(v))

    def __add__(self, o):
        o = o if isinstance(o, R) else R(o)
        v = self.v + o.v
        return R(v, self.e + o.e + self._r(v))

    def __radd__(self, o):
        return self + o

    def __sub__(self, o):
        o = o if isinstance(o, R) else R(o)
        v = self.v - o.v
        return R(v, self.e + o.e + self._r(v))

    def __rsub__(self, o):
        return R(o) - self

    def __neg__(self):
        return R(-self.v, self.e)

    def __mul__(self, o):
        o = o if isinstance(o, R) else R(o)
        v = self.v * o.v
        return R(v, abs(float(self.v)) * o.e + abs(float(o.v)) * self.e + self.e * o.e + self._r(v))

    def __rmul__(self, o):
        return R(o) * self

    def div(self, o, ulps=0.5):
        o = o if isinstance(o, R) else R(o)
        v = self.v / o.v
        room = abs(float(o.v)) - o.e
        e = (self.e + abs(float(v)) * o.e) / room if room > 0 else math.inf
        return R(v, e + 2 * ulps * self._r(v))

    def __truediv__(self, o):
        return self.div(o)

    def __rtruediv__(self, o):
        return R(o).div(self)

    def sqrt(self):
        v = mp.sqrt(self.v)
        lo = max(float(self.v) - self.e, 0.0)
        return R(v, self.e / (float(v) + math.sqrt(lo)) + self._r(v) if float(v) > 0 else math.sqrt(self.e))


def fma(a, b, c):
    a, b, c = (x if isinstance(x, R) else R(x) for x in (a, b, c))
    v = a.v * b.v + c.v
    return R(v, abs(float(a.v)) * b.e + abs(float(b.v)) * a.e + a.e * b.e + c.e + R._r(v))


def div_fast(a, b):
    return (a if isinstance(a, R) else R(a)).div(b, ulps=1.0)


def sincos(x, libm=None):
    """sincos_fast (|x| < 2^20; its libm branch above) or, libm=True, the device libm's sin / cos."""
    s, c = mp.sin(x.v), mp.cos(x.v)
    if libm is None:
        libm = abs(float(x.v)) >= 2.0**20
    k, a = (ULP_LIBM, 0.0) if libm else (ULP_SINCOS, ABS_SINCOS)
    d2 = x.e * x.e / 2
    return (R(s, abs(float(c)) * x.e + d2 + 2 * k * R._r(s) + a), R(c, abs(float(s)) * x.e + d2 + 2 * k * R._r(c) + a))


def j1(x):
    v = mp.besselj(1, x.v)
    return R(v, x.e + ABS_J1 + R._r(v))


def libm1(f, x):
    """a device libm function of one argument (expm1): 2 ulp, propagated through its derivative (numerically, in mpmath)."""
    v = f(x.v)
    return R(v, abs(float(mp.diff(f, x.v))) * x.e + 2 * 2 * R._r(v))


def check(got, ref, what):
    """got[i] within ref[i].e of ref[i].v; returns the worst error / bound."""
    worst = 0.0
    for i, (g, r) in enumerate(zip(np.ravel(got), np.ravel(ref))):
        err = abs(mp.mpf(float(g)) - r.v)
        assert float(err) <= r.e, "%s [%d]: got %r, exact %s, error %.3g > bound %.3g" % (what, i, g, mp.nstr(r.v, 20), float(err), r.e)
        if r.e > 0 and math.isfinite(r.e):
            worst = max(worst, float(err) / r.e)
    return worst


# ------------------------------------------------------------------------------------------------- vectors of terms, and their sums
class V:
    """R for a vector of terms: |value| and error bound per element as numpy doubles, the same rules (module docstring).  Only
    products and quotients: the terms of the weighted sums do not cancel, so a double is magnitude enough for a bound."""
    __slots__ = ("a", "e")

    def __init__(self, a, e=0.0):
        self.a = np.abs(np.asarray(a, dtype=float))
        self.e = np.broadcast_to(np.asarray(e, dtype=float), self.a.shape).copy()

    def times(self, o, rounded=True):
        """the product; rounded=False where it is the product inside an fma, which the sum's own rounding covers"""
        o = o if isinstance(o, V) else V(o)
        a = self.a * o.a
        return V(a, self.a * o.e + o.a * self.e + self.e * o.e + (U * a if rounded else 0.0))

    def __mul__(self, o):
        return self.times(o)

    def __rtruediv__(self, num):
        """num / self for an exact double `num` (1.0 / (e e)): one correctly rounded division."""
        a = abs(float(num)) / self.a
        room = self.a - self.e
        return V(a, np.where(room > 0, a * self.e / np.where(room > 0, room, 1.0), np.inf) + U * a)


def slots_of(nq):
    """q slots per lane of one wave over nq points: the loop `for (k = lane; k < nq; k += WAVE)` runs this often in lane 0."""
    return -(-int(nq) // WAVE)


def sum_roundings(slots, waves=1):
    """Rounded additions on the longest path from a term to the reduced sum, read off the source:
      slots - 1   a lane's accumulation `s += t` / `s = fma(x, y, s)` over its slots, the first onto 0.0 being exact
                  (chain_body.inc: `s1 += wt; s2 = fma(wt, test[j], s2); s3 = fma(CHAIN_WI(j), test[j], s3);`, host_calls.hip
                  bgfit_kernel: `sw += w; si += w * I[k]; ...`) — where the source has fma the product is not rounded on its own
                  and the term's bound carries no rounding for it; where it has `s += x * y` the product's rounding is the term's
      6           device_util.h wave_sum3: `a += dpp_f64<0xB1>(a)` ... `a += dpp_f64<0x143, 0xC>(a)`, six lines, one add each
      waves - 1   chain_wide.h wide_sum3: `for (v = 0; v < NW; ++v) t1 += slot[v * 4 + 0]`, the first onto 0.0 being exact
    A host loop `S += t` over n terms (host_internal.h WeighedData) is sum_roundings_sequential(n)."""
    return (int(slots) - 1) + 6 + (int(waves) - 1)


def sum_roundings_sequential(n):
    """host_internal.h WeighedData: `Sw += wi; SI += wi * I; SII += wi * I * I` over the nq points in order, the first onto 0.0
    exact: n - 1 rounded additions on the path of the first term."""
    return max(int(n) - 1, 0)


def gamma(k):
    """k roundings compounded: (1 + u)^k - 1 <= k u / (1 - k u)."""
    return k * U / (1.0 - k * U)


def reduced_sum(exact, terms, roundings):
    """The sum of `terms` (a V; `exact` their exact sum, mpmath) as a kernel accumulates it through `roundings` rounded additions
    on its longest path: every computed term t^ = t + d, |d| <= e, goes through at most that many roundings, so the sum is off by
    at most sum e + gamma(roundings) sum (|t| + e)."""
    e = float(np.sum(terms.e)) + gamma(roundings) * float(np.sum(terms.a + terms.e))
    return R(exact, e)

// Host build of mcsas_amd/csrc/fastmath.h for tests/test_fastmath.py (CPU test infrastructure only).
// The header is written for both sides (MCSAS_HD); on the host the hardware reciprocal seeds are replaced
// by float-precision stand-ins, everything else is the arithmetic the kernels execute (fma = one rounding).
#include "../../mcsas_amd/csrc/fastmath.h"
#include <math.h>

// the N-wide variants over n arguments in groups of N (the caller pads n to a multiple of N)
template <int N>
static void poly_n(int n, const double *x, double *s, double *c, int *q) {
    for (int i = 0; i + N <= n; i += N) {
        double xx[N], ss[N], cc[N];
        int qq[N];
        for (int j = 0; j < N; ++j) xx[j] = x[i + j];
        mcsas::sincos_poly_n<N>(xx, ss, cc, qq);
        for (int j = 0; j < N; ++j) { s[i + j] = ss[j]; c[i + j] = cc[j]; q[i + j] = qq[j]; }
    }
}
template <int N>
static void core_n(int n, const double *x, double *s, double *c) {
    for (int i = 0; i + N <= n; i += N) {
        double xx[N], ss[N], cc[N];
        for (int j = 0; j < N; ++j) xx[j] = x[i + j];
        mcsas::sincos_core_n<N>(xx, ss, cc);
        for (int j = 0; j < N; ++j) { s[i + j] = ss[j]; c[i + j] = cc[j]; }
    }
}
template <int N>
static void smxc_abs_n(int n, const double *x, double *g) {
    for (int i = 0; i + N <= n; i += N) {
        double xx[N], gg[N];
        for (int j = 0; j < N; ++j) xx[j] = x[i + j];
        mcsas::sin_minus_xcos_abs_n<N>(xx, gg);
        for (int j = 0; j < N; ++j) g[i + j] = gg[j];
    }
}

extern "C" {
void fm_sincos_fast(int n, const double *x, double *s, double *c) { for (int i = 0; i < n; ++i) mcsas::sincos_fast(x[i], s + i, c + i); }
void fm_sincos_core(int n, const double *x, double *s, double *c) { for (int i = 0; i < n; ++i) mcsas::sincos_core(x[i], s + i, c + i); }
void fm_sincos_poly(int n, const double *x, double *s, double *c, int *q) { for (int i = 0; i < n; ++i) mcsas::sincos_poly(x[i], s + i, c + i, q + i); }
void fm_sin_minus_xcos_abs(int n, const double *x, double *y) { for (int i = 0; i < n; ++i) y[i] = mcsas::sin_minus_xcos_abs(x[i]); }
void fm_sin_minus_xcos(int n, const double *x, double *y) { for (int i = 0; i < n; ++i) y[i] = mcsas::sin_minus_xcos(x[i]); }
// what sin_minus_xcos(_abs) is documented to equal: fma(-x, cos x, sin x) with sin x, cos x from sincos_core
void fm_sin_minus_xcos_via_core(int n, const double *x, double *y) {
    for (int i = 0; i < n; ++i) { double s, c; mcsas::sincos_core(x[i], &s, &c); y[i] = fma(-x[i], c, s); }
}
void fm_sincos_poly_n4(int n, const double *x, double *s, double *c, int *q) { poly_n<4>(n, x, s, c, q); }
void fm_sincos_poly_n8(int n, const double *x, double *s, double *c, int *q) { poly_n<8>(n, x, s, c, q); }
void fm_sincos_core_n4(int n, const double *x, double *s, double *c) { core_n<4>(n, x, s, c); }
void fm_sincos_core_n8(int n, const double *x, double *s, double *c) { core_n<8>(n, x, s, c); }
void fm_sin_minus_xcos_abs_n4(int n, const double *x, double *g) { smxc_abs_n<4>(n, x, g); }
void fm_sin_minus_xcos_abs_n8(int n, const double *x, double *g) { smxc_abs_n<8>(n, x, g); }
void fm_j1_fast(int n, const double *x, double *y) { for (int i = 0; i < n; ++i) y[i] = mcsas::j1_fast(x[i]); }
void fm_j1_core(int n, const double *x, double *y) { for (int i = 0; i < n; ++i) y[i] = mcsas::j1_core(x[i], 1.0 / x[i]); }
void fm_j1_core_small(int n, const double *x, double *y) { for (int i = 0; i < n; ++i) y[i] = mcsas::j1_core_small(x[i]); }
void fm_j1_core_large(int n, const double *x, double *y) { for (int i = 0; i < n; ++i) y[i] = mcsas::j1_core_large(x[i], 1.0 / x[i]); }
void fm_div_fast(int n, const double *a, const double *b, double *y) { for (int i = 0; i < n; ++i) y[i] = mcsas::div_fast(a[i], b[i]); }
void fm_expm1_neg_fast(int n, const double *x, double *y) { for (int i = 0; i < n; ++i) y[i] = mcsas::expm1_neg_fast(x[i]); }
void fm_ref_expm1(int n, const double *x, double *hi, double *lo) {
    for (int i = 0; i < n; ++i) { const long double q = expm1l((long double)x[i]); hi[i] = (double)q; lo[i] = (double)(q - (long double)hi[i]); }
}
void fm_rsqrt_fast(int n, const double *x, double *y) { for (int i = 0; i < n; ++i) y[i] = mcsas::rsqrt_fast(x[i]); }
// references in x87 extended precision (64-bit significand): error 2^-64 relative, far below half an ulp of double
void fm_ref_sincos(int n, const double *x, double *s_hi, double *s_lo, double *c_hi, double *c_lo) {
    for (int i = 0; i < n; ++i) {
        const long double s = sinl((long double)x[i]), c = cosl((long double)x[i]);
        s_hi[i] = (double)s; s_lo[i] = (double)(s - (long double)s_hi[i]);
        c_hi[i] = (double)c; c_lo[i] = (double)(c - (long double)c_hi[i]);
    }
}
// sin x - x cos x in x87: absolute error <= ~3 * 2^-64 (|sin x| + |x cos x|), 2^-12 of what the bound of the double
// evaluation allows at any x (tests/test_fastmath.py derives it from the same two magnitudes)
void fm_ref_sin_minus_xcos(int n, const double *x, double *hi, double *lo) {
    for (int i = 0; i < n; ++i) {
        const long double X = x[i], q = sinl(X) - X * cosl(X);
        hi[i] = (double)q; lo[i] = (double)(q - (long double)hi[i]);
    }
}
void fm_ref_div(int n, const double *a, const double *b, double *hi, double *lo) {
    for (int i = 0; i < n; ++i) { const long double q = (long double)a[i] / (long double)b[i]; hi[i] = (double)q; lo[i] = (double)(q - (long double)hi[i]); }
}
void fm_ref_rsqrt(int n, const double *x, double *hi, double *lo) {
    for (int i = 0; i < n; ++i) { const long double q = 1.0L / sqrtl((long double)x[i]); hi[i] = (double)q; lo[i] = (double)(q - (long double)hi[i]); }
}
int fm_long_double_digits(void) { return __LDBL_MANT_DIG__; }
}

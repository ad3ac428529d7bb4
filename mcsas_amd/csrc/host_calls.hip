// host_calls.hip — the one-call entry points of libmcsas_hip.so and their kernels: model.calc, the background / scaling fit,
// observability, McSAS.histogram() and the input preparation (uncertainty floor, re-binning).  Nothing here knows about plans.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "host_internal.h"
#include "small_kernels.h"   // model_rows_kernel, observability_kernel, hist_rows_kernel
#include "model_list.h"      // MCSAS_FOR_MODELS: the built-in models

using namespace mcsas;

// ------------------------------------------------------------------------------ small kernels
// cumInt += it, contribution by contribution (scatteringmodel.py:101): thread per q, fixed order
__global__ void rows_cumsum_kernel(int nq, int n, const double *rows, double *cum) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nq) return;
    double s = 0.;
    for (int i = 0; i < n; ++i) s += rows[(size_t)i * nq + k];
    cum[k] = s;
}

// BackgroundScalingFit.calc with the closed-form minimiser; one wave
__global__ __launch_bounds__(64) void bgfit_kernel(int nq, const double *I, const double *sigma, const double *C,
                                                   int find_bg, int pos_bg, int num_params, double *out) {
    const int lane = threadIdx.x;
    double sw = 0, si = 0, sii = 0, sc = 0, scc = 0, sic = 0, ss2 = 0;
    for (int k = lane; k < nq; k += WAVE) {
        double e = sigma[k] == 0.0 ? 1.0 : sigma[k];       // backgroundscalingfit.py:117
        double w = 1.0 / (e * e);
        sw += w; si += w * I[k]; sii += w * I[k] * I[k];
        sc += w * C[k]; scc += w * C[k] * C[k]; sic += w * I[k] * C[k]; ss2 += e * e;
    }
    wave_sum3(sw, si, sii); wave_sum3(sc, scc, sic); ss2 = wave_sum(ss2);
    ChainArgs a{};
    a.Sw = sw; a.SI = si; a.SII = sii; a.nq = nq; a.find_bg = find_bg; a.pos_bg = pos_bg;
    FitResult f = solve_fit(a, sc, scc, sic);
    double rs = 0, r2 = 0;
    for (int k = lane; k < nq; k += WAVE) {
        double e = sigma[k] == 0.0 ? 1.0 : sigma[k];
        double r = I[k] - (C[k] * f.A + f.b);
        rs += (r / e) * (r / e); r2 += r * r;
    }
    rs = wave_sum(rs); r2 = wave_sum(r2);
    if (lane == 0) {
        out[0] = f.A; out[1] = f.b; out[2] = rs / nq;
        out[3] = r2 / ss2 * ((double)nq / (double)(nq - num_params));   // aGoFsAlpha :79-84, :136-138
    }
}

// ------------------------------------------------------------------------------ histogram(), batched
// per rep: cumInt = sum of its rows in contribution order (scatteringmodel.py:101), then the closed-form
// scale/background fit (mcsas.py:559); one wave per rep
__global__ __launch_bounds__(64) void hist_fit_kernel(int nq, const double *I, const double *sigma, int N, int R, int r0,
                                                      const double *rows, int find_bg, int pos_bg, double *scaling) {
    const int rl = blockIdx.x, r = r0 + rl, lane = threadIdx.x;
    const double *base = rows + (size_t)rl * N * nq;
    double sw = 0, si = 0, sii = 0, sc = 0, scc = 0, sic = 0;
    for (int k = lane; k < nq; k += WAVE) {
        double C = 0.;
        for (int n = 0; n < N; ++n) C += base[(size_t)n * nq + k];
        const double e = sigma[k] == 0.0 ? 1.0 : sigma[k];
        const double w = 1.0 / (e * e);
        sw += w; si += w * I[k]; sii += w * I[k] * I[k];
        sc += w * C; scc += w * C * C; sic += w * I[k] * C;
    }
    wave_sum3(sw, si, sii); wave_sum3(sc, scc, sic);
    ChainArgs a{};
    a.Sw = sw; a.SI = si; a.SII = sii; a.nq = nq; a.find_bg = find_bg; a.pos_bg = pos_bg;
    const FitResult f = solve_fit(a, sc, scc, sic);
    if (lane == 0) { scaling[r] = f.A; scaling[R + r] = f.b; }
}

// ---- McSAS.histogram() on the device (mcsas_hip_histogram, mcsas_hip_histogram_batch) --------------------------------------------
// The arithmetic of each kernel is a device function of one (data set, repetition): the single call's kernel hands it its own
// arguments, the batch kernel (further down) what its set's record says.

// min over q of sigma*vf / (A*I_c(q)), I_c != 0 (mcsas.py:582-590) from the stored row of contribution c of repetition r
__device__ __forceinline__ void hist_obs_body(int nq, const double *sigma, int R, int c, int r, const double *row, const double *scaling,
                                              const double *vset, const double *wset, double *min_req) {
    const double A = scaling[r];
    const double vf = wset[(size_t)c * R + r] * A / vset[(size_t)c * R + r];      // modeldata.py:57-61
    double best = INFINITY;
    for (int k = threadIdx.x; k < nq; k += WAVE) {
        const double scaled = A * row[k];
        if (scaled != 0.) best = fmin(best, (sigma[k] * vf) / scaled);
    }
    best = wave_min(best);
    if (threadIdx.x == 0) min_req[(size_t)c * R + r] = best;
}
__global__ __launch_bounds__(64) void hist_obs_kernel(int nq, const double *sigma, int N, int R, int r0, const double *rows,
                                                      const double *scaling, const double *vset, const double *wset,
                                                      double *min_req) {
    const int c = blockIdx.x, rl = blockIdx.y, r = r0 + rl;
    hist_obs_body(nq, sigma, R, c, r, rows + ((size_t)rl * N + c) * nq, scaling, vset, wset, min_req);
}

// cum[k] = sum_n rows[n][k] of one repetition in contribution order (scatteringmodel.py:101): one thread per q, loads in batches of 8
__device__ __forceinline__ void hist_colsum_body(int nq, int N, int k, const double *rows, double *cum) {
    if (k >= nq) return;
    const double *base = rows + k;
    double s = 0.;
    int n = 0;
    for (; n + 8 <= N; n += 8) {
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = base[(size_t)(n + i) * nq];
#pragma unroll
        for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; n < N; ++n) s += base[(size_t)n * nq];
    cum[k] = s;
}
__global__ void hist_colsum_kernel(int nq, int N, const double *rows, double *cum) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, rl = blockIdx.y;
    hist_colsum_body(nq, N, k, rows + (size_t)rl * N * nq, cum + (size_t)rl * nq);
}
// hist_fit_kernel with the summed intensity of repetition r given (same sums in the same order): one wave
__device__ __forceinline__ void hist_fit_cum_body(int nq, const double *I, const double *sigma, int R, int r, const double *cum,
                                                  int find_bg, int pos_bg, double *scaling) {
    const int lane = threadIdx.x;
    double sw = 0, si = 0, sii = 0, sc = 0, scc = 0, sic = 0;
    for (int k = lane; k < nq; k += WAVE) {
        const double C = cum[k];
        const double e = sigma[k] == 0.0 ? 1.0 : sigma[k];
        const double w = 1.0 / (e * e);
        sw += w; si += w * I[k]; sii += w * I[k] * I[k];
        sc += w * C; scc += w * C * C; sic += w * I[k] * C;
    }
    wave_sum3(sw, si, sii); wave_sum3(sc, scc, sic);
    ChainArgs a{};
    a.Sw = sw; a.SI = si; a.SII = sii; a.nq = nq; a.find_bg = find_bg; a.pos_bg = pos_bg;
    const FitResult f = solve_fit(a, sc, scc, sic);
    if (lane == 0) { scaling[r] = f.A; scaling[R + r] = f.b; }
}
__global__ __launch_bounds__(64) void hist_fit_cum_kernel(int nq, const double *I, const double *sigma, int R, int r0, const double *cum,
                                                          int find_bg, int pos_bg, double *scaling) {
    const int rl = blockIdx.x;
    hist_fit_cum_body(nq, I, sigma, R, r0 + rl, cum + (size_t)rl * nq, find_bg, pos_bg, scaling);
}
// fractions and their visibility limits, normalised per repetition (mcsas.py:561-604): frac8 = [vf nf qf sf | mv mn mq ms][N][R].
// One wave per rep; the three totals are taken by one lane each, over the contributions in order (builtin sum()).
__device__ __forceinline__ void hist_fractions_body(int N, int R, int r, const double *scaling, const double *vset, const double *wset,
                                                    const double *sset, const double *mv, double *frac8) {
    __shared__ double tot[3];
    const int lane = threadIdx.x;
    const size_t NR = (size_t)N * R;
    const double A = scaling[r];
    double *vf = frac8, *nf = frac8 + NR, *qf = frac8 + 2 * NR, *sf = frac8 + 3 * NR;
    double *omv = frac8 + 4 * NR, *mn = frac8 + 5 * NR, *mq = frac8 + 6 * NR, *ms = frac8 + 7 * NR;
    for (int c = lane; c < N; c += WAVE) {
        const size_t i = (size_t)c * R + r;
        const double v = vset[i], w = wset[i], s = sset[i], m = mv[i];
        const double vfc = w * A / v;                          // modeldata.py:57-61
        const double nfc = vfc / v, mnc = m / v;               // mcsas.py:567-571, :591-594
        vf[i] = vfc; nf[i] = nfc; qf[i] = vfc * v; sf[i] = nfc * s;
        omv[i] = m; mn[i] = mnc; mq[i] = mnc * m * m; ms[i] = mnc * s;
    }
    __syncthreads();
    if (lane < 3) {
        const double *src = lane == 0 ? nf : (lane == 1 ? qf : sf);
        double t = 0.;
        for (int c = 0; c < N; ++c) t += src[(size_t)c * R + r];
        tot[lane] = t;
    }
    __syncthreads();
    const double tn = tot[0], tq = tot[1], ts = tot[2];
    for (int c = lane; c < N; c += WAVE) {
        const size_t i = (size_t)c * R + r;
        if (tn != 0.) { nf[i] /= tn; mn[i] /= tn; }           // :596-604
        if (tq != 0.) { qf[i] /= tq; mq[i] /= tq; }
        if (ts != 0.) { sf[i] /= ts; ms[i] /= ts; }
    }
}
__global__ __launch_bounds__(64) void hist_fractions_kernel(int N, int R, const double *scaling, const double *vset, const double *wset,
                                                            const double *sset, const double *mv, double *frac8) {
    hist_fractions_body(N, R, blockIdx.x, scaling, vset, wset, sset, mv, frac8);
}
struct HistSpecDev { int32_t pidx, weight, nb, pad; int64_t edge_off, out_off; double lo, hi; };
// One wave per (histogram, repetition).  The repetition's parameter values, fractions and limits are staged in LDS (hl: 3 N doubles);
// lane b owns bin b (64 bins per pass) and walks the contributions in order; the cumulative distribution and the moments are
// sequential sums again, taken by one lane (two for skew and kurtosis).  utils/parameter.py:84-122, :441-479.
__device__ __forceinline__ void hist_bins_body(int N, int P, int R, int r, const HistSpecDev s, const double *contribs, const double *frac8,
                                               const double *edges_all, double *out, double *hl) {
    __shared__ double mom[8];
    const int lane = threadIdx.x, nb = s.nb;
    const size_t NR = (size_t)N * R;
    const double *fr = frac8 + (size_t)s.weight * NR, *lim = frac8 + (size_t)(4 + s.weight) * NR;
    const double *edges = edges_all + s.edge_off;
    double *bins = out + s.out_off, *obs = bins + (size_t)nb * R, *cdf = obs + (size_t)nb * R, *mo = cdf + (size_t)nb * R;
    double *lx = hl, *lf = hl + N, *ll = hl + 2 * (size_t)N;
    for (int c = lane; c < N; c += WAVE) {
        lx[c] = contribs[((size_t)c * P + s.pidx) * R + r];
        lf[c] = fr[(size_t)c * R + r]; ll[c] = lim[(size_t)c * R + r];
    }
    __syncthreads();
    const double last = nb > 0 ? edges[nb] : 0.;
    for (int b0 = 0; b0 < nb; b0 += WAVE) {
        const int b = b0 + lane;
        if (b < nb) {
            const double elo = edges[b], ehi = edges[b + 1];
            double sb = 0., so = 0., cnt = 0.;
            for (int c = 0; c < N; ++c) {
                const double x = lx[c];
                if (x >= elo && x < ehi && x < last) { sb += lf[c]; so += ll[c]; cnt += 1.; }
            }
            bins[(size_t)b * R + r] = (sb != sb) ? 0. : sb;    // bins[isnan(bins)] = 0
            obs[(size_t)b * R + r] = cnt > 0. ? so / cnt : 0.;
        }
    }
    __syncthreads();
    if (lane == 0) {
        double run = 0., top = -__builtin_inf();
        for (int b = 0; b < nb; ++b) { run += bins[(size_t)b * R + r]; cdf[(size_t)b * R + r] = run; top = fmax(top, run); }
        for (int b = 0; b < nb; ++b) cdf[(size_t)b * R + r] = (top == 0.) ? 0. : cdf[(size_t)b * R + r] / top;
    }
    // moments: total, mean, variance by lane 32 (runs beside lane 0's distribution), then skew / kurtosis by lanes 32 / 33
    if (lane == 32) {
        double tot = 0., m1 = 0.;
        int any = 0;
        for (int c = 0; c < N; ++c) { const double x = lx[c]; const bool ok = x > s.lo && x < s.hi; any |= ok; tot += ok ? lf[c] : 0.; }
        for (int c = 0; c < N; ++c) { const double x = lx[c]; const bool ok = x > s.lo && x < s.hi; m1 += ok ? x * lf[c] : 0.; }
        if (tot != 0.) m1 /= tot;
        double v2 = 0.;
        for (int c = 0; c < N; ++c) { const double x = lx[c], d = x - m1; const bool ok = x > s.lo && x < s.hi; v2 += ok ? (d * d) * lf[c] : 0.; }
        const double var = v2 / tot, sg = sqrt(fabs(var));
        mom[0] = tot; mom[1] = m1; mom[2] = var; mom[3] = sg; mom[4] = (double)any;
    }
    __syncthreads();
    if (lane == 32 || lane == 33) {
        const double tot = mom[0], m1 = mom[1], sg = mom[3];
        const bool any = mom[4] != 0., ok3 = any && (tot * sg) != 0.;      // (utils/parameter.py:106-107: only an exact zero is skipped; NaN goes on)
        const double sg2 = sg * sg;
        double acc = 0.;
        for (int c = 0; c < N; ++c) {
            const double x = lx[c], d = x - m1, d2 = d * d;
            const bool ok = x > s.lo && x < s.hi;
            acc += ok ? (lane == 32 ? d2 * d : d2 * d2) * lf[c] : 0.;
        }
        const double val = ok3 ? acc / (tot * (lane == 32 ? sg2 * sg : sg2 * sg2)) : 0.;
        mo[(size_t)(3 + (lane - 32)) * R + r] = val;
        if (lane == 32) { mo[r] = any ? tot : 0.; mo[(size_t)R + r] = any ? m1 : 0.; mo[(size_t)2 * R + r] = any ? mom[2] : 0.; }
    }
}
__global__ __launch_bounds__(64) void hist_bins_kernel(int N, int P, int R, const double *contribs, const double *frac8, const double *edges_all,
                                                       const HistSpecDev *specs, double *out) {
    extern __shared__ double hl[];
    hist_bins_body(N, P, R, blockIdx.y, specs[blockIdx.x], contribs, frac8, edges_all, out, hl);
}

// ---- the same for a batch of data sets (mcsas_hip_histogram_batch): one launch each over the (set, repetition) blocks of a chunk.
// A set's record (HistSetDev, small_kernels.h) says where its arrays lie in the packed upload `in`, the packed download `back` and
// the scratch blocks; blockIdx.x picks the (set, repetition), blockIdx.y runs to the chunk's largest extent (contributions, q blocks,
// histograms): a block beyond its own set's returns on its index alone, ahead of any barrier.
struct HistSetView {
    const HistSetDev &s;
    const int r;
    const size_t NR;
    __device__ HistSetView(const HistSetDev *sets, const ChainRef *blocks)
        : s(sets[__builtin_amdgcn_readfirstlane(blocks[blockIdx.x].set)]), r(__builtin_amdgcn_readfirstlane(blocks[blockIdx.x].rep)),
          NR((size_t)s.N * s.R) {}
    __device__ double *scaling(double *back) const { return back + s.back_off; }
    __device__ double *frac8(double *back) const { return back + s.back_off + 2 * (size_t)s.R; }
    __device__ double *out(double *back) const { return back + s.back_off + 2 * (size_t)s.R + 8 * NR; }
};
__global__ void hist_colsum_batch_kernel(const HistSetDev *__restrict__ sets, const ChainRef *__restrict__ blocks, const double *rows, double *cum) {
    const HistSetView v(sets, blocks);
    const HistSetDev &s = v.s;
    if ((int)(blockIdx.y * blockDim.x) >= s.nq) return;
    hist_colsum_body(s.nq, s.N, blockIdx.y * blockDim.x + threadIdx.x, rows + s.rows_off + (size_t)v.r * s.N * s.nq, cum + s.cum_off + (size_t)v.r * s.nq);
}
__global__ __launch_bounds__(64) void hist_fit_cum_batch_kernel(const HistSetDev *__restrict__ sets, const ChainRef *__restrict__ blocks,
                                                                const double *__restrict__ in, const double *cum, double *back) {
    const HistSetView v(sets, blocks);
    const HistSetDev &s = v.s;
    hist_fit_cum_body(s.nq, in + s.I_off, in + s.sg_off, s.R, v.r, cum + s.cum_off + (size_t)v.r * s.nq, s.find_bg, s.pos_bg, v.scaling(back));
}
__global__ __launch_bounds__(64) void hist_obs_batch_kernel(const HistSetDev *__restrict__ sets, const ChainRef *__restrict__ blocks,
                                                            const double *__restrict__ in, const double *rows, const double *back, double *vws) {
    const HistSetView v(sets, blocks);
    const HistSetDev &s = v.s;
    const int c = blockIdx.y;
    if (c >= s.N) return;
    double *w = vws + s.vws_off;
    hist_obs_body(s.nq, in + s.sg_off, s.R, c, v.r, rows + s.rows_off + ((size_t)v.r * s.N + c) * s.nq, back + s.back_off, w, w + v.NR, w + 3 * v.NR);
}
__global__ __launch_bounds__(64) void hist_fractions_batch_kernel(const HistSetDev *__restrict__ sets, const ChainRef *__restrict__ blocks,
                                                                  const double *vws, double *back) {
    const HistSetView v(sets, blocks);
    const HistSetDev &s = v.s;
    const double *w = vws + s.vws_off;
    hist_fractions_body(s.N, s.R, v.r, v.scaling(back), w, w + v.NR, w + 2 * v.NR, w + 3 * v.NR, v.frac8(back));
}
// histograms [h0, h0 + gridDim.y) of every set that has that many
__global__ __launch_bounds__(64) void hist_bins_batch_kernel(const HistSetDev *__restrict__ sets, const ChainRef *__restrict__ blocks, int h0,
                                                             const double *__restrict__ in, double *back) {
    extern __shared__ double hl[];
    const HistSetView v(sets, blocks);
    const HistSetDev &s = v.s;
    const int h = h0 + blockIdx.y;
    if (h >= s.n_hist) return;
    const HistSpecDev *specs = reinterpret_cast<const HistSpecDev *>(in + s.spec_off);
    hist_bins_body(s.N, s.P, s.R, v.r, specs[h], in + s.c_off, v.frac8(back), in + s.edge_off, v.out(back), hl);
}

// ------------------------------------------------------------------------------ input preparation
// DataObj._prepareUncertainty (dataobj/dataobj.py:204-227)
__global__ void prepare_uncertainty_kernel(int n, const double *I, const double *su, double fu_min, double *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double floor_u = fu_min * I[i];
    double u = su ? fmax(su[i], floor_u) : floor_u;          // numpy.maximum propagates NaN; fmax would not:
    if (su && (su[i] != su[i] || floor_u != floor_u)) u = NAN;
    out[i] = isfinite(u) ? u : INFINITY;
}

// DataObj._reBin (dataobj/dataobj.py:319-337): one wavefront per bin
__global__ __launch_bounds__(64) void rebin_kernel(int n, const double *x, const double *f, const double *fu,
                                                   const double *edges, double *xb, double *fb, double *ub, int32_t *cnt_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double lo = edges[b], hi = edges[b + 1];
    double cnt = 0., sx = 0., sf = 0., su2 = 0., x1 = 0., f1 = 0., u1 = 0.;
    for (int i = lane; i < n; i += WAVE) {
        const double xi = x[i];
        if (xi >= lo && xi < hi) { cnt += 1.; sx += xi; sf += f[i]; su2 += fu[i] * fu[i]; x1 = xi; f1 = f[i]; u1 = fu[i]; }
    }
    const double mine = cnt;
    cnt = wave_sum(cnt); sx = wave_sum(sx); sf = wave_sum(sf); su2 = wave_sum(su2);
    const int c = (int)cnt;
    if (c == 1) {                                          // the lane that holds the point copies it (:327-329)
        if (mine == 1.) { xb[b] = x1; fb[b] = f1; ub[b] = u1; }
    } else if (c > 1) {
        const double mf = sf / cnt;
        double ss = 0.;
        for (int i = lane; i < n; i += WAVE) {
            const double xi = x[i];
            if (xi >= lo && xi < hi) { const double dlt = f[i] - mf; ss += dlt * dlt; }
        }
        ss = wave_sum(ss);
        if (lane == 0) {
            xb[b] = sx / cnt; fb[b] = mf;
            const double sem = sqrt(ss / (cnt - 1.)) / sqrt(cnt), prop = sqrt(su2 / cnt);
            ub[b] = (sem != sem || prop != prop) ? NAN : fmax(sem, prop);     // numpy.maximum
        }
    }
    if (lane == 0) cnt_out[b] = c;
}

// ------------------------------------------------------------------------------ model.calc
extern "C" int mcsas_hip_model_calc(const mcsas_problem *p, const double *pset, int32_t n, double *cum_int,
                                    double *vset, double *wset, double *sset, double *rows) {
    if (!p || n < 1 || !p->q || p->nq < 1 || (!pset && p->n_active > 0)) return fail(MCSAS_EINVAL, "bad argument");
    ModelArgs m;
    int rc = fill_model_args(p, &m);
    if (rc) return rc;
    DeviceGuard dev_guard;
    rc = select_device(p->device);
    if (rc) return rc;
    const size_t Q = p->nq, P = p->n_active;                 // P == 0: every row is the model at its fixed values
    DevBuf<double> dq, dp, dr, dv, dw, ds, dc;
    HIPCHK(dq.alloc(Q)); HIPCHK(dp.alloc(n * P)); HIPCHK(dr.alloc((size_t)n * Q));
    HIPCHK(dv.alloc(n)); HIPCHK(dw.alloc(n)); HIPCHK(ds.alloc(n)); HIPCHK(dc.alloc(Q));
    HIPCHK(hipMemcpy(dq.p, p->q, sizeof(double) * Q, hipMemcpyHostToDevice));
    if (P > 0) HIPCHK(hipMemcpy(dp.p, pset, sizeof(double) * n * P, hipMemcpyHostToDevice));
    SmearDev smear;
    rc = smear.upload(p, p->nq, &m);
    if (rc) return rc;
    size_t lds = sizeof(double) * table_doubles_host(p->model_id, m.int_div);
    switch (p->model_id) {
#define CASE_K(mm) case mm: model_rows_kernel<mm><<<n, WAVE, lds>>>(m, p->nq, dq.p, dp.p, n, dr.p, dv.p, dw.p, ds.p); break;
        MCSAS_FOR_MODELS(CASE_K)
#undef CASE_K
        default:
            if (!is_plugin_model(p->model_id)) return fail(MCSAS_EINVAL, "model %d", p->model_id);
            rc = plugin_small_launch(p->model_id, PLUGIN_MODEL_ROWS, dim3(n), lds, m, (int)p->nq, (const double *)dq.p, (const double *)dp.p, (int)n, dr.p, dv.p, dw.p, ds.p);
            if (rc) return rc;
    }
    HIPCHK(hipGetLastError());
    rows_cumsum_kernel<<<(p->nq + 255) / 256, 256>>>(p->nq, n, dr.p, dc.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    if (cum_int) HIPCHK(hipMemcpy(cum_int, dc.p, sizeof(double) * Q, hipMemcpyDeviceToHost));
    if (vset) HIPCHK(hipMemcpy(vset, dv.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (wset) HIPCHK(hipMemcpy(wset, dw.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (sset) HIPCHK(hipMemcpy(sset, ds.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (rows) HIPCHK(hipMemcpy(rows, dr.p, sizeof(double) * n * Q, hipMemcpyDeviceToHost));
    return MCSAS_OK;
}

extern "C" int mcsas_hip_bgfit(int32_t nq, const double *I, const double *sigma, const double *C, int32_t find_bg,
                               int32_t pos_bg, int32_t num_params, int32_t device, double out[4]) {
    if (nq < 1 || !I || !sigma || !C || !out) return fail(MCSAS_EINVAL, "bad argument");
    DeviceGuard dev_guard;
    int rc = select_device(device);
    if (rc) return rc;
    DevBuf<double> dI, dS, dC, dO;
    HIPCHK(dI.alloc(nq)); HIPCHK(dS.alloc(nq)); HIPCHK(dC.alloc(nq)); HIPCHK(dO.alloc(4));
    HIPCHK(hipMemcpy(dI.p, I, sizeof(double) * nq, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dS.p, sigma, sizeof(double) * nq, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dC.p, C, sizeof(double) * nq, hipMemcpyHostToDevice));
    bgfit_kernel<<<1, WAVE>>>(nq, dI.p, dS.p, dC.p, find_bg != 0, pos_bg != 0, num_params, dO.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dO.p, sizeof(double) * 4, hipMemcpyDeviceToHost));
    return MCSAS_OK;
}

extern "C" int mcsas_hip_observability(const mcsas_problem *p, const double *contribs, const double *scaling,
                                       const double *vol_frac, double *min_req_vol) {
    if (!p || !contribs || !scaling || !vol_frac || !min_req_vol || !p->q || !p->sigma) return fail(MCSAS_EINVAL, "bad argument");
    ModelArgs m;
    int rc = fill_model_args(p, &m);
    if (rc) return rc;
    DeviceGuard dev_guard;
    rc = select_device(p->device);
    if (rc) return rc;
    const size_t Q = p->nq, P = p->n_active, N = p->n_contrib, R = p->n_reps;
    DevBuf<double> dq, dsg, dc, dsc, dvf, dm;
    HIPCHK(dq.alloc(Q)); HIPCHK(dsg.alloc(Q)); HIPCHK(dc.alloc(N * P * R)); HIPCHK(dsc.alloc(R));
    HIPCHK(dvf.alloc(N * R)); HIPCHK(dm.alloc(N * R));
    HIPCHK(hipMemcpy(dq.p, p->q, sizeof(double) * Q, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsg.p, p->sigma, sizeof(double) * Q, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dc.p, contribs, sizeof(double) * N * P * R, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsc.p, scaling, sizeof(double) * R, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dvf.p, vol_frac, sizeof(double) * N * R, hipMemcpyHostToDevice));
    SmearDev smear;
    rc = smear.upload(p, p->nq, &m);
    if (rc) return rc;
    size_t lds = sizeof(double) * table_doubles_host(p->model_id, m.int_div);
    dim3 grid((unsigned)N, (unsigned)R);
    switch (p->model_id) {
#define CASE_K(mm) case mm: observability_kernel<mm><<<grid, WAVE, lds>>>(m, p->nq, dq.p, dsg.p, (int)N, (int)R, dc.p, dsc.p, dvf.p, dm.p); break;
        MCSAS_FOR_MODELS(CASE_K)
#undef CASE_K
        default: {
            if (!is_plugin_model(p->model_id)) return fail(MCSAS_EINVAL, "model %d", p->model_id);
            int rcp = plugin_small_launch(p->model_id, PLUGIN_OBSERVABILITY, grid, lds, m, (int)p->nq, (const double *)dq.p, (const double *)dsg.p, (int)N, (int)R,
                                          (const double *)dc.p, (const double *)dsc.p, (const double *)dvf.p, dm.p);
            if (rcp) return rcp;
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(min_req_vol, dm.p, sizeof(double) * N * R, hipMemcpyDeviceToHost));
    return MCSAS_OK;
}

// hist_rows_kernel of the problem's model for repetitions [r0, r0 + grid.y) on the null stream (both histogram entry points)
static int launch_hist_rows(const mcsas_problem *p, const ModelArgs &m, dim3 grid, size_t lds, const double *dq, int N, int R, int r0,
                            const double *dc, double *drows, double *dv, double *dw, double *ds) {
    switch (p->model_id) {
#define CASE_K(mm) case mm: hist_rows_kernel<mm><<<grid, WAVE, lds>>>(m, p->nq, dq, N, R, r0, dc, drows, dv, dw, ds); break;
        MCSAS_FOR_MODELS(CASE_K)
#undef CASE_K
        default: {
            if (!is_plugin_model(p->model_id)) return fail(MCSAS_EINVAL, "model %d", p->model_id);
            int rcp = plugin_small_launch(p->model_id, PLUGIN_HIST_ROWS, grid, lds, m, (int)p->nq, dq, N, R, r0, dc, drows, dv, dw, ds);
            if (rcp) return rcp;
        }
    }
    HIPCHK(hipGetLastError());
    return MCSAS_OK;
}

extern "C" int mcsas_hip_histogram_prep(const mcsas_problem *p, const double *contribs, double *scaling, double *vset,
                                        double *wset, double *sset, double *min_req_vol) {
    if (!p || !contribs || !scaling || !vset || !wset || !sset || !min_req_vol || !p->q || !p->intensity || !p->sigma ||
        p->nq < 1 || p->n_contrib < 1 || p->n_reps < 1)
        return fail(MCSAS_EINVAL, "bad argument");
    ModelArgs m;
    int rc = fill_model_args(p, &m);
    if (rc) return rc;
    DeviceGuard dev_guard;
    rc = select_device(p->device);
    if (rc) return rc;
    const size_t Q = p->nq, P = p->n_active, N = p->n_contrib, R = p->n_reps;
    // the rows of a block of repetitions stay in HBM between the three kernels; blocks of at most ~8 GB
    const size_t per_rep = N * Q * sizeof(double);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(R, ((size_t)8 << 30) / per_rep));
    DevBuf<double> dq, dI, dsg, dc, drows, dsc, dv, dw, ds, dm;
    HIPCHK(dq.alloc(Q)); HIPCHK(dI.alloc(Q)); HIPCHK(dsg.alloc(Q)); HIPCHK(dc.alloc(N * P * R)); HIPCHK(drows.alloc(chunk * N * Q));
    HIPCHK(dsc.alloc(2 * R)); HIPCHK(dv.alloc(N * R)); HIPCHK(dw.alloc(N * R)); HIPCHK(ds.alloc(N * R)); HIPCHK(dm.alloc(N * R));
    HIPCHK(hipMemcpy(dq.p, p->q, sizeof(double) * Q, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dI.p, p->intensity, sizeof(double) * Q, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsg.p, p->sigma, sizeof(double) * Q, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dc.p, contribs, sizeof(double) * N * P * R, hipMemcpyHostToDevice));
    SmearDev smear;
    rc = smear.upload(p, p->nq, &m);
    if (rc) return rc;
    const size_t lds = sizeof(double) * table_doubles_host(p->model_id, m.int_div);
    for (size_t r0 = 0; r0 < R; r0 += chunk) {
        const unsigned nr = (unsigned)std::min(chunk, R - r0);
        const dim3 grid((unsigned)N, nr);
        rc = launch_hist_rows(p, m, grid, lds, dq.p, (int)N, (int)R, (int)r0, dc.p, drows.p, dv.p, dw.p, ds.p);
        if (rc) return rc;
        hist_fit_kernel<<<nr, WAVE>>>(p->nq, dI.p, dsg.p, (int)N, (int)R, (int)r0, drows.p, p->find_background != 0,
                                      p->positive_background != 0, dsc.p);
        HIPCHK(hipGetLastError());
        hist_obs_kernel<<<grid, WAVE>>>(p->nq, dsg.p, (int)N, (int)R, (int)r0, drows.p, dsc.p, dv.p, dw.p, dm.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpy(scaling, dsc.p, sizeof(double) * 2 * R, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(vset, dv.p, sizeof(double) * N * R, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(wset, dw.p, sizeof(double) * N * R, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sset, ds.p, sizeof(double) * N * R, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(min_req_vol, dm.p, sizeof(double) * N * R, hipMemcpyDeviceToHost));
    return MCSAS_OK;
}

// McSAS.histogram() complete (include/mcsas_hip.h): ONE packed upload (data vectors, parameter sets, bin edges, histogram records) from
// a pinned staging block, the kernels back to back on the null stream, ONE packed download — a call costs two transfers and no
// allocation once its block sizes have been seen (MemCache).
extern "C" int mcsas_hip_histogram(const mcsas_problem *p, const double *contribs, int32_t n_hist, const mcsas_histogram_spec *specs,
                                   double *scaling, double *fractions, double *out) {
    if (!p || !contribs || !scaling || !p->q || !p->intensity || !p->sigma || p->nq < 1 || p->n_contrib < 1 || p->n_reps < 1 || n_hist < 0 ||
        (n_hist > 0 && (!specs || !out)))
        return fail(MCSAS_EINVAL, "bad argument");
    if (p->n_contrib > 4096) return fail(MCSAS_EINVAL, "mcsas_hip_histogram stages a repetition's contributions in LDS: n_contrib %d > 4096 (use mcsas_hip_histogram_prep)", p->n_contrib);
    ModelArgs m;
    int rc = fill_model_args(p, &m);
    if (rc) return rc;
    DeviceGuard dev_guard;
    rc = select_device(p->device);
    if (rc) return rc;
    const size_t Q = p->nq, P = p->n_active, N = p->n_contrib, R = p->n_reps, NR = N * R;
    size_t n_edges = 0, n_out = 0;
    std::vector<HistSpecDev> hs((size_t)n_hist);
    for (int h = 0; h < n_hist; ++h) {
        const mcsas_histogram_spec &sp = specs[h];
        if (sp.n_bin < 0 || sp.n_bin > (1 << 20) || sp.param_index < 0 || sp.param_index >= (int)std::max<size_t>(P, 1) || sp.weighting < 0 || sp.weighting > 3 ||
            (sp.n_bin > 0 && !sp.edges) || P == 0)
            return fail(MCSAS_EINVAL, "histogram %d: param_index %d, weighting %d, n_bin %d", h, sp.param_index, sp.weighting, sp.n_bin);
        hs[h] = HistSpecDev{sp.param_index, sp.weighting, sp.n_bin, 0, (int64_t)n_edges, (int64_t)n_out, sp.lower, sp.upper};
        n_edges += (size_t)sp.n_bin + 1;
        n_out += (size_t)3 * sp.n_bin * R + 5 * R;
    }
    // staging layout (doubles): in = [q | I | sigma | contribs | edges | specs], back = [scaling 2R | fractions 8NR | out]
    const size_t spec_d = (sizeof(HistSpecDev) * (size_t)n_hist + 7) / 8;
    const size_t n_in = 3 * Q + N * P * R + n_edges + spec_d, n_back = 2 * R + 8 * NR + n_out;
    const size_t per_rep = N * Q * sizeof(double);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(R, ((size_t)8 << 30) / per_rep));
    DevBuf<double> din, dback, drows, dcum, dvws;
    HIPCHK(din.alloc(n_in)); HIPCHK(dback.alloc(n_back)); HIPCHK(drows.alloc(chunk * N * Q)); HIPCHK(dcum.alloc(chunk * Q)); HIPCHK(dvws.alloc(4 * NR));
    struct Pinned {
        double *p = nullptr; size_t bytes = 0;
        ~Pinned() { cached_host_free(p, bytes, hipHostMallocDefault); }
    } hin, hback;
    hin.bytes = sizeof(double) * n_in; hback.bytes = sizeof(double) * n_back;
    HIPCHK(cached_host_malloc((void **)&hin.p, hin.bytes, hipHostMallocDefault));
    HIPCHK(cached_host_malloc((void **)&hback.p, hback.bytes, hipHostMallocDefault));
    // every early return below leaves copies / kernels queued on the null stream: wait for them before the staging blocks above
    // (destroyed after this guard) go back to the cache, where the next call would overwrite them under the DMA
    struct SyncGuard {
        bool armed = true;
        ~SyncGuard() { if (armed) (void)hipStreamSynchronize(nullptr); }
    } sync_guard;
    double *w = hin.p;
    memcpy(w, p->q, sizeof(double) * Q); w += Q;
    memcpy(w, p->intensity, sizeof(double) * Q); w += Q;
    memcpy(w, p->sigma, sizeof(double) * Q); w += Q;
    memcpy(w, contribs, sizeof(double) * N * P * R); w += N * P * R;
    for (int h = 0; h < n_hist; ++h) { memcpy(w, specs[h].edges, sizeof(double) * ((size_t)specs[h].n_bin + 1)); w += (size_t)specs[h].n_bin + 1; }
    if (n_hist) memcpy(w, hs.data(), sizeof(HistSpecDev) * (size_t)n_hist);
    HIPCHK(hipMemcpyAsync(din.p, hin.p, hin.bytes, hipMemcpyHostToDevice, nullptr));
    const double *dq = din.p, *dI = din.p + Q, *dsg = din.p + 2 * Q, *dc = din.p + 3 * Q, *dedges = dc + N * P * R;
    const HistSpecDev *dspecs = reinterpret_cast<const HistSpecDev *>(dedges + n_edges);
    double *dsc = dback.p, *dfrac = dback.p + 2 * R, *dout = dfrac + 8 * NR;
    double *dv = dvws.p, *dw = dvws.p + NR, *ds = dvws.p + 2 * NR, *dm = dvws.p + 3 * NR;
    SmearDev smear;
    rc = smear.upload(p, p->nq, &m);
    if (rc) return rc;
    const size_t lds = sizeof(double) * table_doubles_host(p->model_id, m.int_div);
    for (size_t r0 = 0; r0 < R; r0 += chunk) {
        const unsigned nr = (unsigned)std::min(chunk, R - r0);
        const dim3 grid((unsigned)N, nr);
        rc = launch_hist_rows(p, m, grid, lds, dq, (int)N, (int)R, (int)r0, dc, drows.p, dv, dw, ds);
        if (rc) return rc;
        hist_colsum_kernel<<<dim3((unsigned)((Q + 255) / 256), nr), 256>>>(p->nq, (int)N, drows.p, dcum.p);
        HIPCHK(hipGetLastError());
        hist_fit_cum_kernel<<<nr, WAVE>>>(p->nq, dI, dsg, (int)R, (int)r0, dcum.p, p->find_background != 0, p->positive_background != 0, dsc);
        HIPCHK(hipGetLastError());
        hist_obs_kernel<<<grid, WAVE>>>(p->nq, dsg, (int)N, (int)R, (int)r0, drows.p, dsc, dv, dw, dm);
        HIPCHK(hipGetLastError());
    }
    hist_fractions_kernel<<<(unsigned)R, WAVE>>>((int)N, (int)R, dsc, dv, dw, ds, dm, dfrac);
    HIPCHK(hipGetLastError());
    if (n_hist > 0) {
        if (sizeof(double) * 3 * N > 64 * 1024)
            HIPCHK(hipFuncSetAttribute((const void *)hist_bins_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * 3 * N)));
        hist_bins_kernel<<<dim3((unsigned)n_hist, (unsigned)R), WAVE, sizeof(double) * 3 * N>>>((int)N, (int)P, (int)R, dc, dfrac, dedges, dspecs, dout);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(hback.p, dback.p, hback.bytes, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    sync_guard.armed = false;
    memcpy(scaling, hback.p, sizeof(double) * 2 * R);
    if (fractions) memcpy(fractions, hback.p + 2 * R, sizeof(double) * 8 * NR);
    if (n_out) memcpy(out, hback.p + 2 * R + 8 * NR, sizeof(double) * n_out);
    return MCSAS_OK;
}

// hist_rows_batch_kernel of built-in model `model_id` over the grid.x blocks that `dblocks` begins with
static int launch_hist_rows_batch(int model_id, dim3 grid, size_t lds, const HistSetDev *dsets, const ChainRef *dblocks, const double *din,
                                  double *drows, double *dvws) {
    switch (model_id) {
#define CASE_K(mm) case mm: hist_rows_batch_kernel<mm><<<grid, WAVE, lds>>>(dsets, dblocks, din, drows, dvws); break;
        MCSAS_FOR_MODELS(CASE_K)
#undef CASE_K
        default: return fail(MCSAS_EINVAL, "model %d has no batch kernel", model_id);
    }
    HIPCHK(hipGetLastError());
    return MCSAS_OK;
}

// the rows budget of a batch chunk: 2 GiB, or MCSAS_HIP_HIST_BATCH_MB (a number of MiB, fractions allowed) — read at every call
static size_t hist_batch_budget() {
    double mb = 2048.;
    if (const char *e = getenv("MCSAS_HIP_HIST_BATCH_MB")) { char *end = nullptr; const double v = strtod(e, &end); if (end != e && v >= 0. && v < 1e9) mb = v; }
    return (size_t)(mb * 1048576.);
}

// McSAS.histogram() of a batch of data sets (include/mcsas_hip.h).  Every refusal comes before a device is touched.  The sets are
// taken in order, in chunks whose rows fit the budget; a chunk is one launch per kernel (hist_rows: one per model in it).  A plug-in
// model's set, and one whose rows alone exceed the budget, closes the chunk before it and runs through mcsas_hip_histogram.
extern "C" int mcsas_hip_histogram_batch(int32_t n_sets, const mcsas_problem *problems, const double *const *contribs, const int32_t *n_hist,
                                         const mcsas_histogram_spec *const *specs, double *const *scaling, double *const *fractions,
                                         double *const *out) {
    if (n_sets < 0) return fail(MCSAS_EINVAL, "histogram_batch: n_sets %d", n_sets);
    if (n_sets == 0) return MCSAS_OK;
    if (!problems || !contribs || !n_hist || !specs || !scaling || !out)
        return fail(MCSAS_EINVAL, "histogram_batch: NULL table (problems, contribs, n_hist, specs, scaling and out are needed; fractions may be NULL)");
    const size_t S = (size_t)n_sets;
    struct Set { ModelArgs m; size_t n_edges = 0, n_out = 0, n_in = 0, n_back = 0, rows = 0; bool single = false; int rec = -1; };
    std::vector<Set> sets(S);
    const size_t budget = hist_batch_budget();
    for (size_t s = 0; s < S; ++s) {
        const mcsas_problem *p = &problems[s];
        const int si = (int)s, nh = n_hist[s];
        if (!contribs[s] || !scaling[s] || !p->q || !p->intensity || !p->sigma || p->nq < 1 || p->n_contrib < 1 || p->n_reps < 1 || nh < 0 ||
            (nh > 0 && (!specs[s] || !out[s])))
            return fail(MCSAS_EINVAL, "histogram_batch: set %d: bad argument", si);
        if (p->n_contrib > 4096)
            return fail(MCSAS_EINVAL, "histogram_batch: set %d: a repetition's contributions are staged in LDS: n_contrib %d > 4096 (use mcsas_hip_histogram_prep)", si, p->n_contrib);
        if (p->device != problems[0].device)
            return fail(MCSAS_EINVAL, "histogram_batch: set %d names device %d, set 0 device %d: one device per batch", si, p->device, problems[0].device);
        int rc = fill_model_args(p, &sets[s].m);
        if (!rc) rc = SmearDev::check(p);
        if (rc) { const std::string why = g_err; return fail(rc, "histogram_batch: set %d: %s", si, why.c_str()); }
        const size_t P = p->n_active, R = p->n_reps;
        for (int h = 0; h < nh; ++h) {
            const mcsas_histogram_spec &sp = specs[s][h];
            if (sp.n_bin < 0 || sp.n_bin > (1 << 20) || sp.param_index < 0 || sp.param_index >= (int)std::max<size_t>(P, 1) || sp.weighting < 0 || sp.weighting > 3 ||
                (sp.n_bin > 0 && !sp.edges) || P == 0)
                return fail(MCSAS_EINVAL, "histogram_batch: set %d: histogram %d: param_index %d, weighting %d, n_bin %d", si, h, sp.param_index, sp.weighting, sp.n_bin);
            sets[s].n_edges += (size_t)sp.n_bin + 1;
            sets[s].n_out += (size_t)3 * sp.n_bin * R + 5 * R;
        }
        const size_t Q = p->nq, N = p->n_contrib;
        sets[s].rows = N * R * Q;
        sets[s].n_in = 3 * Q + N * P * R + sets[s].n_edges + (sizeof(HistSpecDev) * (size_t)nh + 7) / 8;
        sets[s].n_back = 2 * R + 8 * N * R + sets[s].n_out;
        sets[s].single = is_plugin_model(p->model_id) || sets[s].rows * sizeof(double) > budget;
    }
    DeviceGuard dev_guard;
    int rc = select_device(problems[0].device);
    if (rc) return rc;
    // chunks of consecutive batched sets; the block table keeps a chunk's (set, repetition) entries together, grouped by model
    struct Chunk { size_t first, end; size_t blk_first = 0, n_blk = 0, rows = 0, cum = 0; };   // sets [first, end): none of them single, a single set closes a chunk
    std::vector<Chunk> chunks;
    size_t n_rec = 0, n_blk = 0, n_in = 0, n_back = 0, n_vws = 0, max_rows = 0, max_cum = 0;
    for (size_t s = 0; s < S; ++s) {
        if (sets[s].single) continue;
        const bool open = !chunks.empty() && chunks.back().end == s && (chunks.back().rows + sets[s].rows) * sizeof(double) <= budget;
        if (!open) chunks.push_back(Chunk{s, s});
        Chunk &c = chunks.back();
        c.end = s + 1; c.rows += sets[s].rows; c.cum += (size_t)problems[s].n_reps * problems[s].nq; c.n_blk += problems[s].n_reps;
        sets[s].rec = (int)n_rec++;
        n_in += sets[s].n_in; n_back += sets[s].n_back; n_vws += 4 * (size_t)problems[s].n_contrib * problems[s].n_reps;
        max_rows = std::max(max_rows, c.rows); max_cum = std::max(max_cum, c.cum);
    }
    for (Chunk &c : chunks) { c.blk_first = n_blk; n_blk += c.n_blk; }
    // staging layout (doubles): in = per batched set [q | I | sigma | contribs | edges | specs], then the records, then the block table;
    // back = per batched set [scaling 2R | fractions 8NR | out]
    const size_t rec_d = (sizeof(HistSetDev) * n_rec + 7) / 8, blk_d = (sizeof(ChainRef) * n_blk + 7) / 8;
    const size_t in_total = n_in + rec_d + blk_d;
    std::vector<SmearDev> smears(n_rec);                       // (freed after the guard below has waited for the kernels)
    DevBuf<double> din, dback, drows, dcum, dvws;
    struct Pinned {
        double *p = nullptr; size_t bytes = 0;
        ~Pinned() { cached_host_free(p, bytes, hipHostMallocDefault); }
    } hin, hback;
    if (n_rec) {
        HIPCHK(din.alloc(in_total)); HIPCHK(dback.alloc(n_back)); HIPCHK(drows.alloc(max_rows)); HIPCHK(dcum.alloc(max_cum)); HIPCHK(dvws.alloc(n_vws));
        hin.bytes = sizeof(double) * in_total; hback.bytes = sizeof(double) * n_back;
        HIPCHK(cached_host_malloc((void **)&hin.p, hin.bytes, hipHostMallocDefault));
        HIPCHK(cached_host_malloc((void **)&hback.p, hback.bytes, hipHostMallocDefault));
    }
    // as in mcsas_hip_histogram: an early return waits for what is queued before the staging blocks go back to the cache
    struct SyncGuard {
        bool armed = true;
        ~SyncGuard() { if (armed) (void)hipStreamSynchronize(nullptr); }
    } sync_guard;
    std::vector<size_t> back_off(S, 0);
    if (n_rec) {
        HistSetDev *recs = reinterpret_cast<HistSetDev *>(hin.p + n_in);
        ChainRef *blks = reinterpret_cast<ChainRef *>(hin.p + n_in + rec_d);
        size_t w = 0, b = 0, v = 0;
        for (const Chunk &c : chunks) {
            size_t rows = 0, cum = 0, nb = c.blk_first;
            for (size_t s = c.first; s < c.end; ++s) {
                const mcsas_problem *p = &problems[s];
                const size_t Q = p->nq, P = p->n_active, N = p->n_contrib, R = p->n_reps;
                const int nh = n_hist[s];
                HistSetDev &d = recs[sets[s].rec];
                memset(&d, 0, sizeof d);
                rc = smears[sets[s].rec].upload(p, p->nq, &sets[s].m);
                if (rc) return rc;
                d.model = sets[s].m;
                d.nq = (int)Q; d.N = (int)N; d.P = (int)P; d.R = (int)R; d.n_hist = nh;
                d.find_bg = p->find_background != 0; d.pos_bg = p->positive_background != 0;
                d.q_off = (int64_t)w; d.I_off = d.q_off + Q; d.sg_off = d.I_off + Q; d.c_off = d.sg_off + Q;
                d.edge_off = d.c_off + N * P * R; d.spec_off = d.edge_off + sets[s].n_edges;
                d.back_off = (int64_t)b; d.rows_off = (int64_t)rows; d.cum_off = (int64_t)cum; d.vws_off = (int64_t)v;
                double *o = hin.p + w;
                memcpy(o, p->q, sizeof(double) * Q); o += Q;
                memcpy(o, p->intensity, sizeof(double) * Q); o += Q;
                memcpy(o, p->sigma, sizeof(double) * Q); o += Q;
                memcpy(o, contribs[s], sizeof(double) * N * P * R); o += N * P * R;
                size_t e_off = 0, o_off = 0;
                HistSpecDev *hs = reinterpret_cast<HistSpecDev *>(hin.p + d.spec_off);
                for (int h = 0; h < nh; ++h) {
                    const mcsas_histogram_spec &sp = specs[s][h];
                    memcpy(o, sp.edges, sizeof(double) * ((size_t)sp.n_bin + 1)); o += (size_t)sp.n_bin + 1;
                    hs[h] = HistSpecDev{sp.param_index, sp.weighting, sp.n_bin, 0, (int64_t)e_off, (int64_t)o_off, sp.lower, sp.upper};
                    e_off += (size_t)sp.n_bin + 1; o_off += (size_t)3 * sp.n_bin * R + 5 * R;
                }
                back_off[s] = b;
                w += sets[s].n_in; b += sets[s].n_back; v += 4 * N * R; rows += sets[s].rows; cum += R * Q;
            }
            // the chunk's blocks, model by model (hist_rows runs once per model; the other kernels take the chunk whole)
            for (int mid = 0; mid < MCSAS_MODEL_COUNT; ++mid)
                for (size_t s = c.first; s < c.end; ++s)
                    if (problems[s].model_id == mid)
                        for (int r = 0; r < problems[s].n_reps; ++r) blks[nb++] = ChainRef{sets[s].rec, r};
        }
        HIPCHK(hipMemcpyAsync(din.p, hin.p, hin.bytes, hipMemcpyHostToDevice, nullptr));
    }
    const HistSetDev *dsets = reinterpret_cast<const HistSetDev *>(din.p + n_in);
    const ChainRef *dblocks = reinterpret_cast<const ChainRef *>(din.p + n_in + rec_d);
    size_t next_chunk = 0;
    for (size_t s = 0; s < S; ++s) {
        if (sets[s].single) {
            rc = mcsas_hip_histogram(&problems[s], contribs[s], n_hist[s], specs[s], scaling[s], fractions ? fractions[s] : nullptr, out[s]);
            if (rc) { const std::string why = g_err; return fail(rc, "histogram_batch: set %d: %s", (int)s, why.c_str()); }
            continue;
        }
        if (next_chunk >= chunks.size() || chunks[next_chunk].first != s) continue;       // (inside a chunk already launched)
        const Chunk &c = chunks[next_chunk++];
        const ChainRef *cb = dblocks + c.blk_first;
        size_t maxN = 0, maxQ = 0, maxH = 0;
        for (size_t t = c.first; t < c.end; ++t) {
            maxN = std::max<size_t>(maxN, problems[t].n_contrib); maxQ = std::max<size_t>(maxQ, problems[t].nq); maxH = std::max<size_t>(maxH, n_hist[t]);
        }
        size_t g_first = 0;
        for (int mid = 0; mid < MCSAS_MODEL_COUNT; ++mid) {
            size_t g_blk = 0, g_N = 0, lds = 0;
            for (size_t t = c.first; t < c.end; ++t)
                if (problems[t].model_id == mid) {
                    g_blk += problems[t].n_reps; g_N = std::max<size_t>(g_N, problems[t].n_contrib);
                    lds = std::max(lds, sizeof(double) * table_doubles_host(mid, sets[t].m.int_div));
                }
            if (!g_blk) continue;
            rc = launch_hist_rows_batch(mid, dim3((unsigned)g_blk, (unsigned)g_N), lds, dsets, cb + g_first, din.p, drows.p, dvws.p);
            if (rc) return rc;
            g_first += g_blk;
        }
        const unsigned nb = (unsigned)c.n_blk;
        hist_colsum_batch_kernel<<<dim3(nb, (unsigned)((maxQ + 255) / 256)), 256>>>(dsets, cb, drows.p, dcum.p);
        HIPCHK(hipGetLastError());
        hist_fit_cum_batch_kernel<<<nb, WAVE>>>(dsets, cb, din.p, dcum.p, dback.p);
        HIPCHK(hipGetLastError());
        hist_obs_batch_kernel<<<dim3(nb, (unsigned)maxN), WAVE>>>(dsets, cb, din.p, drows.p, dback.p, dvws.p);
        HIPCHK(hipGetLastError());
        hist_fractions_batch_kernel<<<nb, WAVE>>>(dsets, cb, dvws.p, dback.p);
        HIPCHK(hipGetLastError());
        if (maxH > 0) {
            const size_t lds = sizeof(double) * 3 * maxN;
            if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)hist_bins_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            for (size_t h0 = 0; h0 < maxH; h0 += 65535) {      // (a grid's y extent ends at 65535)
                hist_bins_batch_kernel<<<dim3(nb, (unsigned)std::min<size_t>(65535, maxH - h0)), WAVE, lds>>>(dsets, cb, (int)h0, din.p, dback.p);
                HIPCHK(hipGetLastError());
            }
        }
    }
    if (n_rec) {
        HIPCHK(hipMemcpyAsync(hback.p, dback.p, hback.bytes, hipMemcpyDeviceToHost, nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
    }
    sync_guard.armed = false;
    for (size_t s = 0; s < S; ++s) {
        if (sets[s].single) continue;
        const size_t R = problems[s].n_reps, NR = (size_t)problems[s].n_contrib * R;
        const double *b = hback.p + back_off[s];
        memcpy(scaling[s], b, sizeof(double) * 2 * R);
        if (fractions && fractions[s]) memcpy(fractions[s], b + 2 * R, sizeof(double) * 8 * NR);
        if (sets[s].n_out) memcpy(out[s], b + 2 * R + 8 * NR, sizeof(double) * sets[s].n_out);
    }
    return MCSAS_OK;
}

extern "C" int mcsas_hip_prepare_uncertainty(int32_t n, const double *intensity, const double *sigma_raw, double fu_min,
                                             int32_t device, double *sigma_out) {
    if (n < 1 || !intensity || !sigma_out) return fail(MCSAS_EINVAL, "bad argument");
    DeviceGuard dev_guard;
    int rc = select_device(device);
    if (rc) return rc;
    DevBuf<double> dI, dS, dO;
    HIPCHK(dI.alloc(n)); HIPCHK(dO.alloc(n));
    HIPCHK(hipMemcpy(dI.p, intensity, sizeof(double) * n, hipMemcpyHostToDevice));
    if (sigma_raw) { HIPCHK(dS.alloc(n)); HIPCHK(hipMemcpy(dS.p, sigma_raw, sizeof(double) * n, hipMemcpyHostToDevice)); }
    prepare_uncertainty_kernel<<<(n + 255) / 256, 256>>>(n, dI.p, sigma_raw ? dS.p : nullptr, fu_min, dO.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(sigma_out, dO.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    return MCSAS_OK;
}

extern "C" int mcsas_hip_rebin(int32_t n, const double *x, const double *f, const double *fu, int32_t n_bin,
                               const double *edges, int32_t device, double *x_out, double *f_out, double *fu_out,
                               int32_t *n_out) {
    if (n < 1 || n_bin < 1 || n_bin > 1000000 || !x || !f || !fu || !edges || !x_out || !f_out || !fu_out || !n_out)
        return fail(MCSAS_EINVAL, "bad argument");
    DeviceGuard dev_guard;
    int rc = select_device(device);
    if (rc) return rc;
    DevBuf<double> dx, df, du, de, bx, bf, bu;
    DevBuf<int32_t> bc;
    HIPCHK(dx.alloc(n)); HIPCHK(df.alloc(n)); HIPCHK(du.alloc(n)); HIPCHK(de.alloc(n_bin + 1));
    HIPCHK(bx.alloc(n_bin)); HIPCHK(bf.alloc(n_bin)); HIPCHK(bu.alloc(n_bin)); HIPCHK(bc.alloc(n_bin));
    HIPCHK(hipMemcpy(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(df.p, f, sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(du.p, fu, sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(de.p, edges, sizeof(double) * (n_bin + 1), hipMemcpyHostToDevice));
    rebin_kernel<<<n_bin, WAVE>>>(n, dx.p, df.p, du.p, de.p, bx.p, bf.p, bu.p, bc.p);
    HIPCHK(hipGetLastError());
    std::vector<double> hx(n_bin), hf(n_bin), hu(n_bin);
    std::vector<int32_t> hc(n_bin);
    HIPCHK(hipMemcpy(hx.data(), bx.p, sizeof(double) * n_bin, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hf.data(), bf.p, sizeof(double) * n_bin, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hu.data(), bu.p, sizeof(double) * n_bin, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hc.data(), bc.p, sizeof(int32_t) * n_bin, hipMemcpyDeviceToHost));
    int32_t k = 0;
    for (int b = 0; b < n_bin; ++b)                               // empty bins (and NaN means) are dropped (:339-341)
        if (hc[b] > 0 && hf[b] == hf[b]) { x_out[k] = hx[b]; f_out[k] = hf[b]; fu_out[k] = hu[b]; ++k; }
    *n_out = k;
    return MCSAS_OK;
}

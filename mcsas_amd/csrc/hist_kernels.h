// hist_kernels.h — the device text of McSAS.histogram() (include/mcsas_hip.h: mcsas_hip_histogram and its kin): the hist_*_body
// functions, the kernels of one set (the joint fit's hist_fit_sets_kernel / hist_obs_sets_kernel and the caller-filled rows'
// hist_pset_kernel / hist_take_vws_kernel among them) and the *_batch_kernel forms over the sets of a batch.  The rows are
// small_kernels.h's; the partial intensities and the joint histogram of two parameters have hist_partial_kernel.h and
// hist2d_kernel.h.  Included once, by host_hist.hip, which launches every kernel here: they are no templates, so one unit keeps them.
#pragma once
#include <cstdint>

#include "../../include/mcsas_hip.h"   // MCSAS_MAX_SETS
#include "small_kernels.h"             // HistSetDev, ChainRef, visibility_limit, solve_fit, the wave sums

using namespace mcsas;

// The arithmetic of each kernel is a device function of one (data set, repetition): the single call's kernel hands it its own
// arguments, the batch kernel (further down) what its set's record says.

// the visibility limit (visibility_limit, small_kernels.h) of contribution c of repetition r from its stored row, at the volume
// fraction its fitted scale gives it
__device__ __forceinline__ void hist_obs_body(int nq, const double *sigma, int R, int c, int r, const double *row, const double *scaling,
                                              const double *vset, const double *wset, double *min_req) {
    const double A = scaling[r];
    const double vf = wset[(size_t)c * R + r] * A / vset[(size_t)c * R + r];      // modeldata.py:57-61
    visibility_limit(nq, sigma, vf, A, [&](int k) { return row[k]; }, min_req + (size_t)c * R + r);
}
__global__ __launch_bounds__(64) void hist_obs_kernel(int nq, const double *sigma, int N, int R, int r0, const double *rows,
                                                      const double *scaling, const double *vset, const double *wset, double *min_req) {
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
// the closed-form scale / background fit (mcsas.py:559) of repetition r against its summed intensity `cum`: one wave
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
// ---- the same two for a joint fit (mcsas_hip_histogram_sets): the nq points are n_sets sets one after the other.  Where the sets begin
// goes by value and is indexed by unrolled loops alone (a run-time index would send the block to scratch); each set's fit lies in
// set_fit[2][MCSAS_MAX_SETS][R] (scales, then backgrounds), which the visibility kernel reads.
struct HistSetOffs { int32_t o[MCSAS_MAX_SETS + 1]; };        // set s: points [o[s], o[s + 1]); o[n_sets ..] = nq
// One wave per repetition.  Each set's six sums as hist_fit_cum_body forms them on the set's own points; then per set solve_fit
// (MCSAS_SETS_SCALE_PER_SET), or ONE scale A = Σ num_s / Σ den_s and b_s = (SI_s - A SC_s) / Sw_s with the centred pieces of
// chain_sets.h: set_parts (MCSAS_SETS_SCALE_SHARED; with one set solve_fit, as the chain does).  scaling[2][R] = set ref_set's pair.
__global__ __launch_bounds__(64) void hist_fit_sets_kernel(int nq, const double *I, const double *sigma, int R, int r0, const double *cum_all,
                                                           int find_bg, int n_sets, HistSetOffs off, int shared, int ref_set, double *scaling,
                                                           double *set_fit) {
    const int lane = threadIdx.x, rl = blockIdx.x, r = r0 + rl;
    const double *cum = cum_all + (size_t)rl * nq;
    double sw[MCSAS_MAX_SETS], si[MCSAS_MAX_SETS], sc[MCSAS_MAX_SETS], A[MCSAS_MAX_SETS], b[MCSAS_MAX_SETS];
    double Num = 0., Den = 0.;
#pragma unroll
    for (int s = 0; s < MCSAS_MAX_SETS; ++s) {
        sw[s] = si[s] = sc[s] = A[s] = b[s] = 0.;
        if (s < n_sets) {
            double w0 = 0, i0 = 0, ii0 = 0, c0 = 0, cc0 = 0, ic0 = 0;
            for (int k = off.o[s] + lane; k < off.o[s + 1]; k += WAVE) {
                const double C = cum[k];
                const double e = sigma[k] == 0.0 ? 1.0 : sigma[k];
                const double w = 1.0 / (e * e);
                w0 += w; i0 += w * I[k]; ii0 += w * I[k] * I[k];
                c0 += w * C; cc0 += w * C * C; ic0 += w * I[k] * C;
            }
            wave_sum3(w0, i0, ii0); wave_sum3(c0, cc0, ic0);
            if (!shared || n_sets == 1) {
                ChainArgs a{};
                a.Sw = w0; a.SI = i0; a.SII = ii0; a.nq = off.o[s + 1] - off.o[s]; a.find_bg = find_bg; a.pos_bg = 0;
                const FitResult f = solve_fit(a, c0, cc0, ic0);
                A[s] = f.A; b[s] = f.b;
            } else {
                double num = ic0, den = cc0;
                if (find_bg) { num = fma(-(i0 / w0), c0, ic0); den = fma(-(c0 * (1.0 / w0)), c0, cc0); }
                Num += num; Den += den;
                sw[s] = w0; si[s] = i0; sc[s] = c0;
            }
        }
    }
    double Aref = 0., bref = 0.;
    const double Ashared = Num / Den;
#pragma unroll
    for (int s = 0; s < MCSAS_MAX_SETS; ++s)
        if (s < n_sets) {
            if (shared && n_sets > 1) { A[s] = Ashared; b[s] = find_bg ? (si[s] - Ashared * sc[s]) / sw[s] : 0.; }
            if (s == ref_set) { Aref = A[s]; bref = b[s]; }
            if (lane == 0) { set_fit[(size_t)s * R + r] = A[s]; set_fit[((size_t)MCSAS_MAX_SETS + s) * R + r] = b[s]; }
        }
    if (lane == 0) { scaling[r] = Aref; scaling[R + r] = bref; }
}
// One wave per (contribution, repetition): visibility_limit over the points of the sets named in `visible`, each point's product taken
// with its OWN set's scale, at the volume fraction the reference scale (scaling[r]) gives the contribution.
__global__ __launch_bounds__(64) void hist_obs_sets_kernel(int nq, const double *sigma, int N, int R, int r0, const double *rows, const double *scaling,
                                                           const double *set_fit, int n_sets, HistSetOffs off, uint32_t visible, const double *vset,
                                                           const double *wset, double *min_req) {
    const int c = blockIdx.x, rl = blockIdx.y, r = r0 + rl;
    const double *row = rows + ((size_t)rl * N + c) * nq;
    const double vf = wset[(size_t)c * R + r] * scaling[r] / vset[(size_t)c * R + r];   // modeldata.py:57-61
    double best = __builtin_inf();
#pragma unroll
    for (int s = 0; s < MCSAS_MAX_SETS; ++s)
        if (s < n_sets && ((visible >> s) & 1u)) {
            const double A = set_fit[(size_t)s * R + r];
            for (int k = off.o[s] + (int)threadIdx.x; k < off.o[s + 1]; k += WAVE) {
                const double scaled = A * row[k];
                if (scaled != 0.) best = fmin(best, (sigma[k] * vf) / scaled);
            }
        }
    best = wave_min(best);
    if (threadIdx.x == 0) min_req[(size_t)c * R + r] = best;
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

// ---- a round of mcsas_hip_histogram_device_rows: n_rows = k N rows of the caller's, row rl N + c = contribution c of repetition r0 + rl.
// Plain loads and stores, one thread per element; the host reads neither buffer.
// the round's parameter sets, unclipped, in activeParams() order: pset[row][p] = contribs[c][p][r0 + rl]
__global__ void hist_pset_kernel(int N, int P, int R, int r0, size_t n_rows, const double *__restrict__ contribs, double *__restrict__ pset) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows * P) return;
    const size_t row = i / P, rl = row / N, c = row % N, p = i % P;
    pset[i] = contribs[(c * P + p) * R + r0 + rl];
}
// the round's volumes, weights and surfaces, vws[3][capacity] as the caller filled them, into the [c R + r] arrays of the kernels above
__global__ void hist_take_vws_kernel(int N, int R, int r0, size_t n_rows, size_t capacity, const double *__restrict__ vws,
                                     double *__restrict__ vset, double *__restrict__ wset, double *__restrict__ sset) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const size_t j = (i % N) * R + r0 + i / N;
    vset[j] = vws[i]; wset[j] = vws[capacity + i]; sset[j] = vws[2 * capacity + i];
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

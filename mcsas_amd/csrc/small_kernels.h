// small_kernels.h — the model-templated kernels behind ScatteringModel.calc / McSAS.histogram (mcsas_hip_model_calc,
// mcsas_hip_observability, mcsas_hip_histogram_prep, mcsas_hip_histogram and its batch form).  A header so that the run-time compiler
// instantiates them for a plug-in model as well (plugin_model.h, host_plugin.hip: PLUGIN_SMALL_EXPRS names them); the built-in models'
// instances live in host_calls.hip and host_hist.hip, which reach them through small_launch.h.  What a wave does for one parameter
// set is written once — prepared_contrib, row_intensity, visibility_limit — and each kernel is those over its own layout.
#pragma once
#include "chain_common.h"

namespace mcsas {

// I_c(q[k]) of a prepared contribution: through the smearing table where one is given and the model can be smeared (sasmodel.py:56-79)
template <int M>
__device__ __forceinline__ double row_intensity(const ModelArgs &m, const Contrib<M> &c, const double *q, int k, const double *tab) {
    if (Contrib<M>::CAN_SMEAR && m.smear_nk > 0) return smeared_intensity<M>(c, m.smear_locs_t, m.smear_cw, m.smear_nk, m.smear_stride, k, tab);
    return c.intensity(q[k], tab);
}

// What every wave of these kernels begins with: the block's table, then the contribution of the parameter set whose value p is
// params[p * stride] — pset[i][p] of model_rows_kernel (stride 1), contribs[c][p][r] of the others (stride R).
template <int M>
__device__ __forceinline__ Contrib<M> prepared_contrib(const ModelArgs &m, double *tab, const double *params, size_t stride) {
    Contrib<M>::fill_table(m, tab, threadIdx.x, WAVE);
    __syncthreads();
    double row[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
    for (int p = 0; p < m.n_active; ++p) row[p] = params[p * stride];
    Contrib<M> c;
    c.prepare(m, row);
    return c;
}

// min over q of sigma*vf / (A*I_c(q)), I_c != 0 (mcsas.py:582-590), +inf where no point is kept: one wave, `intensity(k)` being
// I_c(q[k]) — evaluated by observability_kernel, read from the stored row by hist_obs_body (hist_kernels.h)
template <class Intensity>
__device__ __forceinline__ void visibility_limit(int nq, const double *sigma, double vf, double A, Intensity intensity, double *min_req) {
    double best = __builtin_inf();
    for (int k = threadIdx.x; k < nq; k += WAVE) {
        const double scaled = A * intensity(k);
        if (scaled != 0.) best = fmin(best, (sigma[k] * vf) / scaled);
    }
    best = wave_min(best);
    if (threadIdx.x == 0) *min_req = best;
}

// rows[n][q] = SASModel.calcIntensity()[0] for contribution n (sasmodel.py:46-79); one wave per row
template <int M>
__global__ __launch_bounds__(64) void model_rows_kernel(ModelArgs m, int nq, const double *q, const double *pset,
                                                        int n, double *rows, double *vset, double *wset, double *sset) {
    extern __shared__ double tab[];
    const int i = blockIdx.x;
    const Contrib<M> c = prepared_contrib<M>(m, tab, pset + (size_t)i * m.n_active, 1);
    if (threadIdx.x == 0) { vset[i] = c.v; wset[i] = c.w; sset[i] = c.s; }
    for (int k = threadIdx.x; k < nq; k += WAVE) rows[(size_t)i * nq + k] = row_intensity<M>(m, c, q, k, tab);
}

// the visibility limit of contribution c of repetition r at the caller's volume fraction; one wave per (contribution, rep)
template <int M>
__global__ __launch_bounds__(64) void observability_kernel(ModelArgs m, int nq, const double *q, const double *sigma,
                                                           int N, int R, const double *contribs, const double *scaling,
                                                           const double *vol_frac, double *min_req) {
    extern __shared__ double tab[];
    const int c = blockIdx.x, r = blockIdx.y;
    const Contrib<M> cc = prepared_contrib<M>(m, tab, contribs + (size_t)c * m.n_active * R + r, R);
    visibility_limit(nq, sigma, vol_frac[(size_t)c * R + r], scaling[r], [&](int k) { return row_intensity<M>(m, cc, q, k, tab); },
                     min_req + (size_t)c * R + r);
}

// rows[r][c][q] = calcIntensity of contribution c of rep r, plus its v/w/s: what one wave does for (c, r), `out` being that row.
// The one text of both kernels below.
template <int M>
__device__ __forceinline__ void hist_rows_body(const ModelArgs &m, int nq, const double *q, int R, int c, int r, const double *contribs,
                                               double *out, double *vset, double *wset, double *sset) {
    extern __shared__ double tab[];
    const Contrib<M> cc = prepared_contrib<M>(m, tab, contribs + (size_t)c * m.n_active * R + r, R);
    if (threadIdx.x == 0) { vset[(size_t)c * R + r] = cc.v; wset[(size_t)c * R + r] = cc.w; sset[(size_t)c * R + r] = cc.s; }
    for (int k = threadIdx.x; k < nq; k += WAVE) out[k] = row_intensity<M>(m, cc, q, k, tab);
}

// one wave per (c, r) of one data set; rows of repetitions [r0, r0 + gridDim.y)
template <int M>
__global__ __launch_bounds__(64) void hist_rows_kernel(ModelArgs m, int nq, const double *q, int N, int R, int r0,
                                                       const double *contribs, double *rows, double *vset, double *wset,
                                                       double *sset) {
    const int c = blockIdx.x, rl = blockIdx.y, r = r0 + rl;
    hist_rows_body<M>(m, nq, q, R, c, r, contribs, rows + ((size_t)rl * N + c) * nq, vset, wset, sset);
}

// ---- a batch of data sets in one launch (mcsas_hip_histogram_batch) ---------------------------------------------------------
// One record per data set: its model, sizes and fit flags, and where its arrays lie (offsets in doubles): q | I | sigma | contribs |
// edges | histogram records in the packed upload, scaling | fractions | histograms in the packed download, rows, summed rows and
// v / w / s / limits in the scratch blocks.  Block b of a batch kernel works on repetition blocks[b].rep of set blocks[b].set
// (ChainRef, as the chain batch); a second grid dimension runs to the batch's largest extent, and a block beyond its own set's
// returns on its index alone.
struct HistSetDev {
    ModelArgs model;
    int32_t nq, N, P, R, n_hist, find_bg, pos_bg, pad;
    int64_t q_off, I_off, sg_off, c_off, edge_off, spec_off;
    int64_t back_off, rows_off, cum_off, vws_off;
};
// The smearing tables of a record are pointers read from memory; read through a constant-space view of the table the compiler
// takes them for global pointers, as it takes a kernel argument's (chain_wave.h: ConstChainArgs) — the q loop's loads stay global_*.
typedef const __attribute__((address_space(4))) HistSetDev ConstHistSetDev;

// hist_rows_kernel over the sets of ONE built-in model: grid (blocks, largest N of them), dynamic LDS the largest table
template <int M>
__global__ __launch_bounds__(64) void hist_rows_batch_kernel(const HistSetDev *__restrict__ sets, const ChainRef *__restrict__ blocks,
                                                             const double *__restrict__ in, double *rows, double *vws) {
    const ChainRef b = blocks[blockIdx.x];
    const int set = __builtin_amdgcn_readfirstlane(b.set), r = __builtin_amdgcn_readfirstlane(b.rep), c = blockIdx.y;
    ConstHistSetDev &cs = ((ConstHistSetDev *)sets)[set];
    if (c >= cs.N) return;
    ModelArgs m = sets[set].model;                             // once per block, ahead of the q loop
    m.smear_locs_t = cs.model.smear_locs_t; m.smear_cw = cs.model.smear_cw;
    const int nq = cs.nq, N = cs.N, R = cs.R;
    const size_t NR = (size_t)N * R;
    double *v = vws + cs.vws_off;
    hist_rows_body<M>(m, nq, in + cs.q_off, R, c, r, in + cs.c_off, rows + cs.rows_off + ((size_t)r * N + c) * nq, v, v + NR, v + 2 * NR);
}

}  // namespace mcsas

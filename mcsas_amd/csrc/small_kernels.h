// small_kernels.h — the model-templated kernels behind ScatteringModel.calc / McSAS.histogram (mcsas_hip_model_calc,
// mcsas_hip_observability, mcsas_hip_histogram_prep, mcsas_hip_histogram and its batch form).  A header so that the run-time compiler instantiates them for a
// plug-in model as well (plugin_model.h); the built-in models' instances live in mcsas_hip.hip.
#pragma once
#include "chain_common.h"

namespace mcsas {

// rows[n][q] = SASModel.calcIntensity()[0] for contribution n (sasmodel.py:46-79); one wave per row
template <int M>
__global__ __launch_bounds__(64) void model_rows_kernel(ModelArgs m, int nq, const double *q, const double *pset,
                                                        int n, double *rows, double *vset, double *wset, double *sset) {
    extern __shared__ double tab[];
    Contrib<M>::fill_table(m, tab, threadIdx.x, WAVE);
    __syncthreads();
    const int i = blockIdx.x;
    double row[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
    for (int p = 0; p < m.n_active; ++p) row[p] = pset[(size_t)i * m.n_active + p];
    Contrib<M> c;
    c.prepare(m, row);
    if (threadIdx.x == 0) { vset[i] = c.v; wset[i] = c.w; sset[i] = c.s; }
    for (int k = threadIdx.x; k < nq; k += WAVE) {
        double it;
        if (Contrib<M>::CAN_SMEAR && m.smear_nk > 0) it = smeared_intensity<M>(c, m.smear_locs_t, m.smear_cw, m.smear_nk, m.smear_stride, k, tab);
        else it = c.intensity(q[k], tab);
        rows[(size_t)i * nq + k] = it;
    }
}

// min over q of sigma*vf / (A*I_c(q)), I_c != 0 (mcsas.py:582-590); one wave per (contribution, rep)
template <int M>
__global__ __launch_bounds__(64) void observability_kernel(ModelArgs m, int nq, const double *q, const double *sigma,
                                                           int N, int R, const double *contribs, const double *scaling,
                                                           const double *vol_frac, double *min_req) {
    extern __shared__ double tab[];
    Contrib<M>::fill_table(m, tab, threadIdx.x, WAVE);
    __syncthreads();
    const int c = blockIdx.x, r = blockIdx.y, P = m.n_active;
    double row[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
    for (int p = 0; p < P; ++p) row[p] = contribs[((size_t)c * P + p) * R + r];
    Contrib<M> cc;
    cc.prepare(m, row);
    const double vf = vol_frac[(size_t)c * R + r], A = scaling[r];
    double best = __builtin_inf();
    for (int k = threadIdx.x; k < nq; k += WAVE) {
        double it;
        if (Contrib<M>::CAN_SMEAR && m.smear_nk > 0) it = smeared_intensity<M>(cc, m.smear_locs_t, m.smear_cw, m.smear_nk, m.smear_stride, k, tab);
        else it = cc.intensity(q[k], tab);
        double scaled = A * it;
        if (scaled != 0.) best = fmin(best, (sigma[k] * vf) / scaled);
    }
    best = wave_min(best);
    if (threadIdx.x == 0) min_req[(size_t)c * R + r] = best;
}

// rows[r][c][q] = calcIntensity of contribution c of rep r, plus its v/w/s: what one wave does for (c, r), `out` being that row.
// The one text of both kernels below.
template <int M>
__device__ __forceinline__ void hist_rows_body(const ModelArgs &m, int nq, const double *q, int R, int c, int r, const double *contribs,
                                               double *out, double *vset, double *wset, double *sset) {
    extern __shared__ double tab[];
    Contrib<M>::fill_table(m, tab, threadIdx.x, WAVE);
    __syncthreads();
    const int P = m.n_active;
    double row[MCSAS_MAX_ACTIVE] = {0., 0., 0., 0.};
    for (int p = 0; p < P; ++p) row[p] = contribs[((size_t)c * P + p) * R + r];
    Contrib<M> cc;
    cc.prepare(m, row);
    if (threadIdx.x == 0) { vset[(size_t)c * R + r] = cc.v; wset[(size_t)c * R + r] = cc.w; sset[(size_t)c * R + r] = cc.s; }
    for (int k = threadIdx.x; k < nq; k += WAVE) {
        double it;
        if (Contrib<M>::CAN_SMEAR && m.smear_nk > 0) it = smeared_intensity<M>(cc, m.smear_locs_t, m.smear_cw, m.smear_nk, m.smear_stride, k, tab);
        else it = cc.intensity(q[k], tab);
        out[k] = it;
    }
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

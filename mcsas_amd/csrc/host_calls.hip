// host_calls.hip — the small one-call entry points of libmcsas_hip.so and their kernels: model.calc, the background / scaling fit,
// observability and the input preparation (uncertainty floor, re-binning); McSAS.histogram() is host_hist.hip.  The two kernels that
// evaluate a model (model_rows_kernel, observability_kernel: small_kernels.h) are launched by model id through small_launch.h.
// Nothing here knows about plans.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "small_launch.h"    // model_rows_kernel, observability_kernel: from a model id to the instance

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
    rc = launch_small_kernel<ModelRowsFamily>(p->model_id, dim3(n), lds, m, p->nq, dq.p, dp.p, n, dr.p, dv.p, dw.p, ds.p);
    if (rc) return rc;
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
    rc = launch_small_kernel<ObservabilityFamily>(p->model_id, grid, lds, m, p->nq, dq.p, dsg.p, N, R, dc.p, dsc.p, dvf.p, dm.p);
    if (rc) return rc;
    HIPCHK(hipMemcpy(min_req_vol, dm.p, sizeof(double) * N * R, hipMemcpyDeviceToHost));
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

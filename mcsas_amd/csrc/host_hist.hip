// host_hist.hip — McSAS.histogram() on the device, the host side: the entry points mcsas_hip_histogram_prep, mcsas_hip_histogram,
// mcsas_hip_histogram_sets (the sets of a joint fit seen together), mcsas_hip_histogram_batch, mcsas_hip_histogram_device_rows (the
// rows filled by the caller), the forms of the second and the last that also return partial intensities
// (mcsas_hip_histogram_partial*) and mcsas_hip_histogram2d.  Every kernel they launch lies in a header: hist_kernels.h (the hist_*
// kernels and their batch forms), hist_partial_kernel.h, hist2d_kernel.h, and small_kernels.h for the rows.  What makes a set
// acceptable (check_hist_set), how a set lies in the staging blocks (HistSizes, pack_hist_set, unpack_hist_set) and how many
// repetitions share a block of rows (hist_rep_chunk) are each said once here, for the single call and the batch alike; how one set
// is held on the device, taken through its blocks of rows and finished (HistOnDevice: upload, run, finish) and how a bins kernel is
// launched (launch_hist_bins) once for the entry points that differ only in who fills the rows and which fit follows them.  Every
// entry point runs under no_bad_alloc.  Nothing here knows about plans.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_decide.h"          // check_hist_sets_request
#include "small_launch.h"         // hist_rows_kernel, hist_rows_batch_kernel (from a model id to the instance)
#include "hist_kernels.h"         // the hist_* kernels of one set and of a batch, HistSetOffs, HistSpecDev
#include "hist_partial_kernel.h"  // HistPartialDev, hist_partial_lds_bytes, hist_partial_kernel
#include "hist2d_kernel.h"        // Hist2dSpecDev, hist2d_staged_bytes, hist2d_shared_bytes, hist2d_kernel

using namespace mcsas;

// mcsas_hip_histogram stages a repetition's contributions in LDS (hist_bins_body: 3 N doubles); engine.HISTOGRAM_MAX_CONTRIBS
constexpr int HIST_MAX_CONTRIBS = 4096;
static_assert(HIST_PARTIAL_MAX_CONTRIBS == HIST_MAX_CONTRIBS, "hist_partial_kernel.h: the call's own cap");
static_assert(HIST2D_MAX_CONTRIBS == HIST_MAX_CONTRIBS, "hist2d_kernel.h: the 1-D cap");
// what a kernel may ask of dynamic LDS without its limit being raised first, and where a grid's y extent ends
constexpr size_t LDS_UNRAISED_MAX = 64 * 1024, GRID_Y_MAX = 65535;

// ------------------------------------------------------------------------------ one set: what is acceptable, and where it lies
// The staging blocks of a set, in doubles.  Going in: [q | I | sigma | contribs | edges | specs] — the edges of its histograms one after
// the other, then their HistSpecDev records, whose edge_off / out_off count from the set's own edges and outputs.  Coming back:
// [scaling 2R | fractions 8NR | out].  The *_off are the places of the parts in their block; the device reads the coming-back ones
// through HistSetView.  vws_back (mcsas_hip_histogram_prep): [scaling 2R | volumes, weights, surfaces, visibility limits 4NR] instead.
struct HistSizes {
    size_t n_edges = 0, n_out = 0;                             // edges and output doubles of all the set's histograms
    size_t I_off = 0, sg_off = 0, c_off = 0, edge_off = 0, spec_off = 0, n_in = 0, frac_off = 0, out_off = 0, n_back = 0;
    size_t rows = 0;                                           // the rows of all repetitions: N R Q
    bool vws_back = false;
};
// the places, once n_edges and n_out are known
static void lay_out_hist_set(HistSizes *sz, const mcsas_problem *p, int n_hist) {
    const size_t Q = p->nq, P = p->n_active, N = p->n_contrib, R = p->n_reps;
    sz->I_off = Q; sz->sg_off = 2 * Q; sz->c_off = 3 * Q; sz->edge_off = sz->c_off + N * P * R; sz->spec_off = sz->edge_off + sz->n_edges;
    sz->n_in = sz->spec_off + (sizeof(HistSpecDev) * (size_t)n_hist + 7) / 8;
    sz->frac_off = 2 * R; sz->out_off = sz->frac_off + 8 * N * R; sz->n_back = sz->out_off + sz->n_out; sz->rows = N * R * Q;
}
// a histogram's outputs: bins, observability and cumulative distribution [n_bin][R] each, then the moments [5][R] (hist_bins_body)
static size_t hist_out_doubles(int n_bin, size_t R) { return (size_t)3 * n_bin * R + 5 * R; }

// Every check of a set that needs no device; fills the model arguments and the sizes.  m == NULL: the rows are the caller's
// (mcsas_hip_histogram_device_rows), the model and its smearing are not looked at.
static int check_hist_set(const mcsas_problem *p, const double *contribs, int n_hist, const mcsas_histogram_spec *specs, double *scaling, double *out,
                          ModelArgs *m, HistSizes *sz) {
    if (!p || !contribs || !scaling || !p->q || !p->intensity || !p->sigma || p->nq < 1 || p->n_contrib < 1 || p->n_reps < 1 || n_hist < 0 ||
        (n_hist > 0 && (!specs || !out)))
        return fail(MCSAS_EINVAL, "bad argument");
    if (p->n_contrib > HIST_MAX_CONTRIBS)
        return fail(MCSAS_EINVAL, "mcsas_hip_histogram stages a repetition's contributions in LDS: n_contrib %d > %d (use mcsas_hip_histogram_prep)", p->n_contrib, HIST_MAX_CONTRIBS);
    if (m) {
        if (int rc = fill_model_args(p, m)) return rc;
        if (int rc = SmearDev::check(p)) return rc;
    }
    const size_t P = p->n_active, R = p->n_reps;
    *sz = HistSizes{};
    for (int h = 0; h < n_hist; ++h) {
        const mcsas_histogram_spec &sp = specs[h];
        if (sp.n_bin < 0 || sp.n_bin > (1 << 20) || sp.param_index < 0 || sp.param_index >= (int)std::max<size_t>(P, 1) || sp.weighting < 0 || sp.weighting > 3 ||
            (sp.n_bin > 0 && !sp.edges) || P == 0)
            return fail(MCSAS_EINVAL, "histogram %d: param_index %d, weighting %d, n_bin %d", h, sp.param_index, sp.weighting, sp.n_bin);
        sz->n_edges += (size_t)sp.n_bin + 1;
        sz->n_out += hist_out_doubles(sp.n_bin, R);
    }
    lay_out_hist_set(sz, p, n_hist);
    return MCSAS_OK;
}

// a checked set's going-in block
static void pack_hist_set(double *dst, const mcsas_problem *p, const double *contribs, int n_hist, const mcsas_histogram_spec *specs, const HistSizes &sz) {
    const size_t Q = p->nq, R = p->n_reps;
    memcpy(dst, p->q, sizeof(double) * Q);
    memcpy(dst + sz.I_off, p->intensity, sizeof(double) * Q);
    memcpy(dst + sz.sg_off, p->sigma, sizeof(double) * Q);
    memcpy(dst + sz.c_off, contribs, sizeof(double) * (sz.edge_off - sz.c_off));
    HistSpecDev *hs = reinterpret_cast<HistSpecDev *>(dst + sz.spec_off);
    size_t e_off = 0, o_off = 0;
    for (int h = 0; h < n_hist; ++h) {
        const mcsas_histogram_spec &sp = specs[h];
        memcpy(dst + sz.edge_off + e_off, sp.edges, sizeof(double) * ((size_t)sp.n_bin + 1));
        hs[h] = HistSpecDev{sp.param_index, sp.weighting, sp.n_bin, 0, (int64_t)e_off, (int64_t)o_off, sp.lower, sp.upper};
        e_off += (size_t)sp.n_bin + 1; o_off += hist_out_doubles(sp.n_bin, R);
    }
}

// a set's results out of its coming-back block (fractions may be NULL)
static void unpack_hist_set(const double *src, const HistSizes &sz, double *scaling, double *fractions, double *out) {
    memcpy(scaling, src, sizeof(double) * sz.frac_off);
    if (fractions) memcpy(fractions, src + sz.frac_off, sizeof(double) * (sz.out_off - sz.frac_off));
    if (sz.n_out) memcpy(out, src + sz.out_off, sizeof(double) * sz.n_out);
}

// a pinned staging block from the process-level cache
struct Pinned {
    double *p = nullptr; size_t bytes = 0;
    ~Pinned() { cached_host_free(p, bytes, hipHostMallocDefault); }
    hipError_t alloc(size_t n) { bytes = sizeof(double) * n; return cached_host_malloc((void **)&p, bytes, hipHostMallocDefault); }
};
// Every early return after the first asynchronous copy leaves copies / kernels queued on the null stream: this guard, declared after
// the staging blocks and so destroyed before them, waits for what is queued before they go back to the cache, where the next call
// would overwrite them under the DMA.
struct SyncGuard { bool armed = true; ~SyncGuard() { if (armed) (void)hipStreamSynchronize(nullptr); } };

// The rows of a block of repetitions stay in HBM between the kernels: how many repetitions share a block of at most ~8 GB.
static size_t hist_rep_chunk(size_t N, size_t Q, size_t R) { return std::max<size_t>(1, std::min<size_t>(R, ((size_t)8 << 30) / (N * Q * sizeof(double)))); }

// ------------------------------------------------------------------------------ one set on the null stream: what its entry points share
// Where a set's arrays lie on the device: the data vectors and the parameter sets [N][P][R]; the summed rows of a block of
// repetitions, Q doubles each; scaling [2][R]; volumes, weights, surfaces and visibility limits, [N][R] each.
struct HistArrays { const double *q, *I, *sg, *c; double *cum, *sc, *v, *w, *s, *m; };

// ---- partial intensities (mcsas_hip_histogram_partial, mcsas_hip_histogram_partial_device_rows): the scattering curve of only the
// contributions inside a histogram's value range, and of each of its bins, taken from a block of rows while it still lies in HBM.
// the n + 1 edges of an axis with bins: finite, and none below the one before it (the bin curves here, both axes of mcsas_hip_histogram2d)
static bool hist2d_edges_ok(const double *e, int n) {
    for (int k = 0; k <= n; ++k)
        if (!std::isfinite(e[k]) || (k > 0 && e[k] < e[k - 1])) return false;
    return true;
}
// What a checked call wants: the records of the wanted histograms in order, the doubles of their curves (per wanted histogram
// range [nq][R], then bin [n_bin][nq][R] where the bins are wanted too), the most dynamic LDS a block of them asks for.
struct HistPartialPlan { std::vector<HistPartialDev> recs; size_t n_out = 0, lds = 0; };
constexpr size_t HIST_PARTIAL_MAX_BYTES = (size_t)2 << 30;

// Every check of the wishes, after check_hist_set has passed the set itself: needs no device.  want == NULL with no histogram: nothing wanted.
static int check_hist_partial(const mcsas_problem *p, int n_hist, const mcsas_histogram_spec *specs, const int32_t *want, const double *partial,
                              HistPartialPlan *pl) {
    static const char who[] = "histogram_partial";
    if (n_hist > 0 && !want)
        return fail(MCSAS_EINVAL, "%s: want is NULL with %d histograms (per histogram 0: nothing, 1: the range curve, 2: the range curve and the bin curves)", who, n_hist);
    const size_t Q = p->nq, N = p->n_contrib, R = p->n_reps;
    size_t e_off = 0;
    for (int h = 0; h < n_hist; ++h) {
        const mcsas_histogram_spec &sp = specs[h];
        const int w = want[h];
        if (w < 0 || w > 2)
            return fail(MCSAS_EINVAL, "%s: histogram %d: want %d (0: nothing, 1: the range curve, 2: the range curve and the bin curves)", who, h, w);
        if (w && !partial) return fail(MCSAS_EINVAL, "%s: histogram %d wants curves (want %d), but partial is NULL", who, h, w);
        if (w == 2 && sp.n_bin > HIST_PARTIAL_MAX_BINS)
            return fail(MCSAS_EINVAL, "%s: histogram %d: the bin curves keep every bin's running sums in LDS: n_bin %d > %d (want 1 gives the range curve alone)", who,
                        h, sp.n_bin, HIST_PARTIAL_MAX_BINS);
        if (w == 2 && sp.n_bin > 0 && !hist2d_edges_ok(sp.edges, sp.n_bin))
            return fail(MCSAS_EINVAL, "%s: histogram %d: bin curves need edges that are finite and non-decreasing (a contribution lies in one bin)", who, h);
        if (w) {
            pl->recs.push_back(HistPartialDev{sp.param_index, sp.n_bin, w, 0, (int64_t)e_off, (int64_t)pl->n_out, sp.lower, sp.upper});
            pl->n_out += Q * R * (1 + (w == 2 ? (size_t)sp.n_bin : 0));
            pl->lds = std::max(pl->lds, hist_partial_lds_bytes(N, sp.n_bin, w));
            if (pl->n_out * sizeof(double) > HIST_PARTIAL_MAX_BYTES)
                return fail(MCSAS_EINVAL, "%s: histogram %d: the curves wanted up to here take %zu bytes, more than 2 GiB in all (ask for fewer histograms or bins per call)", who,
                            h, pl->n_out * sizeof(double));
        }
        e_off += (size_t)sp.n_bin + 1;
    }
    return MCSAS_OK;
}

// A bins kernel — hist_bins_kernel or its batch form — over `grid`: its dynamic LDS is 3 N doubles (hist_bins_body), and the limit of
// that is raised first where N asks for more than a kernel gets unasked
template <class... P>
static int launch_hist_bins(void (*kernel)(P...), dim3 grid, size_t N, typename as_declared<P>::type... args) {
    const size_t lds = sizeof(double) * 3 * N;
    if (lds > LDS_UNRAISED_MAX) HIPCHK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kernel<<<grid, WAVE, lds>>>(args...);
    HIPCHK(hipGetLastError());
    return MCSAS_OK;
}

// A checked set on the device and the one frame of every call that has one: ONE packed upload (data vectors, parameter sets, bin
// edges, histogram records) from a pinned staging block, the kernels back to back on the null stream, ONE packed download — a call
// costs two transfers and no allocation once its block sizes have been seen (MemCache).  An entry point is its checks, upload(),
// run() with who fills a block of rows and which fit follows them, finish() (mcsas_hip_histogram_prep: download()), and what it
// alone unpacks.  The members go in the reverse of this order: first the guard waits for what is queued, on every way out, a
// failing rows callback's too; only then the smearing tables the kernels read, the staging blocks the copies read and write, the
// device blocks and the rows go back to where the next call would take them from.  (In an unnamed namespace:
// the library's list of symbols stays what it was.)
namespace {
struct HistOnDevice {
    const mcsas_problem *p = nullptr;
    const ModelArgs *m = nullptr;                              // the model that fills the rows, or NULL: the caller does
    int n_hist = 0;
    size_t block = 0;                                          // repetitions per block of rows
    const double *rows = nullptr;                              // a block's rows: row rl N + c = contribution c of repetition r0 + rl
    const HistPartialPlan *pl = nullptr;                       // the curves wanted: their records (one small upload) and the curves in a
    bool curves = false;                                       // block of their own (one more download), where there are any
    HistSizes sz;
    DevBuf<double> drows;                                      // (the model's rows; the caller's are the caller's)
    DevBuf<double> din, dback, dcum, dvws, drec, dcurves;
    Pinned hin, hback, hrec, hcurves;
    SmearDev smear;                                            // (the built-in rows' tables; none where the rows are the caller's)
    SyncGuard sync_guard;
    HistArrays a{};

    // The set and the wishes (or NULL) to the device.  `block_reps`: how many repetitions share a block of rows.  m_: the problem's
    // model fills them (its smearing tables go up here), or NULL and caller_rows is where the caller fills them.
    int upload(const mcsas_problem *p_, const double *contribs, int n_hist_, const mcsas_histogram_spec *specs, const HistSizes &sz_, size_t block_reps,
               ModelArgs *m_, const double *caller_rows, const HistPartialPlan *wishes) {
        p = p_; m = m_; n_hist = n_hist_; sz = sz_; block = block_reps; pl = wishes; curves = pl && !pl->recs.empty();
        const size_t NR = (size_t)p->n_contrib * p->n_reps;
        if (m) HIPCHK(drows.alloc(block * p->n_contrib * p->nq));
        rows = m ? drows.p : caller_rows;
        HIPCHK(din.alloc(sz.n_in)); HIPCHK(dback.alloc(sz.n_back)); HIPCHK(dcum.alloc(block * p->nq));
        if (!sz.vws_back) HIPCHK(dvws.alloc(4 * NR));
        HIPCHK(hin.alloc(sz.n_in)); HIPCHK(hback.alloc(sz.n_back));
        pack_hist_set(hin.p, p, contribs, n_hist, specs, sz);
        HIPCHK(hipMemcpyAsync(din.p, hin.p, hin.bytes, hipMemcpyHostToDevice, nullptr));
        double *vws = sz.vws_back ? dback.p + sz.frac_off : dvws.p;
        a = HistArrays{din.p, din.p + sz.I_off, din.p + sz.sg_off, din.p + sz.c_off, dcum.p, dback.p, vws, vws + NR, vws + 2 * NR, vws + 3 * NR};
        if (m)
            if (int rc = smear.upload(p, p->nq, m_)) return rc;
        if (curves) {
            const size_t rec_bytes = sizeof(HistPartialDev) * pl->recs.size(), rec_doubles = (rec_bytes + 7) / 8;
            HIPCHK(drec.alloc(rec_doubles)); HIPCHK(dcurves.alloc(pl->n_out)); HIPCHK(hrec.alloc(rec_doubles)); HIPCHK(hcurves.alloc(pl->n_out));
            memcpy(hrec.p, pl->recs.data(), rec_bytes);
            HIPCHK(hipMemcpyAsync(drec.p, hrec.p, hrec.bytes, hipMemcpyHostToDevice, nullptr));
        }
        return MCSAS_OK;
    }
    // who fills the rows, unless the caller: the problem's model, with their volumes, weights and surfaces
    auto model_rows() {
        return [this](size_t r0, unsigned nr) {
            return launch_small_kernel<HistRowsFamily>(p->model_id, dim3((unsigned)p->n_contrib, nr), sizeof(double) * table_doubles_host(p->model_id, m->int_div),
                                                       *m, p->nq, a.q, p->n_contrib, p->n_reps, r0, a.c, drows.p, a.v, a.w, a.s);
        };
    }
    // which fit follows, where the points are one set: the closed-form scale / background fit (mcsas.py:559), the visibility limits
    auto fit_obs() {
        return [this](size_t r0, unsigned nr) {
            const int nq = p->nq, N = p->n_contrib, R = p->n_reps;
            hist_fit_cum_kernel<<<nr, WAVE>>>(nq, a.I, a.sg, R, (int)r0, a.cum, p->find_background != 0, p->positive_background != 0, a.sc);
            HIPCHK(hipGetLastError());
            hist_obs_kernel<<<dim3((unsigned)N, nr), WAVE>>>(nq, a.sg, N, R, (int)r0, rows, a.sc, a.v, a.w, a.m);
            HIPCHK(hipGetLastError());
            return (int)MCSAS_OK;
        };
    }
    // hist_partial_kernel over repetitions [r0, r0 + nr), whose rows begin at `rows` and whose scales the fit has left in a.sc
    int launch_curves(size_t r0, unsigned nr) {
        const size_t nq = p->nq, N = p->n_contrib, n_want = pl->recs.size();
        if (pl->lds > LDS_UNRAISED_MAX) HIPCHK(hipFuncSetAttribute((const void *)hist_partial_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl->lds));
        const unsigned tiles = (unsigned)((nq + HIST_PARTIAL_TILE - 1) / HIST_PARTIAL_TILE);
        for (size_t z0 = 0; z0 < nr; z0 += GRID_Y_MAX)
            for (size_t y0 = 0; y0 < n_want; y0 += GRID_Y_MAX) {
                const dim3 grid(tiles, (unsigned)std::min(GRID_Y_MAX, n_want - y0), (unsigned)std::min<size_t>(GRID_Y_MAX, nr - z0));
                hist_partial_kernel<<<grid, WAVE, pl->lds>>>(p->nq, p->n_contrib, p->n_active, p->n_reps, (int)(r0 + z0), rows + z0 * N * nq, a.c, a.sc,
                                                            din.p + sz.edge_off, reinterpret_cast<const HistPartialDev *>(drec.p) + y0, dcurves.p);
                HIPCHK(hipGetLastError());
            }
        return MCSAS_OK;
    }
    // The first half of histogram(), a block of repetitions at a time: fill_rows(r0, nr) leaves the rows of repetitions [r0, r0 + nr)
    // at `rows` and files their volumes, weights and surfaces; cumInt = the sum of the rows in contribution order
    // (scatteringmodel.py:101); fit(r0, nr) leaves every repetition's scale in a.sc and every contribution's visibility limit in
    // a.m; then, where curves are wanted, hist_partial_kernel on the same rows while they still lie in HBM.
    template <class Rows, class Fit>
    int run(Rows fill_rows, Fit fit) {
        const size_t R = p->n_reps;
        for (size_t r0 = 0; r0 < R; r0 += block) {
            const unsigned nr = (unsigned)std::min(block, R - r0);
            if (int rc = fill_rows(r0, nr)) return rc;
            hist_colsum_kernel<<<dim3((unsigned)(((size_t)p->nq + 255) / 256), nr), 256>>>(p->nq, p->n_contrib, rows, a.cum);
            HIPCHK(hipGetLastError());
            if (int rc = fit(r0, nr)) return rc;
            if (curves)
                if (int rc = launch_curves(r0, nr)) return rc;
        }
        if (curves) HIPCHK(hipMemcpyAsync(hcurves.p, dcurves.p, hcurves.bytes, hipMemcpyDeviceToHost, nullptr));
        return MCSAS_OK;
    }
    // the coming-back block, and the wait for everything queued
    int download() {
        HIPCHK(hipMemcpyAsync(hback.p, dback.p, hback.bytes, hipMemcpyDeviceToHost, nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
        sync_guard.armed = false;
        return MCSAS_OK;
    }
    // the second half of histogram() once every repetition has its scale and limits: fractions, bins, the download, the results
    int finish(double *scaling, double *fractions, double *out, double *partial = nullptr) {
        const int N = p->n_contrib, R = p->n_reps;
        double *dfrac = dback.p + sz.frac_off;
        hist_fractions_kernel<<<(unsigned)R, WAVE>>>(N, R, a.sc, a.v, a.w, a.s, a.m, dfrac);
        HIPCHK(hipGetLastError());
        if (n_hist > 0)
            if (int rc = launch_hist_bins(hist_bins_kernel, dim3((unsigned)n_hist, (unsigned)R), N, N, p->n_active, R, a.c, dfrac, din.p + sz.edge_off,
                                          reinterpret_cast<const HistSpecDev *>(din.p + sz.spec_off), dback.p + sz.out_off))
                return rc;
        if (int rc = download()) return rc;
        unpack_hist_set(hback.p, sz, scaling, fractions, out);
        if (curves) memcpy(partial, hcurves.p, sizeof(double) * pl->n_out);
        return MCSAS_OK;
    }
};
}  // namespace

// ------------------------------------------------------------------------------ one set: mcsas_hip_histogram_prep, mcsas_hip_histogram

// The first half of histogram() alone (McSAS.histogram() goes on in Python, whatever the number of contributions): HistOnDevice
// with no histograms and its own coming-back block, [scaling | volumes, weights, surfaces, visibility limits] in the one download.
// check_hist_set's cap on the contributions is the bins kernel's and does not hold here.
extern "C" int mcsas_hip_histogram_prep(const mcsas_problem *p, const double *contribs, double *scaling, double *vset,
                                        double *wset, double *sset, double *min_req_vol) {
    return no_bad_alloc("histogram_prep", [&]() -> int {
        if (!p || !contribs || !scaling || !vset || !wset || !sset || !min_req_vol || !p->q || !p->intensity || !p->sigma ||
            p->nq < 1 || p->n_contrib < 1 || p->n_reps < 1)
            return fail(MCSAS_EINVAL, "bad argument");
        ModelArgs m;
        if (int rc = fill_model_args(p, &m)) return rc;
        DeviceGuard dev_guard;
        if (int rc = select_device(p->device)) return rc;
        const size_t NR = (size_t)p->n_contrib * p->n_reps;
        HistSizes sz;
        lay_out_hist_set(&sz, p, 0);
        sz.vws_back = true; sz.n_back = sz.frac_off + 4 * NR;
        HistOnDevice d;
        if (int rc = d.upload(p, contribs, 0, nullptr, sz, hist_rep_chunk(p->n_contrib, p->nq, p->n_reps), &m, nullptr, nullptr)) return rc;
        if (int rc = d.run(d.model_rows(), d.fit_obs())) return rc;
        if (int rc = d.download()) return rc;
        memcpy(scaling, d.hback.p, sizeof(double) * sz.frac_off);
        double *const back[4] = {vset, wset, sset, min_req_vol};
        for (int i = 0; i < 4; ++i) memcpy(back[i], d.hback.p + sz.frac_off + i * NR, sizeof(double) * NR);
        return MCSAS_OK;
    });
}

// McSAS.histogram() complete (include/mcsas_hip.h): the set on the device (HistOnDevice), its rows by the model's kernel a chunk of
// repetitions at a time.  Every refusal of the set itself comes before a device is touched.  `asked`: the call is
// mcsas_hip_histogram_partial, and want / partial say which curves hist_partial_kernel takes from each block of rows; with nothing
// wanted the call is mcsas_hip_histogram.
static int histogram_call(const mcsas_problem *p, const double *contribs, int32_t n_hist, const mcsas_histogram_spec *specs, bool asked,
                          const int32_t *want, double *scaling, double *fractions, double *out, double *partial) {
    ModelArgs m; HistSizes sz; HistPartialPlan pl;
    if (int rc = check_hist_set(p, contribs, n_hist, specs, scaling, out, &m, &sz)) return rc;
    if (asked)
        if (int rc = check_hist_partial(p, n_hist, specs, want, partial, &pl)) return rc;
    DeviceGuard dev_guard;
    if (int rc = select_device(p->device)) return rc;
    HistOnDevice d;
    if (int rc = d.upload(p, contribs, n_hist, specs, sz, hist_rep_chunk(p->n_contrib, p->nq, p->n_reps), &m, nullptr, &pl)) return rc;
    if (int rc = d.run(d.model_rows(), d.fit_obs())) return rc;
    return d.finish(scaling, fractions, out, partial);
}
extern "C" int mcsas_hip_histogram(const mcsas_problem *p, const double *contribs, int32_t n_hist, const mcsas_histogram_spec *specs,
                                   double *scaling, double *fractions, double *out) {
    return no_bad_alloc("histogram", [&] { return histogram_call(p, contribs, n_hist, specs, false, nullptr, scaling, fractions, out, nullptr); });
}
extern "C" int mcsas_hip_histogram_partial(const mcsas_problem *p, const double *contribs, int32_t n_hist, const mcsas_histogram_spec *specs,
                                           const int32_t *want, double *scaling, double *fractions, double *out, double *partial) {
    return no_bad_alloc("histogram_partial", [&] { return histogram_call(p, contribs, n_hist, specs, true, want, scaling, fractions, out, partial); });
}

// ------------------------------------------------------------------------------ the sets of a joint fit: mcsas_hip_histogram_sets
// The frame of histogram_call over the points of all sets: the rows kernel and the column sums take nq = Σ set_nq as it is, the fit
// and the visibility limits know the sets (hist_fit_sets_kernel, hist_obs_sets_kernel), HistOnDevice::finish goes on with the
// reference scale.  Every set's fit comes back behind the set's own coming-back block, in the one download.  What the call refuses
// beyond check_hist_set is host_decide.hip's (check_hist_sets_request), before a device is touched.
extern "C" int mcsas_hip_histogram_sets(const mcsas_problem *p, const double *contribs, int32_t n_hist, const mcsas_histogram_spec *specs, int32_t n_sets,
                                        const int32_t *set_nq, int32_t scale_mode, int32_t ref_set, uint32_t visible_sets, double *scaling,
                                        double *fractions, double *out, mcsas_sets_result *sets) {
    return no_bad_alloc("histogram_sets", [&]() -> int {
        HistSetOffs off;
        if (int rc = check_hist_sets_request(p, n_sets, set_nq, scale_mode, ref_set, visible_sets, sets, off.o)) return rc;
        ModelArgs m; HistSizes sz;
        if (int rc = check_hist_set(p, contribs, n_hist, specs, scaling, out, &m, &sz)) return fail_within(rc, "histogram_sets");
        DeviceGuard dev_guard;
        if (int rc = select_device(p->device)) return rc;
        const int nq = p->nq, N = p->n_contrib, R = p->n_reps, shared = scale_mode == MCSAS_SETS_SCALE_SHARED;
        const size_t fit_off = sz.n_back;                          // [2][MCSAS_MAX_SETS][R] behind the set's coming-back block
        sz.n_back += 2 * (size_t)MCSAS_MAX_SETS * R;
        HistOnDevice d;                                            // (smearing is refused: the model's arguments say "none")
        if (int rc = d.upload(p, contribs, n_hist, specs, sz, hist_rep_chunk(N, nq, R), &m, nullptr, nullptr)) return rc;
        double *const dfit = d.dback.p + fit_off;
        HIPCHK(hipMemsetAsync(dfit, 0, sizeof(double) * 2 * MCSAS_MAX_SETS * R, nullptr));
        const HistArrays &a = d.a;
        const int rc = d.run(d.model_rows(), [&](size_t r0, unsigned nr) {
            hist_fit_sets_kernel<<<nr, WAVE>>>(nq, a.I, a.sg, R, (int)r0, a.cum, p->find_background != 0, n_sets, off, shared, ref_set, a.sc, dfit);
            HIPCHK(hipGetLastError());
            hist_obs_sets_kernel<<<dim3((unsigned)N, nr), WAVE>>>(nq, a.sg, N, R, (int)r0, d.rows, a.sc, dfit, n_sets, off, visible_sets, a.v, a.w, a.m);
            HIPCHK(hipGetLastError());
            return (int)MCSAS_OK;
        });
        if (rc) return rc;
        if (int rc2 = d.finish(scaling, fractions, out)) return rc2;
        const double *hfit = d.hback.p + fit_off;
        for (int s = 0; s < n_sets; ++s) {
            memcpy(sets->scaling + (size_t)s * R, hfit + (size_t)s * R, sizeof(double) * R);
            memcpy(sets->background + (size_t)s * R, hfit + ((size_t)MCSAS_MAX_SETS + s) * R, sizeof(double) * R);
        }
        return MCSAS_OK;
    });
}

// ------------------------------------------------------------------------------ one set, the rows filled by the caller: mcsas_hip_histogram_device_rows
// rows of 256 MiB at the most make a useful round, never less than one repetition's; the row pitch is nq: hist_colsum_body walks a
// repetition's rows densely
static size_t hist_rows_useful(size_t N, size_t Q, size_t R) {
    const size_t cap = ((size_t)256 << 20) / (Q * sizeof(double)) / N * N;
    return std::max(N, std::min(N * R, cap));
}
// what the shape query and the entry point refuse of a problem alike, ahead of check_hist_set
static int check_hist_rows_problem(const char *who, const mcsas_problem *p) {
    if (!p) return fail(MCSAS_EINVAL, "%s: problem is NULL", who);
    if (p->struct_size != sizeof(mcsas_problem))
        return fail(MCSAS_EINVAL, "%s: mcsas_problem size %u, library expects %zu (ABI mismatch)", who, p->struct_size, sizeof(mcsas_problem));
    if (p->nq < 1 || p->n_contrib < 1 || p->n_reps < 1)
        return fail(MCSAS_EINVAL, "%s: nq %d, n_contrib %d, n_reps %d (each >= 1)", who, p->nq, p->n_contrib, p->n_reps);
    return MCSAS_OK;
}
extern "C" int mcsas_hip_histogram_rows_shape(const mcsas_problem *p, int64_t *min_rows, int64_t *useful_rows, int32_t *row_stride) {
    return no_bad_alloc("histogram_rows_shape", [&]() -> int {
        if (int rc = check_hist_rows_problem("histogram_rows_shape", p)) return rc;
        if (min_rows) *min_rows = p->n_contrib;
        if (useful_rows) *useful_rows = (int64_t)hist_rows_useful(p->n_contrib, p->nq, p->n_reps);
        if (row_stride) *row_stride = p->nq;
        return MCSAS_OK;
    });
}

// The second half of mcsas_hip_histogram with the first half's rows handed over by the caller, a round of whole repetitions at a
// time (include/mcsas_hip.h): hist_pset_kernel lays the round's parameter sets out for the callback, the callback fills d_rows and
// d_vws, hist_take_vws_kernel files the three per-row values, and HistOnDevice::run goes on with the rows where they lie.
// After the last round the call is mcsas_hip_histogram again.  Every refusal of the arguments comes before a device is touched, the
// buffers are looked at before anything is queued, and from the upload on the set's guard waits on every way out, a failing callback's too.
// (`asked`, want, partial: as histogram_call takes them, for mcsas_hip_histogram_partial_device_rows; the body runs under no_bad_alloc)
static int histogram_device_rows_call(const mcsas_problem *p, const double *contribs, double *d_pset, double *d_rows, double *d_vws,
                                      int64_t capacity_rows, mcsas_device_rows_callback rows_cb, void *user, int32_t n_hist,
                                      const mcsas_histogram_spec *specs, bool asked, const int32_t *want, double *scaling, double *fractions,
                                      double *out, double *partial) {
    static const char who[] = "histogram_device_rows";
    return no_bad_alloc(who, [&]() -> int {
        const struct { const char *name; const void *ptr; } needed[] = {{"problem", p}, {"contribs", contribs}, {"d_pset", d_pset}, {"d_rows", d_rows},
                                                                        {"d_vws", d_vws}, {"rows_cb", (const void *)rows_cb}, {"out", out}};
        for (const auto &a : needed)
            if (!a.ptr) return fail(MCSAS_EINVAL, "%s: %s is NULL", who, a.name);
        if (int rc = check_hist_rows_problem(who, p)) return rc;
        HistSizes sz;
        if (int rc = check_hist_set(p, contribs, n_hist, specs, scaling, out, nullptr, &sz)) return fail_within(rc, "%s", who);
        if (p->n_active < 1 || p->n_active > MCSAS_MAX_ACTIVE) return fail(MCSAS_EINVAL, "%s: n_active %d (1..%d)", who, p->n_active, MCSAS_MAX_ACTIVE);
        if (capacity_rows < p->n_contrib)
            return fail(MCSAS_EINVAL, "%s: capacity_rows %lld < %d = n_contrib, the rows of one repetition (mcsas_hip_histogram_rows_shape)", who,
                        (long long)capacity_rows, p->n_contrib);
        if (p->smear_nk != 0 || p->smear_locs || p->smear_q_offset || p->smear_weights)
            return fail(MCSAS_EINVAL, "%s: a smearing table (smear_nk %d) is given, but the rows are the caller's: nothing here would apply it", who, p->smear_nk);
        HistPartialPlan pl;
        if (asked)
            if (int rc = check_hist_partial(p, n_hist, specs, want, partial, &pl)) return rc;
        DeviceGuard dev_guard;
        if (int rc = select_device(p->device)) return rc;
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        if (int rc = check_device_buffer(who, "d_pset", d_pset, dev)) return rc;
        if (int rc = check_device_buffer(who, "d_rows", d_rows, dev)) return rc;
        if (int rc = check_device_buffer(who, "d_vws", d_vws, dev)) return rc;
        const size_t P = p->n_active, N = p->n_contrib, R = p->n_reps, cap = (size_t)capacity_rows;
        const size_t per_round = std::min<size_t>({R, cap / N, GRID_Y_MAX});       // (whole repetitions)
        HistOnDevice d;
        if (int rc = d.upload(p, contribs, n_hist, specs, sz, per_round, nullptr, d_rows, &pl)) return rc;
        const int rc = d.run([&](size_t r0, unsigned nr) {
            const size_t n_rows = nr * N;
            hist_pset_kernel<<<(unsigned)((n_rows * P + 255) / 256), 256>>>((int)N, (int)P, (int)R, (int)r0, n_rows, d.a.c, d_pset);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(nullptr));                                 // the sets are complete before the caller reads them
            if (const int cb = rows_cb(user, (int32_t)n_rows)) return fail(MCSAS_ECALLBACK, "%s: rows callback returned %d", who, cb);
            hist_take_vws_kernel<<<(unsigned)((n_rows + 255) / 256), 256>>>((int)N, (int)R, (int)r0, n_rows, cap, d_vws, d.a.v, d.a.w, d.a.s);
            HIPCHK(hipGetLastError());
            return (int)MCSAS_OK;
        }, d.fit_obs());
        if (rc) return rc;
        return d.finish(scaling, fractions, out, partial);
    });
}
extern "C" int mcsas_hip_histogram_device_rows(const mcsas_problem *p, const double *contribs, double *d_pset, double *d_rows, double *d_vws,
                                               int64_t capacity_rows, mcsas_device_rows_callback rows_cb, void *user, int32_t n_hist,
                                               const mcsas_histogram_spec *specs, double *scaling, double *fractions, double *out) {
    return histogram_device_rows_call(p, contribs, d_pset, d_rows, d_vws, capacity_rows, rows_cb, user, n_hist, specs, false, nullptr, scaling, fractions,
                                      out, nullptr);
}
extern "C" int mcsas_hip_histogram_partial_device_rows(const mcsas_problem *p, const double *contribs, double *d_pset, double *d_rows, double *d_vws,
                                                       int64_t capacity_rows, mcsas_device_rows_callback rows_cb, void *user, int32_t n_hist,
                                                       const mcsas_histogram_spec *specs, const int32_t *want, double *scaling, double *fractions,
                                                       double *out, double *partial) {
    return histogram_device_rows_call(p, contribs, d_pset, d_rows, d_vws, capacity_rows, rows_cb, user, n_hist, specs, true, want, scaling, fractions,
                                      out, partial);
}

// ------------------------------------------------------------------------------ a batch of sets: mcsas_hip_histogram_batch
// the rows budget of a batch chunk: 2 GiB, or MCSAS_HIP_HIST_BATCH_MB (a number of MiB, fractions allowed) — read at every call
static size_t hist_batch_budget() {
    double mb = 2048.;
    if (const char *e = getenv("MCSAS_HIP_HIST_BATCH_MB")) { char *end = nullptr; const double v = strtod(e, &end); if (end != e && v >= 0. && v < 1e9) mb = v; }
    return (size_t)(mb * 1048576.);
}

// A set of the batch: the caller's arguments for it and what check_hist_set made of them.  single: it runs through
// mcsas_hip_histogram; otherwise rec is its record, and the *_off are where its blocks begin in the upload, the download and the
// scratch blocks (rows and cum: of its chunk).
struct HistBatchSet {
    const mcsas_problem *p; const double *contribs; int n_hist; const mcsas_histogram_spec *specs; double *scaling, *fractions, *out;
    ModelArgs m; HistSizes sz; bool single; int rec; size_t in_off, back_off, vws_off, rows_off, cum_off;
};
// sets [first, end), none of them single; their (set, repetition) blocks [blk_first, blk_first + n_blk) of the block table; the
// doubles of their rows and summed intensities; their largest extents
struct HistChunk { size_t first, end; size_t blk_first = 0, n_blk = 0, rows = 0, cum = 0, maxN = 0, maxQ = 0, maxH = 0; };
// The staging layout of a batch (doubles): in = per batched set its going-in block, then the records, then the block table; back = per
// batched set its coming-back block.
struct HistBatchPlan {
    std::vector<HistChunk> chunks;
    size_t n_rec = 0, n_blk = 0, n_in = 0, n_back = 0, n_vws = 0, max_rows = 0, max_cum = 0;
    size_t rec_d() const { return (sizeof(HistSetDev) * n_rec + 7) / 8; }
    size_t in_total() const { return n_in + rec_d() + (sizeof(ChainRef) * n_blk + 7) / 8; }
};
struct HistBatchDev { const HistSetDev *sets; const ChainRef *blocks; double *in, *back, *rows, *cum, *vws; };

// Chunks of consecutive batched sets whose rows fit the budget (a single set closes the chunk before it); numbers the records.  The
// block table keeps a chunk's blocks together.
static HistBatchPlan plan_hist_chunks(std::vector<HistBatchSet> &sets, size_t budget) {
    HistBatchPlan pl;
    for (size_t s = 0; s < sets.size(); ++s) {
        HistBatchSet &t = sets[s];
        if (t.single) continue;
        const size_t R = t.p->n_reps, N = t.p->n_contrib, Q = t.p->nq;
        const bool open = !pl.chunks.empty() && pl.chunks.back().end == s && (pl.chunks.back().rows + t.sz.rows) * sizeof(double) <= budget;
        if (!open) pl.chunks.push_back(HistChunk{s, s});
        HistChunk &c = pl.chunks.back();
        t.rec = (int)pl.n_rec++;
        t.in_off = pl.n_in; t.back_off = pl.n_back; t.vws_off = pl.n_vws; t.rows_off = c.rows; t.cum_off = c.cum;
        c.end = s + 1; c.rows += t.sz.rows; c.cum += R * Q; c.n_blk += R;
        c.maxN = std::max(c.maxN, N); c.maxQ = std::max(c.maxQ, Q); c.maxH = std::max<size_t>(c.maxH, t.n_hist);
        pl.n_in += t.sz.n_in; pl.n_back += t.sz.n_back; pl.n_vws += 4 * N * R;
        pl.max_rows = std::max(pl.max_rows, c.rows); pl.max_cum = std::max(pl.max_cum, c.cum);
    }
    for (HistChunk &c : pl.chunks) { c.blk_first = pl.n_blk; pl.n_blk += c.n_blk; }
    return pl;
}

// Fills the upload block `hin`: every batched set's going-in block and record (its smearing tables go to the device here), and the
// block table, a chunk's blocks model by model (hist_rows runs once per model; the other kernels take the chunk whole).
static int pack_hist_batch(const HistBatchPlan &pl, std::vector<HistBatchSet> &sets, std::vector<SmearDev> &smears, double *hin) {
    HistSetDev *recs = reinterpret_cast<HistSetDev *>(hin + pl.n_in);
    ChainRef *blks = reinterpret_cast<ChainRef *>(hin + pl.n_in + pl.rec_d());
    for (const HistChunk &c : pl.chunks) {
        for (size_t s = c.first; s < c.end; ++s) {
            HistBatchSet &t = sets[s];
            const mcsas_problem *p = t.p; const HistSizes &sz = t.sz; const size_t w = t.in_off;
            HistSetDev &d = recs[t.rec];
            memset(&d, 0, sizeof d);
            if (int rc = smears[t.rec].upload(p, p->nq, &t.m)) return rc;
            d.model = t.m;
            d.nq = p->nq; d.N = p->n_contrib; d.P = p->n_active; d.R = p->n_reps; d.n_hist = t.n_hist;
            d.find_bg = p->find_background != 0; d.pos_bg = p->positive_background != 0;
            d.q_off = (int64_t)w; d.I_off = (int64_t)(w + sz.I_off); d.sg_off = (int64_t)(w + sz.sg_off); d.c_off = (int64_t)(w + sz.c_off);
            d.edge_off = (int64_t)(w + sz.edge_off); d.spec_off = (int64_t)(w + sz.spec_off);
            d.back_off = (int64_t)t.back_off; d.rows_off = (int64_t)t.rows_off; d.cum_off = (int64_t)t.cum_off; d.vws_off = (int64_t)t.vws_off;
            pack_hist_set(hin + w, p, t.contribs, t.n_hist, t.specs, sz);
        }
        size_t nb = c.blk_first;
        for (int mid = 0; mid < MCSAS_MODEL_COUNT; ++mid)
            for (size_t s = c.first; s < c.end; ++s)
                if (sets[s].p->model_id == mid)
                    for (int r = 0; r < sets[s].p->n_reps; ++r) blks[nb++] = ChainRef{sets[s].rec, r};
    }
    return MCSAS_OK;
}

// the kernels of one chunk on the null stream: one launch each over the chunk's blocks (hist_rows: one per model in it)
static int launch_hist_chunk(const std::vector<HistBatchSet> &sets, const HistChunk &c, const HistBatchDev &d) {
    const ChainRef *cb = d.blocks + c.blk_first;
    size_t g_first = 0;
    for (int mid = 0; mid < MCSAS_MODEL_COUNT; ++mid) {
        size_t g_blk = 0, g_N = 0, lds = 0;
        for (size_t t = c.first; t < c.end; ++t)
            if (sets[t].p->model_id == mid) {
                g_blk += sets[t].p->n_reps; g_N = std::max<size_t>(g_N, sets[t].p->n_contrib);
                lds = std::max(lds, sizeof(double) * table_doubles_host(mid, sets[t].m.int_div));
            }
        if (!g_blk) continue;
        // (hist_rows_batch_kernel of built-in model `mid` over the g_blk blocks of its sets)
        if (int rc = launch_small_kernel<HistRowsBatchFamily>(mid, dim3((unsigned)g_blk, (unsigned)g_N), lds, d.sets, cb + g_first, d.in, d.rows, d.vws)) return rc;
        g_first += g_blk;
    }
    const unsigned nb = (unsigned)c.n_blk;
    hist_colsum_batch_kernel<<<dim3(nb, (unsigned)((c.maxQ + 255) / 256)), 256>>>(d.sets, cb, d.rows, d.cum);
    HIPCHK(hipGetLastError());
    hist_fit_cum_batch_kernel<<<nb, WAVE>>>(d.sets, cb, d.in, d.cum, d.back);
    HIPCHK(hipGetLastError());
    hist_obs_batch_kernel<<<dim3(nb, (unsigned)c.maxN), WAVE>>>(d.sets, cb, d.in, d.rows, d.back, d.vws);
    HIPCHK(hipGetLastError());
    hist_fractions_batch_kernel<<<nb, WAVE>>>(d.sets, cb, d.vws, d.back);
    HIPCHK(hipGetLastError());
    for (size_t h0 = 0; h0 < c.maxH; h0 += GRID_Y_MAX)
        if (int rc = launch_hist_bins(hist_bins_batch_kernel, dim3(nb, (unsigned)std::min(GRID_Y_MAX, c.maxH - h0)), c.maxN, d.sets, cb, h0, d.in, d.back)) return rc;
    return MCSAS_OK;
}

// McSAS.histogram() of a batch of data sets (include/mcsas_hip.h).  Every refusal comes before a device is touched.  The sets are
// taken in order, in chunks whose rows fit the budget; a chunk is one launch per kernel.  A plug-in model's set, and one whose rows
// alone exceed the budget, closes the chunk before it and runs through mcsas_hip_histogram.
extern "C" int mcsas_hip_histogram_batch(int32_t n_sets, const mcsas_problem *problems, const double *const *contribs, const int32_t *n_hist,
                                         const mcsas_histogram_spec *const *specs, double *const *scaling, double *const *fractions,
                                         double *const *out) {
    return no_bad_alloc("histogram_batch", [&]() -> int {
        if (n_sets < 0) return fail(MCSAS_EINVAL, "histogram_batch: n_sets %d", n_sets);
        if (n_sets == 0) return MCSAS_OK;
        if (!problems || !contribs || !n_hist || !specs || !scaling || !out)
            return fail(MCSAS_EINVAL, "histogram_batch: NULL table (problems, contribs, n_hist, specs, scaling and out are needed; fractions may be NULL)");
        std::vector<HistBatchSet> sets((size_t)n_sets);
        const size_t budget = hist_batch_budget();
        for (int s = 0; s < n_sets; ++s) {
            HistBatchSet &t = sets[s] = HistBatchSet{&problems[s], contribs[s], n_hist[s], specs[s], scaling[s], fractions ? fractions[s] : nullptr, out[s]};
            if (t.p->device != problems[0].device)
                return fail(MCSAS_EINVAL, "histogram_batch: set %d names device %d, set 0 device %d: one device per batch", s, t.p->device, problems[0].device);
            if (int rc = check_hist_set(t.p, t.contribs, t.n_hist, t.specs, t.scaling, t.out, &t.m, &t.sz)) return fail_within(rc, "histogram_batch: set %d", s);
            t.single = is_plugin_model(t.p->model_id) || t.sz.rows * sizeof(double) > budget;
        }
        DeviceGuard dev_guard;
        if (int rc = select_device(problems[0].device)) return rc;
        const HistBatchPlan pl = plan_hist_chunks(sets, budget);
        std::vector<SmearDev> smears(pl.n_rec);                    // (freed after the guard below has waited for the kernels)
        DevBuf<double> din, dback, drows, dcum, dvws;
        Pinned hin, hback;
        SyncGuard sync_guard;
        if (pl.n_rec) {
            HIPCHK(din.alloc(pl.in_total())); HIPCHK(dback.alloc(pl.n_back)); HIPCHK(drows.alloc(pl.max_rows)); HIPCHK(dcum.alloc(pl.max_cum)); HIPCHK(dvws.alloc(pl.n_vws));
            HIPCHK(hin.alloc(pl.in_total())); HIPCHK(hback.alloc(pl.n_back));
            if (int rc = pack_hist_batch(pl, sets, smears, hin.p)) return rc;
            HIPCHK(hipMemcpyAsync(din.p, hin.p, hin.bytes, hipMemcpyHostToDevice, nullptr));
        }
        const HistBatchDev dev{reinterpret_cast<const HistSetDev *>(din.p + pl.n_in), reinterpret_cast<const ChainRef *>(din.p + pl.n_in + pl.rec_d()),
                               din.p, dback.p, drows.p, dcum.p, dvws.p};
        size_t next_chunk = 0;
        for (int s = 0; s < n_sets; ++s) {
            const HistBatchSet &t = sets[s];
            if (t.single) {
                if (int rc = mcsas_hip_histogram(t.p, t.contribs, t.n_hist, t.specs, t.scaling, t.fractions, t.out)) return fail_within(rc, "histogram_batch: set %d", s);
            } else if (next_chunk < pl.chunks.size() && pl.chunks[next_chunk].first == (size_t)s) {   // (otherwise: inside a chunk already launched)
                if (int rc = launch_hist_chunk(sets, pl.chunks[next_chunk++], dev)) return rc;
            }
        }
        if (pl.n_rec) {
            HIPCHK(hipMemcpyAsync(hback.p, dback.p, hback.bytes, hipMemcpyDeviceToHost, nullptr));
            HIPCHK(hipStreamSynchronize(nullptr));
        }
        sync_guard.armed = false;
        for (const HistBatchSet &t : sets)
            if (!t.single) unpack_hist_set(hback.p + t.back_off, t.sz, t.scaling, t.fractions, t.out);
        return MCSAS_OK;
    });
}


// ------------------------------------------------------------------------------ two parameters at once: mcsas_hip_histogram2d
// The joint histogram of two parameter columns from fractions a histogram call returned (include/mcsas_hip.h): no model, no rows.
// Per axis every rule is hist_bins_body's, so that one y column that holds every value gives that kernel's bins bit for bit.

// a histogram's outputs: bins and observability [n_bin_x][n_bin_y][R] each, then the moments [7][R] (hist2d_body)
static size_t hist2d_out_doubles(size_t cells, size_t R) { return 2 * cells * R + 7 * R; }

// One packed upload [contribs | fractions | edges | records], hist2d_kernel on the null stream, one packed download, as HistOnDevice
// holds a set; every refusal of the arguments comes before a device is touched.
extern "C" int mcsas_hip_histogram2d(int32_t n_contrib, int32_t n_active, int32_t n_reps, const double *contribs, const double *fractions,
                                     int32_t n_hist, const mcsas_histogram2d_spec *specs, double *out, int32_t device) {
    static const char who[] = "histogram2d";
    return no_bad_alloc(who, [&]() -> int {
        if (n_hist < 0) return fail(MCSAS_EINVAL, "%s: n_hist %d", who, n_hist);
        if (n_hist == 0) return MCSAS_OK;
        if (!contribs || !fractions || !specs || !out) return fail(MCSAS_EINVAL, "%s: NULL table (contribs, fractions, specs and out are needed)", who);
        if (n_contrib < 1 || n_contrib > HIST_MAX_CONTRIBS || n_active < 1 || n_reps < 1)
            return fail(MCSAS_EINVAL, "%s: n_contrib %d (1..%d: a repetition's contributions are staged in LDS), n_active %d, n_reps %d (each >= 1)", who,
                        n_contrib, HIST_MAX_CONTRIBS, n_active, n_reps);
        const size_t N = n_contrib, P = n_active, R = n_reps;
        if ((size_t)n_hist * R > (size_t)INT32_MAX) return fail(MCSAS_EINVAL, "%s: n_hist %d x n_reps %d blocks", who, n_hist, n_reps);
        size_t n_edges = 0, n_out = 0, shared = 0;
        for (int h = 0; h < n_hist; ++h) {
            const mcsas_histogram2d_spec &sp = specs[h];
            if (sp.reserved != 0) return fail(MCSAS_EINVAL, "%s: histogram %d: reserved %d (must be 0)", who, h, sp.reserved);
            if (sp.param_x < 0 || sp.param_x >= n_active || sp.param_y < 0 || sp.param_y >= n_active || sp.weighting < 0 || sp.weighting > 3)
                return fail(MCSAS_EINVAL, "%s: histogram %d: param_x %d, param_y %d (0..%d), weighting %d (0..3)", who, h, sp.param_x, sp.param_y,
                            n_active - 1, sp.weighting);
            if (sp.n_bin_x < 0 || sp.n_bin_y < 0 || (int64_t)sp.n_bin_x * sp.n_bin_y > HIST2D_MAX_CELLS)
                return fail(MCSAS_EINVAL, "%s: histogram %d: n_bin_x %d, n_bin_y %d (each >= 0, at most %d cells)", who, h, sp.n_bin_x, sp.n_bin_y, HIST2D_MAX_CELLS);
            if ((sp.n_bin_x > 0 && !sp.edges_x) || (sp.n_bin_y > 0 && !sp.edges_y))
                return fail(MCSAS_EINVAL, "%s: histogram %d: an axis with bins has no edges", who, h);
            if ((sp.n_bin_x > 0 && !hist2d_edges_ok(sp.edges_x, sp.n_bin_x)) || (sp.n_bin_y > 0 && !hist2d_edges_ok(sp.edges_y, sp.n_bin_y)))
                return fail(MCSAS_EINVAL, "%s: histogram %d: edges must be finite and non-decreasing", who, h);
            const size_t cells = (size_t)sp.n_bin_x * sp.n_bin_y;
            if (cells) n_edges += (size_t)sp.n_bin_x + sp.n_bin_y + 2;
            n_out += hist2d_out_doubles(cells, R);
            shared = std::max(shared, hist2d_shared_bytes(N, sp.n_bin_x, sp.n_bin_y));
        }
        DeviceGuard dev_guard;
        if (int rc = select_device(device)) return rc;
        const size_t f_off = N * P * R, e_off = f_off + 8 * N * R, s_off = e_off + n_edges, n_in = s_off + (sizeof(Hist2dSpecDev) * (size_t)n_hist + 7) / 8;
        DevBuf<double> din, dout;
        Pinned hin, hout;
        SyncGuard sync_guard;                                      // (after the blocks: it waits before they go back)
        HIPCHK(din.alloc(n_in)); HIPCHK(dout.alloc(n_out)); HIPCHK(hin.alloc(n_in)); HIPCHK(hout.alloc(n_out));
        memcpy(hin.p, contribs, sizeof(double) * f_off);
        memcpy(hin.p + f_off, fractions, sizeof(double) * 8 * N * R);
        Hist2dSpecDev *hs = reinterpret_cast<Hist2dSpecDev *>(hin.p + s_off);
        size_t eo = 0, oo = 0;
        for (int h = 0; h < n_hist; ++h) {
            const mcsas_histogram2d_spec &sp = specs[h];
            const size_t cells = (size_t)sp.n_bin_x * sp.n_bin_y;
            hs[h] = Hist2dSpecDev{sp.param_x, sp.param_y, sp.weighting, sp.n_bin_x, sp.n_bin_y, 0, (int64_t)eo, (int64_t)oo, sp.lower_x, sp.upper_x, sp.lower_y, sp.upper_y};
            if (cells) {
                memcpy(hin.p + e_off + eo, sp.edges_x, sizeof(double) * ((size_t)sp.n_bin_x + 1));
                memcpy(hin.p + e_off + eo + sp.n_bin_x + 1, sp.edges_y, sizeof(double) * ((size_t)sp.n_bin_y + 1));
                eo += (size_t)sp.n_bin_x + sp.n_bin_y + 2;
            }
            oo += hist2d_out_doubles(cells, R);
        }
        HIPCHK(hipMemcpyAsync(din.p, hin.p, hin.bytes, hipMemcpyHostToDevice, nullptr));
        const size_t lds = hist2d_staged_bytes(N) + shared;
        if (lds > LDS_UNRAISED_MAX) HIPCHK(hipFuncSetAttribute((const void *)hist2d_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hist2d_kernel<<<(unsigned)((size_t)n_hist * R), WAVE, lds>>>((int)N, (int)P, (int)R, din.p, din.p + f_off, din.p + e_off,
                                                                     reinterpret_cast<const Hist2dSpecDev *>(din.p + s_off), dout.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hout.p, dout.p, hout.bytes, hipMemcpyDeviceToHost, nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
        sync_guard.armed = false;
        memcpy(out, hout.p, sizeof(double) * n_out);
        return MCSAS_OK;
    });
}

// hist2d_kernel.h — the joint histogram of two parameter columns (include/mcsas_hip.h: mcsas_hip_histogram2d): the record of a
// histogram on the device, the LDS a (histogram, repetition) needs, and hist2d_kernel.  host_hist.hip packs the records and launches
// it; tools/microbench_hist2d.hip times it alone.  Per axis every rule is hist_bins_body's (hist_kernels.h), so that one y column
// that holds every value gives that kernel's bins bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "device_util.h"

using mcsas::WAVE;

constexpr int HIST2D_MAX_CONTRIBS = 4096;                  // host_hist.hip HIST_MAX_CONTRIBS, engine.HISTOGRAM_MAX_CONTRIBS
constexpr int HIST2D_MAX_CELLS = 4096;                     // engine.HISTOGRAM2D_MAX_CELLS
constexpr unsigned HIST2D_NO_CELL = 0xffffu;               // a contribution in no cell; a cell's flat index stays below HIST2D_MAX_CELLS
struct Hist2dSpecDev { int32_t px, py, weight, nx, ny, pad; int64_t edge_off, out_off; double lox, hix, loy, hiy; };

// The dynamic LDS of one (histogram, repetition), in bytes.  Staged for the whole block: f [N], lim [N] doubles and cell [N] 16-bit.
// Behind them one shared region, used three times over: the two edge vectors while the cells are looked up; the cells' sums, limit
// sums (doubles) and counts (32-bit) while the contributions are walked; x [N], y [N] for the moments once the cells are written out.
__host__ __device__ constexpr size_t hist2d_staged_bytes(size_t N) { return 16 * N + (2 * N + 7) / 8 * 8; }
__host__ __device__ constexpr size_t hist2d_shared_bytes(size_t N, size_t nx, size_t ny) {
    const size_t cells = (nx * ny * 20 + 7) / 8 * 8, edges = nx * ny ? 8 * (nx + ny + 2) : 0, xy = 16 * N;
    return cells > edges ? (cells > xy ? cells : xy) : (edges > xy ? edges : xy);
}
// at the caps (4096 contributions; 4096 cells as 1 x 4096, the longest edges, or 64 x 64) a block fits the 160 KiB of a CU
static_assert(hist2d_staged_bytes(HIST2D_MAX_CONTRIBS) + hist2d_shared_bytes(HIST2D_MAX_CONTRIBS, 1, HIST2D_MAX_CELLS) + 64 <= 160 * 1024, "hist2d LDS");
static_assert(hist2d_staged_bytes(HIST2D_MAX_CONTRIBS) + hist2d_shared_bytes(HIST2D_MAX_CONTRIBS, 64, 64) + 64 <= 160 * 1024, "hist2d LDS");

// #{k : e[k] <= x} - 1 over the n + 1 non-decreasing edges e[0..n]: -1 for a NaN (no comparison holds) and below e[0], n from e[n] on
__device__ __forceinline__ int hist2d_column(const double *e, int n, double x) {
    int lo = 0, hi = n + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// The ordered sums read their LDS operands a batch ahead of the additions that wait for one another (as hist_colsum_body does with
// its rows): the order of the additions, and so every bit of a sum, is that of the plain loop.
constexpr int HIST2D_BATCH = 8;
// acc = 0.; acc += term(x[c], y[c], f[c]) over c = 0 .. N - 1 in order
template <class Term>
__device__ __forceinline__ double hist2d_ordered_sum(int N, const double *lx, const double *ly, const double *lf, Term term) {
    double acc = 0.;
    int c = 0;
    for (; c + HIST2D_BATCH <= N; c += HIST2D_BATCH) {
        double x[HIST2D_BATCH], y[HIST2D_BATCH], f[HIST2D_BATCH];
#pragma unroll
        for (int i = 0; i < HIST2D_BATCH; ++i) { x[i] = lx[c + i]; y[i] = ly[c + i]; f[i] = lf[c + i]; }
#pragma unroll
        for (int i = 0; i < HIST2D_BATCH; ++i) acc += term(x[i], y[i], f[i]);
    }
    for (; c < N; ++c) acc += term(lx[c], ly[c], lf[c]);
    return acc;
}

// One wave per (histogram, repetition), in two phases.
// Cells: lane l looks up the cells of contributions l, l + 64, ... by binary search over the edges in LDS and stages cell, fraction and
// limit; then every lane walks ALL contributions in order and adds contribution c iff cell[c] % 64 is its own lane — a cell has one
// owner, so there is no atomic and no race, a cell's sum is in contribution order whatever the bin counts, and the walk costs N
// iterations whatever the cell count (hist_bins_body's lane-per-bin walk would cost N cells / 64).
// Moments: ordered single-lane sums like hist_bins_body's, side by side: lanes 0 / 1 / 2 take tot, mx, my, then vxx, vyy, cxy.
__device__ __forceinline__ void hist2d_body(int N, int P, int R, int r, const Hist2dSpecDev s, const double *contribs, const double *frac8,
                                            const double *edges_all, double *out, unsigned char *lds) {
    __shared__ double mom[4];
    const int lane = threadIdx.x, nx = s.nx, ny = s.ny, cells = nx * ny;
    const size_t NR = (size_t)N * R;
    const double *fr = frac8 + (size_t)s.weight * NR, *lim = frac8 + (size_t)(4 + s.weight) * NR;
    double *bins = out + s.out_off, *obs = bins + (size_t)cells * R, *mo = obs + (size_t)cells * R;
    double *lf = reinterpret_cast<double *>(lds), *ll = lf + N;
    unsigned short *lcell = reinterpret_cast<unsigned short *>(ll + N);
    unsigned char *shared = lds + hist2d_staged_bytes(N);
    for (int c = lane; c < N; c += WAVE) lf[c] = fr[(size_t)c * R + r];
    if (cells > 0) {
        double *ex = reinterpret_cast<double *>(shared), *ey = ex + nx + 1;
        const double *gx = edges_all + s.edge_off, *gy = gx + nx + 1;
        for (int k = lane; k <= nx; k += WAVE) ex[k] = gx[k];
        for (int k = lane; k <= ny; k += WAVE) ey[k] = gy[k];
        __syncthreads();
        for (int c = lane; c < N; c += WAVE) {
            const int i = hist2d_column(ex, nx, contribs[((size_t)c * P + s.px) * R + r]);
            const int j = hist2d_column(ey, ny, contribs[((size_t)c * P + s.py) * R + r]);
            lcell[c] = (unsigned short)((i >= 0 && i < nx && j >= 0 && j < ny) ? (unsigned)(i * ny + j) : HIST2D_NO_CELL);
            ll[c] = lim[(size_t)c * R + r];
        }
        __syncthreads();                                       // (the edges are done with: the cells take their place)
        double *sb = reinterpret_cast<double *>(shared), *so = sb + cells;
        unsigned *cnt = reinterpret_cast<unsigned *>(so + cells);
        for (int k = lane; k < cells; k += WAVE) { sb[k] = 0.; so[k] = 0.; cnt[k] = 0u; }
        __syncthreads();
        const auto add = [&](unsigned k, double f, double l) {
            if (k != HIST2D_NO_CELL && (int)(k % WAVE) == lane) { sb[k] += f; so[k] += l; cnt[k] += 1u; }
        };
        int c = 0;
        for (; c + HIST2D_BATCH <= N; c += HIST2D_BATCH) {     // (the staged values of a batch are read ahead of its additions)
            unsigned k[HIST2D_BATCH];
            double f[HIST2D_BATCH], l[HIST2D_BATCH];
#pragma unroll
            for (int i = 0; i < HIST2D_BATCH; ++i) { k[i] = lcell[c + i]; f[i] = lf[c + i]; l[i] = ll[c + i]; }
#pragma unroll
            for (int i = 0; i < HIST2D_BATCH; ++i) add(k[i], f[i], l[i]);
        }
        for (; c < N; ++c) add(lcell[c], lf[c], ll[c]);
        for (int k = lane; k < cells; k += WAVE) {             // (a lane's own cells: k % 64 == lane)
            const double v = sb[k], n = (double)cnt[k];
            bins[(size_t)k * R + r] = (v != v) ? 0. : v;       // bins[isnan(bins)] = 0
            obs[(size_t)k * R + r] = n > 0. ? so[k] / n : 0.;
        }
    }
    __syncthreads();                                           // (the cells are written out: x and y take their place)
    double *lx = reinterpret_cast<double *>(shared), *ly = lx + N;
    for (int c = lane; c < N; c += WAVE) {
        lx[c] = contribs[((size_t)c * P + s.px) * R + r];
        ly[c] = contribs[((size_t)c * P + s.py) * R + r];
    }
    __syncthreads();
    double acc = 0.;
    int any = 0;
    const auto inside = [&](double x, double y) { return x > s.lox && x < s.hix && y > s.loy && y < s.hiy; };
    if (lane < 3)
        acc = hist2d_ordered_sum(N, lx, ly, lf, [&](double x, double y, double f) {
            const bool ok = inside(x, y);
            any |= ok;
            return ok ? (lane == 0 ? f : (lane == 1 ? x : y) * f) : 0.;
        });
    if (lane == 0) mom[0] = acc;
    __syncthreads();
    const double tot = mom[0];
    if ((lane == 1 || lane == 2) && tot != 0.) acc /= tot;
    if (lane == 1 || lane == 2) mom[lane] = acc;
    __syncthreads();
    const double mx = mom[1], my = mom[2];
    acc = 0.;
    if (lane < 3)
        acc = hist2d_ordered_sum(N, lx, ly, lf, [&](double x, double y, double f) {
            const double dx = x - mx, dy = y - my;
            const double a = lane == 1 ? dy : dx, b = lane == 0 ? dx : dy;       // lane 0: dx dx, 1: dy dy, 2: dx dy
            return inside(x, y) ? (a * b) * f : 0.;
        });
    __syncthreads();                                           // (mom[1], mom[2] are read: the second moments take their place beside tot)
    if (lane < 3) mom[1 + lane] = acc / tot;
    __syncthreads();
    if (lane == 0) {
        const double vxx = mom[1], vyy = mom[2], cxy = mom[3];
        const double den = sqrt(fabs(vxx)) * sqrt(fabs(vyy));
        const double rho = den != 0. ? cxy / den : 0.;         // (only an exact zero is skipped; NaN goes on, as hist_bins_body's skew does)
        const double m7[7] = {tot, mx, my, vxx, vyy, cxy, rho};
        for (int k = 0; k < 7; ++k) mo[(size_t)k * R + r] = any ? m7[k] : 0.;
    }
}
// block b = histogram b / R, repetition b % R
__global__ __launch_bounds__(64) void hist2d_kernel(int N, int P, int R, const double *contribs, const double *frac8, const double *edges_all,
                                                    const Hist2dSpecDev *specs, double *out) {
    extern __shared__ double hl[];
    hist2d_body(N, P, R, (int)(blockIdx.x % (unsigned)R), specs[blockIdx.x / (unsigned)R], contribs, frac8, edges_all, out,
                reinterpret_cast<unsigned char *>(hl));
}

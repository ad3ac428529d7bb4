// hist_partial_kernel.h — the partial intensities of histogram ranges and bins (include/mcsas_hip.h: mcsas_hip_histogram_partial,
// mcsas_hip_histogram_partial_device_rows; the reference's Moments.intensity, utils/parameter.py:124-154): the record of a wanted
// histogram on the device, the LDS a block needs, and hist_partial_kernel.  host_hist.hip packs the records and launches it on a
// block of repetitions' rows while they still lie in HBM, behind the fit (HistOnDevice::run; the scale of a repetition is known by then).
//   range[k][r]  = A * sum_c rows[c][k] over the contributions with lower < x_c < upper        (hist_bins_body's `ok`)
//   bin[b][k][r] = A * sum_c rows[c][k] over those with edges[b] <= x_c < edges[b+1] && x_c < edges[n_bin]   (its bins)
// each sum in contribution order from +0.0, ONE product with A = scaling[0][r] at the end; with -ffp-contract=off that is what
// parameter.partial_intensities does in numpy, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "device_util.h"

constexpr int HIST_PARTIAL_MAX_CONTRIBS = 4096;            // host_hist.hip HIST_MAX_CONTRIBS, engine.HISTOGRAM_MAX_CONTRIBS
constexpr int HIST_PARTIAL_MAX_BINS = 256;                 // engine.HISTOGRAM_PARTIAL_MAX_BINS: a bin's 64 running sums lie in LDS
constexpr int HIST_PARTIAL_TILE = 64;                      // q-points of a block: one per lane
constexpr unsigned HIST_PARTIAL_NO_BIN = 0x7fffu;          // the low 15 bits of a contribution's word: its bin, or none
constexpr unsigned HIST_PARTIAL_IN_RANGE = 0x8000u;        // ... and the top bit: inside the value range
static_assert(HIST_PARTIAL_MAX_BINS < (int)HIST_PARTIAL_NO_BIN, "a bin index fits the word");
static_assert(HIST_PARTIAL_TILE == mcsas::WAVE, "one wave per block, one q-point per lane");

// a wanted histogram: its parameter column, bins and value range, what is wanted (1: the range curve, 2: the bin curves too),
// where its edges begin among the set's edges and its curves in the block of curves: range [nq][R], then bin [nb][nq][R]
struct HistPartialDev { int32_t pidx, nb, want, pad; int64_t edge_off, out_off; double lo, hi; };

// The dynamic LDS of one block, in bytes: a 16-bit word per contribution; with bin curves, in front of them, the running sums
// acc[nb][64] (lane-contiguous doubles: a wave's read or write of one bin's 64 sums touches every bank equally) and the nb + 1 edges.
__host__ __device__ constexpr size_t hist_partial_lds_bytes(size_t N, size_t nb, int want) {
    return (want == 2 ? 8 * (nb * HIST_PARTIAL_TILE + nb + 1) : 0) + (2 * N + 7) / 8 * 8;
}
// at the caps (256 bins, 4096 contributions) a block takes about 138 KiB of a CU's 160 KiB
static_assert(hist_partial_lds_bytes(HIST_PARTIAL_MAX_CONTRIBS, HIST_PARTIAL_MAX_BINS, 2) == 256 * 64 * 8 + 257 * 8 + 4096 * 2, "hist_partial LDS");
static_assert(hist_partial_lds_bytes(HIST_PARTIAL_MAX_CONTRIBS, HIST_PARTIAL_MAX_BINS, 2) + 64 <= 160 * 1024, "hist_partial LDS");

// #{k : e[k] <= x} - 1 over the n + 1 non-decreasing edges e[0..n]: -1 for a NaN (no comparison holds) and below e[0], n from e[n]
// on.  With 0 <= b < n that is hist_bins_body's `e[b] <= x && x < e[b + 1] && x < e[n]`, and the one b for which it holds.
__device__ __forceinline__ int hist_partial_bin(const double *e, int n, double x) {
    int lo = 0, hi = n + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

constexpr int HIST_PARTIAL_BATCH = 8;                      // rows read ahead of their additions, as hist_colsum_body reads them

// One wave: wanted histogram w, repetition r (whose N rows begin at `rows`, pitch nq), q-points 64 tile .. 64 tile + 63.
// Words: lane l files contributions l, l + 64, ...: the bin by binary search over the edges staged in LDS, the range flag by the
// two strict comparisons.  Walk: lane l owns q index k = 64 tile + l and adds the rows in contribution order — a row is one
// coalesced 512-byte read; the word of a contribution is the same for the whole wave, so neither test diverges; an in-range row
// goes to a register, a bin's member to acc[bin][l], which no other lane touches: no atomic, no barrier inside the walk, and
// nothing depends on how blocks are scheduled.  A lane beyond nq loads and stores nothing.
__device__ __forceinline__ void hist_partial_body(int nq, int N, int P, int R, int r, int tile, const HistPartialDev w, const double *rows,
                                                  const double *contribs, const double *scaling, const double *edges_all, double *partial,
                                                  unsigned char *lds) {
    const int lane = threadIdx.x, nb = w.want == 2 ? w.nb : 0;
    double *acc = reinterpret_cast<double *>(lds), *le = acc + (size_t)nb * HIST_PARTIAL_TILE;
    unsigned short *word = reinterpret_cast<unsigned short *>(lds + (w.want == 2 ? 8 * ((size_t)nb * HIST_PARTIAL_TILE + nb + 1) : 0));
    if (w.want == 2) {
        const double *ge = edges_all + w.edge_off;
        for (int k = lane; k <= nb; k += HIST_PARTIAL_TILE) le[k] = ge[k];
        __syncthreads();
    }
    for (int c = lane; c < N; c += HIST_PARTIAL_TILE) {
        const double x = contribs[((size_t)c * P + w.pidx) * R + r];
        unsigned s = (x > w.lo && x < w.hi) ? HIST_PARTIAL_IN_RANGE : 0u;
        const int b = nb > 0 ? hist_partial_bin(le, nb, x) : -1;
        s |= (b >= 0 && b < nb) ? (unsigned)b : HIST_PARTIAL_NO_BIN;
        word[c] = (unsigned short)s;
    }
    __syncthreads();
    const int k = tile * HIST_PARTIAL_TILE + lane;
    if (k >= nq) return;                                       // (behind the last barrier)
    double *mine = acc + lane;                                 // acc[b][lane] = mine[64 b]
    for (int b = 0; b < nb; ++b) mine[(size_t)b * HIST_PARTIAL_TILE] = 0.;
    const double *base = rows + k;
    double in_range = 0.;
    const auto add = [&](unsigned s, double v) {
        s = (unsigned)__builtin_amdgcn_readfirstlane((int)s);  // (the same word in every lane: the tests below are scalar)
        if (s & HIST_PARTIAL_IN_RANGE) in_range += v;
        const unsigned b = s & HIST_PARTIAL_NO_BIN;
        if (b != HIST_PARTIAL_NO_BIN) mine[(size_t)b * HIST_PARTIAL_TILE] += v;
    };
    int c = 0;
    for (; c + HIST_PARTIAL_BATCH <= N; c += HIST_PARTIAL_BATCH) {
        double v[HIST_PARTIAL_BATCH];
        unsigned s[HIST_PARTIAL_BATCH];
#pragma unroll
        for (int i = 0; i < HIST_PARTIAL_BATCH; ++i) { v[i] = base[(size_t)(c + i) * nq]; s[i] = word[c + i]; }
#pragma unroll
        for (int i = 0; i < HIST_PARTIAL_BATCH; ++i) add(s[i], v[i]);
    }
    for (; c < N; ++c) add(word[c], base[(size_t)c * nq]);
    const double A = scaling[r];
    double *range = partial + w.out_off, *bin = range + (size_t)nq * R;
    range[(size_t)k * R + r] = A * in_range;
    for (int b = 0; b < nb; ++b) bin[((size_t)b * nq + k) * R + r] = A * mine[(size_t)b * HIST_PARTIAL_TILE];
}
// grid (q tiles, wanted histograms, repetitions of the block): repetition r0 + blockIdx.z, whose rows are the blockIdx.z-th N of `rows`
__global__ __launch_bounds__(64) void hist_partial_kernel(int nq, int N, int P, int R, int r0, const double *rows, const double *contribs,
                                                          const double *scaling, const double *edges_all, const HistPartialDev *wanted,
                                                          double *partial) {
    extern __shared__ double hl[];
    const int rl = blockIdx.z;
    hist_partial_body(nq, N, P, R, r0 + rl, (int)blockIdx.x, wanted[blockIdx.y], rows + (size_t)rl * N * nq, contribs, scaling, edges_all, partial,
                      reinterpret_cast<unsigned char *>(hl));
}

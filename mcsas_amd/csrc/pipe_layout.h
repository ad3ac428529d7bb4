// pipe_layout.h — what the host and the kernels of the whole-chip pipeline (chain_pipe.h) share: the argument blocks and the
// per-chain records as they lie in memory, the PIPE_* constants, and the geometry of a launch (pipe_geometry, host).
// No device code: the host unit (mcsas_hip.hip) includes this header and none of the kernel templates.
#pragma once
#include "chain_common.h"

namespace mcsas {

struct PipeSnap {                 // what the producer needs to know about a chain
    int32_t attempt, t_init, alive, pad;
    uint64_t init_base;           // draw index of the initial parameter set of this attempt
    uint64_t step_base;           // draw index of step 0 of this attempt
};

struct PipeChain {                // per-chain scanner state, lives in HBM between ticks
    PipeSnap snap[2];
    double SC, SIC, SCC, A, b, chi2;
    double X;                     // chi²·Q as the decisions carry it (PipeGeom::resum_every)
    int64_t num_iter, num_moves, total_steps;
    uint64_t draw_pos, t_start;
    int32_t attempts, converged, stopped, overflow, done, pad;
#ifdef MCSAS_STAMPS
    int64_t dbg[20];
    uint64_t last_end;            // wall clock (10 ns) at the end of this chain's previous scan block
#endif
};

struct PipeGeom {
    int32_t kb;                   // steps per window (tick)
    int32_t w;                    // steps per sub-window = rows per producer block = 8 * rows_per_wave (<= 64)
    int32_t rows_per_wave;        // producer: rows per wave
    int32_t prod_blocks_y;        // producer blocks (= sub-windows) per chain and tick
    int32_t scan_waves;           // waves of a scan block
    int32_t qpl;
    int32_t gram_off;             // producer LDS: offset (doubles) of the Gram reduction buffer
    int32_t sub_per_block;        // scan sub-windows per producer block (8 * rows_per_wave / w)
    int32_t lazy_rows;            // no `new` rows are stored: an accepted step marks its contribution's cached row stale and the producer that
                                  // next needs it as `old` evaluates it again from the parameter set (rows without an integral only)
    int32_t overlap;              // producer variant (tuning): the Gram MFMAs of sub-window s are issued between the rows of s + 1, operands from HBM/L2
    int32_t gram_lds;             // producer: the sub-window's d rows are also kept in LDS and the Gram MFMAs read them from there
    int32_t drow_off;             // producer LDS: offset (doubles) of those rows, row stride qpad + PIPE_DROW_PAD
    int32_t resum_every;          // 0: the running sums are re-derived from ft at the end of every window (the window is fixed: rows without an
                                  // integral); n: at every n-th step of the attempt instead, and chi²·Q is carried across windows exactly —
                                  // nothing a chain decides then depends on the window, which follows the chain count for rows with an integral
    int32_t rowq;                 // rows with an integral (round 4): the producer waves of a chain PULL the window's rows from a queue, most expensive
                                  // first (no static deal), and the scan block works out the 8-step Gram blocks itself from the rows in its LDS
    int32_t rec_off;              // producer LDS offset (doubles) of the proposal records: the window's (rowq), the block's (gram_lds: PIPE_PROP_DOUBLES each)
    int32_t help;                 // rowq: a producer block whose chain's queue is empty joins another chain's (pipe_prod_rowq)
    uint64_t prod_lds, scan_lds;
};

struct PipeArgs {
    ChainArgs c;                  // c.cache_rows = N + 2*kb
    PipeGeom g;
    PipeChain *chains;            // [R]
    double *ft, *wft;             // [R][qpad]
    int32_t *slot_of;             // [R][N]
    int32_t *stage_slot;          // [R][2][kb]
    double *dwin;                 // [R][2][kb][qpad]   d rows of the window
    double *gwin;                 // [R][2][kb][w]      Gram blocks: row = step in the window, column = step in ITS sub-window
    double *scal;                 // [R][2][kb][4]   a = Σ w d, e = Σ wI d, g = Σ w d² of every step's row
    int32_t *row_valid;           // [R][N]  lazy_rows: 1 = the contribution's cached row is current
    double *pval;                 // [R][2][kb][MAX_ACTIVE]
    int32_t *povf;                // [R][2][kb]
    int32_t *rowq;                // [R][2]  rowq: next row of the window to hand out, by tick parity (zeroed by the scan block a tick ahead)
    int32_t *n_done;              // host-mapped: set to the number of chains when the last one has finished
    int32_t *n_done_dev;          // device counter behind it (one system-scope atomic per chain cost the last tick 30 us)
    int32_t tick, pad;            // unused: the tick travels as its own kernel argument
    uint64_t *timeline;           // stamps build: [blocks][8 waves][2] wall clock (10 ns) at wave start / end of tick `timeline_tick`
    int32_t timeline_tick, pad1;
};

// What a workgroup needs in its first microsecond, passed BY VALUE (kernel-argument segment, scalar loads): reading these
// through the argument block in device memory costs a dependent global round trip before the first useful load can be
// issued — pointer, then data — on the critical path of every tick.
struct PipeHot {
    const double *q, *w, *wI, *q3inv;                          // q3inv = 1 / q^3, host-made (the same IEEE operations as on the device)
    PipeChain *chains;
    int32_t n_reps, n_contrib, n_active, qpad, kb, prod_blocks_y, w_sub, pad;
    int64_t max_iter;
};

constexpr int PIPE_BLOCK = 512;      // threads per workgroup of the tick kernel (8 waves)
constexpr int PIPE_WAVES = PIPE_BLOCK / 64;
constexpr int PIPE_GRAM_TILES_PER_ROUND = 2;   // producer: 16x16 Gram tiles summed across the 8 waves per LDS round (32 KB), one thread per tile element
constexpr int PIPE_DROW_PAD = 8;         // LDS d rows: stride qpad + 8 doubles, so that the 64 16-byte operands of one Gram load hit 64 different bank groups
constexpr int PIPE_PROP_DOUBLES = 12;    // producer: doubles per Contrib record in LDS (a stale row's; a proposal's, whose last double holds its two row slots)
constexpr int PIPE_GRAM_NT_MAX = 3;         // overlapped producer: tiles per sub-window — W <= 32 (two 16-row groups: 3 tiles) or 24 packed (2)
constexpr int PIPE_RESUM_STEPS = 64;        // rows with an integral: the running sums are re-derived from ft every 64 steps of an attempt (a multiple of the 8-step sub-window)
constexpr int PIPE_MAX_ROW_DOUBLES = 32;   // scan block: doubles per lane held in row registers (rows per wave and sub-window x q per lane)
#define PIPE_TL_WORDS 30                 /* timeline record of a wave: start, end, HW_ID, XCC_ID, then 26 marks */

// rows_per_wave_req: 0 = automatic, else the requested rows per producer wave (diagnostic / tuning)
static inline int pipe_geometry(int nq, int n_contrib, int tab_doubles, int heavy_rows, int rows_per_wave_req, int sub_req, int gram_global_req, int eager_req, int n_chains, int n_cus, PipeGeom *g,
                                int contrib_doubles) {
    int qpl = 1;
    while (qpl * 64 < nq) qpl *= 2;
    if (qpl > 16) return 1;
    const int qpad = qpl * 64;
    g->rowq = 0; g->rec_off = 0; g->help = 0;
    if (heavy_rows) {
        // Rows that cost an integral each (round 4).  The window is as long as 2 Kb <= N allows (a multiple of the 8-step Gram
        // blocks, at most 512 steps: one proposal per thread of a block) — shortened by the few-chains rule below, which DOES
        // follow the chain count —, every chain gets the producer blocks that are left beside the scan blocks, and their waves pull the window's rows from
        // a queue in order of predicted cost: a wave that drew a cheap row simply comes back sooner.
        int kb = (n_contrib / 2) & ~7;
        int cap = PIPE_BLOCK;                                  // (one proposal per thread; 13 worm chains: 296 steps per window 4.12e6 steps/s, 256: 3.86e6)
#ifndef __HIPCC_RTC__
        if (const char *e = getenv("MCSAS_HIP_PIPE_KB_CAP")) { const int v = atoi(e) & ~7; if (v >= 8 && v <= PIPE_BLOCK) cap = v; }   // (measurement knob, host only)
#endif
        if (kb > cap) kb = cap;
        // Few chains (round 5): a tick hands R x Kb rows to 8 waves per CU, and while that is only a few "rounds" of rows the
        // tick lasts c0 + ceil(rounds) x (a row's time) — config 3's per-GPU share, 25 chains x 200 rows on 2048 wave slots, is 2.44
        // rounds: a third round for a sixth of the rows; a window of 160 steps (1.95 rounds) runs 8.5 % faster (tools/kb_probe.py:
        // 5.72 against 5.27e6 steps/s; the fixed part c0 of a tick — proposal records, scan blocks, the boundary — measured 0.7-0.95
        // of a row's time, which is why halving the window to get ONE round loses: 13 worm chains, 296 -> 152 steps, -22 %).  Between two
        // and four rounds the window is the multiple of 8 in [Kb/2, Kb] that maximises Kb / (0.75 + ceil(rounds)), the longest unless another
        // is 2 % better; from four rounds on the queue evens the rounds out and the longest window wins (measured: configs 3 at 200
        // chains, 4 at 50).  Nothing a chain decides depends on the window (PipeGeom::resum_every): same arrays, bit for bit.
        if (n_chains > 0 && n_cus > 0) {
            const double slots = 8.0 * (double)n_cus;
            auto rate = [&](int c) { const double r = (double)n_chains * c / slots; return (double)c / (0.75 + (double)(long long)(r + 1.0 - 1e-9)); };
            const double rmax = (double)n_chains * kb / slots;
            if (rmax > 2.0 && rmax < 4.0) {                      // (a third or fourth round to shed; 2 -> 1 loses: 6 chains of config 4, 496 -> 336 steps, -10 %)
                int best = kb;
                double best_v = rate(kb);
                for (int c = kb - 8; c >= 8 && 2 * c >= kb; c -= 8)
                    if (rate(c) > best_v * 1.02) { best_v = rate(c); best = c; }
                kb = best;
            }
        }
#ifndef __HIPCC_RTC__
        if (const char *e = getenv("MCSAS_HIP_PIPE_KB")) { const int v = atoi(e) & ~7; if (v >= 8 && v <= ((n_contrib / 2) & ~7) && v <= cap) kb = v; }     // (measurement knob, host only)
#endif
        if (kb < 8) return 1;
        // producer blocks per chain: enough to cover every CU by themselves — the launch then holds more workgroups than CUs, the
        // scan blocks (dispatched first) are done within a tenth of a tick, and the producer blocks that were waiting take over
        // their CUs and pull what is left of their chain's window (a static deal would leave those CUs idle for the rest of the tick)
        int by = 8;
        if (n_chains > 0 && n_cus > 0) { by = (n_cus + n_chains - 1) / n_chains; if (by < 1) by = 1; if (by > 32) by = 32; if (by * 8 > kb) by = (kb + 7) / 8; }
        g->kb = kb; g->qpl = qpl; g->w = 8; g->sub_per_block = 1; g->rows_per_wave = 1; g->prod_blocks_y = by;
        g->gram_off = 4 * qpad + tab_doubles; g->resum_every = PIPE_RESUM_STEPS;
        g->overlap = 0; g->gram_lds = 0; g->drow_off = 0; g->lazy_rows = 0;
        g->rowq = 1; g->rec_off = g->gram_off + 16;
        const size_t rec = (size_t)kb * (contrib_doubles + MCSAS_MAX_ACTIVE + 2) + ((size_t)3 * kb + 1) / 2;      // records; rank -> step and the two row slots (int32)
        g->prod_lds = sizeof(double) * ((size_t)g->rec_off + rec);
        g->help = (n_chains > 1 && (size_t)n_chains <= 2 * rec) ? 1 : 0;       // (the helpers' table of rows left per chain takes the records' place)
#ifndef __HIPCC_RTC__
        if (const char *e = getenv("MCSAS_HIP_PIPE_HELP")) g->help = atoi(e) ? g->help : 0;                           // (measurement knob, host only)
#endif
        g->scan_waves = PIPE_WAVES;
        g->scan_lds = sizeof(double) * ((size_t)g->w * qpad + 2 * (size_t)g->w * g->w + 3 * (size_t)qpad + (size_t)g->kb * 4 + 64)
                    + sizeof(int32_t) * (4 * (size_t)g->kb + 1 + 1 + 64 + 4 + 8) + 64;
        if (g->scan_lds > 160 * 1024 || g->prod_lds > 160 * 1024) return 2;     // (2: the window's records / row buffers do not fit the LDS)
        return 0;
    }
    // window: as many steps as 2*Kb <= N allows, Kb = (sub-windows) x (8 producer waves) x (rows per wave).
    // Rows per wave set the sub-window W = 8 rpw: measured on config 2 (tools/sweep_flags.sh) W = 48 beats 64
    // (Gram tiles per step fall from 10/64 to 6/48 and four producer blocks per chain instead of three fill
    // the CUs the scan blocks leave free) and 32 (more scan sub-windows per tick): candidates in that order,
    // the first one whose window is within 15 % of the largest wins.
    // scan sub-window for `r` rows per producer wave: the largest multiple of 8 that divides the producer block's rows and
    // whose d rows fit the scan block's LDS row buffer (the accepted rows are applied to ft from there, not from HBM).
    // The overlapped producer (Gram of sub-window s between the rows of s + 1) has tile schemes for W <= 32.
    const bool overlap = gram_global_req;
    auto pick_w = [&](int r) {
        int w = 8;
        for (int ws = 8; ws <= 8 * r && ws <= (overlap ? 32 : 64); ws += 8) {
            const int rps = ws / 8;
            if (rps == 5 || rps == 7 || rps * qpl > PIPE_MAX_ROW_DOUBLES) continue;   // the kernels instantiate 1, 2, 3, 4, 6, 8 rows per wave
            if ((8 * r) % ws == 0 && sizeof(double) * (size_t)ws * qpad <= 96 * 1024 && (sub_req == 0 || ws <= 8 * sub_req)) w = ws;
        }
        return w;
    };
    int rpw = 0, by = 0;
    if (rows_per_wave_req >= 1 && rows_per_wave_req <= 8) {
        rpw = rows_per_wave_req;
        while (rpw > 1 && 2 * 8 * rpw > n_contrib) --rpw;
        if (2 * 8 * rpw > n_contrib) return 1;
        by = n_contrib / (2 * 8 * rpw);
        if (by * 8 * rpw > 256) by = 256 / (8 * rpw);
    } else {
        static const int order[6] = {6, 8, 4, 3, 2, 1};
        int kbs[6], best_kb = 0;
        for (int c = 0; c < 6; ++c) {
            const int r = order[c];
            int b = (2 * 8 * r > n_contrib) ? 0 : n_contrib / (2 * 8 * r);
            if (b * 8 * r > 256) b = 256 / (8 * r);
            kbs[c] = b * 8 * r;
            if (kbs[c] > best_kb) best_kb = kbs[c];
        }
        if (best_kb == 0) return 1;
        // default: the first candidate whose window is within 15 % of the largest
        int rpw_d = 0, by_d = 0;
        for (int c = 0; c < 6 && !rpw_d; ++c)
            if (kbs[c] > 0 && 20 * kbs[c] >= 17 * best_kb) { rpw_d = order[c]; by_d = kbs[c] / (8 * rpw_d); }
        // Few chains: more, smaller producer blocks per chain shorten the producers' critical path (start-up + rows
        // per wave + Gram) down to where the scan block becomes the longer one — as long as every block still gets a
        // CU of its own.  Measured at 512 q x 400 (tools/sweep_rpw.sh): 3 rows per wave 3.1-3.3 ms per launch up to 28
        // chains, 6 rows 3.8-4.0 ms up to 51.  Only candidates with the SAME window and the same scan sub-window as
        // the default qualify: a chain's decisions depend on both (where the running sums are re-derived from ft, which
        // pairs of steps go through the Gram block), and a repetition must come out the same whether it runs beside 6
        // others (one of eight GPUs) or beside 49.
        if (n_chains > 0 && n_cus > 0) {
            static const int small_first[6] = {3, 4, 6, 8, 2, 1};
            for (int c = 0; c < 6 && !rpw; ++c) {
                const int r = small_first[c];
                int b = (2 * 8 * r > n_contrib) ? 0 : n_contrib / (2 * 8 * r);
                if (b * 8 * r > 256) b = 256 / (8 * r);
                if (b > 0 && b * 8 * r == by_d * 8 * rpw_d && pick_w(r) == pick_w(rpw_d) && n_chains * (b + 1) <= n_cus) { rpw = r; by = b; }
            }
        }
        if (!rpw) { rpw = rpw_d; by = by_d; }
    }
    g->kb = by * 8 * rpw; g->qpl = qpl;
    g->w = pick_w(rpw);
    g->sub_per_block = 8 * rpw / g->w;
    g->rows_per_wave = rpw;
    g->prod_blocks_y = by;
    g->gram_off = 4 * qpad + tab_doubles;
    g->resum_every = 0;
    {
        // reduction buffer of the Gram tiles: [8 waves][tiles][256]; the overlapped producer keeps two of them (the block of
        // sub-window s is summed while the partial tiles of s + 1 are being parked)
        const size_t red = overlap ? (size_t)2 * PIPE_WAVES * PIPE_GRAM_NT_MAX * 256 : (size_t)PIPE_WAVES * PIPE_GRAM_TILES_PER_ROUND * 256;
        g->prod_lds = sizeof(double) * ((size_t)g->gram_off + 16 + red);    // 16 doubles: counters
        g->overlap = overlap ? 1 : 0;
        // Rows without an integral: the Gram phase is a third of the producer's tick; with the sub-window's d rows parked
        // in LDS on their way to HBM it is MFMA-bound instead of waiting for an L2 round trip per sub-window.
        // Behind the rows the block's proposal records (its waves claim rows one by one and read a row's proposal from there).
        g->gram_lds = 0; g->drow_off = 0;
        const size_t drows = (size_t)g->w * (qpad + PIPE_DROW_PAD);
        const size_t with_rows = g->prod_lds + sizeof(double) * (drows + (size_t)8 * rpw * PIPE_PROP_DOUBLES);
        if (!overlap && with_rows <= 160 * 1024) {
            g->gram_lds = 1; g->drow_off = g->gram_off + 16 + (int)red; g->rec_off = g->drow_off + (int)drows; g->prod_lds = with_rows;
        }
        // ... and no `new` rows go to HBM either (4 KB per step at Q = 512, a fifth of the tick's memory traffic): see lazy_rows
        g->lazy_rows = ((g->gram_lds || overlap) && !eager_req) ? 1 : 0;
        // pipe_prod_block has these two paths and no third: with neither, no window row would be written and the scan would
        // decide on stale buffers.  (With tables of up to 1264 doubles the row buffer and the records fit for every W pick_w
        // allows — the tightest is 512 q, W = 24, six rows per wave —; the built-in models without an integral have none.)  The overlapped producer exists in a tuning build only.
        if (!g->gram_lds && !g->overlap) return 2;
#ifndef MCSAS_TUNING
        if (g->overlap) return 2;
#endif
    }
    g->scan_waves = PIPE_WAVES;
    // scan block LDS: the sub-window's d rows, two Gram blocks (double buffer), ft and w*ft, the window's scalars, h of
    // the sub-window, flags / slot tables / accepted lists
    g->scan_lds = sizeof(double) * ((size_t)g->w * qpad + 2 * (size_t)g->w * g->w + 2 * (size_t)qpad + (size_t)g->kb * 4 + 64)
                + sizeof(int32_t) * (4 * (size_t)g->kb + 1 + 1 + 64 + 4 + 8) + 64;
    if (g->scan_lds > 160 * 1024 || g->prod_lds > 160 * 1024) return 2;
    return 0;
}

}  // namespace mcsas

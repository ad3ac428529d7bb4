// host_decide.h — what libmcsas_hip.so decides without a device (host_decide.hip), beside what host_internal.h declares of that unit
// for every host unit (the refusals, the family table, the trace block's layout): how a problem runs, how a kernel family is launched
// and named, a fetched trace block's transposition, a pipeline launch's ticks.  None of it calls the HIP runtime.
#pragma once
#include "host_internal.h"
#include "chain_wg.h"    // WgGeom / wg_geometry only; the kernels are instantiated in kern_*.hip
#include "pipe_layout.h" // the pipeline's argument blocks, constants and pipe_geometry (no kernel templates)

#pragma GCC visibility push(hidden)

// ------------------------------------------------------------------------------ how a problem runs
int validate_problem(const mcsas_problem *p);
// what the pipeline's tuning word asks for; all zero (automatic) in the release library
struct TuneWord { int rpw = 0, sub = 0, gram_global = 0, eager = 0; };
TuneWord tune_word(const mcsas_problem *p);
// doubles of model tables a block of `waves_per_block` waves keeps in LDS: the shared table and one row scratch per wave
int table_doubles_block(int model_id, int int_div, int waves_per_block);
// How a problem runs: q slots per lane, execution mode, waves per chain, the geometry of the speculative modes and the rows of
// the intensity cache (before the spare row of alloc_rows).  A pure function of its arguments — the caller asks the device for its
// CU count and, where MCSAS_EXEC_AUTO decides, for its free memory (SIZE_MAX: not known, nothing is ruled out by it).
struct PlanShape {
    int qpl = 1, qpad = 0;
    bool wide = false;
    int waves = 1, mode = MCSAS_EXEC_WAVE, cache_rows = 0;
    mcsas::WgGeom wg{};
    mcsas::PipeGeom pipe{};
};
int decide_shape(const mcsas_problem *p, const mcsas::ModelArgs &margs, int n_cus, size_t free_bytes, const TuneWord &tw, PlanShape *s);

// ------------------------------------------------------------------------------ how a kernel family is launched and named
// threads per block of the family's kernel, `waves` being the plan's waves per chain
unsigned family_block(KernelFamily family, int waves);
// A plug-in's kernel of a family: the name expression the run-time compiler instantiates and the key of the program that holds it
// (started and cold kernels are programs of their own, each compiled when first asked for); `given` on a family without a start
// is refused.
int plugin_kernel_name(int model_id, KernelFamily family, int qpl, bool flag, bool given, std::string *expr, std::string *key);

// ------------------------------------------------------------------------------ a fetched trace block, a pipeline launch's ticks
// a slot's block as fetched (TraceLayout: [rep][capacity]) into the caller's [capacity][n_reps] arrays; what lies behind the last
// attempt's out[r].num_moves moves is an earlier attempt's or nothing: -1 / NaN
void trace_transpose(const char *block, size_t R, size_t K, size_t P, const mcsas::ChainOut *out, mcsas_trace *tr);
// The most ticks a pipeline launch enqueues: every attempt runs to max_iter (saturating: max_iter may be 2^62 and a product of two such
// numbers must not wrap to a negative budget).  One attempt: its last window (index ceil(max_iter / Kb) - 1) is scanned at tick
// ceil(max_iter / Kb), exactly; with retries the schedule depends on when attempts end: a generous bound, the host leaves when all are done.
long long pipeline_tick_budget(int64_t max_iter, int32_t max_retries, int kb);

#pragma GCC visibility pop

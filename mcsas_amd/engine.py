"""Array-level front of the HIP library: builds `mcsas_problem` blocks and runs them.

This is the thin layer the class-level mirror (`mcsas_amd.mcsas.McSAS`, `mcsas_amd.scatteringmodels`)
and the reference-side binding shown in INTEGRATION.md both sit on.  Everything numerical happens
in libmcsas_hip.so; nothing here evaluates a form factor or a chi-squared on the CPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field, replace

import numpy as np

from . import _lib
from ._lib import MAX_ACTIVE, MAX_DEVICES, MAX_PARAMS, MAX_SETS, Problem, Result, as_dp, check, f64

MODEL_SPHERE, MODEL_CYL_ISO, MODEL_ELL_CS, MODEL_KHOLODENKO = 0, 1, 2, 3
MODEL_ELL_ISO, MODEL_SPH_CS, MODEL_GAUSS_CHAIN, MODEL_LMA_SPHERE = 4, 5, 6, 7
MODEL_PLUGIN0 = 64      # first id of a run-time model plug-in (include/mcsas_hip.h: MCSAS_MODEL_PLUGIN0)
MODEL_HOST = -1         # a model that exists only as host code (Python formfactor / volume: rows through analyse_host_rows; torch calcIntensityBatch: analyse_device_rows, histogram_device_rows)


class PluginCompileError(ValueError):
    """A model plug-in's HIP source does not compile; .log holds the compiler output."""
    def __init__(self, message, log):
        super().__init__(message + "\n" + log)
        self.log = log


def release_cached_memory(tuning=False):
    """Returns the device / pinned memory parked by destroyed plans to the driver (mcsas_hip_release_cached_memory)."""
    check(_lib.load(tuning).mcsas_hip_release_cached_memory(), _lib.load(tuning))


def compile_plugin(source: str, tuning=False) -> int:
    """Registers HIP source text for a model outside the built-in ones (mcsas_hip_plugin_compile, include/mcsas_hip.h: the
    four functions mcsas_plugin_formfactor / _volume / _absvolume / _surface) and returns its model id.  Needs no GPU; the
    same text gives the same id.  This is what stands in for the reference's model discovery (utils/findmodels.py:120-186)."""
    lib = _lib.load(tuning)
    mid = C.c_int32(-1)
    rc = lib.mcsas_hip_plugin_compile(source.encode("utf-8"), C.byref(mid))
    if rc != 0:
        raise PluginCompileError(lib.mcsas_hip_last_error().decode("utf-8", "replace"),
                                 lib.mcsas_hip_plugin_log().decode("utf-8", "replace"))
    return int(mid.value)
EXEC_AUTO, EXEC_WAVE, EXEC_WORKGROUP, EXEC_PIPELINE = 0, 1, 2, 3
GEN_UNIFORM, GEN_EXP1, GEN_EXP2, GEN_EXP3 = 0, 1, 2, 3
WAVE_MAX_Q = 4096       # q-points one wavefront per chain takes (include/mcsas_hip.h: MCSAS_EXEC_WAVE)
WG_MAX_Q = 1024         # ... and the workgroup-window kernel; beyond, MCSAS_EXEC_WORKGROUP is the q-split kernel, which takes a start
INT64_MAX = (1 << 63) - 1


@dataclass
class ModelSetup:
    """A configured scattering model, flattened: full parameter vector (order of the reference's
    `parameters` tuple) plus, per active parameter, generator range/kind and clip range."""
    model_id: int
    params: np.ndarray                 # all parameter values (SI)
    active_index: tuple                # ascending indices into params
    gen_lo: np.ndarray                 # activeRange ∩ valueRange
    gen_hi: np.ndarray
    gen_kind: tuple
    clip_lo: np.ndarray                # valueRange
    clip_hi: np.ndarray
    start_value: np.ndarray = None     # startFromMinimum fill (mcsas.py:310-315)

    @property
    def n_active(self):
        return len(self.active_index)


@dataclass
class Settings:
    """The algorithm parameters of mcsas/mcsasparameters.json that reach the hot path."""
    n_contrib: int = 300
    n_reps: int = 10
    max_iter: int = 100000
    comp_exp: float = 0.6666666
    conv_crit: float = 1.0
    find_background: bool = True
    positive_background: bool = False
    start_from_minimum: bool = False
    max_retries: int = 5
    show_incomplete: bool = False
    # execution knobs (no reference counterpart)
    seed: int = 0
    rep_offset: int = 0
    device: int = -1                   # HIP device ordinal (-1: current)
    devices: tuple = ()                # several GPUs: analyse() runs contiguous blocks of repetitions on these at once
    waves_per_chain: int = 0
    cache_intensities: int = -1
    exec_mode: int = 0                 # MCSAS_EXEC_*: 0 auto, 1 wave, 2 workgroup, 3 pipeline
    debug_flags: int = 0               # tuning / ablation word: non-zero runs on the measurement build (libmcsas_hip_tuning.so)


def _fill(arr, values, n):
    for i in range(n):
        arr[i] = values[i]


class HipProblem:
    """Owns the numpy buffers a `mcsas_problem` points at (ctypes does not keep them alive)."""

    def __init__(self, model: ModelSetup, q, intensity, sigma, st: Settings, replay=None, stop=None, smear=None):
        if model.n_active < 0 or model.n_active > MAX_ACTIVE:
            raise ValueError("0..%d active parameters supported, got %d" % (MAX_ACTIVE, model.n_active))
        self.q, self.I, self.sigma = f64(q).ravel(), f64(intensity).ravel(), f64(sigma).ravel()
        if not (len(self.q) == len(self.I) == len(self.sigma)):
            raise ValueError("q, intensity and sigma must have the same length")
        self.model, self.st = model, st
        p = Problem()
        p.struct_size = C.sizeof(Problem)
        p.model_id = model.model_id
        p.nq = len(self.q)
        p.q, p.intensity, p.sigma = as_dp(self.q), as_dp(self.I), as_dp(self.sigma)
        _fill(p.params, list(model.params) + [0.0] * (MAX_PARAMS - len(model.params)), MAX_PARAMS)
        P = model.n_active
        p.n_active = P
        _fill(p.active_index, model.active_index, P)
        _fill(p.gen_lo, model.gen_lo, P); _fill(p.gen_hi, model.gen_hi, P)
        _fill(p.gen_kind, model.gen_kind, P)
        _fill(p.clip_lo, model.clip_lo, P); _fill(p.clip_hi, model.clip_hi, P)
        sv = model.start_value if model.start_value is not None else np.zeros(P)
        _fill(p.start_value, sv, P)
        p.n_contrib, p.n_reps = int(st.n_contrib), int(st.n_reps)
        p.max_iter = int(min(float(st.max_iter), float(INT64_MAX // 2)))
        p.comp_exp, p.conv_crit = float(st.comp_exp), float(st.conv_crit)
        p.max_retries = int(st.max_retries)
        p.find_background = int(bool(st.find_background))
        p.positive_background = int(bool(st.positive_background))
        p.start_from_minimum = int(bool(st.start_from_minimum))
        p.seed = int(st.seed) & 0xFFFFFFFFFFFFFFFF
        p.rep_offset = int(st.rep_offset)
        p.reserved0 = int(st.debug_flags)
        self.replay = None
        if replay is not None:
            self.replay = f64(replay).reshape(p.n_reps, -1)
            p.replay_stream = as_dp(self.replay)
            p.replay_len = self.replay.shape[1]
        self.stop = stop                      # ctypes c_int32 the caller may set to 1
        if stop is not None:
            p.stop = C.pointer(stop)
        p.device = int(st.device)
        devs = tuple(int(d) for d in (st.devices or ()))
        if len(devs) > MAX_DEVICES:
            raise ValueError("at most %d devices, got %d" % (MAX_DEVICES, len(devs)))
        p.n_devices = len(devs)
        _fill(p.devices, devs, len(devs))
        p.waves_per_chain = int(st.waves_per_chain)
        p.cache_intensities = int(st.cache_intensities)
        p.exec_mode = int(st.exec_mode)
        # beam-profile smearing: `smear` carries what SASConfig.prepareSmearing produced (locs[Q][K],
        # q_offset[K], weights[K]; dataobj.Smearing or anything with those attributes), or None
        self.smear = None
        if smear is not None and getattr(smear, "q_offset", None) is not None:
            locs = f64(smear.locs)
            if locs.ndim != 2 or locs.shape[0] != p.nq:
                raise ValueError("smear.locs must be (nq, K), got %r" % (locs.shape,))
            self.smear = (locs, f64(smear.q_offset).ravel(), f64(smear.weights).ravel())
            if not (locs.shape[1] == len(self.smear[1]) == len(self.smear[2])):
                raise ValueError("smear: locs, q_offset and weights disagree on K")
            p.smear_nk = locs.shape[1]
            p.smear_locs, p.smear_q_offset, p.smear_weights = (as_dp(a) for a in self.smear)
        self.c = p


class ChainResults:
    """numpy-backed `mcsas_result`."""

    def __init__(self, n_contrib, n_active, n_reps, nq):
        self.contribs = np.zeros((n_contrib, n_active, n_reps))
        self.fit = np.zeros((nq, n_reps))
        self.chisq = np.zeros(n_reps); self.scaling = np.zeros(n_reps); self.background = np.zeros(n_reps)
        self.num_iter = np.zeros(n_reps, dtype=np.int64); self.num_moves = np.zeros(n_reps, dtype=np.int64)
        self.attempts = np.zeros(n_reps, dtype=np.int32); self.converged = np.zeros(n_reps, dtype=np.int32)
        self.seconds = np.zeros(n_reps); self.draws = np.zeros(n_reps, dtype=np.int64)
        r = Result()
        r.struct_size = C.sizeof(Result)
        r.contribs, r.fit = as_dp(self.contribs), as_dp(self.fit)
        r.chisq, r.scaling, r.background = as_dp(self.chisq), as_dp(self.scaling), as_dp(self.background)
        r.num_iter = self.num_iter.ctypes.data_as(C.POINTER(C.c_int64))
        r.num_moves = self.num_moves.ctypes.data_as(C.POINTER(C.c_int64))
        r.attempts = self.attempts.ctypes.data_as(C.POINTER(C.c_int32))
        r.converged = self.converged.ctypes.data_as(C.POINTER(C.c_int32))
        r.seconds = as_dp(self.seconds)
        r.draws = self.draws.ctypes.data_as(C.POINTER(C.c_int64))
        self.c = r
        self.trace = None                 # a ChainTrace where the analysis was asked for one (analyse(trace=K), Plan.set_trace)


class ChainTrace:
    """numpy-backed `mcsas_trace`: per repetition the accepted moves of its last attempt (what the reference logs as "good iter",
    mcsas.py:385-390).  count[R] = all moves made (== num_moves), chisq0[R] = reduced chi-squared of the attempt's initial set;
    the first min(count, capacity) moves: step[K][R] (numIter of the move; contribution = step % n_contrib), chisq[K][R] (conval
    after it), values[K][P][R] (the accepted set); entries behind them are -1 / NaN."""

    def __init__(self, capacity, n_active, n_reps):
        self.capacity = int(capacity)
        self.count = np.zeros(n_reps, dtype=np.int64); self.chisq0 = np.full(n_reps, np.nan)
        self.step = np.full((self.capacity, n_reps), -1, dtype=np.int64)
        self.chisq = np.full((self.capacity, n_reps), np.nan)
        self.values = np.full((self.capacity, n_active, n_reps), np.nan)
        t = _lib.Trace()
        t.struct_size = C.sizeof(_lib.Trace)
        t.capacity = self.capacity
        t.count = self.count.ctypes.data_as(C.POINTER(C.c_int64)); t.chisq0 = as_dp(self.chisq0)
        t.step = self.step.ctypes.data_as(C.POINTER(C.c_int64)); t.chisq = as_dp(self.chisq); t.values = as_dp(self.values)
        self.c = t

    def asdict(self):
        return dict(count=self.count, chisq0=self.chisq0, step=self.step, chisq=self.chisq, values=self.values)


def kernel_mode(what, exec_mode, nq, who, auto_beyond_wave=False, mode_word="exec_mode", q_word="q-points"):
    """The execution mode the library is asked for (EXEC_WAVE or EXEC_WORKGROUP) where an analysis of `nq` q-points under `exec_mode`
    comes with a given start or a trace, or goes into a batch (`what`: "start", "trace", "batch"); ValueError where no kernel takes it.
    This is the one place that says so in Python (the library: csrc/host_internal.h):
    - EXEC_AUTO and EXEC_WAVE run one wavefront per chain, which takes up to WAVE_MAX_Q q-points;
    - EXEC_WORKGROUP with more than WG_MAX_Q q-points runs the q-split kernel (up to 16384 q-points: the library's refusal), except
      in a batch, which is one wavefront per chain throughout;
    - the workgroup-window kernel (EXEC_WORKGROUP up to WG_MAX_Q q-points) and the pipeline take neither a start nor a trace.
    Beyond WAVE_MAX_Q q-points without the q-split kernel the callers differ:
    - a trace and a batch raise: neither ever picks the mode;
    - a start returns EXEC_WAVE and leaves the refusal to the library (engine.analyse, analyse_many, and McSAS with execMode wave);
    - a start with `auto_beyond_wave` (McSAS) returns EXEC_WORKGROUP where EXEC_AUTO left the choice open: no other kernel takes the data.
    `who`, `mode_word` (exec_mode / execMode) and `q_word` (q-points / points) are the caller's wording of the messages."""
    q_split = what != "batch" and exec_mode == EXEC_WORKGROUP and nq > WG_MAX_Q
    if exec_mode not in (EXEC_AUTO, EXEC_WAVE) and not q_split:
        if what == "batch":
            raise ValueError("%s asks for %s %d; a batch runs one wavefront per chain" % (who, mode_word, exec_mode))
        raise ValueError("%s: a %s runs one wavefront per chain, or a workgroup per chain with more than %d %s; "
                         "%s %d was asked with %d %s (0 or 1, or 2 beyond %d %s)"
                         % (who, what, WG_MAX_Q, q_word, mode_word, exec_mode, nq, q_word, WG_MAX_Q, q_word))
    if nq > WAVE_MAX_Q and not q_split:
        if what == "batch":
            raise ValueError("%s has %d %s; one wavefront per chain takes up to %d" % (who, nq, q_word, WAVE_MAX_Q))
        if what == "trace":
            raise ValueError("%s: %d %s; with %s %d a trace runs one wavefront per chain, which takes up to %d: "
                             "set %s to workgroup (%d)" % (who, nq, q_word, mode_word, exec_mode, WAVE_MAX_Q, mode_word, EXEC_WORKGROUP))
        if auto_beyond_wave and exec_mode == EXEC_AUTO:
            return EXEC_WORKGROUP
    return EXEC_WORKGROUP if q_split else EXEC_WAVE


def _check_trace(trace, model: ModelSetup, st: Settings, nq, who="analyse"):
    """The capacity of a trace as an int; ValueError where no traced kernel exists for the analysis (kernel_mode: the trace never
    picks the mode), for a model that exists only as host code and for a device list — before any library call."""
    k = int(trace)
    if k < 1:
        raise ValueError("%s: trace is the number of moves kept per repetition (>= 1), got %r" % (who, trace))
    if model.model_id == MODEL_HOST:
        raise ValueError("%s: a model that exists only as host code keeps no trace (a trace runs one wavefront per chain)" % who)
    kernel_mode("trace", st.exec_mode, nq, who)
    if st.devices:
        raise ValueError("%s: a trace is kept on one device; a device list %r was given" % (who, tuple(st.devices)))
    return k


def _check_start(start, model: ModelSetup, st: Settings, who="analyse"):
    """The start set of an analysis as a contiguous [n_contrib][n_active][R >= n_reps] array (the layout of ChainResults.contribs);
    ValueError for a wrong shape or a model that exists only as host code — before any library call."""
    if model.model_id == MODEL_HOST:
        raise ValueError("%s: a model that exists only as host code takes no start (a start runs one wavefront per chain)" % who)
    a = f64(start)
    if a.ndim != 3 or a.shape[0] != int(st.n_contrib) or a.shape[1] != model.n_active:
        raise ValueError("%s: start must be (n_contrib, n_active, n_reps) = (%d, %d, >= %d), got %r"
                         % (who, st.n_contrib, model.n_active, st.n_reps, a.shape))
    return a


def _start_columns(a, st: Settings, rep_first, who="analyse"):
    if rep_first < 0 or rep_first + int(st.n_reps) > a.shape[2]:
        raise ValueError("%s: start has %d repetitions, %d..%d asked" % (who, a.shape[2], rep_first, rep_first + int(st.n_reps) - 1))


def analyse(model: ModelSetup, q, intensity, sigma, st: Settings, replay=None, stop=None, smear=None, start=None, trace=None) -> ChainResults:
    """All repetitions of McSAS.analyse (mcsas.py:214-262) in one kernel launch.  `start`: [n_contrib][n_active][n_reps] (a
    ChainResults.contribs; further repetitions are ignored), the set the first attempt of every repetition starts from instead of
    a random one (mcsas_hip_analyse_from, include/mcsas_hip.h) — one wavefront per chain, or with exec_mode 2 and more than
    WG_MAX_Q q-points the q-split workgroup kernel (the only one beyond WAVE_MAX_Q); exec_mode 2 below that and 3 are refused.
    `trace`: K >= 1 keeps the first K accepted moves of every repetition's last attempt in the result's .trace (a ChainTrace;
    mcsas_hip_analyse_traced): one wavefront per chain, or the q-split workgroup kernel under the same condition as for a start,
    cold or from a start; every other array is what it is without a trace."""
    if trace is not None:
        trace = _check_trace(trace, model, st, int(np.size(q)))
    if start is not None and model.n_active > 0:
        a = _check_start(start, model, st)
        _start_columns(a, st, 0)
        if a.shape[2] != int(st.n_reps):
            a = f64(a[:, :, :int(st.n_reps)])
    lib = _lib.load(tuning=bool(st.debug_flags))
    prob = HipProblem(model, q, intensity, sigma, st, replay, stop, smear)
    res = ChainResults(st.n_contrib, model.n_active, st.n_reps, len(prob.q))
    if trace is not None:
        res.trace = ChainTrace(trace, model.n_active, st.n_reps)
        given = as_dp(a) if start is not None and model.n_active > 0 else None
        check(lib.mcsas_hip_analyse_traced(C.byref(prob.c), given, C.byref(res.c), C.byref(res.trace.c)), lib)
    elif start is not None and model.n_active > 0:
        check(lib.mcsas_hip_analyse_from(C.byref(prob.c), as_dp(a), C.byref(res.c)), lib)
    else:
        check(lib.mcsas_hip_analyse(C.byref(prob.c), C.byref(res.c)), lib)
    return res


class SetsResults(ChainResults):
    """A joint fit of several data sets (analyse_sets): ChainResults over the concatenated points — `fit` holds every point with its
    own set's scale and background, `chisq` the reduced chi-squared over all points, `scaling` / `background` set 0's — plus, per set,
    set_scaling[S][R], set_background[S][R], set_chisq[S][R] (the sum over the set / its number of points) and `slices`, where each
    set lies among the points."""

    def __init__(self, n_contrib, n_active, n_reps, set_nq):
        super().__init__(n_contrib, n_active, n_reps, int(sum(set_nq)))
        S = len(set_nq)
        self.set_nq = np.ascontiguousarray(set_nq, dtype=np.int32)
        edges = np.concatenate([[0], np.cumsum(self.set_nq)])
        self.slices = [slice(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]
        self.set_scaling = np.zeros((S, n_reps)); self.set_background = np.zeros((S, n_reps)); self.set_chisq = np.zeros((S, n_reps))
        s = _lib.SetsResult()
        s.struct_size = C.sizeof(_lib.SetsResult)
        s.n_sets = S
        s.scaling, s.background, s.chisq = as_dp(self.set_scaling), as_dp(self.set_background), as_dp(self.set_chisq)
        self.sets_c = s


def _sets_scale_mode(scale, who):
    if not isinstance(scale, str) or scale not in _lib.SETS_SCALE:
        raise ValueError("%s: scale %r ('per_set': a scale per set, 'shared': one scale for all sets)" % (who, scale))
    return _lib.SETS_SCALE[scale]


def _sets_triples(sets, who):
    triples = [tuple(f64(v).ravel() for v in trip) for trip in sets]
    if any(len(trip) != 3 for trip in triples):
        raise ValueError("%s: sets is a list of (q, I, sigma)" % who)
    for s, (q, i, e) in enumerate(triples):
        if not (len(q) == len(i) == len(e)):
            raise ValueError("%s: set %d: q, intensity and sigma must have the same length" % (who, s))
    cat = [np.concatenate([trip[k] for trip in triples]) if triples else np.zeros(0) for k in range(3)]
    return triples, cat


def analyse_sets(model: ModelSetup, sets, st: Settings, replay=None, stop=None, scale="per_set") -> SetsResults:
    """One population fitted to several data sets at once (mcsas_hip_analyse_sets_mode, include/mcsas_hip.h): `sets` is a list of 1 to
    MAX_SETS triples (q, I, sigma) of at least 3 points each — measurements of the same specimen whose backgrounds are not known.
    `scale`: "per_set" (curves whose relative scale is not known: every set gets its own least-squares scale and background at every
    step) or "shared" (curves on an absolute scale: ONE least-squares scale for all sets, a background per set; set_scaling then
    holds the same number for every set).  Every chain holds one set of contributions and is judged by all sets, and the chain
    minimises the reduced chi-squared over all points.  One wavefront per chain,
    cached rows; together the sets, each padded to a multiple of 64 points, take at most 1024 entries.  Refused (ValueError here or
    MCSAS_EINVAL from the library, before a device is touched): positive_background, a device list, a model plug-in or a model that
    exists only as host code, no active parameter, cache_intensities == 0, an exec_mode other than EXEC_AUTO / EXEC_WAVE; there is
    no plan, batch, start, trace or smearing form."""
    mode = _sets_scale_mode(scale, "analyse_sets")
    triples, cat = _sets_triples(sets, "analyse_sets")
    if model.model_id == MODEL_HOST:
        raise ValueError("analyse_sets: a model that exists only as host code is not supported (built-in models only)")
    if model.model_id >= MODEL_PLUGIN0:
        raise ValueError("analyse_sets: a model plug-in is not supported (built-in models only)")
    if st.devices:
        raise ValueError("analyse_sets: a device list %r was given; the joint fit runs on one device" % (tuple(st.devices),))
    if st.debug_flags:
        raise ValueError("analyse_sets: debug_flags select variants of the pipeline mode; the joint fit has none")
    lib = _lib.load()
    prob = HipProblem(model, cat[0], cat[1], cat[2], st, replay, stop, None)
    res = SetsResults(st.n_contrib, model.n_active, st.n_reps, [len(trip[0]) for trip in triples])
    check(lib.mcsas_hip_analyse_sets_mode(C.byref(prob.c), len(triples), res.set_nq.ctypes.data_as(C.POINTER(C.c_int32)), mode,
                                          C.byref(res.c), C.byref(res.sets_c)), lib)
    return res


def analyse_host_rows(model: ModelSetup, q, intensity, sigma, st: Settings, row_fn, replay=None, stop=None, window=64) -> ChainResults:
    """McSAS.analyse for a model that exists only as host code (mcsas_hip_analyse_host_rows, include/mcsas_hip.h): the library draws
    the proposals of the next `window` steps of every chain, `row_fn(pset[n][n_active]) -> rows[n][nq]` evaluates the caller's own
    calcIntensity for all of them (bases/model/scatteringmodel.py:90-99, sasmodel.py:46-79), the device does the rest of mcFit."""
    lib = _lib.load()
    prob = HipProblem(model, q, intensity, sigma, st, replay, stop, None)
    prob.c.model_id = MODEL_HOST
    nq, P = len(prob.q), model.n_active
    res = ChainResults(st.n_contrib, P, st.n_reps, nq)

    def fill(n, pset_p, rows_p):
        pset = np.ctypeslib.as_array(pset_p, shape=(n, P))
        out = np.ctypeslib.as_array(rows_p, shape=(n, nq))
        out[:, :] = np.asarray(row_fn(pset), dtype=np.float64).reshape(n, nq)

    cb, failure = _rows_callback(_lib.RowsCallback, fill)
    rc = lib.mcsas_hip_analyse_host_rows(C.byref(prob.c), cb, None, int(window), C.byref(res.c))
    if failure:
        raise failure[0]
    check(rc, lib)
    return res


def _rows_callback(ctype, fill):
    """(callback, failure): `fill(n, ...)`, a rows callback's arguments after `user`, wrapped for ctypes.  An exception must not
    cross the C frame: the callback hands it over in `failure` and returns 1, and the caller re-raises failure[0] after the call."""
    failure = []

    def cb(user, *args):
        try:
            fill(*args)
            return 0
        except BaseException as e:
            failure.append(e)
            return 1
    return ctype(cb), failure


def device_rows_shape(model: ModelSetup, q, st: Settings, window=64):
    """(min_rows, useful_rows, row_stride) of analyse_device_rows for this problem (mcsas_hip_device_rows_shape; no device is touched):
    the least and the most rows of a round, and the row pitch of the rows buffer (the q count rounded up to 64)."""
    q = f64(q).ravel()
    prob = HipProblem(model, q, np.ones_like(q), np.ones_like(q), st)
    return _shape_triple(_lib.load().mcsas_hip_device_rows_shape, prob, int(window))


def _shape_triple(query, prob, *args):
    """(min_rows, useful_rows, row_stride) as a shape query of the library answers for `prob`"""
    lo, hi, stride = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    check(query(C.byref(prob.c), *args, C.byref(lo), C.byref(hi), C.byref(stride)))
    return lo.value, hi.value, stride.value


def _device_rows_tensors(who, shape, capacity, takes, device, n_active, vws=False):
    """The torch side of a device-rows call: `capacity` (default: the most a round uses) checked against the shape query's answer,
    then (capacity, device, pset[capacity][n_active], rows[capacity][stride], and with `vws` a third tensor [3][capacity]) on
    `device` (< 0: torch's current one), complete before the library — which works on the null stream of its own — sees them."""
    import torch
    min_rows, useful_rows, stride = shape
    capacity = int(useful_rows if capacity is None else capacity)
    if capacity < min_rows:
        raise ValueError("%s: capacity %d < %d rows, what %s" % (who, capacity, min_rows, takes))
    _one_hip_runtime()
    dev = torch.device("cuda", torch.cuda.current_device() if int(device) < 0 else int(device))
    sizes = [(capacity, n_active), (capacity, stride)] + ([(3, capacity)] if vws else [])
    tensors = [torch.empty(s, dtype=torch.float64, device=dev) for s in sizes]
    torch.cuda.synchronize(dev)
    return (capacity, dev, *tensors)


def _one_hip_runtime():
    """A torch wheel brings a HIP runtime of its own.  Loaded after torch, libmcsas_hip.so binds to that one (same soname) and a
    tensor is device memory to both; loaded before torch, it has bound to the system's runtime, the process holds two, and memory
    of the one is unknown to the other.  RuntimeError then, instead of an analysis on buffers the library cannot see."""
    try:
        with open("/proc/self/maps") as f:
            paths = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    except OSError:
        return
    if len(paths) > 1:
        raise RuntimeError("analyse_device_rows: this process holds two HIP runtimes (%s): the library was loaded before torch. "
                           "Import torch before the first call into mcsas_amd" % ", ".join(sorted(paths)))


def analyse_device_rows(model: ModelSetup, q, intensity, sigma, st: Settings, row_fn, replay=None, stop=None, window=64,
                        capacity=None) -> ChainResults:
    """McSAS.analyse for a model whose rows the caller computes ON THE DEVICE with torch (mcsas_hip_analyse_device_rows,
    include/mcsas_hip.h): the library generates the proposals of a round into a torch tensor, `row_fn(pset[n][n_active],
    rows[n][nq])` fills the rows view in place, or returns a tensor [n][nq] that is copied into it, and the device does the rest
    of mcFit on the rows where they lie.  pset is not yet clipped.  `capacity`: rows of the two tensors (default: the most a round
    uses, device_rows_shape).  torch is imported here, not with the package."""
    import torch                                 # (ahead of the library's first load: see _one_hip_runtime)
    lib = _lib.load()
    _one_hip_runtime()                           # (this call's first refusal; _device_rows_tensors asks again, to no effect)
    prob = HipProblem(model, q, intensity, sigma, st, replay, stop, None)
    prob.c.model_id = MODEL_HOST
    nq, P = len(prob.q), model.n_active
    capacity, device, pset, rows = _device_rows_tensors(
        "analyse_device_rows", _shape_triple(lib.mcsas_hip_device_rows_shape, prob, int(window)), capacity,
        "one chain's round takes (max(n_contrib, window))", st.device, P)
    res = ChainResults(st.n_contrib, P, st.n_reps, nq)

    def fill(n):
        with torch.cuda.device(device):
            view = rows[:n, :nq]
            out = row_fn(pset[:n], view)
            if out is not None and out is not view:
                view.copy_(torch.as_tensor(out, dtype=torch.float64, device=device).reshape(n, nq))
            torch.cuda.current_stream(device).synchronize()

    cb, failure = _rows_callback(_lib.DeviceRowsCallback, fill)
    rc = lib.mcsas_hip_analyse_device_rows(C.byref(prob.c), C.c_void_p(pset.data_ptr()), C.c_void_p(rows.data_ptr()), capacity,
                                           cb, None, int(window), C.byref(res.c))
    if failure:
        raise failure[0]
    check(rc, lib)
    return res


def _as_problem(p):
    """A problem of analyse_many / analyse_batch as a dict: given as one, or as (model, q, intensity, sigma, settings)"""
    return p if isinstance(p, dict) else dict(model=p[0], q=p[1], intensity=p[2], sigma=p[3], st=p[4])


def _analyse_problem(pr):
    """analyse() of such a dict, for what runs at its place in the sequence instead of with the others"""
    return analyse(pr["model"], pr["q"], pr["intensity"], pr["sigma"], pr["st"], pr.get("replay"), pr.get("stop"), pr.get("smear"),
                   start=pr.get("start"))


def analyse_many(problems, streams=2):
    """Independent analyses — a series of data sets (gui/calc.py:271-330 runs them one after the other) — side by side: every
    problem gets a plan of its own (creation is cheap: the library keeps destroyed plans' memory), the plans go round `streams`
    HIP streams, two per stream in flight, so the chip always has one analysis' scan-bound ticks beside another's producer-bound
    ones.  `problems`: sequence of (model: ModelSetup, q, intensity, sigma, settings) or of dicts with those keys
    plus optional replay / stop / smear.  Returns the ChainResults in order — each identical to analyse() of that problem."""
    problems = [_as_problem(p) for p in problems]
    if not problems:
        return []
    lib = _lib.load(tuning=bool(problems[0]["st"].debug_flags))
    per_dev = {}                                              # device ordinal -> the stream handles created on THAT device

    def stream_for(dev, k):
        hs = per_dev.setdefault(dev, [])
        if len(hs) < max(1, streams):
            h = C.c_void_p()
            check(lib.mcsas_hip_stream_create(C.c_int32(dev), C.byref(h)), lib)
            hs.append(h)
        return hs[k % len(hs)]

    out, pending, launched = [None] * len(problems), [], {}
    try:
        for i, pr in enumerate(problems):
            st = pr["st"]
            # what a plan cannot do goes through mcsas_hip_analyse at its place in the sequence: a model with no active parameter
            # (one contribution, nothing to fit: mcsas.py:198-199) and a device list (the library shards the repetitions itself)
            if pr["model"].n_active == 0 or st.devices:
                out[i] = _analyse_problem(pr)
                continue
            cap = 2 * max(1, streams)
            while len(pending) >= cap:
                j, pl = pending.pop(0)
                out[j] = pl.fetch(); pl.close()
            if pr.get("start") is not None:                  # (a start runs one wavefront per chain or the q-split kernel: kernel_mode)
                try:
                    st = replace(st, exec_mode=kernel_mode("start", st.exec_mode, np.size(pr["q"]), "analyse_many"))
                except ValueError:
                    raise ValueError("analyse_many: problem %d asks for exec_mode %d with a start and %d q-points (0 or 1, or 2 with more than %d q-points)"
                                     % (i, st.exec_mode, np.size(pr["q"]), WG_MAX_Q)) from None
            pl = Plan(pr["model"], pr["q"], pr["intensity"], pr["sigma"], st, pr.get("replay"), pr.get("stop"), pr.get("smear"))
            if pr.get("start") is not None:
                try:
                    pl.set_start(pr["start"])
                except Exception:
                    pl.close()
                    raise
            k = launched.get(st.device, 0); launched[st.device] = k + 1
            pl.launch(stream=stream_for(st.device, k).value)
            pending.append((i, pl))
        while pending:
            j, pl = pending.pop(0)
            out[j] = pl.fetch(); pl.close()
    finally:
        for _, pl in pending:
            pl.close()
        for hs in per_dev.values():
            for h in hs:
                lib.mcsas_hip_stream_destroy(h)
    return out


def analyse_batch(problems):
    """Independent analyses — a series of data sets — in ONE wavefront-per-chain launch per kernel (mcsas_hip_analyse_batch,
    include/mcsas_hip.h): every repetition of every data set is one chain of the same launch, so a series of a few repetitions per
    data set fills the chip.  `problems` as for analyse_many.  Returns the ChainResults in order; each is identical to analyse() of
    that problem with exec_mode = EXEC_WAVE (seconds aside), whatever else is in the batch.  Device lists and models without an
    active parameter run through analyse() at their place; a model that exists only as host code (MODEL_HOST) or a data set of
    more than WAVE_MAX_Q q-points raises ValueError before anything is launched.  A problem may carry a "start" key (see analyse);
    a batch with one runs through resident plans (Plan.set_start, launch_batch, fetch), the problems without a start included, and
    each result is then identical to analyse(..., start=...) of that problem."""
    problems = [_as_problem(p) for p in problems]
    starts = {}
    for i, pr in enumerate(problems):
        if pr.get("start") is not None and pr["model"].n_active > 0:
            starts[i] = _check_start(pr["start"], pr["model"], pr["st"], "analyse_batch: problem %d" % i)
            _start_columns(starts[i], pr["st"], 0, "analyse_batch: problem %d" % i)
    for i, pr in enumerate(problems):
        if pr["model"].model_id == MODEL_HOST:
            raise ValueError("analyse_batch: problem %d: a model that exists only as host code has no device kernel to batch" % i)
        kernel_mode("batch", EXEC_WAVE, np.size(pr["q"]), "analyse_batch: problem %d" % i)   # (the size; the mode a problem asks for: below)
    if not problems:
        return []
    out, batched = [None] * len(problems), []
    for i, pr in enumerate(problems):
        if not (pr["model"].n_active == 0 or pr["st"].devices):
            batched.append(i)
    if batched and any(i in starts for i in batched):
        plans = []
        try:
            for i in batched:
                pr = problems[i]
                st = replace(pr["st"], exec_mode=kernel_mode("batch", pr["st"].exec_mode, np.size(pr["q"]), "analyse_batch: problem %d" % i))
                plans.append(Plan(pr["model"], pr["q"], pr["intensity"], pr["sigma"], st, pr.get("replay"), pr.get("stop"), pr.get("smear")))
                if i in starts:
                    plans[-1].set_start(starts[i])
            launch_batch(plans)
            failure = None
            for i, pl in zip(batched, plans):                # (every plan is fetched, so that none is destroyed in flight)
                try:
                    out[i] = pl.fetch()
                except _lib.McSASHipError as e:
                    failure = failure or e
            if failure is not None:
                raise failure
        finally:
            for pl in plans:
                pl.close()
    elif batched:
        lib = _lib.load(tuning=bool(problems[batched[0]]["st"].debug_flags))
        probs, results = [], []
        for i in batched:
            pr = problems[i]
            probs.append(HipProblem(pr["model"], pr["q"], pr["intensity"], pr["sigma"], pr["st"], pr.get("replay"), pr.get("stop"),
                                    pr.get("smear")))
            results.append(ChainResults(pr["st"].n_contrib, pr["model"].n_active, pr["st"].n_reps, len(probs[-1].q)))
        parr = (Problem * len(probs))(*[p.c for p in probs])
        rarr = (Result * len(results))(*[r.c for r in results])
        check(lib.mcsas_hip_analyse_batch(parr, len(probs), rarr), lib)
        for i, r in zip(batched, results):
            out[i] = r
    for i, pr in enumerate(problems):
        if out[i] is None:
            out[i] = _analyse_problem(pr)
    return out


def launch_batch(plans, stream=None):
    """Enqueues resident wavefront-per-chain plans together (mcsas_hip_plan_launch_batch): one launch per group of plans with the
    same kernel, every plan's slot 0.  Fetch each plan afterwards (Plan.fetch).  All plans on one device, one stop word or none."""
    plans = list(plans)
    if not plans:
        raise ValueError("launch_batch: no plans")
    lib = plans[0].lib
    hs = (C.c_void_p * len(plans))(*[p.h.value for p in plans])
    check(lib.mcsas_hip_plan_launch_batch(hs, len(plans), C.c_void_p(stream or 0)), lib)


class Plan:
    """Resident plan: data and workspaces stay in HBM; launch/fetch can be repeated (bench.py)."""

    def __init__(self, model: ModelSetup, q, intensity, sigma, st: Settings, replay=None, stop=None, smear=None):
        self.lib = _lib.load(tuning=bool(st.debug_flags))
        self.prob = HipProblem(model, q, intensity, sigma, st, replay, stop, smear)
        self.h = C.c_void_p()
        check(self.lib.mcsas_hip_plan_create(C.byref(self.prob.c), C.byref(self.h)), self.lib)
        self.trace_capacity = 0

    def launch(self, stream=None, slot=0):
        """Enqueues one analysis.  `slot`: which of the plan's result sets (mcsas_hip.h: MCSAS_PLAN_SLOTS) it writes — launch
        into slot 1 while slot 0 is fetched and the device never waits for the host (same stream: the slots share the workspaces)."""
        check(self.lib.mcsas_hip_plan_launch_slot(self.h, C.c_void_p(stream or 0), C.c_int32(slot)), self.lib)

    def fetch(self, want_arrays=True, slot=0):
        st = self.prob.st
        res = ChainResults(st.n_contrib, self.prob.model.n_active, st.n_reps, len(self.prob.q)) if want_arrays else None
        check(self.lib.mcsas_hip_plan_fetch_slot(self.h, C.c_int32(slot), C.byref(res.c) if res is not None else None), self.lib)
        if res is not None and self.trace_capacity:
            res.trace = self.fetch_trace(slot)
        return res

    def set_trace(self, capacity):
        """Every later launch of this plan keeps the first `capacity` accepted moves of every repetition's last attempt, per slot
        (mcsas_hip_plan_set_trace); fetch() then fills ChainResults.trace.  0 or None clears it.  Plans in the wavefront mode and
        in the workgroup mode with more than WG_MAX_Q q-points (the q-split kernel); the others refuse, and so does launch_batch for a plan with a trace."""
        k = int(capacity or 0)
        check(self.lib.mcsas_hip_plan_set_trace(self.h, C.c_int32(k)), self.lib)
        self.trace_capacity = k

    def fetch_trace(self, slot=0, capacity=None):
        """The trace of the slot's last launch (mcsas_hip_plan_fetch_trace), after its fetch()."""
        tr = ChainTrace(self.trace_capacity if capacity is None else capacity, self.prob.model.n_active, self.prob.st.n_reps)
        check(self.lib.mcsas_hip_plan_fetch_trace(self.h, C.c_int32(slot), C.byref(tr.c)), self.lib)
        return tr

    def set_start(self, contribs, rep_first=0):
        """Every later launch of this plan (launch_batch included) starts repetition r from contribs[:, :, rep_first + r]
        ([n_contrib][n_active][R], e.g. a fetched ChainResults.contribs) instead of a random set, for its first attempt
        (mcsas_hip_plan_set_start).  The plan keeps a copy.  None clears it.  Plans in the wavefront mode, and workgroup plans of more
        than WG_MAX_Q q-points (the q-split kernel); the others refuse."""
        if contribs is None:
            check(self.lib.mcsas_hip_plan_set_start(self.h, None, 0, 0), self.lib)
            return
        a = _check_start(contribs, self.prob.model, self.prob.st, "Plan.set_start")
        _start_columns(a, self.prob.st, int(rep_first), "Plan.set_start")
        check(self.lib.mcsas_hip_plan_set_start(self.h, as_dp(a), C.c_int32(a.shape[2]), C.c_int32(int(rep_first))), self.lib)

    def reseed(self, seed, rep_offset=0):
        check(self.lib.mcsas_hip_plan_reseed(self.h, C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), C.c_int32(rep_offset)), self.lib)

    @property
    def info(self):
        """dict: exec mode the library chose, waves per chain, q slots per lane, window, launches, cache."""
        v = (C.c_int32 * 8)()
        check(self.lib.mcsas_hip_plan_info(self.h, v), self.lib)
        names = {1: "wave", 2: "workgroup", 3: "pipeline"}
        return dict(exec_mode=names.get(v[0], str(v[0])), waves_per_chain=v[1], q_per_lane=v[2], window=v[3],
                    launches=v[4], cached_rows=bool(v[5]))

    @property
    def last_ms(self):
        v = C.c_double()
        check(self.lib.mcsas_hip_plan_last_ms(self.h, C.byref(v)), self.lib)
        return v.value

    @property
    def total_steps(self):
        v = C.c_int64()
        check(self.lib.mcsas_hip_plan_total_steps(self.h, C.byref(v)), self.lib)
        return v.value

    def close(self):
        if self.h:
            self.lib.mcsas_hip_plan_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def model_calc(model: ModelSetup, q, pset, comp_exp, want_rows=False, device=-1, smear=None):
    """ScatteringModel.calc(data, pset, compensationExponent) (scatteringmodel.py:79-109) on the GPU.
    Returns cumInt, vset, wset, sset (and rows[n][Q] when asked)."""
    lib = _lib.load()
    q = f64(q).ravel()
    pset = f64(pset).reshape(-1, model.n_active)
    st = Settings(n_contrib=1, n_reps=1, comp_exp=comp_exp, device=device)
    prob = HipProblem(model, q, np.ones_like(q), np.ones_like(q), st, smear=smear)
    n = len(pset)
    cum = np.zeros(len(q)); vset = np.zeros(n); wset = np.zeros(n); sset = np.zeros(n)
    rows = np.zeros((n, len(q))) if want_rows else None
    check(lib.mcsas_hip_model_calc(C.byref(prob.c), as_dp(pset), n, as_dp(cum), as_dp(vset), as_dp(wset),
                                   as_dp(sset), as_dp(rows) if rows is not None else None))
    return (cum, vset, wset, sset, rows) if want_rows else (cum, vset, wset, sset)


def bgfit(intensity, sigma, model_int, find_background=True, positive_background=False, num_params=1, device=-1):
    """BackgroundScalingFit.calc (backgroundscalingfit.py:112-139): returns (sc[2], conval, aGoFs)."""
    lib = _lib.load()
    I, s, c = f64(intensity).ravel(), f64(sigma).ravel(), f64(model_int).ravel()
    out = np.zeros(4)
    check(lib.mcsas_hip_bgfit(len(I), as_dp(I), as_dp(s), as_dp(c), int(find_background), int(positive_background),
                              int(num_params), int(device), as_dp(out)))
    return out[:2].copy(), float(out[2]), float(out[3])


def observability(model: ModelSetup, q, sigma, contribs, scaling, vol_frac, comp_exp, device=-1, smear=None):
    """Per-contribution minimum visible volume fraction (mcsas.py:575-590) for all reps."""
    lib = _lib.load()
    contribs = f64(contribs)
    N, P, R = contribs.shape
    q = f64(q).ravel(); sigma = f64(sigma).ravel()
    st = Settings(n_contrib=N, n_reps=R, comp_exp=comp_exp, device=device)
    prob = HipProblem(model, q, np.ones_like(q), sigma, st, smear=smear)
    scaling = f64(scaling).ravel(); vol_frac = f64(vol_frac).reshape(N, R)
    out = np.zeros((N, R))
    check(lib.mcsas_hip_observability(C.byref(prob.c), as_dp(contribs), as_dp(scaling), as_dp(vol_frac), as_dp(out)))
    return out


def histogram_prep(model: ModelSetup, q, intensity, sigma, contribs, comp_exp, find_background=True,
                   positive_background=False, device=-1, smear=None):
    """First half of McSAS.histogram() (mcsas.py:549-594) for all repetitions in one call: returns
    scaling[2][R] (scale, background per rep), vset, wset, sset and the visibility limits, each [N][R]."""
    lib = _lib.load()
    contribs = f64(contribs)
    N, P, R = contribs.shape
    st = Settings(n_contrib=N, n_reps=R, comp_exp=comp_exp, device=device, find_background=find_background,
                  positive_background=positive_background)
    prob = HipProblem(model, q, intensity, sigma, st, smear=smear)
    sc = np.zeros((2, R)); v = np.zeros((N, R)); w = np.zeros((N, R)); s = np.zeros((N, R)); mv = np.zeros((N, R))
    check(lib.mcsas_hip_histogram_prep(C.byref(prob.c), as_dp(contribs), as_dp(sc), as_dp(v), as_dp(w), as_dp(s), as_dp(mv)))
    return sc, v, w, s, mv


HISTOGRAM_MAX_CONTRIBS = 4096     # mcsas_hip_histogram stages a repetition's contributions in LDS
YWEIGHT_INDEX = {"vol": 0, "num": 1, "int": 2, "surf": 3}


HISTOGRAM_PARTIAL_MAX_BINS = 256  # bin curves keep a bin's 64 running sums in LDS (csrc/hist_partial_kernel.h)
PARTIAL_WANT = {None: 0, False: 0, 0: 0, 1: 1, 2: 2, "range": 1, "bins": 2}


def histogram_device(model: ModelSetup, q, intensity, sigma, contribs, comp_exp, specs, find_background=True,
                     positive_background=False, device=-1, smear=None, partial=None):
    """McSAS.histogram() (mcsas.py:445-615) for all repetitions on the device in one call (mcsas_hip_histogram).
    `specs`: per histogram a dict(param_index, yweight, edges (n_bin + 1 lower edges), lower, upper).
    Returns (scaling[2][R], fractions dict like mcsas.histogram's {'vol': (vf, mv), ...}, per histogram a dict with
    bins[n_bin][R], obs[n_bin][R], cdf[n_bin][R], moments[5][R]).
    `partial`: per spec 0, 1 (or "range") or 2 (or "bins"), or each spec dict may carry `partial` — the partial intensities
    (mcsas_hip_histogram_partial): a histogram that asks gains intensity[nq][R], the scattering curve of the contributions inside
    lower < x < upper times the repetition's scale, and with 2 also bin_intensity[n_bin][nq][R], the same of each bin's members
    (n_bin <= HISTOGRAM_PARTIAL_MAX_BINS); parameter.partial_intensities is the numpy form, equal bit for bit.  Without a request
    the call is the plain one."""
    lib = _lib.load()
    call = _HistogramCall(model, q, intensity, sigma, contribs, comp_exp, specs, find_background, positive_background, device, smear, partial)
    if call.want is None:
        check(lib.mcsas_hip_histogram(C.byref(call.prob.c), as_dp(call.contribs), len(call.specs), call.arr, as_dp(call.sc), as_dp(call.frac),
                                      as_dp(call.out)), lib)
    else:
        check(lib.mcsas_hip_histogram_partial(C.byref(call.prob.c), as_dp(call.contribs), len(call.specs), call.arr, call.want_p(), as_dp(call.sc),
                                              as_dp(call.frac), as_dp(call.out), as_dp(call.partial)), lib)
    return call.unpack()


def histogram_sets(model: ModelSetup, sets, contribs, comp_exp, specs, find_background=True, device=-1, scale="per_set", ref_set=0,
                   visible=None):
    """McSAS.histogram() of a joint fit (mcsas_hip_histogram_sets, include/mcsas_hip.h): histogram_device over the points of all
    `sets` (analyse_sets' list of (q, I, sigma)).  Per repetition the summed intensity is fitted per set (`scale` "per_set") or with
    one scale for all sets ("shared"); volume fractions are by set `ref_set`'s scale (the shared one in shared mode), and a
    contribution's visibility limit is the lowest over the points of the sets in `visible` (indices; None: all sets), each point with
    its own set's scale.  -> (scaling[2][R] of ref_set, fractions, histograms) as histogram_device, then set_scaling[S][R] and
    set_background[S][R].  No partial intensities, smearing or positive background; built-in models only."""
    mode = _sets_scale_mode(scale, "histogram_sets")
    triples, cat = _sets_triples(sets, "histogram_sets")
    S = len(triples)
    vis = range(S) if visible is None else [int(v) for v in visible]
    if any(v < 0 or v >= 32 for v in vis):
        raise ValueError("histogram_sets: visible %r names a set that is not there (%d sets)" % (list(vis), S))
    mask = 0
    for v in vis:
        mask |= 1 << v
    if any(sp.get("partial") for sp in specs):
        raise ValueError("histogram_sets: partial intensities are not offered for the histogram of a joint fit")
    lib = _lib.load()
    call = _HistogramCall(model, cat[0], cat[1], cat[2], contribs, comp_exp, specs, find_background, False, device, None)
    R = call.contribs.shape[2]
    set_nq = np.ascontiguousarray([len(t[0]) for t in triples], dtype=np.int32)
    set_scaling, set_background = np.zeros((max(S, 1), R)), np.zeros((max(S, 1), R))
    sr = _lib.SetsResult()
    sr.struct_size = C.sizeof(_lib.SetsResult)
    sr.n_sets = S
    sr.scaling, sr.background, sr.chisq = as_dp(set_scaling), as_dp(set_background), None
    check(lib.mcsas_hip_histogram_sets(C.byref(call.prob.c), as_dp(call.contribs), len(call.specs), call.arr, S,
                                       set_nq.ctypes.data_as(C.POINTER(C.c_int32)), mode, int(ref_set), mask, as_dp(call.sc), as_dp(call.frac),
                                       as_dp(call.out), C.byref(sr)), lib)
    return call.unpack() + (set_scaling[:S], set_background[:S])


class _HistogramCall:
    """The arguments of one mcsas_hip_histogram call (or of one set of mcsas_hip_histogram_batch) and the arrays it fills; owns
    every numpy buffer the C structures point at."""

    def __init__(self, model, q, intensity, sigma, contribs, comp_exp, specs, find_background=True, positive_background=False,
                 device=-1, smear=None, partial=None):
        self.contribs = f64(contribs)
        N, P, R = self.contribs.shape
        st = Settings(n_contrib=N, n_reps=R, comp_exp=comp_exp, device=device, find_background=find_background,
                      positive_background=positive_background)
        self.prob = HipProblem(model, q, intensity, sigma, st, smear=smear)
        self.specs = list(specs)
        self.arr = (_lib.HistogramSpec * max(len(self.specs), 1))()
        self.edges, n_out = [], 0
        for h, sp in enumerate(self.specs):
            e = f64(sp["edges"]).ravel()
            self.edges.append(e)
            a = self.arr[h]
            a.param_index = int(sp["param_index"]); a.weighting = YWEIGHT_INDEX[sp["yweight"]]
            a.n_bin = len(e) - 1; a.lower = float(sp["lower"]); a.upper = float(sp["upper"]); a.edges = as_dp(e)
            n_out += 3 * (len(e) - 1) * R + 5 * R
        self.sc = np.zeros((2, R)); self.frac = np.zeros((8, N, R)); self.out = np.zeros(max(n_out, 1))
        # the partial intensities asked for: `partial` per spec, or a spec's own entry; want None: nobody asks, the plain call
        if partial is not None and len(partial) != len(self.specs):
            raise ValueError("partial: %d entries for %d histograms" % (len(partial), len(self.specs)))
        asked = list(partial) if partial is not None else [sp.get("partial") for sp in self.specs]
        for a in asked:
            if isinstance(a, (bool, np.bool_)) and a or (a is not None and a not in PARTIAL_WANT):
                raise ValueError("partial: %r (0, 1 or 'range', 2 or 'bins')" % (a,))
        self.want = None
        if any(PARTIAL_WANT[a] for a in asked):
            nq = len(self.prob.q)
            self.want = np.array([PARTIAL_WANT[a] for a in asked], dtype=np.int32)
            n_part = sum(nq * R * (1 + (len(e) - 1 if w == 2 else 0)) for e, w in zip(self.edges, self.want) if w)
            self.partial = np.zeros(max(n_part, 1))

    def want_p(self):
        return self.want.ctypes.data_as(C.POINTER(C.c_int32))

    def unpack(self):
        frac, out, R = self.frac, self.out, self.contribs.shape[2]
        fractions = dict(vol=(frac[0], frac[4]), num=(frac[1], frac[5]), int=(frac[2], frac[6]), surf=(frac[3], frac[7]))
        hists, off = [], 0
        for e in self.edges:
            nb = len(e) - 1
            blk = out[off:off + 3 * nb * R + 5 * R]
            hists.append(dict(bins=blk[:nb * R].reshape(nb, R), obs=blk[nb * R:2 * nb * R].reshape(nb, R),
                              cdf=blk[2 * nb * R:3 * nb * R].reshape(nb, R), moments=blk[3 * nb * R:].reshape(5, R)))
            off += 3 * nb * R + 5 * R
        if self.want is not None:                            # per wanted histogram: range [nq][R], then bin [n_bin][nq][R]
            nq, off = len(self.prob.q), 0
            for h, e, w in zip(hists, self.edges, self.want):
                if w:
                    h["intensity"] = self.partial[off:off + nq * R].reshape(nq, R)
                    off += nq * R
                if w == 2:
                    nb = len(e) - 1
                    h["bin_intensity"] = self.partial[off:off + nb * nq * R].reshape(nb, nq, R)
                    off += nb * nq * R
        return self.sc, fractions, hists


def histogram_device_batch(items):
    """histogram_device for a list of data sets in one library call (mcsas_hip_histogram_batch): one upload, one launch per kernel
    over all sets, one download.  Each item is histogram_device's arguments, as a dict by name (model, q, intensity, sigma, contribs,
    comp_exp, specs, find_background, positive_background, device, smear) or as a tuple in that order; all on one device.
    Returns, per item, histogram_device's triple — the same arrays bit for bit."""
    lib = _lib.load()
    calls = [_HistogramCall(**it) if isinstance(it, dict) else _HistogramCall(*it) for it in items]   # (kept alive to the end of the call)
    n = len(calls)
    if any(c.want is not None for c in calls):
        raise ValueError("histogram_device_batch: the batch call has no partial intensities (histogram_device(partial=...) per set)")
    if n:
        dpp = C.POINTER(C.c_double) * n
        probs = (Problem * n)(*[c.prob.c for c in calls])
        n_hist = (C.c_int32 * n)(*[len(c.specs) for c in calls])
        specs = (C.POINTER(_lib.HistogramSpec) * n)(*[C.cast(c.arr, C.POINTER(_lib.HistogramSpec)) for c in calls])
        check(lib.mcsas_hip_histogram_batch(n, probs, dpp(*[as_dp(c.contribs) for c in calls]), n_hist, specs, dpp(*[as_dp(c.sc) for c in calls]),
                                            dpp(*[as_dp(c.frac) for c in calls]), dpp(*[as_dp(c.out) for c in calls])), lib)
    return [c.unpack() for c in calls]


HISTOGRAM2D_MAX_CELLS = 4096      # mcsas_hip_histogram2d keeps a histogram's cells in LDS


def fractions_array(fractions):
    """The [8][N][R] array mcsas_hip_histogram returns (vol, num, int, surf fractions, then their visibility limits) from the dict
    McSAS.fractions holds, {'vol': (vf, mv), ...}; an array is taken as it is."""
    if isinstance(fractions, dict):
        names = sorted(YWEIGHT_INDEX, key=YWEIGHT_INDEX.get)
        fractions = np.stack([fractions[k][0] for k in names] + [fractions[k][1] for k in names])
    return f64(fractions)


def histogram2d_device(contribs, fractions, specs, device=-1):
    """Joint histograms of two parameter columns on the device in one call (mcsas_hip_histogram2d; no model is evaluated).
    `contribs` [N][P][R]; `fractions`: the dict McSAS.fractions holds or the [8][N][R] array; `specs`: per histogram a dict(param_x,
    param_y, yweight, edges_x (n_bin_x + 1 lower edges), edges_y, lower_x, upper_x, lower_y, upper_y).  N <= HISTOGRAM_MAX_CONTRIBS
    and n_bin_x * n_bin_y <= HISTOGRAM2D_MAX_CELLS (beyond: parameter.Histogram2D.calc).
    Returns, per histogram, dict(bins[n_bin_x][n_bin_y][R], obs[n_bin_x][n_bin_y][R], moments[7][R]: total, mean x, mean y,
    variance x, variance y, covariance, correlation)."""
    lib = _lib.load()
    contribs = f64(contribs)
    if contribs.ndim != 3:
        raise ValueError("histogram2d_device: contribs must be (n_contrib, n_active, n_reps), got %r" % (contribs.shape,))
    N, P, R = contribs.shape
    frac = fractions_array(fractions)
    if frac.shape != (8, N, R):
        raise ValueError("histogram2d_device: fractions must be (8, %d, %d), got %r" % (N, R, frac.shape))
    specs = list(specs)
    arr = (_lib.Histogram2dSpec * max(len(specs), 1))()
    edges, n_out = [], 0
    for h, sp in enumerate(specs):
        ex, ey = f64(sp["edges_x"]).ravel(), f64(sp["edges_y"]).ravel()
        edges.append((ex, ey))                               # (kept alive to the end of the call)
        a = arr[h]
        a.param_x = int(sp["param_x"]); a.param_y = int(sp["param_y"]); a.weighting = YWEIGHT_INDEX[sp["yweight"]]
        a.n_bin_x = len(ex) - 1; a.n_bin_y = len(ey) - 1
        a.lower_x = float(sp["lower_x"]); a.upper_x = float(sp["upper_x"]); a.lower_y = float(sp["lower_y"]); a.upper_y = float(sp["upper_y"])
        a.edges_x = as_dp(ex); a.edges_y = as_dp(ey)
        n_out += 2 * max(a.n_bin_x, 0) * max(a.n_bin_y, 0) * R + 7 * R
    out = np.zeros(max(n_out, 1))
    check(lib.mcsas_hip_histogram2d(N, P, R, as_dp(contribs), as_dp(frac), len(specs), arr, as_dp(out), int(device)), lib)
    hists, off = [], 0
    for ex, ey in edges:
        nx, ny = len(ex) - 1, len(ey) - 1
        n = nx * ny * R
        hists.append(dict(bins=out[off:off + n].reshape(nx, ny, R), obs=out[off + n:off + 2 * n].reshape(nx, ny, R),
                          moments=out[off + 2 * n:off + 2 * n + 7 * R].reshape(7, R)))
        off += 2 * n + 7 * R
    return hists


def histogram_rows_shape(model: ModelSetup, q, st_or_sizes):
    """(min_rows, useful_rows, row_stride) of histogram_device_rows (mcsas_hip_histogram_rows_shape; no device is touched): the
    least and the most rows of a round, and the row pitch of the rows buffer (the q count, dense).  `st_or_sizes`: a Settings, or
    (n_contrib, n_reps)."""
    if isinstance(st_or_sizes, Settings):
        st = st_or_sizes
    else:
        n_contrib, n_reps = st_or_sizes
        st = Settings(n_contrib=int(n_contrib), n_reps=int(n_reps))
    q = f64(q).ravel()
    return _shape_triple(_lib.load().mcsas_hip_histogram_rows_shape, HipProblem(model, q, np.ones_like(q), np.ones_like(q), st))


def histogram_device_rows(model: ModelSetup, q, intensity, sigma, contribs, specs, row_fn, find_background=True,
                          positive_background=False, device=-1, capacity=None, partial=None):
    """histogram_device for a model whose rows the caller computes ON THE DEVICE with torch (mcsas_hip_histogram_device_rows,
    include/mcsas_hip.h): a round of whole repetitions at a time the library lays the parameter sets out in a torch tensor,
    `row_fn(pset[n][n_active]) -> (it[n][nq], v[n], w[n], s[n])` — calcIntensityBatch's return; pset is not yet clipped — gives the
    rows and each row's volume, weight and surface, which are copied into the library's views, and the scale / background fit, the
    visibility limits, fractions, bins and moments are taken on the device from the rows where they lie.  `capacity`: rows of the
    tensors (default: the most a round uses, histogram_rows_shape; at least n_contrib).  Returns histogram_device's triple.
    `partial`: as histogram_device takes it (mcsas_hip_histogram_partial_device_rows): the curves of a round are taken from the
    rows tensor as row_fn's answer was copied into it.
    torch is imported here, not with the package."""
    import torch                                 # (ahead of the library's first load: see _one_hip_runtime)
    lib = _lib.load()
    c3 = f64(contribs)
    if c3.ndim != 3 or c3.shape[1] != model.n_active or model.n_active < 1:
        raise ValueError("histogram_device_rows: contribs must be (n_contrib, n_active, n_reps) with n_active = %d >= 1, got %r"
                         % (model.n_active, c3.shape))
    call = _HistogramCall(model, q, intensity, sigma, c3, 0.0, specs, find_background, positive_background, device, None, partial)
    call.prob.c.model_id = MODEL_HOST
    nq = len(call.prob.q)
    capacity, dev, pset, rows, vws = _device_rows_tensors(
        "histogram_device_rows", _shape_triple(lib.mcsas_hip_histogram_rows_shape, call.prob), capacity,
        "one repetition takes (n_contrib)", device, model.n_active, vws=True)

    def fill(n):
        with torch.cuda.device(dev):
            it, v, w, s = row_fn(pset[:n])
            rows[:n, :nq].copy_(torch.as_tensor(it, dtype=torch.float64, device=dev).reshape(n, nq))
            for k, x in enumerate((v, w, s)):
                vws[k, :n].copy_(torch.as_tensor(x, dtype=torch.float64, device=dev))
            torch.cuda.current_stream(dev).synchronize()

    cb, failure = _rows_callback(_lib.DeviceRowsCallback, fill)
    if call.want is None:
        rc = lib.mcsas_hip_histogram_device_rows(C.byref(call.prob.c), as_dp(call.contribs), C.c_void_p(pset.data_ptr()),
                                                 C.c_void_p(rows.data_ptr()), C.c_void_p(vws.data_ptr()), capacity,
                                                 cb, None, len(call.specs), call.arr, as_dp(call.sc), as_dp(call.frac), as_dp(call.out))
    else:
        rc = lib.mcsas_hip_histogram_partial_device_rows(C.byref(call.prob.c), as_dp(call.contribs), C.c_void_p(pset.data_ptr()),
                                                         C.c_void_p(rows.data_ptr()), C.c_void_p(vws.data_ptr()), capacity,
                                                         cb, None, len(call.specs), call.arr, call.want_p(), as_dp(call.sc),
                                                         as_dp(call.frac), as_dp(call.out), as_dp(call.partial))
    if failure:
        raise failure[0]
    check(rc, lib)
    return call.unpack()


def prepare_uncertainty(intensity, sigma_raw, fu_min, device=-1):
    """DataObj._prepareUncertainty (dataobj/dataobj.py:204-227) on the GPU."""
    lib = _lib.load()
    I = f64(intensity).ravel()
    su = None if sigma_raw is None else f64(sigma_raw).ravel()
    out = np.zeros(len(I))
    check(lib.mcsas_hip_prepare_uncertainty(len(I), as_dp(I), as_dp(su) if su is not None else None, float(fu_min),
                                            int(device), as_dp(out)))
    return out


def rebin(x, f, fu, n_bin, device=-1):
    """DataObj._reBin (dataobj/dataobj.py:288-345) on the GPU: (x_binned, f_binned, fu_binned).  The
    log-spaced edges are the reference's numpy expression (:312-316), evaluated here on the host."""
    lib = _lib.load()
    x, f, fu = f64(x).ravel(), f64(f).ravel(), f64(fu).ravel()
    n_bin = int(n_bin)
    edges = np.logspace(np.log10(x.min()), np.log10(x.max() + np.diff(x)[-1] / 100.), n_bin + 1)
    xo, fo, uo = np.zeros(n_bin), np.zeros(n_bin), np.zeros(n_bin)
    k = C.c_int32(0)
    check(lib.mcsas_hip_rebin(len(x), as_dp(x), as_dp(f), as_dp(fu), n_bin, as_dp(edges), int(device),
                              as_dp(xo), as_dp(fo), as_dp(uo), C.byref(k)))
    return xo[:k.value].copy(), fo[:k.value].copy(), uo[:k.value].copy()


def device_count():
    return _lib.load().mcsas_hip_device_count()


def shard(n_reps, n_devices, index):
    """(first, count): the block of repetitions mcsas_hip_analyse gives device-list entry `index`."""
    first, count = C.c_int32(0), C.c_int32(0)
    check(_lib.load().mcsas_hip_shard(int(n_reps), int(n_devices), int(index), C.byref(first), C.byref(count)))
    return first.value, count.value

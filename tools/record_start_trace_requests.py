#!/usr/bin/env python3
"""What every entry point answers to a request for a given start, a trace, or both, over the execution modes and the q counts at
which the rule for them turns: tests/golden/start_trace_requests.json.

    python tools/record_start_trace_requests.py [output.json]

The rule (one wavefront per chain up to 4096 q-points; the q-split kernel where the workgroup mode is asked for more than 1024, up
to 16384; neither from the workgroup-window kernel nor the pipeline) is stated in the library and again in Python; this record
holds every layer's answer, so that a change of the rule's text cannot change an answer unseen.  tests/test_request_record.py asks
the working tree the same questions (answers() below) and compares; it never writes the file.

An answer is a string.  The C entries: "passes" for MCSAS_OK or MCSAS_ENODEV (as far as the device: there may be none), else
"rc <code>: <the library's message>".  The Python entries run against a stand-in for the library that notes whether it was loaded
and ends the call at the first library function: "passes: <function> with exec_mode [<of each problem handed over>]", else
"<exception> (before|after) load: <message>"; McSAS._problem needs no library: "passes: exec_mode <of the problem>".
Every problem is a sphere with 8 contributions, 2 or 3 repetitions and 10 steps, so that with a device a passing case is quick.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import mcsas_amd                                   # noqa: E402
from mcsas_amd import _lib, engine                 # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "start_trace_requests.json")
MODES = (0, 1, 2, 3)
NQ = (40, 1024, 1025, 4096, 4097, 16384, 16385)
N, CAPACITY = 8, 4
MCSAS_OK, MCSAS_ENODEV = 0, -2
# entry -> the requests it can be asked for ("none": the batch entries refuse by mode and size without either)
ENTRIES = (
    ("mcsas_hip_analyse_from", ("start",)),
    ("mcsas_hip_analyse_traced", ("trace", "both")),
    ("mcsas_hip_analyse_batch", ("none",)),
    ("engine.analyse", ("start", "trace", "both")),
    ("engine.analyse_many", ("start",)),
    ("engine.analyse_batch", ("none", "start")),
    ("McSAS.calc", ("start", "trace", "both")),
    ("McSAS._problem", ("start",)),
    ("run_series", ("start",)),
    ("run_series(batch)", ("start",)),
    ("run_series(overlap)", ("start",)),
)


def _data(nq):
    q = np.linspace(1e8, 2e9, nq)
    I = 1.0 / (1.0 + (q * 2e-9) ** 4)
    return q, I, 0.02 * I


def _sphere():
    m = mcsas_amd.Sphere()
    m.radius.setActiveRange((2e-9, 3e-7))
    return m


def _start(R):
    return np.full((N, 1, R), 5e-8)


class _Reached(Exception):
    pass


class _StandIn(object):
    """In place of _lib.load for the duration of one question: notes that the library was asked for, and ends the call at the first
    library function with the execution mode of every mcsas_problem among its arguments."""

    def __init__(self):
        self.loaded = False
        self.saved = _lib.load
        _lib.load = self.load

    def load(self, *a, **k):
        self.loaded = True
        return self

    def __getattr__(self, name):
        def call(*args):
            modes = []
            for a in args:
                a = getattr(a, "_obj", a)                  # (what C.byref holds)
                if isinstance(a, _lib.Problem):
                    modes.append(int(a.exec_mode))
                elif isinstance(a, C.Array) and len(a) and isinstance(a[0], _lib.Problem):
                    modes += [int(p.exec_mode) for p in a]
            raise _Reached("passes: %s with exec_mode %r" % (name, modes))
        return call

    def close(self):
        _lib.load = self.saved


def _algo(nq, mode):
    q, I, sig = _data(nq)
    algo = mcsas_amd.McSAS.factory()(seed=1, execMode=mode)
    algo.numContribs.setValue(N); algo.numReps.setValue(3); algo.maxIterations.setValue(10)
    algo.model = _sphere()
    algo.data = mcsas_amd.SASData(q, I, sig)
    return algo


def _ask_c(entry, request, mode, nq):
    R = 2
    lib = _lib.load()
    q, I, sig = _data(nq)
    st = engine.Settings(n_contrib=N, n_reps=R, max_iter=10, conv_crit=1e-9, max_retries=0, exec_mode=mode)
    prob = engine.HipProblem(_sphere().setup(), q, I, sig, st)
    res = engine.ChainResults(N, 1, R, nq)
    start = _start(R) if request in ("start", "both") else None
    given = None if start is None else _lib.as_dp(start)
    if entry == "mcsas_hip_analyse_from":
        rc = lib.mcsas_hip_analyse_from(C.byref(prob.c), given, C.byref(res.c))
    elif entry == "mcsas_hip_analyse_traced":
        tr = engine.ChainTrace(CAPACITY, 1, R)
        rc = lib.mcsas_hip_analyse_traced(C.byref(prob.c), given, C.byref(res.c), C.byref(tr.c))
    else:
        rc = lib.mcsas_hip_analyse_batch((_lib.Problem * 1)(prob.c), 1, (_lib.Result * 1)(res.c))
    if rc in (MCSAS_OK, MCSAS_ENODEV):
        return "passes"
    return "rc %d: %s" % (rc, lib.mcsas_hip_last_error().decode("utf-8", "replace"))


def _ask_python(entry, request, mode, nq):
    R = 3
    kw = {}
    if request in ("start", "both"):
        kw["start"] = _start(R)
    if request in ("trace", "both"):
        kw["trace"] = CAPACITY
    q, I, sig = _data(nq)
    st = engine.Settings(n_contrib=N, n_reps=R, max_iter=10, exec_mode=mode)
    pr = dict(model=_sphere().setup(), q=q, intensity=I, sigma=sig, st=st, **kw)
    lib = _StandIn()
    try:
        if entry == "engine.analyse":
            engine.analyse(pr["model"], q, I, sig, st, **kw)
        elif entry == "engine.analyse_many":
            engine.analyse_many([pr])
        elif entry == "engine.analyse_batch":
            engine.analyse_batch([pr])
        elif entry == "McSAS.calc":
            _algo(nq, mode).calc(**kw)
        elif entry == "McSAS._problem":
            return "passes: exec_mode %d" % _algo(nq, mode)._problem(**kw)["st"].exec_mode
        else:
            algo = _algo(40, mode)
            mcsas_amd.run_series(algo, [algo.data, _algo(nq, mode).data], start=kw["start"],
                                 batch=entry == "run_series(batch)", overlap=entry == "run_series(overlap)")
        return "returned"                                  # (no entry gets by without the library)
    except _Reached as e:
        return str(e)
    except Exception as e:
        return "%s %s load: %s" % (type(e).__name__, "after" if lib.loaded else "before", e)
    finally:
        lib.close()


def questions():
    for entry, requests in ENTRIES:
        for request in requests:
            for mode in MODES:
                for nq in NQ:
                    yield entry, request, mode, nq


def ask(entry, request, mode, nq):
    return (_ask_c if entry.startswith("mcsas_hip_") else _ask_python)(entry, request, mode, nq)


def answers():
    """[(entry, request, exec_mode, nq, answer)] of the package as it is imported now."""
    return [(e, r, m, n, ask(e, r, m, n)) for e, r, m, n in questions()]


def main(out=DEFAULT_OUT):
    texts, rows = [], []
    for e, r, m, n, a in answers():
        if a not in texts:
            texts.append(a)
        rows.append([e, r, m, n, texts.index(a)])
    with open(out, "w") as f:
        f.write('{"columns": ["entry", "request", "exec_mode", "nq", "answer"],\n "answers": [\n  ')
        f.write(",\n  ".join(json.dumps(t) for t in texts))
        f.write('\n ],\n "rows": [\n  ')
        f.write(",\n  ".join(json.dumps(row) for row in rows))
        f.write("\n ]}\n")
    print("%s: %d rows, %d distinct answers" % (out, len(rows), len(texts)))


if __name__ == "__main__":
    main(*sys.argv[1:2])

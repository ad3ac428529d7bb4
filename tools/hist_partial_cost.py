"""What the partial intensities cost, at config 2's shape: a sphere, 512 q x 400 contributions x 50 repetitions, one
50-bin histogram, fabricated contributions (uniform inside the active range: the cost does not depend on how good the fit is).

 1. engine.histogram_device without a request, on this tree and on a built checkout of the parent commit (--parent-tree), each in
    processes of its own, alternating, three times each: medians of 7 after a warm-up, and the parent's own run-to-run spread
    (largest less smallest of its medians) — the existing path did not change, so the two must agree within it.
 2. On this tree the call with "range" and with "bins": the added time beside what re-reading the rows costs at the HBM rate
    (wanted histograms x N R nq 8 bytes), and the host alternative: engine.model_calc(want_rows=True) per repetition plus the numpy
    form (parameter.partial_intensities).
Prints one JSON line; one machine, one shape.

    python tools/hist_partial_cost.py [--parent-tree DIR] [--repeats 7]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, N, REPS, BINS = 512, 400, 50, 50
LO, HI = 2e-9, 1e-7


def child(tree, modes, repeats):
    sys.path.insert(0, tree)
    import mcsas_amd
    from mcsas_amd import engine
    from bench import synthetic_data
    q, I, sig = synthetic_data(NQ)
    m = mcsas_amd.Sphere()
    m.radius.setActiveRange((LO, HI))
    setup = m.setup()
    contribs = np.random.RandomState(7).uniform(LO, HI, (N, 1, REPS))
    spec = dict(param_index=0, yweight="vol", edges=np.geomspace(LO, HI, BINS + 1), lower=LO, upper=HI)
    out = {}

    def run(mode):
        t0 = time.perf_counter()
        if mode == "none":
            engine.histogram_device(setup, q, I, sig, contribs, 0.6666666, [spec])
        elif mode in ("range", "bins"):
            engine.histogram_device(setup, q, I, sig, contribs, 0.6666666, [spec], partial=[mode])
        else:                                               # the host alternative, given the scales of a plain call
            from mcsas_amd.parameter import partial_intensities
            for r in range(REPS):
                rows = engine.model_calc(setup, q, contribs[:, :, r], 0.6666666, want_rows=True)[4]
                partial_intensities(rows, contribs[:, 0, r], scale[r], LO, HI, spec["edges"], mode == "host_bins")
        return time.perf_counter() - t0
    scale = engine.histogram_device(setup, q, I, sig, contribs, 0.6666666, [spec])[0][0]
    for mode in modes:
        for _ in range(2):
            run(mode)
        ms = 1e3 * np.array([run(mode) for _ in range(repeats)])
        out[mode] = dict(median=round(float(np.median(ms)), 3), min=round(float(ms.min()), 3), max=round(float(ms.max()), 3))
    print(json.dumps(out))


def spawn(tree, modes, repeats):
    env = dict(os.environ)
    env.pop("MCSAS_HIP_LIB", None)
    text = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", tree, "--modes", ",".join(modes), "--repeats", str(repeats)],
                                   env=env, timeout=600).decode()
    return json.loads([x for x in text.splitlines() if x.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--child", default=None)
    ap.add_argument("--modes", default="none")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.modes.split(","), a.repeats)
    out = dict(shape="sphere %d q x %d x %d, one %d-bin histogram" % (NQ, N, REPS, BINS), repeats=a.repeats)
    this, parent = [], []
    for _ in range(3):
        this.append(spawn(ROOT, ["none"], a.repeats)["none"])
        if a.parent_tree:
            parent.append(spawn(os.path.abspath(a.parent_tree), ["none"], a.repeats)["none"])
    out["without_request_ms"] = dict(this_tree=this, parent=parent)
    if parent:
        out["parent_run_to_run_spread_ms"] = round(max(p["median"] for p in parent) - min(p["median"] for p in parent), 3)
        out["this_tree_run_to_run_spread_ms"] = round(max(t["median"] for t in this) - min(t["median"] for t in this), 3)
        out["this_minus_parent_ms"] = round(float(np.mean([t["median"] for t in this]) - np.mean([p["median"] for p in parent])), 3)
    rest = spawn(ROOT, ["none", "range", "bins", "host_range", "host_bins"], a.repeats)
    out["this_tree_ms"] = rest
    out["added_ms"] = dict(range=round(rest["range"]["median"] - rest["none"]["median"], 3), bins=round(rest["bins"]["median"] - rest["none"]["median"], 3))
    out["rows_reread_bytes"] = N * REPS * NQ * 8
    print(json.dumps(out))


if __name__ == "__main__":
    main()

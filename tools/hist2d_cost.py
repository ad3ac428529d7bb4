"""What one joint histogram costs.

 1. McSAS.histogram() wall time with and without one 32 x 32 Histogram2D(radius, length), on fabricated contributions of the
    cylinders model (uniform inside the active ranges: histogram()'s cost does not depend on how good the fit is), alternating
    without, with after a warm-up of both; median, min, max and spread (max - min) of the repeats, at two shapes:
    512 q x 400 contributions x 50 repetitions and 100 q x 300 x 10.
 2. The device time of hist2d_kernel alone by HIP events (tools/microbench_hist2d.hip, built here if it is not): N = 4096, R = 50,
    cells 0 x 0 (the moments alone), 1 x 1, 8 x 8, 32 x 32 and 64 x 64, and the ratio 64 x 64 / 8 x 8.
Prints one JSON line; one machine, one shape each.

    python tools/hist2d_cost.py [--repeats 9]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcsas_amd                                    # noqa: E402
from bench import synthetic_data                    # noqa: E402

LO, HI = (2e-9, 5e-9), (4e-8, 2e-7)                 # radius, length


def make_algo(nq, n, reps):
    q, I, sig = synthetic_data(nq)
    m = mcsas_amd.CylindersIsotropic()
    m.useAspect.setValue(False)
    for p in m.params():
        if hasattr(p, "setActive"):
            p.setActive(p.name() in ("radius", "length"))
    m.radius.setActiveRange((LO[0], HI[0])); m.length.setActiveRange((LO[1], HI[1]))
    m.radius.histograms().append(mcsas_amd.Histogram(m.radius, LO[0], HI[0], binCount=50, xscale="log", yweight="vol"))
    m.length.histograms().append(mcsas_amd.Histogram(m.length, LO[1], HI[1], binCount=50, xscale="log", yweight="vol"))
    algo = mcsas_amd.McSAS(seed=1)
    algo.model = m
    algo.data = mcsas_amd.SASData(q, I, sig)
    rs = np.random.RandomState(7)
    contribs = np.stack([rs.uniform(LO[0], HI[0], (n, reps)), rs.uniform(LO[1], HI[1], (n, reps))], axis=1)
    algo.result = [dict(contribs=contribs)]
    joint = mcsas_amd.Histogram2D(m.radius, m.length, (LO[0], HI[0]), (LO[1], HI[1]), binCount=(32, 32), yweight="vol")
    return algo, joint


def stats(t):
    ms = 1e3 * np.array(t)
    return dict(median=round(float(np.median(ms)), 3), min=round(float(ms.min()), 3), max=round(float(ms.max()), 3),
                spread=round(float(np.ptp(ms)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()
    if mcsas_amd.device_count() < 1:
        raise SystemExit("hist2d_cost: no GPU; this is a measurement and has no fall-back")
    out = dict(repeats=a.repeats)
    for nq, n, reps in ((512, 400, 50), (100, 300, 10)):
        algo, joint = make_algo(nq, n, reps)

        def timed(with_joint):
            algo.histograms2d = [joint] if with_joint else []
            t0 = time.perf_counter()
            algo.histogram()                         # (returns after its last device-to-host copy)
            return time.perf_counter() - t0
        for _ in range(2):
            timed(False); timed(True)
        runs = {False: [], True: []}
        for _ in range(a.repeats):
            for w in (False, True):
                runs[w].append(timed(w))
        one = algo.model.radius.histograms()[0]
        key = "cylinders_%dq_%dx%d" % (nq, n, reps)
        out[key] = dict(without_ms=stats(runs[False]), with_one_32x32_ms=stats(runs[True]),
                        added_ms=round(stats(runs[True])["median"] - stats(runs[False])["median"], 3),
                        cells_sum_over_bins_sum=float(joint.bins.full.sum() / one.bins.full.sum()))
    exe = os.path.join(ROOT, "tools", "microbench_hist2d")
    if not os.path.exists(exe):
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I", os.path.join(ROOT, "mcsas_amd", "csrc"),
                               os.path.join(ROOT, "tools", "microbench_hist2d.hip"), "-o", exe])
    lines = [json.loads(x) for x in subprocess.check_output([exe, "4096", "50", "21"], timeout=120).decode().splitlines() if x.startswith("{")]
    out["kernel_alone_us"] = lines
    by = {(x["nx"], x["ny"]): x["median_us"] for x in lines}
    out["ratio_64x64_over_8x8"] = round(by[(64, 64)] / by[(8, 8)], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

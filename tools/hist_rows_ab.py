"""McSAS.histogram() and McSAS.calc() of a model typed in torch (calcIntensityBatch), with histogram() on the host path — the rows
downloaded, one engine.bgfit call per repetition, the visibility limits in a numpy loop, Histogram.calc in numpy: what histogram()
did for such a model before mcsas_hip_histogram_device_rows, kept as McSAS.deviceRowsHistogram = False — against histogram() on the
rows where the model left them on the device (True).  TorchSphere, 100 q x 200 contributions x 10 repetitions, four histograms.
After a warm-up of both the runs alternate host, device, host, device ...; median and spread (max - min) of the repeats of each.
histogram() is timed on the contributions of one analysis; calc() is that analysis (a fixed budget of steps with a criterion no
chain reaches, same seed) followed by histogram().  Both paths' results are compared as a check that they did the same work.
Prints one JSON line; --md writes the table of profiles/hist_rows_ab.md.

    python tools/hist_rows_ab.py [--repeats 9] [--steps 2000] [--md profiles/hist_rows_ab.md]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcsas_amd                                    # noqa: E402
from bench import synthetic_data                    # noqa: E402


class TorchSphere(mcsas_amd.SASModel):
    """models/sphere.py:12-63 typed in torch: the batch form of calcIntensity."""
    parameters = mcsas_amd.Sphere.parameters

    def __init__(self):
        super().__init__()
        self.radius.setActive(True)

    def calcIntensityBatch(self, q, pset, compensationExponent):
        import torch
        r = pset[:, 0]
        vol = (np.pi * 4. / 3.) * r**3
        qr = q[None, :] * r[:, None]
        ff = 3. * (torch.sin(qr) - qr * torch.cos(qr)) / (qr**3)
        w = vol ** (2 * compensationExponent)
        return ff**2 * w[:, None], vol * self.sld()**2, w, 4. * np.pi * r * r


def make_algo(steps):
    q, I, sig = synthetic_data(100)
    m = TorchSphere()
    lo, hi = 2e-9, 3e-7
    m.radius.setActiveRange((lo, hi))
    for nb, xscale, yweight in ((50, "log", "vol"), (50, "log", "num"), (50, "lin", "int"), (50, "log", "surf")):
        m.radius.histograms().append(mcsas_amd.Histogram(m.radius, lo, hi, binCount=nb, xscale=xscale, yweight=yweight))
    algo = mcsas_amd.McSAS(seed=1)
    algo.numContribs.setValue(200); algo.numReps.setValue(10); algo.maxIterations.setValue(steps)
    algo.convergenceCriterion.setValue(0.0); algo.showIncomplete.setValue(True)
    algo.maxRetries = mcsas_amd.mcsas._Setting("maxRetries", 0)
    algo.model = m
    algo.data = mcsas_amd.SASData(q, I, sig)
    return algo


def snapshot(algo):
    h = [x for p in algo.model.activeParams() for x in p.histograms()]
    return [np.array(algo.result[0]["scalingFactors"])] + [np.array(x.bins.full) for x in h] + [np.array(x.moments.fields) for x in h]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("hist_rows_ab: no GPU; this is a measurement and has no fall-back")
    algo = make_algo(a.steps)
    kinds = (("host", False), ("device", True))

    def timed(what, on_device):
        algo.deviceRowsHistogram = on_device
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        getattr(algo, what)()                      # (both paths return after their last device-to-host copy)
        return time.perf_counter() - t0

    logging_off()
    for _ in range(2):                             # warm-up: code objects, torch's kernels and allocator, the library's memory cache
        for kind, on in kinds:
            timed("calc", on)
            timed("histogram", on)
    runs = {(what, kind): [] for what in ("histogram", "calc") for kind, _ in kinds}
    results = {}
    for what in ("histogram", "calc"):             # (histogram: on the contributions the last calc() stored)
        for _ in range(a.repeats):
            for kind, on in kinds:
                runs[(what, kind)].append(timed(what, on))
                results[(what, kind)] = snapshot(algo)
    worst = 0.
    for x, y in zip(results[("histogram", "host")], results[("histogram", "device")]):
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(x - y) / np.abs(x)
        rel = rel[np.isfinite(rel)]
        worst = max(worst, float(rel.max()) if rel.size else 0.)
    out = dict(shape="torch sphere, 100 q x 200 contributions x 10 repetitions, 4 histograms of 50 bins", steps_per_chain=a.steps,
               repeats=a.repeats, device=torch.cuda.get_device_name(0), largest_relative_difference=worst)
    for (what, kind), t in runs.items():
        ms = 1e3 * np.array(t)
        out["%s_%s_ms" % (what, kind)] = dict(median=round(float(np.median(ms)), 3), min=round(float(ms.min()), 3),
                                              max=round(float(ms.max()), 3), spread=round(float(np.ptp(ms)), 3))
    for what in ("histogram", "calc"):
        h, d = out["%s_host_ms" % what], out["%s_device_ms" % what]
        out["%s_gain_ms" % what] = round(h["median"] - d["median"], 3)
        out["%s_gain_exceeds_spread" % what] = bool(h["median"] - d["median"] > max(h["spread"], d["spread"]))
    print(json.dumps(out))
    if a.md:
        with open(a.md, "w") as f:
            f.write("# histogram() of a torch model: host path against device rows\n\n")
            f.write("`python tools/hist_rows_ab.py --repeats %d --steps %d` on one %s; %s.  Wall time in ms around the call, "
                    "runs alternating host, device after a warm-up of both; spread = max - min of the repeats.\n\n"
                    % (a.repeats, a.steps, out["device"], out["shape"]))
            f.write("| call | path | median | min | max | spread |\n|---|---|---|---|---|---|\n")
            for what in ("histogram", "calc"):
                for kind, _ in kinds:
                    r = out["%s_%s_ms" % (what, kind)]
                    f.write("| `%s()` | %s | %.3f | %.3f | %.3f | %.3f |\n" % (what, kind, r["median"], r["min"], r["max"], r["spread"]))
            f.write("\nGain of the device path (difference of the medians): histogram() %.3f ms, calc() %.3f ms (%d steps per chain); "
                    "larger than the spread of either path's repeats: %s / %s.  Largest relative difference between the two paths' "
                    "scaling factors, bins and moments: %.2e.\n"
                    % (out["histogram_gain_ms"], out["calc_gain_ms"], a.steps, out["histogram_gain_exceeds_spread"],
                       out["calc_gain_exceeds_spread"], worst))


def logging_off():
    import logging
    logging.disable(logging.WARNING)               # (every calc() warns that the criterion was not reached: that is the set-up)


if __name__ == "__main__":
    main()

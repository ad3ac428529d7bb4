#!/usr/bin/env python3
"""A series of data sets, four ways, at two shapes — prints one JSON line (profiles/*_series_batch.json keeps the measured one).

Shapes, both at a fixed budget (conv_crit 0, max_iter 20 000, no retries), seeded synthetic sphere data sets whose size
distributions differ from one data set to the next:
  a  reference defaults: 100 q x 300 contributions x 10 repetitions x 200 data sets
  b  config 2's shape:   512 q x 400 contributions x 50 repetitions x 160 data sets
Per shape, MC steps per second of
  sequential     engine.analyse per data set, one after the other (exec mode auto: what run_series(overlap=False) runs)
  analyse_many   the overlapped series (a plan per data set, two per stream on two streams)
  analyse_batch  every chain of every data set in one wavefront-per-chain launch (wall, plans created and fetched included)
  batch_device   resident plans, engine.launch_batch, device time of the launch (HIP events)
  single_wave    the upper bound: one wave-mode plan with the same total chain count on ONE data set, device time
Shape a also runs run_series(batch=True) end to end, with the histograms per data set and in one batched pass (batch_histograms),
and reports median and spread of the wall time, the share of it in the histograms and the split of that into the library call and
the Python around it; one McSAS.histogram() at config 2's shape is timed the same way (--hist-only: these two alone).
Every timed quantity is repeated until at least a second has been timed (after a warm-up run), and 16 chains of different data
sets from the timed batch are checked against the plain-C oracle on the same Philox streams.

    python3 tools/bench_series_batch.py [--steps 20000] [--shapes a,b]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mcsas_amd                      # noqa: E402
from mcsas_amd import engine          # noqa: E402

SHAPES = {"a": dict(nq=100, n=300, reps=10, sets=200), "b": dict(nq=512, n=400, reps=50, sets=160)}


def dataset(nq, d):
    """Synthetic sphere curve (bench.synthetic_data's q grid and noise model) of data set d: a two-mode population whose mode
    radii, widths and weights follow d."""
    q = np.logspace(7, np.log10(3e9), nq)
    rs = np.random.RandomState(1000 + d)
    r1, r2 = 5.0 + 10.0 * rs.rand(), 30.0 + 60.0 * rs.rand()
    radii = np.abs(np.concatenate([rs.normal(r1, 0.3 * r1, 300), rs.normal(r2, 0.15 * r2, int(50 + 150 * rs.rand()))])) + 0.5
    radii *= 1e-9
    I = np.zeros(nq)
    for R in radii:
        x = q * R
        I += (4 * np.pi / 3 * R**3)**2 * (3 * (np.sin(x) - x * np.cos(x)) / x**3)**2
    I *= 1e3 / I.max()
    sigma = 0.01 * I
    return q, I + sigma * rs.normal(size=nq), sigma


def timed(fn, min_s=1.0):
    """(seconds per call, last result) over as many calls as make at least min_s, after one warm-up call."""
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        out = fn()
        n += 1
        el = time.perf_counter() - t0
        if el >= min_s:
            return el / n, out


def timed_device(launch, plans, min_s=1.0):
    """Device seconds per launch (HIP events of the plans' launches: max over the plans of a launch), summed until min_s."""
    launch(); [p.fetch(want_arrays=False) for p in plans]
    tot, n = 0.0, 0
    while tot < min_s:
        launch()
        for p in plans:
            p.fetch(want_arrays=False)
        tot += max(p.last_ms for p in plans) * 1e-3
        n += 1
    return tot / n


def run_shape(key, steps, check):
    sh = SHAPES[key]
    nq, n, reps, sets = sh["nq"], sh["n"], sh["reps"], sh["sets"]
    q = dataset(nq, 0)[0]
    lo, hi = np.pi / q.max(), np.pi / q.min()
    model = mcsas_amd.Sphere(); model.radius.setActiveRange((lo, hi))
    setup = model.setup()
    data = [dataset(nq, d) for d in range(sets)]

    def st(d, **kw):
        return engine.Settings(**{**dict(n_contrib=n, n_reps=reps, max_iter=steps, conv_crit=0.0, max_retries=0, seed=7000 + d), **kw})

    probs = [(setup, q, I, s, st(d)) for d, (q, I, s) in enumerate(data)]
    total = float(sets) * reps * steps
    out = dict(shape="%d q x %d contributions x %d reps x %d data sets" % (nq, n, reps, sets), steps=steps, chains=sets * reps)
    t_seq, _ = timed(lambda: [engine.analyse(*p) for p in probs])
    t_many, _ = timed(lambda: engine.analyse_many(probs))
    t_batch, got = timed(lambda: engine.analyse_batch(probs))
    assert all((g.num_iter == steps).all() for g in got)
    plans = [engine.Plan(*p[:4], st(d, exec_mode=engine.EXEC_WAVE)) for d, p in enumerate(probs)]
    t_bdev = timed_device(lambda: engine.launch_batch(plans), plans)
    info = plans[0].info
    for p in plans:
        p.close()
    one = engine.Plan(setup, *data[0], st(0, n_reps=sets * reps, exec_mode=engine.EXEC_WAVE))
    t_single = timed_device(lambda: one.launch(), [one])
    one.close()
    out.update(q_per_lane=info["q_per_lane"], cached_rows=info["cached_rows"],
               steps_per_s=dict(sequential=total / t_seq, analyse_many=total / t_many, analyse_batch=total / t_batch,
                                batch_device=total / t_bdev, single_wave=total / t_single),
               seconds=dict(sequential=t_seq, analyse_many=t_many, analyse_batch=t_batch, batch_device=t_bdev, single_wave=t_single))
    out["batch_device_over_single_wave"] = t_single / t_bdev
    out["analyse_batch_over_analyse_many"] = t_many / t_batch
    out["analyse_batch_over_sequential"] = t_seq / t_batch
    if check:
        from oracle import c_oracle
        picks = [(int(d), int(r)) for d, r in zip(np.linspace(0, sets - 1, 16).round(), np.arange(16) * 7 % reps)]
        for d, r in picks:
            qd, Id, sd = data[d]
            ref = c_oracle.analyse_sphere(qd, Id, sd, lo, hi, n, 1, steps, 0.0, seed=7000 + d, rep_offset=r, threads=1)
            assert got[d].num_moves[r] == ref.num_moves[0], (key, d, r)
            np.testing.assert_allclose(got[d].contribs[:, :, r], ref.contribs[:, :, 0], rtol=1e-12)
            np.testing.assert_allclose(got[d].chisq[r], ref.chisq[0], rtol=1e-7)
        out["oracle_chains_checked"] = len(picks)
    return out, model, data


def stats(xs):
    """median and spread (largest minus smallest) of the repeats"""
    xs = sorted(float(x) for x in xs)
    return dict(median=xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]), spread=xs[-1] - xs[0], n=len(xs))


class Stopwatch:
    """Adds up the time spent inside the callables it wraps (one wrapped callable inside another counts once)."""

    def __init__(self):
        self.s, self.depth = 0.0, 0

    def wrap(self, fn):
        def timed(*a, **k):
            t0 = time.perf_counter()
            self.depth += 1
            try:
                return fn(*a, **k)
            finally:
                self.depth -= 1
                if self.depth == 0:
                    self.s += time.perf_counter() - t0
        return timed


def series_wall(model, data, steps, repeats=7):
    """run_series(batch=True) end to end over shape a's data sets, `repeats` times after a warm-up run, in this process: wall time,
    the time in McSAS.histogram() (the call per data set) or in engine.histogram_device_batch (the batched pass), and how much of
    either is spent inside the library call — the rest is the Python around it: setup_from_model, the histogram records,
    Histogram.setFromDevice and its Moments.  One entry per value of batch_histograms the installed run_series knows."""
    import inspect
    from mcsas_amd import _lib, series
    q = data[0][0]
    model.radius.histograms().append(mcsas_amd.Histogram(model.radius, np.pi / q.max(), np.pi / q.min(), binCount=50, xscale='log',
                                                         yweight='vol'))
    datasets = [mcsas_amd.SASData(*d) for d in data]
    algo = mcsas_amd.McSAS(seed=11)
    algo.numContribs.setValue(SHAPES["a"]["n"]); algo.numReps.setValue(SHAPES["a"]["reps"]); algo.maxIterations.setValue(steps)
    algo.convergenceCriterion.setValue(0.0); algo.maxRetries.setValue(0); algo.showIncomplete.setValue(True)
    algo.model = model
    lib = _lib.load()
    in_hist, in_lib, in_apply = Stopwatch(), Stopwatch(), Stopwatch()
    algo.histogram = in_hist.wrap(algo.histogram)
    lib.mcsas_hip_histogram = in_lib.wrap(lib.mcsas_hip_histogram)
    modes = {"per_data_set": {}}
    if "batch_histograms" in inspect.signature(mcsas_amd.run_series).parameters:
        modes = {"per_data_set": dict(batch_histograms=False), "batched": dict(batch_histograms=True)}
        lib.mcsas_hip_histogram_batch = in_lib.wrap(lib.mcsas_hip_histogram_batch)
        engine.histogram_device_batch = in_hist.wrap(engine.histogram_device_batch)
        algo._histogram_item = in_hist.wrap(algo._histogram_item)
        algo._histogram_from_device = in_apply.wrap(algo._histogram_from_device)
    out = dict(data_sets=len(datasets), repeats=repeats)
    for name, kw in modes.items():
        mcsas_amd.run_series(algo, datasets, batch=True, **kw)             # (warm-up)
        wall, hist, libs = [], [], []
        for _ in range(repeats):
            in_hist.s = in_lib.s = in_apply.s = 0.0
            t0 = time.perf_counter()
            results, _series = mcsas_amd.run_series(algo, datasets, batch=True, **kw)
            wall.append(time.perf_counter() - t0)
            # (the per-data-set loop applies the results inside histogram(); the batched pass applies them in the loop after it)
            hist.append(in_hist.s + (in_apply.s if name == "batched" else 0.0)); libs.append(in_lib.s)
            assert all(r is not None for r in results)
        out[name] = dict(wall_s=stats(wall), histogram_s=stats(hist), library_s=stats(libs), python_s=stats([h - l for h, l in zip(hist, libs)]),
                         histogram_share=stats([h / w for h, w in zip(hist, wall)]),
                         library_share_of_histogram=stats([l / h for h, l in zip(hist, libs)]))
    if "batched" in out:
        gain = out["per_data_set"]["wall_s"]["median"] - out["batched"]["wall_s"]["median"]
        out["gain_s"] = gain
        out["batched_is_faster_beyond_spread"] = bool(gain > max(out["per_data_set"]["wall_s"]["spread"], out["batched"]["wall_s"]["spread"]))
        out["default_batch_histograms"] = bool(series.BATCH_HISTOGRAMS_DEFAULT)
    return out


def single_histogram(repeats=9):
    """One McSAS.histogram() at config 2's shape (50 repetitions x 400 contributions x 512 q, one 50-bin histogram), seeded
    contributions: seconds per call of the whole method and of the library call in it."""
    from bench import synthetic_data
    from mcsas_amd import _lib
    q, I, sig = synthetic_data(512)
    lo, hi = np.pi / q.max(), np.pi / q.min()
    model = mcsas_amd.Sphere(); model.radius.setActiveRange((lo, hi))
    model.radius.histograms().append(mcsas_amd.Histogram(model.radius, lo, hi, binCount=50, xscale='log', yweight='vol'))
    algo = mcsas_amd.McSAS(seed=5)
    algo.model = model
    algo.data = mcsas_amd.SASData(q, I, sig)
    algo.result = [dict(contribs=np.exp(np.random.RandomState(5).uniform(np.log(lo), np.log(hi), (400, 1, 50))))]
    lib = _lib.load()
    in_lib = Stopwatch()
    lib.mcsas_hip_histogram = in_lib.wrap(lib.mcsas_hip_histogram)
    algo.histogram()                                                      # (warm-up)
    wall, libs = [], []
    for _ in range(repeats):
        in_lib.s = 0.0
        t0 = time.perf_counter()
        algo.histogram()
        wall.append(time.perf_counter() - t0); libs.append(in_lib.s)
    return dict(shape="512 q x 400 contributions x 50 reps, one 50-bin histogram", histogram_s=stats(wall), library_s=stats(libs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--hist-only", action="store_true", help="only the histogram measurements: run_series over shape a and the single call at config 2's shape")
    args = ap.parse_args()
    line = dict(metric="series_batch", steps=args.steps, shapes={})
    if args.hist_only:
        q = dataset(SHAPES["a"]["nq"], 0)[0]
        model = mcsas_amd.Sphere(); model.radius.setActiveRange((np.pi / q.max(), np.pi / q.min()))
        line["single_histogram_config2"] = single_histogram()
        line["run_series_batch"] = series_wall(model, [dataset(SHAPES["a"]["nq"], d) for d in range(SHAPES["a"]["sets"])], args.steps)
        print(json.dumps(line))
        return
    for key in args.shapes.split(","):
        res, model, data = run_shape(key, args.steps, not args.no_check)
        line["shapes"][key] = res
        if key == "a":
            line["run_series_batch"] = series_wall(model, data, args.steps)
    line["single_histogram_config2"] = single_histogram()
    print(json.dumps(line))


if __name__ == "__main__":
    main()

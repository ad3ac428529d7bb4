#!/usr/bin/env python3
"""A drifting series through run_series, every frame cold against every frame started from the previous frame's result
(run_series(start="previous")): Monte-Carlo steps per chain and frame to a fixed criterion.  The series: polydisperse spheres
(log-normal radii) whose median radius grows by 1 % per frame, 2 % noise.  Both runs go one wavefront per chain with the same seed.
A measurement: it asserts nothing."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mcsas_amd
from mcsas_amd import engine

FRAMES, NQ, N, REPS, CRIT = 24, 100, 300, 10, 1.5
q = np.geomspace(5e7, 2e9, NQ)
m = mcsas_amd.Sphere()
m.radius.setActiveRange((np.pi / q.max(), np.pi / q.min()))
rng = np.random.default_rng(1)
datasets = []
for k in range(FRAMES):
    radii = np.exp(rng.normal(np.log(2e-8 * 1.01 ** k), 0.25, 400))
    I = m.calc(q, radii[:, None], 0.6666666).chisqrInt
    I = I / I.max() + 1e-3
    sig = 0.02 * I
    datasets.append(mcsas_amd.SASData(q, I + sig * rng.standard_normal(NQ), sig))
for label, start in (("cold", None), ("from the previous frame", "previous")):
    algo = mcsas_amd.McSAS.factory()(seed=7, device=0, execMode=engine.EXEC_WAVE)
    algo.numContribs.setValue(N); algo.numReps.setValue(REPS); algo.maxIterations.setValue(200000)
    algo.convergenceCriterion.setValue(CRIT); algo.maxRetries.setValue(1)
    algo.model = m
    t0 = time.perf_counter()
    results, _ = mcsas_amd.run_series(algo, datasets, start=start)
    dt = time.perf_counter() - t0
    steps = [r["numIter"] for r in results if r is not None]
    print("%-24s %d frames x %d reps to chi2 <= %.2f: %d frames stored, %.0f steps per chain and frame (first frame %.0f, the others "
          "%.0f), %.1f ms per frame with its histograms" % (label, FRAMES, REPS, CRIT, len(steps), np.mean(steps), steps[0],
                                                            np.mean(steps[1:]), dt / FRAMES * 1e3), flush=True)

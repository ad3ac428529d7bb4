"""What the joint fit of several data sets costs per step: engine.analyse_sets on 2 x 256 points against the existing
wavefront kernel (engine.analyse, one wavefront per chain, cached rows) on one set of 512 points — the same 8 q slots per lane, the
same rows; what differs is the per-set reduction, solve and comparison.  Sphere and CylindersIsotropic, 4096 chains, a fixed budget
of steps, criterion 0 (no chain converges), one seed.  Neither call has a plan to ask for its device time, so each is timed by the
host clock around the call (which ends in a device synchronise) at a budget of K and of 2 K steps: the difference is the time of
K steps per chain, and what both calls pay besides — allocation, the initial sets, copies — drops out.  The four runs alternate and
repeat; medians.  Prints one JSON line per model.  --scale shared times the joint fit with one scale for all sets
(mcsas_hip_analyse_sets_mode, MCSAS_SETS_SCALE_SHARED) beside the per-set mode, alternating with it, on sets brought to one scale.

    python tools/sets_cost.py [--model sphere|cyl|both] [--chains 4096] [--contribs 200] [--repeats 3] [--scale per_set|shared]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcsas_amd                                    # noqa: E402
from mcsas_amd import engine                        # noqa: E402
from bench import synthetic_data                    # noqa: E402

# model: (steps K per chain, factory)
STEPS = {"sphere": 20000, "cyl": 400}


def model_of(name):
    if name == "sphere":
        m = mcsas_amd.Sphere()
        m.radius.setActiveRange((2e-9, 3e-7))
        return m
    m = mcsas_amd.CylindersIsotropic()
    m.radius.setActive(True); m.aspect.setActive(True)
    m.radius.setActiveRange((1e-9, 1e-7)); m.aspect.setActiveRange((0.5, 20.0))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("sphere", "cyl", "both"), default="both")
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--contribs", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=0, help="K (default: %r)" % STEPS)
    ap.add_argument("--scale", choices=("per_set", "shared"), default="per_set", help="shared: also time the shared-scale mode")
    a = ap.parse_args()
    if engine.device_count() < 1:
        sys.exit("sets_cost: no GPU; a timing needs one")
    q, I, sig = synthetic_data(512)
    # the joint fit's sets: the even and the odd points of the same curve, the second through a scale of 250 and a background
    sets = [(q[0::2], I[0::2], sig[0::2]), (q[1::2], 250. * I[1::2] + 40., 250. * sig[1::2])]
    # ... and for the shared mode the same second set divided by its scale of 250, intensities and uncertainties alike
    sets_one_scale = [sets[0], (q[1::2], I[1::2] + 40. / 250., sig[1::2])]
    for name in (("sphere", "cyl") if a.model == "both" else (a.model,)):
        K = a.steps or STEPS[name]
        setup = model_of(name).setup()

        def settings(steps):
            return engine.Settings(n_contrib=a.contribs, n_reps=a.chains, max_iter=steps, conv_crit=0.0, max_retries=0, seed=1,
                                   exec_mode=engine.EXEC_WAVE, cache_intensities=1, device=0)

        def timed(joint, steps):
            t0 = time.perf_counter()
            if joint:
                res = engine.analyse_sets(setup, sets, settings(steps))
            else:
                res = engine.analyse(setup, q, I, sig, settings(steps))
            dt = time.perf_counter() - t0
            assert (res.num_iter == steps).all()
            return dt

        def timed_shared(steps):
            t0 = time.perf_counter()
            res = engine.analyse_sets(setup, sets_one_scale, settings(steps), scale="shared")
            dt = time.perf_counter() - t0
            assert (res.num_iter == steps).all()
            return dt

        timed(False, 64); timed(True, 64)                                        # warm-up: code objects, the row cache's pages
        ts = {1: [], 2: []}
        if a.scale == "shared":
            timed_shared(64)
        t = {(j, k): [] for j in (False, True) for k in (1, 2)}
        for _ in range(a.repeats):
            for j in (False, True):
                for k in (1, 2):
                    t[(j, k)].append(timed(j, k * K))
            if a.scale == "shared":
                for k in (1, 2):
                    ts[k].append(timed_shared(k * K))
        med = {key: float(np.median(v)) for key, v in t.items()}
        steps = float(a.chains) * K
        single, joint = steps / (med[(False, 2)] - med[(False, 1)]), steps / (med[(True, 2)] - med[(True, 1)])
        spread = {("joint" if j else "single") + "_%dK_s" % k: [round(x, 4) for x in v] for (j, k), v in t.items()}
        extra = {}
        if a.scale == "shared":
            shared = steps / (float(np.median(ts[2])) - float(np.median(ts[1])))
            extra = dict(shared_2x256q_steps_per_s=round(shared, 1), shared_over_per_set_time_per_step=round(joint / shared, 4))
            spread.update({"shared_%dK_s" % k: [round(x, 4) for x in v] for k, v in ts.items()})
        print(json.dumps(dict(model=name, chains=a.chains, contribs=a.contribs, steps_K=K, q_slots_per_lane=8,
                              single_512q_steps_per_s=round(single, 1), joint_2x256q_steps_per_s=round(joint, 1),
                              joint_over_single_time_per_step=round(single / joint, 4), **extra, runs=spread)), flush=True)


if __name__ == "__main__":
    main()

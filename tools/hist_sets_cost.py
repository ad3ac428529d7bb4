"""What the histogram of a joint fit costs, at config 2's shape: a sphere, 400 contributions x 50 repetitions, one
50-bin histogram, fabricated contributions (uniform inside the active range: the cost does not depend on how good the fit is).
engine.histogram_sets on 2 x 256 points (the even and the odd points of the curve, all sets visible; per-set and shared scale)
against engine.histogram_device on the 512 points: the same rows kernel over the same points, what differs is the per-set fit and the
visibility kernel that takes each point's own scale.  Host clock around the call, alternating, medians of --repeats after a warm-up.
Prints one JSON line.

    python tools/hist_sets_cost.py [--repeats 7]"""
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

NQ, N, REPS, BINS = 512, 400, 50, 50
LO, HI = 2e-9, 1e-7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if engine.device_count() < 1:
        sys.exit("hist_sets_cost: no GPU; a timing needs one")
    q, I, sig = synthetic_data(NQ)
    sets = [(q[0::2], I[0::2], sig[0::2]), (q[1::2], I[1::2] + 0.16, sig[1::2])]
    m = mcsas_amd.Sphere()
    m.radius.setActiveRange((LO, HI))
    setup = m.setup()
    contribs = np.random.RandomState(7).uniform(LO, HI, (N, 1, REPS))
    spec = dict(param_index=0, yweight="vol", edges=np.geomspace(LO, HI, BINS + 1), lower=LO, upper=HI)
    calls = dict(single_512q=lambda: engine.histogram_device(setup, q, I, sig, contribs, 0.6666666, [spec], device=0),
                 sets_per_set_2x256q=lambda: engine.histogram_sets(setup, sets, contribs, 0.6666666, [spec], device=0, scale="per_set"),
                 sets_shared_2x256q=lambda: engine.histogram_sets(setup, sets, contribs, 0.6666666, [spec], device=0, scale="shared"))
    for f in calls.values():
        f(); f()
    ms = {k: [] for k in calls}
    for _ in range(a.repeats):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            ms[k].append(1e3 * (time.perf_counter() - t0))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps(dict(shape=dict(nq=NQ, n_contrib=N, n_reps=REPS, bins=BINS), median_ms={k: round(v, 3) for k, v in med.items()},
                          min_ms={k: round(min(v), 3) for k, v in ms.items()}, max_ms={k: round(max(v), 3) for k, v in ms.items()},
                          per_set_over_single=round(med["sets_per_set_2x256q"] / med["single_512q"], 4),
                          shared_over_single=round(med["sets_shared_2x256q"] / med["single_512q"], 4))), flush=True)


if __name__ == "__main__":
    main()

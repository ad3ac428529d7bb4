"""What a trace costs: device time of a traced chain kernel against its untraced twin, from mcsas_hip_plan_last_ms.
Two shapes, both Sphere x 256 repetitions with a fixed budget of steps and the same seed: `wave`, 512 q x 400 contributions, one
wavefront per chain; `q-split`, 2048 q x 300 contributions in the workgroup mode (the q-split kernel, 8 q slots per lane, 4 waves).
The runs alternate untraced, traced, untraced, traced, each the median of 5 launches; the two untraced runs give the spread.  Prints
one JSON line.

    python tools/trace_cost.py [--shape wave|q-split] [--steps 20000] [--capacity 4096]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcsas_amd                                    # noqa: E402
from mcsas_amd import engine                        # noqa: E402
from bench import synthetic_data                    # noqa: E402


# name: q-points, contributions, execution mode
SHAPES = {"wave": (512, 400, engine.EXEC_WAVE), "q-split": (2048, 300, engine.EXEC_WORKGROUP)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="wave")
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=5)
    a = ap.parse_args()
    nq, n_contrib, mode = SHAPES[a.shape]
    q, I, sig = synthetic_data(nq)
    m = mcsas_amd.Sphere()
    m.radius.setActiveRange((2e-9, 3e-7))
    st = engine.Settings(n_contrib=n_contrib, n_reps=256, max_iter=a.steps, conv_crit=1e-9, max_retries=0, seed=1, exec_mode=mode)
    pl = engine.Plan(m.setup(), q, I, sig, st)
    runs = []
    try:
        info = pl.info
        pl.launch(); pl.fetch(want_arrays=False)                         # warm-up: code objects, row cache pages
        for k in range(4):
            traced = k % 2 == 1
            pl.set_trace(a.capacity if traced else 0)
            ms, moves = [], None
            for _ in range(a.launches):
                pl.launch()
                res = pl.fetch()
                ms.append(pl.last_ms)
                moves = res.num_moves
            runs.append(dict(traced=traced, ms=[round(x, 4) for x in ms], median_ms=round(float(np.median(ms)), 4),
                             steps=int(pl.total_steps), moves_per_chain_mean=float(moves.mean()), moves_per_chain_max=int(moves.max())))
    finally:
        pl.close()
    un = [r["median_ms"] for r in runs if not r["traced"]]
    tr = [r["median_ms"] for r in runs if r["traced"]]
    print(json.dumps(dict(shape="sphere %d q x %d contributions x 256 repetitions" % (nq, n_contrib), exec_mode=info["exec_mode"],
                          q_per_lane=info["q_per_lane"], waves_per_chain=info["waves_per_chain"], steps_per_chain=a.steps, capacity=a.capacity,
                          runs=runs, untraced_median_ms=round(float(np.median(un)), 4), traced_median_ms=round(float(np.median(tr)), 4),
                          untraced_spread_ms=round(abs(un[0] - un[1]), 4),
                          every_move_recorded=max(r["moves_per_chain_max"] for r in runs) <= a.capacity)))


if __name__ == "__main__":
    main()

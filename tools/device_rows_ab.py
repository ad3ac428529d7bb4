"""A Python model through host-evaluated rows against the same model in torch through device-evaluated rows: wall time per step.
Sphere typed as a Python model (numpy formfactor / volume: engine.analyse_host_rows calls calcIntensity once per parameter set) and
typed in torch (calcIntensityBatch: engine.analyse_device_rows fills the rows of a round in one call on the device); 100 q x 200
contributions x 10 repetitions, a fixed budget of steps with a criterion no chain reaches, window 64, same seed.  After a short
warm-up of both the runs alternate host, device, host, device ...; each pair of runs of one kind gives its spread.  The chains of
the two paths see the same uniform proposals, so their accepted moves are compared as a check that both did the same work.
Prints one JSON line.

    python tools/device_rows_ab.py [--steps 20000] [--repeats 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mcsas_amd                                    # noqa: E402
from mcsas_amd import engine                        # noqa: E402
from mcsas_amd.scatteringmodels import host_model_calc, batch_clip    # noqa: E402
from bench import synthetic_data                    # noqa: E402


class NumpySphere(mcsas_amd.SASModel):
    """models/sphere.py:12-63 as a user of the reference writes it."""
    parameters = mcsas_amd.Sphere.parameters

    def __init__(self):
        super().__init__()
        self.radius.setActive(True)

    def surface(self):
        return 4. * np.pi * self.radius() * self.radius()

    def volume(self):
        return (np.pi * 4. / 3.) * self.radius()**3

    def absVolume(self):
        return self.volume() * self.sld()**2

    def formfactor(self, dataset):
        qr = self.getQ(dataset) * self.radius()
        return 3. * (np.sin(qr) - qr * np.cos(qr)) / (qr**3.)


class TorchSphere(mcsas_amd.SASModel):
    """The same in torch: the batch form of calcIntensity."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--window", type=int, default=64)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("device_rows_ab: no GPU; this is a measurement and has no fall-back")
    q, I, sig = synthetic_data(100)
    data = mcsas_amd.SASData(q, I, sig)
    mn, mt = NumpySphere(), TorchSphere()
    for m in (mn, mt):
        m.radius.setActiveRange((2e-9, 3e-7))
    qd = torch.as_tensor(q, device="cuda")

    def host_rows(pset):
        return host_model_calc(mn, data, pset, 0.6666666, want_rows=True)[4]

    def device_rows(pset, out):
        out.copy_(mt.calcIntensityBatch(qd, batch_clip(mt, pset), 0.6666666)[0])

    def run(kind, steps):
        st = engine.Settings(n_contrib=200, n_reps=10, max_iter=steps, conv_crit=0.0, max_retries=0, seed=1)
        t0 = time.perf_counter()
        if kind == "host":
            res = engine.analyse_host_rows(mn.setup(data), q, I, sig, st, host_rows, window=a.window)
        else:
            res = engine.analyse_device_rows(mt.setup(data), q, I, sig, st, device_rows, window=a.window)
        dt = time.perf_counter() - t0          # (both calls return after the last device-to-host copy of the results)
        assert (res.num_iter == steps).all()
        return dt, res

    for kind in ("host", "device"):            # warm-up: code objects, torch's kernels and allocator, the library's memory cache
        run(kind, 10 * a.window)
    runs, moves = [], {}
    for _ in range(a.repeats):
        for kind in ("host", "device"):
            dt, res = run(kind, a.steps)
            moves[kind] = res.num_moves.copy()
            runs.append(dict(kind=kind, seconds=round(dt, 4), us_per_step=round(dt / (10 * a.steps) * 1e6, 4)))
    med = {k: float(np.median([r["us_per_step"] for r in runs if r["kind"] == k])) for k in ("host", "device")}
    spread = {k: float(np.ptp([r["us_per_step"] for r in runs if r["kind"] == k])) for k in ("host", "device")}
    print(json.dumps(dict(shape="sphere 100 q x 200 contributions x 10 repetitions", steps_per_chain=a.steps, window=a.window,
                          device=torch.cuda.get_device_name(0), runs=runs, host_us_per_step=round(med["host"], 4),
                          device_us_per_step=round(med["device"], 4), host_spread_us=round(spread["host"], 4),
                          device_spread_us=round(spread["device"], 4), host_over_device=round(med["host"] / med["device"], 2),
                          same_moves=bool((moves["host"] == moves["device"]).all()))))


if __name__ == "__main__":
    main()

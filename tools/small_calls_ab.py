"""Wall time of the small one-call entry points, one tree against another (the parent commit's against this one's): each process
imports mcsas_amd from --tree (a checkout with its library built), warms up and times, with the wall clock around calls that return
after their last device-to-host copy,
  - engine.histogram_device at the benchmark's shape (512 q x 400 contributions x 50 repetitions, one 50-bin histogram),
  - engine.histogram_device_batch of 8 such sets,
  - engine.histogram_device_rows at the shape of tools/hist_rows_ab.py (100 q x 200 x 10, four 50-bin histograms, a sphere in torch),
  - engine.model_calc for 400 rows x 512 q,
  - engine.histogram_prep, the call McSAS.histogram() makes, at the benchmark's shape,
  - engine.histogram_device at that shape with the range and bin curves of its histogram (partial=2),
  - engine.histogram_sets of that shape's points as two sets (256 + 256 q),
and prints one JSON line.  With --dump DIR every array of each call's result goes to DIR as well (one .npy each), for
tools/cmp_dumps.py to compare the trees' bits.  Run it in fresh processes alternating between the trees, then hand the lines to --md:

    for t in PARENT . PARENT .; do python tools/small_calls_ab.py --tree $t >> ab.jsonl; done
    python tools/small_calls_ab.py --md profiles/small_calls_refactor_ab.md ab.jsonl

A call counts as unchanged where the difference of the two trees' medians is no larger than the spread (max - min) of the first
tree's own repeats, and as faster where the second tree's median is lower by more than that."""
import argparse
import json
import os
import sys
import time

import numpy as np

CALLS = ("histogram_device", "histogram_device_batch x8", "histogram_device_rows", "model_calc", "histogram_prep", "histogram_device partial=2",
         "histogram_sets x2")


def arrays_of(x, name, out):
    """every numpy array in a call's result (tuples, lists and dicts of them), named by its place"""
    if isinstance(x, dict):
        for k in x:
            arrays_of(x[k], "%s.%s" % (name, k), out)
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            arrays_of(v, "%s.%d" % (name, i), out)
    elif x is not None:
        out[name] = np.asarray(x)
    return out


def measure(tree, repeats, warmup, dump=None):
    import torch                                    # (ahead of the library's first load: engine._one_hip_runtime)
    sys.path.insert(0, os.path.abspath(tree))
    import mcsas_amd
    from mcsas_amd import engine
    from mcsas_amd.scatteringmodels import setup_from_model
    assert os.path.dirname(os.path.dirname(os.path.abspath(mcsas_amd.__file__))) == os.path.abspath(tree), mcsas_amd.__file__
    if not torch.cuda.is_available():
        raise SystemExit("small_calls_ab: no GPU; this is a measurement and has no fall-back")
    sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import synthetic_data
    lo, hi = 2e-9, 3e-7
    m = mcsas_amd.Sphere()
    m.radius.setActive(True); m.radius.setActiveRange((lo, hi))
    rs = np.random.RandomState(7)

    def case(nq, n, reps, n_hist):
        q, I, sig = synthetic_data(nq)
        contribs = np.exp(rs.uniform(np.log(lo), np.log(hi), (n, 1, reps)))
        specs = [dict(param_index=0, yweight=w, edges=np.geomspace(lo, hi, 51), lower=lo, upper=hi) for w in ("vol", "num", "int", "surf")[:n_hist]]
        return setup_from_model(m, mcsas_amd.SASData(q, I, sig)), q, I, sig, contribs, specs

    setup, q, I, sig, contribs, specs = case(512, 400, 50, 1)
    item = dict(model=setup, q=q, intensity=I, sigma=sig, contribs=contribs, comp_exp=0.6666666, specs=specs)
    rsetup, rq, rI, rsig, rcontribs, rspecs = case(100, 200, 10, 4)
    pset = np.ascontiguousarray(contribs[:, :, 0])
    qdev = torch.as_tensor(rq, device="cuda")
    sld2 = float(m.sld()) ** 2

    def torch_sphere(p):                            # models/sphere.py:12-63 in torch, as tools/hist_rows_ab.py
        r = p[:, 0]
        vol = (np.pi * 4. / 3.) * r**3
        qr = qdev[None, :] * r[:, None]
        ff = 3. * (torch.sin(qr) - qr * torch.cos(qr)) / (qr**3)
        w = vol ** (2 * 0.6666666)
        return ff**2 * w[:, None], vol * sld2, w, 4. * np.pi * r * r

    calls = dict(zip(CALLS, (
        lambda: engine.histogram_device(**item),
        lambda: engine.histogram_device_batch([item] * 8),
        lambda: engine.histogram_device_rows(rsetup, rq, rI, rsig, rcontribs, rspecs, torch_sphere),
        lambda: engine.model_calc(setup, q, pset, 0.6666666, want_rows=True),
        lambda: engine.histogram_prep(setup, q, I, sig, contribs, 0.6666666),
        lambda: engine.histogram_device(**item, partial=[2]),
        lambda: engine.histogram_sets(setup, [(q[:256], I[:256], sig[:256]), (q[256:], I[256:], sig[256:])], contribs, 0.6666666, specs))))
    out = dict(tree=tree, device=torch.cuda.get_device_name(0), repeats=repeats, ms={})
    for name, call in calls.items():
        for _ in range(warmup):
            result = call()
        if dump:
            os.makedirs(dump, exist_ok=True)
            for k, a in arrays_of(result, name.replace(" ", "_"), {}).items():
                np.save(os.path.join(dump, k + ".npy"), a)
        t = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            t.append(1e3 * (time.perf_counter() - t0))
        out["ms"][name] = t
    print(json.dumps(out))


def table(md, files):
    runs = [json.loads(line) for f in files for line in open(f) if line.startswith("{")]
    trees = []
    for r in runs:
        if r["tree"] not in trees:
            trees.append(r["tree"])
    assert len(trees) == 2, trees
    names = dict(zip(trees, ("parent", "this tree")))
    with open(md, "w") as f:
        f.write("# The small one-call entry points: parent commit against this tree\n\n")
        f.write("`for t in PARENT . PARENT .; do python tools/small_calls_ab.py --tree $t >> ab.jsonl; done; python tools/small_calls_ab.py "
                "--md %s ab.jsonl` on one %s: %d fresh processes alternating between the trees, each a warm-up and %d timed repeats per "
                "call; wall time in ms around the call.  Spread = max - min of a tree's repeats over its processes.\n\n"
                % (md, runs[0]["device"], len(runs), runs[0]["repeats"]))
        f.write("| call | tree | median | min | max | spread | medians of the processes |\n|---|---|---|---|---|---|---|\n")
        verdicts = []
        for c in CALLS:
            med = {}
            for t in trees:
                per = [np.array(r["ms"][c]) for r in runs if r["tree"] == t]
                ms = np.concatenate(per)
                med[t] = (float(np.median(ms)), float(np.ptp(ms)))
                f.write("| `%s` | %s | %.3f | %.3f | %.3f | %.3f | %s |\n" % (c, names[t], np.median(ms), ms.min(), ms.max(), np.ptp(ms),
                                                                          " / ".join("%.3f" % np.median(p) for p in per)))
            d = med[trees[1]][0] - med[trees[0]][0]
            verdicts.append("`%s` %+.3f ms against a spread of %.3f ms: %s" % (c, d, med[trees[0]][1], "within" if abs(d) <= med[trees[0]][1] else ("faster" if d < 0 else "OUTSIDE")))
        f.write("\nDifference of the medians (this tree - parent) against the spread of the parent's own repeats: " + "; ".join(verdicts) + ".\n")
    print(open(md).read())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=None)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--md", default=None)
    ap.add_argument("--dump", default=None)
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    if a.md:
        table(a.md, a.files)
    else:
        measure(a.tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__))), a.repeats, a.warmup, a.dump)

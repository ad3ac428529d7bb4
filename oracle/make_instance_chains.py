#!/usr/bin/env python3
"""Kholodenko's chains of the instance matrix (tests/instance_cases.py), computed once by the numpy oracle on the CPU and stored as
its recorded outputs in tests/golden/instance_chains_kholodenko.npz.  The oracle's Kholodenko row is a QUADPACK integral per q-point
(0.6 ms): the ten shapes, two repetitions, a cold and a continued chain each, are about twenty minutes single-threaded, which no
test should spend.  Every other model's chains are computed live by the tests.

    python3 oracle/make_instance_chains.py [--jobs 16]            # writes the fixture from the seeds in instance_cases
    python3 oracle/make_instance_chains.py --search NQ [NQ ...]   # prints the figures of candidate seed pairs at those shapes

A row's points are independent integrals: the pool evaluates a row in chunks of q-points, which gives the single-process row bit for
bit (tests/test_instances_host.py recomputes the two smallest shapes without a pool and compares).  TEST INFRASTRUCTURE ONLY: numbers
from the project's own oracle, nothing else involved."""
import argparse
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import mcsas_oracle as O          # noqa: E402

_REAL_ROW = O.ff_kholodenko


def _chunk(args):
    return _REAL_ROW(*args)


def pooled_rows(pool, jobs):
    """O.ff_kholodenko with the q-points of a row dealt to the pool's processes."""
    def ff(q, radius, len_kuhn, len_contour):
        parts = np.array_split(np.asarray(q, dtype=float), min(4 * jobs, max(1, len(q) // 8)))
        return np.concatenate(pool.map(_chunk, [(part, radius, len_kuhn, len_contour) for part in parts]))
    return ff


def figures(both):
    cs = both["cold"] + both["cont"]
    return "margins %s lowest chi2 %s moves %s" % (["%.2e" % c["margin"] for c in cs], ["%.3g" % c["lowest"] for c in cs],
                                                   [c["ref"].num_moves for c in cs])


def acceptable(both):
    """The conditions tests/test_instances_host.py holds Kholodenko's chains to."""
    import instance_cases as IC
    from test_sets_host import KHOLODENKO_MARGIN
    cs = both["cold"] + both["cont"]
    return (all(c["margin"] >= KHOLODENKO_MARGIN and c["lowest"] >= 1.0 and IC.MIN_MOVES <= c["ref"].num_moves < IC.CAPACITY for c in cs)
            and all(not np.array_equal(both[k][0]["trace"]["step"], both[k][1]["trace"]["step"]) for k in ("cold", "cont")))


def main():
    import instance_cases as IC
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--search", type=int, nargs="+", metavar="NQ")
    ap.add_argument("--candidates", type=int, default=8)
    args = ap.parse_args()
    jobs = max(1, min(args.jobs, 16))
    with multiprocessing.Pool(jobs) as pool:
        O.ff_kholodenko = pooled_rows(pool, jobs)
        try:
            if args.search:
                for nq in args.search:
                    for k in range(args.candidates):
                        pair = (IC.DEFAULT_SEEDS[0] + 2 * k, IC.DEFAULT_SEEDS[1] + 2 * k)
                        both = IC.compute_chains("kholodenko", nq, pair)
                        good = acceptable(both)
                        print("kholodenko", nq, "seeds", pair, figures(both), "ok" if good else "-", flush=True)
                        if good:
                            break
                return
            by_nq = {}
            for nq in IC.KHOLODENKO_NQ:
                by_nq[nq] = IC.compute_chains("kholodenko", nq)
                print("kholodenko", nq, "seeds", IC.seeds("kholodenko", nq), figures(by_nq[nq]), "ok" if acceptable(by_nq[nq]) else "NOT ACCEPTABLE",
                      flush=True)
        finally:
            O.ff_kholodenko = _REAL_ROW
    np.savez_compressed(IC.FIXTURE, **IC.pack_chains(by_nq))
    print("wrote", IC.FIXTURE, os.path.getsize(IC.FIXTURE), "bytes")


if __name__ == "__main__":
    main()

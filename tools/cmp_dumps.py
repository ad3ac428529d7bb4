#!/usr/bin/env python3
"""tools/cmp_dumps.py a.npz b.npz ... : are the arrays of tools/time_c2.py's dumps identical to the first one's?
tools/cmp_dumps.py DIR_A DIR_B ... : the same for directories written by `bench.py --dump-outputs DIR` (one .npy per array);
exit status 1 if an array differs or is missing."""
import os, sys, numpy as np
if os.path.isdir(sys.argv[1]):
    names = sorted(f for f in os.listdir(sys.argv[1]) if f.endswith(".npy"))
    bad = 0
    for d in sys.argv[2:]:
        eq = {}
        for f in names:
            p = os.path.join(d, f)
            eq[f[:-4]] = os.path.exists(p) and bool(np.array_equal(np.load(os.path.join(sys.argv[1], f)), np.load(p)))
        extra = sorted(set(f for f in os.listdir(d) if f.endswith(".npy")) - set(names))
        bad += sum(not v for v in eq.values()) + len(extra)
        print(d, "%d arrays, %d equal" % (len(eq), sum(eq.values())), "DIFFERENT: %s" % [k for k, v in eq.items() if not v] if bad else "", "only there: %s" % extra if extra else "")
    sys.exit(1 if bad else 0)
a = np.load(sys.argv[1])
for f in sys.argv[2:]:
    b = np.load(f)
    print(f, {k: bool(np.array_equal(a[k], b[k])) for k in a.files}, "moves", int(b["moves"].sum()))

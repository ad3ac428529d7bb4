"""What the library decides without a device (csrc/host_decide.hip) as a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/plan_decisions_check.hip, compiled here together with that unit and run as a child process.
No GPU, nothing loaded into this process.  The recorded plan shapes (tests/golden/plan_shapes_mi355x.json) are replayed through
decide_shape with the recording's CU count; the free-memory gate of MCSAS_EXEC_AUTO, which no device of the library's own kind
exercises, is checked at its threshold; the family table, the trace block's layout and the tick budget against values worked
out by hand.  Of a joint fit of several sets (mcsas_hip_analyse_sets): where the sets lie in the padded vectors, the vectors and
each set's constants, its refusals; of every chain run the settings block of the kernels' arguments; of the wave and q-split instance
matrix (tests/instance_cases.py) the mode, slot count and wave count of every shape."""
import json
import os
import shutil
import subprocess

import pytest

from mcsas_amd import engine
from helpers import PLAN_SHAPE_CASES, PLAN_SHAPES_GOLDEN, make_models, plan_shape_problem

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mcsas_amd", "csrc")
# the rows that need the run-time compiler: they stay with tests/test_plan_lifecycle_gpu.py
PLUGIN_ROWS = {"plugin_auto", "plugin_wave", "no_plugin_wave_q1500"}
MODE_NAMES = {1: "wave", 2: "workgroup", 3: "pipeline"}


def build_check(tmp_path):
    """The check program, built; a function that runs it with arguments and standard input and returns what it printed."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "plan_decisions_check")
    # the Makefile's language flags; the sanitizers on the host side only, their runtimes inside the program (clang's default)
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                            "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result",
                            "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I" + CSRC,
                            "-o", exe, os.path.join(HERE, "plan_decisions_check.hip"), os.path.join(CSRC, "host_decide.hip")],
                           capture_output=True, text=True)
    if build.returncode and ("cannot find" in build.stderr or "unsupported" in build.stderr) and "san" in build.stderr:
        pytest.skip("the compiler has no sanitizer runtimes: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr

    def run(*args, text=""):
        r = subprocess.run([exe] + list(args), input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        return r.stdout
    return run


def problem_line(name, m, q, I, sig, st, smear=None):
    """The fields of the mcsas_problem that engine.HipProblem fills, as the line of text the check program reads."""
    p = engine.HipProblem(m.setup(), q, I, sig, st, smear=smear).c
    fields = [name, p.model_id, p.nq, p.n_contrib, p.n_reps, p.exec_mode, p.waves_per_chain, p.smear_nk, p.n_active]
    fields += [p.active_index[c] for c in range(p.n_active)] + [repr(float(x)) for x in p.params]
    return " ".join(str(f) for f in fields) + "\n"


def recorded_plan_shapes(check):
    """Every row of the recording but the three plug-in rows: mode, waves per chain, q slots per lane and window, or the refusal's
    code and message.  (`launches` and `cached_rows` come from the device.)"""
    rec = json.load(open(PLAN_SHAPES_GOLDEN))
    assert rec["cu_count"] == 256                                             # (what the check program hands decide_shape)
    cases = [c for c in PLAN_SHAPE_CASES if c[0] not in PLUGIN_ROWS]
    assert set(c[0] for c in cases) == set(rec["rows"]) - PLUGIN_ROWS and all(c[8] == "plugin" for c in PLAN_SHAPE_CASES if c[0] in PLUGIN_ROWS)
    out = check("shapes", text="".join(problem_line(c[0], *plan_shape_problem(c)) for c in cases))
    got = {}
    for line in out.splitlines():
        name, kind, rest = line.split(" ", 2)
        if kind == "shape":
            mode, waves, qpl, window = (int(x) for x in rest.split())
            got[name] = dict(exec_mode=MODE_NAMES[mode], waves_per_chain=waves, q_per_lane=qpl, window=window)
        else:
            code, msg = rest.split(" ", 1)
            got[name] = dict(error_code=int(code), error="libmcsas_hip error %d: %s" % (int(code), msg))
    assert set(got) == set(c[0] for c in cases)
    for name, row in got.items():
        want = {k: v for k, v in rec["rows"][name].items() if k not in ("launches", "cached_rows")}
        assert row == want, name


def free_memory_gate(check):
    """The case of test_auto_mode_never_picks_a_mode_whose_working_set_does_not_fit (9000 chains of 1000 core-shell ellipsoids on
    1024 q-points), which an MI355X with more than 290e9 bytes free skips: the pipeline just above twice its need, not at or below
    it, one wavefront per chain at 288 GiB, the pipeline when the free memory is not known."""
    from bench import synthetic_data
    q, I, sig = synthetic_data(1024)
    m, _ = make_models("ellcs", [1e-9, 2e-9, 2e-10], [1e-7, 2e-7, 1e-8])
    st = engine.Settings(n_contrib=1000, n_reps=9000, max_iter=10, conv_crit=0.0, max_retries=0, seed=1)
    out = check("gate", text=problem_line("gate", m, q, I, sig, st)).split()
    assert out[0] == "ok", out
    # twice the need lies above 288 GiB: at the card's own memory size the gate decides, as the GPU test's docstring says
    assert 2 * int(out[2]) > 288 * 2 ** 30, out


# set_nq -> slots per set, padded offsets, q slots per lane, end_mask: each set padded to whole slots of 64 entries, one after the
# other; qpl the next power of two that holds them; a bit of end_mask for every set's last slot
SETS_LAYOUTS = [
    ((3,), (1,), (0,), 1, 0x1),
    ((64,), (1,), (0,), 1, 0x1),
    ((65,), (2,), (0,), 2, 0x2),
    ((37, 100), (1, 2), (0, 64), 4, 0x5),
    ((64, 3, 63, 130), (1, 1, 1, 3), (0, 64, 128, 192), 8, 0x27),
    ((193, 193, 193, 193), (4, 4, 4, 4), (0, 256, 512, 768), 16, 0x8888),
]
# (nq, set_nq) -> words of the refusal
SETS_SHAPE_REFUSALS = [
    (836, (257, 193, 193, 193), ("17 padded slots", "1024")),
    (90, (88, 2), ("set 1 has 2 points", "at least 3")),
    (90, (40, 49), ("sum of set_nq 89 != nq 90",)),
]


def sets_layouts(check):
    """Where the sets of a joint fit lie (host_decide.hip: check_sets_request); the LDS need is checked by the program against the
    rule restated there."""
    lines = ["L%d %d %d %s\n" % (i, sum(nqs), len(nqs), " ".join(map(str, nqs))) for i, (nqs, *_) in enumerate(SETS_LAYOUTS)]
    lines += ["R%d %d %d %s\n" % (i, nq, len(nqs), " ".join(map(str, nqs))) for i, (nq, nqs, _) in enumerate(SETS_SHAPE_REFUSALS)]
    out = dict(line.split(" ", 1) for line in check("sets", text="".join(lines)).splitlines())
    assert len(out) == len(lines)
    for i, (nqs, slots, pad_off, qpl, end_mask) in enumerate(SETS_LAYOUTS):
        kind, total, got_qpl, got_mask, *per_set = out["L%d" % i].split()
        assert kind == "layout" and (int(total), int(got_qpl), int(got_mask, 16)) == (sum(slots), qpl, end_mask), (nqs, out["L%d" % i])
        assert tuple(int(x) for x in per_set[0::2]) == slots and tuple(int(x) for x in per_set[1::2]) == pad_off, (nqs, per_set)
    for i, (nq, nqs, words) in enumerate(SETS_SHAPE_REFUSALS):
        kind, code, msg = out["R%d" % i].split(" ", 2)
        assert kind == "error" and int(code) == -1 and msg.startswith("analyse_sets:") and all(w in msg for w in words), (nqs, msg)


def generated_sets_layouts(check):
    """Every generated input of the joint fit's GPU tests (sets_exact.GENERATED: the instance matrix, the chain text's edges) selects
    the slot count its name says, uses that instance's last slot, and ends its last set there or one slot before a padding slot."""
    import sets_exact as SX
    shapes = {name: SX.generated_shape(name) for name in SX.GENERATED}
    assert sorted({(tag, qpl) for tag, _, qpl in (shapes[n] for n in SX.MATRIX)}) == sorted((t, q) for t in SX.MATRIX_MODELS for q in (1, 2, 4, 8, 16))
    lines = ["%s %d %d %s\n" % (name, sum(nqs), len(nqs), " ".join(map(str, nqs))) for name, (_, nqs, _) in shapes.items()]
    out = dict(line.split(" ", 1) for line in check("sets", text="".join(lines)).splitlines())
    assert len(out) == len(lines)
    for name, (tag, nqs, qpl) in shapes.items():
        kind, total, got_qpl, got_mask, *per_set = out[name].split()
        print(name, nqs, "slots", total, "qpl", got_qpl, "end_mask", got_mask)
        assert kind == "layout" and int(got_qpl) == qpl and qpl // 2 < int(total) <= qpl, (name, out[name])
        assert bin(int(got_mask, 16)).count("1") == len(nqs) and int(got_mask, 16) >> (int(total) - 1) == 1, (name, got_mask)
    full = out[SX.matrix_name("sphere", 16)].split()
    assert (int(full[1]), int(full[3], 16) >> 15) == (16, 1)                  # bit 15 of end_mask, no padding slot


def instance_matrix_shapes(check):
    """Every shape of the wave and q-split instance matrix (tests/instance_cases.py; tests/test_instances_gpu.py) selects the mode, the
    slot count and the wave count its name says.  (The row cache is the device's: Plan.info confirms it there.)"""
    import instance_cases as IC
    want, lines = {}, []
    for tag, qpl, cache in IC.WAVE:
        name, nq = "wave_%s_q%d_c%d" % (tag, qpl, cache), IC.wave_nq(qpl)
        want[name] = ("wave", 1, qpl)
        lines.append(problem_line(name, IC.models(tag)[0], *IC.data(nq), IC.engine_settings(tag, nq, engine.EXEC_WAVE, cache)))
    for tag, qpl, shape in IC.WIDE:
        name, (nq, waves) = "wide_%s_q%d_%s" % (tag, qpl, shape), IC.WIDE_SHAPES[qpl][shape]
        want[name] = ("workgroup", waves, qpl)
        lines.append(problem_line(name, IC.models(tag)[0], *IC.data(nq), IC.engine_settings(tag, nq, engine.EXEC_WORKGROUP)))
    assert len(want) == len(lines) == 96 + 45
    got = {}
    for line in check("shapes", text="".join(lines)).splitlines():
        name, kind, rest = line.split(" ", 2)
        assert kind == "shape", line
        mode, waves, got_qpl, _ = (int(x) for x in rest.split())
        got[name] = (MODE_NAMES[mode], waves, got_qpl)
        print(name, "->", *got[name])
    assert got == want, sorted(n for n in want if got.get(n) != want[n])


def sets_refusals(check):
    """Every row of test_sets_host.REFUSALS through the function that makes them, in the stand-alone program: the same words."""
    from test_sets_host import REFUSALS, _request
    lines = []
    for what in sorted(REFUSALS):
        st_kw, spoil, _ = REFUSALS[what]
        prob = _request(**st_kw)[0]
        if spoil:
            spoil(prob)
        c = prob.c
        lines.append("%s %d %d %d %d %d %d %d\n" % (what, c.model_id, c.n_active, c.n_devices, c.positive_background, c.smear_nk,
                                                    c.cache_intensities, c.exec_mode))
    lines.append("valid %d 1 0 0 0 -1 0\n" % engine.MODEL_SPHERE)
    out = dict(line.split(" ", 1) for line in check("refusals", text="".join(lines)).splitlines())
    assert len(out) == len(REFUSALS) + 1 and out["valid"].strip() == "0"
    for what, (_, _, words) in REFUSALS.items():
        code, msg = out[what].split(" ", 1)
        assert int(code) == -1 and words in msg and msg.startswith("analyse_sets:"), (what, msg)


def test_plan_decisions_without_a_device(tmp_path):
    check = build_check(tmp_path)
    # the family table, the trace block's layout and transposition, the tick budget; the settings block of a chain run; the padded
    # vectors and constants of (37, 100) points in two sets, and of 65 in one against the single-set sums
    assert check().strip() == "ok"
    sets_layouts(check)
    generated_sets_layouts(check)
    instance_matrix_shapes(check)
    sets_refusals(check)
    recorded_plan_shapes(check)
    free_memory_gate(check)

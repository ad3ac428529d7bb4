"""The producer blocks' LDS as pipe_geometry (csrc/pipe_layout.h) lays it out, against values worked out by hand: the roles of the
Gram phase (csrc/pipe_gram.h: waves 0-3 on the MFMAs, waves 4-7 on a row of the next sub-window held in REGISTERS) take no LDS of
their own — a second row buffer would not fit beside the 150 KB in use.  tests/pipe_geometry_check.hip, compiled here and run as a
child process; no GPU.

qpad = 64 * (q per lane); tables q, w, wI, 1/q^3: 4 qpad doubles (the sphere has no table of its own) = gram_off; 16 doubles of
counters; the reduction buffer, 8 waves x 2 tiles x 256 doubles; the row buffer, W rows of qpad + 8; the block's proposal records,
8 * (rows per wave) of 12 doubles."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mcsas_amd", "csrc")

RED = 8 * 2 * 256
# (q-points, contributions, chains): window, W, rows per wave, blocks per chain, sub-windows per block, qpad
SHAPES = {
    (512, 400, 50): (192, 24, 6, 4, 2, 512),         # the headline workload (bench.py, config 2)
    (512, 100, 86): (48, 24, 6, 1, 2, 512),          # tests/test_pipe_gram_roles.py: a row held across a Gram phase
    (512, 100, 4): (48, 24, 3, 2, 1, 512),           # two blocks of one sub-window
    (64, 100, 3): (48, 48, 6, 1, 1, 64),             # one q per lane
}


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("geom") / "pipe_geometry_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function",
                            "-I" + CSRC, "-I" + os.path.join(HERE, "..", "include"), "-o", exe, os.path.join(HERE, "pipe_geometry_check.hip")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr

    def run(nq, n, chains):
        r = subprocess.run([exe, str(nq), str(n), str(chains)], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr)
        return [int(x) for x in r.stdout.split()]
    return run


@pytest.mark.parametrize("shape", list(SHAPES))
def test_producer_lds_is_what_it_was_before_the_gram_roles(check, shape):
    kb, w, rpw, by, nsb, qpad = SHAPES[shape]
    rc, g_kb, g_w, g_rpw, g_by, g_nsb, gram_lds, lazy, gram_off, drow_off, rec_off, prod_lds = check(*shape)
    assert (rc, g_kb, g_w, g_rpw, g_by, g_nsb, gram_lds, lazy) == (0, kb, w, rpw, by, nsb, 1, 1)
    assert gram_off == 4 * qpad
    assert drow_off == gram_off + 16 + RED
    assert rec_off == drow_off + w * (qpad + 8)
    assert prod_lds == 8 * (rec_off + 8 * rpw * 12)
    assert prod_lds <= 160 * 1024


def test_the_headline_workload_uses_150_kb_and_has_no_room_for_a_second_row_buffer(check):
    prod_lds = check(512, 400, 50)[-1]
    assert prod_lds == 153728
    assert prod_lds + 8 * 24 * (512 + 8) > 160 * 1024

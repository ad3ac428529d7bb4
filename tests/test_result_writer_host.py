"""The one writer of a mcsas_result (csrc/host_result.h) as a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/result_writer_check.cpp, compiled and run here.  No GPU, no HIP runtime, nothing loaded into
this process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_result_writer_whole_and_in_blocks_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "result_writer_check")
    # the sanitizers' runtimes inside the program (clang's default; gcc: -static-libasan): it then runs whatever else the
    # environment has the loader bring in ahead of it
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all"] + static + ["-o", exe, os.path.join(HERE, "result_writer_check.cpp")],
                           capture_output=True, text=True)
    if build.returncode and ("cannot find" in build.stderr or "unsupported" in build.stderr) and "san" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtimes: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)


def test_the_writer_header_keeps_hip_out():
    """host_result.h is compiled above without a HIP runtime: it includes the public header and the standard library only; and the
    four places that fill a result go through it, with no copy of the field list left beside it."""
    csrc = os.path.join(HERE, "..", "mcsas_amd", "csrc")
    text = open(os.path.join(csrc, "host_result.h")).read()
    assert "hip_runtime" not in text and "host_internal.h" not in text
    for unit in ("mcsas_hip.hip", "host_analyse.hip", "host_rows.hip"):
        code = open(os.path.join(csrc, unit)).read()
        assert '#include "host_result.h"' in code and "result_put_row(" in code, unit
        assert "res->scaling" not in code and "res->num_moves" not in code, unit

"""The tile-fill record of the result sinks (csrc/mk_tilefill.hpp) on the host: tests/tilefill_test.cpp, which
includes that header alone, built with the host C++ compiler under the address and undefined-behaviour
sanitizers and run as a program of its own.  It checks the tile counts (ragged last tile, one tile, one
site), the first missing tile as tiles are marked, that another kept window forgets or outdates every tile,
and that the missing-tile messages of the scores, maps and pairs are the strings their entry points used to
build by hand."""
import os
import shutil
import subprocess

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd",
                    "csrc")


def test_tilefill_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++, c++ or clang++) to build tilefill_test.cpp with")
    exe = str(tmp_path / "tilefill_test")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(TESTS, "tilefill_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr

"""CPU side of the areal prediction (include/mk.h "areal prediction").  The region spec's checks and layout
(csrc/mk_regionspec.hpp) on the host: tests/regionspec_test.cpp, which includes that header alone, built
with the host C++ compiler under the address and undefined-behaviour sanitizers and run as a program of its
own -- every refusal and the index it names, the normalised weights, the packed factor offsets.  And the
binding against the header: structs field for field, argument counts, the constants, the Python buffers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CSRC = os.path.join(ROOT, "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "mk.h")


def test_regionspec_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++, c++ or clang++) to build regionspec_test.cpp with")
    exe = str(tmp_path / "regionspec_test")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(TESTS, "regionspec_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def test_regionspec_header_uses_standard_headers_only():
    src = open(os.path.join(CSRC, "mk_regionspec.hpp")).read()
    inc = re.findall(r"#include\s+(\S+)", src)
    assert inc and all(i.startswith("<") and not i.startswith("<hip") for i in inc), inc


def test_region_structs_and_entry_points_match_header(mk):
    binding = __import__(mk.__name__ + "._lib", fromlist=["x"])
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for cname, py, want in (("mk_region_spec", binding.RegionSpec, ["n_regions", "offsets", "weights", "n_thresholds", "thresholds"]),
                            ("mk_regions", binding.Regions, ["region_predict", "planes", "region_samples", "singular",
                                                             "timing_ms"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        fields = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*;", body)
        assert fields == [f[0] for f in py._fields_] == want
    assert int(re.search(r"#define MK_REGION_MAXM (\d+)", src).group(1)) == binding.REGION_MAXM == 128
    assert float(re.search(r"#define MK_REGION_PIVOT_TOL (\S+)", src).group(1)) == 1e-12
    hpp = open(os.path.join(CSRC, "mk_regionspec.hpp")).read()
    assert int(re.search(r"REGION_MAXM = (\d+)", hpp).group(1)) == 128
    assert int(re.search(r"REGION_MAXT = (\d+)", hpp).group(1)) == binding.MAP_MAXT
    lib = mk.load()
    for name in ("mk_session_set_regions", "mk_session_regions"):
        decl = re.search(r"\bint %s\((.*?)\);" % name, src, flags=re.S)
        assert decl, name
        assert decl.group(1).count(",") + 1 == 2 == len(binding.EXPORTS[name][1]), name
        assert hasattr(lib, name)
    assert mk.session.KS_REGIONS == 19 and mk.session.KS_PAIRS == 18
    outbuf = __import__(mk.__name__ + ".outbuf", fromlist=["x"])
    assert outbuf.region_names(2) == ["mean", "sd", "exc_1", "exc_2"]
    rb = outbuf.RegionBuffers(2, 3, 4, 1, 20, samples=True)
    assert rb.region_predict.shape == (2, 12, 200) and rb.planes.shape == (2, 3, 12)
    assert rb.region_samples.shape == (2, 20, 12) and rb.singular.shape == (2, 12) and rb.singular.dtype == np.int32
    got = rb.unpack((0.2,))
    assert got["region_predict"][1].shape == (200, 12) and got["subsets"][0].shape == (12, 3)
    assert got["region_samples"][0].shape == (12, 20) and got["thresholds"] == [0.2] and got["timing_ms"].shape == (3,)
    off, w, u, m = outbuf.region_spec([0, 2, 5], 5, [1, 1, 2, 2, 2], (0.3,))
    assert m.n_regions == 2 and m.n_thresholds == 1 and off.dtype == np.int32 and w.tolist() == [1.0, 1.0, 2.0, 2.0, 2.0]
    with pytest.raises(ValueError):
        outbuf.region_spec([0, 2, 5], 5, [1, 1, 2])               # a weight per site
    with pytest.raises(ValueError):
        outbuf.region_spec([0], 5)
    assert callable(mk.spRegions) and callable(mk.combine_regions)
    assert mk.combine_regions([{"parameters": None}]) is None     # subsets fitted without regions


def test_regions_fail_loudly_without_a_session(mk):
    lib = mk.load()
    binding = __import__(mk.__name__ + "._lib", fromlist=["x"])
    sp, rg = binding.RegionSpec(), binding.Regions()
    assert lib.mk_session_set_regions(None, ctypes.byref(sp)) == binding.MK_E_ARG
    assert lib.mk_session_set_regions(None, None) == binding.MK_E_ARG
    assert lib.mk_session_regions(None, ctypes.byref(rg)) == binding.MK_E_ARG
    assert b"null session" in lib.mk_last_error()

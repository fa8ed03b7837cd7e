"""CPU side of the empirical variogram (include/mk.h "empirical variogram").  Every refusal of
mk_variogram_compute through the loaded library, made before any device is touched, with the index it names;
the exponential fit and the phi suggestion (host code); the binding against the header; and the spec's
checks and tile schedule (csrc/mk_variogramspec.hpp) by tests/variogramspec_test.cpp, which includes that
header alone, built with the host C++ compiler under the address and undefined-behaviour sanitizers and run
as a program of its own."""
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


def test_variogramspec_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++, c++ or clang++) to build variogramspec_test.cpp with")
    exe = str(tmp_path / "variogramspec_test")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(TESTS, "variogramspec_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def test_variogramspec_header_uses_standard_headers_only():
    src = open(os.path.join(CSRC, "mk_variogramspec.hpp")).read()
    inc = re.findall(r"#include\s+(\S+)", src)
    assert inc and all(i.startswith("<") and not i.startswith("<hip") for i in inc), inc


def _binding(mk):
    return __import__(mk.__name__ + "._lib", fromlist=["x"])


def test_variogram_struct_and_entry_point_match_header(mk):
    binding = _binding(mk)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct mk_variogram \{(.*?)\} mk_variogram;", src, flags=re.S).group(1)
    fields = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*;", body)
    assert fields == [f[0] for f in binding.Variogram._fields_] == ["count", "dist", "gamma", "ms"]
    hpp = open(os.path.join(CSRC, "mk_variogramspec.hpp")).read()
    assert int(re.search(r"#define MK_VG_MAXBINS (\d+)", src).group(1)) == binding.VG_MAXBINS == 64
    assert int(re.search(r"VG_MAXBINS = (\d+)", hpp).group(1)) == 64
    assert int(re.search(r"#define MK_VG_MAXQ (\d+)", src).group(1)) == binding.VG_MAXQ == 4
    assert int(re.search(r"VG_MAXQ = (\d+)", hpp).group(1)) == 4
    decl = re.search(r"\bint mk_variogram_compute\((.*?)\);", src, flags=re.S)
    assert decl.group(1).count(",") + 1 == 8 == len(binding.EXPORTS["mk_variogram_compute"][1])
    lib = mk.load()
    edge = int(re.search(r"#define MK_VG_EDGE (\d+)", src).group(1))
    assert lib.mk_variogram_tile_edge() == edge == int(re.search(r"VG_EDGE = (\d+)", hpp).group(1))
    vg = __import__(mk.__name__ + ".variogram", fromlist=["x"])
    assert vg.tile_edge() == edge
    assert vg.outcome_pairs(3) == [(0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2)]
    for name in ("variogram", "glm_residuals", "fit_exponential", "suggest_phi", "residual_variogram"):
        assert callable(getattr(mk, name)), name


def _call(mk, coords, n, z, q, n_bins, max_dist, null=()):
    """mk_variogram_compute on device 0 with caller-side buffers; null: names of pointers to pass as NULL."""
    binding = _binding(mk)
    lib = mk.load()
    T = max(q * (q + 1) // 2, 1)
    nb = min(max(n_bins, 1), 64)
    count, dist, gamma = np.zeros(nb, dtype=np.int64), np.zeros(nb), np.zeros(T * nb)
    out = binding.Variogram(None if "count" in null else count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                            None if "dist" in null else binding.dptr(dist),
                            None if "gamma" in null else binding.dptr(gamma), 0.0)
    rc = lib.mk_variogram_compute(None if "coords" in null else binding.dptr(coords), n,
                                  None if "z" in null else binding.dptr(z), q, n_bins, max_dist,
                                  None if "out" in null else ctypes.byref(out), 0)
    return rc, lib.mk_last_error().decode()


def test_every_refusal_is_made_on_the_host_and_names_the_index(mk):
    binding = _binding(mk)
    coords = np.array([0.0, 1.0, 2.0, 0.0, 0.5, 1.0])            # 3 sites, column-major
    z = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])

    def refused(what, *args, **kw):
        rc, msg = _call(mk, *args, **kw)
        assert rc == binding.MK_E_ARG and what in msg, (rc, msg)

    for name in ("coords", "z", "count", "dist", "gamma", "out"):
        refused("null", coords, 3, z, 1, 4, 1.0, null=(name,))
    refused("n = 1 sites", coords, 1, z, 1, 4, 1.0)
    refused("n = 0 sites", coords, 0, z, 1, 4, 1.0)
    refused("n = -3 sites", coords, -3, z, 1, 4, 1.0)
    refused("q = 0 is outside 1 .. 4", coords, 3, z, 0, 4, 1.0)
    refused("q = 5 is outside 1 .. 4", coords, 3, z, 5, 4, 1.0)
    refused("n_bins = 0 is outside 1 .. 64", coords, 3, z, 1, 0, 1.0)
    refused("n_bins = 65 is outside 1 .. 64", coords, 3, z, 1, 65, 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("max_dist = ", coords, 3, z, 1, 4, bad)
    for bad in (float("nan"), float("inf"), float("-inf")):
        c = coords.copy()
        c[4] = bad
        c[5] = bad                                               # the first of two is named
        refused("coordinate 4 (site 1, column 1)", c, 3, z, 2, 4, 1.0)
        v = z.copy()
        v[3] = bad
        refused("z value 3 (site 1, outcome 1)", coords, 3, v, 2, 4, 1.0)
        refused("z value 3 (site 3, outcome 0)", np.zeros(12), 6, v, 1, 4, 1.0)
        c = coords.copy()
        c[0] = bad                                               # a bad coordinate is found before a bad z
        refused("coordinate 0 (site 0, column 0)", c, 3, v, 2, 4, 1.0)
    with pytest.raises(mk.MkError, match="z value 1 "):
        mk.variogram(np.zeros((3, 2)), [0.0, float("nan"), 0.0], n_bins=4, max_dist=1.0)
    with pytest.raises(ValueError):
        mk.variogram(np.zeros((3, 3)), np.zeros(3))


def _exact_vg(phi, nugget, psill, n_bins=15, max_dist=0.6):
    edges = np.arange(n_bins + 1) * (max_dist / n_bins)
    h = 0.5 * (edges[:-1] + edges[1:])
    gamma = nugget + psill * -np.expm1(-phi * h)
    return {"h": h, "count": np.arange(1, n_bins + 1) * 1000, "gamma": gamma[None, :], "pairs": [(0, 0)], "edges": edges,
            "max_dist": max_dist, "n_bins": n_bins}


@pytest.mark.parametrize("phi,nugget,psill", [(6.0, 0.1, 0.9), (3.0, 0.0, 1.0), (20.0, 0.3, 0.5), (11.7, 0.05, 2.0)])
def test_fit_exponential_recovers_an_exact_variogram(mk, phi, nugget, psill):
    """An exact exponential variogram: the sse is zero at the truth and quadratic about it, so the golden
    section (on log phi, inside one cell of the 512-value grid) places the minimiser to about sqrt(2^-52) =
    1.5e-8 relative; 1e-6 leaves room for the conditioning of (c0, c, phi) on 15 bins."""
    f = mk.fit_exponential(_exact_vg(phi, nugget, psill))
    assert abs(f["phi"] / phi - 1.0) < 1e-6, f
    assert abs(f["nugget"] - nugget) < 1e-6 and abs(f["psill"] - psill) < 1e-6, f
    assert f["range"] == 3.0 / f["phi"] and f["sse"] < 1e-12


def test_fit_exponential_needs_bins_and_skips_empty_ones(mk):
    vg = _exact_vg(6.0, 0.1, 0.9)
    vg["count"] = vg["count"].copy()
    vg["count"][[0, 7]] = 0
    vg["gamma"] = vg["gamma"].copy()
    vg["gamma"][0, [0, 7]] = np.nan
    assert abs(mk.fit_exponential(vg)["phi"] / 6.0 - 1.0) < 1e-6
    vg["count"][2:] = 0
    with pytest.raises(ValueError):
        mk.fit_exponential(vg)


def test_suggest_phi_gives_the_reference_ratios(mk):
    """MK.R:60-63: phi = 3/0.5 and Unif(3/0.75, 3/0.25) are suggest_phi's answer at a fitted range of 0.5."""
    s = mk.suggest_phi(None, fits=[{"phi": 6.0, "range": 0.5}])
    assert s["starting"].tolist() == [6.0] and s["unif"][0].tolist() == [4.0] and s["unif"][1].tolist() == [12.0]
    cfg = mk.SamplerConfig(1, 2, [0.0, 0.0], [0.1, 0.1])
    assert cfg.phi_starting.tolist() == s["starting"].tolist()
    assert cfg.phi_a.tolist() == s["unif"][0].tolist() and cfg.phi_b.tolist() == s["unif"][1].tolist()
    # from a variogram: one fit per outcome, off the direct planes (a, a)
    one, two = _exact_vg(6.0, 0.1, 0.9), _exact_vg(12.0, 0.2, 0.4)
    vg = dict(one, gamma=np.vstack([one["gamma"], 0.5 * (one["gamma"] + two["gamma"]), two["gamma"]]),
              pairs=[(0, 0), (1, 0), (1, 1)])
    s = mk.suggest_phi(vg)
    assert np.allclose(s["starting"], [6.0, 12.0], rtol=1e-6)
    assert np.allclose(s["unif"][0], [4.0, 8.0], rtol=1e-6) and np.allclose(s["unif"][1], [12.0, 24.0], rtol=1e-6)
    cfg = mk.SamplerConfig(2, 2, [0.0, 0.0], [0.1, 0.1], phi_starting=s["starting"], phi_unif=s["unif"])
    assert np.allclose(cfg.phi_a, [4.0, 8.0], rtol=1e-6)


def test_pearson_residuals_and_unobserved_sites(mk):
    vg = __import__(mk.__name__ + ".variogram", fromlist=["x"])
    r = vg.pearson_residuals([1.0, 0.0, 3.0, 0.0], [1.0, 1.0, 4.0, 0.0], [0.5, 0.2, 0.5, 0.3])
    assert r[:3].tolist() == [1.0, -0.2 / np.sqrt(0.2 * 0.8), 1.0] and np.isnan(r[3])

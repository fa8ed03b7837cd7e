"""The variogram reference (tests/variogram_ref.py) against answers worked by hand: three collinear points,
and the 8 x 8 lattice whose arithmetic is exact in fp64, so the half-open bins are fixed without tolerance.
CPU only; no library."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import variogram_ref as vr  # noqa: E402

LATTICE_COUNTS = [0, 210, 336, 340, 322, 376, 224, 162, 36, 10]


def test_three_collinear_points():
    # sites at 0, 1, 3 on a line, z = 1, 2, 4: distances 1 (sites 0, 1), 2 (1, 2), 3 (0, 2)
    coords = np.array([[0.0, 0.0], [1.0, 0.0], [3.0, 0.0]])
    z = np.array([1.0, 2.0, 4.0])
    r = vr.variogram(coords, z, 4, 4.0)                  # s = 1: bins [0,1) [1,2) [2,3) [3,4)
    assert r["count"] == [0, 1, 1, 1] and r["n_in"] == 3
    assert r["sum_d"].tolist() == [0.0, 1.0, 2.0, 3.0]
    assert r["sum_zz"][0].tolist() == [0.0, 1.0, 4.0, 9.0]
    assert np.isnan(r["gamma"][0, 0]) and np.isnan(r["dist"][0])
    assert r["gamma"][0, 1:].tolist() == [0.5, 2.0, 4.5] and r["dist"][1:].tolist() == [1.0, 2.0, 3.0]
    # max_dist = 3 with three bins: d = 3 is on the outer edge and half-open bins leave it out
    r = vr.variogram(coords, z, 3, 3.0)
    assert r["count"] == [0, 1, 1] and r["n_in"] == 2
    # two outcomes, the second the negative of the first: the cross-variogram is minus the direct one
    r = vr.variogram(coords, np.column_stack([z, -z]), 4, 4.0)
    assert r["pairs"] == [(0, 0), (1, 0), (1, 1)]
    assert r["gamma"][1, 1:].tolist() == [-0.5, -2.0, -4.5] and r["gamma"][2, 1:].tolist() == [0.5, 2.0, 4.5]
    # a coincident pair falls in bin 0
    r = vr.variogram(np.array([[0.5, 0.5], [0.5, 0.5], [0.5, 1.0]]), z, 2, 1.0)
    assert r["count"] == [1, 2] and r["sum_zz"][0].tolist() == [1.0, 13.0] and r["sum_d"].tolist() == [0.0, 1.0]


def test_lattice_counts_and_edges_in_integers():
    coords, ix, iy = vr.lattice(8)
    z = (ix + 2 * iy).astype(np.float64)
    r = vr.variogram(coords, z, 10, 1.25)                # s = 8: d s = sqrt(di^2 + dj^2)
    assert r["count"] == LATTICE_COUNTS and r["n_in"] == 2016 == 64 * 63 // 2
    # the same in integers: k = isqrt(di^2 + dj^2); a pair is on an edge when that is a perfect square
    count, on_edge = [0] * 10, 0
    szz, sd = [0] * 10, [0.0] * 10
    for a in range(64):
        for b in range(a + 1, 64):
            m2 = int(ix[a] - ix[b]) ** 2 + int(iy[a] - iy[b]) ** 2
            k = math.isqrt(m2)
            on_edge += k * k == m2
            count[k] += 1
            szz[k] += int(z[a] - z[b]) ** 2
            sd[k] += math.sqrt(m2) / 8.0
    assert count == LATTICE_COUNTS and on_edge == 528
    assert r["sum_zz"][0].tolist() == [float(v) for v in szz]
    assert np.allclose(r["sum_d"], sd, rtol=1e-14, atol=0)
    assert r["edge_gap"] == 0.0                          # 3-4-5 triangles and the axes: d s is an integer
    # max_dist below the spacing: nothing is counted
    r = vr.variogram(coords, z, 5, 0.1)
    assert r["count"] == [0] * 5 and r["n_in"] == 0 and np.isnan(r["gamma"]).all() and np.isnan(r["dist"]).all()

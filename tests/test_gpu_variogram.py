"""mk_variogram_compute on the device against the longdouble reference (tests/variogram_ref.py).

Per case: the counts equal the reference's exactly and add up to its number of pairs with d s < n_bins; every
sum (of d, and of the products recovered as gamma 2 N) lies within (N_k + 8) 2^-52 sum|term| of the
reference's -- the worst case of any fixed-order fp64 sum of N_k rounded terms (each term carries at most
three roundings, 1.5 x 2^-52 of itself; the N_k - 1 additions at most 2^-53 of a partial sum each, which
sum|term| bounds; the division by N_k and the product that undoes it two more), derived and not tuned.

A device d can differ from the reference's by an ulp, so a pair within an ulp of a bin edge could change
bins: every case with random coordinates first asserts, on the reference alone, that no pair with d > 0 has
|d s - round(d s)| < 1e-9 (d = 0 is exact on both sides and belongs to bin 0).  The lattice sits on the edges
on purpose: its arithmetic is exact in fp64 on both sides.

The sizes are the smallest at which the kernel can go wrong: n = 2, the tile edge E - 1, E, E + 1 (the
diagonal mask, one ragged row and column) and 2 E + 1 (off-diagonal tiles, several workgroups); the bin
counts on both sides of every change of launch shape (one pass | split: 31 | 32 bins at q = 1, 17 | 18 at
q = 2, 10 | 11 at q = 3, 6 | 7 at q = 4; 64 bins: the split's counting pass on 128 lanes)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import variogram_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu
EDGE_GAP = 1e-9
SEED = 20250114


@functools.lru_cache(maxsize=None)
def _data(kind, n, q, seed=SEED):
    """uniform / clustered (20 centres, sigma 1e-3) sites on the unit square with N(0, 1) values; 'dup'
    appends copies of the first 10 sites with values of their own, so that d = 0 occurs."""
    rng = np.random.default_rng(seed)
    base = kind.split("+")[0]
    if base == "uniform":
        coords = rng.uniform(size=(n, 2))
    else:
        centres = rng.uniform(size=(20, 2))
        coords = centres[rng.integers(20, size=n)] + 1e-3 * rng.normal(size=(n, 2))
    z = rng.normal(size=(n, q))
    if kind.endswith("+dup"):
        coords = np.vstack([coords, coords[:10]])
        z = np.vstack([z, rng.normal(size=(10, q))])
    coords.setflags(write=False)
    z.setflags(write=False)
    return coords, z


@functools.lru_cache(maxsize=None)
def _ref(kind, n, q, n_bins, max_dist):
    if kind == "lattice":
        coords, ix, iy = vr.lattice(8)
        z = np.column_stack([ix + 2.0 * iy, (ix * iy) % 3 - 1.0])[:, :q]
    else:
        coords, z = _data(kind, n, q)
    return coords, z, vr.variogram(coords, z, n_bins, max_dist)


def _check(mk, kind, n, q, n_bins, max_dist):
    coords, z, ref = _ref(kind, n, q, n_bins, max_dist)
    if kind != "lattice":
        assert ref["edge_gap"] >= EDGE_GAP, ref["edge_gap"]       # on the reference alone: no ambiguous pair
    vg = mk.variogram(coords, z, n_bins=n_bins, max_dist=max_dist)
    T = q * (q + 1) // 2
    assert vg["gamma"].shape == (T, n_bins) and vg["pairs"] == ref["pairs"] and vg["ms"] > 0
    assert vg["count"].dtype == np.int64 and vg["count"].tolist() == ref["count"]
    assert int(vg["count"].sum()) == ref["n_in"]
    N = vg["count"].astype(np.float64)
    empty = N == 0
    assert np.isnan(vg["h"][empty]).all() and np.isnan(vg["gamma"][:, empty]).all()
    assert np.isfinite(vg["h"][~empty]).all() and np.isfinite(vg["gamma"][:, ~empty]).all()
    bound = (N + 8.0) * 2.0 ** -52
    err_d = np.where(empty, 0.0, np.abs(np.where(empty, 0.0, vg["h"]) * N - ref["sum_d"]))
    err_z = np.where(empty, 0.0, np.abs(np.where(empty, 0.0, vg["gamma"]) * 2.0 * N - ref["sum_zz"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        worst_d = np.nanmax(np.where(ref["abs_d"] > 0, err_d / (bound * ref["abs_d"]), 0.0))
        worst_z = np.nanmax(np.where(ref["abs_zz"] > 0, err_z / (bound * ref["abs_zz"]), 0.0))
    print(f"{kind} n={coords.shape[0]} q={q} bins={n_bins} max_dist={max_dist}: pairs {ref['n_in']}, "
          f"error / bound: d {worst_d:.3g}, zz {worst_z:.3g}, {vg['ms']:.3f} ms")
    assert (err_d <= bound * ref["abs_d"]).all(), (err_d, bound * ref["abs_d"])
    assert (err_z <= bound * ref["abs_zz"]).all(), (err_z, bound * ref["abs_zz"])
    return vg


def _sizes(mk):
    E = __import__(mk.__name__ + ".variogram", fromlist=["x"]).tile_edge()
    assert E == 256
    return [2, E - 1, E, E + 1, 2 * E + 1]


@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("which", range(5))
def test_sizes_around_the_tile_edge(mk, which, q):
    _check(mk, "uniform", _sizes(mk)[which], q, 15, 0.5)


@pytest.mark.parametrize("n_bins,max_dist", [(32, 0.8), (30, 0.7)])
@pytest.mark.parametrize("kind", ["uniform+dup", "clustered+dup"])
def test_thousand_sites_three_outcomes(mk, kind, n_bins, max_dist):
    coords, z, ref = _ref(kind, 1000, 3, n_bins, max_dist)
    assert coords.shape[0] == 1010 and ref["count"][0] >= 10      # the coincident pairs are in bin 0
    _check(mk, kind, 1000, 3, n_bins, max_dist)


@pytest.mark.parametrize("q", [1, 2])
def test_lattice_on_the_bin_edges(mk, q):
    vg = _check(mk, "lattice", 64, q, 10, 1.25)
    assert vg["count"].tolist() == [0, 210, 336, 340, 322, 376, 224, 162, 36, 10]
    _, _, ref = _ref("lattice", 64, q, 10, 1.25)
    keep = vg["count"] > 0
    assert (vg["gamma"][:, keep] == ref["gamma"][:, keep]).all()   # integer products: every sum is exact


def test_max_dist_below_the_smallest_distance(mk):
    vg = _check(mk, "lattice", 64, 2, 5, 0.1)
    assert vg["count"].tolist() == [0] * 5 and np.isnan(vg["h"]).all() and np.isnan(vg["gamma"]).all()


@pytest.mark.parametrize("q,n_bins,max_dist", [(1, 1, 0.5), (1, 31, 0.6), (1, 32, 0.6), (1, 64, 0.9), (2, 1, 0.5),
                                               (2, 17, 0.5), (2, 18, 0.5), (2, 64, 0.9), (3, 10, 0.5), (3, 11, 0.5),
                                               (3, 64, 0.9), (4, 6, 0.5), (4, 7, 0.5), (4, 40, 0.6)])
def test_bin_counts_where_the_launch_shape_changes(mk, q, n_bins, max_dist):
    _check(mk, "uniform", 513, q, n_bins, max_dist)


def test_constant_z_gives_gamma_exactly_zero(mk):
    coords, _ = _data("uniform", 513, 2)
    vg = mk.variogram(coords, np.full((513, 2), 0.37), n_bins=15, max_dist=0.5)
    assert (vg["count"] > 0).all() and (vg["gamma"] == 0.0).all()


def test_two_calls_return_the_same_bytes(mk):
    coords, z = _data("uniform+dup", 1000, 3)

    def call():
        vg = mk.variogram(coords, z, n_bins=32, max_dist=0.8)
        return vg["count"].tobytes() + vg["h"].tobytes() + vg["gamma"].tobytes()

    first, second = call(), call()
    small = _data("uniform", 255, 1)
    mk.variogram(small[0], small[1], n_bins=7, max_dist=0.3)       # an unrelated call in between
    assert first == second == call()

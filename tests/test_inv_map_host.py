"""The block -> job map of the inverse levels' launches (inv_map_job, csrc/mk_types.hpp; MK_INV_MAP),
evaluated on the host by the kernel's own code through mk_inv_map_jobs (no GPU work).

A level's launch (level sz, one phase) over `count` listed factors of nt 128-tiles computes tile (i, j) of
every block pair T = [T0, T0 + sz), B = [B0, B0 + sz), B0 = T0 + sz, with i < nt, on `sub` workgroups per
tile.  A workgroup's work is its K range in tiles: B0 - j in phase 0, i - B0 + 1 in phase 1.

Checked for the work-balanced map: the launch grid's blocks enumerate every live (entry, tile, sub-tile)
exactly once and nothing else (a duplicate would be invisible on the GPU: it stores the same values
twice), with the grid sized for max_entries >= count; each XCD's (block % 8) work is within one longest
job (sz) of the mean; along an XCD's block order K never increases, its blocks without a job come last,
and the sub-tiles of a tile are adjacent.  For the other arm: the map is xcd_map's."""
import numpy as np
import pytest

NTS = (1, 2, 3, 4, 5, 8, 16)
COUNTS = (0, 1, 2, 7, 8, 9, 13, 83, 250)


def _levels(nt):
    sz = 1
    while sz < nt:
        yield sz
        sz *= 2


def _jobs(mk, use_map, count, max_entries, nt, sz, phase, sub):
    lib = mk._lib.load()
    grid = lib.mk_inv_map_jobs(use_map, count, max_entries, nt, sz, phase, sub, None, 0)
    out = np.full((grid, 5), -2, dtype=np.int32)
    assert lib.mk_inv_map_jobs(use_map, count, max_entries, nt, sz, phase, sub, mk._lib.iptr(out), grid) == grid
    return out


def _live(count, nt, sz, sub):
    """Every (entry, pair, i, j, sub-tile) of a level, as rows."""
    rows = [(p, 2 * p * sz + sz + ii, 2 * p * sz + jj)
            for p in range((nt + 2 * sz - 1) // (2 * sz)) for ii in range(sz) for jj in range(sz)
            if 2 * p * sz + sz + ii < nt]
    t = np.array(rows, dtype=np.int64).reshape(-1, 3)
    e, ti, st = np.meshgrid(np.arange(count), np.arange(len(t)), np.arange(sub), indexing="ij")
    return np.column_stack([e.ravel(), t[ti.ravel()], st.ravel()])


def _key(rows, nt, sub):
    p, i, j, st = (rows[:, c].astype(np.int64) for c in (1, 2, 3, 4))
    return (((rows[:, 0].astype(np.int64) * (nt + 1) + p) * (nt + 1) + i) * (nt + 1) + j) * sub + st


def _work(rows, sz, phase):
    B0 = 2 * rows[:, 1] * sz + sz
    return B0 - rows[:, 3] if phase == 0 else rows[:, 2] - B0 + 1


@pytest.mark.parametrize("sub", [1, 4])
@pytest.mark.parametrize("nt", NTS)
def test_work_balanced_map(mk, nt, sub):
    assert list(_levels(1)) == []          # nt = 1 has no level
    for sz in _levels(nt):
        for phase in (0, 1):
            for count in COUNTS:
                for max_entries in sorted({count, 250}):
                    tag = (nt, sz, phase, sub, count, max_entries)
                    out = _jobs(mk, 1, count, max_entries, nt, sz, phase, sub)
                    has = out[:, 0] >= 0
                    assert np.all((out[~has] == -1)), tag
                    jobs = out[has]
                    live = _live(count, nt, sz, sub)
                    # exact cover: every live item once, nothing else, none beyond the grid
                    assert len(jobs) == len(live), tag
                    got = _key(jobs, nt, sub)
                    assert np.array_equal(np.sort(got), np.sort(_key(live, nt, sub))), tag
                    assert len(np.unique(got)) == len(got), tag
                    if count == 0:
                        continue
                    w = _work(out, sz, phase)
                    assert w[has].min() >= 1 and w[has].max() <= sz, tag
                    mean = w[has].sum() / 8.0
                    for x in range(8):
                        hx, wx, ox = has[x::8], w[x::8], out[x::8]
                        n = int(hx.sum())
                        assert np.all(hx[:n]) and not np.any(hx[n:]), tag        # surplus blocks come last
                        assert abs(wx[:n].sum() - mean) <= sz, (tag, x, wx[:n].sum(), mean)
                        assert np.all(np.diff(wx[:n]) <= 0), (tag, x)            # longest K ranges first
                        if n == 0:
                            continue
                        # the sub-tiles of a tile: one run of consecutive blocks, in sub-tile order
                        tile = _key(ox[:n], nt, sub) // sub
                        change = np.flatnonzero(np.diff(tile) != 0) + 1
                        starts = np.concatenate([[0], change])
                        assert len(np.unique(tile[starts])) == len(starts), (tag, x)
                        same = np.diff(tile) == 0
                        assert np.all(np.diff(ox[:n, 4])[same] == 1), (tag, x)


def test_grid_bound_is_the_documented_one(mk):
    """8 (ceil(max_entries / 8) + 1) live tiles of a matrix, times sub."""
    lib = mk._lib.load()
    for nt in NTS:
        for sz in _levels(nt):
            tiles = len(_live(1, nt, sz, 1))
            for max_entries in COUNTS:
                for sub in (1, 4, 16):
                    assert lib.mk_inv_map_jobs(1, 0, max_entries, nt, sz, 0, sub, None, 0) == \
                        8 * ((max_entries + 7) // 8 + 1) * tiles * sub


@pytest.mark.parametrize("sub", [1, 4])
@pytest.mark.parametrize("nt", NTS)
def test_map_off_is_xcd_map(mk, nt, sub):
    """MK_INV_MAP=0: xcd_map (block b on XCD b % 8 takes item (b % 8) C + b // 8 of the count * per items,
    C = ceil(count per / 8)) over the matrices' npairs sz^2 sub slots, on xcd_map's grid."""
    for sz in _levels(nt):
        npairs = (nt + 2 * sz - 1) // (2 * sz)
        per = npairs * sz * sz * sub
        for phase in (0, 1):
            for count in COUNTS:
                for max_entries in sorted({count, 250}):
                    out = _jobs(mk, 0, count, max_entries, nt, sz, phase, sub)
                    assert len(out) == 8 * ((max_entries + 7) // 8) * per
                    b = np.arange(len(out))
                    W = count * per
                    C = (W + 7) // 8
                    item = (b % 8) * C + b // 8
                    ok = (b // 8 < C) & (item < W)
                    e, t = item // max(per, 1), item % max(per, 1)
                    st, t = t % sub, t // sub
                    p, t = t // (sz * sz), t % (sz * sz)
                    i = 2 * p * sz + sz + (t % sz if phase == 0 else t // sz)
                    j = 2 * p * sz + (t // sz if phase == 0 else t % sz)
                    ok &= i < nt
                    ref = np.where(ok[:, None], np.column_stack([e, p, i, j, st]), -1)
                    assert np.array_equal(out, ref), (nt, sz, phase, sub, count, max_entries)

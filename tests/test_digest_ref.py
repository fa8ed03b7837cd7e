"""tests/digest_ref.py under test on the CPU: the restatement the device digest is compared with is pinned to
sums worked by hand.  With x = 0 the terms are the outputs of splitmix64 seeded with 0, whose first three are
published with the generator (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F); the others were worked
with unbounded integers reduced mod 2^64."""
import numpy as np

import digest_ref as dr

SPLITMIX_0 = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)
MASK = (1 << 64) - 1


def test_no_words_is_zero():
    assert dr.digest(np.zeros(0)) == 0
    assert dr.digest(np.zeros((0, 3), dtype=np.uint64)) == 0


def test_zero_words_are_the_splitmix64_stream():
    assert int(dr.mix(np.array([0x9E3779B97F4A7C15], dtype=np.uint64))[0]) == SPLITMIX_0[0]
    assert dr.digest(np.zeros(1)) == SPLITMIX_0[0]
    assert dr.digest(np.zeros(2)) == (SPLITMIX_0[0] + SPLITMIX_0[1]) & MASK == 0x509946A41CD733A3
    assert dr.digest(np.zeros(3)) == sum(SPLITMIX_0) & MASK


def test_sums_worked_by_hand():
    assert dr.words_of(np.array([1.0]))[0] == 0x3FF0000000000000
    assert dr.digest(np.array([1.0])) == 0x88D7C35BBBF3EDED
    assert dr.digest(np.array([MASK], dtype=np.uint64)) == 0xE4D971771B652C20          # x + golden wraps
    assert dr.digest(np.array([1, 2, 3], dtype=np.uint64)) == 0xEDBE5CA3654F5804
    assert dr.digest(np.array([2, 1, 3], dtype=np.uint64)) == 0xF32FAC2652772036       # position matters
    assert dr.digest(np.array([1, 2, 3], dtype=np.int64)) == 0xEDBE5CA3654F5804        # bit patterns, any 8-byte type


def test_regions_enumerate_column_major():
    M = np.arange(25, dtype=np.float64).reshape(5, 5)       # M[r, c] = 5 r + c
    assert dr.region_tri(M, 3).tolist() == [0, 5, 10, 6, 11, 12]
    assert dr.region_tri(M, 0).size == 0
    T = [np.arange(128 * 128, dtype=np.float64).reshape(128, 128) + 1e6 * k for k in range(2)]
    tri = dr.region_tiles(T, 130, full=False)
    assert tri.size == 128 * 129 // 2 + 3 and tri[:3].tolist() == [0, 128, 256]
    assert tri[-3:].tolist() == [1e6, 1e6 + 128, 1e6 + 129]
    full = dr.region_tiles(T, 130, full=True)
    assert full.size == 2 * 64 * 64 + 4 and full[-4:].tolist() == [1e6, 1e6 + 128, 1e6 + 1, 1e6 + 129]
    assert full[:2].tolist() == [0, 128] and full[4096:4098].tolist() == [64 * 128 + 64, 65 * 128 + 64]   # quadrant 1
    assert dr.region_tiles(T, 70, full=True).size == 64 * 64 + 6 * 6

"""The state digest kernel (include/mk.h "checkpoints"; csrc/mk_checkpoint.hip k_state_digest) through its
stand-alone entry mk_digest, against the NumPy restatement tests/digest_ref.py (pinned on the CPU by
tests/test_digest_ref.py), and the digests of a fresh session against the same regions cut out of what the parity
entry points return.  Everything here is an equality of 64-bit integers."""
import numpy as np
import pytest

import digest_ref as dr
import krig_ref as kr

pytestmark = pytest.mark.gpu

# the partial last 16-byte load (odd counts), the workgroup's 512-word column edge, the 1,000-word chunk edge
COUNTS = [0, 1, 2, 255, 256, 257, 4095, 4097, 2 ** 20 + 3]
_words = {}


def _w(n):
    """n words shared by the tests and left unchanged: doubles, with the patterns an inverse holds -- zeros, a
    negative zero, denormals, a NaN payload, infinities."""
    if n not in _words:
        rng = np.random.default_rng(1000 + n)
        x = rng.standard_normal(n)
        special = [0.0, -0.0, 5e-324, np.inf, -np.inf, np.nan, 1.0]
        for i, v in enumerate(special[:n]):
            x[(i * 37) % n] = v
        x.setflags(write=False)
        _words[n] = x
    return _words[n]


@pytest.mark.parametrize("n", COUNTS)
def test_digest_equals_the_restatement(mk, n):
    x = _w(n)
    assert mk.digest(x) == dr.digest(x)
    assert mk.digest(x.view(np.uint64)) == dr.digest(x)


@pytest.mark.parametrize("n", COUNTS)
def test_digest_does_not_depend_on_the_upload_chunk(mk, monkeypatch, n):
    x = _w(n)
    whole = mk.digest(x)
    monkeypatch.setenv("MK_DIGEST_CHUNK", "1000")
    assert mk.digest(x) == whole == dr.digest(x)


@pytest.mark.parametrize("n", [c for c in COUNTS if c >= 1])
def test_digest_sees_one_bit_and_the_order(mk, n):
    x = _w(n)
    base = mk.digest(x)
    for pos, bit in ((0, 0), (n - 1, 63), (n // 2, 31)):
        y = x.view(np.uint64).copy()
        y[pos] ^= np.uint64(1) << np.uint64(bit)
        assert mk.digest(y) != base, (pos, bit)
    if n >= 2:
        u = x.view(np.uint64)
        i, j = 0, next(k for k in range(n - 1, 0, -1) if u[k] != u[0])
        y = u.copy()
        y[i], y[j] = u[j], u[i]
        assert mk.digest(y) != base


def test_digest_refuses_other_word_sizes(mk):
    with pytest.raises(ValueError, match="8-byte words"):
        mk.digest(np.zeros(4, dtype=np.float32))


def _fresh(mk, monkeypatch, sweep=None):
    """A fresh E1 session whose starting phi is the logit's fixed point (theta = 0 gives phi = (a + b) / 2 = 8
    exactly), and the parity entry points' factor and inverse of every subset at that phi."""
    if sweep is not None:
        monkeypatch.setenv("MK_SWEEP", sweep)
    pb = kr.problem("E1")
    cfg = mk.SamplerConfig(1, 2, np.zeros(2), np.full(2, 0.05), n_batch=4, batch_length=10, burn_in=21, seed=12,
                           phi_starting=[8.0], phi_unif=([4.0], [12.0]))
    with mk.Session(pb["subsets"], cfg, subset_base=2) as ses:
        dg = ses.digest()
        stats = ses.kernel_stats(mk.session.KS_CKPT)
    ref = []
    for sb in pb["subsets"]:
        R = mk.correlation_batched(sb["coords"][None], 8.0)
        L, _ld, Q = mk.cholesky_batched(R, inverse=True)
        ref.append((L[0], Q[0]))
    return pb, dg, ref, stats


def test_session_digest_of_the_factor_equals_the_parity_factor(mk, monkeypatch):
    """Session.digest()'s L column against mk.digest of the lower triangle below n_s of mk_cholesky_batched's
    factor of mk_correlation_batched's R at the starting phi: the session's bordered, padded factorisation and the
    parity entry's plain one are the same bits there.  (mk_cholesky_batched returns L and R^-1; no entry point
    returns W = L^-1 or its diagonal tiles, so those two columns are checked for being there -- non-zero, and
    different per subset -- and bit for bit by the restore of tests/test_gpu_checkpoint.py.)"""
    pb, dg, ref, stats = _fresh(mk, monkeypatch)
    assert dg.shape == (4, 4) and dg.dtype == np.uint64 and stats["launches"] > 0
    for i, sb in enumerate(pb["subsets"]):
        ns = sb["coords"].shape[0]
        assert int(dg[i, 0]) == mk.digest(dr.region_tri(ref[i][0], ns)) == dr.digest(dr.region_tri(ref[i][0], ns)), i
    assert np.all(dg[:, 1] != 0) and np.all(dg[:, 2] != 0) and len(set(dg[:, 2].tolist())) == 4
    assert np.all(dg[:, 3] == 0)          # the site sweep keeps no QB


def test_session_digest_of_qb_equals_the_parity_inverse(mk, monkeypatch):
    """The block sweep (MK_SWEEP=1) keeps QB, the diagonal 64 x 64 quadrants of the diagonal 128-tiles of R^-1:
    its digest against the same quadrants cut out of mk_cholesky_batched's inverse."""
    pb, dg, ref, _ = _fresh(mk, monkeypatch, sweep="1")
    for i, sb in enumerate(pb["subsets"]):
        ns = sb["coords"].shape[0]
        Q = ref[i][1]
        tiles = []
        for k in range((ns + 127) // 128):
            T = np.zeros((128, 128))
            m = min(128, ns - 128 * k)
            T[:m, :m] = Q[128 * k:128 * k + m, 128 * k:128 * k + m]
            tiles.append(T)
        want = dr.digest(dr.region_tiles(tiles, ns, full=True))
        print(f"QB subset {i}: session {int(dg[i, 3]):016x} parity {want:016x}")
        assert int(dg[i, 3]) == want, i

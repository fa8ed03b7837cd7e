"""The kriging predictor (MK.R:87) -- k_pred_PT, k_pred_PT_matern, k_pred_var, k_pred_var_reduce,
k_trmv_Z, k_krig_g and the four draw kernels -- against an 80-bit reference that shares none of its
formulas with the device or the CPU oracle (tests/krig_ref.py, itself under test in
tests/test_krig_ref.py), at geometrically hard test sites.

A session records everything the predictor consumes per kept state: samples (K = A A', phi_h, nu_h),
w_samples (w = A u) and, through Philox, the kriging normals.  The reference recomputes every draw of
w_pred_samples in np.longdouble from the device's own recorded states, so no chain can diverge, and the
conditioning enters through the derived bars of tests/krig_ref.py (hard bar at every site; at regular
sites, sd_ref >= 0.05, also 16 x the error of the same predictor through LAPACK) instead of a flat 1e-8.

Test sites (tests/krig_ref.py problem): per subset one observed site and copies of it 1e-9, 1e-6 and
1e-3 away in x, (3, 3), (50, 50), one test site twice, the rest uniform; the specials sit at indices 0,
255, 256, 260, 1..3, ... -- tile and workgroup edges of n_test = 261 (256 + a ragged tail of 5).
Every session: n_batch = 2, batch_length = 4, burn_in = 5 (8 iterations, 4 kept states).

  case  model  q  subset sizes        what it pins
  E1    exp    1  127, 129, 255, 2    N = 128 fills one tile; the bordered row in a tile of its own; ragged
                                      shard; tiny subset; k_pred_draw, k_pred_tab_draw, k_pred_draw_runs,
                                      k_pred_cheb_draw<1>
  E2    exp    1  513                 the second 512-row pass of the draw kernels' row loop, one live row
                                      (n_test = 71: tile 256 stays fused, the -1 arm draws from the tables)
  E3    exp    1  255, 60 in a 1e-3   kappa_2 ~ 1e6: the bars scale, and the comparative bar still bites
                  box
  L1    exp    2  129, 127            the per-outcome s_h, m_h and the A mix; k_pred_cheb_draw<2>
  M1    matern 1  200, 129            k_pred_PT_matern at x = 0, at x < 0.5 (exact series) and at (50, 50)
                                      beyond its tables

Largest values per case and arm (MK_KRIG_CHEB, predict_tile) over subsets and kept states, device | LAPACK
(MI355X; kappa_2 on the host; ratio: device to LAPACK scale max(e_L, floor) at the regular sites):

  case cheb tile   kappa_2    regular sites         near-singular sites   ratio   largest |dev - ref| / hard bar
   E1    0    0   4.95e+03   1.45e-14 | 2.04e-14   8.43e-09 | 8.43e-09    0.31   2.4e-01
   E1   -1    0   4.95e+03   1.91e-14 | 2.04e-14   1.41e-08 | 8.43e-09    0.30   2.8e-03
   E1    0  256   4.95e+03   1.45e-14 | 2.04e-14   8.43e-09 | 8.43e-09    0.31   2.4e-01
   E1   -1  256   4.95e+03   2.35e-14 | 2.04e-14   1.41e-08 | 8.43e-09    0.50   2.8e-03
   E2    0    0   1.31e+04   2.33e-14 | 5.31e-14   1.07e-13 | 2.17e-13    0.18   4.1e-04
   E2   -1  256   1.31e+04   2.85e-14 | 5.31e-14   2.96e-13 | 2.17e-13    0.18   3.7e-06
   E3    0    0   2.70e+06   3.29e-14 | 1.02e-13   3.78e-14 | 6.18e-13    0.36   5.2e-04
   E3   -1  256   2.70e+06   2.64e-14 | 1.02e-13   8.99e-13 | 6.18e-13    0.35   1.1e-06
   L1    0    0   3.49e+03   7.09e-15 | 6.77e-15   8.33e-13 | 5.64e-13    0.18   5.2e-03
   L1   -1  256   3.49e+03   6.12e-15 | 6.77e-15   1.09e-12 | 5.64e-13    0.17   5.5e-05
   M1    0    0   8.57e+04   1.68e-13 | 6.31e-14   8.03e-09 | 7.00e-11    2.37   2.6e-03
   M1    0  256   8.57e+04   1.68e-13 | 6.31e-14   8.03e-09 | 7.00e-11    2.37   2.6e-03

(regular: sd_ref >= 0.05; the near-singular sites are the copies of observed sites at d <= 1e-3, where a
rounding-level 1 - s sets sd: 8.43e-09 is sqrt(7e-17) |z*| at a d = 0 site, on the device and through
LAPACK alike.  0.24 of the hard bar is E1's two-site subset, whose bar is 3 eps: one ulp of a draw.  The
comparative margin of 16 was never approached: the largest ratio is 2.4, at the Matern tables.)
"""
import numpy as np
import pytest

from oracle import philox

import krig_ref as kr

pytestmark = pytest.mark.gpu

WIN = dict(n_batch=2, batch_length=4, burn_in=5)
SEED, BASE = 12, 2
_ARMS = [(case, arm) for case in kr.CASES for arm in kr.CASES[case]["arms"]]
_case = {}        # case -> the first arm's recorded states and the reference computed from them


def _run(mk, monkeypatch, pb, cfg, mode):
    monkeypatch.setenv("MK_KRIG_CHEB", mode)
    with mk.Session(pb["subsets"], cfg, coords_test=pb["coords_test"], subset_base=BASE, record_w=True) as ses:
        ses.run(cfg.n_samples)
        out = ses.outputs(quantiles=False, samples=True, w_samples=True, w_pred_samples=True)
        out["cheb"] = ses.kernel_stats(mk.session.KS_KRIG_CHEB)
        out["fallback"] = ses.kernel_stats(mk.session.KS_KRIG_FALLBACK)
    monkeypatch.delenv("MK_KRIG_CHEB", raising=False)
    return out


def _reference(case, pb, cfg, out):
    """predict_state of every (subset, kept state) from the recorded states of `out`."""
    c = kr.CASES[case]
    q, p = cfg.q, cfg.p
    ntri = q * (q + 1) // 2
    matern = c["model"] == "matern"
    refs = {}
    for s, sb in enumerate(pb["subsets"]):
        sub = kr.SubsetRef(sb["coords"], pb["coords_test"], matern)
        key = philox.make_key(cfg.seed, BASE + s)
        for k in range(cfg.kept):
            it = cfg.burn_in - 1 + k
            row = out["samples"][s][it]
            nu = row[p + ntri + q:p + ntri + 2 * q] if matern else np.zeros(q)
            refs[s, k] = kr.predict_state(sub, row[p:p + ntri], row[p + ntri:p + ntri + q], nu, out["w_samples"][s][:, it],
                                          key, it)
    return refs


@pytest.mark.parametrize("case,arm", _ARMS, ids=[f"{c}-cheb{a[0]}-tile{a[1]}" for c, a in _ARMS])
def test_kriging_draws_against_the_80_bit_reference(mk, monkeypatch, case, arm):
    """One case, one arm: every draw of every kept state of every subset is finite and inside the hard
    bar, the regular sites inside the comparative bar; the chain is the case's chain bit for bit; a -1
    arm interpolated (fused tables or tiled nodes) and did not fall back."""
    mode, tile = arm
    c = kr.CASES[case]
    q = c["q"]
    pb = kr.problem(case)
    T = pb["coords_test"].shape[0]
    cfg = mk.SamplerConfig(q, 2 * q, np.zeros(2 * q), np.full(2 * q, 0.05), cov_model=c["model"], seed=SEED,
                           predict_tile=tile, **WIN)
    out = _run(mk, monkeypatch, pb, cfg, mode)
    if mode == "-1":
        assert out["cheb"]["launches"] > 0 and out["fallback"]["launches"] == 0, (out["cheb"], out["fallback"])
    else:
        assert out["cheb"]["launches"] == 0 and out["fallback"]["launches"] == 0, (out["cheb"], out["fallback"])
    if case not in _case:
        _case[case] = (out["samples"], out["w_samples"], _reference(case, pb, cfg, out))
    samples, w_samples, refs = _case[case]
    for s in range(len(pb["subsets"])):                       # kriging does not feed back into the chain
        assert np.array_equal(out["samples"][s], samples[s]), s
        assert np.array_equal(out["w_samples"][s], w_samples[s]), s
    bad, figs = [], []
    for (s, k), ref in refs.items():
        dev = out["w_pred_samples"][s][:, k].reshape(T, q)
        b, f = kr.judge(dev, ref, interpolated=mode == "-1")
        bad += [f"subset {s} state {k}: {x}" for x in b]
        figs.append(f)
    top = {key: max(f[key] for f in figs) for key in figs[0]}
    ratio = max(f["dev_regular"] / f["scale"] for f in figs)
    print(f"\nKRIG_PARITY  {case:<3} {mode:>3} {tile:>4}   {top['kappa']:.2e}   {top['dev_regular']:.2e} | "
          f"{top['lapack_regular']:.2e}   {top['dev_singular']:.2e} | {top['lapack_singular']:.2e}   {ratio:5.2f}   "
          f"{top['hard_slack']:.1e}")
    assert not bad, "\n".join(bad[:12] + [f"... {len(bad)} in all"])

// Kriging on the host side: the kriging buffers, the fused path's phi tables (krig_tables) and the
// tiled replay after the fit, phi-interpolated (predict_tile_cheb) or exact (predict_tile).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <vector>
#include "mk_session.hpp"

using namespace mk;

// (Re)allocate the kriging buffers for n_test_all test sites (coords_test: n_test_all x 2
// column-major) and upload the sites: all of them in d_ct_all, the fused path's copy in the tile
// buffer d_ct.  Tiled sessions size the buffers for one tile.  Refreshes the group views.
int mk::kriging_buffers(mk_session* s, int n_test_all, const double* coords_test) {
  Model& md = s->md;
  for (void* b : s->kbufs) s->release(b);
  s->kbufs.clear();
  md.PT = md.XK = md.s_pred = md.s_part = md.w_pred = nullptr;
  md.span_pt = nullptr;
  const int S = s->S, q = s->q, nt = s->nt, n_pad = s->n_pad;
  s->n_test_all = n_test_all;
  s->n_test_pad_all = round_up(std::max(n_test_all, 1), 256);
  s->pred_tile = s->tiled ? std::min(s->tile_req, std::max(n_test_all, 1)) : n_test_all;
  double* d_ct = nullptr;
  double* d_spt = nullptr;
  int rc;
  // Tiled sessions whose buffers for the requested tile do not fit in HBM (X and P^T are n_pad x tile
  // per pair, the draws n_kept x tile per subset: configs[4]'s 250 subsets at 65,536 sites on one GPU
  // would need ~700 GB) take the largest tile that fits, halving it (in 256-site steps) until the
  // allocations succeed.  The draws do not depend on the tile (keyed by the global site index);
  // mk_session_predict_tile reports the tile in use.
  // MK_KRIG_MEM_GB (optional): a budget for the tile's kriging buffers (tests; hosts sharing the GPU)
  const char* cap_env = std::getenv("MK_KRIG_MEM_GB");
  const double cap = (cap_env && *cap_env) ? std::atof(cap_env) * 1e9 : 0.0;
  for (;;) {
    const int n_test = n_test_all > 0 ? s->pred_tile : 0;
    const int n_test_pad = round_up(std::max(n_test, 1), 256);
    const double bytes = 8.0 * ((double)S * q * n_test_pad * (1.0 + nt + (n_test > 0 ? (s->pred_gen ? 1 : 2) * n_pad : 0)) +
                                (double)S * md.n_kept * q * std::max(n_test, 1));
    if (cap > 0.0 && bytes > cap && s->tiled && s->pred_tile > 256) {
      s->pred_tile = std::max(256, round_up(s->pred_tile / 2, 256));
      continue;
    }
    md.n_test = n_test;
    md.n_test_pad = n_test_pad;
    md.ntt = n_test_pad / MK_NB;
    d_ct = d_spt = nullptr;
    md.PT = md.XK = md.s_pred = md.s_part = md.w_pred = nullptr;
    s->d_ct_all = nullptr;
    if ((rc = s->alloc(&d_ct, (size_t)2 * n_test_pad)) || (rc = s->alloc(&s->d_ct_all, (size_t)2 * s->n_test_pad_all)) ||
        (rc = s->alloc(&d_spt, (size_t)S)) ||
        (rc = s->alloc(&md.s_pred, (size_t)S * q * n_test_pad)) ||
        (rc = s->alloc(&md.s_part, (size_t)S * q * nt * n_test_pad)) ||
        (n_test > 0 && !s->pred_gen && (rc = s->alloc(&md.PT, (size_t)S * q * n_pad * n_test_pad))) ||
        (n_test > 0 && (rc = s->alloc(&md.XK, (size_t)S * q * n_pad * n_test_pad))) ||
        (rc = s->alloc(&md.w_pred, (size_t)S * md.n_kept * q * std::max(n_test, 1)))) {
      for (void* b : {(void*)d_ct, (void*)s->d_ct_all, (void*)d_spt, (void*)md.s_pred, (void*)md.s_part, (void*)md.PT,
                      (void*)md.XK, (void*)md.w_pred})
        s->release(b);
      md.PT = md.XK = md.s_pred = md.s_part = md.w_pred = nullptr;
      s->d_ct_all = nullptr;
      if (rc == MK_E_NOMEM && s->tiled && s->pred_tile > 256) {
        s->pred_tile = std::max(256, round_up(s->pred_tile / 2, 256));
        continue;
      }
      return rc;
    }
    break;
  }
  md.coords_test = d_ct;
  s->kbufs = {d_ct, s->d_ct_all, md.s_pred, md.s_part, md.PT, md.XK, md.w_pred, d_spt};
  {   // Matern kriging tables (k_pred_PT_matern): a bound on every subset-site to test-site distance
    double tb[4];
    site_bbox(coords_test, coords_test + n_test_all, n_test_all, tb);
    std::vector<double> hs(S);
    for (int i = 0; i < S; ++i) hs[i] = n_test_all > 0 ? matern_span_pt(s->bbox.data() + 4 * i, tb) : 0.0;
    HIPCHK(hipMemcpy(d_spt, hs.data(), (size_t)S * 8, hipMemcpyHostToDevice));
    md.span_pt = d_spt;
    s->span_pt_h = hs;
  }
  HIPCHK(hipMemset(md.s_pred, 0, (size_t)S * q * md.n_test_pad * 8));
  const int npa = s->n_test_pad_all;
  std::vector<double> hct((size_t)2 * npa, 0.0);
  for (int t = 0; t < n_test_all; ++t) {
    hct[t] = coords_test[t];
    hct[npa + t] = coords_test[n_test_all + t];
  }
  HIPCHK(hipMemcpy(s->d_ct_all, hct.data(), hct.size() * 8, hipMemcpyHostToDevice));
  s->ct_h.assign(coords_test, coords_test + (size_t)2 * n_test_all);
  // fused kriging reads every site from d_ct ([2][n_test_pad]); tiled mode fills it per tile
  if (!s->tiled) HIPCHK(hipMemcpy(d_ct, hct.data(), hct.size() * 8, hipMemcpyHostToDevice));
  s->all.md = s->md;
  for (auto& g : s->groups) g.md = model_view(s->md, g.s0, g.S);
  return 0;
}

// The result sinks of a tiled session, in the order a tile replay fills them.  These two functions are the
// list: a new sink adds one line to each ("adding a sink").
//
// The sinks that are on take their share of tile [t0, ..), whose draws are in md.w_pred ([S][n_kept][Ct]),
// while the draws exist (no second replay); the first error ends it.
static int tile_sinks(mk_session* s, int t0, int n_kept, int Ct) {
  int rc = 0;
  if (s->diag_on) rc = tile_diagnostics(s, t0, n_kept, Ct);
  if (!rc && s->val.on) rc = tile_scores(s, t0, n_kept, Ct);
  if (!rc && s->maps.on) rc = tile_maps(s, t0, n_kept, Ct);
  if (!rc && s->pairs.on) rc = tile_pairs(s, t0, n_kept, Ct);
  if (!rc && s->regions.on) rc = tile_regions(s, t0, n_kept, Ct);   // fed inside the replay loop, not from md.w_pred
  return rc;
}

// The test sites go: every sink was sized for them, and the held-out data belonged to them.
static void detach_sinks(mk_session* s) {
  s->diag_on = false;
  s->diag_sink = mk_diagnostics{};
  validation_detach(s);
  maps_detach(s);
  pairs_detach(s);
  regions_detach(s);
}

extern "C" int mk_session_set_test_sites(mk_session* s, int32_t n_test, const double* coords_test) {
  if (!s) return set_err(MK_E_ARG, "null session");
  if (!s->tiled)
    return set_err(MK_E_ARG, "the session keeps no chain states: create it with predict_tile > 0 (and no test sites)");
  if (n_test < 1 || !coords_test) return set_err(MK_E_ARG, "n_test must be >= 1 with coordinates");
  MK_ENTRY_DEVICE(s->device);
  HIPCHK(hipStreamSynchronize(s->stream));
  detach_sinks(s);
  int rc = set_test_covars(s, nullptr);   // the covariates belonged to the sites that go
  if (rc) return rc;
  return kriging_buffers(s, n_test, coords_test);
}

int mk::set_test_covars(mk_session* s, const double* x_test) {
  s->release(s->d_xt);
  s->d_xt = nullptr;
  if (!x_test) return 0;
  const size_t n = (size_t)s->q * s->n_test_all * s->p;
  int rc = s->alloc(&s->d_xt, n);
  if (rc) return rc;
  HIPCHK(hipMemcpy(s->d_xt, x_test, n * 8, hipMemcpyHostToDevice));
  return 0;
}

extern "C" int mk_session_set_test_covars(mk_session* s, const double* x_test) {
  if (!s) return set_err(MK_E_ARG, "null session");
  if (s->n_test_all < 1) return set_err(MK_E_ARG, "x_test needs test sites: the session has none");
  if (!x_test) return set_err(MK_E_ARG, "null x_test");
  MK_ENTRY_DEVICE(s->device);
  HIPCHK(hipStreamSynchronize(s->stream));
  return set_test_covars(s, x_test);
}

ProbSrc mk::prob_src(const mk_session* s, int t0) {
  const Model& md = s->md;
  ProbSrc ps;
  ps.samples = md.samples + (long)(md.kept0 + s->win_lo) * md.P;
  ps.subset_stride = (long)md.n_samples * md.P;
  ps.row_stride = md.P;
  ps.x = s->d_xt;
  ps.ldx = (long)s->q * s->n_test_all;
  ps.x_off = (long)t0 * s->q;
  ps.p = md.p;
  ps.link = md.link;
  return ps;
}

int mk::pred_prob_to_host(mk_session* s, int subset, int t0, int n_rows, int n_cols, double* scratch, double* dst,
                          size_t ld_dst) {
  ProbSrc ps = prob_src(s, t0);
  ps.samples += (long)subset * ps.subset_stride;
  const long n = (long)n_rows * n_cols;
  MK_LAUNCH(k_pred_prob, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream,
            s->md.w_pred + (size_t)subset * n_rows * n_cols, (long)n_cols, n_rows, n_cols, scratch, ps);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy2DAsync(dst, ld_dst * 8, scratch, (size_t)n_cols * 8, (size_t)n_cols * 8, n_rows, hipMemcpyDeviceToHost,
                          s->stream));
  return 0;
}

extern "C" int mk_session_set_kept_window(mk_session* s, int32_t first, int32_t last) {
  if (!s) return set_err(MK_E_ARG, "null session");
  const int lo = s->md.kept0 + 1, hi = s->md.n_samples;
  // a session that is not tiled but recorded samples and w: the window serves mk_session_criteria alone
  const bool crit_only = !s->tiled && s->md.samples && s->md.w_samples;
  if (!s->tiled && !crit_only) return set_err(MK_E_ARG, "kept windows need a session created with predict_tile > 0");
  if (first < lo || last < first || last > hi)
    return set_err(MK_E_ARG, "kept window must satisfy burn_in <= first <= last <= n.samples");
  if (crit_only) {
    s->crit.win_lo = first - lo;
    s->crit.win_n = last - first + 1;
    return 0;
  }
  s->win_lo = first - lo;
  s->win_n = last - first + 1;
  return 0;
}

// A tile's draws are in md.w_pred ([S][n_kept][Ct]): its 200-level grids into dq (and those of
// p = pred_prob(draw) into dqp) and, if o->w_pred_samples / o->p_pred_samples, the draws to the host.
// Returns after the stream is idle.
static int tile_outputs(mk_session* s, int t0, double* dq, double* dqp, mk_outputs* o, int n_kept, int Ct) {
  Model& md = s->md;
  const int S = s->S, q = s->q;
  const long C = (long)q * s->n_test_all;
  hipStream_t st = s->stream;
  if (dq) {
    const int rq = launch_quantiles(S * Ct, st, md.w_pred, (long)n_kept * Ct, (long)Ct, n_kept, Ct, s->d_probs,
                                    MK_N_LEVELS, dq);
    if (rq) return rq;
  }
  const bool p_draws = o && o->p_pred_samples;   // predict_tile checked that the session has x_test
  if (dqp) {
    const int rq = launch_quantiles_prob(S * Ct, st, md.w_pred, (long)n_kept * Ct, (long)Ct, n_kept, Ct, s->d_probs,
                                         MK_N_LEVELS, dqp, prob_src(s, t0));
    if (rq) return rq;
  }
  DevBufs scratch;
  if (p_draws) {   // one subset at a time through a [n_kept][Ct] scratch
    double* dp = scratch.get<double>((size_t)n_kept * Ct);
    if (!dp) return set_err(MK_E_NOMEM, "p draw scratch");
    for (int i = 0; i < S; ++i) {
      const int rc = pred_prob_to_host(s, i, t0, n_kept, Ct, dp, o->p_pred_samples + (size_t)i * n_kept * C + (size_t)t0 * q,
                                       (size_t)C);
      if (rc) return rc;
    }
  }
  if (o && o->w_pred_samples)   // per subset (C x kept) column-major
    for (int i = 0; i < S; ++i)
      HIPCHK(hipMemcpy2DAsync(o->w_pred_samples + (size_t)i * n_kept * C + (size_t)t0 * q, (size_t)C * 8,
                              md.w_pred + (size_t)i * n_kept * Ct, (size_t)Ct * 8, (size_t)Ct * 8, n_kept,
                              hipMemcpyDeviceToHost, st));
  const int rc = tile_sinks(s, t0, n_kept, Ct);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(st));
  // The replay factored the kept states again.  Each was an accepted candidate of the fit, so a flag
  // here means the device disagreed with itself: an error (the draws above came from a NaN factor),
  // and the flag is cleared for the chain's next candidates.
  std::vector<int> info((size_t)S * q);
  HIPCHK(hipMemcpy(info.data(), md.info, info.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int sh = 0; sh < S * q; ++sh)
    if (info[sh]) {
      HIPCHK(hipMemset(md.info, 0, info.size() * sizeof(int)));
      return set_err(MK_E_HIP, "kriging replay: subset " + std::to_string(md.subset_base + sh / q) + ", outcome " +
                                   std::to_string(sh % q) + ": a kept state's factorisation failed (it succeeded in the fit)");
    }
  return 0;
}

// ------------------------------------------------------------------ kriging variance by phi interpolation
// (exponential; the tiled replay for any q, the fused tables for q = 1; DESIGN.md 4.7, mk_mcmc.hip
// section 11).  s(t; phi) = rho_t' R(phi)^-1 rho_t is analytic in phi: it is computed exactly (the
// replay's own kernels: candidate, Cholesky, inverse, X = W P^T) at nc Chebyshev nodes (first kind) of a
// phi range per (subset, outcome) pair and interpolated (barycentric) wherever a draw needs it.
// nc = 6 + ceil((phi_hi - phi_lo) * d_max), at least 10, at most 32 (d_max:
// the subset's largest site-to-site or site-to-test-site distance, so the rule counts the range in units
// of the correlation decay; measured in float64 on 2,000-site subsets with clustered sites and test
// sites 1e-6 from a site, d_max 1.41: |error| 2e-14 over phi in [3.3, 11.8] with the rule's 18 nodes,
// 1e-14 over [4.5, 10.5] with 15, 1e-14 over [6, 8] with 10; on the GPU at configs[4] 4 + ceil(.), at
// least 8, left 6.5e-12 and 8 + ceil(.), at least 12, 2.6e-14).  The
// exact values at nchk check points (the range's ends, then interior points) bound the interpolant's
// error before any draw uses it.

// Nodes of [lo, hi] for each (subset, outcome) pair i = s q + h: nc[i], the slots' phi (nodes, then nchk
// check points) and the barycentric weights; d_max is the subset's, and at least dmax_regions (the largest
// distance inside a region while regions are on the interpolated route, else 0: S_h holds the correlations
// between a region's sites).  Returns the slot count E (the largest nc + nchk).
static int cheb_plan(mk_session* s, const std::vector<double>& lo, const std::vector<double>& hi, int force_n, int nchk,
                     std::vector<int>& nc, std::vector<std::vector<double>>& sphi, std::vector<double>& wts,
                     double dmax_regions = 0.0) {
  const int S = s->S * s->q;
  nc.assign(S, 0);
  sphi.assign(S, {});
  wts.assign((size_t)S * MK_CHEB_MAX, 0.0);
  int E = 0;
  for (int i = 0; i < S; ++i) {
    const double* bb = s->bbox.data() + 4 * (i / s->q);
    const double dmax = std::fmax(std::fmax(s->span_pt_h[i / s->q], std::hypot(bb[1] - bb[0], bb[3] - bb[2])), dmax_regions);
    const int n = force_n > 1 ? std::min(force_n, MK_CHEB_MAX)
                              : std::max(10, std::min(MK_CHEB_MAX, 6 + (int)std::ceil((hi[i] - lo[i]) * dmax)));
    nc[i] = n;
    const double c = 0.5 * (lo[i] + hi[i]), h = 0.5 * (hi[i] - lo[i]);
    for (int m = 0; m < n; ++m) {
      const double ang = M_PI * (2.0 * m + 1.0) / (2.0 * n);
      sphi[i].push_back(c + h * std::cos(ang));
      wts[(size_t)i * MK_CHEB_MAX + m] = ((m & 1) ? -1.0 : 1.0) * std::sin(ang);
    }
    static const double frac[5] = {0.0, 1.0, 0.5, 0.25, 0.75};
    for (int k = 0; k < nchk; ++k) sphi[i].push_back(lo[i] + frac[k] * (hi[i] - lo[i]));
    E = std::max(E, n + nchk);
  }
  return E;
}

// Exact s of every planned slot into Sn ([slot][S q][n_test_pad] of mt's sites) and the slots' device phi
// into nphi; then the interpolant against the check points (largest difference over pairs and sites
// into *emax).  Slot e is one pass of the replay's own kernels over the pairs that have a slot e, all
// outcomes of a subset together: its theta record carries each outcome's own slot-e phi_h, and the
// lists are the replay's (per outcome the subsets, then the pairs sh = s q + h).  A pair with fewer
// slots than E is simply not listed past its last one -- nothing is factored or refreshed for it, and
// its rows of the later slots of Sn stay zero and unread (its unused phi_h in those records repeats
// its first node, so the record stays a valid theta).  The factor slots, cur and W serve as scratch:
// callers are the tiled replay (the chain is finished) and session set-up (before the initial
// factorisation).  The host stays at most four slots ahead of the device.
// ri (regions on the interpolated route, else NULL): every slot's X also gives the regions' S (regions_node),
// and the interpolant of S is checked like that of s (regions_check; its own largest difference into
// *emax_regions, and folded into *emax).
static int cheb_eval(mk_session* s, Model mt, const std::vector<int>& nc, const std::vector<std::vector<double>>& sphi,
                     const std::vector<double>& wts, int E, int nchk, DevBufs& scratch, ChebK* ck, double* emax,
                     RegionInterp* ri = nullptr, double* emax_regions = nullptr) {
  Model& md = s->md;
  const int S = s->S, q = s->q, SQ = S * q, nth = md.n_theta, T_pad = md.n_test_pad;
  hipStream_t st = s->stream;
  Group g = s->all;
  // slot e's theta (phi in the candidate's logit form; the device's phi of it is what counts) and its
  // lists: [q][S] subsets per outcome, [q] their counts, [S q] pairs (outcome-major, as k_kept_dirty
  // lists them), [1] their count
  const size_t LS = (size_t)2 * SQ + q + 1;
  std::vector<double> thn((size_t)E * S * nth, 0.0);
  std::vector<int> lists((size_t)E * LS, 0);
  for (int e = 0; e < E; ++e) {
    int* L = lists.data() + (size_t)e * LS;
    int pc = 0;
    for (int h = 0; h < q; ++h) {
      const double pa = md.phi_a[h], pb = md.phi_b[h];
      int cnt = 0;
      for (int i = 0; i < S; ++i) {
        const std::vector<double>& sp = sphi[(size_t)i * q + h];
        const bool has = e < (int)sp.size();
        const double ph = has ? sp[e] : sp[0];
        thn[((size_t)e * S + i) * nth + md.ntri + h] = std::log((ph - pa) / (pb - ph));
        if (has) {
          L[h * S + cnt++] = i;
          L[SQ + q + pc++] = i * q + h;
        }
      }
      L[SQ + h] = cnt;
    }
    L[2 * SQ + q] = pc;
  }
  double* d_thn = scratch.get<double>(thn.size());
  double* d_nphi = scratch.get<double>((size_t)E * SQ);
  double* d_wts = scratch.get<double>(wts.size());
  int* d_nc = scratch.get<int>((size_t)SQ);
  int* d_lists = scratch.get<int>(lists.size());
  double* d_Sn = scratch.get<double>((size_t)E * SQ * T_pad);
  unsigned long long* d_err = scratch.get<unsigned long long>(1);
  if (!d_thn || !d_nphi || !d_wts || !d_nc || !d_lists || !d_Sn || !d_err) return MK_CHEB_EXACT;
  HIPCHK(hipMemcpyAsync(d_thn, thn.data(), thn.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_wts, wts.data(), wts.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_nc, nc.data(), (size_t)SQ * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_lists, lists.data(), lists.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d_Sn, 0, (size_t)E * SQ * T_pad * 8, st));
  HIPCHK(hipMemsetAsync(d_err, 0, 8, st));
  MK_LAUNCH(k_kept_phi, dim3((unsigned)(((long)E * SQ + 255) / 256)), dim3(256), 0, st, md, d_thn, E, d_nphi);
  for (int e = 0; e < E; ++e) {
    int* SL = d_lists + (size_t)e * LS;   // subsets per outcome
    int* SC = SL + SQ;
    int* L = SC + q;                      // pairs
    int* C = L + SQ;
    mt.theta = d_thn + (size_t)e * S * nth;
    mt.s_pred = d_Sn + (size_t)e * SQ * T_pad;
    for (int h = 0; h < q; ++h) {
      launch_candidates(mt, g.ms, st, S, h, 1, 2, 0, SL + h * S, SC + h);
      launch_cholesky(s, g, h, 1, SL + h * S, SC + h);
    }
    MK_LAUNCH(k_flip_pairs, dim3((SQ + 255) / 256), dim3(256), 0, st, g.ms, L, C);
    launch_trinv(s, g, SQ, L, C);
    Group gp = g;
    gp.md = mt;
    gp.d_plist = L;
    gp.d_pcount = C;
    launch_pred_refresh(s, gp);
    HIPCHK(hipGetLastError());
    if (ri) {
      const int rc = regions_node(s, gp, *ri, e);
      if (rc) return rc;
    }
    if (e % 4 == 3) HIPCHK(hipStreamSynchronize(st));   // four slots are ~0.6 s of GEMMs at configs[4]
  }
  ck->Sn = d_Sn;
  ck->nphi = d_nphi;
  ck->wts = d_wts;
  ck->nc = d_nc;
  ck->nchk = nchk;
  ck->T_pad = T_pad;
  MK_LAUNCH(k_cheb_check, dim3(SQ * ((mt.n_test + 255) / 256)), dim3(256), 0, st, mt, *ck, d_err);
  unsigned long long eb = 0;
  HIPCHK(hipMemcpyAsync(&eb, d_err, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::memcpy(emax, &eb, 8);
  if (ri) {
    const int rc = regions_check(s, *ri, *ck, emax_regions);
    if (rc) return rc;
    if (!(*emax_regions <= *emax)) *emax = *emax_regions;   // the kernel turned a NaN into +inf
  }
  return 0;
}

static double cheb_tol() {
  const char* tenv = std::getenv("MK_KRIG_CHEB_TOL");
  return (tenv && *tenv) ? std::atof(tenv) : 1e-10;
}

// MK_KRIG_CHEB, read at every call (every session's tables, every tile): 0 never interpolate (the
// exact refresh / replay), 1 (default) auto -- where it saves exact evaluations, each caller's own
// rule --, -1 always, n > 1 always with n nodes.
static int cheb_mode() { return env_int("MK_KRIG_CHEB", 1); }

// Fused kriging by phi tables (called by mk_session_create before the initial factorisation; exponential,
// q = 1, one group).  The fused path refreshes X = W P^T at every kept iteration for the pairs whose phi
// changed (~0.4 of them at configs[2]: 6.9 ms of a kept iteration at 250 subsets).  Instead, s(t; phi)
// is computed once over the prior's whole phi range [a, b] (MK.R:63 phi.Unif), so it holds wherever the
// chain goes: Chebyshev nodes of [a, b] per subset, checked at a, b, the middle and the quarters (5
// points); a difference above MK_KRIG_CHEB_TOL keeps the exact refresh for the session (KS_KRIG_FALLBACK).
// Kept iterations then draw with g = W' z (one W pass) and the interpolated s (k_pred_tab_draw).
// Auto mode (cheb_mode): where the kept window's expected refreshes (0.25 n_kept per subset, below the
// amcmc target's 0.43) exceed the nodes and checks.
int mk::krig_tables(mk_session* s) {
  Model& md = s->md;
  s->kt.on = false;
  const int force_n = cheb_mode();
  const int S = s->S;
  if (force_n == 0 || s->tiled || md.n_test <= 0 || s->q != 1 || md.cov_model != MK_COV_EXPONENTIAL ||
      s->groups.size() != 1 || (int)s->span_pt_h.size() != S)
    return 0;
  const double pa = md.phi_a[0], pb = md.phi_b[0], eps = (pb - pa) * 1e-9;
  std::vector<double> lo(S, pa + eps), hi(S, pb - eps);
  std::vector<int> nc;
  std::vector<std::vector<double>> sphi;
  std::vector<double> wts;
  const int nchk = MK_CHEB_CHECKS_MAX;
  const int E = cheb_plan(s, lo, hi, force_n, nchk, nc, sphi, wts);
  double evals = 0.0;
  for (int i = 0; i < S; ++i) evals += nc[i] + nchk;
  if (force_n == 1 && 0.25 * md.n_kept * S <= evals) return 0;
  Model mt = md;   // every test site (the fused path's buffers hold them all)
  DevBufs scratch;
  ChebK ck;
  double emax = 0.0;
  const int rc = cheb_eval(s, mt, nc, sphi, wts, E, nchk, scratch, &ck, &emax);
  if (rc < 0) return rc;
  if (rc == MK_CHEB_EXACT) return 0;   // scratch memory short: exact refreshes
  s->kt.check = emax;
  if (!(emax <= cheb_tol())) {          // the check failed: exact refreshes
    s->kt.fail += 1;
    return 0;
  }
  // keep the node slots (the checks are not needed past this point)
  int nmax = 0;
  for (int i = 0; i < S; ++i) nmax = std::max(nmax, nc[i]);
  const size_t sn = (size_t)nmax * S * md.n_test_pad;
  double *Sn = nullptr, *nphi = nullptr, *w = nullptr;
  int* n = nullptr;
  if (s->alloc(&Sn, sn) || s->alloc(&nphi, (size_t)nmax * S) || s->alloc(&w, wts.size()) || s->alloc(&n, (size_t)S) ||
      s->alloc(&s->kt.g, (size_t)S * md.n_pad) || s->alloc(&s->kt.z, (size_t)S * (md.n_pad + 2))) {
    // HBM short: the session keeps the exact refresh (the tables are an optimisation, not a requirement)
    for (void* b : {(void*)Sn, (void*)nphi, (void*)w, (void*)n, (void*)s->kt.g, (void*)s->kt.z}) s->release(b);
    s->kt.g = s->kt.z = nullptr;
    set_err(0, "");
    return 0;
  }
  for (auto& e : s->kt.ev)
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return set_err(MK_E_HIP, "table event");
  HIPCHK(hipMemcpyAsync(Sn, ck.Sn, sn * 8, hipMemcpyDeviceToDevice, s->stream));
  HIPCHK(hipMemcpyAsync(nphi, ck.nphi, (size_t)nmax * S * 8, hipMemcpyDeviceToDevice, s->stream));
  HIPCHK(hipMemcpyAsync(w, ck.wts, wts.size() * 8, hipMemcpyDeviceToDevice, s->stream));
  HIPCHK(hipMemcpyAsync(n, ck.nc, (size_t)S * sizeof(int), hipMemcpyDeviceToDevice, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  s->kt.tab.Sn = Sn;
  s->kt.tab.nphi = nphi;
  s->kt.tab.wts = w;
  s->kt.tab.nc = n;
  s->kt.tab.nchk = 0;
  s->kt.tab.T_pad = md.n_test_pad;
  s->kt.evals = evals;
  s->kt.on = true;
  return 0;
}

// Tile [t0, t0 + Tc) of the tiled replay by phi interpolation, per (subset, outcome) pair sh = s q + h
// (under the LMC s_h, m_h and the normal are outcome h's own; A_k mixes them afterwards): nodes over each
// pair's kept phi_h range, checked at its ends and middle (a difference above MK_KRIG_CHEB_TOL, default
// 1e-10, at any pair and site sends the whole tile to the exact replay: KS_KRIG_FALLBACK); the mean
// m_k,h(t) = rho_t(phi_k,h)' g_k,h with g_k,h = W_k,h' z_k,h made once per kept window (the exact replay's
// factorisations where phi_h changed, one W' z per state and pair).  At configs[4] (q = 1): ~490 X
// refreshes per subset and tile become 13-21 nodes + 3 checks.  Auto mode (cheb_mode): where the nodes
// and checks of all pairs cost fewer exact evaluations than the exact replay's refreshes of all pairs.
// Returns 0, MK_CHEB_EXACT (the exact replay must run) or an error (< 0).
static int predict_tile_cheb(mk_session* s, int t0, double* dq, mk_outputs* o, double* dqp) {
  Model& md = s->md;
  const int force_n = cheb_mode();
  if (force_n == 0 || md.cov_model != MK_COV_EXPONENTIAL) return MK_CHEB_EXACT;
  // the joint covariance of a region needs X: the exact replay forms it at every state, this one at its nodes,
  // which serves the regions only on the route that asks for it
  const bool rint = s->regions.on && s->regions.route == MK_REGIONS_INTERP;
  if (s->regions.on && !rint) return MK_CHEB_EXACT;
  const int S = s->S, q = s->q, SQ = S * q, nth = md.n_theta, n_pad = md.n_pad;
  const int k_lo = s->win_lo, n_kept = s->win_n < 0 ? md.n_kept : s->win_n;
  if (n_kept < 1 || (int)s->span_pt_h.size() != S) return MK_CHEB_EXACT;
  const int T_pad = md.n_test_pad, Tc = std::min(s->pred_tile, s->n_test_all - t0);
  hipStream_t st = s->stream;
  Group g = s->all;
  s->la.next = -1;   // the replay factors into the free slots
  s->cov.pre = -1;
  // 1. phi_k,h of the window's kept states, [state][pair] (once per window)
  if (s->cg.iter != s->iter || s->cg.lo != k_lo || s->cg.n != n_kept) {
    s->release(s->cg.G);
    s->release(s->cg.phi);
    s->release(s->cg.phit);
    s->cg.G = s->cg.phi = s->cg.phit = nullptr;
    s->cg.iter = -1;
    if (s->alloc(&s->cg.phi, (size_t)n_kept * SQ)) return MK_CHEB_EXACT;
    MK_LAUNCH(k_kept_phi, dim3((unsigned)(((long)n_kept * SQ + 255) / 256)), dim3(256), 0, st, md,
              md.kth + (long)k_lo * S * nth, n_kept, s->cg.phi);
    s->cg.phi_h.assign((size_t)n_kept * SQ, 0.0);
    HIPCHK(hipMemcpyAsync(s->cg.phi_h.data(), s->cg.phi, (size_t)n_kept * SQ * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->cg.iter = s->iter;
    s->cg.lo = k_lo;
    s->cg.n = n_kept;
  }
  // 2. per pair: nodes over its kept phi range, inside its outcome's prior (a nearly fixed phi: a short
  //    interval around it)
  std::vector<double> lo(SQ), hi(SQ);
  long refreshes = 0;
  for (int i = 0; i < SQ; ++i) {
    const double pa = md.phi_a[i % q], pb = md.phi_b[i % q];
    double l = s->cg.phi_h[i], h = l;
    refreshes += 1;
    for (int j = 1; j < n_kept; ++j) {
      const double v = s->cg.phi_h[(size_t)j * SQ + i];
      refreshes += v != s->cg.phi_h[(size_t)(j - 1) * SQ + i];
      l = std::fmin(l, v);
      h = std::fmax(h, v);
    }
    const double mag = std::fmax(1.0, std::fabs(l));
    if (h - l < 1e-6 * mag) {
      const double c = 0.5 * (l + h);
      l = c - 5e-7 * mag;
      h = c + 5e-7 * mag;
    }
    const double eps = (pb - pa) * 1e-9;
    lo[i] = std::fmax(l, pa + eps);
    hi[i] = std::fmin(h, pb - eps);
  }
  std::vector<int> nc;
  std::vector<std::vector<double>> sphi;
  std::vector<double> wts;
  const int E = cheb_plan(s, lo, hi, force_n, MK_CHEB_CHECKS, nc, sphi, wts, rint ? s->regions.dmax : 0.0);
  long evals = 0;
  for (int i = 0; i < SQ; ++i) evals += nc[i] + MK_CHEB_CHECKS;
  // auto: only where it saves exact evaluations, summed over the pairs -- the exact replay refreshes a
  // pair's X at its first state and wherever its phi_h changed (a short window, e.g. the bench's 6-state
  // kriging sample, refreshes less often than a range needs nodes)
  if (force_n == 1 && evals >= refreshes) return MK_CHEB_EXACT;
  // 3. g_k = W_k' z_k of the window's kept states (once per window): the exact replay's
  //    factorisations where phi changed, then one W' z per state
  const int nkp = (n_kept + 7) / 8 * 8;
  if (!s->cg.G) {
    if (s->alloc(&s->cg.G, (size_t)SQ * n_pad * nkp)) return MK_CHEB_EXACT;
    if (s->alloc(&s->cg.phit, (size_t)SQ * nkp)) {
      s->release(s->cg.G);
      s->cg.G = nullptr;
      return MK_CHEB_EXACT;
    }
    std::vector<double> pt((size_t)SQ * nkp);
    for (int i = 0; i < SQ; ++i)
      for (int j = 0; j < nkp; ++j) pt[(size_t)i * nkp + j] = s->cg.phi_h[(size_t)std::min(j, n_kept - 1) * SQ + i];
    HIPCHK(hipMemcpyAsync(s->cg.phit, pt.data(), pt.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(s->cg.G, 0, (size_t)SQ * n_pad * nkp * 8, st));
    Model mt = md;
    for (int j = 0; j < n_kept; ++j) {
      const int k = k_lo + j;
      mt.theta = md.kth + (long)k * S * nth;
      const double* prev = j ? md.kth + (long)(k - 1) * S * nth : nullptr;
      MK_LAUNCH(k_kept_dirty, dim3(1), dim3(256), 0, st, mt, prev, s->d_slist, s->d_scount, g.d_plist, g.d_pcount);
      for (int h = 0; h < q; ++h) {
        launch_candidates(mt, g.ms, st, S, h, 1, 2, 0, s->d_slist + h * S, s->d_scount + h);
        launch_cholesky(s, g, h, 1, s->d_slist + h * S, s->d_scount + h);
      }
      MK_LAUNCH(k_flip_pairs, dim3((SQ + 255) / 256), dim3(256), 0, st, g.ms, g.d_plist, g.d_pcount);
      launch_trinv(s, g, SQ, g.d_plist, g.d_pcount);
      MK_LAUNCH(k_krig_g, dim3(SQ * (n_pad / 4)), dim3(256), 0, st, mt, g.ms, md.kz + (long)k * SQ * n_pad, s->cg.G,
                j, nkp);
      HIPCHK(hipGetLastError());
      // the host stays at most 32 states (~2,000 launches) ahead: rocprofv3's queue intercept read
      // past its packet buffer with tens of thousands queued
      if (j % 32 == 31) HIPCHK(hipStreamSynchronize(st));
    }
  }
  // 4. the tile's sites (as predict_tile), exact s at every slot, the check
  HIPCHK(hipMemsetAsync((void*)md.coords_test, 0, (size_t)2 * T_pad * 8, st));
  HIPCHK(hipMemcpyAsync((void*)md.coords_test, s->d_ct_all + t0, (size_t)Tc * 8, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync((void*)(md.coords_test + T_pad), s->d_ct_all + s->n_test_pad_all + t0, (size_t)Tc * 8,
                        hipMemcpyDeviceToDevice, st));
  Model mt = md;
  mt.n_kept = n_kept;
  mt.n_test = Tc;
  mt.t_off = t0;
  mt.ntt = (Tc + MK_NB - 1) / MK_NB;
  DevBufs scratch;
  RegionInterp ri;   // the regions' node, means and factor-chunk buffers: this replay's, and only on their route
  if (rint) {
    const int rb = regions_interp_begin(s, ri, t0, Tc, n_kept, E);
    if (rb) return rb;   // HBM short (MK_CHEB_EXACT: the tile runs exactly, as without the route) or an error
  }
  ChebK ck;
  double emax = 0.0, emax_regions = 0.0;
  const int rc = cheb_eval(s, mt, nc, sphi, wts, E, MK_CHEB_CHECKS, scratch, &ck, &emax, rint ? &ri : nullptr, &emax_regions);
  if (rc) return rc;
  if (!(emax <= cheb_tol())) {
    Stat& f = s->prof.stats[KS_KRIG_FALLBACK];
    f.launches += 1;
    f.ms = std::fmax(f.ms, std::isfinite(emax) ? emax : 1e300);
    return MK_CHEB_EXACT;
  }
  // 5. the draws
  void (*k_pred_cheb_draw_q)(Model, ChebK, const double*, const double*, const double*, const double*, int, int, double*) =
      rint ? (q == 1 ? k_pred_cheb_draw<1, true> : q == 2 ? k_pred_cheb_draw<2, true> : q == 3 ? k_pred_cheb_draw<3, true>
                                                                                               : k_pred_cheb_draw<4, true>)
           : (q == 1 ? k_pred_cheb_draw<1, false> : q == 2 ? k_pred_cheb_draw<2, false> : q == 3 ? k_pred_cheb_draw<3, false>
                                                                                                  : k_pred_cheb_draw<4, false>);
  MK_LAUNCH(k_pred_cheb_draw_q, dim3(S * ((Tc + 255) / 256)), dim3(256), 0, st, mt, ck, s->cg.G, s->cg.phit, md.coords,
            md.kA, k_lo, nkp, ri.means);
  HIPCHK(hipGetLastError());
  if (rint) {   // the factors of every chunk's phi runs and the regional draws, from the nodes' S and the means
    const int rr = regions_interp_draws(s, ri, mt, ck, n_kept);
    if (rr) return rr;
    s->regions.ran = MK_REGIONS_INTERP;
    s->regions.check = emax_regions;
  }
  Stat& c = s->prof.stats[KS_KRIG_CHEB];
  c.launches += 1;
  c.flops += (double)evals;
  c.ms = std::fmax(c.ms, emax);
  return tile_outputs(s, t0, dq, dqp, o, n_kept, s->q * Tc);
}

// spPredict after the fit (MK.R:87-89) over test-site tiles: replays the kriging of every kept
// iteration from the recorded chain states (z, theta, A).  A factor is recomputed only where
// (phi, nu) changed since the previous kept sample, with the same kernels and inputs as in the
// fit (rows < n_s of a factor do not depend on its border row), so the draws, the quantiles and
// their sum are bit-identical to the fused path.  Per tile the device holds q*T x kept draws
// per subset instead of q*n_test x kept.
// One tile [t0, t0 + Tc): the replay, then the tile's 200-level grids into dq ([S][q*Tc][200] in
// HBM, on s->stream; dqp: those of the predictive probabilities, from the same draws) and, if
// o->w_pred_samples / o->p_pred_samples, its draws to the host.  Returns after the stream is idle.
int mk::predict_tile(mk_session* s, int t0, double* dq, mk_outputs* o, double* dqp) {
  if ((dqp || (o && o->p_pred_samples)) && !s->d_xt) return set_err(MK_E_ARG, "predictive probabilities need x_test");
  if (s->diag_on && (s->diag_sink.p_predict || s->diag_sink.p_predict_worst) && !s->d_xt)
    return set_err(MK_E_ARG, "the diagnostics sink asks for p_predict: that needs x_test");
  // the flag of a lookahead candidate that no iteration will decide on is not a kept state's
  // (tile_outputs reads the flags after the replay)
  HIPCHK(hipMemsetAsync(s->md.info, 0, (size_t)s->S * s->q * sizeof(int), s->stream));
  if (s->regions.on) {   // until the interpolated route has served them
    s->regions.ran = MK_REGIONS_EXACT;
    s->regions.check = 0.0;
  }
  const int rc_cheb = predict_tile_cheb(s, t0, dq, o, dqp);
  if (rc_cheb != MK_CHEB_EXACT) return rc_cheb;
  Model& md = s->md;
  const int S = s->S, q = s->q;
  const int k_lo = s->win_lo, n_kept = s->win_n < 0 ? md.n_kept : s->win_n;   // kept states replayed
  const int T = s->pred_tile, T_pad = md.n_test_pad, n_test = s->n_test_all;
  const long C = (long)q * n_test;
  const int Tc = std::min(T, n_test - t0);
  const int Ct = q * Tc;
  hipStream_t st = s->stream;
  Group g = s->all;
  s->la.next = -1;   // the replay factors into the free slots: a lookahead candidate is gone
  s->cov.pre = -1;   // and so is an early-assembled one
  // nor is a flag of the interpolation nodes that sent this tile here
  HIPCHK(hipMemsetAsync(md.info, 0, (size_t)S * q * sizeof(int), st));
  HIPCHK(hipMemsetAsync((void*)md.coords_test, 0, (size_t)2 * T_pad * 8, st));
  HIPCHK(hipMemcpyAsync((void*)md.coords_test, s->d_ct_all + t0, (size_t)Tc * 8, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync((void*)(md.coords_test + T_pad), s->d_ct_all + s->n_test_pad_all + t0, (size_t)Tc * 8,
                        hipMemcpyDeviceToDevice, st));
  Model mt = md;
  mt.n_kept = n_kept;   // w_pred holds the window's draws
  mt.n_test = Tc;
  mt.t_off = t0;
  mt.ntt = (Tc + MK_NB - 1) / MK_NB;   // a short last tile: only its valid 128-site column blocks
                                        // (strides stay those of the full tile, n_test_pad)
  // q = 1 (MK_DRAW_RUNS, default on): a subset's draws wait until its X is about to change, and the
  // states of one phi run then read X once per 4 (k_pred_draw_runs; the same bits as per state)
  static const int runs_env = env_int("MK_DRAW_RUNS", 1);
  const bool runs = q == 1 && runs_env;
  const int per = (Tc + 3) / 4;
  if (runs) {
    int rc;
    if (!s->d_run_start && (rc = s->alloc(&s->d_run_start, (size_t)S))) return rc;
    HIPCHK(hipMemsetAsync(s->d_run_start, 0, (size_t)S * sizeof(int), st));
  }
  if (s->regions.on) {
    const int rc = regions_begin(s, t0, Tc, n_kept);
    if (rc) return rc;
  }
  for (int j = 0; j < n_kept; ++j) {
    const int k = k_lo + j;   // kept state k = iteration kept0 + k
    mt.theta = md.kth + (long)k * S * md.n_theta;
    mt.z = md.kz + (long)k * S * q * md.n_pad;
    mt.A_full = md.kA + (long)k * S * q * q;
    const double* prev = j ? md.kth + (long)(k - 1) * S * md.n_theta : nullptr;
    MK_LAUNCH(k_kept_dirty, dim3(1), dim3(256), 0, st, mt, prev, s->d_slist, s->d_scount, g.d_plist,
                       g.d_pcount);
    if (runs && j > 0) {   // the listed subsets' X changes now: their pending states first
      MK_LAUNCH(k_pred_draw_runs, dim3(S * per), dim3(256), 0, st, mt, md.kz, md.kA, k_lo, g.d_plist, g.d_pcount,
                s->d_run_start, j);
      MK_LAUNCH(k_run_start, dim3((S + 255) / 256), dim3(256), 0, st, g.d_plist, g.d_pcount, s->d_run_start, j);
    }
    for (int h = 0; h < q; ++h) {
      launch_candidates(mt, g.ms, st, S, h, 1, 2, 0, s->d_slist + h * S, s->d_scount + h);
      launch_cholesky(s, g, h, 1, s->d_slist + h * S, s->d_scount + h);
    }
    MK_LAUNCH(k_flip_pairs, dim3((S * q + 255) / 256), dim3(256), 0, st, g.ms, g.d_plist, g.d_pcount);
    launch_trinv(s, g, S * q, g.d_plist, g.d_pcount);
    g.md = mt;
    launch_pred_refresh(s, g);
    if (!runs) MK_LAUNCH(k_pred_draw, dim3(S * per), dim3(256), 0, st, mt, md.kept0 + k, j);
    HIPCHK(hipGetLastError());
    if (s->regions.on) {   // X is current for every subset: this state's factors where phi changed, then its regional draws
      const int rc = regions_state(s, g, mt, md.kept0 + k, j, n_kept);
      if (rc) return rc;
    }
  }
  if (runs && n_kept > 0) {   // every subset's last run
    MK_LAUNCH(k_pred_draw_runs, dim3(S * per), dim3(256), 0, st, mt, md.kz, md.kA, k_lo, (const int*)nullptr,
              (const int*)nullptr, s->d_run_start, n_kept);
    HIPCHK(hipGetLastError());
  }
  return tile_outputs(s, t0, dq, dqp, o, n_kept, Ct);
}

int mk::predict_tiled(mk_session* s, mk_outputs* o) {
  const int S = s->S, q = s->q;
  const int T = s->pred_tile, n_test = s->n_test_all;
  const long C = (long)q * n_test;
  hipStream_t st = s->stream;
  DevBufs scratch;
  double* dq = scratch.get<double>((size_t)S * q * T * MK_N_LEVELS);
  double* dsum = scratch.get<double>((size_t)q * T * MK_N_LEVELS);
  if (!dq || !dsum) return set_err(MK_E_NOMEM, "tiled kriging scratch");
  const bool grids = o->w_predict || o->w_predict_sum;
  const bool pgrids = o->p_predict || o->p_predict_sum;
  double* dqp = pgrids ? scratch.get<double>((size_t)S * q * T * MK_N_LEVELS) : nullptr;
  if (pgrids && !dqp) return set_err(MK_E_NOMEM, "tiled kriging scratch");
  for (int t0 = 0; t0 < n_test; t0 += T) {
    const int Ct = q * std::min(T, n_test - t0);
    int rc = predict_tile(s, t0, grids ? dq : nullptr, o, dqp);
    if (rc) return rc;
    // this tile's columns of every array, p before w; dsum serves both (stream order)
    if (pgrids && (rc = grids_to_host(s, dqp, Ct, (long)t0 * q, C, o->p_predict, o->p_predict_sum, dsum))) return rc;
    if (grids && (rc = grids_to_host(s, dq, Ct, (long)t0 * q, C, o->w_predict, o->w_predict_sum, dsum))) return rc;
    HIPCHK(hipStreamSynchronize(st));
  }
  return 0;
}

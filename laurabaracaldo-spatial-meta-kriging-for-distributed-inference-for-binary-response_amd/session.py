"""Host handle on one GPU shard of subsets (mk_session in include/mk.h).

This is the batched replacement of ``foreach(i=1:n.core) %dopar%
partitioned_spMvGLM(...)`` (MetaKriging_BinaryResponse.R:108): all subsets of
the shard live in HBM, every MCMC iteration advances all of them at once.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import Config, Problem, check, dptr, iptr
from .outbuf import (CriteriaBuffers, DiagnosticBuffers, LooBuffers, MapBuffers, OutputBuffers, PairBuffers, RegionBuffers,
                     ScoreBuffers, map_names, map_spec, pair_spec, region_spec, validation_arrays)

COV_MODELS = {"exponential": _lib.MK_COV_EXPONENTIAL, "matern": _lib.MK_COV_MATERN}
LINKS = {"logit": _lib.MK_LINK_LOGIT, "probit": _lib.MK_LINK_PROBIT}

# kernel-stat ids (mk_session.hpp)
(KS_CHOL_UPDATE, KS_CHOL_DIAG, KS_CHOL_TRSM, KS_SWEEP, KS_LAUUM, KS_ITER, KS_INV, KS_CHOL_UPDATE_SUB, KS_UPDATE_BUSY,
 KS_PRED_VAR, KS_COV, KS_SWEEP_FALLBACK, KS_KRIG_CHEB, KS_KRIG_FALLBACK) = range(14)
KS_DIAG = 14      # the chain-diagnostic launches (always timed; 0 launches unless diagnostics were asked for)
KS_CRIT = 15      # the model-assessment launches (always timed; 0 launches unless criteria were asked for)
KS_SCORE = 16     # the held-out scoring launches (always timed; 0 launches unless validation data were attached)
KS_MAPS = 17      # the posterior-map launches (always timed; 0 launches unless maps were asked for)
KS_PAIRS = 18     # the cross-outcome launches (always timed; 0 launches unless pairs were asked for)
KS_REGIONS = 19   # the areal-prediction launches (always timed; 0 launches unless regions were attached)
KS_LOO = 20       # the PSIS-LOO launches (always timed; 0 launches unless loo() was called)
KS_CKPT = 21      # the state-digest launches (always timed; 0 launches unless checkpoint(), restore() or digest() ran)


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


class SamplerConfig:
    """spMvGLM arguments of MK.R:56-64, 80-85 in one place (R names in comments)."""

    def __init__(self, q, p, beta_starting, beta_tuning, cov_model="exponential", n_batch=100, batch_length=50,
                 accept_rate=0.43, burn_in=None, phi_starting=None, phi_tuning=None, phi_unif=None,
                 A_starting=None, A_tuning=None, w_starting=0.0, w_tuning=0.5, nu_starting=None, nu_tuning=None,
                 nu_unif=None, K_IW_df=None, K_IW_S=None, seed=20250114, n_streams=0, predict_tile=0,
                 link="logit"):
        if cov_model not in COV_MODELS:
            raise ValueError(f"error: specified cov.model '{cov_model}' is not a valid option")
        if link not in LINKS:
            raise ValueError(f"error: link must be 'logit' (the reference) or 'probit', not '{link}'")
        self.link = link
        self.q, self.p = int(q), int(p)
        self.cov_model = cov_model
        self.n_batch, self.batch_length = int(n_batch), int(batch_length)
        self.n_samples = self.n_batch * self.batch_length
        self.accept_rate = float(accept_rate)
        self.burn_in = int(0.75 * self.n_samples) if burn_in is None else int(burn_in)   # MK.R:85
        bt = np.asarray(beta_tuning, dtype=np.float64)
        if bt.ndim == 2:
            bt = np.diag(bt)           # amcmc uses one scalar tuning per beta (build decision)
        if bt.shape != (self.p,):
            raise ValueError(f"error: beta tuning must be of length {self.p}")
        self.beta_starting = _f64(beta_starting).reshape(self.p)
        self.beta_tuning = _f64(bt)
        q = self.q
        self.phi_starting = _f64(np.full(q, 3.0 / 0.5) if phi_starting is None else phi_starting).reshape(q)
        self.phi_tuning = _f64(np.ones(q) if phi_tuning is None else phi_tuning).reshape(q)
        if phi_unif is None:
            phi_unif = (np.full(q, 3.0 / 0.75), np.full(q, 3.0 / 0.25))
        self.phi_a = _f64(phi_unif[0]).reshape(q)
        self.phi_b = _f64(phi_unif[1]).reshape(q)
        ntri = q * (q + 1) // 2
        if A_starting is None:   # diag(1,q)[lower.tri(diag(1,q), TRUE)]  (MK.R:56)
            A_starting = np.array([1.0 if i == j else 0.0 for j in range(q) for i in range(j, q)])
        self.A_starting = _f64(A_starting).reshape(ntri)
        self.A_tuning = _f64(np.full(ntri, 0.1) if A_tuning is None else A_tuning).reshape(ntri)
        self.w_starting, self.w_tuning = float(w_starting), float(w_tuning)
        matern = cov_model == "matern"
        if matern:
            self.nu_starting = _f64(np.full(q, 0.5) if nu_starting is None else nu_starting).reshape(q)
            self.nu_tuning = _f64(np.full(q, 0.1) if nu_tuning is None else nu_tuning).reshape(q)
            if nu_unif is None:
                nu_unif = (np.full(q, 0.1), np.full(q, 2.0))
            self.nu_a = _f64(nu_unif[0]).reshape(q)
            self.nu_b = _f64(nu_unif[1]).reshape(q)
        else:
            self.nu_starting = self.nu_tuning = self.nu_a = self.nu_b = None
        self.K_IW_df = float(q if K_IW_df is None else K_IW_df)
        self.K_IW_S = _f64(np.diag(np.full(q, 0.1)) if K_IW_S is None else K_IW_S).reshape(q, q)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.n_streams = int(n_streams)     # device execution only (0 = library default); no effect on results
        self.predict_tile = int(predict_tile)   # 0: kriging fused into kept iterations; else test sites per pass

    @property
    def n_theta(self):
        return self.q * (self.q + 1) // 2 + self.q * (2 if self.cov_model == "matern" else 1)

    @property
    def P(self):
        return self.p + self.n_theta

    @property
    def kept(self):
        return self.n_samples - self.burn_in + 1

    def to_c(self, device=0, record_w=False):
        keep = []

        def p_(a):
            if a is None:
                return None
            a = _f64(a)
            keep.append(a)
            return dptr(a)

        c = Config()
        c.cov_model = COV_MODELS[self.cov_model]
        c.n_batch, c.batch_length, c.accept_rate, c.burn_in = self.n_batch, self.batch_length, self.accept_rate, self.burn_in
        c.beta_starting, c.beta_tuning = p_(self.beta_starting), p_(self.beta_tuning)
        c.phi_starting, c.phi_tuning = p_(self.phi_starting), p_(self.phi_tuning)
        c.A_starting, c.A_tuning = p_(self.A_starting), p_(self.A_tuning)
        c.nu_starting, c.nu_tuning = p_(self.nu_starting), p_(self.nu_tuning)
        c.w_starting, c.w_tuning = self.w_starting, self.w_tuning
        c.phi_unif_a, c.phi_unif_b = p_(self.phi_a), p_(self.phi_b)
        c.nu_unif_a, c.nu_unif_b = p_(self.nu_a), p_(self.nu_b)
        c.K_IW_df = self.K_IW_df
        c.K_IW_S = p_(np.asfortranarray(self.K_IW_S).ravel(order="F"))
        c.seed = self.seed
        c.record_samples = 1
        c.record_w = 1 if record_w else 0
        c.device = int(device)
        c.n_streams = self.n_streams
        c.predict_tile = self.predict_tile
        c.link = LINKS[self.link]
        return c, keep


def _x_test(x_test, q, n_test, p):
    """x.test as libmk reads it ((q n_test) x p column-major, flat), or ValueError on another shape."""
    xt = np.asarray(x_test, dtype=np.float64)
    if xt.ndim != 2 or xt.shape != (q * n_test, p):
        raise ValueError(f"error: x_test must be (q*n_test) x p = {q * n_test} x {p}, not {xt.shape}")
    return _f64(xt.ravel(order="F"))


class PackedProblem:
    """mk_problem of a list of subsets (the R layout libmk reads: per subset column-major coords,
    location-major y / weights, (n_s q) x p design), with the arrays it points into kept alive.
    x_test: the test sites' covariates ((q n_test) x p, location-major rows), or None."""

    def __init__(self, subsets, cfg, coords_test=None, subset_base=0, x_test=None):
        self.n_part = np.ascontiguousarray([s["coords"].shape[0] for s in subsets], dtype=np.int32)
        self.S = len(subsets)
        self.coords = _f64(np.concatenate([np.asarray(s["coords"], float).ravel(order="F") for s in subsets]))
        self.y = _f64(np.concatenate([np.asarray(s["y"], float).ravel() for s in subsets]))
        self.weights = _f64(np.concatenate([np.asarray(s["weights"], float).ravel() for s in subsets]))
        self.x = _f64(np.concatenate([np.asarray(s["x"], float).reshape(-1, cfg.p).ravel(order="F") for s in subsets]))
        for s, ns in zip(subsets, self.n_part):
            if np.asarray(s["y"]).size != ns * cfg.q or np.asarray(s["x"]).shape != (ns * cfg.q, cfg.p):
                raise ValueError("error: subset y/x sizes must be n_s*q and (n_s*q) x p")
        self.n_test = 0 if coords_test is None else int(np.asarray(coords_test).shape[0])
        self.coords_test = None if coords_test is None else _f64(np.asarray(coords_test, float).ravel(order="F"))
        pr = Problem()
        pr.n_subsets, pr.subset_base, pr.q, pr.p = self.S, int(subset_base), cfg.q, cfg.p
        pr.n_part = iptr(self.n_part)
        pr.coords, pr.y, pr.weights, pr.x = dptr(self.coords), dptr(self.y), dptr(self.weights), dptr(self.x)
        pr.n_test = self.n_test
        pr.coords_test = dptr(self.coords_test) if self.coords_test is not None else None
        self.x_test = None if x_test is None else _x_test(x_test, cfg.q, self.n_test, cfg.p)
        pr.x_test = dptr(self.x_test)
        self.c = pr


class Session:
    """One shard of subsets resident on one GPU.

    subsets: list of dicts with 'coords' (n_s,2), 'y' (n_s*q,), 'weights' (n_s*q,), 'x' (n_s*q, p).
    """
    _fused = False

    def __init__(self, subsets, cfg, coords_test=None, subset_base=0, device=0, record_w=False, lookahead=None,
                 x_test=None, criteria=False):
        self.cfg = cfg
        self.q, self.p = cfg.q, cfg.p
        self._prob = PackedProblem(subsets, cfg, coords_test, subset_base, x_test=x_test)
        lib = _lib.load()
        self.n_part, self.S = self._prob.n_part, self._prob.S
        self.n_test, self.coords_test = self._prob.n_test, self._prob.coords_test
        self.x_test = self._prob.x_test          # the test sites' covariates (flat, column-major) or None
        pr = self._prob.c
        c, self._keep = cfg.to_c(device=device, record_w=record_w)
        self.record_w = record_w
        h = ctypes.c_void_p()
        check(lib.mk_session_create(ctypes.byref(pr), ctypes.byref(c), ctypes.byref(h)))
        self._h = h
        self._lib = lib
        self._window = None     # kept states of the next outputs(), once set_kept_window narrowed them
        self._map_thresholds = None     # set_maps' thresholds while maps are attached
        self._pair_thresholds = None    # set_pairs' thresholds while pairs are attached
        self._regions = None            # set_regions' (G, thresholds) while regions are attached
        # kriging fused into the kept iterations (mk_session_create's rule): a kept window then serves
        # criteria() alone, outputs() keeps every kept state
        self._fused = not (cfg.predict_tile > 0 and (self.n_test == 0 or cfg.predict_tile < self.n_test))
        try:
            if lookahead is not None:
                self.set_lookahead(lookahead)
            if criteria:                # in-chain DIC / WAIC sums from the first kept iteration on
                check(lib.mk_session_set_criteria(self._h, 1))
        except Exception:
            self.close()
            raise

    def run(self, n_iter):
        check(self._lib.mk_session_run(self._h, int(n_iter)))

    def chain_state(self, i):
        """Subset i's chain state now (mk_session_chain_state): beta, theta (A tri with log diagonal |
        logit phi | logit nu), w (n_s q), tune (log proposal sds) and accept (this batch's counts), in
        spMvGLM's MH order -- enough to resume the chain on another host at iteration `self.iteration`."""
        cfg = self.cfg
        nq = int(self.n_part[i]) * cfg.q
        nmh = cfg.p + cfg.n_theta + nq
        st = dict(beta=np.zeros(cfg.p), theta=np.zeros(cfg.n_theta), w=np.zeros(nq), tune=np.zeros(nmh),
                  accept=np.zeros(nmh))
        check(self._lib.mk_session_chain_state(self._h, int(i), dptr(st["beta"]), dptr(st["theta"]), dptr(st["w"]),
                                               dptr(st["tune"]), dptr(st["accept"])))
        st["iteration"] = self.iteration
        return st

    def notpd_counts(self):
        """(S, q) int64: per (subset, outcome), the phi / nu candidates rejected so far because their
        Cholesky factorisation met a pivot that is not > 0 (mk_session_notpd_counts)."""
        out = np.zeros((self.S, self.q), dtype=np.int64)
        check(self._lib.mk_session_notpd_counts(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def import_chain(self, samples, w_samples, acceptance=None):
        """A recorded chain into a session that never ran (mk_session_import_chain): afterwards the session
        serves outputs(), tile_grids(), set_test_sites() and every sink as one whose run() is complete.
        samples: per subset n_samples x P (p.beta.theta.samples: beta | lower-tri K | phi | nu), a list or one
        stacked array; w_samples: per subset (n_s q) x n_w, the w of the LAST n_w iterations (p.w.samples or
        its trailing columns; kept <= n_w <= n_samples, and n_samples when the session records w);
        acceptance: per subset n_batch x (P + 1), or None.  The session must keep chain states
        (predict_tile > 0, and no test sites or more than the tile).  MkError names the subset, the
        iteration and the column or row of a value the import refuses."""
        cfg = self.cfg
        sm = [np.asarray(a, dtype=np.float64) for a in samples]
        ws = [np.asarray(a, dtype=np.float64) for a in w_samples]
        if len(sm) != self.S or len(ws) != self.S:
            raise ValueError(f"error: import_chain needs samples and w_samples of {self.S} subsets")
        for i, a in enumerate(sm):
            if a.shape != (cfg.n_samples, cfg.P):
                raise ValueError(f"error: samples of subset {i} must be n_samples x P = {cfg.n_samples} x {cfg.P}, not {a.shape}")
        n_w = ws[0].shape[1] if ws[0].ndim == 2 else -1
        for i, a in enumerate(ws):
            if a.ndim != 2 or a.shape != (int(self.n_part[i]) * cfg.q, n_w):
                raise ValueError(f"error: w_samples of subset {i} must be (n_s q) x n_w = {int(self.n_part[i]) * cfg.q} x {n_w}, "
                                 f"not {a.shape}")
        c = _lib.Chain()
        hs = _f64(np.stack([a.T for a in sm]))
        hw = _f64(np.concatenate([a.T.ravel() for a in ws]))
        c.samples, c.w_samples, c.n_w = dptr(hs), dptr(hw), int(n_w)
        ha = None
        if acceptance is not None:
            ac = [np.asarray(a, dtype=np.float64) for a in acceptance]
            if len(ac) != self.S or any(a.shape != (cfg.n_batch, cfg.P + 1) for a in ac):
                raise ValueError(f"error: acceptance must be n_batch x (P + 1) = {cfg.n_batch} x {cfg.P + 1} per subset")
            ha = _f64(np.stack([a.T for a in ac]))
        c.acceptance = dptr(ha)
        check(self._lib.mk_session_import_chain(self._h, ctypes.byref(c)))

    @property
    def imported(self):
        """True once import_chain succeeded: the session replays a recorded chain, it cannot run()."""
        return bool(self._lib.mk_session_imported(self._h))

    def import_stats(self):
        """What the import cost (mk_session_import_stats): the (subset, outcome) factorisations it made and the
        milliseconds of the factor refreshes and of the z = W u launches."""
        n, a, b = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        check(self._lib.mk_session_import_stats(self._h, ctypes.byref(n), ctypes.byref(a), ctypes.byref(b)))
        return dict(factorisations=n.value, ms_factor=a.value, ms_z=b.value)

    def _ckpt_words(self, iteration=-1):
        w = np.zeros(_lib.CKPT_NFIELDS, dtype=np.int64)
        check(self._lib.mk_session_checkpoint_layout(self._h, int(iteration), w.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return w

    def checkpoint(self, first=0, count=None):
        """The state of subsets [first, first + count) after the iterations done so far (mk_session_checkpoint;
        the fields are listed in include/mk.h): a dict of numpy arrays -- 'iteration', 'words' (the words per
        subset of every field), every field of _lib.CKPT_FIELDS as (count, words) float64 ('notpd': int64) and
        'digests', (count q, 4) uint64, the digests of the pairs' factor buffers L, Winv, W, QB.  restore() of a
        session made over the same subsets and configuration takes it back and run() continues the chain bit for
        bit.  Only the rows of the record that exist are held."""
        count = self.S - int(first) if count is None else int(count)
        first = int(first)
        if first < 0 or count < 1 or first + count > self.S:
            raise ValueError(f"error: checkpoint of subsets ({first}, {count}) is outside the session's {self.S} subsets")
        words = self._ckpt_words()
        st = {"iteration": np.array(self.iteration), "words": words}
        c = _lib.Checkpoint()
        for f, name in enumerate(_lib.CKPT_FIELDS):
            st[name] = np.zeros((count, int(words[f])), dtype=np.int64 if name == "notpd" else np.float64)
            c.field[f] = st[name].ctypes.data if words[f] else None
        st["digests"] = np.zeros((count * self.q, _lib.CKPT_NDIGEST), dtype=np.uint64)
        c.digests = st["digests"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        check(self._lib.mk_session_checkpoint(self._h, first, count, ctypes.byref(c)))
        st["lookahead"] = np.array(bool(c.lookahead))      # the schedule that wrote the state
        return st

    def restore(self, state):
        """A checkpoint()'s state into this session, which must be as it was created: no iteration run, nothing
        imported, over the subsets the state holds and the configuration of the session that wrote it
        (mk_session_restore).  Afterwards `iteration` is the state's and run() continues the chain, on the schedule
        that wrote the state when it was written mid-chain (`lookahead` reports it); at n_samples
        the outputs and sinks are served.  The factors are re-derived from the restored theta and their digests
        compared with the state's: MkError names the pair and the buffer of a mismatch, and the session is then
        unusable.  MkError names the subset and the field of a size or a value the restore refuses."""
        for k in ["iteration", "words", "digests", "lookahead"] + _lib.CKPT_FIELDS:
            if k not in state:
                raise ValueError(f"error: the state lacks the key '{k}'")
        words = np.ascontiguousarray(np.asarray(state["words"], dtype=np.int64).reshape(-1))
        if words.shape != (_lib.CKPT_NFIELDS,):
            raise ValueError(f"error: the state's key 'words' has shape {words.shape}, not ({_lib.CKPT_NFIELDS},)")
        c = _lib.Checkpoint()
        keep = []
        for f, name in enumerate(_lib.CKPT_FIELDS):
            a = np.ascontiguousarray(np.asarray(state[name], dtype=np.int64 if name == "notpd" else np.float64))
            if a.shape != (self.S, int(words[f])):
                raise ValueError(f"error: the state's key '{name}' has shape {a.shape}; the session's {self.S} subsets and "
                                 f"the key 'words' give {(self.S, int(words[f]))}")
            keep.append(a)
            c.field[f] = a.ctypes.data if a.size else None
        dg = np.ascontiguousarray(np.asarray(state["digests"], dtype=np.uint64))
        if dg.shape != (self.S * self.q, _lib.CKPT_NDIGEST):
            raise ValueError(f"error: the state's key 'digests' has shape {dg.shape}, not {(self.S * self.q, _lib.CKPT_NDIGEST)}")
        c.digests = dg.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        c.lookahead = int(bool(state["lookahead"]))
        check(self._lib.mk_session_restore(self._h, int(state["iteration"]), words.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                           ctypes.byref(c)))

    def digest(self):
        """(S q, 4) uint64: the digests of every (subset, outcome) pair's factor buffers now -- L, Winv, W, QB over
        the region later iterations read (mk_session_digest; QB is 0 where the session's sweep keeps none)."""
        out = np.zeros((self.S * self.q, _lib.CKPT_NDIGEST), dtype=np.uint64)
        check(self._lib.mk_session_digest(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out

    def restore_stats(self):
        """What restore() cost in milliseconds (mk_session_restore_stats): the re-derivation of the factors, the
        digests (both by device events) and the uploads (host clock)."""
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(self._lib.mk_session_restore_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return dict(ms_derive=a.value, ms_digest=b.value, ms_upload=c.value)

    def set_test_sites(self, coords_test, x_test=None):
        """Kriging sites for the next outputs() of a session created with predict_tile > 0
        (its kept chain states were recorded during the run): spPredict without refitting.
        x_test ((q n_test) x p): their covariates, for the predictive probabilities; the covariates
        of the earlier sites are dropped either way."""
        ct = np.asarray(coords_test, float).reshape(-1, 2)
        xt = None if x_test is None else _x_test(x_test, self.q, int(ct.shape[0]), self.p)
        self.n_test = int(ct.shape[0])
        self.coords_test = _f64(ct.ravel(order="F"))
        self.x_test = None
        self._map_thresholds = None     # the library detaches the maps with the sites
        self._pair_thresholds = None    # and the pairs
        self._regions = None            # and the regions
        check(self._lib.mk_session_set_test_sites(self._h, self.n_test, dptr(self.coords_test)))
        if xt is not None:
            self.set_test_covars(xt, _flat=True)

    def set_test_covars(self, x_test, _flat=False):
        """Covariates ((q n_test) x p) of the current test sites (mk_session_set_test_covars)."""
        xt = x_test if _flat else _x_test(x_test, self.q, self.n_test, self.p)
        check(self._lib.mk_session_set_test_covars(self._h, dptr(xt)))
        self.x_test = xt

    def grids_device(self, which, out_ptr):
        """Write the shard's (S, C, 200) grids -- which 0 parameters, 1 w.predict, 2 p.predict -- into device memory
        at out_ptr (HBM of the session's device, e.g. a torch CUDA tensor's data_ptr()): the
        device-resident combine's input, no host round trip."""
        check(self._lib.mk_session_grids(self._h, int(which), ctypes.c_void_p(int(out_ptr)), 1))

    def _diag_buffers(self, draws=True):
        """Buffers for every diagnostics field this session can fill: the parameters and, with draws,
        the w draws when it has test sites and the p draws when it also has their covariates."""
        kinds = ["parameters"] + (["w_predict"] if draws and self.n_test else []) + \
            (["p_predict"] if draws and self.n_test and self.x_test is not None else [])
        return DiagnosticBuffers(self.S, self.cfg, self.n_test, {k + sfx for k in kinds for sfx in ("_diag", "_diag_worst")})

    def tile_grids(self, t0, prob=False, diagnostics=False):
        """Tiled session (predict_tile > 0), after the run: (S, 200, q*Tc) w.predict grids of test
        sites [t0, t0 + Tc) -- one tile's kriging replay only (configs[4]'s per-tile combine).
        prob=True: (w grids, p.predict grids) of the same replay (needs x_test).
        diagnostics=True: the return value gains a last element, the dict of this tile's chain
        diagnostics from the same replay -- 'w_predict_diag' (per subset 3 x q*Tc: ess, mcse, rhat),
        'w_predict_diag_worst' (3 x q*Tc) and, with x_test, the 'p_predict_*' pair."""
        if diagnostics:
            db = self._diag_buffers()
            sink = [f for f in db.buf if not f.startswith("parameters")]
            check(self._lib.mk_session_set_diagnostics(self._h, ctypes.byref(db.struct(sink))))
            try:
                res = self.tile_grids(t0, prob=prob)
            finally:
                check(self._lib.mk_session_set_diagnostics(self._h, None))
            c0 = int(t0) * self.q
            c1 = c0 + self.q * min(self.predict_tile, self.n_test - int(t0))
            d = {f: ([a[:, c0:c1] for a in v] if isinstance(v, list) else v[:, c0:c1])
                 for f, v in db.unpack().items() if f in sink}
            return (res if isinstance(res, tuple) else (res,)) + (d,)
        T = self.predict_tile
        Tc = min(T, self.n_test - int(t0))
        out = np.zeros((self.S, self.q * Tc, _lib.N_LEVELS))
        if not prob:
            check(self._lib.mk_session_tile_grids(self._h, int(t0), out.ctypes.data_as(ctypes.c_void_p), 0))
            return np.ascontiguousarray(np.transpose(out, (0, 2, 1)))
        outp = np.zeros_like(out)
        check(self._lib.mk_session_tile_grids_wp(self._h, int(t0), out.ctypes.data_as(ctypes.c_void_p),
                                                 outp.ctypes.data_as(ctypes.c_void_p), 0))
        return (np.ascontiguousarray(np.transpose(out, (0, 2, 1))), np.ascontiguousarray(np.transpose(outp, (0, 2, 1))))

    def set_kept_window(self, first, last):
        """Replay only iterations first..last (1-based; spPredict's start / end) in the next outputs()."""
        check(self._lib.mk_session_set_kept_window(self._h, int(first), int(last)))
        self._window = int(last) - int(first) + 1

    def criteria(self, thin=1, pointwise=False):
        """DIC and WAIC per subset after the run (mk_session_criteria; the definitions are in
        include/mk.h): {'subsets': (S, 8), 'total': (8,) their sums in subset order, 'names': the rows
        -- bar.D, D.bar.Omega, pD, DIC, lppd, p.waic, WAIC, lconst}; pointwise=True adds 'pointwise', per
        subset (n_s q) x 2: lppd_i and the Welford variance term of p.waic.  A session made with
        criteria=True closes its in-chain sums (kept states burn_in..n.samples); with a kept window
        (set_kept_window), thin > 1 or no in-chain sums the recorded chain is replayed, which needs
        record_w.  The likelihood drops the binomial coefficient: lconst is what full-likelihood
        figures add (-2 lconst to the deviance rows and WAIC, + lconst to lppd)."""
        cb = CriteriaBuffers(self.S, self.q, self.n_part, pointwise=pointwise)
        check(self._lib.mk_session_criteria(self._h, int(thin), ctypes.byref(cb.c)))
        return cb.unpack()

    def loo(self, thin=1, pointwise=False):
        """PSIS-LOO per subset after the run (mk_session_loo; the definitions are in include/mk.h):
        {'subsets': (S, 8), 'total': (8,), 'names': the rows -- elpd_loo, p_loo, looic, se_elpd_loo, lppd,
        k_max, n_k_bad, lconst}; pointwise=True adds 'pointwise', per subset (n_s q) x 3: elpd_loo_i, the
        Pareto shape k-hat_i (above 0.7 the term is not reliable) and lppd_i.  Always replays the recorded
        chain (record_w) over criteria()'s window and thin: 25 .. 8192 states."""
        lb = LooBuffers(self.S, self.q, self.n_part, pointwise=pointwise)
        check(self._lib.mk_session_loo(self._h, int(thin), ctypes.byref(lb.c)))
        return lb.unpack()

    def set_validation(self, y_test, weights_test=1):
        """Attach held-out outcomes at the current test sites (mk_session_set_validation): y_test
        (q*n_test, location-major like x_test) successes of weights_test trials (1: binary; 0 marks a
        column that was not observed).  Needs test sites and x_test.  scores() then gives the log score,
        Brier score and error rate per subset; a tiled session scores each tile from the replay that
        makes its grids (outputs(), tile_grids()).  y_test=None detaches; so does set_test_sites."""
        if y_test is None:
            check(self._lib.mk_session_set_validation(self._h, None))
            return
        _y, _wt, v = validation_arrays(y_test, weights_test, self.q * self.n_test)
        check(self._lib.mk_session_set_validation(self._h, ctypes.byref(v)))      # copied to HBM

    def scores(self, pointwise=False):
        """Held-out scores per subset after the run (mk_session_scores; the definitions are in
        include/mk.h): {'subsets': (S, 5), 'names': the rows -- n (columns with trials), lpd (the log
        predictive density of the held-out outcomes, binomial coefficient dropped), brier, err (share of
        held-out trials the rule pmean >= 0.5 gets wrong), lconst (what full-likelihood log scores add)};
        pointwise=True adds 'pointwise', per subset (q n_test) x 2: the posterior predictive mean
        pmean_c of p(y = 1) and lpd_c.  A tiled session must have replayed every tile since
        set_validation (MkError naming the first missing tile otherwise)."""
        sb = ScoreBuffers(self.S, self.q * self.n_test, pointwise=pointwise)
        check(self._lib.mk_session_scores(self._h, ctypes.byref(sb.c)))
        return sb.unpack()

    def set_maps(self, thresholds=()):
        """Ask for the posterior maps at the current test sites (mk_session_set_maps): per test column the
        mean and sd of w and of p(y = 1) and, per threshold u (probability scale, at most 8), the
        posterior probability that p > u.  Needs test sites and x_test.  maps() then gives the planes; a
        tiled session fills each tile's columns from the replay that makes its grids (outputs(),
        tile_grids()).  thresholds=None detaches; so does set_test_sites."""
        self._map_thresholds = None
        if thresholds is None:
            check(self._lib.mk_session_set_maps(self._h, None))
            return
        u, m = map_spec(thresholds)
        check(self._lib.mk_session_set_maps(self._h, ctypes.byref(m)))
        self._map_thresholds = u

    def maps(self):
        """The posterior maps per subset after the run (mk_session_maps; the definitions are in
        include/mk.h): {'names': w_mean, w_sd, p_mean, p_sd, exc_1..J, 'thresholds', 'subsets': per subset
        (q n_test) x (4 + J)}.  A tiled session must have replayed every tile over the current kept window
        since set_maps (MkError naming the first missing tile otherwise)."""
        u = self._map_thresholds if self._map_thresholds is not None else np.zeros(0)
        mb = MapBuffers(self.S, self.q * self.n_test, u.size)
        check(self._lib.mk_session_maps(self._h, ctypes.byref(mb.c)))
        return mb.unpack(u)

    def set_pairs(self, thresholds=()):
        """Ask for the cross-outcome outputs at the current test sites (mk_session_set_pairs; q >= 2): per
        site and pair of outcomes (a, b) the 200-level grids of p_a p_b (both occur) and p_a - p_b, and the
        planes both_mean, both_sd, diff_mean, diff_sd, corr, a_gt_b and, per threshold u (at most 8), the
        posterior probability that p_a > u and p_b > u.  Needs test sites and x_test.  pairs() then gives
        them; a tiled session fills each tile's pair columns from the replay that makes its grids
        (outputs(), tile_grids()).  thresholds=None detaches; so does set_test_sites."""
        self._pair_thresholds = None
        if thresholds is None:
            check(self._lib.mk_session_set_pairs(self._h, None))
            return
        u, m = pair_spec(thresholds)
        check(self._lib.mk_session_set_pairs(self._h, ctypes.byref(m)))
        self._pair_thresholds = u

    def pairs(self, grids=True, planes=True):
        """The cross-outcome outputs per subset after the run (mk_session_pairs; the definitions are in
        include/mk.h): {'names': both_mean, both_sd, diff_mean, diff_sd, corr, a_gt_b, joint_1..J, 'pairs': the
        (a, b) list in column order, 'thresholds', 'both_predict' / 'diff_predict': per subset 200 x C2,
        'subsets': per subset C2 x (6 + J)}, C2 = n_pairs n_test pair columns, site-major.  grids=False /
        planes=False leave that part out (a fused session then does not compute it).  A tiled session must
        have replayed every tile over the current kept window since set_pairs (MkError naming the first
        missing tile otherwise)."""
        u = self._pair_thresholds if self._pair_thresholds is not None else np.zeros(0)
        pb = PairBuffers(self.S, self.q, self.n_test, u.size, grids=grids, planes=planes)
        check(self._lib.mk_session_pairs(self._h, ctypes.byref(pb.c)))
        return pb.unpack(u)

    def set_regions(self, offsets, weights=None, thresholds=(), interpolate=False):
        """Attach regions to the current test sites (mk_session_set_regions): offsets[0..G] cuts the sites, in
        their order, into G contiguous runs of at most 128; weights (one per site, default equal) make the
        regional prevalence r = sum_i omega_i p_i of joint kriging draws of the region's sites; thresholds (at
        most 8) give the posterior probability that r > u.  Needs a session created with predict_tile > 0 whose
        tile holds every test site, x_test and recorded samples.  regions() then gives the outputs of the
        replay that makes the grids (outputs(), tile_grids()).  offsets=None detaches; so does set_test_sites.
        interpolate=True (mk_session_set_regions_route, MK_REGIONS_INTERP) lets that replay interpolate over phi
        wherever it would without regions (exponential models, MK_KRIG_CHEB's rule, the checks passed) and
        serves the regions from it; the default is the exact replay.  Every attach starts from the default."""
        if not isinstance(interpolate, (bool, np.bool_)):
            raise TypeError("error: interpolate must be True or False")
        self._regions = None
        if offsets is None:
            check(self._lib.mk_session_set_regions(self._h, None))
            return
        off, _w, u, m = region_spec(offsets, self.n_test, weights, thresholds)
        check(self._lib.mk_session_set_regions(self._h, ctypes.byref(m)))
        self._regions = (int(off.size - 1), u)
        if interpolate:
            check(self._lib.mk_session_set_regions_route(self._h, _lib.REGIONS_INTERP))

    def regions(self, samples=False):
        """The areal prediction per subset after a replay (mk_session_regions; the definitions are in
        include/mk.h): {'names': mean, sd, exc_1..J, 'thresholds', 'region_predict': per subset 200 x C3,
        'subsets': per subset C3 x (2 + J), 'singular': per subset C3 counts of kept states whose factor was
        flagged, 'timing_ms'}, C3 = G q region columns (region-major); samples=True adds 'region_samples' (per
        subset C3 x kept).  'route' is the route the replay took ("exact" or "interpolated": a replay that
        could not interpolate ran exactly) and 'check' the interpolated route's largest |interpolant - exact| over
        the entries of the regions' covariances at its check slots (0.0 on the exact route).  The tile must have
        been replayed over the current kept window since set_regions (MkError otherwise)."""
        G, u = self._regions if self._regions is not None else (0, np.zeros(0))
        kept = self.cfg.kept if self._window is None else self._window
        rb = RegionBuffers(self.S, self.q, G, u.size, kept, samples=samples)
        check(self._lib.mk_session_regions(self._h, ctypes.byref(rb.c)))
        ran, chk = ctypes.c_int32(), ctypes.c_double()
        check(self._lib.mk_session_regions_route(self._h, None, ctypes.byref(ran), ctypes.byref(chk)))
        out = rb.unpack(u)
        out["route"], out["check"] = _lib.REGION_ROUTE_NAMES[ran.value], chk.value
        return out

    def set_lookahead(self, mode):
        """Launch schedule before the first run: True / 1 lookahead (the next iteration's phi
        candidates factored while this iteration's inverse and sweep run), False / 0 sequential,
        -1 the library default.  The chain is the same either way (to rounding)."""
        check(self._lib.mk_session_set_lookahead(self._h, int(mode)))

    @property
    def lookahead(self):
        return bool(self._lib.mk_session_lookahead(self._h))

    @property
    def iteration(self):
        return self._lib.mk_session_iteration(self._h)

    @property
    def predict_tile(self):
        """Test sites per kriging tile in use (0: fused): cfg.predict_tile, or smaller where the tile's
        kriging buffers would not fit in HBM (the draws do not depend on it)."""
        return int(self._lib.mk_session_predict_tile(self._h))

    def profile(self, on=True, kinds=None, every=1):
        """Per-kernel HIP-event timing from the next run on: every kind, or only `kinds`
        (KS_* constants; fewer events in the stream); every > 1 brackets only the launches of every
        every-th iteration (a sample: per-launch events cost ~4 % of the rate at 32 subsets)."""
        check(self._lib.mk_session_profile_every(self._h, int(every)))
        if not on:
            v = 0
        elif kinds is None:
            v = 1
        else:
            v = 0
            for k in kinds:
                v |= 2 << int(k)
        check(self._lib.mk_session_profile(self._h, v))

    def kernel_stats(self, which):
        n = ctypes.c_int64()
        ms = ctypes.c_double()
        fl = ctypes.c_double()
        check(self._lib.mk_session_kernel_stats(self._h, which, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)))
        return dict(launches=n.value, ms=ms.value, flops=fl.value)

    def outputs(self, quantiles=True, samples=False, w_samples=False, w_pred_samples=False, acceptance=False,
                w_predict_sum=False, w_predict=True, p_predict=None, p_pred_samples=False, p_predict_sum=False,
                diagnostics=False):
        """quantiles: obj[[i]]$parameters (and $w.predict unless w_predict=False -- at 1M test sites the
        per-subset grids are 1.6 GB each; w_predict_sum gives this shard's term of the combine).
        p_predict / p_pred_samples / p_predict_sum: the same three of p(y = 1) = linkinv(x.test beta + w)
        per kept state (they need x_test); p_predict defaults to on when quantiles is and the session has
        covariates.
        diagnostics: adds the chain diagnostics of the kept states (the kept window when one is set) --
        'parameters_diag', 'w_predict_diag', 'p_predict_diag': per subset 3 x C arrays, rows ess (Geyer's
        initial monotone sequence), mcse (of the column mean) and split R-hat -- and the three
        '*_diag_worst' arrays (3 x C: min ess, max mcse, max rhat over the subsets).  A tiled session
        diagnoses each tile's draws from the replay that makes its grids; diagnostics="parameters"
        leaves the kriging draws out."""
        have = bool(self.n_test)       # the w outputs are simply absent without test sites
        if p_predict is None:
            p_predict = bool(quantiles) and self.x_test is not None and have
        on = dict(parameters=quantiles, w_predict=quantiles and w_predict and have, samples=samples,
                  w_samples=w_samples, w_pred_samples=w_pred_samples and have, acceptance=acceptance,
                  w_predict_sum=w_predict_sum and have, p_predict=p_predict, p_pred_samples=p_pred_samples,
                  p_predict_sum=p_predict_sum)
        kept = self.cfg.kept if self._window is None or self._fused else self._window
        fields = {f for f, v in on.items() if v}
        if not diagnostics:
            ob = OutputBuffers(self.S, self.cfg, self.n_part, self.n_test, kept, fields)
            check(self._lib.mk_session_outputs(self._h, ctypes.byref(ob.c)))
            return ob.unpack()
        db = self._diag_buffers(draws=diagnostics != "parameters")
        sink = [f for f in db.buf if not f.startswith("parameters")] if self.predict_tile else []
        replays = {"w_predict", "w_pred_samples", "w_predict_sum", "p_predict", "p_pred_samples", "p_predict_sum"}
        extra = {"w_predict_sum"} if sink and not (fields & replays) else set()    # the sink needs the tile replays
        ob = OutputBuffers(self.S, self.cfg, self.n_part, self.n_test, kept, fields | extra)
        if sink:
            check(self._lib.mk_session_set_diagnostics(self._h, ctypes.byref(db.struct(sink))))
        try:
            check(self._lib.mk_session_outputs(self._h, ctypes.byref(ob.c)))
        finally:
            if sink:
                check(self._lib.mk_session_set_diagnostics(self._h, None))
        direct = db.struct([f for f in db.buf if f not in sink])
        check(self._lib.mk_session_diagnostics(self._h, ctypes.byref(direct)))
        out = {f: v for f, v in ob.unpack().items() if f in fields}
        out.update(db.unpack())
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mk_session_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def combine(grids, device=0, mean=True):
    """MK.R:123-133 on device: (grid_1 + ... + grid_K)/K in the reference's sequential order
    (mean=False: the sum only -- a shard's term of the combine)."""
    lib = _lib.load()
    g = _f64(np.stack([np.asarray(x, float) for x in grids]))
    K = g.shape[0]
    out = np.zeros(g.shape[1:])
    fn = lib.mk_combine if mean else lib.mk_combine_sum
    check(fn(dptr(g.reshape(K, -1)), K, int(np.prod(g.shape[1:])), dptr(out), int(device)))
    return out


def digest(words, device=0):
    """The 64-bit state digest of a sequence of 8-byte words on the device (mk_digest; the kernel the sessions'
    checkpoints use): D = sum_i mix(x_i + (i + 1) 0x9E3779B97F4A7C15) mod 2^64, mix the splitmix64 finaliser.
    words: an array of float64, int64 or uint64, taken in C order by its bit patterns.  0 for no words."""
    lib = _lib.load()
    a = np.asarray(words)
    if a.dtype not in (np.float64, np.int64, np.uint64):
        raise ValueError(f"error: digest takes 8-byte words (float64, int64 or uint64), not {a.dtype}")
    a = np.ascontiguousarray(a).reshape(-1)
    out = ctypes.c_uint64()
    check(lib.mk_digest(a.ctypes.data if a.size else None, int(a.size), int(device), ctypes.byref(out)))
    return int(out.value)


def chain_diagnostics(x, axis=0, device=0):
    """ess, mcse and split R-hat of caller-given chains on the device (mk_chain_diagnostics; the
    kernel the sessions use).  x: 2-d, time along `axis`, one chain per index of the other axis (a
    coda mcmc matrix such as p.beta.theta.samples is axis=0; p.w.samples is axis=1).  Returns 3 x C."""
    lib = _lib.load()
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("error: chain_diagnostics takes a 2-d array")
    chains = _f64(x.T if axis in (0, -2) else x)             # one contiguous chain per row
    C, n = chains.shape
    out = np.zeros((C, _lib.N_DIAG))
    check(lib.mk_chain_diagnostics(dptr(chains), int(n), int(C), dptr(out), int(device)))
    return out.T.copy()


def score_grid(p, y, weights=1, pointwise=False, device=0):
    """Held-out scores of a grid of probabilities on the device (mk_score_grid; the kernels the sessions
    use): p is n_rows x C, its rows equally weighted states of p(y = 1) per test column -- the combined
    200-level grid result3, say; y (C) successes of weights trials.  Returns the row by name (n, lpd,
    brier, err, lconst) and, with pointwise, 'pointwise' (C x 2: pmean_c, lpd_c)."""
    lib = _lib.load()
    p = np.asarray(p, dtype=np.float64)
    if p.ndim != 2:
        raise ValueError("error: score_grid takes a 2-d array (states x columns)")
    n, C = p.shape
    cols = _f64(p.T)                                          # one contiguous column of states per row
    yv, wt, _v = validation_arrays(y, weights, C)
    pw = np.zeros((2, C)) if pointwise else None
    row = np.zeros(_lib.N_SCORE)
    check(lib.mk_score_grid(dptr(cols), int(n), int(C), dptr(yv), dptr(wt), dptr(pw), dptr(row), int(device)))
    out = dict(zip(_lib.SCORE_NAMES, row.tolist()))
    if pointwise:
        out["pointwise"] = pw.T.copy()
    return out


def psis_loo(ell, pointwise=True, device=0):
    """PSIS-LOO of a matrix of log-likelihood terms on the device (mk_loo_matrix; the kernel the sessions
    use): ell is n_states x n_obs, its rows equally weighted states -- a chain from other software, say.
    Returns the row by name (elpd_loo, p_loo, looic, se_elpd_loo, lppd, k_max, n_k_bad, lconst = 0) and,
    with pointwise, 'pointwise' (n_obs x 3: elpd_loo_i, k-hat_i, lppd_i).  25 .. 8192 states."""
    lib = _lib.load()
    e = np.asarray(ell, dtype=np.float64)
    if e.ndim != 2:
        raise ValueError("error: psis_loo takes a 2-d array (states x observations)")
    n, N = e.shape
    cols = _f64(e.T)                                          # one contiguous row of states per observation
    pw = np.zeros((3, N)) if pointwise else None
    row = np.zeros(_lib.N_LOO)
    check(lib.mk_loo_matrix(dptr(cols), int(N), int(n), dptr(pw), dptr(row), int(device)))
    out = dict(zip(_lib.LOO_NAMES, row.tolist()))
    if pointwise:
        out["pointwise"] = pw.T.copy()
    return out


def loo_compare(a, b):
    """Two PSIS-LOO results with pointwise values over the same observations (Session.loo(pointwise=True),
    spLoo, psis_loo): {'elpd_diff': sum_i (a_i - b_i), 'se_diff': sqrt(N var_i (a_i - b_i)) with the N - 1
    denominator, 'n_k_bad': observations whose k-hat exceeds 0.7 in either fit}.  Positive favours a."""
    def pw(r):
        if not isinstance(r, dict) or "pointwise" not in r:
            raise ValueError("error: loo_compare needs results with pointwise values (pointwise=True)")
        p = r["pointwise"]
        return np.concatenate(p, axis=0) if isinstance(p, (list, tuple)) else np.asarray(p)
    pa, pb = pw(a), pw(b)
    if pa.shape != pb.shape or pa.ndim != 2 or pa.shape[1] != 3:
        raise ValueError(f"error: loo_compare needs the same observations in both fits, not {pa.shape} and {pb.shape}")
    d = pa[:, 0] - pb[:, 0]
    N = d.size
    se = float(np.sqrt(N * np.sum((d - d.mean()) ** 2) / (N - 1))) if N > 1 else float("nan")
    return {"elpd_diff": float(d.sum()), "se_diff": se, "n_k_bad": int(np.sum((pa[:, 1] > 0.7) | (pb[:, 1] > 0.7)))}


def map_grid(grid, thresholds=(), device=0):
    """Mean, sd and exceedance probabilities of a grid on the device (mk_map_grid; the kernel the sessions
    use): grid is n_rows x C, its rows equally weighted states per column -- the combined 200-level grids
    result2 or result3, say.  Returns {'names': mean, sd, exc_1..J, 'thresholds', 'planes': C x (2 + J)}: the
    sd is Welford's over the rows in order (NaN for one row), exc_j the share of rows > thresholds[j]."""
    lib = _lib.load()
    g = np.asarray(grid, dtype=np.float64)
    if g.ndim != 2:
        raise ValueError("error: map_grid takes a 2-d array (states x columns)")
    n, C = g.shape
    cols = _f64(g.T)                                          # one contiguous column of states per row
    u, _m = map_spec(thresholds)
    out = np.zeros((2 + u.size, C))
    check(lib.mk_map_grid(dptr(cols), int(n), int(C), dptr(u) if u.size else None, int(u.size), dptr(out), int(device)))
    return {"names": map_names(u.size, ("mean", "sd")), "thresholds": u.tolist(), "planes": out.T.copy()}


def correlation_batched(coords, phi, nu=None, cov_model="exponential", device=0):
    """R_k = rho(|s_i - s_j|) for a batch of point sets (coords (S, n, 2))."""
    lib = _lib.load()
    coords = np.asarray(coords, float)
    S, n, _ = coords.shape
    c = _f64(np.stack([coords[i].ravel(order="F") for i in range(S)]))
    ph = _f64(np.broadcast_to(np.asarray(phi, float), (S,)))
    nv = None if nu is None else _f64(np.broadcast_to(np.asarray(nu, float), (S,)))
    out = np.zeros((S, n, n))
    check(lib.mk_correlation_batched(dptr(c), S, n, dptr(ph), dptr(nv) if nv is not None else None,
                                     COV_MODELS[cov_model], dptr(out), int(device)))
    return np.ascontiguousarray(np.transpose(out, (0, 2, 1)))   # column-major -> (S, n, n) row-major


def correlation_cross_batched(coords, phi, nu=None, cov_model="exponential", coords_test=None, stored_tables=False,
                              want_R=True, device=0):
    """(R, PT) of a batch of point sets by the session's own kernels (mk_correlation_cross_batched): R (S, n, n)
    between the sites coords (S, n, 2) by the candidate kernel (None unless want_R), PT (S, n, n_test) from
    them to the sets' own test sites coords_test (S, n_test, 2) by the kriging kernels (None without test
    sites).  stored_tables: the Matern Chebyshev tables as a session has them -- bounded by phi x the sites'
    extent, stored by their own kernels and loaded by the tile workgroups; else built in the kernels,
    unbounded (correlation_batched's configuration)."""
    lib = _lib.load()
    coords = np.asarray(coords, float)
    S, n, _ = coords.shape
    c = _f64(np.stack([coords[i].ravel(order="F") for i in range(S)]))
    ph = _f64(np.broadcast_to(np.asarray(phi, float), (S,)))
    nv = None if nu is None else _f64(np.broadcast_to(np.asarray(nu, float), (S,)))
    ct, n_test, PT = None, 0, None
    if coords_test is not None:
        coords_test = np.asarray(coords_test, float)
        if coords_test.ndim != 3 or coords_test.shape[0] != S or coords_test.shape[2] != 2:
            raise ValueError("error: coords_test is (S, n_test, 2), one set of test sites per point set")
        n_test = coords_test.shape[1]
        ct = _f64(np.stack([coords_test[i].ravel(order="F") for i in range(S)]))
        PT = np.zeros((S, n, n_test))
    R = np.zeros((S, n, n)) if want_R else None
    check(lib.mk_correlation_cross_batched(dptr(c), S, n, dptr(ct) if ct is not None else None, int(n_test), dptr(ph),
                                           dptr(nv) if nv is not None else None, COV_MODELS[cov_model],
                                           int(bool(stored_tables)), dptr(R) if want_R else None,
                                           dptr(PT) if PT is not None else None, int(device)))
    if want_R:
        R = np.ascontiguousarray(np.transpose(R, (0, 2, 1)))   # column-major -> (S, n, n) row-major
    return R, PT


def cholesky_batched(A, inverse=False, device=0):
    """Lower Cholesky factors, log-determinants (and inverses) of a batch of SPD matrices (S, n, n)."""
    lib = _lib.load()
    A = np.asarray(A, float)
    S, n, _ = A.shape
    a = _f64(np.transpose(A, (0, 2, 1)))          # row-major (S,n,n) -> column-major per matrix
    L = np.zeros((S, n, n))
    ld = np.zeros(S)
    inv = np.zeros((S, n, n)) if inverse else None
    check(lib.mk_cholesky_batched(dptr(a), S, n, dptr(L), dptr(ld), dptr(inv) if inverse else None, int(device)))
    L = np.ascontiguousarray(np.transpose(L, (0, 2, 1)))
    if inverse:
        inv = np.ascontiguousarray(np.transpose(inv, (0, 2, 1)))
        return L, ld, inv
    return L, ld

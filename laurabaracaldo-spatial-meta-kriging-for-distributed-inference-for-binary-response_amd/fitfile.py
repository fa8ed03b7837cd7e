"""A fit on disk: save a session's recorded chain, rebuild the session from it in a later process.

One uncompressed .npz (numpy arrays only: it is read back with allow_pickle=False) holds what a session was
made from and what its chain reported:

  version                     FORMAT_VERSION
  n_part (S), subset_base, q, p
  coords (sum n_s, 2), y (sum n_s q), weights (sum n_s q), x (sum n_s q, p)     the subsets' data, concatenated
  cfg_<field>                 every SamplerConfig field, as scalars and arrays (nu_* empty unless Matern)
  samples (S, n_samples, P)   p.beta.theta.samples per subset
  w_samples (sum n_s q, n_w)  p.w.samples per subset, rows concatenated: all n_samples columns of a session that
                              records w, or the kept columns alone (kept_only)
  acceptance (S, n_batch, P + 1)

read() returns the arrays without touching a device; load_session() creates the session over the data and imports
the chain (Session.import_chain), for the whole file or a contiguous range of its subsets -- a fit made on one GPU
is then replayed on several.

A running chain has a file of its own (the second half of this module): save_checkpoint() writes a session's
state after the iterations done so far, load_checkpoint() makes a session that continues the chain bit for bit."""
import numpy as np

from .session import SamplerConfig, Session

FORMAT_VERSION = 1
_CFG_SCALARS = ("q", "p", "cov_model", "link", "n_batch", "batch_length", "accept_rate", "burn_in", "w_starting", "w_tuning",
                "K_IW_df", "seed", "n_streams", "predict_tile")
_CFG_ARRAYS = ("beta_starting", "beta_tuning", "phi_starting", "phi_tuning", "phi_a", "phi_b", "A_starting", "A_tuning",
               "nu_starting", "nu_tuning", "nu_a", "nu_b", "K_IW_S")
_DATA = ("coords", "y", "weights", "x")
KEYS = ("version", "n_part", "subset_base", "q", "p") + _DATA + tuple("cfg_" + f for f in _CFG_SCALARS + _CFG_ARRAYS) + \
    ("samples", "w_samples", "acceptance")


def config_arrays(cfg):
    """Every SamplerConfig field as a numpy scalar or array, keyed cfg_<field>."""
    out = {}
    for f in _CFG_SCALARS:
        v = getattr(cfg, f)
        out["cfg_" + f] = np.array(v, dtype=np.uint64) if f == "seed" else np.array(v)
    for f in _CFG_ARRAYS:
        v = getattr(cfg, f)
        out["cfg_" + f] = np.zeros(0) if v is None else np.array(v, dtype=np.float64)
    return out


def config_from(arrays, predict_tile=None):
    """The SamplerConfig a file's cfg_ arrays describe (predict_tile: another tile than the saved one)."""
    g = lambda f: arrays["cfg_" + f]                                          # noqa: E731
    matern = str(g("cov_model")) == "matern"
    return SamplerConfig(
        int(g("q")), int(g("p")), g("beta_starting"), g("beta_tuning"), cov_model=str(g("cov_model")), n_batch=int(g("n_batch")),
        batch_length=int(g("batch_length")), accept_rate=float(g("accept_rate")), burn_in=int(g("burn_in")),
        phi_starting=g("phi_starting"), phi_tuning=g("phi_tuning"), phi_unif=(g("phi_a"), g("phi_b")),
        A_starting=g("A_starting"), A_tuning=g("A_tuning"), w_starting=float(g("w_starting")), w_tuning=float(g("w_tuning")),
        nu_starting=g("nu_starting") if matern else None, nu_tuning=g("nu_tuning") if matern else None,
        nu_unif=(g("nu_a"), g("nu_b")) if matern else None, K_IW_df=float(g("K_IW_df")), K_IW_S=g("K_IW_S"),
        seed=int(g("seed")), n_streams=int(g("n_streams")),
        predict_tile=int(g("predict_tile")) if predict_tile is None else int(predict_tile), link=str(g("link")))


def pack(subsets, cfg, subset_base, samples, w_samples, acceptance):
    """The arrays of a file from host data: subsets as a Session takes them, per subset samples (n_samples x P),
    w_samples ((n_s q) x n_w) and acceptance (n_batch x (P + 1))."""
    q, p = cfg.q, cfg.p
    out = dict(version=np.array(FORMAT_VERSION), subset_base=np.array(int(subset_base)), q=np.array(q), p=np.array(p),
               n_part=np.array([np.asarray(s["coords"]).shape[0] for s in subsets], dtype=np.int32))
    out["coords"] = np.concatenate([np.asarray(s["coords"], dtype=np.float64).reshape(-1, 2) for s in subsets])
    out["y"] = np.concatenate([np.asarray(s["y"], dtype=np.float64).reshape(-1) for s in subsets])
    out["weights"] = np.concatenate([np.asarray(s["weights"], dtype=np.float64).reshape(-1) for s in subsets])
    out["x"] = np.concatenate([np.asarray(s["x"], dtype=np.float64).reshape(-1, p) for s in subsets])
    out.update(config_arrays(cfg))
    out["samples"] = np.stack([np.asarray(a, dtype=np.float64) for a in samples])
    out["w_samples"] = np.concatenate([np.asarray(a, dtype=np.float64) for a in w_samples])
    out["acceptance"] = np.stack([np.asarray(a, dtype=np.float64) for a in acceptance])
    return out


def write(path, arrays):
    """One uncompressed .npz of numpy arrays alone (an object array would need pickle: refused)."""
    for k, a in arrays.items():
        if np.asarray(a).dtype == object:
            raise ValueError(f"error: fit file key '{k}' is not a plain array")
    with open(path, "wb") as f:
        np.savez(f, **{k: np.asarray(a) for k, a in arrays.items()})


def save_session(ses, path, kept_only=False):
    """The session's data, configuration and recorded chain into `path`.  The session must have finished its
    chain and record w (record_w: the file is what import_chain needs, and w is recorded nowhere else);
    kept_only writes the kept iterations' columns of w alone -- a smaller file whose session serves everything
    but the criteria's replay."""
    if not ses.record_w:
        raise ValueError("error: save_session needs a session created with record_w=True (the file holds p.w.samples)")
    out = ses.outputs(quantiles=False, samples=True, w_samples=True, acceptance=True)
    pr = ses._prob
    n = [int(v) for v in ses.n_part]
    q, p = ses.q, ses.p
    so = np.concatenate([[0], np.cumsum(n)])
    coords = pr.coords
    subsets = []
    for i, ns in enumerate(n):
        c = coords[2 * so[i]:2 * so[i + 1]].reshape(2, ns).T
        x = pr.x[so[i] * q * p:so[i + 1] * q * p].reshape(p, ns * q).T
        subsets.append(dict(coords=c, y=pr.y[so[i] * q:so[i + 1] * q], weights=pr.weights[so[i] * q:so[i + 1] * q], x=x))
    ws = [w[:, -ses.cfg.kept:] for w in out["w_samples"]] if kept_only else out["w_samples"]
    write(path, pack(subsets, ses.cfg, int(pr.c.subset_base), out["samples"], ws, out["acceptance"]))


def read(path, subsets=None):
    """The arrays of a fit file, by key, without touching a device.  subsets=(first, count): that contiguous
    range of the file's subsets alone (n_part, the data, samples, w_samples and acceptance cut to it;
    subset_base moved by first).  ValueError naming the key for an unknown version, a missing key or a shape
    that disagrees with n_part."""
    with np.load(path, allow_pickle=False) as z:
        if "version" not in z.files:
            raise ValueError("error: fit file lacks the key 'version'")
        if int(z["version"]) != FORMAT_VERSION:
            raise ValueError(f"error: fit file key 'version' is {int(z['version'])}; this build reads version {FORMAT_VERSION}")
        for k in KEYS:
            if k not in z.files:
                raise ValueError(f"error: fit file lacks the key '{k}'")
        for k in z.files:
            if k not in KEYS:
                raise ValueError(f"error: fit file holds the key '{k}', which this format does not have")
        a = {k: z[k] for k in KEYS}
    n_part = a["n_part"]
    S, q, p = int(n_part.shape[0]), int(a["q"]), int(a["p"])
    cfg = config_from(a)
    ntot = int(n_part.sum())
    n_w = a["w_samples"].shape[1] if a["w_samples"].ndim == 2 else -1
    want = dict(coords=(ntot, 2), y=(ntot * q,), weights=(ntot * q,), x=(ntot * q, p), samples=(S, cfg.n_samples, cfg.P),
                w_samples=(ntot * q, n_w), acceptance=(S, cfg.n_batch, cfg.P + 1))
    for k, shape in want.items():
        if a[k].shape != shape:
            raise ValueError(f"error: fit file key '{k}' has shape {a[k].shape}; n_part and the configuration give {shape}")
    if not (cfg.kept <= n_w <= cfg.n_samples):
        raise ValueError(f"error: fit file key 'w_samples' has {n_w} columns, outside kept .. n_samples = {cfg.kept} .. "
                         f"{cfg.n_samples}")
    if subsets is not None:
        first, count = int(subsets[0]), int(subsets[1])
        if first < 0 or count < 1 or first + count > S:
            raise ValueError(f"error: subsets=({first}, {count}) is outside the file's {S} subsets")
        so = np.concatenate([[0], np.cumsum(n_part)])
        lo, hi = int(so[first]), int(so[first + count])
        a["n_part"] = n_part[first:first + count].copy()
        a["subset_base"] = np.array(int(a["subset_base"]) + first)
        a["coords"] = a["coords"][lo:hi].copy()
        for k in ("y", "weights", "x", "w_samples"):
            a[k] = a[k][lo * q:hi * q].copy()
        for k in ("samples", "acceptance"):
            a[k] = a[k][first:first + count].copy()
    return a


def subsets_of(arrays):
    """The list of subsets (coords, y, weights, x) a Session takes, from read()'s arrays."""
    q = int(arrays["q"])
    so = np.concatenate([[0], np.cumsum(arrays["n_part"])])
    return [dict(coords=arrays["coords"][so[i]:so[i + 1]], y=arrays["y"][so[i] * q:so[i + 1] * q],
                 weights=arrays["weights"][so[i] * q:so[i + 1] * q], x=arrays["x"][so[i] * q:so[i + 1] * q])
            for i in range(len(so) - 1)]


def chain_of(arrays):
    """(samples, w_samples, acceptance) per subset, as Session.import_chain takes them."""
    q = int(arrays["q"])
    so = np.concatenate([[0], np.cumsum(arrays["n_part"])]) * q
    ws = [arrays["w_samples"][so[i]:so[i + 1]] for i in range(len(so) - 1)]
    return list(arrays["samples"]), ws, list(arrays["acceptance"])


def load_session(path, device=0, predict_tile=None, subsets=None):
    """A session over the file's data with the file's chain imported: it serves outputs(), set_test_sites() and
    every sink as the session that was saved (to rounding; samples and w_samples byte for byte).
    predict_tile: another kriging tile than the saved configuration's; subsets=(first, count): a contiguous
    range of the file's subsets, with subset_base + first.  The session records w when the file holds every
    iteration's w."""
    return session_from(read(path, subsets=subsets), device=device, predict_tile=predict_tile)


# ------------------------------------------------------------------ checkpoints: a running chain on disk
# One uncompressed .npz again, read back with allow_pickle=False, with a version key of its own:
#
#   ckpt_version                CKPT_VERSION
#   n_part, subset_base, q, p, coords, y, weights, x, cfg_<field>      as in a fit file (pack)
#   coords_test (n_test, 2), x_test (q n_test, p)    the session's test sites and their covariates (empty: none)
#   record_w, criteria          how the session was made
#   lookahead                   the schedule that wrote the state (a restore at 0 < iteration < n_samples continues on it)
#   iteration, n_pad, words     the iterations done, the padded subset size and the words per subset of every field
#   state_<field> (S, words)    the fields of mk_checkpoint (include/mk.h "checkpoints"), float64 but state_notpd
#   digests (S q, 4)            uint64: the digests of the pairs' factor buffers
CKPT_VERSION = 1
_CKPT_HEAD = ("ckpt_version", "n_part", "subset_base", "q", "p") + _DATA + tuple("cfg_" + f for f in _CFG_SCALARS + _CFG_ARRAYS)
_CKPT_META = ("coords_test", "x_test", "record_w", "criteria", "lookahead", "iteration", "n_pad", "words")


def _ckpt_keys():
    from ._lib import CKPT_FIELDS
    return _CKPT_HEAD + _CKPT_META + tuple("state_" + f for f in CKPT_FIELDS) + ("digests",)


def checkpoint_words(cfg, n_pad, iteration, n_test, record_w, criteria):
    """The words per subset of every checkpoint field after `iteration` iterations (the layout of
    mk_session_checkpoint_layout, restated for files read without a device)."""
    from ._lib import CKPT_FIELDS
    q, p, P, nth = cfg.q, cfg.p, cfg.P, cfg.n_theta
    Np = n_pad * q
    k = max(0, iteration - (cfg.burn_in - 1))
    tiled = cfg.predict_tile > 0 and (n_test == 0 or cfg.predict_tile < n_test)
    w = dict(beta=p, theta=nth, w=Np, eta=Np, tune=P + Np, acc=P + Np, u=q * n_pad, z=q * n_pad, Z=q * q * n_pad, logdetR=q,
             quad=q, A_full=q * q, Ainv=q * q, notpd=q,
             crit_acc=6 * Np if criteria and k > 0 else 0, crit_part=k * ((Np + 255) // 256) if criteria else 0,
             crit_sbeta=p if criteria and k > 0 else 0,
             samples=iteration * P, w_samples=iteration * Np if record_w else 0,
             acc_hist=(iteration // cfg.batch_length) * (P + 1),
             kz=k * q * n_pad if tiled else 0, kth=k * nth if tiled else 0, kA=k * q * q if tiled else 0,
             w_pred=k * q * n_test if (not tiled and n_test > 0) else 0)
    return np.array([w[f] for f in CKPT_FIELDS], dtype=np.int64)


def pack_checkpoint(subsets, cfg, subset_base, state, coords_test=None, x_test=None, record_w=False, criteria=False):
    """The arrays of a checkpoint file from host data: subsets as a Session takes them and a Session.checkpoint()
    state of all of them."""
    from ._lib import CKPT_FIELDS
    S = len(subsets)
    empty = np.zeros((S, 0))
    out = pack(subsets, cfg, subset_base, [empty] * S, [empty] * S, [empty] * S)
    for k in ("version", "samples", "w_samples", "acceptance"):
        del out[k]
    out["ckpt_version"] = np.array(CKPT_VERSION)
    n_test = 0 if coords_test is None else int(np.asarray(coords_test).shape[0])
    out["coords_test"] = np.zeros((0, 2)) if coords_test is None else np.asarray(coords_test, dtype=np.float64).reshape(-1, 2)
    out["x_test"] = np.zeros((0, cfg.p)) if x_test is None else np.asarray(x_test, dtype=np.float64).reshape(cfg.q * n_test, cfg.p)
    out["record_w"] = np.array(bool(record_w))
    out["criteria"] = np.array(bool(criteria))
    out["lookahead"] = np.array(bool(state["lookahead"]))
    out["iteration"] = np.array(int(state["iteration"]))
    n_max = max(int(np.asarray(s["coords"]).shape[0]) for s in subsets)
    out["n_pad"] = np.array((n_max + 1 + 127) // 128 * 128)
    out["words"] = np.asarray(state["words"], dtype=np.int64)
    for f in CKPT_FIELDS:
        out["state_" + f] = np.asarray(state[f])
    out["digests"] = np.asarray(state["digests"], dtype=np.uint64)
    return out


def write_atomic(path, arrays):
    """write() to a temporary name in path's directory, renamed over path once complete: a writer that dies half
    way leaves the previous file as it was."""
    import os
    path = os.fspath(path)
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        write(tmp, arrays)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise


def save_checkpoint(ses, path):
    """The session's data, configuration, test sites and state after the iterations done so far into `path`
    (Session.checkpoint of every subset), atomically.  load_checkpoint in a later process continues the chain
    bit for bit."""
    pr = ses._prob
    n = [int(v) for v in ses.n_part]
    q, p = ses.q, ses.p
    so = np.concatenate([[0], np.cumsum(n)])
    subsets = []
    for i, ns in enumerate(n):
        c = pr.coords[2 * so[i]:2 * so[i + 1]].reshape(2, ns).T
        x = pr.x[so[i] * q * p:so[i + 1] * q * p].reshape(p, ns * q).T
        subsets.append(dict(coords=c, y=pr.y[so[i] * q:so[i + 1] * q], weights=pr.weights[so[i] * q:so[i + 1] * q], x=x))
    # the test sites the session was created with (they decide whether its kriging is fused or tiled); sites set
    # later by set_test_sites serve the outputs after the chain, and the caller sets them again
    ct = None if not pr.n_test else np.asarray(pr.coords_test).reshape(2, pr.n_test).T
    xt = None if pr.x_test is None or not pr.n_test else np.asarray(pr.x_test).reshape(p, q * pr.n_test).T
    from ._lib import CKPT_FIELDS
    crit = bool(ses._ckpt_words(ses.cfg.n_samples)[CKPT_FIELDS.index("crit_part")] > 0)
    write_atomic(path, pack_checkpoint(subsets, ses.cfg, int(pr.c.subset_base), ses.checkpoint(), coords_test=ct, x_test=xt,
                                       record_w=ses.record_w, criteria=crit))


def read_checkpoint(path, subsets=None):
    """The arrays of a checkpoint file, by key, without touching a device.  subsets=(first, count): that range of
    the file's subsets alone (n_part, the data, the state and the digests cut to it; subset_base moved by first).
    ValueError naming the key for an unknown version, a missing or unknown key, or a shape that disagrees with
    n_part, the configuration and the iteration."""
    from ._lib import CKPT_FIELDS, CKPT_NDIGEST
    keys = _ckpt_keys()
    with np.load(path, allow_pickle=False) as z:
        if "ckpt_version" not in z.files:
            raise ValueError("error: checkpoint file lacks the key 'ckpt_version'")
        if int(z["ckpt_version"]) != CKPT_VERSION:
            raise ValueError(f"error: checkpoint file key 'ckpt_version' is {int(z['ckpt_version'])}; this build reads "
                             f"version {CKPT_VERSION}")
        for k in keys:
            if k not in z.files:
                raise ValueError(f"error: checkpoint file lacks the key '{k}'")
        for k in z.files:
            if k not in keys:
                raise ValueError(f"error: checkpoint file holds the key '{k}', which this format does not have")
        a = {k: z[k] for k in keys}
    n_part = a["n_part"]
    S, q, p = int(n_part.shape[0]), int(a["q"]), int(a["p"])
    cfg = config_from(a)
    ntot = int(n_part.sum())
    it = int(a["iteration"])
    if not 0 <= it <= cfg.n_samples:
        raise ValueError(f"error: checkpoint file key 'iteration' is {it}, outside 0 .. n_samples = {cfg.n_samples}")
    if a["coords_test"].ndim != 2 or a["coords_test"].shape[1] != 2:
        raise ValueError(f"error: checkpoint file key 'coords_test' has shape {a['coords_test'].shape}, not (n_test, 2)")
    n_test = int(a["coords_test"].shape[0])
    n_pad = int(a["n_pad"])
    if n_pad % 128 or n_pad < int(n_part.max()) + 1:
        raise ValueError(f"error: checkpoint file key 'n_pad' is {n_pad}; the largest subset of n_part needs a multiple of "
                         f"128 of at least {int(n_part.max()) + 1}")
    words = checkpoint_words(cfg, n_pad, it, n_test, bool(a["record_w"]), bool(a["criteria"]))
    want = dict(coords=(ntot, 2), y=(ntot * q,), weights=(ntot * q,), x=(ntot * q, p), words=words.shape,
                digests=(S * q, CKPT_NDIGEST))
    if a["x_test"].size:
        want["x_test"] = (q * n_test, p)
    for f, nw in zip(CKPT_FIELDS, words):
        want["state_" + f] = (S, int(nw))
    for k, shape in want.items():
        if a[k].shape != shape:
            raise ValueError(f"error: checkpoint file key '{k}' has shape {a[k].shape}; n_part, the configuration and "
                             f"iteration {it} give {shape}")
    if not np.array_equal(a["words"], words):
        raise ValueError(f"error: checkpoint file key 'words' is {a['words'].tolist()}; n_part, the configuration and "
                         f"iteration {it} give {words.tolist()}")
    if subsets is not None:
        first, count = int(subsets[0]), int(subsets[1])
        if first < 0 or count < 1 or first + count > S:
            raise ValueError(f"error: subsets=({first}, {count}) is outside the file's {S} subsets")
        so = np.concatenate([[0], np.cumsum(n_part)])
        lo, hi = int(so[first]), int(so[first + count])
        a["n_part"] = n_part[first:first + count].copy()
        a["subset_base"] = np.array(int(a["subset_base"]) + first)
        a["coords"] = a["coords"][lo:hi].copy()
        for k in ("y", "weights", "x"):
            a[k] = a[k][lo * q:hi * q].copy()
        for f in CKPT_FIELDS:
            a["state_" + f] = a["state_" + f][first:first + count].copy()
        a["digests"] = a["digests"][first * q:(first + count) * q].copy()
    return a


def _first_difference(a, data, cfg):
    """The first key of a checkpoint's arrays that differs from the caller's data (a list of subsets) or
    configuration, or None.  n_streams is how a session executes, not what it computes: not compared."""
    if data is not None:
        b = pack(data, config_from(a) if cfg is None else cfg, int(a["subset_base"]), [np.zeros(0)] * len(data),
                 [np.zeros(0)] * len(data), [np.zeros(0)] * len(data))
        for k in ("n_part",) + _DATA:
            if a[k].shape != b[k].shape or a[k].tobytes() != np.asarray(b[k], dtype=a[k].dtype).tobytes():
                return k
    if cfg is not None:
        b = config_arrays(cfg)
        for f in _CFG_SCALARS + _CFG_ARRAYS:
            k = "cfg_" + f
            if f != "n_streams" and (a[k].shape != b[k].shape or a[k].tobytes() != np.asarray(b[k], dtype=a[k].dtype).tobytes()):
                return k
    return None


def load_checkpoint(path, subsets=None, device=0, data=None, cfg=None, n_streams=None, **session_kw):
    """A session over the file's data and test sites with the file's state restored, ready for run(): it continues
    the chain that was checkpointed, bit for bit.  The two schedules round z differently, so a state written
    mid-chain continues on the schedule that wrote it, whatever session_kw's lookahead= says (Session.lookahead
    reports it); n_streams > 1 has the sequential schedule alone and refuses a lookahead state written mid-chain
    (MkError).
    subsets=(first, count): a contiguous range of the file's subsets, with subset_base + first -- a chain started
    on one GPU continues on several (the range's largest subset must round to the file's n_pad).  data (the list
    of subsets the caller would fit) and cfg (its SamplerConfig): when given, a file whose data or configuration
    differ is refused, naming the first key that differs; record_w= and criteria= likewise (the session is made
    as the file says)."""
    a = read_checkpoint(path, subsets=subsets)
    k = _first_difference(a, data, cfg)
    for name in ("record_w", "criteria"):        # how the caller would have made the session, when it says so
        want = session_kw.pop(name, None)
        if k is None and want is not None and bool(want) != bool(a[name]):
            k = name
    if k is not None:
        raise ValueError(f"error: checkpoint file key '{k}' differs from what the caller passes; the file continues the "
                         f"chain it was written from and no other")
    return session_from_checkpoint(a, device=device, n_streams=n_streams, **session_kw)


def session_from_checkpoint(a, device=0, n_streams=None, **session_kw):
    """load_checkpoint's second half: the session of read_checkpoint()'s arrays."""
    from ._lib import CKPT_FIELDS
    cfg = config_from(a)
    if n_streams is not None:
        cfg.n_streams = int(n_streams)
    ct = a["coords_test"] if a["coords_test"].shape[0] else None
    xt = a["x_test"] if a["x_test"].size else None
    # the schedule that wrote the state, unless the caller names one (several stream groups have the sequential
    # one alone)
    if "lookahead" not in session_kw and cfg.n_streams <= 1:
        session_kw["lookahead"] = bool(a["lookahead"])
    ses = Session(subsets_of(a), cfg, coords_test=ct, subset_base=int(a["subset_base"]), device=device,
                  record_w=bool(a["record_w"]), x_test=xt, criteria=bool(a["criteria"]), **session_kw)
    try:
        state = {f: a["state_" + f] for f in CKPT_FIELDS}
        state.update(iteration=a["iteration"], words=a["words"], digests=a["digests"], lookahead=a["lookahead"])
        ses.restore(state)
    except Exception:
        ses.close()
        raise
    return ses


def session_from(a, device=0, predict_tile=None):
    """load_session's second half: the session of read()'s arrays."""
    cfg = config_from(a, predict_tile=predict_tile)
    if cfg.predict_tile <= 0:
        raise ValueError("error: load_session needs predict_tile > 0 (the saved configuration has none: pass one)")
    samples, ws, acc = chain_of(a)
    ses = Session(subsets_of(a), cfg, subset_base=int(a["subset_base"]), device=device,
                  record_w=a["w_samples"].shape[1] == cfg.n_samples)
    try:
        ses.import_chain(samples, ws, acc)
    except Exception:
        ses.close()
        raise
    return ses

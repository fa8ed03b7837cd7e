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
is then replayed on several."""
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

"""Numpy restatement of the multi-DLA model (DESIGN.md "Multi-DLA"; Ho, Bird & Garnett 2020,
arXiv:2003.11036), built on oracle.gpdla_oracle's prepare_spectrum / voigt_mex / log_mvnpdf_low_rank.

Level 1 is process_qsos.m:184-198.  At level d >= 2 sample j carries its own DLA plus the d - 1 DLAs of
a base sample b_d(j) drawn from the level-(d-1) posterior of the same spectrum:

  weights     m = max of the non-NaN l_{d-1}; w_i = exp(l_{d-1}[i] - m), NaN -> 0; C = cumsum(w); W = C[-1]
  resampling  b_d(j) = the smallest i with C_i > u_{d,j} W (the last i with w_i > 0 if none)
  chain       c_d(j) = [b_d(j)] ++ c_{d-1}(b_d(j)), c_1 empty
  absorption  a = A_j * prod_{i in c_d(j)} A_i, each A a separately broadened voigt profile
  likelihood  log_mvnpdf_low_rank(y, mu a, M a, omega^2 a^2 + sigma^2)
  exclusion   NaN if |z_j - z_i| < min_z_separation for an i in c_d(j)
  evidence    m_d + log(mean over the non-NaN samples of exp(l_d - m_d)) - (d - 1) occam_log_penalty
  degenerate  W = 0 or not finite (or an unusable spectrum): NaN rows, NaN evidence, base indices -1,
              at this and every deeper level

All sample indices are in the caller's order.
"""
import math

import numpy as np

from oracle import gpdla_oracle as O

KMS_TO_Z_3000 = 3000 * 1000 / 299792458


# --------------------------------------------------------------------------------------- resampler
def weights(ll):
    ll = np.asarray(ll, dtype=np.float64)
    finite = ~np.isnan(ll)
    if not finite.any():
        return np.zeros(ll.size)
    m = np.max(ll[finite])
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(finite, np.exp(np.where(finite, ll, 0.0) - m), 0.0)


def prefix_fsum(w):
    """Correctly rounded prefix sums (Shewchuk partials, as math.fsum keeps them)."""
    partials, out = [], np.empty(len(w))
    for n, x in enumerate(w):
        x = float(x)
        i = 0
        for y in partials:
            if abs(x) < abs(y):
                x, y = y, x
            hi = x + y
            lo = y - (hi - x)
            if lo:
                partials[i] = lo
                i += 1
            x = hi
        partials[i:] = [x]
        out[n] = math.fsum(partials)
    return out


def resample(ll, u, prefix="cumsum"):
    """Steps 1-2 for one row: int64 indices, -1 throughout a degenerate row."""
    w = weights(ll)
    u = np.asarray(u, dtype=np.float64)
    C = np.cumsum(w) if prefix == "cumsum" else prefix_fsum(w)
    W = C[-1]
    if not (np.isfinite(W) and W > 0):
        return np.full(u.size, -1, dtype=np.int64)
    idx = np.searchsorted(C, u * W, side="right")      # the smallest i with C_i > u W
    last = np.flatnonzero(w > 0)[-1]
    return np.where(idx >= w.size, last, idx).astype(np.int64)


def ambiguous(ll, u, rel=1e-9):
    """Entries whose u W lies within rel W of a prefix-sum edge (fsum prefix): there a device prefix sum
    in another order may land on the neighbouring non-zero-weight index.  Also returns the nearest
    relative edge distance of the row."""
    w = weights(ll)
    C = prefix_fsum(w)
    W = C[-1]
    if not (np.isfinite(W) and W > 0):
        return np.zeros(np.size(u), dtype=bool), np.inf
    t = np.asarray(u, dtype=np.float64) * W
    edges = np.unique(C)
    pos = np.searchsorted(edges, t)
    dist = np.minimum(np.abs(edges[np.clip(pos, 0, edges.size - 1)] - t), np.abs(edges[np.clip(pos - 1, 0, edges.size - 1)] - t))
    return dist <= rel * W, float(dist.min() / W)


def neighbours_ok(ll, got, want):
    """For ambiguous entries: ``got`` is ``want`` or the non-zero-weight index next to it."""
    nz = np.flatnonzero(weights(ll) > 0)
    pg, pw = np.searchsorted(nz, got), np.searchsorted(nz, want)
    return np.isin(got, nz) & (np.abs(pg - pw) <= 1)


# ------------------------------------------------------------------------------------------- model
def log_mean_exp_nan(ll):
    ll = np.asarray(ll, dtype=np.float64)
    v = ll[~np.isnan(ll)]
    if v.size == 0:
        return np.nan
    m = np.max(v)
    return m + np.log(np.mean(np.exp(v - m)))


def usable(spec):
    rest = np.asarray(spec["wavelengths"]) / (1 + spec["z_qso"])
    ind = (rest >= O.MIN_LAMBDA) & (rest <= O.MAX_LAMBDA) & ~np.asarray(spec["pixel_mask"], dtype=bool)
    return bool(ind.any())


class SpectrumOracle:
    """One spectrum: the prepared quantities, every sample's broadened profile (cached) and levels."""

    def __init__(self, spec, model, samples, num_lines=3, absorption_mode="reference"):
        self.S = np.asarray(samples["offset_samples"]).size
        self.ok = usable(spec)
        if not self.ok:
            return
        self.prep = O.prepare_spectrum(spec["wavelengths"], spec["flux"], spec["noise_variance"], spec["pixel_mask"],
                                       spec["z_qso"], model, absorption_mode)
        p = self.prep
        self.z = p["zmin"] + (p["zmax"] - p["zmin"]) * np.asarray(samples["offset_samples"], dtype=np.float64)
        nhi = np.asarray(samples["nhi_samples"], dtype=np.float64)
        self.A = np.stack([O.voigt_mex(p["padded"], z, N, num_lines)[p["absorption_index"]]
                           for z, N in zip(self.z, nhi)])

    def ll_of(self, absorption):
        p = self.prep
        return O.log_mvnpdf_low_rank(p["y"], p["mu"] * absorption, p["M"] * absorption[:, None],
                                     p["omega2"] * absorption ** 2 + p["noise"])

    def level1(self):
        if not self.ok:
            return np.full(self.S, np.nan)
        return np.array([self.ll_of(a) for a in self.A])

    def level(self, chains, min_z_separation=KMS_TO_Z_3000):
        """l_d for chains [S][d-1] (caller-order indices, -1 = none)."""
        out = np.full(self.S, np.nan)
        if not self.ok:
            return out
        for j, c in enumerate(chains):
            c = np.asarray(c)
            if c.size == 0 or np.any(c < 0) or np.any(np.abs(self.z[j] - self.z[c]) < min_z_separation):
                continue
            out[j] = self.ll_of(self.A[j] * np.prod(self.A[c], axis=0))
        return out


def process_spectrum_multi(spec, model, samples, max_dlas, uniforms=None, forced=None,
                           min_z_separation=KMS_TO_Z_3000, occam_log_penalty=None, num_lines=3,
                           absorption_mode="reference", oracle=None):
    """Every level of one spectrum.  ``uniforms`` (D-1) x S, or ``forced`` (D-1) x S base indices.
    Returns sample rows D x S, evidences D, base indices (D-1) x S (int64, -1 = none)."""
    so = oracle or SpectrumOracle(spec, model, samples, num_lines, absorption_mode)
    S, D = so.S, int(max_dlas)
    pen = math.log(S) if occam_log_penalty is None else occam_log_penalty
    sll = np.full((D, S), np.nan)
    lld = np.full(D, np.nan)
    base = np.full((max(D - 1, 0), S), -1, dtype=np.int64)
    sll[0] = so.level1()
    lld[0] = O.log_mean_exp(sll[0]) if so.ok else np.nan
    chains = np.zeros((S, 0), dtype=np.int64)
    for d in range(2, D + 1):
        b = np.asarray(forced[d - 2], dtype=np.int64) if forced is not None else resample(sll[d - 2], uniforms[d - 2])
        base[d - 2] = b
        safe = np.where(b >= 0, b, 0)
        chains = np.where((b >= 0)[:, None], np.concatenate([b[:, None], chains[safe]], axis=1), -1)
        sll[d - 1] = so.level(chains, min_z_separation)
        lld[d - 1] = log_mean_exp_nan(sll[d - 1]) - (d - 1) * pen
    out = dict(sample_log_likelihoods_dla=sll, log_likelihoods_dla=lld, base_sample_inds=base)
    if so.ok:
        out.update(log_likelihood_no_dla=O.null_log_likelihood(so.prep), min_z_dla=so.prep["zmin"],
                   max_z_dla=so.prep["zmax"], n=so.prep["n"])
    else:
        out.update(log_likelihood_no_dla=np.nan, min_z_dla=np.nan, max_z_dla=np.nan, n=0)
    return out


def compute(model, samples, packed, params, device=0, max_dlas=1, uniforms=None):
    """A stand-in for the engine in process.process_qsos(..., compute=...): Engine.process's arrays for
    max_dlas = 1, Engine.process_multi's for more."""
    off = np.asarray(packed["offsets"])
    Q = off.size - 1
    S = np.asarray(samples["offset_samples"]).size
    D = int(max_dlas)
    if uniforms is None and D > 1:
        uniforms = np.random.default_rng(2003).random((D - 1, S))
    res = []
    for q in range(Q):
        a, b = off[q], off[q + 1]
        spec = dict(wavelengths=packed["wavelengths"][a:b], flux=packed["flux"][a:b],
                    noise_variance=packed["noise_variance"][a:b], pixel_mask=packed["pixel_mask"][a:b].astype(bool),
                    z_qso=float(packed["z_qsos"][q]))
        res.append(process_spectrum_multi(spec, model, samples, D, uniforms, num_lines=params.num_lines,
                                          absorption_mode=params.absorption_mode))
    out = dict(log_likelihoods_no_dla=np.array([r["log_likelihood_no_dla"] for r in res]),
               min_z_dlas=np.array([r["min_z_dla"] for r in res]), max_z_dlas=np.array([r["max_z_dla"] for r in res]),
               num_pixels=np.array([r["n"] for r in res], dtype=np.int32))
    sll = np.stack([r["sample_log_likelihoods_dla"] for r in res], axis=1)          # D x Q x S
    lld = np.stack([r["log_likelihoods_dla"] for r in res], axis=1)                 # D x Q
    if D == 1:
        out.update(sample_log_likelihoods_dla=sll[0], log_likelihoods_dla=lld[0])
    else:
        out.update(sample_log_likelihoods_dla=sll, log_likelihoods_dla=lld, max_dlas=D,
                   base_sample_inds=np.stack([r["base_sample_inds"] for r in res], axis=1).astype(np.int32))
    return out

"""Numpy restatement of the model spectra, on oracle.gpdla_oracle.

For one spectrum and 0 to 4 absorbers, on the likelihood's n pixels, with prepare_spectrum's mu, M, omega^2, y,
sigma^2 (after mean_flux_scope_oracle.apply_forest when a forest is given):
    a = prod_i voigt_mex(padded, z_i, N_i, num_lines)[absorption_index]
    d = a^2 omega^2 + sigma^2,  r = y - a mu,  V = diag(a) M
every output is computed two ways, which test_model_spectra.py holds to each other:
    woodbury   B = I + V'D^-1 V, u = V'D^-1 r, w = B^-1 u: continuum mu + M w, variance diag(M B^-1 M'),
               chi2 = r'D^-1 r - u'w, log det K = log det B + sum log d
    dense      K = V V' + D (n x n): continuum mu + M V'K^-1 r, covariance M (I - V'K^-1 V) M', chi2 = r'K^-1 r,
               slogdet(K)
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from oracle import gpdla_oracle as O  # noqa: E402

import mean_flux_scope_oracle as FS  # noqa: E402

LOG_2PI = np.log(2 * np.pi)
KEYS = ("absorption", "model_mean", "continuum", "continuum_sd")
SCALARS = ("chi2", "log_likelihood")


def prepare(spec, model, absorption_mode="reference", forest=None):
    """prepare_spectrum (None for a spectrum without a usable pixel), under ``forest`` when given, plus the
    indices of the likelihood's pixels within the spectrum."""
    wl = np.asarray(spec["wavelengths"], dtype=np.float64)
    rest = wl / (1 + spec["z_qso"])
    ind = (rest >= O.MIN_LAMBDA) & (rest <= O.MAX_LAMBDA) & ~np.asarray(spec["pixel_mask"], dtype=bool)
    if not ind.any():
        return None
    prep = O.prepare_spectrum(spec["wavelengths"], spec["flux"], spec["noise_variance"], spec["pixel_mask"],
                              spec["z_qso"], model, absorption_mode)
    if forest is not None:
        prep = FS.apply_forest(prep, spec, model, forest)
    prep = dict(prep)
    prep["pixel_inds"] = np.flatnonzero(ind)
    return prep


def absorption(prep, z_dlas, nhis, num_lines):
    a = np.ones(prep["n"])
    for z, N in zip(z_dlas, nhis):
        a = a * O.voigt_mex(prep["padded"], z, N, num_lines)[prep["absorption_index"]]
    return a


def _terms(prep, a):
    d = a ** 2 * prep["omega2"] + prep["noise"]
    r = prep["y"] - a * prep["mu"]
    return d, r, a[:, None] * prep["M"]


def woodbury(prep, a):
    d, r, V = _terms(prep, a)
    M, k = prep["M"], prep["M"].shape[1]
    B = np.eye(k) + V.T @ (V / d[:, None])
    u = V.T @ (r / d)
    w = np.linalg.solve(B, u)
    chi2 = r @ (r / d) - u @ w
    logdet = np.linalg.slogdet(B)[1] + np.sum(np.log(d))
    var = np.einsum("ij,ij->i", M, np.linalg.solve(B, M.T).T)
    return dict(absorption=a, model_mean=a * prep["mu"], continuum=prep["mu"] + M @ w,
                continuum_sd=np.sqrt(np.maximum(var, 0.0)), continuum_var=var, chi2=chi2,
                log_likelihood=-0.5 * (chi2 + logdet + prep["n"] * LOG_2PI))


def dense(prep, a):
    d, r, V = _terms(prep, a)
    M, k = prep["M"], prep["M"].shape[1]
    K = V @ V.T + np.diag(d)
    Kr = np.linalg.solve(K, r)
    chi2 = r @ Kr
    cov = M @ (np.eye(k) - V.T @ np.linalg.solve(K, V)) @ M.T
    var = np.diag(cov)
    return dict(absorption=a, model_mean=a * prep["mu"], continuum=prep["mu"] + M @ (V.T @ Kr),
                continuum_sd=np.sqrt(np.maximum(var, 0.0)), continuum_var=var, chi2=chi2,
                log_likelihood=-0.5 * (chi2 + np.linalg.slogdet(K)[1] + prep["n"] * LOG_2PI))


def model_spectrum(spec, model, z_dlas, nhis, num_lines=3, absorption_mode="reference", forest=None, form=woodbury):
    """One spectrum's outputs (plus ``pixel_inds`` and ``n``), or None when it has no usable pixel."""
    prep = prepare(spec, model, absorption_mode, forest)
    if prep is None:
        return None
    out = form(prep, absorption(prep, z_dlas, nhis, num_lines))
    out.update(pixel_inds=prep["pixel_inds"], n=prep["n"])
    return out


def forms_agree(spec, model, z_dlas, nhis, num_lines=3, absorption_mode="reference", forest=None):
    """max over every output of |woodbury - dense| / max(|value|, 1): the condition on a test's inputs."""
    prep = prepare(spec, model, absorption_mode, forest)
    a = absorption(prep, z_dlas, nhis, num_lines)
    w, dn = woodbury(prep, a), dense(prep, a)
    worst = 0.0
    for key in KEYS + SCALARS + ("continuum_var",):
        x, y = np.atleast_1d(w[key]), np.atleast_1d(dn[key])
        worst = max(worst, float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1.0))))
    return worst

"""Numpy restatement of the sub-DLA model and the Lyman-series forest (Ho, Bird &
Garnett 2020, arXiv:2003.11036), built on oracle.gpdla_oracle's prepare_spectrum / sample_log_likelihood
and on multi_dla_oracle.py.

Forest, for a pixel at observed wavelength lambda, quasar redshift z_Q and line i = 1..L:
  lambda_i = TRANSITION_WAVELENGTHS[i-1] 1e8,  c_i = LEADING_CONSTANTS[i-1] / LEADING_CONSTANTS[0]
  z_i = (lambda - lambda_i) / lambda_i,  t_i(tau_0, beta) = tau_0 c_i (1 + z_i)^beta [z_i <= z_Q]
  variance series  omega^2 = exp(2 log omega) (1 - exp(-sum_i t_i(tau_0, beta)) + c_0)^2   (the model's)
  mean flux        mu <- mu exp(-sum_i t_i(tau_0^mf, beta^mf))                             (Kim et al. 2007)
Both act on the unmasked in-range pixels at their own wavelengths, for every model.

Sub-DLA: sample j is one absorber at z_j = min_z + (max_z - min_z) offset_j with column density N^sub_j; its
likelihood is the level-1 likelihood with N^sub_j, its evidence the log-mean-exp of process_qsos.m:202-209.

Priors: Pr(sub) = r p, Pr(exactly d DLAs) as in the multi-DLA model, Pr(none) = 1 - p - r p.
"""
import math

import numpy as np

import multi_dla_oracle as MO
import posterior_summary_oracle as PO
from oracle import gpdla_oracle as O

LINE_WAVELENGTHS = O.TRANSITION_WAVELENGTHS * 1e8
LINE_STRENGTHS = O.LEADING_CONSTANTS / O.LEADING_CONSTANTS[0]
MEAN_FLUX_TAU_0, MEAN_FLUX_BETA = 0.0023, 3.65
FOREST_DEFAULTS = dict(num_forest_lines=31, variance_series=True, mean_flux=True, mean_flux_tau_0=MEAN_FLUX_TAU_0,
                       mean_flux_beta=MEAN_FLUX_BETA)


# ------------------------------------------------------------------------------------------ forest
def forest_tau(wavelengths, z_qso, tau_0, beta, num_lines=31):
    """sum_i t_i(tau_0, beta) per pixel, in line order."""
    lam = np.asarray(wavelengths, dtype=np.float64)
    total = np.zeros(lam.shape)
    for i in range(num_lines):
        zi = (lam - LINE_WAVELENGTHS[i]) / LINE_WAVELENGTHS[i]
        total = total + np.where(zi <= z_qso, tau_0 * LINE_STRENGTHS[i] * (1 + zi) ** beta, 0.0)
    return total


def forest_tau_loops(wavelengths, z_qso, tau_0, beta, num_lines=31):
    """The same sum as a plain double loop over pixels and lines (python floats)."""
    out = []
    for lam in np.asarray(wavelengths, dtype=np.float64).tolist():
        s = 0.0
        for i in range(num_lines):
            li = float(LINE_WAVELENGTHS[i])
            zi = (lam - li) / li
            if zi <= z_qso:
                s += tau_0 * float(LINE_STRENGTHS[i]) * math.pow(1 + zi, beta)
        out.append(s)
    return np.array(out)


def active_lines(rest_wavelength, z_qso, num_lines=31):
    """How many lines have z_i <= z_Q for the pixel at this rest wavelength."""
    lam = rest_wavelength * (1 + z_qso)
    zi = (lam - LINE_WAVELENGTHS[:num_lines]) / LINE_WAVELENGTHS[:num_lines]
    return int(np.count_nonzero(zi <= z_qso))


def unmasked_wavelengths(spec):
    """The observed wavelengths of the pixels prepare_spectrum keeps (process_qsos.m:102-113)."""
    w = np.asarray(spec["wavelengths"], dtype=np.float64)
    rest = w / (1 + spec["z_qso"])
    ind = (rest >= O.MIN_LAMBDA) & (rest <= O.MAX_LAMBDA) & ~np.asarray(spec["pixel_mask"], dtype=bool)
    return w[ind]


def apply_forest(prep, spec, model, forest, wavelengths=None):
    """prepare_spectrum's dict with mu and / or omega^2 replaced as ``forest`` says (None: unchanged).
    ``wavelengths`` overrides the pixels' own wavelengths (tests: what a wrong pairing would give)."""
    if forest is None:
        return prep
    f = dict(FOREST_DEFAULTS, **forest)
    w = unmasked_wavelengths(spec) if wavelengths is None else np.asarray(wavelengths, dtype=np.float64)
    z = spec["z_qso"]
    out = dict(prep)
    if f["variance_series"]:
        c_0, tau_0, beta = (np.exp(model[k]) for k in ("log_c_0", "log_tau_0", "log_beta"))
        log_omega = np.interp(w / (1 + z), model["rest_wavelengths"], model["log_omega"])
        scaling = 1 - np.exp(-forest_tau(w, z, tau_0, beta, f["num_forest_lines"])) + c_0
        out["omega2"] = np.exp(2 * log_omega) * scaling ** 2
    if f["mean_flux"]:
        out["mu"] = prep["mu"] * np.exp(-forest_tau(w, z, f["mean_flux_tau_0"], f["mean_flux_beta"], f["num_forest_lines"]))
    return out


# ------------------------------------------------------------------------------------------- model
class SpectrumOracle(MO.SpectrumOracle):
    """multi_dla_oracle's spectrum with the forest applied to the prepared quantities, plus the sub-DLA rows."""

    def __init__(self, spec, model, samples, num_lines=3, absorption_mode="reference", forest=None):
        super().__init__(spec, model, samples, num_lines, absorption_mode)
        self.num_lines = num_lines
        if self.ok:
            self.prep = apply_forest(self.prep, spec, model, forest)

    def sub_level(self, sub_nhi):
        """The sub-DLA sample rows: one absorber at the engine's z_j with column density sub_nhi[j]."""
        if not self.ok:
            return np.full(self.S, np.nan)
        return np.array([O.sample_log_likelihood(self.prep, z, N, self.num_lines) for z, N in zip(self.z, sub_nhi)])


def evidence(sample_ll):
    """reduce_kernel's log-mean-exp: any NaN -> NaN."""
    sample_ll = np.asarray(sample_ll, dtype=np.float64)
    return np.nan if np.isnan(sample_ll).any() else O.log_mean_exp(sample_ll)


def process_spectrum(spec, model, samples, max_dlas=1, sub_nhi=None, forest=None, uniforms=None, forced=None,
                     num_lines=3, absorption_mode="reference", oracle=None):
    """multi_dla_oracle.process_spectrum_multi under the forest, plus ``sample_log_likelihoods_lls`` /
    ``log_likelihood_lls`` when ``sub_nhi`` is given."""
    so = oracle or SpectrumOracle(spec, model, samples, num_lines, absorption_mode, forest)
    out = MO.process_spectrum_multi(spec, model, samples, max_dlas, uniforms, forced, num_lines=num_lines,
                                    absorption_mode=absorption_mode, oracle=so)
    if sub_nhi is not None:
        out["sample_log_likelihoods_lls"] = so.sub_level(np.asarray(sub_nhi, dtype=np.float64))
        out["log_likelihood_lls"] = evidence(out["sample_log_likelihoods_lls"]) if so.ok else np.nan
    return out


def compute(model, samples, packed, params, device=0, max_dlas=1, sub_dla=None, forest=None, summaries=None,
            save_samples=True, uniforms=None, forced=None):
    """A stand-in for the engine in process.process_qsos(..., compute=...): Engine.process's arrays for
    max_dlas = 1 (process_multi's for more), the sub-DLA arrays of Engine.process_models when ``sub_dla``
    (dict(nhi, log_nhi, ratio)) is given, and with ``summaries`` the MAP arrays (no grid here).  ``forced``
    ((D - 1) x Q x S base indices, 0-based) replaces the resampler, as Engine.process_multi's base_sample_inds."""
    off = np.asarray(packed["offsets"])
    Q = off.size - 1
    S = np.asarray(samples["offset_samples"]).size
    D = int(max_dlas)
    if uniforms is None and forced is None and D > 1:
        uniforms = np.random.default_rng(2003).random((D - 1, S))
    res = []
    for q in range(Q):
        a, b = off[q], off[q + 1]
        spec = dict(wavelengths=packed["wavelengths"][a:b], flux=packed["flux"][a:b],
                    noise_variance=packed["noise_variance"][a:b], pixel_mask=packed["pixel_mask"][a:b].astype(bool),
                    z_qso=float(packed["z_qsos"][q]))
        res.append(process_spectrum(spec, model, samples, D, None if sub_dla is None else sub_dla["nhi"], forest,
                                    uniforms, None if forced is None else np.asarray(forced)[:, q],
                                    num_lines=params.num_lines, absorption_mode=params.absorption_mode))
    out = dict(log_likelihoods_no_dla=np.array([r["log_likelihood_no_dla"] for r in res]),
               min_z_dlas=np.array([r["min_z_dla"] for r in res]), max_z_dlas=np.array([r["max_z_dla"] for r in res]),
               num_pixels=np.array([r["n"] for r in res], dtype=np.int32))
    sll = np.stack([r["sample_log_likelihoods_dla"] for r in res], axis=1)          # D x Q x S
    lld = np.stack([r["log_likelihoods_dla"] for r in res], axis=1)                 # D x Q
    base = np.stack([r["base_sample_inds"] for r in res], axis=1).astype(np.int32)  # (D - 1) x Q x S
    if D == 1:
        out.update(sample_log_likelihoods_dla=sll[0], log_likelihoods_dla=lld[0])
    else:
        out.update(sample_log_likelihoods_dla=sll, log_likelihoods_dla=lld, max_dlas=D, base_sample_inds=base)
    if sub_dla is not None:
        out["sample_log_likelihoods_lls"] = np.stack([r["sample_log_likelihoods_lls"] for r in res])
        out["log_likelihoods_lls"] = np.array([r["log_likelihood_lls"] for r in res])
    if summaries is not None and summaries is not False:
        offs = np.asarray(samples["offset_samples"], dtype=np.float64)
        ind, mll, mz, mn = PO.map_parameters(sll, base, out["min_z_dlas"], out["max_z_dlas"], offs, samples["log_nhi_samples"])
        out.update(map_sample_inds=ind, map_log_likelihoods=mll, MAP_z_dlas=mz[:, :, :D], MAP_log_nhis=mn[:, :, :D])
        if sub_dla is not None:
            ind, mll, mz, mn = PO.map_parameters(out["sample_log_likelihoods_lls"][None], None, out["min_z_dlas"],
                                                 out["max_z_dlas"], offs, sub_dla["log_nhi"])
            out.update(map_sample_ind_lls=ind[0], map_log_likelihood_lls=mll[0], MAP_z_lls=mz[0, :, 0],
                       MAP_log_nhi_lls=mn[0, :, 0])
    return out


# ------------------------------------------------------------------------------------------ priors
def priors(p, ratio, max_dlas):
    """(Pr(none), Pr(exactly d DLAs) [D], Pr(sub)) for the DLA prior p = M / N."""
    D = int(max_dlas)
    dla = [p ** d - p ** (d + 1) for d in range(1, D)] + [p ** D]
    return 1 - p - ratio * p, np.array(dla), ratio * p

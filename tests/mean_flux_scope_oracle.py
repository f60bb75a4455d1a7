"""Numpy restatement of the forest's mean_flux_scope, on sub_dla_forest_oracle.py.

With F = exp(-sum_i t_i(tau_0^mf, beta^mf)) per unmasked in-range pixel at its own wavelength
(sub_dla_forest_oracle.forest_tau), sub_dla_forest_oracle.apply_forest is followed by
  "mu"    nothing                                  (mu <- mu F only: apply_forest itself)
  "mu_M"  M <- M F[:, None]                        (the Ho, Bird & Garnett 2020 lineage's inference)
  "all"   M <- M F[:, None],  omega^2 <- omega^2 F^2   (after the variance series)
so that under "all"  y ~ N(F mu, diag(F) M M' diag(F) + diag(F^2 omega^2 + sigma^2)): the model that
training on y / F, sigma^2 / F^2 learns, written for y.  Every model (null, sub-DLA, every DLA level) uses
the scaled quantities.
"""
import numpy as np

import sub_dla_forest_oracle as SO

SCOPES = {"mu": 0, "mu_M": 1, "all": 2}
FOREST_DEFAULTS = dict(SO.FOREST_DEFAULTS, mean_flux_scope="mu")


def mean_flux(spec, forest, wavelengths=None):
    """F at the pixels prepare_spectrum keeps (or at ``wavelengths``)."""
    f = dict(FOREST_DEFAULTS, **forest)
    w = SO.unmasked_wavelengths(spec) if wavelengths is None else np.asarray(wavelengths, dtype=np.float64)
    return np.exp(-SO.forest_tau(w, spec["z_qso"], f["mean_flux_tau_0"], f["mean_flux_beta"], f["num_forest_lines"]))


def apply_forest(prep, spec, model, forest, wavelengths=None):
    """sub_dla_forest_oracle.apply_forest, then what ``forest["mean_flux_scope"]`` adds."""
    if forest is None:
        return prep
    f = dict(FOREST_DEFAULTS, **forest)
    scope = SCOPES[f.pop("mean_flux_scope")]
    out = SO.apply_forest(prep, spec, model, f, wavelengths)
    if scope == 0:
        return out
    assert f["mean_flux"], "a scope other than mu needs the mean flux"
    F = mean_flux(spec, f, wavelengths)
    out["M"] = prep["M"] * F[:, None]
    if scope == 2:
        out["omega2"] = out["omega2"] * F ** 2
    return out


class SpectrumOracle(SO.SpectrumOracle):
    """sub_dla_forest_oracle's spectrum under a scoped forest.  ``base``: an oracle of the same spectrum,
    model, samples and mode whose sample profiles (which no forest setting touches) are reused."""

    def __init__(self, spec, model, samples, num_lines=3, absorption_mode="reference", forest=None, base=None):
        if base is None:
            super().__init__(spec, model, samples, num_lines, absorption_mode, None)
        else:
            self.__dict__.update(base.__dict__)
        self.num_lines = num_lines
        if self.ok:
            plain = base.plain if base is not None else self.prep
            self.plain = plain                     # prepare_spectrum's own dict
            self.prep = apply_forest(plain, spec, model, forest)


def process_spectrum(spec, model, samples, max_dlas=1, sub_nhi=None, forest=None, uniforms=None, forced=None,
                     num_lines=3, absorption_mode="reference", oracle=None):
    """sub_dla_forest_oracle.process_spectrum under a scoped forest."""
    so = oracle or SpectrumOracle(spec, model, samples, num_lines, absorption_mode, forest)
    return SO.process_spectrum(spec, model, samples, max_dlas, sub_nhi, None, uniforms, forced, num_lines,
                               absorption_mode, oracle=so)


def compute(model, samples, packed, params, device=0, **kw):
    """sub_dla_forest_oracle.compute (the engine stand-in of process_qsos(..., compute=...)) with the
    spectra prepared by this module's SpectrumOracle: its ``forest`` may carry ``mean_flux_scope``."""
    saved = SO.SpectrumOracle
    SO.SpectrumOracle = SpectrumOracle
    try:
        return SO.compute(model, samples, packed, params, device, **kw)
    finally:
        SO.SpectrumOracle = saved

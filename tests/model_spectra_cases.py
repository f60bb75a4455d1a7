"""The inputs test_model_spectra.py (CPU: the oracle's two forms agree on them) and test_gpu_model_spectra.py
(the stand-alone entry against the oracle) share.  A case = a model rank, num_lines, an absorption mode, a few
spectra (Q <= 8, n <= 300) and each spectrum's absorbers [(z, log N_HI), ...].  Noise: synthetic.make_spectrum
draws sigma^2 from U(0.01, 0.09) around a continuum of order 1, so sigma >= 0.1 of the continuum."""
import functools

import numpy as np

from gp_dla_detection_amd import parameters as P
from gp_dla_detection_amd import synthetic as syn

SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)
RANKS = (4, 8, 10, 12, 16, 20, 24)       # GPDLA_FOR_EACH_RANK
BETWEEN = 6                              # runs zero-padded on the rank-8 kernel
FOREST = dict(num_forest_lines=31, variance_series=True, mean_flux=True, mean_flux_tau_0=0.0023, mean_flux_beta=3.65)


def z_range(spec):
    """min_z / max_z of the search on a spectrum (process_qsos.m:160-161)."""
    wl = np.asarray(spec["wavelengths"])
    rest = wl / (1 + spec["z_qso"])
    w = wl[(rest >= P.MIN_LAMBDA) & (rest <= P.MAX_LAMBDA) & ~np.asarray(spec["pixel_mask"], dtype=bool)]
    zmin = max(w.min() / P.LYA_WAVELENGTH - 1, P.LYMAN_LIMIT * (1 + spec["z_qso"]) / P.LYA_WAVELENGTH - 1 + P.MIN_Z_CUT)
    return zmin, w.max() / P.LYA_WAVELENGTH - 1 - P.MAX_Z_CUT


def _mid(spec, f):
    lo, hi = z_range(spec)
    return lo + f * (hi - lo)


def _absorber_sets(spec):
    """0, 1, 2 and 4 absorbers and the edge ones, placed on this spectrum."""
    lo, hi = z_range(spec)
    return [[],
            [(_mid(spec, 0.5), 20.8)],
            [(_mid(spec, 0.40), 21.0), (_mid(spec, 0.41), 20.5)],                       # two overlapping
            [(_mid(spec, 0.2), 20.3), (_mid(spec, 0.45), 21.4), (_mid(spec, 0.6), 20.0), (_mid(spec, 0.9), 22.0)],
            [(lo, 20.6), (hi, 21.2)],                                                   # at min_z and at max_z
            [(_mid(spec, 0.5), 23.0)],                                                  # a ~ 0 over most of the range
            [(_mid(spec, 0.3), 20.0)]]


@functools.lru_cache(maxsize=None)
def cases():
    out = {}

    def add(name, k, spectra, absorbers, num_lines=3, mode="reference", forest=None):
        out[name] = dict(k=k, model=syn.make_model(k=k), spectra=spectra, absorbers=absorbers, num_lines=num_lines,
                         mode=mode, forest=forest, params=P.set_parameters(k=k, num_lines=num_lines, absorption_mode=mode))

    m20 = syn.make_model(k=20)
    for half, sizes in (("a", SIZES[:5]), ("b", SIZES[5:])):
        spectra = [syn.make_spectrum(m20, 10 + i, n_target=n, dla_fraction=0.0) for i, n in enumerate(sizes)]
        spectra.append(syn.make_spectrum(m20, 20, n_target=40, mask_fraction=1.0))      # no usable pixel
        ab = [_absorber_sets(s)[(i + (2 if half == "b" else 0)) % 4] for i, s in enumerate(spectra[:-1])] + [[]]
        add("sizes_" + half, 20, spectra, ab)
    m8 = syn.make_model(k=8)
    masked = [syn.make_spectrum(m8, 30 + i, n_target=257, mask_fraction=0.3) for i in range(7)]
    for mode in ("reference", "unmasked"):
        add("masked_" + mode, 8, masked, [_absorber_sets(s)[i] for i, s in enumerate(masked)], mode=mode)
    m4 = syn.make_model(k=4)
    few = [syn.make_spectrum(m4, 40 + i, n_target=130, mask_fraction=0.1) for i in range(3)]
    for nl in (1, 31):
        add(f"lines_{nl}", 4, few, [_absorber_sets(s)[i + 1] for i, s in enumerate(few)], num_lines=nl)
    for k in RANKS + (BETWEEN,):
        mk = syn.make_model(k=k)
        sp = [syn.make_spectrum(mk, 50 + i, n_target=n, mask_fraction=0.1) for i, n in enumerate((65, 130))]
        add(f"rank_{k}", k, sp, [_absorber_sets(sp[0])[2], _absorber_sets(sp[1])[3]], mode="unmasked")
    fs = [syn.make_spectrum(m8, 60, z_qso=3.1, n_target=None, mask_fraction=0.05, blue_limit=4700.0),
          syn.make_spectrum(m8, 61, n_target=270, mask_fraction=0.05)]
    for scope in (None, "mu", "mu_M", "all"):
        forest = dict(FOREST) if scope is None else dict(FOREST, mean_flux_scope=scope)
        add("forest_" + str(scope), 8, fs, [_absorber_sets(fs[0])[2], _absorber_sets(fs[1])[1]], forest=forest)
    # past GPDLA_MODEL_SPECTRA_LDS (1,024 positions): the per-pixel weights go through the global workspace.  The
    # one shape over n = 300: the path cannot be met below it
    lg = [syn.make_spectrum(m8, 70, z_qso=3.4, n_target=1100, mask_fraction=0.05), syn.make_spectrum(m8, 71, n_target=65)]
    for mode in ("reference", "unmasked"):
        add("long_" + mode, 8, lg, [_absorber_sets(lg[0])[3], _absorber_sets(lg[1])[1]], mode=mode)
    return out


def absorber_arrays(absorbers):
    """[Q][4] NaN-padded z and log N_HI, and the counts."""
    Q = len(absorbers)
    z, n = np.full((Q, 4), np.nan), np.full((Q, 4), np.nan)
    for q, ab in enumerate(absorbers):
        for i, (zz, nn) in enumerate(ab):
            z[q, i], n[q, i] = zz, nn
    return z, n, np.array([len(ab) for ab in absorbers], dtype=np.int32)

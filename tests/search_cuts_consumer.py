"""Run the reference's population statistics under its survey cuts -- CDDF_analysis/calc_cddf.py DLACatalogue with
``lowzcut`` (:351-352, :738-741), with ``filter_noisy_pixels`` (:362-365, :387-438, :742-747) and with both -- on
a processed file written by this package, and print the numbers as JSON.  Executed by
tests/golden/make_search_cuts_fixture.py with an interpreter that has h5py; argv: reference CDDF_analysis dir,
processed file, DLA-samples file, SNR file, then a file holding a JSON object with ``z_bins``, ``nhi_bins``, ``noise_thresh`` and
``pixel_noise`` (one list per spectrum: the noise variance of the pixels of its search range, in pixel order --
what ``find_pixel_noise`` would have stored; its writer is commented out in ``compute_all_snrs``, so the attribute
is set here).  Never runs where the reference is absent."""
import json
import sys
import warnings

sys.dont_write_bytecode = True   # never write __pycache__ into the read-only reference tree

warnings.filterwarnings("ignore")
import numpy as np  # noqa: E402

if not hasattr(np, "bool"):
    np.bool = bool  # calc_cddf.py:84 uses the alias numpy 1.24 removed
if not hasattr(np, "int"):
    np.int = int    # ... and :746
import matplotlib  # noqa: E402

matplotlib.use("Agg")
sys.path.insert(0, sys.argv[1])
import calc_cddf  # noqa: E402

_reference_pdf = calc_cddf.get_poisson_binomial_pdf


def _pdf_of_flat_list(pp):
    """See population_consumer.py: numpy >= 1.24 refuses np.size of a ragged list (calc_cddf.py:1024)."""
    return _reference_pdf([np.concatenate(pp)] if len(pp) else pp)


calc_cddf.get_poisson_binomial_pdf = _pdf_of_flat_list
proc, samp, snrs = sys.argv[2:5]
with open(sys.argv[5]) as fh:      # a file: the noise vectors do not fit an argument list
    ask = json.load(fh)
zb, nb = np.array(ask["z_bins"]), np.array(ask["nhi_bins"])
z_lo, z_hi, n_lo, n_hi = float(zb[0]), float(zb[-1]), float(nb[0]), float(nb[-1])
noise = np.empty(len(ask["pixel_noise"]), dtype=object)
for i, v in enumerate(ask["pixel_noise"]):
    noise[i] = np.array(v, dtype=np.float64)
out = {}
for setting, lowz, pixels in (("proximity", True, False), ("pixels", False, True), ("both", True, True)):
    cat = calc_cddf.DLACatalogue(processed_file=proc, sample_file=samp, raw_file=None, snrs_file=snrs, snr=-2, lowzcut=lowz)
    cat.snrs = np.ravel(cat.snrs)
    if pixels:
        cat.filter_noisy_pixels, cat.noise_thresh, cat.pixel_noise = True, float(ask["noise_thresh"]), noise
    res = dict(proximity_zone=float(cat.proximity_zone))
    for name, nhi, bins in (("nhi", True, nb), ("z", False, zb)):
        kw = dict(lred=z_lo, ured=z_hi, lnhi_min=n_lo, lnhi_max=n_hi, nhi=nhi)
        probs, poissons = cat._split_distributions_single(bins, **kw)
        maxlikes, l68, l95 = cat._get_confidence_intervals(q_bins=bins, **kw)
        res[name] = dict(lists=[np.concatenate(pp).tolist() if len(pp) else [] for pp in probs],
                         poissons=np.asarray(poissons).tolist(), maxlikes=[int(v) for v in maxlikes],
                         l68=[[int(a), int(b)] for a, b in l68], l95=[[int(a), int(b)] for a, b in l95])
    # (the moment estimator cat.omega_dla is not run: it divides by the cut path but bins its samples uncut, since
    # only _split_distributions_single applies the sample tests)
    if setting != "both":     # with both cuts the reference's path squeezes the pixel map: only its sample side is kept
        res["path_total"] = float(cat.path_length(z_lo, z_hi))
        res["path_bins"] = [float(cat.path_length(float(a), float(b))) for a, b in zip(zb[:-1], zb[1:])]
        cent, cddf, c68, c95, _ = cat.column_density_function(z_min=z_lo, z_max=z_hi, lnhi_nbins=nb.size - 1, lnhi_min=n_lo,
                                                              lnhi_max=n_hi)
        res["cddf"] = dict(cent=np.asarray(cent).tolist(), f=np.asarray(cddf).tolist(), f68=np.asarray(c68).tolist(),
                           f95=np.asarray(c95).tolist())
        zc, dndx, d68, d95, _ = cat.line_density(z_min=z_lo, z_max=z_hi)
        res["dndx"] = dict(cent=np.asarray(zc).tolist(), f=np.asarray(dndx).tolist(), f68=np.asarray(d68).tolist(),
                           f95=np.asarray(d95).tolist())
    out[setting] = res
print(json.dumps(out))

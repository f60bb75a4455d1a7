"""Run the reference's own population statistics -- CDDF_analysis/calc_cddf.py DLACatalogue
``_split_distributions_single`` (calc_cddf.py:724-778), ``get_poisson_binomial_pdf`` (:1021-1044),
``_get_combined_levels`` / ``_get_confidence_intervals`` (:780-827), ``path_length`` (:334-385),
``column_density_function`` (:440-464), ``line_density`` (:490-507) and ``omega_dla`` (:638-662) -- on a
processed file written by this package, and print the numbers as JSON.  Executed by
tests/golden/make_population_fixture.py with an interpreter that has h5py; argv: reference CDDF_analysis
dir, processed file, DLA-samples file, SNR file, then a JSON object with ``z_bins`` and ``nhi_bins`` (bin
edges).  Never runs where the reference is absent."""
import json
import sys
import warnings

sys.dont_write_bytecode = True   # never write __pycache__ into the read-only reference tree

warnings.filterwarnings("ignore")
import numpy as np  # noqa: E402

if not hasattr(np, "bool"):
    np.bool = bool  # calc_cddf.py:84 uses the alias numpy 1.24 removed
import matplotlib  # noqa: E402

matplotlib.use("Agg")
sys.path.insert(0, sys.argv[1])
import calc_cddf  # noqa: E402

_reference_pdf = calc_cddf.get_poisson_binomial_pdf


def _pdf_of_flat_list(pp):
    """calc_cddf.py:1024 takes np.size of the list of per-spectrum arrays, which numpy >= 1.24 refuses when
    they differ in length; it only concatenates them afterwards (:1026), so hand it the concatenation."""
    return _reference_pdf([np.concatenate(pp)] if len(pp) else pp)


calc_cddf.get_poisson_binomial_pdf = _pdf_of_flat_list
proc, samp, snrs = sys.argv[2:5]
ask = json.loads(sys.argv[5])
zb, nb = np.array(ask["z_bins"]), np.array(ask["nhi_bins"])
cat = calc_cddf.DLACatalogue(processed_file=proc, sample_file=samp, raw_file=None, snrs_file=snrs, snr=-2)
# a MATLAB-style SNR file gives (1, Q); flatten it so the spectra are indexed as calc_cddf.py:286-291
# intends (see posterior_summary_consumer.py)
cat.snrs = np.ravel(cat.snrs)
z_lo, z_hi, n_lo, n_hi = float(zb[0]), float(zb[-1]), float(nb[0]), float(nb[-1])
LEVELS = (0.5, 0.5 - 0.34, 0.5 + 0.34, 0.5 - 0.475, 0.5 + 0.475, 5e-5, 1 - 5e-5)
out = dict(p_thresh_spec=float(cat.p_thresh_spec), p_thresh_sample=float(cat.p_thresh_sample),
           p_switch=float(cat.p_switch))
for name, nhi, bins in (("nhi", True, nb), ("z", False, zb)):
    kw = dict(lred=z_lo, ured=z_hi, lnhi_min=n_lo, lnhi_max=n_hi, nhi=nhi)
    probs, poissons = cat._split_distributions_single(bins, **kw)
    lists = [np.concatenate(pp).tolist() if len(pp) else [] for pp in probs]
    pdfs, gaps = [], []
    for pp, pmean in zip(probs, poissons):
        pdf = calc_cddf.get_poisson_binomial_pdf(pp)
        pdfs.append(np.asarray(pdf, dtype=np.float64).tolist())
        comb, _ = cat._get_combined_levels(pdf, pmean)
        cdfs = [np.cumsum(comb)] + ([np.cumsum(pdf)] if pmean != 0.0 else [])
        gaps.append(min(float(np.min(np.abs(c[:, None] - np.array(LEVELS)[None, :]))) for c in cdfs))
    maxlikes, l68, l95 = cat._get_confidence_intervals(q_bins=bins, **kw)
    out[name] = dict(lists=lists, poissons=np.asarray(poissons).tolist(), pdfs=pdfs, level_gap=min(gaps),
                     maxlikes=[int(v) for v in maxlikes], l68=[[int(a), int(b)] for a, b in l68],
                     l95=[[int(a), int(b)] for a, b in l95])
out["path_total"] = float(cat.path_length(z_lo, z_hi))
out["path_bins"] = [float(cat.path_length(float(a), float(b))) for a, b in zip(zb[:-1], zb[1:])]
cent, cddf, c68, c95, _ = cat.column_density_function(z_min=z_lo, z_max=z_hi, lnhi_nbins=nb.size - 1, lnhi_min=n_lo,
                                                      lnhi_max=n_hi)
out["cddf"] = dict(cent=np.asarray(cent).tolist(), f=np.asarray(cddf).tolist(), f68=np.asarray(c68).tolist(),
                   f95=np.asarray(c95).tolist())
assert ask["line_density_defaults"], "line_density and omega_dla take their bins from z_min, z_max and bins_per_z"
zc, dndx, d68, d95, _ = cat.line_density(z_min=z_lo, z_max=z_hi)
out["dndx"] = dict(cent=np.asarray(zc).tolist(), f=np.asarray(dndx).tolist(), f68=np.asarray(d68).tolist(),
                   f95=np.asarray(d95).tolist())
zc, om, err, zbins = cat.omega_dla(z_min=z_lo, z_max=z_hi, lnhi_max=n_hi, lnhi_min=n_lo)
out["omega"] = dict(cent=np.asarray(zc).tolist(), omega=np.asarray(om).tolist(), err=np.asarray(err).tolist(),
                    z_bins=np.asarray(zbins).tolist())
print(json.dumps(out))

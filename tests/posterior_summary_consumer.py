"""Run the reference's own population statistics -- CDDF_analysis/calc_cddf.py DLACatalogue
``_get_z_nhi_hist`` (calc_cddf.py:829-870) and ``find_max_like`` (:888-893) -- on a processed file
written by this package, and print the numbers as JSON.  Executed by
tests/golden/make_posterior_summary_fixture.py with an interpreter that has h5py; argv: reference
CDDF_analysis dir, processed file, DLA-samples file, SNR file, then a JSON object with ``z_bins``,
``nhi_bins`` (bin edges) and ``map_rows``.  Never runs where the reference is absent."""
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

proc, samp, snrs = sys.argv[2:5]
ask = json.loads(sys.argv[5])
zb, nb = np.array(ask["z_bins"]), np.array(ask["nhi_bins"])
cat = calc_cddf.DLACatalogue(processed_file=proc, sample_file=samp, raw_file=None, snrs_file=snrs, snr=-2)
# the reference's own SNR files hold a 1-D dataset (calc_cddf.py writes them with h5py); a MATLAB-style
# file gives (1, Q), which turns filter_dla_spectra's np.where into row indices (all 0).  Flatten it so
# the spectra are indexed as calc_cddf.py:286-291 intends.
cat.snrs = np.ravel(cat.snrs)
out = dict(p_thresh_spec=float(cat.p_thresh_spec), hist={}, max_like={})
for nhi in (False, True):
    for moment in (False, True):
        means, variances = cat._get_z_nhi_hist(nb if nhi else zb, lred=float(zb[0]), ured=float(zb[-1]),
                                               lnhi_min=float(nb[0]), lnhi_max=float(nb[-1]), nhi=nhi, moment=moment)
        out["hist"][f"nhi{int(nhi)}_moment{int(moment)}"] = [means.tolist(), variances.tolist()]
for spec in ask["map_rows"]:
    lnhi, z = cat.find_max_like(spec)
    out["max_like"][str(spec)] = [float(lnhi), float(z)]
print(json.dumps(out))

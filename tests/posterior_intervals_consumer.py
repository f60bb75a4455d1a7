"""Run the reference's own likelihood-ratio ranges -- CDDF_analysis/calc_cddf.py DLACatalogue
``find_delta_NHI`` and ``find_delta_z`` (calc_cddf.py:872-886) -- on a processed file written by this package,
and print the numbers as JSON.  Executed by tests/golden/make_posterior_intervals_fixture.py with an interpreter
that has h5py; argv: reference CDDF_analysis dir, processed file, DLA-samples file, SNR file, then a JSON object
with ``rows``.  Never runs where the reference is absent."""
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
cat = calc_cddf.DLACatalogue(processed_file=proc, sample_file=samp, raw_file=None, snrs_file=snrs, snr=-2)
cat.snrs = np.ravel(cat.snrs)    # a MATLAB-style (1, Q) SNR dataset: see posterior_summary_consumer.py
kept = set(int(i) for i in np.ravel(cat.filter_dla_spectra()[0]))
out = dict(p_thresh_spec=float(cat.p_thresh_spec), kept=sorted(kept), delta_nhi={}, delta_z={})
for spec in ask["rows"]:
    # repr round-trips a double exactly
    out["delta_nhi"][str(spec)] = repr(float(cat.find_delta_NHI(spec)))
    out["delta_z"][str(spec)] = repr(float(cat.find_delta_z(spec)))
print(json.dumps(out))

"""Regenerate tests/golden/posterior_intervals.npz: synthetic sample log-likelihood rows, written through this
package's own writers, and the reference's likelihood-ratio ranges of them (CDDF_analysis/calc_cddf.py
``find_delta_NHI`` / ``find_delta_z``, run by tests/posterior_intervals_consumer.py).  CPU only; needs the
reference tree and an interpreter with h5py.

    python tests/golden/make_posterior_intervals_fixture.py <reference/CDDF_analysis> [<python with h5py>]

Q = 8 rows of S = 333, smooth surfaces of different widths.  Asserted here, so the comparison is bit for bit:
every row passes the reference's p_thresh_spec and SNR filters; no sample lies within 1e-9 of m - 2 (the
reference compares after subtracting a constant from every sample, the package before); at least one row has
three or more samples inside the range and at least one exactly one, whose width is 0."""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import posterior_intervals_oracle as IO  # noqa: E402
from gp_dla_detection_amd import matv73 as M  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402

Q, S = 8, 333


def build():
    rng = np.random.default_rng(20261021)
    offset = rng.uniform(0.0, 1.0, S)
    log_nhi = rng.uniform(19.8, 23.2, S)
    samples = dict(offset_samples=offset, log_nhi_samples=log_nhi, nhi_samples=10.0 ** log_nhi)
    min_z = np.array([2.05, 1.80, 2.30, 2.10, 2.60, 2.00, 3.10, 2.20])
    max_z = np.array([3.10, 2.90, 3.60, 3.95, 3.40, 3.20, 4.40, 2.80])
    z0 = np.array([2.4, 2.5, 3.1, 3.7, 2.9, 2.6, 3.8, 2.5])
    n0 = np.array([20.4, 21.2, 20.9, 22.3, 21.7, 20.2, 21.0, 22.8])
    sz = np.array([0.05, 0.30, 0.10, 0.002, 0.15, 0.08, 0.20, 0.04])     # row 3: one sample carries the range
    sn = np.array([0.20, 0.60, 0.15, 0.04, 0.10, 0.30, 0.50, 0.25])
    ll = np.empty((Q, S))
    for q in range(Q):
        z = min_z[q] + (max_z[q] - min_z[q]) * offset
        ll[q] = -1500.0 - 37.0 * q - 0.5 * ((z - z0[q]) / sz[q]) ** 2 - 0.5 * ((log_nhi - n0[q]) / sn[q]) ** 2
    p_dlas = np.array([0.97, 0.41, 0.30, 0.88, 0.0501, 0.51, 0.66, 0.999])
    mx = ll.max(axis=1)
    ll_dla = mx + np.log(np.mean(np.exp(ll - mx[:, None]), axis=1))
    inside = (ll > (mx - 2.0)[:, None]).sum(axis=1)
    assert np.abs(ll - (mx - 2.0)[:, None]).min() > 1e-9, "a sample lies at the threshold"
    assert (inside >= 3).any() and (inside == 1).any(), inside
    return samples, min_z, max_z, ll, p_dlas, ll_dla, inside


def main(ref_cddf: str, py: str):
    samples, min_z, max_z, ll, p_dlas, ll_dla, inside = build()
    out = dict(min_z_dlas=min_z, max_z_dlas=max_z, sample_log_likelihoods_dla=ll, log_likelihoods_dla=ll_dla,
               log_likelihoods_no_dla=np.zeros(Q), log_priors_no_dla=np.zeros(Q), log_priors_dla=np.zeros(Q),
               log_posteriors_no_dla=np.zeros(Q), log_posteriors_dla=ll_dla,
               model_posteriors=np.stack([1 - p_dlas, p_dlas], axis=1), p_no_dlas=1 - p_dlas, p_dlas=p_dlas,
               test_ind=np.ones(Q, dtype=bool), num_lines=3, max_z_cut=0.01, prior_z_qso_increase=0.1,
               training_release="dr12q", training_set_name="synthetic", dla_catalog_name="synthetic",
               prior_ind=np.ones(4, dtype=bool), release="dr12q", test_set_name="synthetic")
    with tempfile.TemporaryDirectory() as tmp:
        proc, samp, snrs = (f"{tmp}/{n}.mat" for n in ("processed_qsos_synthetic", "dla_samples", "snrs_qsos"))
        PR.save_processed_qsos(proc, out)
        PR.save_dla_samples(samp, samples)
        M.savemat73(snrs, dict(snrs=np.full(Q, 5.0)))
        res = subprocess.run([py, "-B", str(ROOT / "tests" / "posterior_intervals_consumer.py"), ref_cddf, proc, samp,
                              snrs, json.dumps(dict(rows=list(range(Q))))], capture_output=True, text=True)
    if res.returncode:
        raise SystemExit(res.stderr[-3000:])
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["kept"] == list(range(Q)), ("a row fails the reference's filters", got["kept"], got["p_thresh_spec"])
    ref_nhi = np.array([float(got["delta_nhi"][str(q)]) for q in range(Q)])
    ref_z = np.array([float(got["delta_z"][str(q)]) for q in range(Q)])
    assert (ref_nhi[inside == 1] == 0.0).all() and (ref_z[inside == 1] == 0.0).all()
    mine = IO.intervals(ll[None], None, min_z, max_z, samples["offset_samples"], samples["log_nhi_samples"], quantiles=False)
    print("oracle == reference:", np.array_equal(mine["log_nhi_lr_ranges"][0, :, 0, 1] - mine["log_nhi_lr_ranges"][0, :, 0, 0], ref_nhi),
          np.array_equal(mine["z_dla_lr_ranges"][0, :, 0, 1] - mine["z_dla_lr_ranges"][0, :, 0, 0], ref_z))
    np.savez(ROOT / "tests" / "golden" / "posterior_intervals.npz", sample_log_likelihoods=ll,
             offset_samples=samples["offset_samples"], log_nhi_samples=samples["log_nhi_samples"], min_z_dlas=min_z,
             max_z_dlas=max_z, lr_counts=inside, ref_delta_nhi=ref_nhi, ref_delta_z=ref_z)
    print(inside, ref_nhi, ref_z)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "/opt/conda/bin/python3.9")

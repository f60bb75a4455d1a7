"""Regenerate tests/golden/posterior_summary.npz: synthetic sample log-likelihood rows, written through
this package's own writers, and what the reference's population statistics make of them
(CDDF_analysis/calc_cddf.py ``_get_z_nhi_hist`` four ways and ``find_max_like``, run by
tests/posterior_summary_consumer.py).  CPU only; needs the reference tree and an interpreter with h5py.

    python tests/golden/make_posterior_summary_fixture.py <reference/CDDF_analysis> [<python with h5py>]

Q = 8 rows of S = 333: smooth surfaces peaked at different (z_DLA, log N_HI); row 5 has 20 % NaN.  The
reference cannot bin a row with NaN (its histogram weights become NaN), so that row and row 2 get a p_dla
below the reference's 0.05 threshold, which exercises the host-side filter; ``find_max_like`` is asked for
the NaN-free rows only.  No sample lies on a bin edge (asserted), so the reference's strict inequalities
and the package's half-open bins select the same samples."""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from gp_dla_detection_amd import matv73 as M  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402

Q, S = 8, 333
NAN_ROW, LOW_ROWS = 5, (2, 5)


def build():
    rng = np.random.default_rng(20261019)
    offset = rng.uniform(0.0, 1.0, S)
    log_nhi = rng.uniform(19.8, 23.2, S)            # some samples fall outside the [20, 23] grid
    samples = dict(offset_samples=offset, log_nhi_samples=log_nhi, nhi_samples=10.0 ** log_nhi)
    min_z = np.array([2.05, 1.80, 2.30, 2.10, 2.60, 2.00, 3.10, 2.20])   # rows 1 and 6 leave the [2, 4] grid
    max_z = np.array([3.10, 2.90, 3.60, 3.95, 3.40, 3.20, 4.40, 2.80])
    z0 = np.array([2.4, 2.5, 3.1, 3.7, 2.9, 2.6, 3.8, 2.5])
    n0 = np.array([20.4, 21.2, 20.9, 22.3, 21.7, 20.2, 21.0, 22.8])
    sz = np.array([0.05, 0.30, 0.10, 0.02, 0.15, 0.08, 0.20, 0.04])
    sn = np.array([0.20, 0.60, 0.15, 0.40, 0.10, 0.30, 0.50, 0.25])
    ll = np.empty((Q, S))
    for q in range(Q):
        z = min_z[q] + (max_z[q] - min_z[q]) * offset
        ll[q] = -1500.0 - 37.0 * q - 0.5 * ((z - z0[q]) / sz[q]) ** 2 - 0.5 * ((log_nhi - n0[q]) / sn[q]) ** 2
    ll[NAN_ROW, rng.permutation(S)[: S // 5]] = np.nan
    p_dlas = np.array([0.97, 0.41, 0.03, 0.88, 0.0501, 0.01, 0.66, 0.999])
    assert all(p_dlas[r] < 0.05 for r in LOW_ROWS)
    mx = np.nanmax(ll, axis=1)
    ll_dla = mx + np.log(np.nanmean(np.exp(ll - mx[:, None]), axis=1))
    z_edges, n_edges = np.linspace(2.0, 4.0, 7), np.linspace(20.0, 23.0, 7)
    for q in range(Q):
        z = min_z[q] + (max_z[q] - min_z[q]) * offset
        assert not np.isin(z, z_edges).any() and not np.isin(log_nhi, n_edges).any(), "a sample lies on a bin edge"
    return samples, min_z, max_z, ll, p_dlas, ll_dla, z_edges, n_edges


def main(ref_cddf: str, py: str):
    samples, min_z, max_z, ll, p_dlas, ll_dla, z_edges, n_edges = build()
    out = dict(min_z_dlas=min_z, max_z_dlas=max_z, sample_log_likelihoods_dla=ll, log_likelihoods_dla=ll_dla,
               log_likelihoods_no_dla=np.zeros(Q), log_priors_no_dla=np.zeros(Q), log_priors_dla=np.zeros(Q),
               log_posteriors_no_dla=np.zeros(Q), log_posteriors_dla=ll_dla,
               model_posteriors=np.stack([1 - p_dlas, p_dlas], axis=1), p_no_dlas=1 - p_dlas, p_dlas=p_dlas,
               test_ind=np.ones(Q, dtype=bool), num_lines=3, max_z_cut=0.01, prior_z_qso_increase=0.1,
               training_release="dr12q", training_set_name="synthetic", dla_catalog_name="synthetic",
               prior_ind=np.ones(4, dtype=bool), release="dr12q", test_set_name="synthetic")
    map_rows = [q for q in range(Q) if not np.isnan(ll[q]).any()]
    with tempfile.TemporaryDirectory() as tmp:
        proc, samp, snrs = (f"{tmp}/{n}.mat" for n in ("processed_qsos_synthetic", "dla_samples", "snrs_qsos"))
        PR.save_processed_qsos(proc, out)
        PR.save_dla_samples(samp, samples)
        M.savemat73(snrs, dict(snrs=np.full(Q, 5.0)))
        ask = dict(z_bins=z_edges.tolist(), nhi_bins=n_edges.tolist(), map_rows=map_rows)
        res = subprocess.run([py, "-B", str(ROOT / "tests" / "posterior_summary_consumer.py"), ref_cddf, proc, samp,
                              snrs, json.dumps(ask)], capture_output=True, text=True)
    if res.returncode:
        raise SystemExit(res.stderr[-3000:])
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["p_thresh_spec"] == 0.05
    ref = {f"ref_{k}": np.array(v) for k, v in got["hist"].items()}           # each 2 x 6: means, variances
    max_like = np.array([got["max_like"][str(q)] for q in map_rows])             # rows x (log N_HI, z)
    np.savez(ROOT / "tests" / "golden" / "posterior_summary.npz", sample_log_likelihoods=ll,
             offset_samples=samples["offset_samples"], log_nhi_samples=samples["log_nhi_samples"],
             nhi_samples=samples["nhi_samples"], min_z_dlas=min_z, max_z_dlas=max_z, p_dlas=p_dlas,
             z_edges=z_edges, log_nhi_edges=n_edges, map_rows=np.array(map_rows), ref_max_like=max_like, **ref)
    print({k: v.shape for k, v in ref.items()}, max_like.shape)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "/opt/conda/bin/python3.9")

"""Regenerate tests/golden/population.npz: synthetic level-1 sample rows, written through this package's
own writers, and what the reference's population statistics make of them (CDDF_analysis/calc_cddf.py
``_split_distributions_single``, ``get_poisson_binomial_pdf``, ``_get_confidence_intervals``,
``path_length``, ``column_density_function``, ``line_density`` and ``omega_dla``, run by
tests/population_consumer.py).  CPU only; needs the reference tree and an interpreter with h5py.

    python tests/golden/make_population_fixture.py <reference/CDDF_analysis> [<python with h5py, scipy and matplotlib>]

Q = 40 rows of S = 300.  Rows 0..11 are sharply peaked (one or two samples carry the row: p >= p_switch)
around two common centres, the others smooth, so both the exact lists and the Poisson planes are populated;
rows 7, 18, 29 have a p_dla below the reference's 0.05 threshold and row 18 also 20 % NaN (the reference
cannot bin a row with NaN).  The grid is what ``line_density`` / ``omega_dla`` build for z in [2, 4] (12 bins) by
``column_density_function`` with 27 bins over [20.3, 23], so the reference's own entry points and one
population grid describe the same bins.

Membership must not hinge on rounding, so the maker asserts, on the reference's numbers alone: no sample z
or log N_HI within 1e-9 of an edge, no p_j within a relative 1e-9 of p_thresh_sample or p_switch, no
combined cdf value within 1e-9 of an interval level.  Change SEED until they hold."""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import population_oracle as PO  # noqa: E402
from gp_dla_detection_amd import matv73 as M  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402

Q, S, SEED = 40, 300, 20261019
LOW_ROWS, NAN_ROW, PEAKED = (7, 18, 29), 18, 12


def build():
    rng = np.random.default_rng(SEED)
    offset = rng.uniform(0.0, 1.0, S)
    log_nhi = rng.uniform(20.0, 23.2, S)             # some samples fall outside the [20.3, 23] grid
    samples = dict(offset_samples=offset, log_nhi_samples=log_nhi, nhi_samples=10.0 ** log_nhi)
    min_z = rng.uniform(1.7, 2.9, Q)                 # some rows start below, some end above the [2, 4] grid
    max_z = min_z + rng.uniform(0.5, 1.6, Q)
    min_z[:6], max_z[:6] = rng.uniform(1.8, 2.2, 6), rng.uniform(2.9, 3.5, 6)
    min_z[6:12], max_z[6:12] = rng.uniform(2.2, 2.4, 6), rng.uniform(3.6, 3.9, 6)
    z0 = rng.uniform(min_z + 0.1, max_z - 0.1)
    n0 = rng.uniform(20.4, 22.6, Q)
    z0[:6], n0[:6] = 2.58, 21.05                     # two clusters, each inside one z bin and one log N_HI bin,
    z0[6:12], n0[6:12] = 3.25, 20.75                 # so some bins collect several exact trials
    sz = np.where(np.arange(Q) < PEAKED, rng.uniform(0.004, 0.02, Q), rng.uniform(0.05, 0.4, Q))
    sn = np.where(np.arange(Q) < PEAKED, rng.uniform(0.02, 0.08, Q), rng.uniform(0.15, 0.8, Q))
    ll = np.empty((Q, S))
    for q in range(Q):
        z = min_z[q] + (max_z[q] - min_z[q]) * offset
        ll[q] = -1800.0 - 11.0 * q - 0.5 * ((z - z0[q]) / sz[q]) ** 2 - 0.5 * ((log_nhi - n0[q]) / sn[q]) ** 2
    ll[NAN_ROW, rng.permutation(S)[: S // 5]] = np.nan
    p_dlas = rng.uniform(0.06, 1.0, Q)
    p_dlas[[0, 3]] = (0.9995, 0.97)
    p_dlas[list(LOW_ROWS)] = (0.03, 0.012, 0.0499)
    mx = np.nanmax(ll, axis=1)
    ll_dla = mx + np.log(np.nanmean(np.exp(ll - mx[:, None]), axis=1))
    z_edges, n_edges = np.linspace(2, 4, 13), np.linspace(20.3, 23.0, 28)
    for q in range(Q):
        z = min_z[q] + (max_z[q] - min_z[q]) * offset
        assert np.abs(z[:, None] - z_edges[None, :]).min() > 1e-9, "a sample z lies on a bin edge"
    assert np.abs(log_nhi[:, None] - n_edges[None, :]).min() > 1e-9, "a sample log N_HI lies on a bin edge"
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
    with tempfile.TemporaryDirectory() as tmp:
        proc, samp, snrs = (f"{tmp}/{n}.mat" for n in ("processed_qsos_synthetic", "dla_samples", "snrs_qsos"))
        PR.save_processed_qsos(proc, out)
        PR.save_dla_samples(samp, samples)
        M.savemat73(snrs, dict(snrs=np.full(Q, 5.0)))
        ask = dict(z_bins=z_edges.tolist(), nhi_bins=n_edges.tolist(), line_density_defaults=True)
        res = subprocess.run([py, "-B", str(ROOT / "tests" / "population_consumer.py"), ref_cddf, proc, samp, snrs,
                              json.dumps(ask)], capture_output=True, text=True)
    if res.returncode:
        raise SystemExit(res.stderr[-3000:])
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert (got["p_thresh_spec"], got["p_thresh_sample"], got["p_switch"]) == (0.05, 1e-4, 0.25)
    # the thresholds: the reference's p_j = exp(l_j - log evidence - log S) p_dla (calc_cddf.py:98,700)
    for q in range(Q):
        if p_dlas[q] <= 0.05:
            continue
        p = np.exp(ll[q] - (ll_dla[q] + np.log(S))) * p_dlas[q]
        for level in (1e-4, 0.25):
            assert np.abs(p / level - 1.0).min() > 1e-9, "a sample probability lies on a threshold"
    save = {}
    worst = 0.0
    for name in ("nhi", "z"):
        g = got[name]
        assert g["level_gap"] > 1e-9, "a combined cdf value lies on an interval level"
        lists = [np.array(v, dtype=np.float64) for v in g["lists"]]
        offsets = np.concatenate([[0], np.cumsum([v.size for v in lists])]).astype(np.int64)
        save[f"ref_{name}_probs"] = np.concatenate(lists) if offsets[-1] else np.zeros(0)
        save[f"ref_{name}_offsets"] = offsets
        save[f"ref_{name}_poissons"] = np.array(g["poissons"])
        save[f"ref_{name}_pdfs"] = np.concatenate([np.array(v, dtype=np.float64) for v in g["pdfs"]])
        save[f"ref_{name}_maxlikes"] = np.array(g["maxlikes"], dtype=np.int64)
        save[f"ref_{name}_l68"] = np.array(g["l68"], dtype=np.int64)
        save[f"ref_{name}_l95"] = np.array(g["l95"], dtype=np.int64)
        # the reference's own deviation from the exact pmf on these lists (its DFT's noise floor)
        for v, pdf in zip(lists, g["pdfs"]):
            worst = max(worst, float(PO.absolute_errors(pdf, PO.exact_pmf(v)).max()))
        assert max(v.size for v in lists) >= 3, "no bin with three exact trials"
    assert save["ref_nhi_offsets"][-1] == save["ref_z_offsets"][-1] > 8
    assert (save["ref_z_poissons"] > 0).sum() > 6
    save["ref_pdf_worst_abs_deviation"] = np.float64(worst)
    save["ref_path_total"], save["ref_path_bins"] = np.float64(got["path_total"]), np.array(got["path_bins"])
    for key in ("cddf", "dndx"):
        for sub, v in got[key].items():
            save[f"ref_{key}_{sub}"] = np.array(v)
    for sub, v in got["omega"].items():
        save[f"ref_omega_{sub}"] = np.array(v)
    np.savez(ROOT / "tests" / "golden" / "population.npz", sample_log_likelihoods=ll,
             offset_samples=samples["offset_samples"], log_nhi_samples=samples["log_nhi_samples"],
             nhi_samples=samples["nhi_samples"], min_z_dlas=min_z, max_z_dlas=max_z, p_dlas=p_dlas,
             z_edges=z_edges, log_nhi_edges=n_edges, **save)
    print({k: getattr(v, "shape", None) for k, v in save.items()}, "reference pmf worst abs deviation", worst)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else sys.executable)

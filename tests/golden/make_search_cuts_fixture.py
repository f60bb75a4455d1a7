"""Regenerate tests/golden/search_cuts.npz: the population fixture's rows (make_population_fixture.build: Q = 40
rows of S = 300, the 12 x 27 grid on z in [2, 4]) with a noise vector for the pixels of every row's search range,
and what the reference's population statistics make of them under ``lowzcut``, under ``filter_noisy_pixels`` and
under both (CDDF_analysis/calc_cddf.py, run by tests/search_cuts_consumer.py).  CPU only; needs the reference
tree and an interpreter with h5py.

    python tests/golden/make_search_cuts_fixture.py <reference/CDDF_analysis> [<python with h5py, scipy and matplotlib>]

Pixel counts n cycle through {2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1250}; rows 0-3 are all good, the others
carry one to three noisy stretches, row 4 is noisy at pixel 0, row 5 at pixel n - 1, and row 39's range is shorter
than the proximity zone.  Stored per setting: the exact lists and Poisson means of both axes and the interval
integers; for one cut alone also the path per bin and in total, f(N) and dN/dX (with both cuts the
reference's path squeezes its pixel map into the shortened range; this package does not, DESIGN.md section 22;
the reference's moment estimator ``omega_dla`` does not cut its samples at all and is left out).

Membership must not hinge on rounding, so the maker asserts, on the reference's expressions alone: no sample's
((z - min_z) / span) n within 1e-9 of an integer, no z within 1e-9 of z_upper or a bin edge, no noise within a
relative 1e-9 of the threshold, no zz[i] within 1e-9 of a pmin / pmax, no p_j on a threshold.  Change SEED until
they hold."""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import make_population_fixture as MP  # noqa: E402
from gp_dla_detection_amd import matv73 as M  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402

SEED, THRESH, ZONE = 20261021, 0.25, 0.1
COUNTS = (2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1250)


def pixel_noise(Q):
    rng = np.random.default_rng(SEED)
    out = []
    for q in range(Q):
        n = COUNTS[q % len(COUNTS)] if q >= 4 else (64, 257, 33, 1250)[q]
        v = rng.uniform(0.01, 0.2, n)
        if q >= 6:
            for _ in range(int(rng.integers(1, 4))):
                a = int(rng.integers(0, n))
                v[a:a + int(rng.integers(1, max(2, n // 5)))] = rng.uniform(0.3, 1.0)
        if q == 4:
            v[0] = 0.7
        if q == 5:
            v[-1] = 0.7
        assert np.abs(v / THRESH - 1.0).min() > 1e-9, "a noise value lies on the threshold"
        out.append(v)
    return out


def check_margins(samples, min_z, max_z, noise, z_edges):
    off = samples["offset_samples"]
    for q in range(min_z.size):
        span = max_z[q] - min_z[q]
        z = min_z[q] + span * off
        assert np.abs(z - (max_z[q] - ZONE)).min() > 1e-9, "a sample z lies on z_upper"
        assert np.abs(z[:, None] - z_edges[None, :]).min() > 1e-9, "a sample z lies on a bin edge"
        n = noise[q].size
        f = (z - min_z[q]) / span * n
        assert np.abs(f - np.rint(f)).min() > 1e-9, "a sample lies on a pixel boundary"
        for top in (max_z[q], max(max_z[q] - ZONE, min_z[q])):
            zz = min_z[q] + (top - min_z[q]) * np.arange(n) / (n - 1)
            marks = np.concatenate([z_edges, [min_z[q], top]])
            d = np.abs(zz[:, None] - marks[None, :])
            d[(zz[:, None] == marks[None, :]) & (np.isin(marks, [min_z[q], top]))[None, :]] = 1.0   # zz_0, zz_{n-1}: exact
            assert d.min() > 1e-9, "a pixel redshift lies on a path bound"


def main(ref_cddf: str, py: str):
    samples, min_z, max_z, ll, p_dlas, ll_dla, z_edges, n_edges = MP.build()
    Q, S = ll.shape
    max_z = max_z.copy()
    max_z[39] = min_z[39] + 0.07                      # the range collapses under the proximity cut
    noise = pixel_noise(Q)
    check_margins(samples, min_z, max_z, noise, z_edges)
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
        ask = dict(z_bins=z_edges.tolist(), nhi_bins=n_edges.tolist(), noise_thresh=THRESH, pixel_noise=[v.tolist() for v in noise])
        Path(f"{tmp}/ask.json").write_text(json.dumps(ask))
        res = subprocess.run([py, "-B", str(ROOT / "tests" / "search_cuts_consumer.py"), ref_cddf, proc, samp, snrs,
                              f"{tmp}/ask.json"], capture_output=True, text=True)
    if res.returncode:
        raise SystemExit(res.stderr[-3000:])
    got = json.loads(res.stdout.strip().splitlines()[-1])
    for q in range(Q):                                 # the thresholds, as make_population_fixture checks them
        if p_dlas[q] > 0.05:
            p = np.exp(ll[q] - (ll_dla[q] + np.log(S))) * p_dlas[q]
            for level in (1e-4, 0.25):
                assert np.abs(p / level - 1.0).min() > 1e-9, "a sample probability lies on a threshold"
    save = {}
    for setting, g in got.items():
        assert g["proximity_zone"] == ZONE
        for name in ("nhi", "z"):
            lists = [np.array(v, dtype=np.float64) for v in g[name]["lists"]]
            offsets = np.concatenate([[0], np.cumsum([v.size for v in lists])]).astype(np.int64)
            save[f"{setting}_{name}_probs"] = np.concatenate(lists) if offsets[-1] else np.zeros(0)
            save[f"{setting}_{name}_offsets"] = offsets
            save[f"{setting}_{name}_poissons"] = np.array(g[name]["poissons"])
            for key in ("maxlikes", "l68", "l95"):
                save[f"{setting}_{name}_{key}"] = np.array(g[name][key], dtype=np.int64)
        if "path_total" in g:
            save[f"{setting}_path_total"], save[f"{setting}_path_bins"] = np.float64(g["path_total"]), np.array(g["path_bins"])
            for key in ("cddf", "dndx"):
                for sub, v in g[key].items():
                    save[f"{setting}_{key}_{sub}"] = np.array(v)
    lens = np.array([v.size for v in noise])
    np.savez(ROOT / "tests" / "golden" / "search_cuts.npz", sample_log_likelihoods=ll,
             offset_samples=samples["offset_samples"], log_nhi_samples=samples["log_nhi_samples"],
             nhi_samples=samples["nhi_samples"], min_z_dlas=min_z, max_z_dlas=max_z, p_dlas=p_dlas, z_edges=z_edges,
             log_nhi_edges=n_edges, noise_offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
             noise_values=np.concatenate(noise), noise_thresh=np.float64(THRESH), proximity_zone=np.float64(ZONE), **save)
    print({k: getattr(v, "shape", None) for k, v in save.items()})


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else sys.executable)

"""Regenerate tests/golden/omega_cddf.npz: what the reference's ``_get_omega_confidence_intervals``
(CDDF_analysis/calc_cddf.py:562-636, run by tests/omega_cddf_consumer.py) makes of the exact lists and Poisson
means of every redshift bin of tests/golden/population.npz, and how far this package's lattice lands from it.
CPU only; needs the reference tree.  Results only: no reference code goes into the file.

    python tests/golden/make_omega_cddf_fixture.py <reference/CDDF_analysis>

The split is the population oracle's (``population_oracle.split_rows``), the pmf the double recurrence and the
lattice ``count_mixture_oracle.numpy_chain`` at CELLS cells, so nothing here needs a GPU.  ``measured_rel_dev``
holds, per level (median, low 68, high 68, low 95, high 95), the largest relative deviation of
``catalog.total_column_intervals`` from the reference over the redshift bins with path; the tests assert at
twice that.  The maker asserts, on the oracle alone, that no lattice cdf value lies within 1e-9 of a level."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import count_mixture_oracle as CO  # noqa: E402
import omega_cddf_consumer as consumer  # noqa: E402
import population_oracle as PO  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402

CELLS, HUBBLE = 2 ** 20, 0.7


def golden_out(g):
    split = PO.split_rows(g["sample_log_likelihoods"], g["min_z_dlas"], g["max_z_dlas"], g["p_dlas"], g["offset_samples"],
                          g["log_nhi_samples"], g["z_edges"], g["log_nhi_edges"])
    out = dict(split)
    for key in ("population_large_inds", "population_large_bins"):
        out[key] = np.asarray(split[key]).astype(np.float64) + 1.0
    out.update(p_dlas=g["p_dlas"], min_z_dlas=g["min_z_dlas"], max_z_dlas=g["max_z_dlas"],
               population_z_edges=g["z_edges"], population_log_nhi_edges=g["log_nhi_edges"])
    return out


def intervals(out, cells, gaps=None):
    lists, means = CAT.split_distributions_grid(out)
    return CAT.total_column_intervals(lists, means, out["population_log_nhi_edges"], cells=cells,
                                      pmf=lambda ls: [PO.recurrence_pmf(v) for v in ls],
                                      mixture=CO.mixture(CO.numpy_chain, gaps))


def main(ref_cddf: str):
    g = np.load(ROOT / "tests" / "golden" / "population.npz")
    out = golden_out(g)
    lists, means = CAT.split_distributions_grid(out)
    nz = means.shape[0]
    ref = np.zeros((nz, 5))
    for iz in range(nz):
        like, l68, l95 = consumer.reference_intervals(ref_cddf, lists[iz], means[iz], g["log_nhi_edges"])
        ref[iz] = (like, l68[0], l68[1], l95[0], l95[1])
        print(iz, ref[iz])
    gaps = []
    mid, l68, l95, steps = intervals(out, CELLS, gaps)
    assert min(gaps) > 1e-9, "a lattice cdf value lies on a level"
    got = np.stack([mid, l68[:, 0], l68[:, 1], l95[:, 0], l95[:, 1]], axis=1)
    path = g["ref_path_bins"] > 0
    assert (ref[path, 0] > 0).sum() >= 6 and (ref[path, 3] > 0).any(), "too few bins with a positive median or lower 95 % end"
    assert np.array_equal(got[path] == 0, ref[path] == 0), "a level is 0 on one side only"
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref > 0, np.abs(got - ref) / ref, 0.0)
    print("relative deviation per bin and level\n", rel)
    measured = rel[path].max(axis=0)
    print("measured", measured, "lattice step / median", (steps[path] / ref[path, 0]).max())
    np.savez(ROOT / "tests" / "golden" / "omega_cddf.npz", cells=np.int64(CELLS), hubble=np.float64(HUBBLE),
             ref_levels=ref, ref_conversion=np.float64(consumer.reference_conversion(ref_cddf, HUBBLE)),
             measured_rel_dev=measured)


if __name__ == "__main__":
    main(sys.argv[1])

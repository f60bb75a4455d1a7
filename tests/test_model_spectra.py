"""Model spectra on the CPU: the oracle's Woodbury and dense forms agree on every input the
GPU tests use (a condition on the inputs, checked here so that the GPU comparison has a reference good to 1e-10),
the catalog helpers on a hand-made output, the capacity bound at the edges of the modelled range, and the argument
checks that need no device."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import model_spectra_cases as MC  # noqa: E402
import model_spectra_oracle as MO  # noqa: E402
from gp_dla_detection_amd import catalog as CT  # noqa: E402
from gp_dla_detection_amd import parameters as P  # noqa: E402
from gp_dla_detection_amd.engine import (MODEL_CAPACITY_GUARD, _absorber_arrays, compact_model_spectra,  # noqa: E402
                                         model_capacities)


@pytest.mark.parametrize("name", sorted(MC.cases()))
def test_oracle_forms_agree_on_the_gpu_inputs(name):
    c = MC.cases()[name]
    worst = 0.0
    for spec, ab in zip(c["spectra"], c["absorbers"]):
        if MO.prepare(spec, c["model"], c["mode"], c["forest"]) is None:
            continue
        z = [a[0] for a in ab]
        nhi = [10.0 ** a[1] for a in ab]
        worst = max(worst, MO.forms_agree(spec, c["model"], z, nhi, c["num_lines"], c["mode"], c["forest"]))
    print(f"{name}: woodbury against dense, worst {worst:.3g}")
    assert worst <= 1e-10


def test_oracle_null_model_is_the_reference_likelihood():
    c = MC.cases()["masked_reference"]
    spec = c["spectra"][0]
    prep = MO.prepare(spec, c["model"])
    got = MO.model_spectrum(spec, c["model"], [], [])
    assert abs(got["log_likelihood"] - MO.O.null_log_likelihood(prep)) <= 1e-10 * abs(got["log_likelihood"])
    assert np.all(got["absorption"] == 1.0) and np.array_equal(got["model_mean"], prep["mu"])
    one = MO.model_spectrum(spec, c["model"], [2.2], [10.0 ** 20.7])
    assert abs(one["log_likelihood"] - MO.O.sample_log_likelihood(prep, 2.2, 10.0 ** 20.7, 3)) <= 1e-10 * abs(one["log_likelihood"])


def _hand_made():
    res = dict(offsets=np.array([0, 3, 3, 5]), pixel_inds=np.array([2, 3, 5, 0, 1], dtype=np.int32),
               absorption=np.array([1.0, 0.5, 0.9, 0.0, np.nan]), model_mean=np.array([1.0, 0.6, 0.9, 0.0, np.nan]),
               continuum=np.array([1.0, 1.2, 1.0, 2.0, np.nan]), continuum_sd=np.array([0.1, 0.2, 0.3, 0.4, np.nan]),
               log_likelihoods=np.array([-3.0, np.nan, -1.0]), chi2=np.array([3.0, np.nan, 8.0]),
               num_pixels=np.array([3, 0, 2], dtype=np.int32))
    return CT.model_spectra_variables(res)


def test_catalog_helpers_on_a_hand_made_output():
    out = _hand_made()
    wl = np.arange(10.0, 16.0)
    s0 = CT.model_spectrum(out, 0, wl)
    assert np.array_equal(s0["pixel_inds"], [2, 3, 5]) and np.array_equal(s0["wavelengths"], [12.0, 13.0, 15.0])
    assert np.array_equal(s0["fit"], [1.0, 0.6, 0.9]) and s0["chi2"] == 3.0 and s0["num_pixels"] == 3
    assert CT.model_spectrum(out, 1)["absorption"].size == 0 and "wavelengths" not in CT.model_spectrum(out, 1)
    with pytest.raises(IndexError):
        CT.model_spectrum(out, 3)
    assert np.array_equal(CT.dla_pixel_mask(out), [False, True, False, True, False])
    assert np.array_equal(CT.dla_pixel_mask(out, 0.95), [False, True, True, True, False])
    with pytest.raises(ValueError):
        CT.dla_pixel_mask(out, 1.5)
    w = CT.wing_correction(out)
    assert w[0] == 1.0 and w[2] == 1.0 / 0.9 and np.isnan(w[1]) and np.isnan(w[3]) and np.isnan(w[4])
    fq = CT.fit_quality(out)
    assert fq["reduced_chi2"][0] == 1.0 and fq["reduced_chi2"][2] == 4.0 and np.isnan(fq["reduced_chi2"][1])
    assert fq["z_score"][0] == 0.0 and fq["z_score"][2] == 3.0 and np.isnan(fq["z_score"][1])


def test_capacity_bounds_n_one_ulp_either_side_of_the_range():
    par = P.set_parameters(k=4)
    z = 2.5
    edges = []
    for lam in (par.min_lambda, par.max_lambda):
        for ulps in (-2, -1, 0, 1, 2):
            r = lam
            for _ in range(abs(ulps)):
                r = np.nextafter(r, np.inf if ulps > 0 else -np.inf)
            edges.append(r * (1 + z))
    wl = np.array(sorted(edges + [1000.0 * (1 + z), 800.0 * (1 + z), 1300.0 * (1 + z)]))
    packed = dict(offsets=np.array([0, wl.size, wl.size]), wavelengths=wl, z_qsos=np.array([z, z]))
    caps = model_capacities(packed, par)
    rest = wl / (1 + z)
    n = np.count_nonzero((rest >= par.min_lambda) & (rest <= par.max_lambda))   # the device's test
    assert caps[0] >= n and caps[0] <= n + 4 and caps[1] == 0
    # every wavelength within the guard band of an edge is counted, whichever way its division rounds
    near = np.abs(rest / par.min_lambda - 1) < 1e-14
    assert near.sum() == 5 and MODEL_CAPACITY_GUARD > 1e-14
    assert caps[0] == 11


def test_absorber_arguments():
    z4, n4, cnt = _absorber_arrays(3, [[2.0, np.nan], [np.nan, np.nan], [2.1, 2.2]], [[20.5, np.nan], [np.nan, np.nan], [21.0, 20.0]], None)
    assert z4.shape == (3, 4) and list(cnt) == [1, 0, 2] and np.isnan(z4[0, 1]) and n4[2, 1] == 20.0
    assert list(_absorber_arrays(2, [], [], None)[2]) == [0, 0]
    with pytest.raises(ValueError):
        _absorber_arrays(1, np.zeros((1, 5)), np.zeros((1, 5)), None)
    with pytest.raises(ValueError):
        _absorber_arrays(1, np.zeros((1, 4)), np.zeros((1, 4)), [5])
    with pytest.raises(ValueError):
        _absorber_arrays(1, np.zeros((1, 2)), np.zeros((1, 3)), None)


def test_compaction_keeps_each_spectrums_leading_values():
    cap = np.array([0, 4, 6, 9])
    out = compact_model_spectra(cap, [2, 0, 3], np.arange(9, dtype=np.int32), dict(absorption=np.arange(9.0)))
    assert list(out["offsets"]) == [0, 2, 2, 5] and list(out["pixel_inds"]) == [0, 1, 6, 7, 8]
    assert list(out["absorption"]) == [0.0, 1.0, 6.0, 7.0, 8.0]

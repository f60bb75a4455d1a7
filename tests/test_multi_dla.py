"""Multi-DLA search, the parts that need no GPU: the numpy oracle of the model (multi_dla_oracle.py),
the priors / posteriors over 1 + D models, and the D > 1 file layout down to the reference's own
consumer (CDDF_analysis/calc_cddf.py DLACatalogue, its ``len(shape) > 2`` branch)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import multi_dla_oracle as MO  # noqa: E402
from oracle import gpdla_oracle as O  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import matv73 as M  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402
from test_matv73 import H5PY_PY, REF_CDDF, needs_h5py  # noqa: E402

K, S, Q = 4, 24, 3


@pytest.fixture(scope="module")
def setup():
    model = syn.make_model(k=K)
    samples = syn.make_samples(S)
    spectra = [syn.make_spectrum(model, q, n_target=120, mask_fraction=0.05, dla_fraction=1.0) for q in range(Q)]
    packed = syn.pack_spectra(spectra)
    params = set_parameters(k=K)
    rng = np.random.default_rng(5)
    prior = dict(z_qsos=rng.uniform(2.0, 4.5, 400), dla_ind=rng.uniform(size=400) < 0.12)
    return dict(model=model, samples=samples, spectra=spectra, packed=packed, params=params, prior=prior)


@pytest.fixture(scope="module")
def outs(setup):
    s = setup
    meta = dict(training_release="dr12q", training_set_name="dr9q_minus_concordance",
                dla_catalog_name="dr9q_concordance", prior_ind=np.ones(400, dtype=bool), release="dr12q",
                test_set_name="dr12q")
    run = lambda D: PR.process_qsos(s["model"], s["samples"], s["packed"], s["prior"], params=s["params"],  # noqa: E731
                                    metadata=meta, max_dlas=D, compute=MO.compute,
                                    test_ind=None)
    o1, o2 = run(1), run(2)
    for o in (o1, o2):
        o["test_ind"] = np.ones(Q, dtype=bool)
    return o1, o2


def test_level_one_is_process_spectrum(setup):
    s = setup
    for spec in s["spectra"]:
        ref = O.process_spectrum(spec["wavelengths"], spec["flux"], spec["noise_variance"], spec["pixel_mask"],
                                 spec["z_qso"], s["model"], s["samples"]["offset_samples"], s["samples"]["nhi_samples"])
        got = MO.process_spectrum_multi(spec, s["model"], s["samples"], 1)
        assert np.array_equal(got["sample_log_likelihoods_dla"][0], ref["sample_log_likelihoods_dla"])
        assert got["log_likelihoods_dla"][0] == ref["log_likelihood_dla"]
        assert got["log_likelihood_no_dla"] == ref["log_likelihood_no_dla"]
        assert got["min_z_dla"] == ref["min_z_dla"] and got["max_z_dla"] == ref["max_z_dla"]


def test_one_dla_priors_and_finish_bitwise(setup, outs):
    s = setup
    z = s["packed"]["z_qsos"]
    lp_no, lp_dla = PR.dla_priors(z, s["prior"]["z_qsos"], s["prior"]["dla_ind"])
    m_no, m_dla = PR.multi_dla_priors(z, s["prior"]["z_qsos"], s["prior"]["dla_ind"], 1)
    assert m_dla.shape == (Q, 1)
    assert np.array_equal(m_no, lp_no) and np.array_equal(m_dla[:, 0], lp_dla)
    # _finish with max_dlas = 1 is today's function: same keys, shapes and bits as the default call
    res = MO.compute(s["model"], s["samples"], s["packed"], s["params"])
    a = PR._finish(res, z, s["prior"], s["params"], None)
    b = PR._finish(res, z, s["prior"], s["params"], None, max_dlas=1)
    assert sorted(a) == sorted(b) and "max_dlas" not in a and "base_sample_inds" not in a
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key
    post, p_no, p_dla = PR.model_posteriors(a["log_posteriors_no_dla"], a["log_posteriors_dla"])
    assert np.array_equal(a["model_posteriors"], post) and a["model_posteriors"].shape == (Q, 2)
    assert a["log_likelihoods_dla"].shape == (Q,) and a["sample_log_likelihoods_dla"].shape == (Q, S)
    o1 = outs[0]
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(o1[key]), equal_nan=True), key


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_priors_sum_to_one(setup, D):
    s = setup
    lp_no, lp_dla = PR.multi_dla_priors(s["packed"]["z_qsos"], s["prior"]["z_qsos"], s["prior"]["dla_ind"], D)
    assert lp_dla.shape == (Q, D)
    total = np.exp(lp_no) + np.exp(lp_dla).sum(axis=1)
    np.testing.assert_allclose(total, 1.0, rtol=0, atol=4e-16)
    with pytest.raises(ValueError):
        PR.multi_dla_priors(s["packed"]["z_qsos"], s["prior"]["z_qsos"], s["prior"]["dla_ind"], 5)


def test_nan_level_enters_with_posterior_zero():
    lp_no = np.array([-10.0, -3.0])
    lp_dla = np.array([[-11.0, np.nan, np.nan], [-2.0, -2.5, -40.0]])
    post, p_no, p_dla = PR.model_posteriors_multi(lp_no, lp_dla)
    assert post.shape == (2, 4) and np.all(post[0, 2:] == 0)
    np.testing.assert_allclose(post.sum(axis=1), 1.0, atol=1e-15)
    assert np.array_equal(p_no, post[:, 0]) and np.array_equal(p_dla, 1 - p_no)


def test_level_two_symmetry_in_the_oracle(setup):
    s = setup
    so = MO.SpectrumOracle(s["spectra"][0], s["model"], s["samples"])
    rng = np.random.default_rng(11)
    b = rng.integers(0, S, S)
    l2 = so.level(b[:, None])
    for j in range(S):
        swapped = so.level(np.where(np.arange(S) == b[j], j, -1)[:, None])[b[j]]   # sample b[j] on base j
        assert (np.isnan(l2[j]) and np.isnan(swapped)) or l2[j] == swapped
    assert np.isfinite(l2).sum() >= S // 2


def test_resampler_oracle_edges():
    u = np.array([0.0, 0.25, 0.4999999, 0.5, 0.75, 0.999999])
    ll = np.array([np.nan, 3.0, -np.inf, 3.0, np.nan, -np.inf])     # weights 0 1 0 1 0 0: C = 0 1 1 2 2 2
    assert MO.resample(ll, u).tolist() == [1, 1, 1, 3, 3, 3]
    assert MO.resample(np.full(6, np.nan), u).tolist() == [-1] * 6
    amb, _ = MO.ambiguous(ll, u)
    assert amb.tolist() == [True, False, False, True, False, False]  # u W exactly on an edge
    w = np.random.default_rng(3).normal(size=200)
    np.testing.assert_allclose(MO.prefix_fsum(MO.weights(w)), np.cumsum(MO.weights(w)), rtol=1e-13)


def test_two_dla_file_layout(tmp_path, setup, outs):
    o1, o2 = outs
    D = 2
    assert o2["log_likelihoods_dla"].shape == (Q, D) and o2["model_posteriors"].shape == (Q, 1 + D)
    np.testing.assert_allclose(o2["model_posteriors"].sum(axis=1), 1.0, atol=1e-15)
    assert np.array_equal(o2["p_dlas"], 1 - o2["model_posteriors"][:, 0])
    path = tmp_path / "processed_qsos_dr12q.mat"
    PR.save_processed_qsos(str(path), o2)
    r = M.loadmat(str(path))
    assert r["sample_log_likelihoods_dla"].shape == (Q, S, D)
    assert np.array_equal(r["sample_log_likelihoods_dla"], o2["sample_log_likelihoods_dla"], equal_nan=True)
    assert np.array_equal(r["sample_log_likelihoods_dla"][:, :, 0], o1["sample_log_likelihoods_dla"])
    for key in ("log_likelihoods_dla", "log_priors_dla", "log_posteriors_dla"):
        assert r[key].shape == (Q, D), key
    assert r["model_posteriors"].shape == (Q, 1 + D)
    assert r["base_sample_inds"].shape == (Q, S) and r["base_sample_inds"].dtype == np.float64
    assert r["base_sample_inds"].min() >= 1 and r["base_sample_inds"].max() <= S       # 1-based
    assert r["max_dlas"].ravel()[0] == 2
    assert set(r) - set(PR.PROCESSED_VARIABLES) == set(PR.MULTI_DLA_VARIABLES)
    # the one-DLA file of the same spectra has none of the extra names
    path1 = tmp_path / "one.mat"
    PR.save_processed_qsos(str(path1), o1)
    assert not set(M.loadmat(str(path1))) & set(PR.MULTI_DLA_VARIABLES)
    # three DLAs: the index array gains its third axis
    s = setup
    o3 = PR.process_qsos(s["model"], s["samples"], s["packed"], s["prior"], params=s["params"], max_dlas=3,
                         compute=MO.compute)
    assert o3["base_sample_inds"].shape == (Q, S, 2) and o3["sample_log_likelihoods_dla"].shape == (Q, S, 3)
    with pytest.raises(ValueError):
        PR.process_qsos(s["model"], s["samples"], s["packed"], max_dlas=5, compute=MO.compute)


def test_sharded_multi_dla_run_not_implemented(tmp_path):
    with pytest.raises(NotImplementedError):
        PR.run_process_qsos(str(tmp_path), "dr12q", "a", "b", None, "dr12q", "dr12q", None, world=2, max_dlas=2)


@needs_h5py
@pytest.mark.skipif(not os.path.isdir(REF_CDDF), reason="reference not present (GPU box)")
def test_reference_consumer_reads_two_dla_file(tmp_path, setup, outs):
    """DLACatalogue takes its 3-D branch (calc_cddf.py:89-90,237-238) on the D = 2 file and loads the
    same log_norm_like as from the D = 1 file of the same spectra."""
    o1, o2 = outs
    samples = setup["samples"]
    got = {}
    for name, out in (("one", o1), ("two", o2)):
        d = tmp_path / name
        d.mkdir()
        proc, samp, snrs = d / "processed_qsos_dr12q.mat", d / "dla_samples.mat", d / "snrs_qsos_dr12q.mat"
        PR.save_processed_qsos(str(proc), out)
        PR.save_dla_samples(str(samp), samples)
        M.savemat73(str(snrs), dict(snrs=np.full(Q, 5.0)))
        res = subprocess.run([H5PY_PY, "-B", str(Path(__file__).parent / "cddf_consumer.py"), REF_CDDF, str(proc),
                              str(samp), str(snrs)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        got[name] = json.loads(res.stdout.strip().splitlines()[-1])
    n1 = {**got["one"]["log_norm_like"], **got["one"]["log_norm_like_on_demand"]}
    n2 = {**got["two"]["log_norm_like"], **got["two"]["log_norm_like_on_demand"]}
    assert n2, "no spectrum passed the reference's p_dla threshold"
    for spec, vals in n2.items():
        want = o2["sample_log_likelihoods_dla"][int(spec), :, 0] - (o2["log_likelihoods_dla"][int(spec), 0] + np.log(S))
        np.testing.assert_allclose(vals, want, rtol=0, atol=1e-12)
        if spec in n1:
            assert np.array_equal(vals, n1[spec])
    assert set(n1) & set(n2), "no spectrum loaded from both files"
    assert np.array_equal(got["two"]["p_dla"], o2["p_dlas"])


def test_multi_entry_points_need_a_device():
    lib = L.load()
    if lib.gpdla_device_count() > 0:
        pytest.skip("a HIP device is present")
    ll, u = np.zeros(8), np.full(8, 0.5)
    out = np.zeros(8, dtype=np.int32)
    assert lib.gpdla_resample_f64(0, L.ptr(ll), 1, 8, 8, L.ptr(u), L.ptr(out, np.ctypeslib.ctypes.c_int32)) == L.GPDLA_EDEVICE
    # argument errors come first, device or not
    u[3] = 1.0
    assert lib.gpdla_resample_f64(0, L.ptr(ll), 1, 8, 8, L.ptr(u), L.ptr(out, np.ctypeslib.ctypes.c_int32)) == L.GPDLA_EINVAL

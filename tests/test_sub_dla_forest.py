"""Sub-DLA model and Lyman-series forest, the parts that need no GPU: the numpy oracle
(sub_dla_forest_oracle.py), the prior ratio, priors / posteriors with the sub-DLA column last, the new
file variables down to the reference's own consumer, and the argument errors."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import multi_dla_oracle as MO  # noqa: E402
import sub_dla_forest_oracle as SO  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import dla_samples as DS  # noqa: E402
from gp_dla_detection_amd import matv73 as M  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402
from test_matv73 import H5PY_PY, REF_CDDF, needs_h5py  # noqa: E402

K, S, Q = 4, 64, 2
FIT = np.array([-0.35, 12.6, -110.0])      # a fixed concave quadratic, peak at log N = 18: both ranges in its tail
RATIO = 0.75


# ------------------------------------------------------------------------------------------ forest
def test_forest_sum_against_double_loop():
    rng = np.random.default_rng(3)
    for z in (2.2, 3.1, 4.9):
        lam = np.sort(rng.uniform(911.75, 1215.5, 200)) * (1 + z)        # (redward of Lya the sum is empty)
        for L_, tau, beta in ((1, 0.0023, 3.65), (3, 0.01, 3.2), (31, 0.0023, 3.65)):
            a, b = SO.forest_tau(lam, z, tau, beta, L_), SO.forest_tau_loops(lam, z, tau, beta, L_)
            # numpy's vector pow and libm's scalar pow may differ in the last place; the sum has <= 31 terms
            np.testing.assert_allclose(a, b, rtol=8 * 2.0 ** -52, atol=0)
            assert np.all(a > 0)
    assert np.array_equal(SO.forest_tau(lam, z, 0.0, 3.65), np.zeros(lam.size))


def test_forest_active_line_counts_by_hand():
    # rest 1215: below Lya (1215.67) only.  rest 1000: below Lya and Lyb (1025.72), above Lyg (972.54).
    # rest 915: below every line down to 915.3 (n = 11, 915.329) at least -- 10 or more
    for z in (2.5, 3.1):
        assert SO.active_lines(1215.0, z) == 1
        assert SO.active_lines(1000.0, z) == 2
        assert SO.active_lines(915.0, z) >= 10
        assert SO.active_lines(915.0, z, num_lines=3) == 3
    assert SO.LINE_WAVELENGTHS[0] == pytest.approx(1215.6701) and SO.LINE_STRENGTHS[0] == 1.0
    assert np.all(np.diff(SO.LINE_WAVELENGTHS) < 0) and np.all(np.diff(SO.LINE_STRENGTHS) < 0)


def test_forest_changes_what_it_should():
    model = syn.make_model(k=K)
    spec = syn.make_spectrum(model, 0, z_qso=3.0, n_target=None, mask_fraction=0.05)   # the whole 911.75-1215.75 range
    from oracle import gpdla_oracle as O
    prep = O.prepare_spectrum(spec["wavelengths"], spec["flux"], spec["noise_variance"], spec["pixel_mask"], spec["z_qso"], model)
    assert SO.unmasked_wavelengths(spec).size == prep["n"]
    assert SO.apply_forest(prep, spec, model, None) is prep
    # one line, variance series only: process_qsos.m:145-147 itself
    one = SO.apply_forest(prep, spec, model, dict(num_forest_lines=1, mean_flux=False))
    np.testing.assert_allclose(one["omega2"], prep["omega2"], rtol=1e-13)
    assert one["mu"] is prep["mu"]
    full = SO.apply_forest(prep, spec, model, {})
    assert np.all(full["omega2"] >= one["omega2"] * (1 - 1e-13)) and np.any(full["omega2"] > one["omega2"] * 1.0001)
    assert np.all(np.abs(full["mu"]) <= np.abs(prep["mu"])) and np.all(np.sign(full["mu"]) == np.sign(prep["mu"]))
    zero = SO.apply_forest(prep, spec, model, dict(variance_series=False, mean_flux_tau_0=0.0))
    assert np.array_equal(zero["mu"], prep["mu"]) and zero["omega2"] is prep["omega2"]


# ------------------------------------------------------------------------------------ prior ratio
def test_sub_dla_prior_ratio_against_quad():
    from scipy.integrate import quad
    g = lambda x: math.exp(np.polyval(FIT, x) - np.polyval(FIT, 20.0))  # noqa: E731
    want = quad(g, 19.5, 20.0, epsabs=0, epsrel=2e-14)[0] / quad(g, 20.0, 23.0, epsabs=0, epsrel=2e-14)[0]
    got = DS.sub_dla_prior_ratio(dict(coeffs=FIT, Z=1.0, bandwidth=0.1))
    assert abs(got - want) <= 1e-12 * want
    assert DS.sub_dla_prior_ratio(FIT) == got
    # a peak between the two ranges (the erf branch) and a convex fit (Gauss-Legendre)
    for coeffs in ((-2.0, 80.4, -800.0), (-1.5, 58.5, -570.0), (0.05, -3.0, 30.0)):
        h = lambda x, c=coeffs: math.exp(np.polyval(c, x) - np.polyval(c, 20.0))  # noqa: E731
        want = quad(h, 19.5, 20.0, epsabs=0, epsrel=2e-14)[0] / quad(h, 20.0, 23.0, epsabs=0, epsrel=2e-14)[0]
        assert abs(DS.sub_dla_prior_ratio(coeffs) - want) <= 1e-12 * want, coeffs
    with pytest.raises(ValueError):
        DS.sub_dla_prior_ratio([1.0, 2.0])
    with pytest.raises(ValueError):
        DS.sub_dla_prior_ratio(FIT, lo=20.0, hi=19.5)


def test_sub_dla_samples_from_given_points():
    u = np.array([0.0, 0.25, 0.5, 1.0])
    d = DS.sub_dla_samples(4, u=u)
    assert np.array_equal(d["lls_log_nhi_samples"], 19.5 + 0.5 * u)
    assert np.array_equal(d["lls_nhi_samples"], 10.0 ** d["lls_log_nhi_samples"])
    with pytest.raises(ValueError):
        DS.sub_dla_samples(3, u=u)
    with pytest.raises(ValueError):
        DS.sub_dla_samples(4, u=u, lo=20.0, hi=20.0)


# ------------------------------------------------------------------------------ priors, posteriors
@pytest.fixture(scope="module")
def setup():
    model = syn.make_model(k=K)
    samples = syn.make_samples(S)
    spectra = [syn.make_spectrum(model, q, n_target=120, mask_fraction=0.05, dla_fraction=1.0) for q in range(Q)]
    packed = syn.pack_spectra(spectra)
    params = set_parameters(k=K)
    rng = np.random.default_rng(5)
    prior = dict(z_qsos=rng.uniform(2.0, 4.5, 400), dla_ind=rng.uniform(size=400) < 0.12)
    sub = DS.sub_dla_samples(S, u=(np.arange(S) * 0.6180339887498949) % 1.0)
    sub["sub_dla_prior_ratio"] = RATIO
    return dict(model=model, samples=samples, spectra=spectra, packed=packed, params=params, prior=prior, sub=sub)


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_priors_with_sub_dla_sum_to_one(setup, D):
    s = setup
    z, pz, pd = s["packed"]["z_qsos"], s["prior"]["z_qsos"], s["prior"]["dla_ind"]
    lp_no, lp_dla, lp_sub = PR.multi_dla_priors(z, pz, pd, D, sub_dla_prior_ratio=RATIO)
    plain_no, plain_dla = PR.multi_dla_priors(z, pz, pd, D)
    assert np.array_equal(lp_dla, plain_dla) and lp_dla.shape == (Q, D)          # Pr(exactly d DLAs) unchanged
    total = np.exp(lp_no) + np.exp(lp_dla).sum(axis=1) + np.exp(lp_sub)
    np.testing.assert_allclose(total, 1.0, rtol=0, atol=4e-16)
    p = np.exp(PR.dla_priors(z, pz, pd)[1])
    none, dla, sub = SO.priors(p, RATIO, D)
    np.testing.assert_allclose(np.exp(lp_no), none, rtol=1e-15)
    np.testing.assert_allclose(np.exp(lp_sub), sub, rtol=1e-15)
    np.testing.assert_allclose(np.exp(lp_dla), dla.T, rtol=1e-14)


def test_prior_of_no_absorber_is_minus_inf_when_exhausted():
    lp_no, lp_sub = PR.sub_dla_priors(np.array([0.1, 0.5, 0.8]), 1.0)
    assert np.isfinite(lp_no[0]) and lp_no[1] == -np.inf and lp_no[2] == -np.inf   # 1 - p - r p = 0.8, 0, -0.6
    np.testing.assert_allclose(np.exp(lp_sub), [0.1, 0.5, 0.8])
    with pytest.raises(ValueError):
        PR.sub_dla_priors(np.array([0.1]), -0.5)
    with pytest.raises(ValueError):
        PR.sub_dla_priors(np.array([0.1]), np.nan)
    post, p_no, p_lls, p_dla = PR.model_posteriors_sub(lp_no + 1.0, np.log([0.1, 0.5, 0.8]) + 2.0, lp_sub + 1.5)
    assert np.all(p_no[1:] == 0) and np.all(np.isfinite(post))
    np.testing.assert_allclose(post.sum(axis=1), 1.0, atol=1e-14)


def test_posterior_rows_and_column_order():
    rng = np.random.default_rng(9)
    lp_no, lp_sub = rng.normal(-300, 5, 7), rng.normal(-300, 5, 7)
    lp_dla = rng.normal(-300, 5, (7, 3))
    lp_dla[2, 2] = np.nan                       # a level without a finite sample enters with posterior 0
    post, p_no, p_lls, p_dla = PR.model_posteriors_sub(lp_no, lp_dla, lp_sub)
    assert post.shape == (7, 1 + 3 + 1) and post[2, 3] == 0
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert np.array_equal(p_no, post[:, 0]) and np.array_equal(p_lls, post[:, -1])   # the sub-DLA column is last
    assert np.array_equal(p_dla, 1 - p_no - p_lls)
    # columns 1..D are model_posteriors_multi's up to the normalisation: "exactly d DLAs" stays at column d
    multi = PR.model_posteriors_multi(lp_no, lp_dla)[0]
    np.testing.assert_allclose(post[:, 1:4] / post[:, 1:4].sum(axis=1, keepdims=True),
                               multi[:, 1:4] / multi[:, 1:4].sum(axis=1, keepdims=True), rtol=1e-13)
    one = PR.model_posteriors_sub(lp_no, lp_dla[:, 0], lp_sub)[0]
    assert one.shape == (7, 3)


# -------------------------------------------------------------------------------- process_qsos, files
@pytest.fixture(scope="module")
def outs(setup):
    s = setup
    meta = dict(training_release="dr12q", training_set_name="dr9q_minus_concordance", dla_catalog_name="dr9q_concordance",
                prior_ind=np.ones(400, dtype=bool), release="dr12q", test_set_name="dr12q")
    seen = {}

    def spy(*a, **kw):
        seen.setdefault("calls", []).append(sorted(kw))
        return SO.compute(*a, **kw)
    run = lambda **kw: PR.process_qsos(s["model"], s["samples"], s["packed"], s["prior"], params=s["params"],  # noqa: E731
                                       metadata=meta, compute=spy, **kw)
    plain = run()
    both = run(sub_dla=s["sub"], forest=True)
    two = run(sub_dla=s["sub"], forest=dict(num_forest_lines=3, mean_flux=False), max_dlas=2)
    for o in (plain, both, two):
        o["test_ind"] = np.ones(Q, dtype=bool)
    return dict(plain=plain, both=both, two=two, seen=seen, meta=meta)


def test_process_qsos_without_the_keywords_is_unchanged(setup, outs):
    s = setup
    assert outs["seen"]["calls"][0] == []                    # a compute replacement sees no new keyword
    assert outs["seen"]["calls"][1] == ["forest", "sub_dla"] and outs["seen"]["calls"][2] == ["forest", "max_dlas", "sub_dla"]
    old = PR.process_qsos(s["model"], s["samples"], s["packed"], s["prior"], params=s["params"], metadata=outs["meta"],
                          compute=MO.compute)                # the multi-DLA oracle knows neither keyword
    plain = dict(outs["plain"])
    plain.pop("test_ind")
    assert sorted(plain) == sorted(old)
    assert sorted(k for k in plain if k not in outs["meta"]) == sorted(
        ["min_z_dlas", "max_z_dlas", "log_likelihoods_no_dla", "log_likelihoods_dla", "num_pixels", "num_lines",
         "max_z_cut", "prior_z_qso_increase", "sample_log_likelihoods_dla", "log_priors_no_dla", "log_priors_dla",
         "log_posteriors_no_dla", "log_posteriors_dla", "model_posteriors", "p_no_dlas", "p_dlas"])
    for key in old:
        a, b = np.asarray(plain[key]), np.asarray(old[key])
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), key
    assert not set(plain) & (set(PR.SUB_DLA_VARIABLES) | set(PR.FOREST_VARIABLES))


def test_process_qsos_end_to_end_with_sub_dla_and_forest(setup, outs):
    s, o = setup, outs["both"]
    assert o["model_posteriors"].shape == (Q, 3) and o["sample_log_likelihoods_lls"].shape == (Q, S)
    np.testing.assert_allclose(o["model_posteriors"].sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert np.array_equal(o["p_lls"], o["model_posteriors"][:, -1])
    assert np.array_equal(o["p_dlas"], 1 - o["p_no_dlas"] - o["p_lls"])             # the p_dlas identity
    assert np.array_equal(o["log_posteriors_lls"], o["log_priors_lls"] + o["log_likelihoods_lls"])
    assert np.array_equal(o["lls_log_nhi_samples"], s["sub"]["lls_log_nhi_samples"]) and o["sub_dla_prior_ratio"] == RATIO
    assert (o["num_forest_lines"], o["forest_variance_series"], o["forest_mean_flux"]) == (31, True, True)
    assert (o["mean_flux_tau_0"], o["mean_flux_beta"]) == (0.0023, 3.65)
    # against the oracle, spectrum by spectrum; the forest moves every likelihood
    for q, spec in enumerate(s["spectra"]):
        ref = SO.process_spectrum(spec, s["model"], s["samples"], 1, s["sub"]["lls_nhi_samples"], {})
        assert np.array_equal(o["sample_log_likelihoods_lls"][q], ref["sample_log_likelihoods_lls"])
        assert o["log_likelihoods_lls"][q] == ref["log_likelihood_lls"] == SO.evidence(ref["sample_log_likelihoods_lls"])
        assert o["log_likelihoods_no_dla"][q] == ref["log_likelihood_no_dla"]
        assert o["log_likelihoods_no_dla"][q] != outs["plain"]["log_likelihoods_no_dla"][q]
        # a sub-DLA absorbs less than a DLA at the same redshift: the two rows differ
        assert not np.array_equal(o["sample_log_likelihoods_lls"][q], o["sample_log_likelihoods_dla"][q])
    p = np.exp(PR.dla_priors(s["packed"]["z_qsos"], s["prior"]["z_qsos"], s["prior"]["dla_ind"])[1])
    np.testing.assert_allclose(np.exp(o["log_priors_no_dla"]), 1 - p - RATIO * p, rtol=1e-15)
    assert np.array_equal(o["log_priors_dla"], outs["plain"]["log_priors_dla"])
    two = outs["two"]
    assert two["model_posteriors"].shape == (Q, 4) and two["log_likelihoods_dla"].shape == (Q, 2)
    np.testing.assert_allclose(two["model_posteriors"].sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert two["num_forest_lines"] == 3 and two["forest_mean_flux"] is False
    assert np.array_equal(two["log_priors_no_dla"], o["log_priors_no_dla"])
    # the oracle's evidence: NaN as soon as one sample is NaN
    assert np.isnan(SO.evidence([1.0, np.nan])) and SO.evidence([2.0, 2.0]) == 2.0


def test_mat_round_trip_of_every_new_variable(tmp_path, setup, outs):
    o = dict(outs["both"])
    o["MAP_z_lls"], o["MAP_log_nhi_lls"] = np.array([2.5, 2.75]), np.array([19.75, 19.875])     # (a summaries run's)
    path = tmp_path / "processed_qsos_dr12q.mat"
    PR.save_processed_qsos(str(path), o)
    r = M.loadmat(str(path))
    for key in PR.SUB_DLA_VARIABLES + PR.FOREST_VARIABLES:
        assert key in r, key
        want = np.asarray(o[key], dtype=np.float64)
        got = np.asarray(r[key], dtype=np.float64)
        assert got.size == want.size and np.array_equal(got.reshape(want.shape), want, equal_nan=True), key
    assert r["sample_log_likelihoods_lls"].shape == (Q, S) and r["model_posteriors"].shape == (Q, 3)
    assert np.array_equal(r["model_posteriors"], o["model_posteriors"])
    assert set(r) - set(PR.PROCESSED_VARIABLES) == set(PR.SUB_DLA_VARIABLES) | set(PR.FOREST_VARIABLES)
    plain = tmp_path / "plain.mat"
    PR.save_processed_qsos(str(plain), outs["plain"])
    assert not set(M.loadmat(str(plain))) - set(PR.PROCESSED_VARIABLES)
    # the samples file carries the two new entries when present, and only then
    samp = tmp_path / "dla_samples.mat"
    PR.save_dla_samples(str(samp), dict(setup["samples"], lls_log_nhi_samples=setup["sub"]["lls_log_nhi_samples"],
                                        sub_dla_prior_ratio=RATIO))
    back = PR.load_dla_samples(str(samp))
    assert np.array_equal(back["lls_log_nhi_samples"], setup["sub"]["lls_log_nhi_samples"]) and back["sub_dla_prior_ratio"] == RATIO
    assert PR._sub_dla_spec(True, back)["ratio"] == RATIO
    assert np.array_equal(PR._sub_dla_spec(True, back)["nhi"], 10.0 ** setup["sub"]["lls_log_nhi_samples"])
    PR.save_dla_samples(str(samp), setup["samples"])
    assert sorted(PR.load_dla_samples(str(samp))) == ["log_nhi_samples", "nhi_samples", "offset_samples"]


def test_argument_errors(tmp_path, setup):
    s = setup
    run = lambda **kw: PR.process_qsos(s["model"], s["samples"], s["packed"], params=s["params"], compute=SO.compute, **kw)  # noqa: E731
    bad = dict(s["sub"], lls_log_nhi_samples=s["sub"]["lls_log_nhi_samples"][:-1])
    bad.pop("lls_nhi_samples")
    for sub in (bad, dict(lls_nhi_samples=np.zeros(S), sub_dla_prior_ratio=1.0),
                dict(lls_nhi_samples=np.full(S, np.inf), sub_dla_prior_ratio=1.0),
                dict(lls_log_nhi_samples=np.full(S, 19.7)),                      # no ratio and no fit to derive it from
                dict(lls_log_nhi_samples=np.full(S, 19.7), sub_dla_prior_ratio=-1.0),
                dict(lls_log_nhi_samples=np.full(S, 19.7), sub_dla_prior_ratio=np.nan),
                dict(nhi=np.ones(S)), "yes"):
        with pytest.raises(ValueError):
            run(sub_dla=sub)
    for forest in (dict(num_forest_lines=0), dict(num_forest_lines=32), dict(mean_flux_tau_0=-1e-3),
                   dict(mean_flux_tau_0=np.inf), dict(mean_flux_beta=np.nan), dict(lines=3), 31):
        with pytest.raises(ValueError):
            run(forest=forest)
    # a ratio derived from the samples' own fit
    with_fit = dict(s["samples"], fit=dict(coeffs=FIT))
    assert PR._sub_dla_spec(dict(lls_log_nhi_samples=np.full(S, 19.7)), with_fit)["ratio"] == DS.sub_dla_prior_ratio(FIT)
    with pytest.raises(NotImplementedError):
        PR.run_process_qsos(str(tmp_path), "dr12q", "a", "b", None, "dr12q", "dr12q", None, world=2, sub_dla=True)


def test_run_process_qsos_writes_the_new_variables(tmp_path):
    """The file-level driver with both keywords, and ``sub_dla=True`` reading the two entries the samples file carries."""
    from test_matv73 import write_reference_tree
    from test_process_sharded import ARGS
    S_, Q_ = 24, 2
    write_reference_tree(tmp_path, Q=Q_, S=S_, k=4)
    d = tmp_path / "dr12q" / "processed"
    sub = dict(DS.sub_dla_samples(S_, u=syn.halton(S_, 3)), sub_dla_prior_ratio=0.5)
    forest = dict(num_forest_lines=3)
    out = PR.run_process_qsos(str(tmp_path), *ARGS, compute=SO.compute, sub_dla=sub, forest=forest)
    r = M.loadmat(str(d / "processed_qsos_dr12q.mat"))
    assert r["model_posteriors"].shape == (Q_, 3) and r["sample_log_likelihoods_lls"].shape == (Q_, S_)
    for key in set(PR.SUB_DLA_VARIABLES) - {"MAP_z_lls", "MAP_log_nhi_lls"} | set(PR.FOREST_VARIABLES):
        assert key in r, key
    assert np.array_equal(r["p_dlas"].ravel(), 1 - r["p_no_dlas"].ravel() - r["p_lls"].ravel())
    assert r["num_forest_lines"].ravel()[0] == 3 and r["forest_mean_flux"].ravel()[0] == 1
    np.testing.assert_allclose(r["model_posteriors"].sum(axis=1), 1.0, rtol=0, atol=1e-14)
    samples = PR.load_dla_samples(str(d / "dla_samples.mat"))
    PR.save_dla_samples(str(d / "dla_samples.mat"), dict(samples, lls_log_nhi_samples=sub["lls_log_nhi_samples"],
                                                         sub_dla_prior_ratio=0.5))
    again = PR.run_process_qsos(str(tmp_path), *ARGS, compute=SO.compute, sub_dla=True, forest=forest, save=False)
    for key in ("model_posteriors", "log_likelihoods_lls", "sample_log_likelihoods_lls", "log_priors_lls", "p_dlas"):
        assert np.array_equal(again[key], out[key]), key
    plain = PR.run_process_qsos(str(tmp_path), *ARGS, compute=SO.compute, save=False)
    assert not set(plain) & (set(PR.SUB_DLA_VARIABLES) | set(PR.FOREST_VARIABLES)) and plain["model_posteriors"].shape == (Q_, 2)


def test_new_entry_points_need_a_device():
    lib = L.load()
    out, lam = np.zeros(4), np.linspace(3600.0, 3700.0, 4)
    # argument errors come first, device or not
    for nl in (0, 32):
        assert lib.gpdla_forest_f64(0, L.ptr(lam), 4, 2.5, 0.0023, 3.65, nl, L.ptr(out)) == L.GPDLA_EINVAL
    assert lib.gpdla_forest_f64(0, L.ptr(lam), 4, 2.5, -1.0, 3.65, 3, L.ptr(out)) == L.GPDLA_EINVAL
    assert lib.gpdla_forest_f64(0, L.ptr(lam), 4, 2.5, 0.0023, float("nan"), 3, L.ptr(out)) == L.GPDLA_EINVAL
    assert lib.gpdla_forest_f64(0, None, 4, 2.5, 0.0023, 3.65, 3, L.ptr(out)) == L.GPDLA_EINVAL
    assert lib.gpdla_engine_set_forest(None, None) == L.GPDLA_EINVAL
    if lib.gpdla_device_count() > 0:
        pytest.skip("a HIP device is present")
    assert lib.gpdla_forest_f64(0, L.ptr(lam), 4, 2.5, 0.0023, 3.65, 3, L.ptr(out)) == L.GPDLA_EDEVICE


@needs_h5py
@pytest.mark.skipif(not os.path.isdir(REF_CDDF), reason="reference not present (GPU box)")
def test_reference_consumer_reads_sub_dla_file(tmp_path, setup, outs):
    """calc_cddf.py's DLACatalogue on a file with the sub-DLA column: p_dlas is 1 - p_no_dlas - p_lls and the
    level-1 sample rows load as from the plain file's layout."""
    o = outs["both"]
    proc, samp, snrs = tmp_path / "processed_qsos_dr12q.mat", tmp_path / "dla_samples.mat", tmp_path / "snrs_qsos_dr12q.mat"
    PR.save_processed_qsos(str(proc), o)
    PR.save_dla_samples(str(samp), dict(setup["samples"], lls_log_nhi_samples=o["lls_log_nhi_samples"], sub_dla_prior_ratio=RATIO))
    M.savemat73(str(snrs), dict(snrs=np.full(Q, 5.0)))
    res = subprocess.run([H5PY_PY, "-B", str(Path(__file__).parent / "cddf_consumer.py"), REF_CDDF, str(proc), str(samp),
                          str(snrs)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert np.array_equal(got["p_dla"], o["p_dlas"])
    assert np.array_equal(got["lnhi"], setup["samples"]["log_nhi_samples"])
    rows = {**got["log_norm_like"], **got["log_norm_like_on_demand"]}
    assert rows, "no spectrum passed the reference's p_dla threshold"
    for spec, vals in rows.items():
        want = o["sample_log_likelihoods_dla"][int(spec)] - (o["log_likelihoods_dla"][int(spec)] + np.log(S))
        np.testing.assert_allclose(vals, want, rtol=0, atol=1e-12)

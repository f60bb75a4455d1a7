"""The forest's mean_flux_scope, CPU part: the numpy restatement
(mean_flux_scope_oracle.py) pinned by a dense Gaussian log-density and by the change of variables that ties
scope "all" to the model training learns on y / F; the argument checks; the saved variables."""
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy.stats import multivariate_normal

sys.path.insert(0, str(Path(__file__).parent))
import mean_flux_scope_oracle as FS  # noqa: E402
import sub_dla_forest_oracle as SO  # noqa: E402
from gp_dla_detection_amd import matv73 as M  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd import training as T  # noqa: E402
from gp_dla_detection_amd.engine import MEAN_FLUX_SCOPES, Engine  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402
from oracle import gpdla_oracle as O  # noqa: E402

K, N_TARGET, S = 4, 300, 40
FOREST = dict(SO.FOREST_DEFAULTS)


def _forest(scope, **kw):
    return dict(FOREST, mean_flux_scope=scope, **kw)


@pytest.fixture(scope="module")
def model():
    return syn.make_model(k=K)


def _prep(spec, model, mode="reference"):
    return O.prepare_spectrum(spec["wavelengths"], spec["flux"], spec["noise_variance"], spec["pixel_mask"], spec["z_qso"],
                              model, mode)


def test_scope_names_and_codes():
    assert MEAN_FLUX_SCOPES == FS.SCOPES == {"mu": 0, "mu_M": 1, "all": 2}
    assert PR.FOREST_DEFAULTS["mean_flux_scope"] == "mu" and PR.MEAN_FLUX_SCOPE_VARIABLES == ("mean_flux_scope",)
    assert "mean_flux_scope" not in PR.FOREST_VARIABLES


# ---------------------------------------------------------------------------------- dense Gaussian
@pytest.mark.parametrize("scope", ["all", "mu_M"])
@pytest.mark.parametrize("z_qso", [2.6, 3.1, 4.5])
def test_oracle_null_likelihood_is_the_dense_gaussian(model, scope, z_qso):
    spec = syn.make_spectrum(model, 0, z_qso=z_qso, n_target=N_TARGET, mask_fraction=0.05)
    plain = _prep(spec, model)
    series = SO.apply_forest(plain, spec, model, dict(FOREST, mean_flux=False))       # omega^2 sf^2, mu untouched
    F = FS.mean_flux(spec, FOREST)
    assert F.shape == plain["y"].shape and np.all((F > 0) & (F <= 1)) and np.count_nonzero(F < 1) > 0.9 * F.size
    Ms = plain["M"] * F[:, None]
    diag = (F ** 2 * series["omega2"] if scope == "all" else series["omega2"]) + plain["noise"]
    ref = multivariate_normal(F * plain["mu"], Ms @ Ms.T + np.diag(diag)).logpdf(plain["y"])
    got = O.null_log_likelihood(FS.apply_forest(plain, spec, model, _forest(scope)))
    assert got == pytest.approx(ref, rel=1e-12)
    # the scope matters: today's evaluation (mu alone) is another number, and so is the other scope
    assert abs(got - O.null_log_likelihood(FS.apply_forest(plain, spec, model, _forest("mu")))) > 1e-6 * abs(got)
    other = "mu_M" if scope == "all" else "all"
    assert abs(got - O.null_log_likelihood(FS.apply_forest(plain, spec, model, _forest(other)))) > 1e-6 * abs(got)
    # "mu" is sub_dla_forest_oracle's own result, key for key
    a, b = FS.apply_forest(plain, spec, model, _forest("mu")), SO.apply_forest(plain, spec, model, FOREST)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[key], b[key]) for key in a)


# ------------------------------------------------------------------------------ change of variables
@pytest.mark.parametrize("mode", ["reference", "unmasked"])
@pytest.mark.parametrize("z_qso", [2.6, 3.1, 4.5])
def test_scope_all_is_the_unabsorbed_model_on_the_divided_spectrum(model, mode, z_qso):
    """N(y; F mu, diag(F) K diag(F)) = N(y / F; mu, K) / prod F, for the null and for every DLA sample (the
    absorption multiplies mu, M and omega^2 alike on both sides)."""
    samples = syn.make_samples(S)
    spec = syn.make_spectrum(model, 1, z_qso=z_qso, n_target=N_TARGET, mask_fraction=0.05)
    F_all = FS.mean_flux(spec, FOREST, wavelengths=spec["wavelengths"])
    divided = dict(spec, flux=spec["flux"] / F_all, noise_variance=spec["noise_variance"] / F_all ** 2)
    shift = np.sum(np.log(FS.mean_flux(spec, FOREST)))                  # over the unmasked in-range pixels
    a = FS.SpectrumOracle(spec, model, samples, 3, mode, _forest("all"))
    b = FS.SpectrumOracle(divided, model, samples, 3, mode, _forest("mu", mean_flux=False))
    got = np.concatenate([[O.null_log_likelihood(a.prep)], a.level1()])
    want = np.concatenate([[O.null_log_likelihood(b.prep)], b.level1()]) - shift
    assert got.shape == (1 + S,) and np.all(np.isfinite(want))
    err = np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))
    print(f"z_QSO={z_qso} {mode}: min F {F_all.min():.3f}, shift {shift:.6g}, max rel err {err:.3g}")
    assert err <= 1e-12
    # without the omega^2 factor the identity fails: "mu_M" is a different model
    c = FS.SpectrumOracle(spec, model, samples, 3, mode, _forest("mu_M"), base=a)
    assert abs(O.null_log_likelihood(c.prep) - want[0]) > 1e-6 * abs(want[0])
    assert np.array_equal(c.A, a.A) and c.plain is a.plain


# --------------------------------------------------------------------------------------- validation
BAD = [dict(mean_flux_scope="M"), dict(mean_flux_scope=2), dict(mean_flux_scope=None),
       dict(mean_flux_scope="mu_M", mean_flux=False), dict(mean_flux_scope="all", mean_flux=False)]


@pytest.mark.parametrize("bad", BAD)
def test_bad_scopes_are_rejected_before_anything_runs(bad, model, tmp_path):
    def never(*a, **kw):
        raise AssertionError("compute was reached")
    packed = syn.pack_spectra([syn.make_spectrum(model, 0, n_target=N_TARGET)])
    with pytest.raises(ValueError, match="mean_flux"):
        PR.process_qsos(model, syn.make_samples(S), packed, params=set_parameters(k=K), compute=never, forest=bad)
    with pytest.raises(ValueError, match="mean_flux"):
        PR.run_process_qsos(str(tmp_path / "nowhere"), "dr0", "a", "b", None, "dr0", "t", None, forest=bad)
    with pytest.raises(ValueError, match="mean_flux"):
        T.learn_qso_model([], [], forest=bad)
    with pytest.raises(ValueError, match="mean_flux"):
        T.run_learn_qso_model(str(tmp_path / "nowhere"), "dr0", "t", None, forest=bad)
    eng = Engine.__new__(Engine)                 # no library, no handle: the check comes before either is used
    with pytest.raises(ValueError, match="mean_flux"):
        eng.set_forest(bad)
    with pytest.raises(ValueError, match="mean_flux"):
        eng.set_forest(True, **bad)


def test_good_scopes_pass_the_spec():
    for scope in MEAN_FLUX_SCOPES:
        assert PR._forest_spec(dict(mean_flux_scope=scope))["mean_flux_scope"] == scope
    assert PR._forest_spec(True)["mean_flux_scope"] == "mu"
    assert PR._forest_spec(dict(mean_flux=False))["mean_flux_scope"] == "mu"
    assert PR._scope_variables(PR._forest_spec(True)) == {}
    assert PR._scope_variables(PR._forest_spec(dict(mean_flux_scope="mu_M"))) == dict(mean_flux_scope=1.0)
    assert PR._scope_variables(PR._forest_spec(dict(mean_flux_scope="all"))) == dict(mean_flux_scope=2.0)


# ----------------------------------------------------------------------------------- saved variables
def test_saved_variables_carry_the_scope_only_when_it_is_set(model, tmp_path):
    samples = syn.make_samples(S)
    spectra = [syn.make_spectrum(model, q, z_qso=z, n_target=N_TARGET, mask_fraction=0.05) for q, z in enumerate((2.6, 3.1))]
    packed = syn.pack_spectra(spectra)
    rng = np.random.default_rng(5)
    prior = dict(z_qsos=rng.uniform(2.0, 4.5, 400), dla_ind=rng.uniform(size=400) < 0.12)
    run = lambda compute, forest: PR.process_qsos(model, samples, packed, prior=prior, params=set_parameters(k=K),  # noqa: E731
                                                  compute=compute, forest=forest)
    today = run(SO.compute, True)                                     # a run without the key
    mu = run(FS.compute, dict(mean_flux_scope="mu"))
    assert sorted(mu) == sorted(today) and "mean_flux_scope" not in mu
    for key in today:
        assert np.array_equal(np.asarray(mu[key]), np.asarray(today[key]), equal_nan=True), key
    outs = {}
    for scope, code in (("mu_M", 1.0), ("all", 2.0)):
        out = outs[scope] = run(FS.compute, dict(mean_flux_scope=scope))
        assert sorted(out) == sorted(list(today) + ["mean_flux_scope"]) and out["mean_flux_scope"] == code
        assert isinstance(out["mean_flux_scope"], float)
        assert np.all(out["log_likelihoods_no_dla"] != today["log_likelihoods_no_dla"])
        for q, spec in enumerate(spectra):
            ref = FS.process_spectrum(spec, model, samples, forest=dict(mean_flux_scope=scope))
            assert out["log_likelihoods_no_dla"][q] == ref["log_likelihood_no_dla"]
            assert np.array_equal(out["sample_log_likelihoods_dla"][q], ref["sample_log_likelihoods_dla"][0])
        path = tmp_path / f"processed_{scope}.mat"
        PR.save_processed_qsos(str(path), out)
        r = M.loadmat(str(path))
        assert np.asarray(r["mean_flux_scope"]).dtype == np.float64 and np.asarray(r["mean_flux_scope"]).ravel()[0] == code
        for key in PR.FOREST_VARIABLES:
            assert key in r, key
    assert np.all(outs["all"]["log_likelihoods_no_dla"] != outs["mu_M"]["log_likelihoods_no_dla"])
    path = tmp_path / "processed_mu.mat"
    PR.save_processed_qsos(str(path), mu)
    r, path2 = M.loadmat(str(path)), tmp_path / "processed_today.mat"
    PR.save_processed_qsos(str(path2), today)
    assert "mean_flux_scope" not in r and sorted(r) == sorted(M.loadmat(str(path2)))

"""The forest's mean_flux_scope on the GPU: every model's likelihoods under "all" and
"mu_M" against the numpy oracle (mean_flux_scope_oracle.py), the change of variables that ties "all" to the
unabsorbed model with the engine on both sides, what must stay bitwise equal, the unusable spectrum, the
argument errors, process_qsos down to the file and the key passing through training.  Shapes as in
test_gpu_sub_dla_forest.py."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import mean_flux_scope_oracle as FS  # noqa: E402
from conftest import tol_ok  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import dla_samples as DS  # noqa: E402
from gp_dla_detection_amd import matv73 as M  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import Engine  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402

pytestmark = pytest.mark.gpu

S_LEVEL = 333            # neither S nor S + 1 is a multiple of 64
FOREST = dict(num_forest_lines=31, variance_series=True, mean_flux=True, mean_flux_tau_0=0.0023, mean_flux_beta=3.65)


def _scoped(scope, **kw):
    return dict(FOREST, mean_flux_scope=scope, **kw)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _all_same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert _same(a[key], b[key]), key


def _sub_samples(S):
    return DS.sub_dla_samples(S, u=syn.halton(S, 3))


def _spectra(model):
    mk = dict(mask_fraction=0.05)
    s0 = syn.make_spectrum(model, 0, z_qso=2.6, n_target=300, **mk)
    scaled = dict(s0, flux=s0["flux"] * 1e-17, noise_variance=s0["noise_variance"] * 1e-34)   # unit scaling E != 0
    return [s0, syn.make_spectrum(model, 1, z_qso=3.1, n_target=None, **mk),   # more series lines active
            syn.make_spectrum(model, 2, n_target=270, **mk), scaled,
            syn.make_spectrum(model, 3, n_target=300, mask_fraction=1.0)]      # J = 0: NaN rows


_cache = {}


def _setup(k, mode):
    """Per (k, mode): the spectra and one oracle per spectrum whose sample profiles every scope shares."""
    key = (k, mode)
    if key not in _cache:
        model = syn.make_model(k=k)
        samples = syn.make_samples(S_LEVEL)
        spectra = _spectra(model)
        base = [FS.SpectrumOracle(s, model, samples, 3, mode, None) for s in spectra]
        forced = np.random.default_rng(77).integers(0, S_LEVEL, (1, len(spectra), S_LEVEL)).astype(np.int32)
        _cache[key] = dict(model=model, samples=samples, spectra=spectra, packed=syn.pack_spectra(spectra),
                           sub=_sub_samples(S_LEVEL), params=set_parameters(k=k, absorption_mode=mode), base=base,
                           forced=forced)
    return _cache[key]


def _reference(s, q, scope, mode):
    so = FS.SpectrumOracle(s["spectra"][q], s["model"], s["samples"], 3, mode, _scoped(scope), base=s["base"][q])
    return FS.process_spectrum(s["spectra"][q], s["model"], s["samples"], 2, s["sub"]["lls_nhi_samples"],
                               forced=s["forced"][:, q], absorption_mode=mode, oracle=so)


def _pairs(out, ref):
    """(got, want) per output, ``ref`` a list of per-spectrum oracle results for the rows of ``out``."""
    return dict(
        null=(out["log_likelihoods_no_dla"], np.array([r["log_likelihood_no_dla"] for r in ref])),
        sub_samples=(out["sample_log_likelihoods_lls"], np.stack([r["sample_log_likelihoods_lls"] for r in ref])),
        sub_evidence=(out["log_likelihoods_lls"], np.array([r["log_likelihood_lls"] for r in ref])),
        level_samples=(out["sample_log_likelihoods_dla"], np.stack([r["sample_log_likelihoods_dla"] for r in ref], axis=1)),
        level_evidence=(out["log_likelihoods_dla"], np.stack([r["log_likelihoods_dla"] for r in ref], axis=1)))


# --------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("scope,k,mode", [("all", 4, "reference"), ("all", 4, "unmasked"), ("all", 6, "reference"),
                                          ("all", 6, "unmasked"), ("all", 20, "reference"), ("all", 20, "unmasked"),
                                          ("mu_M", 4, "reference"), ("mu_M", 20, "unmasked")])
def test_models_under_the_scoped_forest_against_oracle(scope, k, mode):
    s = _setup(k, mode)
    Q = len(s["spectra"])
    ref = [_reference(s, q, scope, mode) for q in range(Q)]
    with Engine(s["model"], s["samples"], s["params"]) as eng:
        eng.set_forest(_scoped(scope))
        out = eng.process_models(s["packed"], 2, sub_dla=s["sub"]["lls_nhi_samples"], base_sample_inds=s["forced"],
                                 raise_numeric=True)
        assert eng.model_stats()["forest_launches"] == 2 and eng.model_stats()["sub_dla_launches"] == 1
    for name, (got, want) in _pairs(out, ref).items():
        assert got.shape == want.shape, name
        assert np.array_equal(np.isnan(got), np.isnan(want)), name            # identical NaN patterns
        fin = np.isfinite(want)
        assert fin.any(), name
        err = np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1.0))
        print(f"{scope} k={k} {mode} {name}: max rel err {err:.3g}")
        assert np.all(tol_ok(got[fin], want[fin], 1e-9)), name
    assert np.all(np.isnan(out["sample_log_likelihoods_lls"][Q - 1])) and np.isnan(out["log_likelihoods_lls"][Q - 1])
    assert np.all(np.isfinite(out["sample_log_likelihoods_lls"][:Q - 1])) and np.all(np.isfinite(out["log_likelihoods_lls"][:Q - 1]))
    # the scope is not a no-op: on the z = 3.1 spectrum every output misses today's model (mu alone) by far
    for name, (got, want) in _pairs(out, [_reference(s, 1, "mu", mode)]).items():
        got = got[:, 1:2] if name.startswith("level") else got[1:2]           # levels are D x Q (x S)
        fin = np.isfinite(want)
        assert got.shape == want.shape and fin.any(), name
        miss = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1.0)
        print(f"{scope} k={k} {mode} {name}: min rel distance from scope mu {miss.min():.3g}")
        assert not np.any(tol_ok(got[fin], want[fin], 1e-6)), name


# ---------------------------------------------------------------- 2. change of variables on the device
@pytest.mark.parametrize("k", [4, 20])
def test_scope_all_is_the_unabsorbed_model_on_the_divided_spectra(k):
    """N(y; F mu, diag(F) K diag(F)) = N(y / F; mu, K) / prod F with the engine on both sides: a Khatri-Rao
    row that disagrees with its scaled u-words, or an omega^2 left behind, breaks it."""
    s = _setup(k, "reference")
    divided, shift = [], []
    for spec in s["spectra"]:
        F = FS.mean_flux(spec, FOREST, wavelengths=spec["wavelengths"])
        divided.append(dict(spec, flux=spec["flux"] / F, noise_variance=spec["noise_variance"] / F ** 2))
        shift.append(np.sum(np.log(FS.mean_flux(spec, FOREST))))            # the unmasked in-range pixels
    shift = np.array(shift)
    with Engine(s["model"], s["samples"], s["params"]) as eng:
        eng.set_forest(_scoped("all"))
        got = eng.process(s["packed"])
        eng.set_forest(dict(FOREST, mean_flux=False))
        plain = eng.process(syn.pack_spectra(divided))
        eng.set_forest(FOREST)
        mu_only = eng.process(s["packed"])
    Q = len(s["spectra"])
    assert np.all(shift[:Q - 1] < -10) and shift[Q - 1] == 0
    for name, sh in (("log_likelihoods_no_dla", shift), ("sample_log_likelihoods_dla", shift[:, None])):
        a, b = got[name], plain[name] - sh
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.isnan(a[Q - 1])), name
        fin = np.isfinite(b)
        assert np.all(fin[:Q - 1]), name
        err = np.max(np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1.0))
        print(f"k={k} {name}: max rel err {err:.3g}")
        assert np.all(tol_ok(a[fin], b[fin], 1e-9)), name
        assert not np.any(tol_ok(mu_only[name][fin], b[fin], 1e-6)), name     # today's model does not satisfy it


# ------------------------------------------------------------------------------- 3. exactness (bitwise)
@pytest.fixture(scope="module")
def exact():
    k, D = 8, 2
    model = syn.make_model(k=k)
    samples = syn.make_samples(S_LEVEL)
    spectra = [syn.make_spectrum(model, 0, n_target=300, mask_fraction=0.05, dla_fraction=1.0),
               syn.make_spectrum(model, 1, z_qso=2.9, n_target=280, mask_fraction=0.05, dla_fraction=0.0),
               syn.make_spectrum(model, 2, n_target=310, mask_fraction=0.05, dla_fraction=0.0)]
    packed = syn.pack_spectra(spectra)
    params = set_parameters(k=k)
    nhi_sub = _sub_samples(S_LEVEL)["lls_nhi_samples"]
    kw = dict(log_nhi_samples=samples["log_nhi_samples"], z_edges=np.linspace(1.9, 3.1, 7), log_nhi_edges=np.linspace(20.0, 23.0, 9))
    r = {}
    with Engine(model, samples, params) as eng:
        run = lambda **more: eng.process_models(packed, D, sub_dla=nhi_sub, raise_numeric=True, **kw, **more)  # noqa: E731
        r["off"] = run()
        r["off_single"] = eng.process(packed)
        eng.set_forest(FOREST)
        r["today"] = run()
        r["today_single"] = eng.process(packed)
        eng.set_forest(_scoped("mu"))
        r["mu"] = run()
        r["mu_single"] = eng.process(packed)
        eng.set_forest(_scoped("mu", mean_flux_tau_0=0.0))
        r["mu_tau_zero"] = run()
        eng.set_forest(_scoped("all", mean_flux_tau_0=0.0))
        r["all_tau_zero"] = run()
        eng.set_forest(_scoped("all"))
        r["all"] = run()
        r["all_again"] = run()
        r["all_dev"] = run(memory="device")
        r["all_single"] = eng.process(packed)
        eng.set_forest(FOREST)                               # the unscoped call resets the scope
        r["after_plain_set"] = run()
        eng.set_forest(_scoped("mu_M"))
        r["mu_M"] = run()
        eng.set_forest(None)
        r["after_none"] = run()
        r["after_none_single"] = eng.process(packed)
    for qb in (1, 2):
        with Engine(model, samples, params, max_batch_spectra=qb) as eng:
            eng.set_forest(_scoped("all"))
            r[f"all_qb{qb}"] = eng.process_models(packed, D, sub_dla=nhi_sub, raise_numeric=True, **kw)
            r[f"all_single_qb{qb}"] = eng.process(packed)         # the host pipeline: copies beside the kernels
            r[f"launches_qb{qb}"] = eng.model_stats()["forest_launches"]
    return r


def test_scope_mu_is_todays_call(exact):
    _all_same(exact["mu"], exact["today"])
    _all_same(exact["mu_single"], exact["today_single"])


def test_zero_mean_flux_makes_every_scope_the_same(exact):
    _all_same(exact["all_tau_zero"], exact["mu_tau_zero"])           # F = exp(-0) = 1: every product is exact


def test_unscoped_set_forest_and_none_reset_the_scope(exact):
    _all_same(exact["after_plain_set"], exact["mu"])
    _all_same(exact["after_none"], exact["off"])
    _all_same(exact["after_none_single"], exact["off_single"])


def test_repeats_memory_spaces_and_batches_agree(exact):
    _all_same(exact["all"], exact["all_again"])
    _all_same(exact["all"], exact["all_dev"])
    for qb in (1, 2):
        _all_same(exact["all"], exact[f"all_qb{qb}"])
        _all_same(exact["all_single"], exact[f"all_single_qb{qb}"])
    # two forest launches per device batch of either call: 3 + 3 batches of one spectrum, 2 + 2 of up to two
    assert exact["launches_qb1"] == 12 and exact["launches_qb2"] == 8
    assert _same(exact["all"]["log_likelihoods_no_dla"], exact["all_single"]["log_likelihoods_no_dla"])
    assert _same(exact["all"]["sample_log_likelihoods_dla"][0], exact["all_single"]["sample_log_likelihoods_dla"])


def test_the_scopes_are_three_models(exact):
    for key in ("log_likelihoods_no_dla", "log_likelihoods_dla", "log_likelihoods_lls"):
        for a, b in (("all", "mu"), ("mu_M", "mu"), ("all", "mu_M")):
            assert np.all(exact[a][key] != exact[b][key]), (key, a, b)


# ------------------------------------------------------------------------------ 4. unusable spectrum
def test_unusable_spectrum_gives_nan_and_no_map_and_the_launch_counts():
    s = _setup(4, "reference")
    Q = len(s["spectra"])
    with Engine(s["model"], s["samples"], s["params"]) as eng:
        eng.set_forest(_scoped("all"))
        out = eng.process_models(s["packed"], 1, sub_dla=s["sub"]["lls_nhi_samples"], log_nhi_samples=s["samples"]["log_nhi_samples"])
        assert eng.model_stats()["forest_launches"] == 2          # one batch: forest_kernel and the covariance kernel
        eng.set_forest(_scoped("mu"))
        eng.process(s["packed"])
        assert eng.model_stats()["forest_launches"] == 3          # one more batch under "mu": forest_kernel alone
    assert np.all(np.isnan(out["sample_log_likelihoods_lls"][Q - 1])) and np.isnan(out["log_likelihoods_lls"][Q - 1])
    assert np.all(np.isnan(out["sample_log_likelihoods_dla"][0, Q - 1])) and np.isnan(out["log_likelihoods_no_dla"][Q - 1])
    assert out["map_sample_ind_lls"][Q - 1] == -1 and np.isnan(out["map_log_likelihood_lls"][Q - 1])
    assert out["map_sample_inds"][0, Q - 1] == -1 and np.isnan(out["MAP_z_dlas"][0, Q - 1, 0])
    assert np.isnan(out["MAP_z_lls"][Q - 1]) and np.isnan(out["MAP_log_nhi_lls"][Q - 1])
    assert np.all(out["map_sample_ind_lls"][:Q - 1] >= 0) and np.all(np.isfinite(out["MAP_z_lls"][:Q - 1]))
    assert np.all(out["map_sample_inds"][0, :Q - 1] >= 0) and np.all(np.isfinite(out["log_likelihoods_no_dla"][:Q - 1]))


# ----------------------------------------------------------------------------------------- 5. errors
def test_argument_errors_leave_the_setting_alone():
    model = syn.make_model(k=8)
    samples = syn.make_samples(64)
    packed = syn.pack_spectra([syn.make_spectrum(model, 0, z_qso=3.1, n_target=220, mask_fraction=0.05)])
    params = set_parameters(k=8)
    fs = lambda **kw: L.Forest(**dict(dict(num_forest_lines=31, variance_series=1, mean_flux=1, mean_flux_tau_0=0.0023,  # noqa: E731
                                           mean_flux_beta=3.65), **kw))
    with Engine(model, samples, params) as eng:
        lib, h = eng.lib, eng._h
        eng.set_forest(_scoped("all"))
        before = eng.process(packed)
        assert lib.gpdla_engine_set_forest_scoped(h, C.byref(fs()), 3) == L.GPDLA_EINVAL
        assert b"mean_flux_scope" in lib.gpdla_last_error()
        assert lib.gpdla_engine_set_forest_scoped(h, C.byref(fs()), -1) == L.GPDLA_EINVAL
        assert lib.gpdla_engine_set_forest_scoped(h, C.byref(fs(mean_flux=0)), 1) == L.GPDLA_EINVAL
        assert b"mean_flux" in lib.gpdla_last_error()
        assert lib.gpdla_engine_set_forest_scoped(h, C.byref(fs(mean_flux=0)), 2) == L.GPDLA_EINVAL
        assert lib.gpdla_engine_set_forest_scoped(h, None, 1) == L.GPDLA_EINVAL
        assert lib.gpdla_engine_set_forest_scoped(h, C.byref(fs(num_forest_lines=32)), 2) == L.GPDLA_EINVAL
        assert lib.gpdla_engine_set_forest_scoped(None, C.byref(fs()), 2) == L.GPDLA_EINVAL
        with pytest.raises(ValueError):
            eng.set_forest(dict(mean_flux_scope="M"))
        _all_same(eng.process(packed), before)                     # the earlier setting still applies
        assert lib.gpdla_engine_set_forest_scoped(h, C.byref(fs()), 0) == L.GPDLA_OK
        mu = eng.process(packed)
        eng.set_forest(FOREST)
        _all_same(eng.process(packed), mu)
        assert mu["log_likelihoods_no_dla"][0] != before["log_likelihoods_no_dla"][0]
        assert lib.gpdla_engine_set_forest_scoped(h, None, 0) == L.GPDLA_OK
    for path in ("fused_i8", "panel_gemm"):
        with Engine(model, samples, params, path=path) as eng:
            before = eng.process(packed)
            for scope in ("mu", "mu_M", "all"):
                with pytest.raises(L.GpdlaError) as ei:
                    eng.set_forest(_scoped(scope))
                assert ei.value.code == L.GPDLA_EUNSUPPORTED and b"fused fp64" in eng.lib.gpdla_last_error()
            _all_same(eng.process(packed), before)


# ------------------------------------------------------------------------- 6. process_qsos to the file
def test_process_qsos_on_the_device_and_the_file(tmp_path):
    k, D = 8, 2
    model = syn.make_model(k=k)
    samples = syn.make_samples(S_LEVEL)
    spectra = [syn.make_spectrum(model, 0, n_target=300, mask_fraction=0.05, dla_fraction=1.0),
               syn.make_spectrum(model, 1, z_qso=2.9, n_target=280, mask_fraction=0.05, dla_fraction=0.0)]
    packed = syn.pack_spectra(spectra)
    params = set_parameters(k=k)
    rng = np.random.default_rng(5)
    prior = dict(z_qsos=rng.uniform(2.0, 4.5, 400), dla_ind=rng.uniform(size=400) < 0.12)
    sub = dict(_sub_samples(S_LEVEL), sub_dla_prior_ratio=0.4)
    kw = dict(prior=prior, params=params, max_dlas=D, summaries=True, sub_dla=sub, forest=dict(mean_flux_scope="all"))
    out = PR.process_qsos(model, samples, packed, **kw)
    Q = len(spectra)
    assert out["model_posteriors"].shape == (Q, 1 + D + 1) and out["mean_flux_scope"] == 2.0
    np.testing.assert_allclose(out["model_posteriors"].sum(axis=1), 1.0, rtol=0, atol=1e-14)
    # the oracle-backed CPU run on the device's own base indices
    forced = (np.asarray(out["base_sample_inds"]).reshape(Q, S_LEVEL, D - 1).transpose(2, 0, 1) - 1).astype(np.int32)
    cpu = PR.process_qsos(model, samples, packed, compute=functools.partial(FS.compute, forced=forced), **kw)
    path = tmp_path / "processed_qsos_dr12q.mat"
    PR.save_processed_qsos(str(path), out)
    r = M.loadmat(str(path))
    assert np.asarray(r["mean_flux_scope"]).ravel()[0] == 2.0
    for key in PR.SUB_DLA_VARIABLES + PR.FOREST_VARIABLES + PR.MEAN_FLUX_SCOPE_VARIABLES + (
            "log_likelihoods_no_dla", "log_likelihoods_dla", "sample_log_likelihoods_dla", "model_posteriors", "p_dlas",
            "log_posteriors_no_dla", "log_posteriors_dla"):
        assert key in r, key
        got, want = np.asarray(r[key], dtype=np.float64).ravel(), np.asarray(cpu[key], dtype=np.float64).ravel()
        assert got.size == want.size and np.array_equal(np.isnan(got), np.isnan(want)), key
        fin = np.isfinite(want)
        err = np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1.0))
        print(f"{key}: max rel err {err:.3g}")
        assert np.all(tol_ok(got[fin], want[fin], 1e-9)), key
    np.testing.assert_allclose(np.asarray(r["model_posteriors"]).sum(axis=1), 1.0, rtol=0, atol=1e-14)
    # the same call under the default scope writes no such variable, and another answer
    plain = PR.process_qsos(model, samples, packed, **dict(kw, forest=True))
    assert "mean_flux_scope" not in plain and sorted(plain) == sorted(set(out) - {"mean_flux_scope"})
    assert np.all(plain["log_likelihoods_no_dla"] != out["log_likelihoods_no_dla"])


# -------------------------------------------------------------------------- 7. training carries the key
def test_training_accepts_the_scope_and_records_it(tmp_path):
    """One dict serves both stages: training is the same under every scope (bit for bit), and the learned file
    records a scope other than "mu"."""
    from gp_dla_detection_amd import training as T
    model = syn.make_model(k=4)
    spectra = syn.make_dr12q_like_spectra(model, 12, seed=9)
    d = tmp_path / "dr12q" / "processed"
    d.mkdir(parents=True)
    M.savemat73(str(d / "catalog.mat"), dict(z_qsos=np.array([s["z_qso"] for s in spectra]),
                                             filter_flags=np.zeros(12, np.uint8)))
    M.savemat73(str(d / "preloaded_qsos.mat"),
                dict(all_wavelengths=[s["wavelengths"] for s in spectra], all_flux=[s["flux"] for s in spectra],
                     all_noise_variance=[s["noise_variance"] for s in spectra],
                     all_pixel_mask=[np.asarray(s["pixel_mask"], dtype=bool) for s in spectra]))
    run = lambda name, forest: T.run_learn_qso_model(str(tmp_path), "dr12q", name, "(catalog.filter_flags == 0)", k=4,  # noqa: E731
                                                     max_iter=2, max_fun_evals=6, forest=forest)
    outs = {name: run(name, forest) for name, forest in (("today", True), ("mu", dict(mean_flux_scope="mu")),
                                                         ("all", dict(mean_flux_scope="all")))}
    files = {name: M.loadmat73(str(d / f"learned_qso_model_{name}.mat")) for name in outs}
    assert sorted(outs["mu"]) == sorted(outs["today"]) and set(files["mu"]) == set(files["today"])
    assert "mean_flux_scope" not in outs["mu"] and "mean_flux_scope" not in files["mu"]
    assert outs["all"]["mean_flux_scope"] == 2.0 and set(files["all"]) == set(files["today"]) | {"mean_flux_scope"}
    got = np.asarray(files["all"]["mean_flux_scope"])
    assert got.dtype == np.float64 and got.size == 1 and float(got.ravel()[0]) == 2.0
    for name in ("mu", "all"):
        for key in ("mu", "M", "log_omega", "log_c_0", "log_tau_0", "log_beta", "log_likelihood"):
            assert _same(outs[name][key], outs["today"][key]), (name, key)
    for key in PR.FOREST_VARIABLES:
        assert float(np.asarray(files["all"][key]).ravel()[0]) == float(np.asarray(files["today"][key]).ravel()[0]), key

"""Sub-DLA model and Lyman-series forest on the GPU against the numpy oracle (sub_dla_forest_oracle.py):
the forest sum alone, every model's likelihoods under the forest, what must stay bitwise equal, the
unusable spectrum, the argument errors and process_qsos down to the file."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import sub_dla_forest_oracle as SO  # noqa: E402
from conftest import tol_ok  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import dla_samples as DS  # noqa: E402
from gp_dla_detection_amd import matv73 as M  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import Engine, forest_optical_depth  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402
from oracle import gpdla_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

S_LEVEL = 333            # neither S nor S + 1 is a multiple of 64
FOREST = dict(num_forest_lines=31, variance_series=True, mean_flux=True, mean_flux_tau_0=0.0023, mean_flux_beta=3.65)
# gpdla_forest_f64 against the oracle, relative.  Budget: every term is positive, so the sum's error is
# bounded by the terms'; one rounding of 1 + z_i grows beta-fold (beta <= 3.65) through the power, the
# device's and numpy's pow each contribute about an ulp, two products, then up to 31 sequential adds:
# ~40 ulp.  Measured on gfx950 over the cases below: FOREST_MEASURED; the bar is
# 10 x that.  Anything above 256 ulp would not be rounding.
FOREST_MEASURED = 4.59e-16        # 2.1 ulp (L = 3; 1.7 ulp at L = 1 and L = 31)
FOREST_BAR = 10 * FOREST_MEASURED


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _sub_samples(S):
    """The default construction (19.5 + 0.5 u) on the Halton base-3 points the synthetic DLA samples use."""
    return DS.sub_dla_samples(S, u=syn.halton(S, 3))


# ------------------------------------------------------------------------------------ 1. forest alone
@pytest.mark.parametrize("L_", [1, 3, 31])
def test_forest_f64_against_oracle(L_):
    worst = 0.0
    for z, tau, beta in ((2.2, 0.0023, 3.65), (3.1, 0.0023, 3.65), (4.6, 0.0105, 3.2)):
        rng = np.random.default_rng(int(100 * z) + L_)
        lam = np.sort(rng.uniform(905.0, 1220.0, 700)) * (1 + z)
        # both sides of every line's edge lambda_i (1 + z_Q), and the edge itself as it rounds
        edge = SO.LINE_WAVELENGTHS * (1 + z)
        near = np.concatenate([edge, np.nextafter(edge, 0), np.nextafter(edge, np.inf), edge * (1 - 1e-12), edge * (1 + 1e-12)])
        lam = np.concatenate([lam, near])
        want = SO.forest_tau(lam, z, tau, beta, L_)
        got = forest_optical_depth(lam, z, tau, beta, L_)
        assert np.array_equal(got == 0, want == 0)             # the same lines active at every pixel
        nz = want > 0
        assert nz.sum() > 600 and (~nz).sum() > 5
        err = np.max(np.abs(got[nz] - want[nz]) / want[nz])
        # every active line's edge has pixels on both sides: the count of active lines steps across it
        for i in range(L_):
            lo = SO.forest_tau(edge[i:i + 1] * (1 - 1e-12), z, tau, beta, L_)
            hi = SO.forest_tau(edge[i:i + 1] * (1 + 1e-12), z, tau, beta, L_)
            assert lo[0] > hi[0]
        worst = max(worst, err)
    print(f"L={L_}: max rel deviation {worst:.3g} = {worst / 2.0 ** -52:.1f} ulp (bar {FOREST_BAR / 2.0 ** -52:.0f} ulp)")
    assert worst <= 256 * 2.0 ** -52, "more than rounding"
    assert worst <= FOREST_BAR


# ------------------------------------------------------------- 2. every model under the forest
def _spectra(model):
    mk = dict(mask_fraction=0.05)
    s0 = syn.make_spectrum(model, 0, z_qso=2.6, n_target=300, **mk)
    scaled = dict(s0, flux=s0["flux"] * 1e-17, noise_variance=s0["noise_variance"] * 1e-34)   # unit scaling E != 0
    return [s0, syn.make_spectrum(model, 1, z_qso=3.1, n_target=None, **mk),   # more series lines active
            syn.make_spectrum(model, 2, n_target=270, **mk), scaled,
            syn.make_spectrum(model, 3, n_target=300, mask_fraction=1.0)]      # J = 0: NaN rows


_cache = {}


def _setup(k, mode):
    key = (k, mode)
    if key not in _cache:
        model = syn.make_model(k=k)
        samples = syn.make_samples(S_LEVEL)
        spectra = _spectra(model)
        sub = _sub_samples(S_LEVEL)
        oracles = [SO.SpectrumOracle(s, model, samples, 3, mode, FOREST) for s in spectra]
        forced = np.random.default_rng(77).integers(0, S_LEVEL, (2, len(spectra), S_LEVEL)).astype(np.int32)
        _cache[key] = dict(model=model, samples=samples, spectra=spectra, packed=syn.pack_spectra(spectra), sub=sub,
                           params=set_parameters(k=k, absorption_mode=mode), oracles=oracles, forced=forced)
    return _cache[key]


@pytest.mark.parametrize("k,mode", [(4, "reference"), (4, "unmasked"), (6, "reference"), (6, "unmasked"),
                                    (20, "reference"), (20, "unmasked")])
def test_models_under_the_forest_against_oracle(k, mode):
    s, D = _setup(k, mode), 3
    Q = len(s["spectra"])
    ref = [SO.process_spectrum(sp, s["model"], s["samples"], D, s["sub"]["lls_nhi_samples"], FOREST, forced=s["forced"][:, q],
                               absorption_mode=mode, oracle=s["oracles"][q]) for q, sp in enumerate(s["spectra"])]
    with Engine(s["model"], s["samples"], s["params"]) as eng:
        eng.set_forest(FOREST)
        out = eng.process_models(s["packed"], D, sub_dla=s["sub"]["lls_nhi_samples"], base_sample_inds=s["forced"],
                                 raise_numeric=True)
        assert eng.model_stats()["forest_launches"] == 1 and eng.model_stats()["sub_dla_launches"] == 1
    pairs = dict(
        null=(out["log_likelihoods_no_dla"], np.array([r["log_likelihood_no_dla"] for r in ref])),
        sub_samples=(out["sample_log_likelihoods_lls"], np.stack([r["sample_log_likelihoods_lls"] for r in ref])),
        sub_evidence=(out["log_likelihoods_lls"], np.array([r["log_likelihood_lls"] for r in ref])),
        level_samples=(out["sample_log_likelihoods_dla"], np.stack([r["sample_log_likelihoods_dla"] for r in ref], axis=1)),
        level_evidence=(out["log_likelihoods_dla"], np.stack([r["log_likelihoods_dla"] for r in ref], axis=1)))
    for name, (got, want) in pairs.items():
        assert got.shape == want.shape, name
        assert np.array_equal(np.isnan(got), np.isnan(want)), name            # identical NaN patterns
        fin = np.isfinite(want)
        assert fin.any(), name
        err = np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1.0))
        print(f"k={k} {mode} {name}: max rel err {err:.3g}")
        assert np.all(tol_ok(got[fin], want[fin], 1e-9)), name
    # the unusable spectrum: NaN throughout; the usable ones: finite null, sub-DLA rows and evidences
    assert np.all(np.isnan(out["sample_log_likelihoods_lls"][Q - 1])) and np.isnan(out["log_likelihoods_lls"][Q - 1])
    assert np.all(np.isfinite(out["sample_log_likelihoods_lls"][:Q - 1])) and np.all(np.isfinite(out["log_likelihoods_lls"][:Q - 1]))
    # the forest is not a no-op here: the oracle without it is far outside the bar
    plain = SO.process_spectrum(s["spectra"][1], s["model"], s["samples"], 1, absorption_mode=mode)
    assert not tol_ok(out["log_likelihoods_no_dla"][1], plain["log_likelihood_no_dla"], 1e-6)
    if mode == "reference":
        # with in-range masked pixels slot pos carries the pos-th in-range wavelength for the profile but the
        # pos-th unmasked pixel's flux and model: the forest evaluated at the former is outside the bar
        spec = s["spectra"][1]
        prep = O.prepare_spectrum(spec["wavelengths"], spec["flux"], spec["noise_variance"], spec["pixel_mask"],
                                  spec["z_qso"], s["model"], mode)
        assert prep["m"] > prep["n"]
        wrong = SO.apply_forest(prep, spec, s["model"], FOREST, wavelengths=prep["padded"][3:3 + prep["n"]])
        assert not tol_ok(out["log_likelihoods_no_dla"][1], O.null_log_likelihood(wrong), 1e-9)


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
    sub = _sub_samples(S_LEVEL)
    nhi_sub = sub["lls_nhi_samples"]
    grid = dict(z_edges=np.linspace(1.9, 3.1, 7), log_nhi_edges=np.linspace(20.0, 23.0, 9))
    kw = dict(log_nhi_samples=samples["log_nhi_samples"], **grid)
    r = {}
    with Engine(model, samples, params) as eng:
        r["single"] = eng.process(packed)
        r["multi"] = eng.process_multi(packed, D, raise_numeric=True)
        r["summ"] = eng.process_summaries(packed, D, samples["log_nhi_samples"], want_samples=True, raise_numeric=True, **grid)
        r["models_none_multi"] = eng.process_models(packed, D, raise_numeric=True)
        r["models_none_summ"] = eng.process_models(packed, D, raise_numeric=True, **kw)
        r["sub"] = eng.process_models(packed, D, sub_dla=nhi_sub, raise_numeric=True, **kw)
        r["sub_again"] = eng.process_models(packed, D, sub_dla=nhi_sub, raise_numeric=True, **kw)
        r["sub_dev"] = eng.process_models(packed, D, sub_dla=nhi_sub, raise_numeric=True, memory="device", **kw)
        eng.set_forest(dict(variance_series=False, mean_flux=True, mean_flux_tau_0=0.0))
        r["tau_zero"] = eng.process_models(packed, D, sub_dla=nhi_sub, raise_numeric=True, **kw)
        eng.set_forest(FOREST)
        r["forest"] = eng.process_models(packed, D, sub_dla=nhi_sub, raise_numeric=True, **kw)
        r["forest_single"] = eng.process(packed)
        eng.set_forest(None)
        r["restored"] = eng.process_models(packed, D, sub_dla=nhi_sub, raise_numeric=True, **kw)
        r["restored_single"] = eng.process(packed)
        r["stats"] = eng.stats()
    with Engine(model, dict(samples, nhi_samples=nhi_sub), params) as eng:
        r["as_dla"] = eng.process(packed)
    for qb in (1, 2):
        with Engine(model, samples, params, max_batch_spectra=qb) as eng:
            eng.set_forest(FOREST)
            r[f"forest_qb{qb}"] = eng.process_models(packed, D, sub_dla=nhi_sub, raise_numeric=True, **kw)
            r[f"forest_single_qb{qb}"] = eng.process(packed)      # the host pipeline: copies beside the kernels
    return r


def _all_same(a, b, skip=()):
    assert sorted(a) == sorted(b)
    for key in a:
        if key not in skip:
            assert _same(a[key], b[key]), key


def test_without_sub_dla_process_models_is_the_plain_call(exact):
    _all_same(exact["models_none_multi"], exact["multi"])
    _all_same(exact["models_none_summ"], exact["summ"])


def test_sub_dla_rows_are_the_engine_on_those_column_densities(exact):
    sub, as_dla = exact["sub"], exact["as_dla"]
    assert _same(sub["sample_log_likelihoods_lls"], as_dla["sample_log_likelihoods_dla"])
    assert _same(sub["log_likelihoods_lls"], as_dla["log_likelihoods_dla"])
    assert np.all(np.isfinite(sub["log_likelihoods_lls"]))
    # the MAP sample of the sub-DLA rows: nanmax's first maximum, its z and log N
    rows = sub["sample_log_likelihoods_lls"]
    j = np.argmax(rows, axis=1)
    assert np.array_equal(sub["map_sample_ind_lls"], j)
    assert np.array_equal(sub["map_log_likelihood_lls"], rows[np.arange(rows.shape[0]), j])
    s = syn.make_samples(S_LEVEL)
    z = sub["min_z_dlas"] + (sub["max_z_dlas"] - sub["min_z_dlas"]) * s["offset_samples"][j]
    assert np.array_equal(sub["MAP_z_lls"], z)
    assert np.array_equal(sub["MAP_log_nhi_lls"], np.log10(_sub_samples(S_LEVEL)["lls_nhi_samples"])[j])


def test_sub_dla_leaves_every_other_result_alone(exact):
    new = {"log_likelihoods_lls", "sample_log_likelihoods_lls", "map_sample_ind_lls", "map_log_likelihood_lls", "MAP_z_lls",
           "MAP_log_nhi_lls"}
    sub = {k: v for k, v in exact["sub"].items() if k not in new}
    assert set(exact["sub"]) - set(sub) == new
    _all_same(sub, exact["summ"])                        # level 1, the null, the deeper level, the summaries
    assert _same(exact["sub"]["sample_log_likelihoods_dla"][0], exact["single"]["sample_log_likelihoods_dla"])
    assert _same(exact["sub"]["log_likelihoods_no_dla"], exact["single"]["log_likelihoods_no_dla"])
    # the sub-DLA sweep's null lane and samples are not counted in gpdla_stats: per call Q spectra, Q S evaluations
    st = exact["stats"]
    assert st["sample_evals"] == st["spectra"] * S_LEVEL and st["likelihood_launches"] == st["prep_launches"]


def test_repeats_memory_spaces_and_batches_agree(exact):
    _all_same(exact["sub"], exact["sub_again"])
    _all_same(exact["sub"], exact["sub_dev"])
    for qb in (1, 2):
        _all_same(exact["forest"], exact[f"forest_qb{qb}"])
        _all_same(exact["forest_single"], exact[f"forest_single_qb{qb}"])


def test_zero_mean_flux_and_restore_are_forest_off(exact):
    _all_same(exact["tau_zero"], exact["sub"])           # mu exp(-0) = mu exactly
    _all_same(exact["restored"], exact["sub"])           # set_forest(None) restores today's output
    _all_same(exact["restored_single"], exact["single"])
    # while it is on, the forest moves the null and every model of every spectrum
    for key in ("log_likelihoods_no_dla", "log_likelihoods_dla", "log_likelihoods_lls"):
        assert np.all(exact["forest"][key] != exact["sub"][key]), key
    assert _same(exact["forest"]["log_likelihoods_no_dla"], exact["forest_single"]["log_likelihoods_no_dla"])
    assert _same(exact["forest"]["sample_log_likelihoods_dla"][0], exact["forest_single"]["sample_log_likelihoods_dla"])


# ------------------------------------------------------------------------------ 4. unusable spectrum
def test_unusable_spectrum_gives_nan_and_no_map():
    s = _setup(4, "reference")
    Q = len(s["spectra"])
    with Engine(s["model"], s["samples"], s["params"]) as eng:
        eng.set_forest(FOREST)
        out = eng.process_models(s["packed"], 1, sub_dla=s["sub"]["lls_nhi_samples"], log_nhi_samples=s["samples"]["log_nhi_samples"])
    assert np.all(np.isnan(out["sample_log_likelihoods_lls"][Q - 1])) and np.isnan(out["log_likelihoods_lls"][Q - 1])
    assert out["map_sample_ind_lls"][Q - 1] == -1 and np.isnan(out["map_log_likelihood_lls"][Q - 1])
    assert np.isnan(out["MAP_z_lls"][Q - 1]) and np.isnan(out["MAP_log_nhi_lls"][Q - 1])
    assert np.all(out["map_sample_ind_lls"][:Q - 1] >= 0) and np.all(np.isfinite(out["MAP_z_lls"][:Q - 1]))
    assert np.all((out["MAP_log_nhi_lls"][:Q - 1] >= 19.5) & (out["MAP_log_nhi_lls"][:Q - 1] <= 20.0))


# ----------------------------------------------------------------------------------------- 5. errors
def _raises(code, fn, *a, **kw):
    with pytest.raises(L.GpdlaError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, ei.value


def test_argument_errors():
    model = syn.make_model(k=8)
    S = 64
    samples = syn.make_samples(S)
    packed = syn.pack_spectra([syn.make_spectrum(model, 0, n_target=220)])
    params = set_parameters(k=8)
    good = _sub_samples(S)["lls_nhi_samples"]
    with Engine(model, samples, params) as eng:
        for bad in (dict(num_forest_lines=0), dict(num_forest_lines=32), dict(mean_flux_tau_0=-1e-3),
                    dict(mean_flux_tau_0=np.inf), dict(mean_flux_tau_0=np.nan), dict(mean_flux_beta=np.nan),
                    dict(mean_flux_beta=np.inf)):
            _raises(L.GPDLA_EINVAL, eng.set_forest, bad)
        for bad in (0.0, -1e19, np.inf, np.nan):
            nhi = good.copy()
            nhi[5] = bad
            _raises(L.GPDLA_EINVAL, eng.process_models, packed, 1, sub_dla=nhi)
        # null arrays, through the C ABI itself (the argument checks come before anything is read)
        lib, h = eng.lib, eng._h
        sp, md, rs = L.Spectra(), L.MultiDla(max_dlas=1), L.ResultsMulti()
        ev = np.zeros(1)
        ok_sub, ok_res = L.SubDla(nhi_samples=L.ptr(good)), L.ResultsSub(log_likelihoods_lls=L.ptr(ev), sample_ld=S)
        call = lambda sub, rsub: lib.gpdla_engine_process_models(h, C.byref(sp), C.byref(md), sub, C.byref(rs), rsub, None, None)  # noqa: E731
        assert call(C.byref(ok_sub), None) == L.GPDLA_EINVAL                                  # null results struct
        assert call(C.byref(ok_sub), C.byref(L.ResultsSub(sample_ld=S))) == L.GPDLA_EINVAL    # null evidence array
        assert call(C.byref(L.SubDla()), C.byref(ok_res)) == L.GPDLA_EINVAL                   # null column densities
        rows = np.zeros(S)
        short = L.ResultsSub(log_likelihoods_lls=L.ptr(ev), sample_log_likelihoods_lls=L.ptr(rows), sample_ld=S - 1)
        assert call(C.byref(ok_sub), C.byref(short)) == L.GPDLA_EINVAL
        assert lib.gpdla_engine_get_model_stats(h, None) == L.GPDLA_EINVAL
        # after the refusals the engine still runs
        out = eng.process_models(packed, 1, sub_dla=good)
        assert np.isfinite(out["log_likelihoods_lls"][0])
    for path in ("fused_i8", "panel_gemm", "panel_gemm_i8"):
        with Engine(model, samples, params, path=path) as eng:
            _raises(L.GPDLA_EUNSUPPORTED, eng.set_forest, FOREST)
            assert b"fused fp64" in eng.lib.gpdla_last_error()
            _raises(L.GPDLA_EUNSUPPORTED, eng.process_models, packed, 1, sub_dla=good)
            assert b"fused fp64" in eng.lib.gpdla_last_error()
            eng.set_forest(None)                                    # restoring is always allowed
            one = eng.process_models(packed, 1)                     # without sub_dla: the engine's own path
            assert np.isfinite(one["log_likelihoods_dla"][0, 0])


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
    kw = dict(prior=prior, params=params, max_dlas=D, summaries=True, sub_dla=sub, forest=True)
    out = PR.process_qsos(model, samples, packed, **kw)
    Q = len(spectra)
    assert out["model_posteriors"].shape == (Q, 1 + D + 1)
    np.testing.assert_allclose(out["model_posteriors"].sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert np.array_equal(out["p_dlas"], 1 - out["p_no_dlas"] - out["p_lls"])
    # the oracle-backed CPU run on the device's own base indices
    forced = (np.asarray(out["base_sample_inds"]).reshape(Q, S_LEVEL, D - 1).transpose(2, 0, 1) - 1).astype(np.int32)
    cpu = PR.process_qsos(model, samples, packed, compute=functools.partial(SO.compute, forced=forced), **kw)
    path = tmp_path / "processed_qsos_dr12q.mat"
    PR.save_processed_qsos(str(path), out)
    r = M.loadmat(str(path))
    for key in PR.SUB_DLA_VARIABLES + PR.FOREST_VARIABLES:
        assert key in r, key
        got, want = np.asarray(r[key], dtype=np.float64).ravel(), np.asarray(cpu[key], dtype=np.float64).ravel()
        assert got.size == want.size and np.array_equal(np.isnan(got), np.isnan(want)), key
        err = np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0))
        print(f"{key}: max rel err {err:.3g}")
        assert np.all(tol_ok(got, want, 1e-9)), key
    assert r["model_posteriors"].shape == (Q, 1 + D + 1) and r["sample_log_likelihoods_lls"].shape == (Q, S_LEVEL)
    assert np.all(tol_ok(r["model_posteriors"], cpu["model_posteriors"], 1e-9))
    # without the two keywords the same call writes today's variables only
    plain = PR.process_qsos(model, samples, packed, prior=prior, params=params, max_dlas=D, summaries=True)
    assert not set(plain) & (set(PR.SUB_DLA_VARIABLES) | set(PR.FOREST_VARIABLES))
    assert plain["model_posteriors"].shape == (Q, 1 + D)

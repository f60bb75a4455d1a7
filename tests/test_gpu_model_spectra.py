"""Model spectra on the GPU: gpdla_engine_model_spectra against the numpy oracle
(model_spectra_oracle.py) on the inputs of model_spectra_cases.py, its tie to the sweeps' likelihoods, what must be
bitwise equal, the units, the capacity error and the argument errors; then the same launch inside a search call
(gpdla_engine_process_spectra_models): its tie to every level's sweep, level selection against
catalog.absorber_table, the intervals in the same call, process_qsos down to the saved file.  Shapes: Q <= 8,
S <= 96, n <= 300, but for the one case that must pass GPDLA_MODEL_SPECTRA_LDS (n = 1,100)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import model_spectra_cases as MC  # noqa: E402
import model_spectra_oracle as MO  # noqa: E402
from conftest import tol_ok  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import Engine, model_capacities  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402

pytestmark = pytest.mark.gpu

FLAT = ("pixel_inds", "absorption", "model_mean", "continuum", "continuum_sd")
PER_Q = ("chi2", "log_likelihoods", "num_pixels")


def _run(c, spectra=None, absorbers=None, **kw):
    spectra = c["spectra"] if spectra is None else spectra
    z, n, cnt = MC.absorber_arrays(c["absorbers"] if absorbers is None else absorbers)
    with Engine(c["model"], syn.make_samples(64), c["params"], max_batch_spectra=kw.pop("max_batch_spectra", 0)) as eng:
        if c["forest"] is not None:
            eng.set_forest(c["forest"])
        return eng.model_spectra(syn.pack_spectra(spectra), z, n, cnt, **kw)


def _same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key


def _rows(out, q):
    sl = slice(int(out["offsets"][q]), int(out["offsets"][q + 1]))
    return {k: out[k][sl] for k in FLAT}


# ----------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("name", sorted(MC.cases()))
def test_standalone_entry_against_the_oracle(name):
    """absorption to gpdla_voigt_f64's bar in test_gpu_parity.py (1e-12 absolute, 1e-9 relative above 1e-200) times
    the number of absorbers; every other output to tol_ok(rtol=1e-9)."""
    c = MC.cases()[name]
    out = _run(c)
    worst = dict.fromkeys(("absorption", "model_mean", "continuum", "continuum_sd", "chi2", "log_likelihood"), 0.0)
    for q, (spec, ab) in enumerate(zip(c["spectra"], c["absorbers"])):
        ref = MO.model_spectrum(spec, c["model"], [a[0] for a in ab], [10.0 ** a[1] for a in ab], c["num_lines"],
                                c["mode"], c["forest"])
        got = _rows(out, q)
        if ref is None:   # no usable pixel: an empty slice and NaN scalars
            assert got["absorption"].size == 0 and out["num_pixels"][q] == 0
            assert np.isnan(out["chi2"][q]) and np.isnan(out["log_likelihoods"][q])
            continue
        assert out["num_pixels"][q] == ref["n"] and np.array_equal(got["pixel_inds"], ref["pixel_inds"])
        na = max(len(ab), 1)
        da = np.abs(got["absorption"] - ref["absorption"])
        assert np.max(da) < 1e-12 * na, (q, np.max(da))
        big = ref["absorption"] > 1e-200
        assert np.max(da[big] / ref["absorption"][big]) < 1e-9 * na
        worst["absorption"] = max(worst["absorption"], float(np.max(da)))
        if not ab:
            assert np.all(got["absorption"] == 1.0)
        for key in ("model_mean", "continuum", "continuum_sd"):
            err = np.max(np.abs(got[key] - ref[key]) / np.maximum(np.abs(ref[key]), 1.0))
            worst[key] = max(worst[key], float(err))
            assert np.all(tol_ok(got[key], ref[key], 1e-9)), (q, key, err)
        for key, okey in (("chi2", "chi2"), ("log_likelihood", "log_likelihoods")):
            err = abs(out[okey][q] - ref[key]) / max(abs(ref[key]), 1.0)
            worst[key] = max(worst[key], float(err))
            assert tol_ok(out[okey][q], ref[key], 1e-9), (q, key, err)
    print(f"{name}: worst deviations " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ------------------------------------------------------------------------------ 2. tie to the sweeps
def test_log_likelihood_is_the_sweeps():
    """The model log-likelihood of sample j's absorber against the level-1 sweep's sample_log_likelihoods_dla[q][j]
    of the same engine, and the null model against log_likelihoods_no_dla: 2e-9 relative (each is within 1e-9 of
    the oracle)."""
    c = MC.cases()["masked_unmasked"]
    samples = syn.make_samples(64)
    packed = syn.pack_spectra(c["spectra"])
    Q = len(c["spectra"])
    worst = 0.0
    with Engine(c["model"], samples, c["params"]) as eng:
        sweep = eng.process(packed)
        for j in (0, 17, 63):
            z = sweep["min_z_dlas"] + (sweep["max_z_dlas"] - sweep["min_z_dlas"]) * samples["offset_samples"][j]
            out = eng.model_spectra(packed, z[:, None], np.full((Q, 1), samples["log_nhi_samples"][j]),
                                    nhis=np.full((Q, 1), samples["nhi_samples"][j]))
            want = sweep["sample_log_likelihoods_dla"][:, j]
            worst = max(worst, float(np.max(np.abs(out["log_likelihoods"] - want) / np.abs(want))))
        null = eng.model_spectra(packed, np.zeros((Q, 0)), np.zeros((Q, 0)))
        worst0 = float(np.max(np.abs(null["log_likelihoods"] - sweep["log_likelihoods_no_dla"]) /
                              np.abs(sweep["log_likelihoods_no_dla"])))
        assert np.array_equal(null["num_pixels"], sweep["num_pixels"])
    print(f"model against sweep: level 1 worst {worst:.3g}, null {worst0:.3g}")
    assert worst <= 2e-9 and worst0 <= 2e-9


# --------------------------------------------------------------------------------- 3. bitwise equal
def test_repeats_batching_and_alone_are_bitwise_equal():
    c = MC.cases()["sizes_b"]
    z, n, cnt = MC.absorber_arrays(c["absorbers"])
    packed = syn.pack_spectra(c["spectra"])
    with Engine(c["model"], syn.make_samples(64), c["params"]) as eng:
        a = eng.model_spectra(packed, z, n, cnt)
        _same(a, eng.model_spectra(packed, z, n, cnt))
        assert eng.model_spectra_stats()["model_spectra_launches"] == 2
        for q in (1, 4):   # a spectrum alone against inside the batch
            one = eng.model_spectra(syn.pack_spectra([c["spectra"][q]]), z[q:q + 1], n[q:q + 1], cnt[q:q + 1])
            for key in FLAT:
                assert np.array_equal(one[key], _rows(a, q)[key], equal_nan=True), key
            for key in PER_Q:
                assert np.array_equal(one[key], a[key][q:q + 1], equal_nan=True), key
    _same(a, _run(c, max_batch_spectra=1))


def test_device_result_memory_is_bitwise_the_host_one():
    c = MC.cases()["masked_reference"]
    z, n, cnt = MC.absorber_arrays(c["absorbers"])
    packed = syn.pack_spectra(c["spectra"])
    Q = len(c["spectra"])
    lib = L.load()
    with Engine(c["model"], syn.make_samples(64), c["params"]) as eng:
        host = eng.model_spectra(packed, z, n, cnt)
        caps = model_capacities(packed, c["params"])
        cap_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
        tot = int(cap_off[-1])
        sizes = dict(pixel_inds=4 * tot, absorption=8 * tot, model_mean=8 * tot, continuum_mean=8 * tot,
                     continuum_sd=8 * tot, chi2=8 * Q, log_likelihoods=8 * Q, num_pixels=4 * Q)
        dev = {}
        try:
            for key, nbytes in sizes.items():
                p = C.c_void_p()
                L.check(lib.gpdla_device_malloc(0, nbytes, C.byref(p)))
                dev[key] = p
            cast = lambda key, t: C.cast(dev[key], C.POINTER(t))
            rs = L.ModelSpectra(memory=L.MEM_DEVICE, cap_offsets=L.ptr(cap_off, C.c_int64),
                                pixel_inds=cast("pixel_inds", C.c_int32), absorption=cast("absorption", C.c_double),
                                model_mean=cast("model_mean", C.c_double), continuum_mean=cast("continuum_mean", C.c_double),
                                continuum_sd=cast("continuum_sd", C.c_double), chi2=cast("chi2", C.c_double),
                                log_likelihoods=cast("log_likelihoods", C.c_double), num_pixels=cast("num_pixels", C.c_int32))
            arr = {k: np.ascontiguousarray(packed[k]) for k in ("offsets", "wavelengths", "flux", "noise_variance", "z_qsos")}
            mk = np.ascontiguousarray(packed["pixel_mask"], dtype=np.uint8)
            sp = L.Spectra(memory=L.MEM_HOST, num_spectra=Q, offsets=L.ptr(arr["offsets"], C.c_int64),
                           wavelengths=L.ptr(arr["wavelengths"]), flux=L.ptr(arr["flux"]),
                           noise_variance=L.ptr(arr["noise_variance"]), pixel_mask=L.ptr(mk, C.c_uint8), z_qsos=L.ptr(arr["z_qsos"]))
            ab = L.ModelAbsorbers(counts=L.ptr(cnt, C.c_int32), z_dlas=L.ptr(z), log_nhis=L.ptr(n), nhis=None)
            L.check(lib.gpdla_engine_model_spectra(eng._h, C.byref(sp), C.byref(ab), C.byref(rs)))
            L.check(lib.gpdla_engine_synchronize(eng._h))
            back = {}
            for key, nbytes in sizes.items():
                buf = np.empty(nbytes // (4 if key in ("pixel_inds", "num_pixels") else 8),
                               dtype=np.int32 if key in ("pixel_inds", "num_pixels") else np.float64)
                L.check(lib.gpdla_memcpy_dtoh(0, buf.ctypes.data_as(C.c_void_p), dev[key], nbytes))
                back[key] = buf
        finally:
            for p in dev.values():
                lib.gpdla_device_free(0, p)
    assert np.array_equal(back["num_pixels"], host["num_pixels"])
    for key, hkey in (("chi2", "chi2"), ("log_likelihoods", "log_likelihoods")):
        assert np.array_equal(back[key], host[hkey], equal_nan=True), key
    for q in range(Q):
        sl = slice(int(cap_off[q]), int(cap_off[q]) + int(host["num_pixels"][q]))
        for key, hkey in (("pixel_inds", "pixel_inds"), ("absorption", "absorption"), ("model_mean", "model_mean"),
                          ("continuum_mean", "continuum"), ("continuum_sd", "continuum_sd")):
            assert np.array_equal(back[key][sl], _rows(host, q)[hkey], equal_nan=True), (q, key)


# ------------------------------------------------------------------------------------------ 4. units
def test_rescaled_spectrum_comes_back_in_the_callers_units():
    """flux x 2^70 and sigma^2 x 2^140 (prep rescales: scale_e != 0), in a batch with a spectrum left as it is,
    against the unscaled run: flux-like outputs x 2^-70 and chi2 to the 1e-9 bar, the log-likelihood after the
    n 70 ln 2 shift.  The two runs describe the same data only if the model is in the same units as the flux, so the
    scaled run's engine holds mu, M x 2^70 and omega x 2^70; an engine has one model, hence two engines."""
    c = MC.cases()["masked_unmasked"]
    s0 = c["spectra"][3]
    big = dict(s0, flux=s0["flux"] * 2.0 ** 70, noise_variance=s0["noise_variance"] * 2.0 ** 140)
    m = c["model"]
    scaled = dict(c, model=dict(m, mu=m["mu"] * 2.0 ** 70, M=np.asfortranarray(m["M"] * 2.0 ** 70),
                                log_omega=m["log_omega"] + 70 * np.log(2.0)))
    ab = c["absorbers"][3]
    plain = _run(c, spectra=[s0, c["spectra"][4]], absorbers=[ab, []])
    out = _run(scaled, spectra=[c["spectra"][4], big], absorbers=[[], ab])
    a, b = _rows(plain, 0), _rows(out, 1)
    out = {k: v[1:] if k in PER_Q else v for k, v in out.items()}
    out = dict(out, chi2=np.array([plain["chi2"][0], out["chi2"][0]]),
               log_likelihoods=np.array([plain["log_likelihoods"][0], out["log_likelihoods"][0]]),
               num_pixels=np.array([plain["num_pixels"][0], out["num_pixels"][0]]))
    assert np.array_equal(a["pixel_inds"], b["pixel_inds"]) and out["num_pixels"][0] == out["num_pixels"][1]
    assert np.array_equal(a["absorption"], b["absorption"])
    for key in ("model_mean", "continuum", "continuum_sd"):
        assert np.all(tol_ok(b[key] * 2.0 ** -70, a[key], 1e-9)), key
    assert np.max(np.abs(b["model_mean"])) > 2.0 ** 60            # really in the caller's (large) units
    assert tol_ok(out["chi2"][1], out["chi2"][0], 1e-9)
    shift = out["num_pixels"][0] * 70 * np.log(2.0)
    assert tol_ok(out["log_likelihoods"][1] + shift, out["log_likelihoods"][0], 1e-9)


# --------------------------------------------------------------------------------------- 5. capacity
def test_capacity_one_short_is_an_error_and_spares_the_neighbours():
    c = MC.cases()["masked_reference"]
    spectra, absorbers = c["spectra"][:3], c["absorbers"][:3]
    full = _run(c, spectra=spectra, absorbers=absorbers)
    exact = _run(c, spectra=spectra, absorbers=absorbers, capacities=full["num_pixels"])
    _same(full, exact)
    caps = full["num_pixels"].astype(np.int64)
    caps[1] -= 1
    with pytest.raises(L.GpdlaError) as ei:
        _run(c, spectra=spectra, absorbers=absorbers, capacities=caps)
    assert ei.value.code == L.GPDLA_EINVAL and "spectrum 1" in str(ei.value) and "capacity" in str(ei.value)
    part = ei.value.partial
    assert part["offsets"][2] == part["offsets"][1] and part["num_pixels"][1] == full["num_pixels"][1]
    for q in (0, 2):
        for key in FLAT:
            assert np.array_equal(_rows(part, q)[key], _rows(full, q)[key], equal_nan=True), (q, key)
        for key in PER_Q:
            assert np.array_equal(part[key][q], full[key][q], equal_nan=True)


# -------------------------------------------------------------------------------- 6. argument errors
@pytest.mark.parametrize("path", ["fused_i8", "panel_gemm", "panel_gemm_i8"])
def test_other_paths_are_unsupported(path):
    c = MC.cases()["rank_20"]
    z, n, cnt = MC.absorber_arrays(c["absorbers"])
    with Engine(c["model"], syn.make_samples(64), c["params"], path=path) as eng:
        with pytest.raises(L.GpdlaError) as ei:
            eng.model_spectra(syn.pack_spectra(c["spectra"]), z, n, cnt)
    assert ei.value.code == L.GPDLA_EUNSUPPORTED and "fused fp64" in str(ei.value)


def test_bad_absorbers_raise_and_nan_absorbers_give_nan():
    c = MC.cases()["rank_4"]
    packed = syn.pack_spectra(c["spectra"])
    with Engine(c["model"], syn.make_samples(64), c["params"]) as eng:
        with pytest.raises(ValueError):
            eng.model_spectra(packed, np.zeros((2, 4)), np.zeros((2, 4)), counts=[5, 0])
        with pytest.raises(ValueError):
            eng.model_spectra(packed, np.zeros((2, 5)), np.zeros((2, 5)))
        # a level without a MAP sample: NaN outputs, n and the pixel indices as usual, no fault
        out = eng.model_spectra(packed, np.full((2, 1), np.nan), np.full((2, 1), np.nan), counts=[1, 0])
        ok = eng.model_spectra(packed, np.zeros((2, 0)), np.zeros((2, 0)))
    assert np.array_equal(out["num_pixels"], ok["num_pixels"]) and np.array_equal(out["pixel_inds"], ok["pixel_inds"])
    assert np.isnan(out["chi2"][0]) and np.isnan(out["log_likelihoods"][0]) and np.all(np.isnan(_rows(out, 0)["continuum"]))
    assert np.all(np.isnan(_rows(out, 0)["absorption"]))
    for key in FLAT:
        assert np.array_equal(_rows(out, 1)[key], _rows(ok, 1)[key]), key


# ------------------------------------------------------------------ 7. inside a search call
S_SEARCH = 96
MODEL_KEYS = ("model_offsets", "model_pixel_inds", "model_absorption", "model_mean", "model_continuum",
              "model_continuum_sd", "model_levels", "model_log_likelihoods", "model_chi2", "model_num_pixels")


def _search_setup():
    c = MC.cases()["masked_unmasked"]
    spectra = c["spectra"][:5] + [MC.cases()["sizes_a"]["spectra"][-1]]      # the last has no usable pixel
    # (sizes_a's spectra were drawn for k = 20; only their pixels matter here)
    samples = syn.make_samples(S_SEARCH)
    Q = len(spectra)
    # log priors that put spectrum q's mass on level 1 + q % 3, so that "best" meets every level
    lp = np.where(np.arange(3)[:, None] == np.arange(Q)[None, :] % 3, np.log(0.3), -200.0)
    return c, spectra, syn.pack_spectra(spectra), samples, lp


def _stand_alone(eng, packed, out, levels):
    """gpdla_engine_model_spectra fed each spectrum's level's MAP pairs of ``out``."""
    Q = levels.size
    z, n = np.full((Q, 4), np.nan), np.full((Q, 4), np.nan)
    for q, d in enumerate(levels):
        if d > 0:
            z[q, :d], n[q, :d] = out["MAP_z_dlas"][d - 1, q, :d], out["MAP_log_nhis"][d - 1, q, :d]
    return eng.model_spectra(packed, z, n, counts=levels.astype(np.int32))


def test_search_call_ties_to_the_sweeps_at_every_level():
    """model_log_likelihoods of level d against map_log_likelihoods[d - 1] of the same call, d = 1..3 on a
    max_dlas = 3 run, and level 0 against log_likelihoods_no_dla: 2e-9 relative; each engine-path result bitwise
    the stand-alone entry fed the same pairs; the summaries bitwise process_summaries'."""
    c, spectra, packed, samples, lp = _search_setup()
    Q = len(spectra)
    with Engine(c["model"], samples, c["params"]) as eng:
        plain = eng.process_summaries(packed, 3, samples["log_nhi_samples"])
        for d in (0, 1, 2, 3):
            out = eng.process_model_spectra(packed, 3, samples["log_nhi_samples"], level=d)
            for key in plain:
                assert np.array_equal(np.asarray(out[key]), np.asarray(plain[key]), equal_nan=True), key
            assert np.all(out["model_levels"] == d)
            want = out["log_likelihoods_no_dla"] if d == 0 else out["map_log_likelihoods"][d - 1]
            got = out["model_log_likelihoods"]
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[Q - 1]) and np.isfinite(got[:Q - 1]).all()
            fin = np.isfinite(want)
            err = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin])))
            print(f"search call, level {d}: model against sweep, worst {err:.3g}")
            assert err <= 2e-9
            alone = _stand_alone(eng, packed, out, np.full(Q, d))
            for key, mkey in (("offsets", "model_offsets"), ("pixel_inds", "model_pixel_inds"), ("absorption", "model_absorption"),
                              ("model_mean", "model_mean"), ("continuum", "model_continuum"),
                              ("continuum_sd", "model_continuum_sd"), ("chi2", "model_chi2"),
                              ("log_likelihoods", "model_log_likelihoods"), ("num_pixels", "model_num_pixels")):
                assert np.array_equal(alone[key], out[mkey], equal_nan=True), (d, key)


def test_best_level_is_the_highest_posterior_and_its_pairs_are_rendered():
    c, spectra, packed, samples, lp = _search_setup()
    Q = len(spectra)
    with Engine(c["model"], samples, c["params"]) as eng:
        out = eng.process_model_spectra(packed, 3, samples["log_nhi_samples"], level="best", log_priors_dla=lp)
        # catalog.absorber_table's rule: argmax of the DLA levels' posteriors, NaN last, first maximum
        post = out["log_likelihoods_dla"] + lp
        want = np.argmax(np.where(np.isnan(post), -np.inf, post), axis=0) + 1
        assert np.array_equal(out["model_levels"], want) and len(set(want[:Q - 1])) > 1, want
        alone = _stand_alone(eng, packed, out, want)
        for key, mkey in (("absorption", "model_absorption"), ("continuum", "model_continuum"), ("chi2", "model_chi2"),
                          ("log_likelihoods", "model_log_likelihoods"), ("pixel_inds", "model_pixel_inds")):
            assert np.array_equal(alone[key], out[mkey], equal_nan=True), key
        # the same call with the intervals: its interval outputs are process_intervals', the model outputs are
        # unchanged, and catalog.absorber_table -- fed this call's arrays in process_qsos's shapes, with the model
        # posteriors of these priors -- takes the same level and lists the pairs that were rendered
        from gp_dla_detection_amd import catalog as CAT
        from gp_dla_detection_amd import process as PR
        ivs = dict(levels=np.array([0.16, 0.5, 0.84]), lr_delta=2.0)
        both = eng.process_model_spectra(packed, 3, samples["log_nhi_samples"], level="best", log_priors_dla=lp, intervals=ivs)
        ref_iv = eng.process_intervals(packed, 3, samples["log_nhi_samples"], levels=ivs["levels"], lr_delta=2.0)
        for key in ref_iv:
            assert np.array_equal(np.asarray(both[key]), np.asarray(ref_iv[key]), equal_nan=True), key
        for key in MODEL_KEYS:
            assert np.array_equal(both[key], out[key], equal_nan=True), key
        tab_in = PR._finish_multi(dict(both), packed["z_qsos"], None, c["params"], None, 3)
        tab_in["log_priors_dla"] = np.ascontiguousarray(lp.T)
        tab_in["log_posteriors_dla"] = tab_in["log_priors_dla"] + tab_in["log_likelihoods_dla"]
        tab_in["model_posteriors"] = PR.model_posteriors_multi(tab_in["log_posteriors_no_dla"], tab_in["log_posteriors_dla"])[0]
        PR._finish_summaries(tab_in, both, True, 3)
        PR._finish_intervals(tab_in, both, ivs, 3)
        table = CAT.absorber_table(tab_in)
        first = np.searchsorted(table["spectrum"], np.arange(Q))
        assert np.array_equal(table["level"][first], both["model_levels"])
        zt, nt = np.full((Q, 4), np.nan), np.full((Q, 4), np.nan)
        zt[table["spectrum"], table["absorber"]] = table["map_z_dla"]
        nt[table["spectrum"], table["absorber"]] = table["map_log_nhi"]
        listed = eng.model_spectra(packed, zt, nt, counts=table["level"][first].astype(np.int32))
        for key, mkey in (("absorption", "model_absorption"), ("continuum", "model_continuum"),
                          ("log_likelihoods", "model_log_likelihoods")):
            assert np.array_equal(listed[key], both[mkey], equal_nan=True), key
        per_q = eng.process_model_spectra(packed, 3, samples["log_nhi_samples"], level=want)
        one = eng.process_model_spectra(packed, 1, samples["log_nhi_samples"])        # D = 1: no priors needed
        assert np.all(one["model_levels"] == 1)
    for key in MODEL_KEYS:
        assert np.array_equal(per_q[key], out[key], equal_nan=True), key


def test_search_call_is_bitwise_stable():
    """Repeats, max_batch_spectra 1 against all-in-one, with against without the sample buffers."""
    c, spectra, packed, samples, lp = _search_setup()
    kw = dict(level="best", log_priors_dla=lp)
    with Engine(c["model"], samples, c["params"]) as eng:
        a = eng.process_model_spectra(packed, 3, samples["log_nhi_samples"], **kw)
        b = eng.process_model_spectra(packed, 3, samples["log_nhi_samples"], **kw)
        w = eng.process_model_spectra(packed, 3, samples["log_nhi_samples"], want_samples=True, **kw)
    with Engine(c["model"], samples, c["params"], max_batch_spectra=1) as eng:
        o = eng.process_model_spectra(packed, 3, samples["log_nhi_samples"], **kw)
    for key in MODEL_KEYS + ("MAP_z_dlas", "map_log_likelihoods", "log_likelihoods_dla"):
        for other in (b, w, o):
            assert np.array_equal(np.asarray(a[key]), np.asarray(other[key]), equal_nan=True), key


def test_search_call_argument_errors():
    c, spectra, packed, samples, lp = _search_setup()
    with Engine(c["model"], samples, c["params"]) as eng:
        for bad in (4, -1, "worst", 1.5, np.zeros(3, dtype=int)):
            with pytest.raises(ValueError):
                eng.process_model_spectra(packed, 3, samples["log_nhi_samples"], level=bad)
        with pytest.raises(ValueError):
            eng.process_model_spectra(packed, 3, samples["log_nhi_samples"])          # best needs the priors
        with pytest.raises(ValueError):
            eng.process_model_spectra(packed, 3, samples["log_nhi_samples"], log_priors_dla=lp[:2])
    with Engine(c["model"], samples, c["params"], path="fused_i8") as eng:
        with pytest.raises(L.GpdlaError) as ei:
            eng.process_model_spectra(packed, 1, samples["log_nhi_samples"])
    assert ei.value.code == L.GPDLA_EUNSUPPORTED


# ------------------------------------------------------------- 8. process_qsos and the saved file
def test_process_qsos_keyword_through_the_saved_file(tmp_path):
    """The variables are in the output and the v7.3 file and equal the engine's; "best" is absorber_table's level
    and the rendered absorbers are the file's MAP pairs; without the keyword the output, the file's variable list
    and every array are bitwise those of the same call with summaries alone."""
    from gp_dla_detection_amd import catalog as CAT
    from gp_dla_detection_amd import matv73 as M
    from gp_dla_detection_amd import process as PR
    c, spectra, packed, samples, lp = _search_setup()
    Q, D = len(spectra), 3
    without = PR.process_qsos(c["model"], samples, packed, params=c["params"], max_dlas=D, summaries=True)
    full = PR.process_qsos(c["model"], samples, packed, params=c["params"], max_dlas=D, model_spectra=True)
    lean = PR.process_qsos(c["model"], samples, packed, params=c["params"], max_dlas=D, model_spectra=dict(level="best"),
                           save_samples=False)
    assert set(full) - set(without) == set(PR.MODEL_SPECTRA_VARIABLES)
    for key in without:
        assert np.array_equal(np.asarray(without[key]), np.asarray(full[key]), equal_nan=True), key
    for key in lean:
        assert np.array_equal(np.asarray(lean[key]), np.asarray(full[key]), equal_nan=True), key
    # the level is the one MAP_z_dlas / absorber_table take, and the absorbers rendered are the file's MAP pairs
    post = full["model_posteriors"][:, 1:1 + D]
    level = np.argmax(np.where(np.isnan(post), -np.inf, post), axis=1) + 1
    assert np.array_equal(full["model_levels"], level)
    with Engine(c["model"], samples, c["params"]) as eng:
        alone = eng.model_spectra(packed, full["MAP_z_dlas"], full["MAP_log_nhis"], counts=level.astype(np.int32))
        direct = eng.process_model_spectra(packed, D, samples["log_nhi_samples"], level="best",
                                           log_priors_dla=np.ascontiguousarray(full["log_priors_dla"].T))
    for key, mkey in CAT.MODEL_SPECTRA_KEYS.items():
        assert np.array_equal(alone[key], full[mkey], equal_nan=True), key
    for key in PR.MODEL_SPECTRA_VARIABLES:
        assert np.array_equal(direct[key], full[key], equal_nan=True), key
    for name, out in (("with", lean), ("without", {k: v for k, v in without.items() if k not in
                                                   ("sample_log_likelihoods_dla", "base_sample_inds")})):
        out = dict(out, test_ind=np.ones(Q, dtype=bool))
        PR.save_processed_qsos(str(tmp_path / f"{name}.mat"), out)
    r, r0 = M.loadmat(str(tmp_path / "with.mat")), M.loadmat(str(tmp_path / "without.mat"))
    names = lambda d: {k for k in d if not k.startswith("_")}
    assert names(r) - names(r0) == set(PR.MODEL_SPECTRA_VARIABLES)
    for key in names(r0):
        assert np.array_equal(np.asarray(r0[key]), np.asarray(r[key]), equal_nan=True), key
    for key in PR.MODEL_SPECTRA_VARIABLES:
        assert np.array_equal(np.asarray(r[key]).reshape(np.shape(lean[key])), lean[key], equal_nan=True), key
    s1 = CAT.model_spectrum(r | {k: np.asarray(r[k]).ravel() for k in PR.MODEL_SPECTRA_VARIABLES}, 1, spectra[1]["wavelengths"])
    assert s1["fit"].size == full["model_num_pixels"][1] and np.all(np.isfinite(s1["fit"]))
    iv = PR.process_qsos(c["model"], samples, packed, params=c["params"], max_dlas=D, model_spectra=True, intervals=True)
    assert set(iv) - set(full) == set(PR.INTERVAL_VARIABLES)
    for key in full:
        assert np.array_equal(np.asarray(iv[key]), np.asarray(full[key]), equal_nan=True), key
    table = CAT.absorber_table(iv)
    assert np.array_equal(table["level"][np.searchsorted(table["spectrum"], np.arange(Q))], iv["model_levels"])
    # a scoped forest inside the search call at a level >= 1: bitwise the stand-alone entry under the same forest
    fst = dict(MC.FOREST, mean_flux_scope="all")
    with Engine(c["model"], samples, c["params"]) as eng:
        plain2 = eng.process_model_spectra(packed, 2, samples["log_nhi_samples"], level=2)
        eng.set_forest(fst)
        fo = eng.process_model_spectra(packed, 2, samples["log_nhi_samples"], level=2)
        fa = _stand_alone(eng, packed, fo, np.full(Q, 2))
    assert not np.array_equal(fo["model_continuum"], plain2["model_continuum"], equal_nan=True)
    for key, mkey in CAT.MODEL_SPECTRA_KEYS.items():
        assert np.array_equal(fa[key], fo[mkey], equal_nan=True), key
    assert np.nanmin(fo["model_absorption"]) < 0.5                     # absorbers were rendered, not a = 1
    one = PR.process_qsos(c["model"], samples, packed, params=c["params"], model_spectra=dict(level=0), forest=True)
    assert np.all(one["model_levels"] == 0) and np.all(one["model_absorption"] == 1.0) and "num_forest_lines" in one


def test_process_qsos_rejects_what_is_not_covered(tmp_path):
    from gp_dla_detection_amd import process as PR
    c, spectra, packed, samples, lp = _search_setup()
    kw = dict(params=c["params"])
    for bad in (dict(sub_dla=True), dict(cuts=dict(proximity_zone=0.1)),
                dict(population=dict(z_edges=np.linspace(2, 4, 3), log_nhi_edges=np.linspace(20, 23, 4)))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            PR.process_qsos(c["model"], samples, packed, model_spectra=True, **bad, **kw)
    for lvl in (2, "deepest", 0.5, [0, 1]):
        with pytest.raises(ValueError, match="level"):
            PR.process_qsos(c["model"], samples, packed, model_spectra=dict(level=lvl), **kw)
    with pytest.raises(ValueError, match="model_spectra"):
        PR.process_qsos(c["model"], samples, packed, model_spectra=dict(depth=1), **kw)
    with pytest.raises(ValueError, match="run_process_qsos"):
        PR.run_process_qsos(str(tmp_path), "a", "b", "c", None, "d", "e", None, model_spectra=True)

"""Multi-DLA search on the GPU against the numpy oracle (multi_dla_oracle.py): the resampler alone,
the level-d sweep with forced base indices, level 1 / batching / memory spaces unchanged, the whole
chain with the engine's own resampler, and the argument errors."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import multi_dla_oracle as MO  # noqa: E402
from conftest import tol_ok  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import Engine, resample  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402

pytestmark = pytest.mark.gpu

S_LEVEL = 333            # neither S nor S + 1 is a multiple of 64


# ------------------------------------------------------------------------------------ 1. resampler
def _rows(S, rng):
    """(exact rows: weights all 0 or 1, sums exact in any order; inexact rows)."""
    flat = np.zeros(S)
    spike = np.full(S, -np.inf)
    spike[S // 3] = 5.0
    two = np.full(S, -np.inf)
    two[S // 5] = two[(4 * S) // 5] = -2.5              # two spikes between runs of -inf
    mixed = rng.choice([2.0, np.nan, -np.inf], size=S)  # 0 / 1 weights with NaNs
    mixed[rng.integers(S)] = 2.0
    allnan = np.full(S, np.nan)
    nans = rng.normal(0.0, 3.0, S)
    nans[rng.random(S) < 0.2] = np.nan
    nans[rng.integers(S)] = 1.0
    wide = -1e5 * rng.random(S)                         # dynamic range 1e5 in l
    smooth = rng.normal(0.0, 1.0, S)
    return np.stack([flat, spike, two, mixed, allnan]), np.stack([nans, wide, smooth])


@pytest.mark.parametrize("S", [1, 63, 64, 65, 200, 1025, 10000])
def test_resampler_alone(S):
    rng = np.random.default_rng(100 + S)
    exact, inexact = _rows(S, rng)
    u = rng.random(S)
    got = resample(np.concatenate([exact, inexact]), u)
    assert got.dtype == np.int32 and got.shape == (8, S)
    for r, row in enumerate(exact):                      # exact sums: every index, ties included
        assert np.array_equal(got[r], MO.resample(row, u)), ("exact row", r)
    assert np.all(got[4] == -1)                          # the all-NaN row
    for r, row in enumerate(inexact):
        want = MO.resample(row, u)
        amb, nearest = MO.ambiguous(row, u)
        print(f"S={S} row {r}: ambiguous {int(amb.sum())}, nearest edge {nearest:.3g} W")
        assert amb.sum() <= 1e-3 * S
        assert np.array_equal(got[5 + r][~amb], want[~amb]), ("inexact row", r)
        assert np.all(MO.neighbours_ok(row, got[5 + r][amb], want[amb]))
    # u exactly on an edge of an exact row: C_i > u W is strict, so u W = C_i selects the next weight
    ue = np.arange(S) / S
    on_edge = ue * S == np.arange(S)
    assert on_edge.any()
    got_e = resample(exact, ue)
    for r, row in enumerate(exact):
        assert np.array_equal(got_e[r], MO.resample(row, ue)), ("edge row", r)
    assert np.array_equal(got_e[0][on_edge], np.arange(S)[on_edge])   # flat row: C_i = i + 1 > j  <=>  i >= j


def test_resampler_prefix_sum_beyond_lds():
    """Above GPDLA_RESAMPLE_LDS = 16,384 samples the prefix sum lives in global memory: another code
    path, which only a row that long can reach (hence the one size above 10^4; two rows, milliseconds)."""
    S = 16384 + 1025
    rng = np.random.default_rng(11)                      # the oracle finds no ambiguous entry (nearest 3e-9 W)
    flat = np.zeros(S)
    flat[rng.random(S) < 0.3] = np.nan                   # exact: weights 0 / 1
    smooth = rng.normal(0.0, 1.0, S)
    u = rng.random(S)
    got = resample(np.stack([flat, smooth, np.full(S, np.nan)]), u)
    assert np.array_equal(got[0], MO.resample(flat, u))
    want = MO.resample(smooth, u)
    amb, nearest = MO.ambiguous(smooth, u)
    print(f"S={S}: ambiguous {int(amb.sum())}, nearest edge {nearest:.3g} W")
    assert amb.sum() <= 1e-3 * S
    assert np.array_equal(got[1][~amb], want[~amb])
    assert np.all(MO.neighbours_ok(smooth, got[1][amb], want[amb]))
    assert np.all(got[2] == -1)


# ----------------------------------------------------------------------- 2. level kernel, forced indices
def _level_spectra(model):
    mk = dict(mask_fraction=0.05)
    return [syn.make_spectrum(model, 0, z_qso=2.6, n_target=300, **mk),
            syn.make_spectrum(model, 1, z_qso=3.1, n_target=None, **mk),
            syn.make_spectrum(model, 2, n_target=270, **mk),
            syn.make_spectrum(model, 3, n_target=300, mask_fraction=1.0)]      # J = 0: NaN rows


_cache = {}


def _setup(k, mode):
    key = (k, mode)
    if key not in _cache:
        model = syn.make_model(k=k)
        samples = syn.make_samples(S_LEVEL)
        spectra = _level_spectra(model)
        oracles = [MO.SpectrumOracle(s, model, samples, 3, mode) for s in spectra]
        forced = np.random.default_rng(77).integers(0, S_LEVEL, (3, len(spectra), S_LEVEL)).astype(np.int32)
        _cache[key] = dict(model=model, samples=samples, spectra=spectra, packed=syn.pack_spectra(spectra),
                           params=set_parameters(k=k, absorption_mode=mode), oracles=oracles, forced=forced)
    return _cache[key]


@pytest.mark.parametrize("k,mode,D", [(4, "reference", 3), (4, "unmasked", 3), (6, "reference", 3),
                                      (6, "unmasked", 3), (20, "reference", 3), (20, "unmasked", 3),
                                      (20, "reference", 4)])
def test_level_kernel_forced_indices(k, mode, D):
    s = _setup(k, mode)
    Q = len(s["spectra"])
    forced = s["forced"][:D - 1]
    ref = [MO.process_spectrum_multi(sp, s["model"], s["samples"], D, forced=forced[:, q], absorption_mode=mode,
                                     oracle=s["oracles"][q]) for q, sp in enumerate(s["spectra"])]
    ref_sll = np.stack([r["sample_log_likelihoods_dla"] for r in ref], axis=1)
    ref_lld = np.stack([r["log_likelihoods_dla"] for r in ref], axis=1)
    # condition on the oracle: the exclusion leaves most of every usable (spectrum, level)
    for q in range(Q - 1):
        for d in range(1, D):
            share = np.isnan(ref_sll[d, q]).mean()
            print(f"k={k} {mode} spectrum {q} level {d + 1}: excluded {share:.3f}")
            assert share <= 0.40
    assert np.all(np.isnan(ref_sll[:, Q - 1])) and np.all(np.isnan(ref_lld[:, Q - 1]))
    with Engine(s["model"], s["samples"], s["params"]) as eng:
        out = eng.process_multi(s["packed"], D, base_sample_inds=forced, raise_numeric=True)
    got = out["sample_log_likelihoods_dla"]
    assert np.array_equal(out["base_sample_inds"], forced)
    assert np.array_equal(np.isnan(got), np.isnan(ref_sll))
    fin = np.isfinite(ref_sll)
    err = np.abs(got[fin] - ref_sll[fin]) / np.maximum(np.abs(ref_sll[fin]), 1.0)
    print(f"k={k} {mode} D={D}: max rel err samples {err.max():.3g}")
    assert np.all(tol_ok(got[fin], ref_sll[fin], 1e-6)) and np.all(tol_ok(got[fin], ref_sll[fin], 1e-9))
    lld = out["log_likelihoods_dla"]
    assert np.array_equal(np.isnan(lld), np.isnan(ref_lld))
    fin = np.isfinite(ref_lld)
    assert np.all(tol_ok(lld[fin], ref_lld[fin], 1e-6)) and np.all(tol_ok(lld[fin], ref_lld[fin], 1e-9))
    null = np.array([r["log_likelihood_no_dla"] for r in ref])
    assert np.all(tol_ok(out["log_likelihoods_no_dla"][:-1], null[:-1], 1e-9)) and np.isnan(out["log_likelihoods_no_dla"][-1])


def test_level_two_symmetry_on_device():
    s = _setup(20, "reference")
    Q = len(s["spectra"])
    p = np.random.default_rng(5).permutation(S_LEVEL).astype(np.int32)
    inv = np.argsort(p).astype(np.int32)
    with Engine(s["model"], s["samples"], s["params"]) as eng:
        a = eng.process_multi(s["packed"], 2, base_sample_inds=np.tile(p, (1, Q, 1)))["sample_log_likelihoods_dla"][1]
        b = eng.process_multi(s["packed"], 2, base_sample_inds=np.tile(inv, (1, Q, 1)))["sample_log_likelihoods_dla"][1]
    # l2(j | base p[j]) against l2(p[j] | base j)
    lhs, rhs = a, b[:, p]
    assert np.array_equal(np.isnan(lhs), np.isnan(rhs))
    fin = np.isfinite(lhs)
    assert fin[:Q - 1].mean() > 0.5
    assert np.all(np.abs(lhs[fin] - rhs[fin]) <= 1e-13 * np.maximum(np.abs(lhs[fin]), 1.0))


# ------------------------------------------------------------------------------- 3. unchanged ground
@pytest.fixture(scope="module")
def chain():
    """Three spectra (one with an injected DLA), k = 8, D = 3 with the engine's own resampler."""
    k, D = 8, 3
    model = syn.make_model(k=k)
    samples = syn.make_samples(S_LEVEL)
    spectra = [syn.make_spectrum(model, 0, n_target=300, mask_fraction=0.05, dla_fraction=1.0),
               syn.make_spectrum(model, 1, z_qso=2.9, n_target=280, mask_fraction=0.05, dla_fraction=0.0),
               syn.make_spectrum(model, 2, n_target=310, mask_fraction=0.05, dla_fraction=0.0)]
    packed = syn.pack_spectra(spectra)
    params = set_parameters(k=k)
    with Engine(model, samples, params) as eng:
        single = eng.process(packed)
        u = eng.default_resample_uniforms(D)
        host = eng.process_multi(packed, D, raise_numeric=True)
        dev = eng.process_multi(packed, D, raise_numeric=True, memory="device")
    with Engine(model, samples, params, max_batch_spectra=2) as eng2:
        batched = eng2.process_multi(packed, D, raise_numeric=True)
    return dict(model=model, samples=samples, spectra=spectra, packed=packed, params=params, D=D, u=u,
                single=single, host=host, dev=dev, batched=batched)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_level_one_is_engine_process_bitwise(chain):
    one, multi = chain["single"], chain["host"]
    assert _same(multi["sample_log_likelihoods_dla"][0], one["sample_log_likelihoods_dla"])
    assert _same(multi["log_likelihoods_dla"][0], one["log_likelihoods_dla"])
    for key in ("log_likelihoods_no_dla", "min_z_dlas", "max_z_dlas", "num_pixels"):
        assert _same(multi[key], one[key]), key


def test_batches_and_memory_spaces_bitwise(chain):
    for other in ("batched", "dev"):
        for key in ("sample_log_likelihoods_dla", "log_likelihoods_dla", "base_sample_inds", "log_likelihoods_no_dla",
                    "min_z_dlas", "max_z_dlas", "num_pixels"):
            assert _same(chain["host"][key], chain[other][key]), (other, key)


# ---------------------------------------------------------------- 4. whole chain, engine's resampler
def test_whole_chain_with_engine_resampler(chain):
    c = chain
    D, u, out = c["D"], c["u"], c["host"]
    assert u.shape == (D - 1, S_LEVEL) and np.all((u >= 0) & (u < 1))
    sll, base = out["sample_log_likelihoods_dla"], out["base_sample_inds"]
    for q, spec in enumerate(c["spectra"]):
        for d in range(2, D + 1):        # the device's indices are the oracle resampler on the device's own rows
            want = MO.resample(sll[d - 2, q], u[d - 2])
            amb, nearest = MO.ambiguous(sll[d - 2, q], u[d - 2])
            print(f"spectrum {q} level {d}: ambiguous {int(amb.sum())}, nearest edge {nearest:.3g} W, "
                  f"{np.unique(base[d - 2, q]).size} distinct base samples")
            assert amb.sum() <= 1e-3 * S_LEVEL
            assert np.array_equal(base[d - 2, q][~amb], want[~amb])
            assert np.all(MO.neighbours_ok(sll[d - 2, q], base[d - 2, q][amb], want[amb]))
        ref = MO.process_spectrum_multi(spec, c["model"], c["samples"], D, forced=base[:, q])
        assert np.array_equal(np.isnan(sll[:, q]), np.isnan(ref["sample_log_likelihoods_dla"]))
        fin = np.isfinite(ref["sample_log_likelihoods_dla"])
        assert np.all(tol_ok(sll[:, q][fin], ref["sample_log_likelihoods_dla"][fin], 1e-9))
        assert np.all(tol_ok(out["log_likelihoods_dla"][:, q], ref["log_likelihoods_dla"], 1e-9))


def test_process_qsos_three_dlas(chain):
    c = chain
    Q, D = len(c["spectra"]), 3
    out = PR.process_qsos(c["model"], c["samples"], c["packed"], params=c["params"], max_dlas=D)
    assert out["sample_log_likelihoods_dla"].shape == (Q, S_LEVEL, D)
    assert out["base_sample_inds"].shape == (Q, S_LEVEL, D - 1) and out["base_sample_inds"].dtype == np.float64
    assert out["base_sample_inds"].min() >= 1 and out["base_sample_inds"].max() <= S_LEVEL
    for key in ("log_likelihoods_dla", "log_priors_dla", "log_posteriors_dla"):
        assert out[key].shape == (Q, D), key
    assert out["model_posteriors"].shape == (Q, 1 + D) and out["max_dlas"] == D
    np.testing.assert_allclose(out["model_posteriors"].sum(axis=1), 1.0, atol=1e-14)
    assert _same(out["sample_log_likelihoods_dla"][:, :, 0], c["single"]["sample_log_likelihoods_dla"])
    assert _same(np.transpose(out["sample_log_likelihoods_dla"], (2, 0, 1)), c["host"]["sample_log_likelihoods_dla"])
    one = PR.process_qsos(c["model"], c["samples"], c["packed"], params=c["params"])
    assert one["log_likelihoods_dla"].shape == (Q,) and "base_sample_inds" not in one


# ----------------------------------------------------------------------------------------- 5. errors
def _raises(code, fn, *a, **kw):
    with pytest.raises(L.GpdlaError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, ei.value


def test_argument_errors():
    model = syn.make_model(k=8)
    samples = syn.make_samples(64)
    packed = syn.pack_spectra([syn.make_spectrum(model, 0, n_target=220)])
    params = set_parameters(k=8)
    S = 64
    with Engine(model, samples, params) as eng:
        _raises(L.GPDLA_EINVAL, eng.process_multi, packed, 0)
        _raises(L.GPDLA_EINVAL, eng.process_multi, packed, 5)
        for bad in (1.0, -0.25, np.nan):
            u = np.full((1, S), 0.5)
            u[0, 7] = bad
            _raises(L.GPDLA_EINVAL, eng.process_multi, packed, 2, resample_uniforms=u)
        for bad in (-2, S):
            b = np.zeros((1, 1, S), dtype=np.int32)
            b[0, 0, 3] = bad
            _raises(L.GPDLA_EINVAL, eng.process_multi, packed, 2, base_sample_inds=b)
        b = np.zeros((1, 1, S), dtype=np.int32)
        b[0, 0, 3] = -1                                      # allowed: that sample has no base, NaN
        out = eng.process_multi(packed, 2, base_sample_inds=b)
        assert np.isnan(out["sample_log_likelihoods_dla"][1, 0, 3])
        assert np.isfinite(out["sample_log_likelihoods_dla"][1, 0]).sum() > S // 2
    for path in ("panel_gemm", "fused_i8", "panel_gemm_i8"):
        with Engine(model, samples, params, path=path) as eng:
            _raises(L.GPDLA_EUNSUPPORTED, eng.process_multi, packed, 2)
            assert b"fused fp64" in eng.lib.gpdla_last_error()
            one = eng.process_multi(packed, 1)                # D = 1 is the engine's own path
            assert np.isfinite(one["log_likelihoods_dla"][0, 0])
    with Engine(model, samples, set_parameters(k=8, num_lines=5)) as eng:
        _raises(L.GPDLA_EUNSUPPORTED, eng.process_multi, packed, 2)
        assert b"num_lines" in eng.lib.gpdla_last_error()
    ll = np.zeros((1, 8))
    with pytest.raises(L.GpdlaError) as ei:
        resample(ll, np.r_[np.full(7, 0.5), 1.0])
    assert ei.value.code == L.GPDLA_EINVAL
    out = np.zeros(8, dtype=np.int32)
    assert L.load().gpdla_resample_f64(0, L.ptr(ll), 1, 8, 4, L.ptr(np.full(8, 0.5)), L.ptr(out, C.c_int32)) == L.GPDLA_EINVAL

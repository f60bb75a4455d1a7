"""Posterior intervals on the GPU (csrc/posterior_intervals.hip) against the fsum oracle
(posterior_intervals_oracle.py): the kernel alone over sizes, row shapes, chains, ties, redshift ranges and
quantile levels; the engine call (bitwise against the stand-alone kernel, batching, repeats, memory spaces, with
and without the sample buffers, every other output untouched); process_qsos(intervals=...) through the saved
file; the argument errors.

Bars, with eps = (S + 16) 2^-52 and F, T from the oracle's own masses: ranges and counts bitwise; a quantile x* is
bitwise a value of the slot with F(x*) >= level T (1 - eps) and F(x*-) <= level T (1 + eps); mean within 2 eps
relative; variance within 4 eps relative plus (2 eps |mean|)^2.  Where every mass is a power of two the cdf sums
are exact and the quantiles equal the oracle's bitwise."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import posterior_intervals_oracle as IO  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import DEFAULT_INTERVAL_LEVELS, Engine, posterior_intervals  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402

pytestmark = pytest.mark.gpu

INTERVAL_KEYS = ("z_dla_quantiles", "log_nhi_quantiles", "z_dla_means", "z_dla_sds", "log_nhi_means", "log_nhi_sds",
                 "z_dla_lr_ranges", "log_nhi_lr_ranges", "lr_counts")
WORST = dict(cdf_low=0.0, cdf_high=0.0, mean=0.0, var=0.0)     # measured deviations in units of the bars' eps


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# the row shapes of test_gpu_posterior_summary.py
ROWS = ("flat", "spike", "two", "last", "pow2", "allnan", "neginf", "nans", "wide", "smooth")


def _rows(S, rng):
    flat = np.zeros(S)
    spike = np.full(S, -np.inf)
    spike[S // 3] = 5.0
    two = rng.normal(0.0, 1.0, S) - 10.0
    two[S // 5] = two[(4 * S) // 5] = 2.5                # two equal maxima
    last = rng.normal(0.0, 1.0, S)
    last[S - 1] = 9.0
    # 0 / 1 weights with NaNs, the finite count a power of two: pi = 2^-k, every cdf sum exact
    P = 1 << (S.bit_length() - 1)
    if P == S and S > 1:
        P //= 2
    pow2 = np.full(S, np.nan)
    pow2[rng.permutation(S)[:P]] = 2.0
    allnan = np.full(S, np.nan)
    neginf = np.full(S, -np.inf)
    nans = rng.normal(0.0, 3.0, S)
    nans[rng.random(S) < 0.2] = np.nan
    nans[rng.integers(S)] = 1.0
    wide = -1e5 * rng.random(S)                          # dynamic range 1e5 in l
    smooth = rng.normal(0.0, 1.0, S)
    return np.stack([flat, spike, two, last, pow2, allnan, neginf, nans, wide, smooth])


def check(got, ll, base, min_z, max_z, offset, log_nhi, levels=DEFAULT_INTERVAL_LEVELS, lr_delta=2.0, exact_rows=(),
          tag=""):
    """Every bar of the module docstring for the outputs ``got`` of one call; rows in ``exact_rows`` (every level)
    have power-of-two masses: their quantiles must equal the oracle's bitwise."""
    ll = np.asarray(ll, dtype=np.float64)
    if ll.ndim == 2:
        ll = ll[None]
    D, R, S = ll.shape
    levels = np.asarray(levels, dtype=np.float64)
    eps = (S + 16) * 2.0 ** -52
    want = IO.intervals(ll, base, min_z, max_z, offset, log_nhi, levels, lr_delta, quantiles=False)
    for key in ("z_dla_lr_ranges", "log_nhi_lr_ranges", "lr_counts"):
        assert got[key].shape == want[key].shape, (tag, key)
        assert _same(got[key], want[key]), (tag, key)
    assert got["lr_counts"].dtype == np.int32
    for d in range(D):
        for r in range(R):
            pi, m, usable = IO.row_masses(ll[d, r])
            c, ok = IO.chains(base, d, r, S)
            T = math.fsum(pi[ok]) if usable else 0.0
            for u in range(D):
                for p, name in enumerate(("z_dla", "log_nhi")):
                    q = got[name + "_quantiles"][d, r, u]
                    mean, sd = got[name + "_means"][d, r, u], got[name + "_sds"][d, r, u]
                    where = (tag, name, d, r, u)
                    live = u <= d and T > 0.0 and (p == 1 or IO.z_range_ok(min_z[r], max_z[r]))
                    if not live:
                        assert np.isnan(q).all() and np.isnan(mean) and np.isnan(sd), where
                        continue
                    x = IO.slot_values(c, u, min_z[r], max_z[r], offset, log_nhi)[p][ok]
                    pv = pi[ok]
                    wm = want[name + "_means"][d, r, u]
                    assert abs(mean - wm) <= 2 * eps * abs(wm), where + (mean, wm)
                    WORST["mean"] = max(WORST["mean"], abs(mean - wm) / (eps * abs(wm)) if wm else 0.0)
                    wv = want[name + "_sds"][d, r, u] ** 2
                    bar = 4 * eps * wv + (2 * eps * abs(wm)) ** 2
                    assert abs(sd * sd - wv) <= bar, where + (sd * sd, wv)
                    WORST["var"] = max(WORST["var"], abs(sd * sd - wv) / bar if bar else 0.0)
                    for k, lv in enumerate(levels):
                        assert (x == q[k]).any(), where + (k, "not a value of the slot")
                        F, Fm = IO.mass_at_or_below(x, pv, q[k]), IO.mass_at_or_below(x, pv, q[k], strict=True)
                        assert F >= lv * T * (1 - eps), where + (k, F, lv * T)
                        assert Fm <= lv * T * (1 + eps), where + (k, Fm, lv * T)
                        WORST["cdf_low"] = max(WORST["cdf_low"], (lv * T - F) / (lv * T * eps))
                        WORST["cdf_high"] = max(WORST["cdf_high"], (Fm - lv * T) / (lv * T * eps))
                        if r in exact_rows:
                            assert q[k] == IO.quantile(x, pv, lv)[0], where + (k, "exact row")
    return want


def _report(tag):
    print(f"{tag}: worst deviations in eps: " + ", ".join(f"{k} {v:.3g}" for k, v in WORST.items()))


# ---------------------------------------------------------------------------------- 1. kernel alone
# the tile edges, the coarse shift 0 -> 1 -> 2 (1024 | 1025, 2048 | 2049) and the workload's own S
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 10000])
def test_kernel_alone(S):
    rng = np.random.default_rng(700 + S)
    ll = _rows(S, rng)
    R = ll.shape[0]
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)
    min_z = np.linspace(1.8, 2.6, R)
    max_z = min_z + np.linspace(0.4, 1.9, R)
    got = posterior_intervals(ll, offset, log_nhi, min_z, max_z)
    assert got["z_dla_quantiles"].shape == (1, R, 1, 5) and got["z_dla_lr_ranges"].shape == (1, R, 1, 2)
    exact = [ROWS.index("pow2")] + ([ROWS.index("flat")] if S & (S - 1) == 0 else [])
    check(got, ll, None, min_z, max_z, offset, log_nhi, exact_rows=exact, tag=f"S={S}")
    for name in ("allnan", "neginf"):      # no usable weight sum: NaN everywhere, count 0
        r = ROWS.index(name)
        assert got["lr_counts"][0, r] == 0
        for key in INTERVAL_KEYS[:-1]:
            assert np.isnan(got[key][0, r]).all(), (name, key)
    r = ROWS.index("spike")                # one sample carries everything
    j = S // 3
    assert got["lr_counts"][0, r] == 1 and np.all(got["log_nhi_quantiles"][0, r, 0] == log_nhi[j])
    assert got["log_nhi_means"][0, r, 0] == log_nhi[j] and got["log_nhi_sds"][0, r, 0] == 0.0
    assert np.all(got["z_dla_lr_ranges"][0, r, 0] == IO.sample_z(min_z[r], max_z[r], offset[j]))
    _report(f"S={S}")


def test_largest_sample_count():
    """Two rows at S = 2^20 (coarse shift 10: the fine passes run in groups of two levels), and one sample more."""
    S = 1 << 20
    rng = np.random.default_rng(11)
    ll = np.stack([np.zeros(S), rng.normal(0.0, 1.5, S)])
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)
    min_z, max_z = np.array([2.0, 2.2]), np.array([3.5, 3.1])
    levels = (0.16, 0.5, 0.84)
    got = posterior_intervals(ll, offset, log_nhi, min_z, max_z, levels=levels)
    check(got, ll, None, min_z, max_z, offset, log_nhi, levels=levels, exact_rows=[0], tag="S=2^20")
    _report("S=2^20")
    with pytest.raises(L.GpdlaError) as ei:
        posterior_intervals(np.zeros((1, S + 1)), np.zeros(S + 1), np.zeros(S + 1), [2.0], [3.0])
    assert ei.value.code == L.GPDLA_EINVAL and "at most 1048576 samples" in str(ei.value)


def test_row_alone_and_repeat():
    """Two calls are bitwise equal, and a row's outputs do not depend on the rows around it."""
    S = 1025
    rng = np.random.default_rng(9)
    ll = rng.normal(0.0, 2.0, (7, S))
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)
    min_z, max_z = np.linspace(2.0, 2.5, 7), np.linspace(3.0, 4.2, 7)
    a = posterior_intervals(ll, offset, log_nhi, min_z, max_z)
    b = posterior_intervals(ll, offset, log_nhi, min_z, max_z)
    c = posterior_intervals(ll[2:5], offset, log_nhi, min_z[2:5], max_z[2:5])
    for key in INTERVAL_KEYS:
        assert _same(a[key], b[key]), key
        assert _same(a[key][:, 2:5], c[key]), key


# ------------------------------------------------------------------------------------------ 2. chains
@pytest.mark.parametrize("levels", [2, 3, 4])
@pytest.mark.parametrize("bases", ["random", "repeated"])
def test_chains(levels, bases):
    """Levels 2..4: chains with -1 and out-of-range entries (void: they contribute to nothing), and chains whose
    bases repeat, so that many samples share one slot value."""
    S, R = 333, 6
    rng = np.random.default_rng(40 + levels + (100 if bases == "repeated" else 0))
    ll = rng.normal(0.0, 2.0, (levels, R, S))
    ll[rng.random(ll.shape) < 0.1] = np.nan
    ll[levels - 1, 4] = np.nan                                   # an unusable row at the deepest level
    base = rng.integers(0, 7 if bases == "repeated" else S, (levels - 1, R, S)).astype(np.int32)
    void = rng.random(base.shape)
    base[void < 0.2] = -1
    base[(void >= 0.2) & (void < 0.25)] = S                      # one past the end
    base[(void >= 0.25) & (void < 0.3)] = -7
    base[levels - 2, 5] = -1                                     # row 5: no valid chain at the deepest level
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)
    min_z, max_z = rng.uniform(1.9, 2.4, R), rng.uniform(2.9, 4.3, R)
    got = posterior_intervals(ll, offset, log_nhi, min_z, max_z, base_sample_inds=base)
    assert got["z_dla_quantiles"].shape == (levels, R, levels, 5)
    check(got, ll, base, min_z, max_z, offset, log_nhi, tag=f"levels={levels} {bases}")
    d = levels - 1
    assert got["lr_counts"][d, 4] == 0 and got["lr_counts"][d, 5] == 0
    assert np.isnan(got["log_nhi_means"][d, 5]).all() and np.isnan(got["log_nhi_quantiles"][d, 5]).all()
    assert np.isfinite(got["log_nhi_means"][d, 0]).all()
    for lv in range(levels):               # slots beyond the level stay NaN
        assert np.isnan(got["z_dla_means"][lv, :, lv + 1:]).all()
    _report(f"levels={levels} {bases}")


# ------------------------------------------------------------------------- 3. ties, ranges, levels
@pytest.mark.parametrize("S", [300, 2049])
def test_ties_in_the_sample_arrays(S):
    """Exact ties in offset and in log N_HI: equal values share a rank, and a quantile is the value itself.  The
    flat-with-NaNs row has power-of-two masses: bitwise the oracle's."""
    rng = np.random.default_rng(S)
    offset = np.round(rng.random(S), 2)                          # about 100 distinct values
    log_nhi = np.round(rng.uniform(20.0, 23.0, S), 1)            # about 30
    P = 1 << (S.bit_length() - 2)
    pow2 = np.full(S, np.nan)
    pow2[rng.permutation(S)[:P]] = -3.0
    ll = np.stack([rng.normal(0.0, 2.0, S), pow2, np.zeros(S)])
    min_z, max_z = np.array([2.0, 2.1, 2.2]), np.array([3.0, 3.3, 2.9])
    got = posterior_intervals(ll, offset, log_nhi, min_z, max_z)
    check(got, ll, None, min_z, max_z, offset, log_nhi, exact_rows=[1], tag=f"ties S={S}")


def test_redshift_ranges():
    """min_z == max_z is legal (every z quantile is that value); max_z < min_z or a non-finite end gives NaN z
    outputs while log N_HI is computed as for any row: the same numbers as with a good range."""
    S = 257
    rng = np.random.default_rng(5)
    row = rng.normal(0.0, 2.0, S)
    ll = np.tile(row, (6, 1))
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)
    min_z = np.array([2.0, 2.5, 3.0, np.nan, np.inf, 2.0])
    max_z = np.array([3.0, 2.5, 2.9, 3.0, 3.0, -np.inf])
    got = posterior_intervals(ll, offset, log_nhi, min_z, max_z)
    check(got, ll, None, min_z, max_z, offset, log_nhi, tag="z ranges")
    assert np.all(got["z_dla_quantiles"][0, 1] == 2.5) and np.all(got["z_dla_lr_ranges"][0, 1] == 2.5)
    for r in (2, 3, 4, 5):
        for key in ("z_dla_quantiles", "z_dla_means", "z_dla_sds", "z_dla_lr_ranges"):
            assert np.isnan(got[key][0, r]).all(), (r, key)
    for key in ("log_nhi_quantiles", "log_nhi_means", "log_nhi_sds", "log_nhi_lr_ranges", "lr_counts"):
        for r in range(1, 6):
            assert _same(got[key][0, r], got[key][0, 0]), (r, key)


@pytest.mark.parametrize("levels", [(0.5,), DEFAULT_INTERVAL_LEVELS, tuple(np.linspace(0.05, 0.95, 8))])
def test_quantile_level_counts(levels):
    S = 2049
    rng = np.random.default_rng(len(levels))
    ll = np.stack([rng.normal(0.0, 2.0, S), np.zeros(S)])
    ll = np.stack([ll, ll[::-1] + rng.normal(0.0, 1.0, (2, S))])
    base = rng.integers(0, S, (1, 2, S)).astype(np.int32)
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)
    min_z, max_z = np.array([2.0, 2.1]), np.array([3.0, 3.3])
    got = posterior_intervals(ll, offset, log_nhi, min_z, max_z, base_sample_inds=base, levels=levels, lr_delta=0.75)
    assert got["log_nhi_quantiles"].shape == (2, 2, 2, len(levels)) and np.array_equal(got["interval_levels"], levels)
    check(got, ll, base, min_z, max_z, offset, log_nhi, levels=levels, lr_delta=0.75, tag=f"{len(levels)} levels")
    full = posterior_intervals(ll, offset, log_nhi, min_z, max_z, base_sample_inds=base, lr_delta=0.75)
    if 0.5 in levels:                        # a level's quantile does not depend on the other levels asked for
        k, k5 = list(levels).index(0.5), list(DEFAULT_INTERVAL_LEVELS).index(0.5)
        assert _same(got["z_dla_quantiles"][..., k], full["z_dla_quantiles"][..., k5])


def test_golden_reference_numbers():
    """The kernel on the fixture's rows against the reference's find_delta_NHI / find_delta_z, bit for bit."""
    from gp_dla_detection_amd import catalog as CAT
    g = np.load(Path(__file__).parent / "golden" / "posterior_intervals.npz")
    got = posterior_intervals(g["sample_log_likelihoods"], g["offset_samples"], g["log_nhi_samples"], g["min_z_dlas"],
                              g["max_z_dlas"])
    as_saved = {key: np.swapaxes(got[key], 0, 1) for key in ("z_dla_lr_ranges", "log_nhi_lr_ranges")}
    as_saved = {key: np.concatenate([v, np.full((v.shape[0], 1, 3, 2), np.nan)], axis=2) for key, v in as_saved.items()}
    assert np.array_equal(CAT.find_delta_nhi(as_saved), g["ref_delta_nhi"])
    assert np.array_equal(CAT.find_delta_z(as_saved), g["ref_delta_z"])
    assert np.array_equal(got["lr_counts"][0], g["lr_counts"])


# ------------------------------------------------------------------------------------------ 4. engine
S_LEVEL = 333
Z_EDGES, N_EDGES = np.linspace(1.6, 4.6, 8), np.linspace(20.0, 23.0, 6)
SUMMARY_KEYS = ("map_sample_inds", "map_log_likelihoods", "MAP_z_dlas", "MAP_log_nhis", "bin_planes")
MULTI_KEYS = ("log_likelihoods_no_dla", "log_likelihoods_dla", "min_z_dlas", "max_z_dlas", "num_pixels")


def _spectra(model):
    mk = dict(mask_fraction=0.05)
    return [syn.make_spectrum(model, 0, z_qso=2.6, n_target=300, **mk),
            syn.make_spectrum(model, 1, z_qso=3.1, n_target=None, **mk),
            syn.make_spectrum(model, 2, n_target=270, **mk),
            syn.make_spectrum(model, 3, n_target=300, mask_fraction=1.0)]      # J = 0: NaN rows


@pytest.mark.parametrize("k,D", [(4, 1), (4, 3), (20, 1), (20, 3)])
def test_engine_intervals(k, D):
    model = syn.make_model(k=k)
    samples = syn.make_samples(S_LEVEL)
    packed = syn.pack_spectra(_spectra(model))
    params = set_parameters(k=k)
    lognhi = samples["log_nhi_samples"]
    kw = dict(z_edges=Z_EDGES, log_nhi_edges=N_EDGES)
    with Engine(model, samples, params) as eng:
        plain = eng.process_summaries(packed, D, lognhi, want_samples=True, **kw)
        full = eng.process_intervals(packed, D, lognhi, want_samples=True, **kw)
        lean = eng.process_intervals(packed, D, lognhi, **kw)
        again = eng.process_intervals(packed, D, lognhi, **kw)
        dev = eng.process_intervals(packed, D, lognhi, memory="device", **kw)
        only = eng.process_intervals(packed, D, lognhi)                    # no summary grid
        stats = eng.interval_stats()
        assert eng.summary_stats()["summary_launches"] == 6
    assert stats["interval_launches"] == 5 and stats["interval_ms"] > 0
    # every pre-existing output is what process_summaries gives without intervals
    for key in MULTI_KEYS + SUMMARY_KEYS + ("sample_log_likelihoods_dla", "base_sample_inds"):
        assert _same(full[key], plain[key]), key
    assert "sample_log_likelihoods_dla" not in lean and "base_sample_inds" not in lean and "bin_planes" not in only
    for other in (lean, again, dev, only):
        for key in INTERVAL_KEYS:
            assert _same(full[key], other[key]), key
    for other in (lean, again, dev):
        for key in MULTI_KEYS + SUMMARY_KEYS:
            assert _same(full[key], other[key]), key
    # ... and the intervals are the stand-alone kernel on the arrays the same run returned
    alone = posterior_intervals(full["sample_log_likelihoods_dla"], samples["offset_samples"], lognhi,
                                full["min_z_dlas"], full["max_z_dlas"],
                                base_sample_inds=full["base_sample_inds"] if D > 1 else None)
    for key in INTERVAL_KEYS:
        assert _same(full[key], alone[key]), key
    assert full["z_dla_quantiles"].shape == (D, 4, D, 5) and full["lr_counts"].shape == (D, 4)
    assert np.isfinite(full["z_dla_quantiles"][0, :3, 0]).all() and (full["lr_counts"][0, :3] >= 1).all()
    assert np.isnan(full["z_dla_quantiles"][:, 3]).all() and (full["lr_counts"][:, 3] == 0).all()
    q = full["log_nhi_quantiles"][0, :3, 0]
    assert np.all(np.diff(q, axis=1) >= 0) and np.all(np.isin(q, lognhi))
    check(full, full["sample_log_likelihoods_dla"], full["base_sample_inds"] if D > 1 else None, full["min_z_dlas"],
          full["max_z_dlas"], samples["offset_samples"], lognhi, tag=f"engine k={k} D={D}")
    # any split into device batches
    for mb in (1, 3):
        with Engine(model, samples, params, max_batch_spectra=mb) as eng:
            batched = eng.process_intervals(packed, D, lognhi, **kw)
        for key in MULTI_KEYS + SUMMARY_KEYS + INTERVAL_KEYS:
            assert _same(full[key], batched[key]), (mb, key)


# ------------------------------------------------------------------------------- 5. process_qsos
def test_process_qsos_round_trip(tmp_path):
    from gp_dla_detection_amd import catalog as CAT
    from gp_dla_detection_amd import matv73 as M
    from gp_dla_detection_amd import process as PR
    k, D = 20, 3
    model = syn.make_model(k=k)
    samples = syn.make_samples(S_LEVEL)
    packed = syn.pack_spectra(_spectra(model)[:3])
    params = set_parameters(k=k)
    grid = dict(z_edges=Z_EDGES, log_nhi_edges=N_EDGES)
    ivs = dict(levels=(0.16, 0.5, 0.84), lr_delta=1.5)
    without = PR.process_qsos(model, samples, packed, params=params, max_dlas=D, summaries=grid)
    full = PR.process_qsos(model, samples, packed, params=params, max_dlas=D, summaries=grid, intervals=ivs)
    lean = PR.process_qsos(model, samples, packed, params=params, max_dlas=D, summaries=grid, intervals=ivs,
                           save_samples=False)
    for key in without:                     # without the keyword nothing changes, with it nothing else does
        assert _same(without[key], full[key]), key
    assert set(full) - set(without) == set(PR.INTERVAL_VARIABLES)
    for key in lean:
        assert _same(lean[key], full[key]), key
    assert full["z_dla_quantiles"].shape == (3, D, 4, 3) and full["log_nhi_lr_ranges"].shape == (3, D, 4, 2)
    assert full["lr_counts"].shape == (3, D) and full["lr_delta"] == 1.5
    ll = np.transpose(full["sample_log_likelihoods_dla"], (2, 0, 1))
    base = np.transpose(full["base_sample_inds"], (2, 0, 1)).astype(np.int32) - 1
    want = IO.intervals(ll, base, full["min_z_dlas"], full["max_z_dlas"], samples["offset_samples"],
                        samples["log_nhi_samples"], ivs["levels"], ivs["lr_delta"], quantiles=False)
    assert _same(np.swapaxes(want["log_nhi_lr_ranges"], 0, 1), full["log_nhi_lr_ranges"][:, :, :D])
    assert _same(want["lr_counts"].T, full["lr_counts"]) and np.isnan(full["z_dla_means"][:, :, D:]).all()
    lean["test_ind"] = np.ones(3, dtype=bool)
    path = tmp_path / "processed_qsos_intervals.mat"
    PR.save_processed_qsos(str(path), lean)
    r = M.loadmat(str(path))
    for key in PR.INTERVAL_VARIABLES:
        assert _same(np.asarray(r[key]).reshape(np.shape(lean[key])), lean[key]), key
    assert _same(CAT.find_delta_nhi(r), full["log_nhi_lr_ranges"][:, 0, 0, 1] - full["log_nhi_lr_ranges"][:, 0, 0, 0])
    table = CAT.absorber_table(r)
    level = np.argmax(full["model_posteriors"][:, 1:], axis=1)
    assert table["spectrum"].size == int((level + 1).sum()) and table["z_dla_quantiles"].shape[1] == 3
    one = PR.process_qsos(model, samples, packed, params=params, intervals=True)     # max_dlas = 1, implied summaries
    assert one["z_dla_quantiles"].shape == (3, 1, 4, 5) and one["MAP_z_dlas"].shape == (3, 1)
    forest = PR.process_qsos(model, samples, packed, params=params, intervals=True, forest=True)
    assert forest["z_dla_quantiles"].shape == (3, 1, 4, 5) and "num_forest_lines" in forest


# ------------------------------------------------------------------------------------------ 6. errors
def _einval(fn, text, *a, **kw):
    with pytest.raises(L.GpdlaError) as ei:
        fn(*a, **kw)
    assert ei.value.code == L.GPDLA_EINVAL and text in str(ei.value), ei.value


BAD = [(dict(lr_delta=0.0), "lr_delta"), (dict(lr_delta=-1.0), "lr_delta"), (dict(lr_delta=np.inf), "lr_delta"),
       (dict(lr_delta=np.nan), "lr_delta"), (dict(levels=()), "num_levels=0"),
       (dict(levels=np.linspace(0.1, 0.9, 9)), "num_levels=9"), (dict(levels=(0.0, 0.5)), "strictly inside (0, 1)"),
       (dict(levels=(0.5, 1.0)), "strictly inside (0, 1)"), (dict(levels=(0.5, np.nan)), "strictly inside (0, 1)"),
       (dict(levels=(0.5, 0.5)), "strictly increasing"), (dict(levels=(0.6, 0.4)), "strictly increasing")]


def test_argument_errors():
    import ctypes as C
    S = 64
    rng = np.random.default_rng(1)
    ll = rng.normal(size=(2, S))
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)
    args = (ll, offset, log_nhi, [2.0, 2.1], [3.0, 3.1])
    for kw, text in BAD:
        _einval(posterior_intervals, text, *args, **kw)
    _einval(posterior_intervals, "base_inds", np.zeros((2, 2, S)), *args[1:])        # two levels without base indices
    ok = posterior_intervals(*args, levels=np.linspace(0.1, 0.9, 8))
    assert ok["z_dla_quantiles"].shape == (1, 2, 1, 8)
    # null required pointers, straight at the C ABI
    lib = L.load()
    ispec = L.IntervalSpec(log_nhi_samples=L.ptr(log_nhi), lr_delta=2.0, num_levels=1)
    ispec.levels[0] = 0.5
    bufs = {name: np.zeros(2 * 4 * 2) for name, _ in L.Intervals._fields_[1:-1]}
    counts = np.zeros(2, dtype=np.int32)
    zmin, zmax = np.array([2.0, 2.1]), np.array([3.0, 3.1])

    def call(drop=None, spec=True, iv=True):
        fields = {name: L.ptr(b) for name, b in bufs.items()}
        fields["lr_counts"] = L.ptr(counts, C.c_int32)
        if drop:
            fields[drop] = None
        v = L.Intervals(memory=L.MEM_HOST, **fields)
        return lib.gpdla_posterior_intervals_f64(0, L.ptr(ll), 2, S, S, L.ptr(offset), L.ptr(log_nhi), L.ptr(zmin),
                                                 L.ptr(zmax), None, 1, C.byref(ispec) if spec else None,
                                                 C.byref(v) if iv else None)
    assert call() == L.GPDLA_OK
    assert call(spec=False) == L.GPDLA_EINVAL and call(iv=False) == L.GPDLA_EINVAL
    for name, _ in L.Intervals._fields_[1:]:
        assert call(drop=name) == L.GPDLA_EINVAL, name

    model = syn.make_model(k=8)
    samples = syn.make_samples(S)
    packed = syn.pack_spectra([syn.make_spectrum(model, 0, n_target=220)])
    with Engine(model, samples, set_parameters(k=8)) as eng:
        for kw, text in BAD:
            _einval(eng.process_intervals, text, packed, 1, samples["log_nhi_samples"], **kw)
        _einval(eng.process_intervals, "max_dlas", packed, 0, samples["log_nhi_samples"])
        good = eng.process_intervals(packed, 1, samples["log_nhi_samples"])
        assert good["z_dla_quantiles"].shape == (1, 1, 1, 5)

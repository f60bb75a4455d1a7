"""The search cuts on the GPU (csrc/search_cuts.hip, and the sample tests of csrc/row_posterior.h): the kernel
alone against the numpy oracle (search_cuts_oracle.py) -- bitmap, pixel counts and upper ends bitwise, the path
within the bound DESIGN.md section 22 derives --, its independence of batching, the cut reductions against the
oracle at the tile edges of both row tiles, a cut that removes nothing (bitwise the uncut call), and the
argument errors."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import search_cuts_oracle as CO  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd.catalog import absorption_distance  # noqa: E402
from gp_dla_detection_amd.engine import level_planes, population_split_levels, search_cuts  # noqa: E402
from test_gpu_level_population import GRIDS, SPLIT_KEYS, THRESHOLDS, standalone_case  # noqa: E402

pytestmark = pytest.mark.gpu
LYA = 1215.67
BITWISE_KEYS = ("cut_z_uppers", "cut_pixel_counts", "cut_bitmap_offsets", "cut_bitmap_words")
PATH_KEYS = ("cut_path_summary", "cut_path_population")
SETTINGS = {"proximity": (0.1, None), "pixels": (None, 0.25), "both": (0.1, 0.25)}
Z_EDGES_12 = np.linspace(2.0, 4.0, 13)
Z_EDGES_1 = np.array([2.0, 4.0])
COUNTS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1250, 40, 40, 97)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def kernel_case(counts=COUNTS, seed=3):
    """One spectrum per pixel count: n pixels inside the search range with stray out-of-range pixels before,
    among and after them (the compaction has something to skip), noise with one to three noisy stretches; the
    first 40-pixel spectrum is all good, the second noisy at pixel 0 and at pixel n - 1, and the last one's range
    is shorter than the proximity zone.  No noise value lies near the threshold."""
    rng = np.random.default_rng(seed)
    Q = len(counts)
    min_z = 2.0 + 0.05 * rng.random(Q) + 0.03 * np.arange(Q)
    max_z = min_z + 0.8 + 0.6 * rng.random(Q)
    max_z[-1] = min_z[-1] + 0.06
    wl, nv = [], []
    for q, n in enumerate(counts):
        lo, hi = LYA * (1.0 + min_z[q]), LYA * (1.0 + max_z[q])
        inside = lo + (hi - lo) * (np.arange(n) + rng.uniform(0.2, 0.8, n)) / max(n, 1)
        w = np.concatenate([lo - 5.0 + np.arange(3), inside, hi + 1.0 + np.arange(4)])
        stray = rng.integers(3, 3 + n + 1, 5)                              # out-of-range pixels among the others
        w = np.insert(w, stray, rng.choice([lo - 20.0, hi + 20.0, np.nan], stray.size))
        v = rng.uniform(0.01, 0.2, w.size)
        sel = np.flatnonzero((lo < w) & (w < hi))
        assert sel.size == n
        for _ in range(int(rng.integers(1, 4))):
            if n >= 2:
                a = int(rng.integers(0, n - 1))
                v[sel[a:a + int(rng.integers(1, max(2, n // 6)))]] = rng.choice([0.3, 7.0, np.inf, np.nan])
        if q == 13:
            v[sel] = 0.05
        if q == 14:
            v[sel[0]] = v[sel[-1]] = 0.9
        wl.append(w)
        nv.append(v)
    return wl, nv, min_z, max_z


def path_bound(terms, counts, z_edges):
    """the device's X and numpy's each carry at most 7 roundings, so one term differs by
    at most 28 u X(z_hi); the fixed-order sum of k non-negative terms adds (ceil(n / 256) + 10) u of the sum,
    which X(z_hi) bounds.  u = 2^-53, z_hi the upper edge of the interval."""
    e = np.asarray(z_edges, dtype=np.float64)
    top = absorption_distance(np.concatenate([e[1:], e[-1:]]))
    depth = (np.asarray(counts)[:, None] + 255) // 256 + 10
    return (28.0 * terms + depth) * 2.0 ** -53 * top[None, :]


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_kernel_alone(setting):
    pz, nt = SETTINGS[setting]
    wl, nv, min_z, max_z = kernel_case()
    kw = dict(proximity_zone=pz, noise_thresh=nt, z_edges_summary=Z_EDGES_12, z_edges_population=Z_EDGES_1)
    want = CO.search_cuts(wl, nv, min_z, max_z, **kw)
    got = search_cuts(wl, nv, min_z, max_z, **kw)
    assert want["cut_pixel_counts"].tolist() == list(COUNTS)
    for key in BITWISE_KEYS:
        assert got[key].dtype == want[key].dtype and _same(got[key], want[key]), key
    assert math.isnan(got["cut_proximity_zone"]) == (pz is None) and math.isnan(got["cut_noise_thresh"]) == (nt is None)
    if pz is not None:
        assert got["cut_z_uppers"][-1] == min_z[-1] and not got["cut_path_summary"][-1].any()   # the range collapsed
    worst = 0.0
    for key, edges, terms in (("cut_path_summary", Z_EDGES_12, want["terms_summary"]),
                              ("cut_path_population", Z_EDGES_1, want["terms_population"])):
        bound = path_bound(terms, COUNTS, edges)
        err = np.abs(got[key] - want[key])
        worst = max(worst, float((err / bound).max()))
        assert got[key].shape == want[key].shape and np.all(err <= bound), key
        assert np.array_equal(got[key] == 0, want[key] == 0), key
    print(f"{setting}: worst path error / bound {worst:.3f}; terms up to {int(want['terms_summary'].max())}")
    if nt is not None:
        assert want["terms_summary"].max() >= 2 and (want["cut_path_summary"][0] == 0).all()    # n = 0: no path
    # a spectrum's outputs are a function of the spectrum alone: again, alone, and in another batch order
    again = search_cuts(wl, nv, min_z, max_z, **kw)
    order = np.random.default_rng(1).permutation(len(wl))
    mixed = search_cuts([wl[q] for q in order], [nv[q] for q in order], min_z[order], max_z[order], **kw)
    for key in BITWISE_KEYS[:2] + PATH_KEYS:
        assert _same(again[key], got[key]) and _same(mixed[key], got[key][order]), key
    assert _same(again["cut_bitmap_words"], got["cut_bitmap_words"])
    for q in (0, 3, 12, 14):
        one = search_cuts([wl[q]], [nv[q]], min_z[q:q + 1], max_z[q:q + 1], **kw)
        for key in BITWISE_KEYS[:2] + PATH_KEYS:
            assert _same(one[key], got[key][q:q + 1]), (key, q)
        o = got["cut_bitmap_offsets"]
        assert _same(one["cut_bitmap_words"], got["cut_bitmap_words"][o[q]:o[q + 1]])


def test_kernel_edge_values():
    """What the reference cannot run: NaN noise and noise equal to the threshold are bad, a NaN range selects
    nothing, span = 0 selects nothing (both bounds strict), n = 1 gives the all-good form or nothing."""
    lo, hi = LYA * 3.0, LYA * 4.0
    w5 = lo + (hi - lo) * (np.arange(5) + 0.5) / 5
    wl = [w5, w5, w5, np.array([lo - 1.0, 0.5 * (lo + hi), hi + 1.0]), np.array([lo - 1.0, 0.5 * (lo + hi), hi + 1.0]), w5]
    nv = [np.array([np.nan, 0.25, 0.1, 0.2, np.inf]), np.full(5, 0.1), np.full(5, 0.1), np.array([0.0, 0.1, 0.0]),
          np.array([0.0, 0.3, 0.0]), np.full(5, 0.1)]
    min_z = np.array([2.0, np.nan, 2.5, 2.0, 2.0, 2.0])
    max_z = np.array([3.0, 3.0, 2.5, 3.0, 3.0, np.nan])
    kw = dict(proximity_zone=0.1, noise_thresh=0.25, z_edges_summary=Z_EDGES_1)
    want = CO.search_cuts(wl, nv, min_z, max_z, **kw)
    got = search_cuts(wl, nv, min_z, max_z, **kw)
    assert want["cut_pixel_counts"].tolist() == [5, 0, 0, 1, 1, 0]
    assert want["goods"][0].tolist() == [False, False, True, True, False]
    for key in BITWISE_KEYS:
        assert _same(got[key], want[key]), key
    assert np.all(np.abs(got["cut_path_summary"] - want["cut_path_summary"]) <= path_bound(want["terms_summary"],
                                                                                            [5, 0, 0, 1, 1, 0], Z_EDGES_1))
    assert np.array_equal(got["cut_path_summary"] == 0, [[False] * 2, [True] * 2, [True] * 2, [False] * 2, [True] * 2, [True] * 2])


def reduction_cuts(c, setting, seed=0):
    """Spectra for the rows of a ``standalone_case`` and their cuts, by the oracle."""
    rng = np.random.default_rng(77 + seed)
    R = len(c["min_z"])
    counts = [1250, 33, 0, 64, 257, 2][:R]
    wl, nv = [], []
    for r in range(R):
        lo, hi = LYA * (1.0 + c["min_z"][r]), LYA * (1.0 + c["max_z"][r])
        n = counts[r]
        wl.append(np.concatenate([[lo - 3.0], lo + (hi - lo) * (np.arange(n) + 0.5) / max(n, 1), [hi + 3.0]]))
        v = rng.uniform(0.01, 0.2, n + 2)
        v[rng.random(n + 2) < 0.15] = 0.6
        if n >= 64:
            a = int(rng.integers(1, n // 2))
            v[a:a + n // 5] = np.nan
        nv.append(v)
    pz, nt = SETTINGS[setting]
    return CO.search_cuts(wl, nv, c["min_z"], c["max_z"], pz, nt)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("S", [1, 255, 256, 257, 513])
def test_cut_reductions_against_the_oracle(S, setting):
    c = standalone_case(S)
    ez, en = GRIDS["7x5"]
    nhi = 10.0 ** c["log_nhi"]
    cuts = reduction_cuts(c, setting)
    dz, di = CO.margins(cuts, c["min_z"], c["max_z"], c["offset"])
    print(f"S={S} {setting}: closest z to z_upper {dz:.2e}, closest pixel coordinate to an integer {di:.2e}")
    assert dz > 1e-9 and di > 1e-9        # a condition on the inputs: rounding decides no membership
    want_planes, count = CO.level_planes(cuts, c["ll"], c["base"], c["min_z"], c["max_z"], c["offset"], c["log_nhi"], nhi, ez, en)
    want_split = CO.level_split(cuts, c["ll"], c["base"], c["min_z"], c["max_z"], c["P"], c["offset"], c["log_nhi"], ez, en,
                                **THRESHOLDS)
    uncut = level_planes(c["ll"], c["offset"], c["log_nhi"], nhi, c["min_z"], c["max_z"], ez, en, base_sample_inds=c["base"])
    worst = 0.0
    for levels in (1, 2, 3, 4):
        ll, base, P = c["ll"][:levels], c["base"][:levels - 1] if levels > 1 else None, c["P"][:levels]
        planes = level_planes(ll, c["offset"], c["log_nhi"], nhi, c["min_z"], c["max_z"], ez, en, base_sample_inds=base, cuts=cuts)
        split = population_split_levels(ll, c["offset"], c["log_nhi"], c["min_z"], c["max_z"], P, ez, en,
                                        base_sample_inds=base, cuts=cuts, **THRESHOLDS)
        assert np.array_equal(split["population_level_large_inds"], want_split["population_level_large_inds"][:, :levels])
        assert np.array_equal(split["population_level_large_bins"], want_split["population_level_large_bins"][:, :levels])
        for d in range(levels):
            tol = ((d + 1) * S + 16) * 2.0 ** -52          # test_gpu_level_population's bound
            for got, want in ((planes[:, d], want_planes[:, d]),
                              (split["population_level_poisson"][:, d], want_split["population_level_poisson"][:, d]),
                              (split["population_level_large_probs"][:, d], want_split["population_level_large_probs"][:, d])):
                assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0, want == 0)   # membership
                ok = ~np.isnan(want) & (want != 0)
                if ok.any():
                    rel = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
                    worst = max(worst, float(rel.max() / tol))
                    assert np.all(rel <= tol), (levels, d)
    print(f"S={S} {setting}: worst error / bound {worst:.3f}")
    assert not planes[2].any() or SETTINGS[setting][1] is None      # the row without pixels keeps nothing under the pixel cut
    if S >= 255:
        assert 0 < (planes[:, :, 0] > 0).sum() and (planes[:, :, 0] != uncut[:, :, 0]).any()   # the cut removed mass
    # rows are independent of their launch
    part = level_planes(ll[:, 2:], c["offset"], c["log_nhi"], nhi, c["min_z"][2:], c["max_z"][2:], ez, en,
                        base_sample_inds=base[:, 2:], cuts=_rows_from(cuts, 2))
    assert _same(part, planes[2:])


def _rows_from(cuts, r0):
    """The cuts of rows r0 .. of a dict, with the bitmap offsets starting at 0 again."""
    o = np.asarray(cuts["cut_bitmap_offsets"])
    out = dict(cuts)
    out.update(cut_z_uppers=cuts["cut_z_uppers"][r0:], cut_pixel_counts=cuts["cut_pixel_counts"][r0:],
               cut_bitmap_offsets=o[r0:] - o[r0], cut_bitmap_words=cuts["cut_bitmap_words"][o[r0]:])
    return out


@pytest.mark.parametrize("S", [1, 256, 513])
def test_a_cut_that_removes_nothing_is_the_uncut_call(S):
    c = standalone_case(S)
    ez, en = GRIDS["7x5"]
    nhi = 10.0 ** c["log_nhi"]
    R = len(c["min_z"])
    wl = [LYA * (1.0 + np.linspace(c["min_z"][r], c["max_z"][r], 40 + r)[1:-1]) for r in range(R)]
    nv = [np.full(w.size, 1e30) for w in wl]
    cuts = search_cuts(wl, nv, c["min_z"], c["max_z"], proximity_zone=0.0, noise_thresh=math.inf)
    assert _same(cuts["cut_z_uppers"], c["max_z"]) and (cuts["cut_pixel_counts"] == [38 + r for r in range(R)]).all()
    want_planes = level_planes(c["ll"], c["offset"], c["log_nhi"], nhi, c["min_z"], c["max_z"], ez, en, base_sample_inds=c["base"])
    want_split = population_split_levels(c["ll"], c["offset"], c["log_nhi"], c["min_z"], c["max_z"], c["P"], ez, en,
                                         base_sample_inds=c["base"], **THRESHOLDS)
    planes = level_planes(c["ll"], c["offset"], c["log_nhi"], nhi, c["min_z"], c["max_z"], ez, en, base_sample_inds=c["base"],
                          cuts=cuts)
    split = population_split_levels(c["ll"], c["offset"], c["log_nhi"], c["min_z"], c["max_z"], c["P"], ez, en,
                                    base_sample_inds=c["base"], cuts=cuts, **THRESHOLDS)
    assert _same(planes, want_planes)
    for key in SPLIT_KEYS:
        assert _same(split[key], want_split[key]), key


def test_argument_errors():
    lib = L.load()
    w = np.linspace(3700.0, 4800.0, 40)
    v = np.full(40, 0.1)
    off = np.array([0, 40], dtype=np.int64)
    zmin, zmax = np.array([2.1]), np.array([2.9])
    e = np.array([2.0, 3.0, 4.0])
    i64, i32, u32 = C.c_int64, C.c_int32, C.c_uint32

    def call(Q=1, offsets=off, pz=0.1, nt=0.25, om=0.279, nzs=2, es=e, nzp=0, ep=None, path_s=True, path_p=False,
             memory=L.MEM_HOST, words=True):
        zu, cnt, wo, ww = np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros(3, dtype=np.int64), np.zeros(4, dtype=np.uint32)
        ps, pp = np.zeros((2, 3)), np.zeros((2, 3))
        spec = L.SearchCuts(proximity_zone=pz, noise_thresh=nt, omega_m=om, num_z_bins_summary=nzs, z_edges_summary=L.ptr(es),
                            num_z_bins_population=nzp, z_edges_population=L.ptr(ep))
        res = L.SearchCutResults(memory=memory, z_uppers=L.ptr(zu), pixel_counts=L.ptr(cnt, i32), bitmap_offsets=L.ptr(wo, i64),
                                 bitmap_words=L.ptr(ww, u32) if words else None, path_summary=L.ptr(ps) if path_s else None,
                                 path_population=L.ptr(pp) if path_p else None)
        return lib.gpdla_search_cuts_f64(0, Q, L.ptr(offsets, i64), L.ptr(w), L.ptr(v), L.ptr(zmin), L.ptr(zmax), C.byref(spec),
                                         C.byref(res))
    assert call() == L.GPDLA_OK
    nan = math.nan
    bad = [dict(Q=0), dict(offsets=np.array([1, 40], dtype=np.int64)), dict(offsets=np.array([0, -1], dtype=np.int64)),
           dict(pz=nan, nt=nan), dict(pz=-0.1), dict(pz=math.inf), dict(om=0.0), dict(om=1.5), dict(om=nan),
           dict(es=np.array([2.0, 2.0, 4.0])), dict(es=np.array([2.0, nan, 4.0])), dict(es=None), dict(nzs=-1), dict(nzs=2000),
           dict(path_s=False), dict(path_p=True), dict(nzp=2, ep=e), dict(memory=L.MEM_DEVICE), dict(words=False)]
    for kw in bad:
        assert call(**kw) == L.GPDLA_EINVAL, kw
        assert b"search cuts" in lib.gpdla_last_error()
    assert call(nzp=2, ep=e, path_p=True) == L.GPDLA_OK and call(pz=nan) == L.GPDLA_OK and call(nt=nan) == L.GPDLA_OK
    assert call(nzs=0, es=None, path_s=False, om=nan) == L.GPDLA_OK                 # omega_m is read only with a grid

    # the cut reductions
    c = standalone_case(4)
    ez, en = GRIDS["7x5"]
    R = len(c["min_z"])
    good = dict(cut_proximity_zone=0.1, cut_noise_thresh=0.25, cut_z_uppers=c["max_z"] - 0.1,
                cut_pixel_counts=np.full(R, 32, dtype=np.int32), cut_bitmap_offsets=np.arange(R + 1, dtype=np.int64),
                cut_bitmap_words=np.full(R, 0xFFFFFFFF, dtype=np.uint32))
    args = (c["ll"][:1], c["offset"], c["log_nhi"], 10.0 ** c["log_nhi"], c["min_z"], c["max_z"], ez, en)
    level_planes(*args, cuts=good)
    for change in (dict(cut_proximity_zone=nan, cut_noise_thresh=nan),                        # neither test
                   dict(cut_pixel_counts=np.full(R, 33, dtype=np.int32)),                     # more pixels than bits
                   dict(cut_pixel_counts=np.full(R, -1, dtype=np.int32)),
                   dict(cut_bitmap_offsets=np.arange(1, R + 2, dtype=np.int64)),              # not from 0
                   dict(cut_bitmap_offsets=np.array([0, 3] + list(range(2, R + 1)), dtype=np.int64))):   # descending
        with pytest.raises(L.GpdlaError) as ei:
            level_planes(*args, cuts={**good, **change})
        assert ei.value.code == L.GPDLA_EINVAL, change
        with pytest.raises(L.GpdlaError) as ei:
            population_split_levels(args[0], c["offset"], c["log_nhi"], c["min_z"], c["max_z"], c["P"][:1], ez, en,
                                    cuts={**good, **change}, **THRESHOLDS)
        assert ei.value.code == L.GPDLA_EINVAL, change


# ------------------------------------------------------------------- the engine and process_qsos
from gp_dla_detection_amd import catalog as CAT  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import Engine  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402
from test_gpu_population import P_EDGES_N, P_EDGES_Z  # noqa: E402

S_CUT, Q_CUT = 300, 8
GRID = dict(z_edges=np.linspace(2.0, 4.0, 4), log_nhi_edges=np.linspace(20.0, 23.0, 3))
GRID_KEYS = ("bin_planes", "population_poisson", "population_large_inds", "population_large_probs", "population_large_bins",
             "bin_planes_levels", "population_level_poisson", "population_level_large_inds", "population_level_large_probs",
             "population_level_large_bins")
CUT_KEYS = ("cut_proximity_zone", "cut_noise_thresh") + BITWISE_KEYS + PATH_KEYS


def synthetic_set():
    k = 4
    model = syn.make_model(k=k)
    samples = syn.make_samples(S_CUT)
    spectra = [syn.make_spectrum(model, i, z_qso=(2.6, 3.1, 2.8, 3.4, 2.9, 3.6, 2.5, 3.2)[i],
                                 n_target=(300, None, 270, 290, 280, 310, 260, 300)[i], mask_fraction=0.05)
               for i in range(Q_CUT)]
    packed = syn.pack_spectra(spectra)
    nv = np.sort(np.asarray(packed["noise_variance"], dtype=np.float64))
    thresh = 0.5 * (nv[(3 * nv.size) // 4] + nv[(3 * nv.size) // 4 + 1])      # a quarter of the pixels are noisy
    assert not np.any(np.abs(nv - thresh) <= 1e-9 * thresh)
    return model, samples, packed, set_parameters(k=k), thresh


def cells_of(packed):
    o = np.asarray(packed["offsets"])
    return ([np.asarray(packed["wavelengths"])[a:b] for a, b in zip(o[:-1], o[1:])],
            [np.asarray(packed["noise_variance"])[a:b] for a, b in zip(o[:-1], o[1:])])


@pytest.mark.parametrize("D", [1, 2])
def test_engine_cuts(D):
    model, samples, packed, params, thresh = synthetic_set()
    lognhi, S, Q = samples["log_nhi_samples"], S_CUT, Q_CUT
    rng = np.random.default_rng(60 + D)
    forced = rng.integers(0, S, (D - 1, Q, S)).astype(np.int32)
    forced[rng.random(forced.shape) < 0.05] = -1
    cuts = dict(proximity_zone=0.1, noise_thresh=thresh)
    with Engine(model, samples, params) as eng:
        first = eng.process_multi(packed, D, base_sample_inds=forced)
        lp_dla = np.stack([first["log_likelihoods_no_dla"] - np.nan_to_num(first["log_likelihoods_dla"][d]) - 0.4 * d
                           for d in range(D)])
        pop = dict(z_edges=P_EDGES_Z, log_nhi_edges=P_EDGES_N, log_nhi_samples=lognhi, log_priors_no_dla=np.full(Q, -0.25),
                   log_priors_dla=lp_dla)
        kw = dict(population=pop, base_sample_inds=forced, log_nhi_samples=lognhi, **GRID)
        plain = eng.process_levels(packed, D, **kw)
        null = eng.process_cuts(packed, D, cuts=None, levels=None, **kw)        # both cut pointers NULL
        assert list(plain) == list(null) and all(_same(plain[key], null[key]) for key in plain)
        eng.reset_stats()
        full = eng.process_cuts(packed, D, cuts=cuts, levels=None, **kw)
        stats = eng.cut_stats()
        repeat = eng.process_cuts(packed, D, cuts=cuts, levels=None, **kw)
        lean = eng.process_cuts(packed, D, cuts=cuts, levels=None, want_samples=False, **kw)
        dev = eng.process_cuts(packed, D, cuts=cuts, levels=None, memory="device", **kw)
        first_only = eng.process_cuts(packed, D, cuts=cuts, **kw)                 # levels=(): the level-1 reductions alone
        prox_only = eng.process_cuts(packed, D, cuts=dict(proximity_zone=0.1, noise_thresh=None), levels=None, **kw)
        with pytest.raises(ValueError):
            eng.process_cuts(packed, D, cuts=dict(proximity_zone=None, noise_thresh=None), **kw)
        with pytest.raises(ValueError):
            eng.process_cuts(packed, D, cuts=cuts, base_sample_inds=forced)      # no grid to cut
        with pytest.raises(L.GpdlaError) as ei:
            eng.process_cuts(packed, D, cuts=cuts, **dict(kw, population=dict(pop, z_edges=P_EDGES_Z[::-1].copy())))
        assert ei.value.code == L.GPDLA_EINVAL
    assert stats["cut_launches"] == 1 and stats["cut_ms"] > 0
    assert set(full) - set(plain) == set(CUT_KEYS)
    for key in plain:                                   # everything that is not a grid reduction is unchanged
        assert key in GRID_KEYS or _same(plain[key], full[key]), key
    for key in ("bin_planes", "population_poisson", "bin_planes_levels", "population_level_poisson"):
        assert not _same(plain[key], full[key]), key
    for other in (repeat, lean, dev):
        for key in other:
            assert _same(full[key], other[key]), key
    for key in first_only:
        assert _same(full[key], first_only[key]), key
    assert math.isnan(prox_only["cut_noise_thresh"]) and _same(prox_only["cut_z_uppers"], full["cut_z_uppers"])
    # the cut variables are the stand-alone kernel's on the same pixels and the ranges the engine reports
    wl, nv = cells_of(packed)
    alone = search_cuts(wl, nv, full["min_z_dlas"], full["max_z_dlas"], z_edges_summary=GRID["z_edges"],
                        z_edges_population=P_EDGES_Z, **cuts)
    for key in BITWISE_KEYS + PATH_KEYS:
        assert _same(full[key], alone[key]), key
    assert (full["cut_pixel_counts"] > 100).all() and (full["cut_path_summary"][:, -1] > 0).all()
    # ... and the grid reductions are the stand-alone cut reductions on the rows the run returned
    rows, base, P = full["sample_log_likelihoods_dla"], full["base_sample_inds"], full["population_level_posteriors"]
    args = (samples["offset_samples"], lognhi)
    zr = (full["min_z_dlas"], full["max_z_dlas"])
    planes = level_planes(rows, *args, samples["nhi_samples"], *zr, GRID["z_edges"], GRID["log_nhi_edges"],
                          base_sample_inds=base, cuts=alone)
    assert _same(full["bin_planes_levels"], planes) and _same(full["bin_planes"], planes[:, 0])
    split = population_split_levels(rows, *args, *zr, P, P_EDGES_Z, P_EDGES_N, base_sample_inds=base, cuts=alone)
    for key in SPLIT_KEYS:
        assert _same(full[key], split[key]), key
    one = population_split_levels(rows[:1], *args, *zr, full["population_p_dlas"][None], P_EDGES_Z, P_EDGES_N, cuts=alone)
    assert _same(full["population_poisson"], one["population_level_poisson"][:, 0])
    assert _same(full["population_large_inds"], one["population_level_large_inds"][:, 0])
    assert _same(full["population_large_probs"], one["population_level_large_probs"][:, 0])
    assert _same(full["population_large_bins"], one["population_level_large_bins"][:, 0, :, 0])
    # ... which the oracle gives from the uncut run's sample arrays
    want_cuts = CO.search_cuts(wl, nv, *zr, z_edges_summary=GRID["z_edges"], **cuts)
    # (the synthetic offsets are dyadic, so pixel coordinates do land on integers; both sides form them with the
    # same correctly rounded operations, and the membership test below would show a disagreement)
    want, _ = CO.level_planes(want_cuts, plain["sample_log_likelihoods_dla"], plain["base_sample_inds"], *zr, *args,
                              samples["nhi_samples"], GRID["z_edges"], GRID["log_nhi_edges"])
    assert np.array_equal(want == 0, planes == 0) and (planes[:, :, 0].sum() < plain["bin_planes_levels"][:, :, 0].sum())
    nzm = want != 0
    assert np.all(np.abs(planes[nzm] - want[nzm]) <= (D * S + 16) * 2.0 ** -52 * np.abs(want[nzm]))
    # ... the split likewise: the same samples in the lists, the same bins, masses within the bound
    want_split = CO.level_split(want_cuts, plain["sample_log_likelihoods_dla"], plain["base_sample_inds"], *zr, P, *args,
                                P_EDGES_Z, P_EDGES_N)
    assert _same(split["population_level_large_inds"], want_split["population_level_large_inds"])
    assert _same(split["population_level_large_bins"], want_split["population_level_large_bins"])
    for key in ("population_level_poisson", "population_level_large_probs"):
        got_v, want_v = split[key], want_split[key]
        assert np.array_equal(np.isnan(got_v), np.isnan(want_v)) and np.array_equal(got_v == 0, want_v == 0), key
        okv = ~np.isnan(want_v) & (want_v != 0)
        assert np.all(np.abs(got_v[okv] - want_v[okv]) <= (D * S + 16) * 2.0 ** -52 * np.abs(want_v[okv])), key
    # any split into device batches
    for batch in (1, 3):
        with Engine(model, samples, params, max_batch_spectra=batch) as eng:
            batched = eng.process_cuts(packed, D, cuts=cuts, levels=None, **kw)
            assert eng.cut_stats()["cut_launches"] == -(-Q // batch)
        for key in full:
            assert _same(full[key], batched[key]), (key, batch)


@pytest.mark.parametrize("D,levels", [(1, "first"), (2, "first"), (2, "all")])
def test_process_qsos_cuts(D, levels, tmp_path):
    model, samples, packed, params, thresh = synthetic_set()
    rng = np.random.default_rng(3)
    prior = dict(z_qsos=rng.uniform(2.0, 4.5, 400), dla_ind=rng.uniform(size=400) < 0.12)
    lv = dict(levels="all") if levels == "all" else {}
    kw = dict(params=params, max_dlas=D, summaries=dict(GRID, **lv), population=dict(z_edges=P_EDGES_Z, log_nhi_edges=P_EDGES_N, **lv))
    cuts = dict(proximity_zone=0.1, noise_thresh=thresh)
    plain = PR.process_qsos(model, samples, packed, prior, **kw)
    cut = PR.process_qsos(model, samples, packed, prior, cuts=cuts, **kw)
    lean = PR.process_qsos(model, samples, packed, prior, cuts=cuts, save_samples=False, **kw)
    assert set(cut) - set(plain) == set(PR.CUT_VARIABLES)
    grid_keys = set(GRID_KEYS)
    for key in plain:
        assert key in grid_keys or _same(plain[key], cut[key]), key
    assert not _same(plain["bin_planes"], cut["bin_planes"]) and not _same(plain["population_poisson"], cut["population_poisson"])
    assert "sample_log_likelihoods_dla" not in lean
    for key in lean:
        assert _same(lean[key], cut[key]), key
    # the stored path is the oracle's, and the catalog functions use it
    wl, nv = cells_of(packed)
    want = CO.search_cuts(wl, nv, cut["min_z_dlas"], cut["max_z_dlas"], z_edges_summary=GRID["z_edges"],
                          z_edges_population=P_EDGES_Z, **cuts)
    counts = want["cut_pixel_counts"]
    assert _same(lean["cut_z_uppers"], want["cut_z_uppers"]) and _same(lean["cut_pixel_counts"], counts.astype(np.float64))
    for name, edges in (("summary", GRID["z_edges"]), ("population", P_EDGES_Z)):
        assert np.all(np.abs(lean["cut_path_" + name] - want["cut_path_" + name]) <= path_bound(want["terms_" + name], counts, edges))
    # the grid reductions are the oracle's on the uncut run's sample arrays, and no batching changes a bit
    rows = np.asarray(plain["sample_log_likelihoods_dla"], dtype=np.float64)
    rows = rows[None] if D == 1 else np.ascontiguousarray(np.transpose(rows, (2, 0, 1)))
    base = None
    if D > 1:      # Q x S for D = 2 (MATLAB drops the trailing singleton), Q x S x (D - 1) beyond
        b = np.asarray(plain["base_sample_inds"]).reshape(Q_CUT, S_CUT, D - 1)
        base = np.ascontiguousarray(np.transpose(b, (2, 0, 1))).astype(np.int64) - 1
    zr = (cut["min_z_dlas"], cut["max_z_dlas"])
    sm = (samples["offset_samples"], samples["log_nhi_samples"])
    want_planes = CO.level_planes(want, rows, base, *zr, *sm, samples["nhi_samples"], GRID["z_edges"], GRID["log_nhi_edges"])[0]
    P = np.asarray(cut["population_level_posteriors"]).T if levels == "all" else np.asarray(cut["population_p_dlas"])[None]
    nl = D if levels == "all" else 1
    want_split = CO.level_split(want, rows[:nl], None if nl == 1 else base, *zr, P, *sm, P_EDGES_Z, P_EDGES_N)
    pairs = [(lean["bin_planes"], want_planes[:, 0])]
    if levels == "all":
        pairs += [(lean["bin_planes_levels"], want_planes), (lean["population_level_poisson"], want_split["population_level_poisson"])]
        assert _same(lean["population_level_large_inds"], want_split["population_level_large_inds"].astype(np.float64) + 1.0)
        assert _same(lean["population_level_large_bins"], want_split["population_level_large_bins"].astype(np.float64) + 1.0)
    else:
        pairs += [(lean["population_poisson"], want_split["population_level_poisson"][:, 0])]
        assert _same(lean["population_large_inds"], want_split["population_level_large_inds"][:, 0].astype(np.float64) + 1.0)
        assert _same(lean["population_large_bins"], want_split["population_level_large_bins"][:, 0, :, 0].astype(np.float64) + 1.0)
    for got_v, want_v in pairs:
        assert got_v.shape == want_v.shape and np.array_equal(got_v == 0, want_v == 0)
        okv = want_v != 0
        assert np.all(np.abs(got_v[okv] - want_v[okv]) <= (D * S_CUT + 16) * 2.0 ** -52 * np.abs(want_v[okv]))
    for batch in (1, 3):
        with Engine(model, samples, params, max_batch_spectra=batch) as eng:
            batched = PR.process_qsos(model, samples, packed, prior, cuts=cuts, save_samples=False, engine=eng, **kw)
        for key in lean:
            assert _same(lean[key], batched[key]), (key, batch)
    z, dndx, l68, l95, _ = CAT.line_density(lean, levels=levels)
    zp, dndx_p = CAT.line_density(plain, levels=levels)[:2]
    path = np.array([math.fsum(lean["cut_path_population"][:, c]) for c in range(P_EDGES_Z.size - 1)])
    counts_z = CAT.confidence_intervals(lean, axis="z", levels=levels)[0]
    assert _same(dndx, (counts_z / np.where(path > 0, path, np.nan))[path > 0]) and z.size >= 3 and _same(z, zp)
    uncut_path = np.array([CAT.path_length(a, b, plain["min_z_dlas"], plain["max_z_dlas"]) for a, b in zip(P_EDGES_Z[:-1], P_EDGES_Z[1:])])
    assert np.all(path <= uncut_path) and path.sum() < 0.9 * uncut_path.sum()
    keep = np.arange(Q_CUT) % 2 == 0
    cent, f = CAT.column_density_function(lean, keep=keep, levels=levels)[:2]
    assert np.all(np.isfinite(f)) and _same(CAT.cut_path_columns(lean, "population", keep)[~keep], np.zeros((4, P_EDGES_Z.size)))
    om = CAT.omega_dla(lean, levels=levels)
    assert np.all(om[1][np.isfinite(om[1])] >= 0) and np.isfinite(om[1]).any()
    with pytest.raises(ValueError):
        CAT.line_density(lean, omega_m=0.3)             # the stored path is for the run's omega_m
    # the file round trip
    PR.save_processed_qsos(str(tmp_path / "cut.mat"), lean)
    from gp_dla_detection_amd.matv73 import loadmat
    back = loadmat(str(tmp_path / "cut.mat"))
    for key in PR.CUT_VARIABLES:
        assert _same(np.asarray(back[key], dtype=np.float64).reshape(np.shape(lean[key])), lean[key]), key
    # keyword errors
    for bad in (dict(cuts=dict(proximity_zone=None, noise_thresh=None)), dict(cuts=dict(zone=0.1)), dict(cuts=cuts, intervals=True),
                dict(cuts=cuts, sub_dla=True), dict(cuts=dict(proximity_zone=-1.0))):
        with pytest.raises(ValueError):
            PR.process_qsos(model, samples, packed, prior, **dict(kw, **bad))
    with pytest.raises(ValueError):
        PR.process_qsos(model, samples, packed, prior, params=params, cuts=cuts)    # no grid, no population


def test_engine_cut_argument_errors():
    """Every GPDLA_EINVAL / GPDLA_EUNSUPPORTED case of gpdla_engine_process_cuts: the struct checks come before
    anything is read, so empty spectra / result structs serve."""
    model = syn.make_model(k=4)
    samples = syn.make_samples(64)
    packed = syn.pack_spectra([syn.make_spectrum(model, 0, n_target=220)])
    lognhi = samples["log_nhi_samples"]
    pop = dict(z_edges=P_EDGES_Z, log_nhi_edges=P_EDGES_N, log_nhi_samples=lognhi, log_priors_no_dla=[-0.1],
               log_priors_dla=[-2.3])
    cuts = dict(proximity_zone=0.1, noise_thresh=0.05)
    lib = L.load()
    params = set_parameters(k=4)
    for path in ("fused_i8", "panel_gemm", "panel_gemm_i8"):
        with Engine(model, samples, params, path=path) as eng:
            with pytest.raises(L.GpdlaError) as ei:
                eng.process_cuts(packed, 1, cuts=cuts, population=pop)
            assert ei.value.code == L.GPDLA_EUNSUPPORTED, path
    e2 = np.array([2.0, 3.0, 4.0])
    buf, ibuf, wbuf, obuf = np.zeros(8), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.int64)
    with Engine(model, samples, params) as eng:
        assert eng.process_cuts(packed, 1, cuts=cuts, population=pop)["cut_path_population"].shape == (1, 8)
        sp, md, rs, sm = L.Spectra(), L.MultiDla(), L.ResultsMulti(), L.Summaries()
        ss = L.SummarySpec(log_nhi_samples=L.ptr(lognhi), num_z_bins=2, num_nhi_bins=1, z_edges=L.ptr(e2),
                           log_nhi_edges=L.ptr(np.array([20.0, 23.0])))

        def call(spec=None, res=None, summary=True, sub=False, **over):
            c = dict(proximity_zone=0.1, noise_thresh=0.05, omega_m=0.279, num_z_bins_summary=2, z_edges_summary=L.ptr(e2),
                     num_z_bins_population=0, z_edges_population=None)
            r = dict(memory=L.MEM_HOST, z_uppers=L.ptr(buf), pixel_counts=L.ptr(ibuf, C.c_int32),
                     bitmap_offsets=L.ptr(obuf, C.c_int64), bitmap_words=L.ptr(wbuf, C.c_uint32), path_summary=L.ptr(buf),
                     path_population=None)
            c.update({k: v for k, v in over.items() if k in c})
            r.update({k: v for k, v in over.items() if k in r})
            cs = L.SearchCuts(**c) if spec is None else spec
            cr = L.SearchCutResults(**r) if res is None else res
            return lib.gpdla_engine_process_cuts(
                eng._h, C.byref(sp), C.byref(md), C.byref(L.SubDla()) if sub else None, C.byref(rs),
                C.byref(L.ResultsSub()) if sub else None, C.byref(ss) if summary else None, C.byref(sm) if summary else None,
                None, None, None, C.byref(cs) if cs is not False else None, C.byref(cr) if cr is not False else None)
        nan = math.nan
        for kw in (dict(spec=False), dict(res=False),                                   # one of the two NULL
                   dict(memory=7), dict(z_uppers=None), dict(pixel_counts=None), dict(bitmap_offsets=None), dict(bitmap_words=None),
                   dict(path_summary=None),                                             # a grid without its path array
                   dict(path_population=L.ptr(buf)),                                    # a path array without its grid
                   dict(proximity_zone=nan, noise_thresh=nan), dict(proximity_zone=-0.5), dict(omega_m=0.0),
                   dict(z_edges_summary=L.ptr(e2[::-1].copy())), dict(num_z_bins_summary=-1),
                   dict(summary=False)):                                                # no grid to cut
            assert call(**kw) == L.GPDLA_EINVAL, kw
        assert call(sub=True) == L.GPDLA_EUNSUPPORTED
        assert b"sub-DLA" in lib.gpdla_last_error()


# ------------------------------------------------------------------- the golden fixture on the device
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_golden_fixture_on_the_device(setting):
    """tests/golden/search_cuts.npz (the reference's DLACatalogue under lowzcut, filter_noisy_pixels and both) through
    the device kernel, the device reductions and catalog.py: the reference's lists, interval integers and curves are
    met as test_search_cuts.py meets them with the oracle."""
    import test_population as TP
    import test_search_cuts as TC
    g = np.load(TC.GOLDEN)
    wl, nv = TC.fixture_spectra(g)
    want = TC.fixture_cuts(g, setting)
    pz, nt = (None if math.isnan(want[k]) else want[k] for k in ("cut_proximity_zone", "cut_noise_thresh"))
    cuts = search_cuts(wl, nv, g["min_z_dlas"], g["max_z_dlas"], pz, nt, z_edges_summary=g["z_edges"], z_edges_population=g["z_edges"])
    for key in BITWISE_KEYS:
        assert _same(cuts[key], want[key]), key
    ll = g["sample_log_likelihoods"][None]
    args = (g["offset_samples"], g["log_nhi_samples"])
    zr = (g["min_z_dlas"], g["max_z_dlas"])
    split = population_split_levels(ll, *args, *zr, g["p_dlas"][None], g["z_edges"], g["log_nhi_edges"], cuts=cuts)
    planes = level_planes(ll, *args, g["nhi_samples"], *zr, g["z_edges"], g["log_nhi_edges"], cuts=cuts)
    out = TC.cut_out(g, cuts, split, planes)
    ref = TC.reference_view(g, setting)
    TP.check_split_against_reference(ref, out)
    TC.check_cut_curves(ref, out, want, None)             # pmf=None: the device pmf

"""The search cuts on the CPU (no GPU): the numpy restatement (search_cuts_oracle.py) against the rules of
include/gpdla.h "Search cuts" worked by hand -- the pixel selection, the good flags at NaN / +inf / equality, the
upper end under the proximity cut, the sample tests, and the path as a sum over run starts -- and the Python
wrappers' argument checks."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import level_population_oracle as LO  # noqa: E402
import search_cuts_oracle as CO  # noqa: E402
from gp_dla_detection_amd import engine as E  # noqa: E402
from gp_dla_detection_amd.catalog import absorption_distance  # noqa: E402

LYA = 1215.67


def X(z):
    return float(absorption_distance(z))


def spectrum(min_z, max_z, n, below=2, above=3):
    """n pixels strictly inside the search range, `below` / `above` outside it on either side."""
    lo, hi = LYA * (1.0 + min_z), LYA * (1.0 + max_z)
    inside = lo + (hi - lo) * (np.arange(n) + 0.5) / max(n, 1)
    return np.concatenate([lo - 1.0 - np.arange(below)[::-1], inside, hi + 1.0 + np.arange(above)])


def test_selection_is_strict_and_in_pixel_order():
    min_z, max_z = 2.0, 3.0
    lo, hi = LYA * 3.0, LYA * 4.0
    w = np.array([lo, lo + 1.0, hi - 1.0, hi, lo + 2.0, np.nan])      # both bounds strict; order is pixel order
    v = np.array([0.0, 0.1, 0.3, 0.0, 0.2, 0.0])
    good, zu = CO.spectrum_cut(w, v, min_z, max_z, None, 0.25)
    assert good.tolist() == [True, False, True] and zu == max_z
    good, _ = CO.spectrum_cut(w, v, min_z, max_z, 0.1, None)           # pixel cut off: all good
    assert good.tolist() == [True, True, True]


def test_bad_pixels_nan_inf_equality():
    w = spectrum(2.0, 3.0, 5, 0, 0)
    v = np.array([np.nan, np.inf, 0.25, 0.2499999, -1.0])
    good, _ = CO.spectrum_cut(w, v, 2.0, 3.0, None, 0.25)
    assert good.tolist() == [False, False, False, True, True]
    good, _ = CO.spectrum_cut(w, v, 2.0, 3.0, None, math.inf)          # +inf threshold: +inf and NaN stay bad
    assert good.tolist() == [False, False, True, True, True]


def test_upper_end():
    assert CO.spectrum_cut([], [], 2.0, 3.0, 0.1, None)[1] == 3.0 - 0.1
    assert CO.spectrum_cut([], [], 2.0, 2.05, 0.1, None)[1] == 2.0     # the range collapses onto min_z
    assert CO.spectrum_cut([], [], 2.0, 3.0, None, 0.5)[1] == 3.0
    assert math.isnan(CO.spectrum_cut([], [], 2.0, math.nan, 0.1, None)[1])


def test_bitmap_layout():
    g = np.zeros(70, dtype=bool)
    g[[0, 31, 32, 69]] = True
    off, words = CO.bitmap([(g, 3), (np.ones(3, dtype=bool), 1), (np.zeros(0, dtype=bool), 0)])
    assert off.tolist() == [0, 3, 4, 4]
    assert words.tolist() == [1 | (1 << 31), 1, 1 << 5, 7]


def test_sample_tests():
    good = np.array([True, False, True, True])
    # span 1, n = 4: pixel index = trunc(4 (z - 2))
    z = np.array([2.0, 2.24, 2.25, 2.49, 2.5, 2.99, 3.0, 3.5, 1.9, 1.7, np.nan])
    kept = CO.slot_kept(z, 2.0, 3.0, 3.0, good, False, True)
    #                 px0   px0   px1    px1    px2   px3   idx 4  idx 6  -0.4->0 -1.2   NaN
    assert kept.tolist() == [True, True, False, False, True, True, False, False, True, False, False]
    kept = CO.slot_kept(z, 2.0, 3.0, 2.9, good, True, False)           # strict z < z_upper; NaN is cut
    assert kept.tolist() == [True, True, True, True, True, False, False, False, True, True, False]
    assert not CO.slot_kept(np.array([2.0, 2.5]), 2.0, 3.0, 3.0, np.zeros(0, dtype=bool), False, True).any()   # n = 0
    assert not CO.slot_kept(np.array([2.0]), 2.0, 2.0, 2.0, good, False, True).any()                           # span = 0
    assert not CO.slot_kept(np.array([2.5]), math.nan, 3.0, 3.0, good, False, True).any()                      # NaN range


def test_path_by_hand():
    min_z, max_z, n = 2.0, 3.0, 6
    z = CO.zz(min_z, max_z, n)
    assert z[0] == 2.0 and z[-1] == 3.0 and z[1] == 2.0 + (1.0 * 1.0) / 5.0
    good = np.array([True, True, False, True, True, True])
    # the whole range: a run from pixel 0 ended by bad pixel 2, a run from pixel 3 to the end
    t = CO.path_terms(good, min_z, max_z, max_z, 1.5, 3.5, True)
    assert t == [X(z[1]) - X(z[0]), X(max_z) - X(z[3])]
    # a bin ending inside the first run: the bad pixel lies at or past pmax, so the run ends at pmax; the second
    # run starts past pmax and is no start
    t = CO.path_terms(good, min_z, max_z, max_z, 1.5, 2.3, True)
    assert t == [X(2.3) - X(z[0])]
    # a bin beginning inside the second run: pixel 3 (2.6) lies below pmin, so pixel 4 is the start
    t = CO.path_terms(good, min_z, max_z, max_z, 2.7, 3.5, True)
    assert t == [X(max_z) - X(z[4])]
    # the proximity cut clips pmax; the map from pixel to redshift keeps the whole range
    t = CO.path_terms(good, min_z, max_z, 2.9, 1.5, 3.5, True)
    assert t == [X(z[1]) - X(z[0]), X(2.9) - X(z[3])]
    # the last pixel is never a start; a lone good last pixel adds nothing
    assert CO.path_terms(np.array([False, False, True]), min_z, max_z, max_z, 1.5, 3.5, True) == []
    # noisy at pixel 0
    t = CO.path_terms(np.array([False, True, True]), min_z, max_z, max_z, 1.5, 3.5, True)
    assert t == [X(max_z) - X(2.5)]
    # no overlap, either side, and a collapsed range
    assert CO.path_terms(good, min_z, max_z, max_z, 3.0, 3.5, True) == []
    assert CO.path_terms(good, min_z, max_z, max_z, 1.0, 2.0, True) == []
    assert CO.path_terms(good, min_z, max_z, min_z, 2.0, 3.0, True) == []


def test_path_small_counts_and_cut_off():
    full = [X(3.0) - X(2.0)]
    none, one_good, one_bad = np.zeros(0, dtype=bool), np.array([True]), np.array([False])
    assert CO.path_terms(none, 2.0, 3.0, 3.0, 1.5, 3.5, True) == []
    assert CO.path_terms(one_good, 2.0, 3.0, 3.0, 1.5, 3.5, True) == full
    assert CO.path_terms(one_bad, 2.0, 3.0, 3.0, 1.5, 3.5, True) == []
    for g in (none, one_bad, np.array([False, False, False])):         # the pixel cut off: the pixels are not read
        assert CO.path_terms(g, 2.0, 3.0, 3.0, 1.5, 3.5, False) == full
    assert CO.path_terms(np.ones(7, dtype=bool), 2.0, 3.0, 3.0, 2.5, 3.5, True) == [X(3.0) - X(2.5)]
    assert CO.path_terms(one_good, 2.0, math.nan, math.nan, 1.5, 3.5, True) == []          # a NaN range: nothing
    assert CO.path_terms(np.array([True, False]), 2.0, 2.0, 2.0, 1.5, 3.5, True) == [0.0]  # span = 0: zz = min_z


def test_path_against_a_dense_count():
    """The sum over run starts is the length of the good stretches: against a brute-force walk over the pixel
    intervals on random flags (every interval [zz_i, zz_i+1] whose left pixel lies in a run and below the run's
    end counts), to the rounding of X."""
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(2, 40))
        good = rng.random(n) < 0.7
        min_z = 2.0 + rng.random()
        max_z = min_z + 0.3 + rng.random()
        z_lo, z_hi = sorted(rng.uniform(min_z - 0.2, max_z + 0.2, 2))
        terms = CO.path_terms(good, min_z, max_z, max_z, z_lo, z_hi, True)
        if bool(np.all(good)):
            continue
        z = CO.zz(min_z, max_z, n)
        pmin, pmax = max(z_lo, min_z), min(z_hi, max_z)
        want, i = 0.0, 0
        if min_z < z_hi and max_z > z_lo:
            while i < n - 1:
                if good[i] and z[i] >= pmin and z[i] <= pmax:
                    j = i
                    while j + 1 < n and good[j + 1]:
                        j += 1
                    top = z[j] if j + 1 < n and z[j + 1] < pmax else pmax     # the run's last good pixel, or pmax
                    want += X(top) - X(z[i])
                    i = j + 1
                else:
                    i += 1
        assert abs(math.fsum(terms) - want) <= 64 * 2.0 ** -53 * X(max_z + 0.2) * max(len(terms), 1)


def test_search_cuts_dict_and_reductions_without_effect():
    rng = np.random.default_rng(11)
    R, S = 3, 40
    min_z, max_z = np.array([2.0, 2.2, 2.4]), np.array([3.0, 3.5, 3.1])
    wl = [spectrum(min_z[r], max_z[r], n) for r, n in enumerate((33, 0, 64))]
    nv = [rng.random(w.size) for w in wl]
    edges = np.linspace(2.0, 4.0, 13)
    cuts = CO.search_cuts(wl, nv, min_z, max_z, 0.1, 0.7, z_edges_summary=edges, z_edges_population=edges[[0, -1]])
    assert cuts["cut_pixel_counts"].tolist() == [33, 0, 64]
    assert cuts["cut_bitmap_offsets"].tolist() == [0, 2, 3, 6]        # ceil(len / 32) words per spectrum
    assert cuts["cut_path_summary"].shape == (R, 13) and cuts["cut_path_population"].shape == (R, 2)
    assert not cuts["cut_path_summary"][1].any()                       # n = 0 under the pixel cut
    # the whole extent is the sum of the bins wherever no run straddles an edge; always: no bin exceeds the uncut path
    uncut = CO.search_cuts(wl, nv, min_z, max_z, 0.0, None, z_edges_summary=edges)
    assert np.all(cuts["cut_path_summary"] <= uncut["cut_path_summary"] + 1e-12)
    # a cut that removes nothing leaves the reductions as they are
    ll = rng.normal(0.0, 1.0, (2, R, S))
    base = rng.integers(0, S, (1, R, S)).astype(np.int32)
    off, ln = rng.random(S), rng.uniform(20.0, 23.0, S)
    en = np.linspace(20.0, 23.0, 6)
    wl[1] = spectrum(min_z[1], max_z[1], 5)
    nv[1] = rng.random(wl[1].size)
    nothing = CO.search_cuts(wl, nv, min_z, max_z, 0.0, math.inf)
    got, _ = CO.level_planes(nothing, ll, base, min_z, max_z, off, ln, 10.0 ** ln, edges, en)
    want, _ = LO.level_planes(ll, base, min_z, max_z, off, ln, 10.0 ** ln, edges, en)
    assert np.array_equal(got, want)
    cut, count = CO.level_planes(cuts, ll, base, min_z, max_z, off, ln, 10.0 ** ln, edges, en)
    assert not cut[1].any() and 0 < count[0].sum() < _[0].sum()        # row 1 has no pixels; row 0 loses some slots


def test_wrapper_argument_checks():
    w = [np.linspace(3700.0, 4800.0, 10)]
    with pytest.raises(ValueError):
        E.search_cuts(w, [np.ones(9)], [2.0], [3.0], 0.1, None)
    with pytest.raises(ValueError):
        E.search_cuts(w, [np.ones(10), np.ones(10)], [2.0], [3.0], 0.1, None)
    with pytest.raises(ValueError):
        E.search_cuts(w, [np.ones(10)], [2.0, 2.1], [3.0], 0.1, None)


# ------------------------------------------------------------------- the reference under its own cuts
import test_population as TP  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from test_population import setup  # noqa: E402,F401  (the module fixture: model, samples, spectra, prior)

GOLDEN = Path(__file__).parent / "golden" / "search_cuts.npz"
SETTINGS = ("proximity", "pixels", "both")


def fixture_spectra(g):
    """Wavelength and noise cells whose search-range pixels are the fixture's noise vectors: n pixels strictly
    inside the Lya range of the row, one outside on either side."""
    o = g["noise_offsets"]
    wl = [spectrum(g["min_z_dlas"][q], g["max_z_dlas"][q], int(o[q + 1] - o[q]), 1, 1) for q in range(o.size - 1)]
    nv = [np.concatenate([[0.0], g["noise_values"][o[q]:o[q + 1]], [0.0]]) for q in range(o.size - 1)]
    return wl, nv


def fixture_cuts(g, setting):
    wl, nv = fixture_spectra(g)
    pz = float(g["proximity_zone"]) if setting != "pixels" else None
    nt = float(g["noise_thresh"]) if setting != "proximity" else None
    return CO.search_cuts(wl, nv, g["min_z_dlas"], g["max_z_dlas"], pz, nt, z_edges_summary=g["z_edges"],
                          z_edges_population=g["z_edges"])


def cut_out(g, cuts, split, planes):
    """What catalog.py reads of a run under the cuts, from level-1 arrays in the level layout."""
    out = dict(population_poisson=split["population_level_poisson"][:, 0],
               population_large_inds=split["population_level_large_inds"][:, 0].astype(np.float64) + 1.0,
               population_large_probs=split["population_level_large_probs"][:, 0],
               population_large_bins=split["population_level_large_bins"][:, 0, :, 0].astype(np.float64) + 1.0,
               p_dlas=g["p_dlas"], min_z_dlas=g["min_z_dlas"], max_z_dlas=g["max_z_dlas"],
               population_z_edges=g["z_edges"], population_log_nhi_edges=g["log_nhi_edges"], bin_planes=planes[:, 0],
               bin_z_edges=g["z_edges"], bin_log_nhi_edges=g["log_nhi_edges"])
    out.update({k: cuts[k] for k in ("cut_proximity_zone", "cut_noise_thresh", "cut_z_uppers", "cut_pixel_counts",
                                     "cut_path_summary", "cut_path_population")})
    return out


def reference_view(g, setting):
    """The fixture's numbers of one setting under the names test_population's checks read."""
    view = {k: g[k] for k in ("p_dlas", "min_z_dlas", "max_z_dlas", "z_edges", "log_nhi_edges")}
    view.update({"ref_" + k[len(setting) + 1:]: g[k] for k in g.files if k.startswith(setting + "_")})
    return view


def check_cut_curves(ref, out, cuts, pmf):
    """test_population.check_curves_against_reference with the cut path: interval integers equal; for one cut
    alone the path within the reference's quadrature tolerance per integral it takes (one per term), and f(N) and
    dN/dX within 1e-12 beyond what that allows."""
    ez = ref["z_edges"]
    for name, axis in (("nhi", "log_nhi"), ("z", "z")):
        n, l68, l95 = CAT.confidence_intervals(out, axis=axis, pmf=pmf)
        assert np.array_equal(n, ref[f"ref_{name}_maxlikes"]), name
        assert np.array_equal(l68, ref[f"ref_{name}_l68"]) and np.array_equal(l95, ref[f"ref_{name}_l95"]), name
    if "ref_path_total" not in ref:
        return
    per_bin, total = CAT._bin_paths(out, "population", ez, None, 0.279)
    tols = np.maximum(cuts["terms_population"].sum(axis=0), 1) * TP.QUAD_ABS_TOL
    tol_bins, tol_total = tols[:-1], tols[-1]
    print(f"path: total deviation {abs(total - ref['ref_path_total']):.3e}, per bin {np.abs(per_bin - ref['ref_path_bins']).max():.3e}")
    assert abs(total - ref["ref_path_total"]) <= tol_total and np.all(np.abs(per_bin - ref["ref_path_bins"]) <= tol_bins)
    cent, f, f68, f95, _ = CAT.column_density_function(out, pmf=pmf)
    rtol = 1e-12 + tol_total / ref["ref_path_total"]
    assert np.array_equal(cent, ref["ref_cddf_cent"])
    for got, want in ((f, ref["ref_cddf_f"]), (f68, ref["ref_cddf_f68"]), (f95, ref["ref_cddf_f95"])):
        assert got.shape == want.shape and np.all(np.abs(got - want) <= rtol * np.abs(want))
    zc, dndx, d68, d95, _ = CAT.line_density(out, pmf=pmf)
    keep = ref["ref_path_bins"] > 0
    rt = 1e-12 + tol_bins[keep] / ref["ref_path_bins"][keep]
    assert np.array_equal(zc, ref["ref_dndx_cent"]) and np.all(np.abs(dndx - ref["ref_dndx_f"]) <= rt * np.abs(ref["ref_dndx_f"]))
    for got, want in ((d68, ref["ref_dndx_f68"]), (d95, ref["ref_dndx_f95"])):
        assert got.shape == want.shape and np.all(np.abs(got - want) <= rt[:, None] * np.abs(want))
    # Omega_DLA by moments is this package's own under the cuts (the reference's omega_dla bins its samples uncut):
    # the cut planes over the cut path
    zc, om, err, zb = CAT.omega_dla(out)
    means = CAT.cddf_moments(out["bin_planes"], out["p_dlas"], None, 0.05, moment=True)[0].sum(axis=1)
    conv = CAT.PROTON_MASS_G * (CAT.H100_PER_S * 0.7) / CAT.LIGHT_CM_PER_S / per_bin[keep] / CAT.rho_crit()
    assert np.array_equal(om[keep], means[keep] * conv) and np.all(om[keep] > 0)


@pytest.mark.parametrize("setting", SETTINGS)
def test_oracle_matches_the_reference_under_its_cuts(setting):
    """The numpy restatement through catalog.py against executed reference code (calc_cddf.py with ``lowzcut``,
    ``filter_noisy_pixels`` and both): the same trials in the same bins in the same order, values and Poisson means
    within test_population's bar, every interval integer equal, paths and curves within the quadrature margin."""
    g = np.load(GOLDEN)
    cuts = fixture_cuts(g, setting)
    ll = g["sample_log_likelihoods"][None]
    args = (g["min_z_dlas"], g["max_z_dlas"])
    split = CO.level_split(cuts, ll, None, *args, g["p_dlas"][None], g["offset_samples"], g["log_nhi_samples"], g["z_edges"],
                           g["log_nhi_edges"])
    planes, _ = CO.level_planes(cuts, ll, None, *args, g["offset_samples"], g["log_nhi_samples"], g["nhi_samples"],
                                g["z_edges"], g["log_nhi_edges"])
    out = cut_out(g, cuts, split, planes)
    ref = reference_view(g, setting)
    TP.check_split_against_reference(ref, out)
    check_cut_curves(ref, out, cuts, TP.recurrence)
    # the cut bites: fewer trials or less Poisson mass than the uncut fixture, and less path
    uncut = np.load(TP.GOLDEN)
    assert ref["ref_z_poissons"].sum() < uncut["ref_z_poissons"].sum()
    if setting != "both":
        assert ref["ref_path_total"] < 0.97 * uncut["ref_path_total"]
    assert cuts["cut_z_uppers"][39] == (g["min_z_dlas"][39] if setting != "pixels" else g["max_z_dlas"][39])


# ------------------------------------------------------------------- process_qsos and catalog.py without a device
import bootstrap_oracle as BO  # noqa: E402
import count_mixture_oracle as MO  # noqa: E402

GRID = dict(z_edges=np.linspace(2.0, 4.0, 4), log_nhi_edges=np.linspace(20.0, 23.0, 3))
POP = dict(z_edges=np.linspace(1.6, 4.6, 8), log_nhi_edges=np.linspace(20.0, 23.0, 6))


def cut_compute(calls):
    """A ``compute`` replacement: test_population's for the uncut run, then the oracle of this module on its
    level-1 rows for every grid reduction, and the cut variables."""
    def compute(model, samples, packed, params, device=0, **kw):
        calls.append(dict(kw))
        cuts = kw.pop("cuts", None)
        lean = kw.pop("save_samples", True) is False
        res = TP.population_compute([])(model, samples, packed, params, device, **kw)
        if cuts is not None:
            o = np.asarray(packed["offsets"])
            cells = [[np.asarray(packed[key])[a:b] for a, b in zip(o[:-1], o[1:])] for key in ("wavelengths", "noise_variance")]
            zr = (np.asarray(res["min_z_dlas"]), np.asarray(res["max_z_dlas"]))
            summaries, pop = kw.get("summaries"), kw.get("population")
            c = CO.search_cuts(*cells, *zr, None if np.isnan(cuts["proximity_zone"]) else cuts["proximity_zone"],
                               None if np.isnan(cuts["noise_thresh"]) else cuts["noise_thresh"],
                               z_edges_summary=None if summaries is None else summaries["z_edges"],
                               z_edges_population=None if pop is None else pop["z_edges"], omega_m=cuts["omega_m"])
            ll = np.asarray(res["sample_log_likelihoods_dla"])[None]
            sm = (samples["offset_samples"], samples["log_nhi_samples"])
            if summaries is not None:
                res["bin_planes"] = CO.level_planes(c, ll, None, *zr, *sm, samples["nhi_samples"], summaries["z_edges"],
                                                    summaries["log_nhi_edges"])[0][:, 0]
            if pop is not None:
                split = CO.level_split(c, ll, None, *zr, np.asarray(res["population_p_dlas"])[None], *sm, pop["z_edges"],
                                       pop["log_nhi_edges"], p_thresh_sample=pop["p_thresh_sample"], p_switch=pop["p_switch"])
                res.update(population_poisson=split["population_level_poisson"][:, 0],
                           population_large_inds=split["population_level_large_inds"][:, 0],
                           population_large_probs=split["population_level_large_probs"][:, 0],
                           population_large_bins=split["population_level_large_bins"][:, 0, :, 0])
            res.update({k: v for k, v in c.items() if k.startswith("cut_")})
        if lean:
            res.pop("sample_log_likelihoods_dla", None)
        return res
    return compute


def run_cut(s, calls=None, **kw):
    calls = [] if calls is None else calls
    return PR.process_qsos(s["model"], s["samples"], s["packed"], s["prior"], params=s["params"], compute=cut_compute(calls), **kw)


def test_process_qsos_cuts_with_a_compute_substitute(setup, tmp_path):  # noqa: F811
    nv = np.sort(np.asarray(setup["packed"]["noise_variance"]))
    thresh = 0.5 * (nv[(3 * nv.size) // 4] + nv[(3 * nv.size) // 4 + 1])
    cuts = dict(proximity_zone=0.02, noise_thresh=thresh)        # the 120-pixel ranges are about 0.1 wide
    calls = []
    plain = run_cut(setup, calls, summaries=GRID, population=POP)
    assert "cuts" not in calls[-1]                                       # the keyword travels only when set
    cut = run_cut(setup, calls, summaries=GRID, population=POP, cuts=cuts)
    assert calls[-1]["cuts"] == dict(proximity_zone=0.02, noise_thresh=thresh, omega_m=0.279)
    half = run_cut(setup, calls, population=POP, cuts=dict(proximity_zone=None, noise_thresh=thresh, omega_m=0.3), save_samples=False)
    assert math.isnan(calls[-1]["cuts"]["proximity_zone"]) and calls[-1]["save_samples"] is False
    assert set(cut) - set(plain) == set(PR.CUT_VARIABLES)
    assert set(half) & set(PR.CUT_VARIABLES) == set(PR.CUT_VARIABLES) - {"cut_path_summary"} and half["cut_omega_m"] == 0.3
    assert math.isnan(half["cut_proximity_zone"]) and TP.same(half["cut_z_uppers"], half["max_z_dlas"])
    grid_keys = {"bin_planes", "population_poisson", "population_large_inds", "population_large_probs", "population_large_bins"}
    for key in plain:
        assert key in grid_keys or TP.same(plain[key], cut[key]), key
    assert cut["bin_planes"][:, 0].sum() < plain["bin_planes"][:, 0].sum()
    assert cut["cut_path_summary"].shape == (3, 4) and cut["cut_path_population"].shape == (3, 8) and cut["cut_pixel_counts"].dtype == np.float64

    # catalog.py: the stored columns are the path whenever the output carries them, keep applied, fsum
    keep = np.array([True, False, True])
    for out, kp in ((cut, None), (cut, keep), (plain, None), (plain, keep)):
        ez = POP["z_edges"]
        if out is cut:
            cols = np.array(out["cut_path_population"])
            if kp is not None:
                cols[~kp] = 0.0
            want = np.array([math.fsum(cols[:, c]) for c in range(ez.size)])
        else:
            want = np.array([CAT.path_length(a, b, out["min_z_dlas"], out["max_z_dlas"], kp) for a, b in zip(ez[:-1], ez[1:])] +
                            [CAT.path_length(ez[0], ez[-1], out["min_z_dlas"], out["max_z_dlas"], kp)])
        n_z = CAT.confidence_intervals(out, kp, axis="z", pmf=TP.recurrence)[0]
        zc, dndx = CAT.line_density(out, kp, pmf=TP.recurrence)[:2]
        ii = want[:-1] > 0
        assert ii.any() and TP.same(dndx, n_z[ii] / want[:-1][ii])
        n_n = CAT.confidence_intervals(out, kp, axis="log_nhi", pmf=TP.recurrence)[0]
        en = POP["log_nhi_edges"]
        assert TP.same(CAT.column_density_function(out, kp, pmf=TP.recurrence)[1], n_n / want[-1] / (10.0 ** en[1:] - 10.0 ** en[:-1]))
        zo, _, om68 = CAT.omega_dla_cddf(out, kp, pmf=TP.recurrence, mixture=MO.mixture(MO.numpy_chain), cells=2 ** 12)[:3]
        assert TP.same(zo, zc) and om68.shape == (zc.size, 2)
        sgrid = np.array([CAT.path_length(a, b, out["min_z_dlas"], out["max_z_dlas"], kp) for a, b in zip(GRID["z_edges"][:-1], GRID["z_edges"][1:])])
        if out is cut:
            scols = np.array(out["cut_path_summary"])
            if kp is not None:
                scols[~kp] = 0.0
            sgrid = np.array([math.fsum(scols[:, c]) for c in range(3)])
        means = CAT.cddf_moments(out["bin_planes"], out["p_dlas"], kp, 0.05, moment=True)[0].sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            conv = CAT.PROTON_MASS_G * (CAT.H100_PER_S * 0.7) / CAT.LIGHT_CM_PER_S / sgrid / CAT.rho_crit()
            assert TP.same(CAT.omega_dla(out, kp)[1], means * conv)
        bm = CAT.bootstrap_moments(out, 2, 7, keep=kp, strata=None, sums=BO.sums_all_ones)
        assert np.all(np.abs(bm["path"] - sgrid[None, :]) <= 4 * 2.0 ** -53 * 3 * sgrid.max())
        se = CAT.sample_errors(out, 2, 7, keep=kp, strata=None, sums=BO.sums_all_ones)
        assert se["z"].size == int((sgrid > 0).sum()) and np.all(np.isfinite(se["dndx_median"]))
    assert CAT.cut_path_columns(plain, "summary") is None and CAT.search_cuts.__doc__
    with pytest.raises(ValueError):
        CAT.line_density(cut, omega_m=0.3, pmf=TP.recurrence)            # the stored path is for the run's omega_m
    with pytest.raises(ValueError):
        CAT.omega_dla({k: v for k, v in cut.items() if k != "cut_path_summary"})   # cut planes, no cut path for them
    with pytest.raises(ValueError):
        CAT.bootstrap_moments(dict(cut, cut_path_summary=cut["cut_path_summary"][:, :3]), 2, 7, strata=None, sums=BO.sums_all_ones)

    # the file
    PR.save_processed_qsos(str(tmp_path / "cut.mat"), cut)
    from gp_dla_detection_amd.matv73 import loadmat
    back = loadmat(str(tmp_path / "cut.mat"))
    for key in PR.CUT_VARIABLES:
        assert TP.same(np.asarray(back[key], dtype=np.float64).reshape(np.shape(cut[key])), cut[key]), key
    PR.save_processed_qsos(str(tmp_path / "plain.mat"), plain)
    assert not set(loadmat(str(tmp_path / "plain.mat"))) & set(PR.CUT_VARIABLES)

    # the keyword
    for bad in (dict(cuts=dict(proximity_zone=None, noise_thresh=None)), dict(cuts=dict(zone=0.1)), dict(cuts=0.1),
                dict(cuts=cuts, intervals=True), dict(cuts=cuts, sub_dla=True), dict(cuts=dict(proximity_zone=-1.0)),
                dict(cuts=dict(proximity_zone=math.inf)), dict(cuts=dict(proximity_zone=0.1, omega_m=0.0))):
        with pytest.raises(ValueError):
            run_cut(setup, summaries=GRID, population=POP, **bad)
    with pytest.raises(ValueError, match="grid"):
        run_cut(setup, cuts=cuts)                                         # no grid, no population
    with pytest.raises(ValueError, match="intervals"):
        run_cut(setup, summaries=GRID, cuts=cuts, intervals=True)
    with pytest.raises(ValueError, match="sub_dla"):
        run_cut(setup, summaries=GRID, cuts=cuts, sub_dla=True)

"""Population statistics over every multi-DLA level, the parts that need no GPU: the numpy oracle
(level_population_oracle.py) pinned to the reference through its level-1 restriction, hand-built exact
cases, mass conservation, and ``process_qsos(..., levels="all")`` with an injected compute through the saved
file and catalog.py."""
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import level_population_oracle as LO  # noqa: E402
import population_oracle as PO  # noqa: E402
import posterior_summary_oracle as SO  # noqa: E402
import test_population as TP  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402
from gp_dla_detection_amd import matv73 as M  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402

SUMMARY_GOLDEN = Path(__file__).parent / "golden" / "posterior_summary.npz"


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ------------------------------------------------------------------------ 1. the level-1 restriction
def test_level_one_restriction_is_the_reference_path():
    """D = 1 with P_1 = p_dlas: the level oracle and catalog.py's ``levels="all"`` path give the trials,
    interval integers and curves that test_population.py establishes against executed reference code."""
    g = np.load(TP.GOLDEN)
    first = TP.golden_out(g, TP.oracle_split(g), TP.oracle_planes(g))
    ll = g["sample_log_likelihoods"][None]
    split = LO.level_split(ll, None, g["min_z_dlas"], g["max_z_dlas"], g["p_dlas"][None], g["offset_samples"],
                           g["log_nhi_samples"], g["z_edges"], g["log_nhi_edges"])
    # slot 0 of the one level is population_oracle's split, entry for entry
    assert same(split["population_level_large_inds"][:, 0], TP.oracle_split(g)["population_large_inds"])
    assert same(split["population_level_large_probs"][:, 0], TP.oracle_split(g)["population_large_probs"])
    assert same(split["population_level_large_bins"][:, 0, :, 0], TP.oracle_split(g)["population_large_bins"])
    assert (split["population_level_large_bins"][:, 0, :, 1:] == -1).all()
    planes, _ = LO.level_planes(ll, None, g["min_z_dlas"], g["max_z_dlas"], g["offset_samples"], g["log_nhi_samples"],
                                g["nhi_samples"], g["z_edges"], g["log_nhi_edges"])
    assert same(planes[:, 0], TP.oracle_planes(g))
    out = dict(first, **LO.one_based(split), bin_planes_levels=planes,
               model_posteriors=np.stack([1.0 - g["p_dlas"], g["p_dlas"]], axis=1))
    for axis in ("log_nhi", "z"):
        lists, means = CAT.split_distributions(out, axis=axis, levels="all")
        want_lists, want_means = CAT.split_distributions(out, axis=axis)
        assert len(lists) == len(want_lists) and all(same(a, b) for a, b in zip(lists, want_lists))   # the trials
        # a bin's Poisson mean: fsum per spectrum then fsum here, against the sample-order sum per spectrum
        assert np.array_equal(means == 0, want_means == 0)
        nzr = want_means != 0
        assert np.all(np.abs(means[nzr] - want_means[nzr]) <= 1e-13 * want_means[nzr])
        got = CAT.confidence_intervals(out, axis=axis, pmf=TP.recurrence, levels="all")
        name = "nhi" if axis == "log_nhi" else "z"
        assert np.array_equal(got[0], g[f"ref_{name}_maxlikes"])                                       # the integers
        assert np.array_equal(got[1], g[f"ref_{name}_l68"]) and np.array_equal(got[2], g[f"ref_{name}_l95"])
    for fn in (CAT.column_density_function, CAT.line_density):                                         # the curves
        for a, b in zip(fn(out, pmf=TP.recurrence, levels="all")[:4], fn(out, pmf=TP.recurrence)[:4]):
            assert same(a, b)
    for a, b in zip(CAT.omega_dla(out, levels="all"), CAT.omega_dla(out)):
        assert same(a, b)
    # and the reference's own split lists, through the levels path alone
    TP.check_split_against_reference(g, dict(out, **{k.replace("_level", ""): np.asarray(v)[:, 0, ..., 0]
                                                     if k.endswith("bins") else np.asarray(v)[:, 0]
                                                     for k, v in LO.one_based(split).items()}))


def test_moments_with_levels_reduce_to_the_plain_ones():
    g = np.load(SUMMARY_GOLDEN)
    ll = g["sample_log_likelihoods"]
    planes = np.stack([SO.bin_planes(ll[q], g["min_z_dlas"][q], g["max_z_dlas"][q], g["offset_samples"],
                                     g["log_nhi_samples"], g["nhi_samples"], g["z_edges"], g["log_nhi_edges"])[0]
                       for q in range(ll.shape[0])])
    for moment in (False, True):
        want = CAT.cddf_moments(planes, g["p_dlas"], moment=moment)
        for got in (CAT.cddf_moments(planes, g["p_dlas"], moment=moment, levels="all"),
                    CAT.cddf_moments(planes[:, None], g["p_dlas"], moment=moment, levels="all",
                                     level_posteriors=g["p_dlas"][:, None])):
            assert same(got[0], want[0]) and same(got[1], want[1])
    # the formula at D = 2
    rng = np.random.default_rng(3)
    pl = rng.uniform(0.0, 1.0, (3, 2, 5, 2, 2))
    P = np.array([[0.5, 0.25], [0.125, 0.5], [0.01, 0.02]])
    p = np.array([0.75, 0.625, 0.03])                     # the last spectrum is below p_thresh_spec
    m, v = CAT.cddf_moments(pl, p, levels="all", level_posteriors=P)
    want_m = sum(P[q, d] * pl[q, d, 0] for q in range(2) for d in range(2))
    want_v = sum(P[q, d] * pl[q, d, 0] - P[q, d] ** 2 * pl[q, d, 1] for q in range(2) for d in range(2)) + want_m
    np.testing.assert_allclose(m, want_m, rtol=1e-15)
    np.testing.assert_allclose(v, want_v, rtol=1e-14)
    with pytest.raises(ValueError):
        CAT.cddf_moments(pl, p, levels="all")             # D = 2 needs the level posteriors
    with pytest.raises(ValueError):
        CAT.cddf_moments(pl, p, levels="every")


# ------------------------------------------------------------------------ 2. exact dyadic cases
EXACT_Z_EDGES, EXACT_N_EDGES = np.array([2.0, 3.0, 4.0]), np.array([20.0, 21.0, 22.0])
EXACT_SWITCH, EXACT_THRESH = 0.125, 1e-4


def exact_case(D):
    """Two rows of S = 8 samples at D levels in dyadic numbers: four equal finite samples per (level, row) and
    the rest NaN, so pi = 0.25; P_d in {0.5, 0.25}, so p is 0.125 (= p_switch: the exact list) or 0.0625 (the
    Poisson plane).  z = 2 + 2 offset and the column densities are powers of two; sample 7 lies outside the
    grid in log N_HI.  Row 1 has an all-NaN level 2 when D > 2."""
    S = 8
    offset = np.array([0.0625, 0.125, 0.25, 0.375, 0.5625, 0.625, 0.75, 0.875])      # z: 2.125 ... 3.75
    log_nhi = np.array([20.5, 20.25, 21.5, 20.75, 21.25, 20.5, 21.75, 22.5])         # sample 7: outside
    nhi = 2.0 ** np.array([1, 2, 3, 1, 2, 3, 1, 2], dtype=np.float64)
    ll = np.full((D, 2, S), np.nan)
    finite = [[(0, 1, 2, 3), (2, 3, 6, 7)], [(0, 3, 4, 7), (1, 2, 5, 6)], [(0, 1, 4, 5), (3, 4, 6, 7)], [(2, 3, 4, 5), (0, 2, 5, 7)]]
    for d in range(D):
        for r in range(2):
            ll[d, r, list(finite[d][r])] = -3.0 - d - r
    if D > 2:
        ll[1, 1, :] = np.nan
    # base[d - 2][r][j]: level d's base index of j.  Level 2, row 0: sample 0 -> 3 (the same bin as 0: two
    # slots of one sample in one bin), 3 -> 7 (a slot outside the grid), 4 -> -1 (a void chain), 7 -> 0
    base = np.array([[[3, 2, 0, 7, -1, 1, 4, 0], [1, 0, 3, 2, 5, 4, 7, 6]],
                     [[1, 0, 7, 2, 3, -1, 5, 4], [2, 3, 0, 1, 6, 7, 4, 5]],
                     [[4, 5, 0, 1, 2, 3, 8, 6], [7, 6, 5, 4, 3, 2, 1, 0]]], dtype=np.int32)[:D - 1]   # (the 8: outside [0, S))
    P = np.array([[0.5, 0.25], [0.25, 0.5], [0.5, 0.5], [0.25, 0.25]])[:D]
    return dict(ll=ll, base=base, min_z=np.array([2.0, 2.0]), max_z=np.array([4.0, 4.0]), P=P, offset=offset,
                log_nhi=log_nhi, nhi=nhi)


def exact_expected(c):
    """The outputs of ``exact_case`` in rational arithmetic, sample by sample and slot by slot (nothing shared
    with the oracle's vectorised code), and the list of special situations met."""
    D, R, S = c["ll"].shape
    nz, nn = EXACT_Z_EDGES.size - 1, EXACT_N_EDGES.size - 1
    planes = [[[[Fraction(0)] * (nz * nn) for _ in range(5)] for _ in range(D)] for _ in range(R)]
    poisson = [[[Fraction(0)] * (nz * nn) for _ in range(D)] for _ in range(R)]
    large = [[[] for _ in range(D)] for _ in range(R)]
    met = set()

    def bin_of(j):
        z = Fraction(2) + Fraction(2) * Fraction(float(c["offset"][j]))
        n = Fraction(float(c["log_nhi"][j]))
        iz = [i for i in range(nz) if Fraction(float(EXACT_Z_EDGES[i])) <= z < Fraction(float(EXACT_Z_EDGES[i + 1]))]
        inn = [i for i in range(nn) if Fraction(float(EXACT_N_EDGES[i])) <= n < Fraction(float(EXACT_N_EDGES[i + 1]))]
        return iz[0] * nn + inn[0] if iz and inn else -1

    for r in range(R):
        for d in range(D):
            fin = [j for j in range(S) if not np.isnan(c["ll"][d, r, j])]
            if not fin:
                met.add("all-NaN level")
                continue
            pi = Fraction(1, len(fin))
            p = Fraction(float(c["P"][d, r])) * pi
            for j in fin:
                chain, ok = [j], True
                for i in range(d):
                    b = int(c["base"][d - 1 - i][r][chain[-1]])
                    if b < 0 or b >= S:
                        ok = False
                        break
                    chain.append(b)
                if not ok:
                    met.add("void chain")
                    continue
                bins = [bin_of(s) for s in chain]
                if -1 in bins:
                    met.add("slot outside")
                if len([b for b in bins if b >= 0]) > len({b for b in bins if b >= 0}):
                    met.add("two slots in one bin")
                for s, b in zip(chain, bins):
                    if b >= 0:
                        N = Fraction(float(c["nhi"][s]))
                        for k, t in enumerate((pi, pi * pi, N * pi, N * N * pi, N * N * pi * pi)):
                            planes[r][d][k][b] += t
                if any(b >= 0 for b in bins):
                    if p >= Fraction(EXACT_SWITCH):
                        met.add("p == p_switch" if p == Fraction(EXACT_SWITCH) else "p > p_switch")
                        large[r][d].append((j, p, bins))
                    elif p > Fraction(EXACT_THRESH):
                        for b in bins:
                            if b >= 0:
                                poisson[r][d][b] += p
    return planes, poisson, large, met


def check_exact(c, planes, split):
    """``planes`` (rows x D x 5 x nz x nn) and the split arrays against ``exact_expected``, bit for bit."""
    D, R, _ = c["ll"].shape
    want_planes, want_poisson, want_large, _ = exact_expected(c)
    assert same(planes.reshape(R, D, 5, -1), np.array([[[[float(v) for v in k] for k in d] for d in r] for r in want_planes]))
    assert same(split["population_level_poisson"].reshape(R, D, -1),
                np.array([[[float(v) for v in d] for d in r] for r in want_poisson]))
    for r in range(R):
        for d in range(D):
            n = len(want_large[r][d])
            assert list(split["population_level_large_inds"][r, d]) == [e[0] for e in want_large[r][d]] + [-1] * (8 - n)
            assert same(split["population_level_large_probs"][r, d], [float(e[1]) for e in want_large[r][d]] + [np.nan] * (8 - n))
            want_bins = np.full((8, 4), -1)
            for i, e in enumerate(want_large[r][d]):
                want_bins[i, :len(e[2])] = e[2]
            assert np.array_equal(split["population_level_large_bins"][r, d], want_bins)


@pytest.mark.parametrize("D", [2, 4])
def test_exact_cases(D):
    c = exact_case(D)
    met = exact_expected(c)[3]
    assert {"void chain", "slot outside", "two slots in one bin", "p == p_switch"} <= met and "p > p_switch" not in met
    assert ("all-NaN level" in met) == (D > 2)
    planes, count = LO.level_planes(c["ll"], c["base"], c["min_z"], c["max_z"], c["offset"], c["log_nhi"], c["nhi"],
                                    EXACT_Z_EDGES, EXACT_N_EDGES)
    split = LO.level_split(c["ll"], c["base"], c["min_z"], c["max_z"], c["P"], c["offset"], c["log_nhi"], EXACT_Z_EDGES,
                           EXACT_N_EDGES, p_thresh_sample=EXACT_THRESH, p_switch=EXACT_SWITCH)
    check_exact(c, planes, split)
    # by hand, level 2 of row 0 (P = 0.25, p = 0.0625, finite samples 0, 3, 4, 7): sample 0 and its base 3 both
    # fall in bin (0, 0); sample 3's base 7 is outside the grid; sample 4 is void; sample 7 (outside) has base 0
    assert planes[0, 1, 0, 0, 0] == 1.0 and planes[0, 1, 0].sum() == 1.0 and count[0, 1].sum() > 4    # (the count includes pi = 0)
    assert planes[0, 1, 2, 0, 0] == 0.25 * (2 + 2 + 2 + 2) and planes[0, 1, 3, 0, 0] == 0.25 * (4 + 4 + 4 + 4)
    assert split["population_level_poisson"][0, 1, 0, 0] == 4 * 0.0625 and (split["population_level_large_inds"][0, 1] == -1).all()
    # level 1 of row 0 (P = 0.5, p = 0.125 = p_switch): all four samples go to the exact list, none to the plane
    assert list(split["population_level_large_inds"][0, 0, :4]) == [0, 1, 2, 3] and split["population_level_poisson"][0, 0].sum() == 0
    assert (split["population_level_large_probs"][0, 0, :4] == 0.125).all()


# ------------------------------------------------------------------------ 3. mass conservation
def random_case(seed, D, rows, S, void_fraction=0.0):
    rng = np.random.default_rng(seed)
    ll = rng.normal(-50.0, 3.0, (D, rows, S))
    ll[rng.uniform(size=ll.shape) < 0.1] = np.nan
    base = rng.integers(0, S, (max(D - 1, 0), rows, S)).astype(np.int32)
    base[rng.uniform(size=base.shape) < void_fraction] = -1
    return dict(ll=ll, base=base, min_z=rng.uniform(2.0, 2.4, rows), max_z=rng.uniform(3.0, 4.0, rows),
                offset=rng.uniform(0.0, 1.0, S), log_nhi=rng.uniform(20.0, 23.0, S), rng=rng)


def test_mass_conservation():
    """On a grid that holds every sample and with unbroken chains, level d's sum-pi plane sums to d: every
    sample's mass is counted once per absorber."""
    D, rows, S = 4, 3, 97
    c = random_case(11, D, rows, S)
    planes, count = LO.level_planes(c["ll"], c["base"], c["min_z"], c["max_z"], c["offset"], c["log_nhi"],
                                    10.0 ** c["log_nhi"], np.linspace(1.0, 5.0, 6), np.linspace(19.0, 24.0, 4))
    for d in range(D):
        assert np.all(count[:, d].sum(axis=(1, 2)) == (d + 1) * S)
        assert np.all(np.abs(planes[:, d, 0].sum(axis=(1, 2)) - (d + 1)) <= (d + 1) * S * 2.0 ** -52)
    P = c["rng"].dirichlet(np.ones(D + 1), rows).T[1:]
    assert np.allclose(LO.expected_counts(planes, P).sum(axis=(1, 2)), (P * np.arange(1, D + 1)[:, None]).sum(axis=0), rtol=1e-13)
    dp, dx = LO.margins(c["ll"], c["base"], c["min_z"], c["max_z"], P, c["offset"], c["log_nhi"], np.linspace(1.0, 5.0, 6),
                        np.linspace(19.0, 24.0, 4))
    assert 0 < dp < np.inf and 0 < dx < np.inf


# ------------------------------------------------------------------------ 4. process_qsos(levels="all")
Z_EDGES, N_EDGES, POP = TP.Z_EDGES, TP.N_EDGES, TP.POP


def level_compute(calls):
    """A ``compute`` replacement: test_population's for everything that was there (it never sees ``levels``),
    the level oracle on the same call's sample rows and base indices for the rest."""
    def compute(model, samples, packed, params, device=0, **kw):
        calls.append({k: (dict(v) if isinstance(v, dict) else v) for k, v in kw.items()})
        summaries, population = kw.get("summaries"), kw.get("population")
        inner = dict(kw)
        for key in ("summaries", "population"):
            if isinstance(kw.get(key), dict):
                inner[key] = {k: v for k, v in kw[key].items() if k != "levels"}
        save = inner.pop("save_samples", True)
        res = TP.population_compute([])(model, samples, packed, params, device, **inner)
        D = kw.get("max_dlas", 1)
        sll = np.asarray(res["sample_log_likelihoods_dla"]).reshape((D,) + np.shape(res["sample_log_likelihoods_dla"])[-2:])
        base = res.get("base_sample_inds")
        if isinstance(summaries, dict) and summaries.get("levels") == "all":
            res["bin_planes_levels"] = LO.level_planes(sll, base, res["min_z_dlas"], res["max_z_dlas"],
                                                       samples["offset_samples"], samples["log_nhi_samples"],
                                                       samples["nhi_samples"], summaries["z_edges"],
                                                       summaries["log_nhi_edges"])[0]
        if population is not None and population.get("levels") == "all":
            lld = np.asarray(res["log_likelihoods_dla"]).reshape(D, -1)
            lp_no = population["log_priors_no_dla"] + res["log_likelihoods_no_dla"]
            lp_dla = (population["log_priors_dla"] + lld).T
            if kw.get("sub_dla") is not None:
                post = PR.model_posteriors_sub(lp_no, lp_dla, population["log_priors_lls"] + res["log_likelihoods_lls"])[0]
            else:
                post = PR.model_posteriors_multi(lp_no, lp_dla)[0]
            P = np.ascontiguousarray(post[:, 1:1 + D].T)
            res["population_level_posteriors"] = P
            res.update(LO.level_split(sll, base, res["min_z_dlas"], res["max_z_dlas"], P, samples["offset_samples"],
                                      samples["log_nhi_samples"], population["z_edges"], population["log_nhi_edges"],
                                      p_thresh_sample=population["p_thresh_sample"], p_switch=population["p_switch"]))
        if not save:
            res.pop("sample_log_likelihoods_dla", None)
            res.pop("base_sample_inds", None)
        return res
    return compute


setup = TP.setup


def run(s, calls=None, **kw):
    calls = [] if calls is None else calls
    return PR.process_qsos(s["model"], s["samples"], s["packed"], s["prior"], params=s["params"],
                           compute=level_compute(calls), **kw)


@pytest.mark.parametrize("D,extra", [(1, {}), (3, {}), (2, dict(sub_dla=dict(lls_log_nhi_samples=np.full(TP.S, 19.7),
                                                                                sub_dla_prior_ratio=0.4)))])
def test_process_qsos_levels(setup, tmp_path, D, extra):
    s, Q, S = setup, TP.Q, TP.S
    grid = dict(z_edges=Z_EDGES, log_nhi_edges=N_EDGES)
    plain = run(s, max_dlas=D, summaries=grid, population=POP, **extra)
    explicit = run(s, max_dlas=D, summaries=dict(grid, levels="first"), population=dict(POP, levels="first"), **extra)
    assert list(plain) == list(explicit) and all(same(plain[k], explicit[k]) for k in plain)
    assert not set(plain) & set(PR.LEVEL_POPULATION_VARIABLES)
    calls = []
    out = run(s, calls, max_dlas=D, summaries=dict(grid, levels="all"), population=dict(POP, levels="all"), **extra)
    for key in plain:                                         # nothing that was there moves
        assert same(out[key], plain[key]), key
    assert set(out) - set(plain) == set(PR.LEVEL_POPULATION_VARIABLES)
    assert calls[0]["summaries"]["levels"] == "all" and calls[0]["population"]["levels"] == "all"
    nz, nn = POP["z_edges"].size - 1, POP["log_nhi_edges"].size - 1
    assert out["bin_planes_levels"].shape == (Q, D, 5, Z_EDGES.size - 1, N_EDGES.size - 1)
    assert out["population_level_posteriors"].shape == (Q, D) and out["population_level_poisson"].shape == (Q, D, nz, nn)
    assert out["population_level_large_inds"].shape == out["population_level_large_probs"].shape == (Q, D, 8)
    assert out["population_level_large_bins"].shape == (Q, D, 8, 4)
    assert same(out["bin_planes_levels"][:, 0], out["bin_planes"])
    assert same(out["population_level_posteriors"], np.asarray(out["model_posteriors"])[:, 1:1 + D])
    # 1-based indices, 0 = none; an entry has at least one bin, and none beyond its level
    inds, bins = out["population_level_large_inds"], out["population_level_large_bins"]
    assert inds.dtype == bins.dtype == np.float64 and inds.min() == 0 and 1 <= inds.max() <= S and bins.max() <= nz * nn
    used = inds > 0
    assert used.any() and np.array_equal(used, ~np.isnan(out["population_level_large_probs"]))
    assert np.array_equal(used, (bins > 0).any(axis=3))
    for d in range(D):
        assert (bins[:, d, :, d + 1:] == 0).all()
    # one half alone
    only = run(s, max_dlas=D, summaries=dict(grid, levels="all"), population=POP, **extra)
    assert set(only) - set(plain) == {"bin_planes_levels"} and same(only["bin_planes_levels"], out["bin_planes_levels"])
    # the saved file
    lean = run(s, max_dlas=D, summaries=dict(grid, levels="all"), population=dict(POP, levels="all"), save_samples=False, **extra)
    for key in lean:
        assert same(lean[key], out[key]), key
    lean["test_ind"] = np.ones(Q, dtype=bool)
    path = tmp_path / "processed_qsos_levels.mat"
    PR.save_processed_qsos(str(path), lean)
    r = M.loadmat(str(path))
    for key in PR.LEVEL_POPULATION_VARIABLES + ("bin_planes", "population_poisson"):
        want = np.asarray(lean[key])
        got = np.asarray(r[key])
        assert got.shape == want.shape or want.shape[1] == 1, key         # MATLAB drops no inner axis but D = 1's
        assert same(got.reshape(want.shape), want), key
    # catalog.py from the file's variables
    r = dict(r)
    r["test_ind"] = lean["test_ind"]
    for axis in ("log_nhi", "z"):
        lists, means = CAT.split_distributions(r, axis=axis, levels="all")
        lists1, means1 = CAT.split_distributions(r, axis=axis)
        assert len(lists) == len(lists1)
        keep = np.asarray(lean["p_dlas"]).ravel() > 0.05
        assert sum(v.size for v in lists) == int((bins[keep] > 0).sum())
        if D == 1:
            # P_1 = e_1 / sum where p_dla = 1 - e_0 / sum: the same trials, a rounding apart
            assert [v.size for v in lists] == [v.size for v in lists1]
            assert np.allclose(np.concatenate(lists), np.concatenate(lists1), rtol=1e-13, atol=0)
            assert np.allclose(means, means1, rtol=1e-13, atol=0)
    zc, dndx, d68, d95, _ = CAT.line_density(r, pmf=TP.recurrence, levels="all")
    assert zc.size == dndx.size == d68.shape[0] and np.all(d68[:, 0] <= d68[:, 1]) and np.all(d95[:, 0] <= d68[:, 0])
    cent, f, f68, f95, _ = CAT.column_density_function(r, pmf=TP.recurrence, levels="all")
    assert cent.size == nn and np.all(f95[:, 1] >= f68[:, 1])
    zo, om, err, _ = CAT.omega_dla(r, levels="all")
    zo1, om1, _, _ = CAT.omega_dla(r)
    assert same(zo, zo1) and om.shape == om1.shape
    if D == 1:
        np.testing.assert_allclose(om, om1, rtol=1e-13)
    else:       # deeper levels only add absorbers
        mom = CAT.cddf_moments(r["bin_planes_levels"], r["p_dlas"], levels="all",
                               level_posteriors=np.asarray(r["model_posteriors"])[:, 1:1 + D])[0]
        want = LO.expected_counts(out["bin_planes_levels"], out["population_level_posteriors"].T)[keep].sum(axis=0)
        np.testing.assert_allclose(mom, want, rtol=1e-13)


def test_levels_arguments(setup, tmp_path):
    s = setup
    grid = dict(z_edges=Z_EDGES, log_nhi_edges=N_EDGES)
    for bad in (dict(summaries=dict(grid, levels="every")), dict(population=dict(POP, levels=True)),
                dict(summaries=dict(levels="all")), dict(population=dict(POP, levels="second"))):
        with pytest.raises(ValueError):
            run(s, **bad)
    with pytest.raises(ValueError):
        CAT.split_distributions({}, levels="second")
    for kw in (dict(population=dict(POP, levels="all")), dict(summaries=dict(grid, levels="all"))):
        with pytest.raises(NotImplementedError):
            PR.run_process_qsos(str(tmp_path), "dr12q", "a", "b", None, "dr12q", "dr12q", None, world=2, **kw)

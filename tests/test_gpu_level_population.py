"""Population statistics over every multi-DLA level on the GPU (csrc/level_population.hip): the stand-alone
kernels against the numpy oracle (level_population_oracle.py) and the exact dyadic cases, their reduction to
the level-1 kernels (bitwise), MAP consistency, the engine call (bitwise against the stand-alone kernels,
batching, memory kinds, the level posteriors against the host's) and ``process_qsos(levels="all")``."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import level_population_oracle as LO  # noqa: E402
import posterior_summary_oracle as SO  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import (Engine, level_planes, population_split, population_split_levels,  # noqa: E402
                                         posterior_summary)
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402
from test_gpu_population import P_EDGES_N, P_EDGES_Z, _spectra, _split_rows  # noqa: E402
from test_level_population import (EXACT_N_EDGES, EXACT_SWITCH, EXACT_THRESH, EXACT_Z_EDGES, check_exact,  # noqa: E402
                                   exact_case)

pytestmark = pytest.mark.gpu
SPLIT_KEYS = ("population_level_poisson", "population_level_large_inds", "population_level_large_probs",
              "population_level_large_bins")
LEVEL_KEYS = SPLIT_KEYS + ("population_level_posteriors", "bin_planes_levels")


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _raises_einval(fn, *a, **kw):
    with pytest.raises(L.GpdlaError) as ei:
        fn(*a, **kw)
    assert ei.value.code == L.GPDLA_EINVAL, ei.value


# ------------------------------------------------------------------- 1. the kernels against the oracle
GRIDS = {"1x1": (np.array([1.9, 4.3]), np.array([20.0, 23.0])),
         "7x5": (np.linspace(1.9, 4.3, 8), np.linspace(20.0, 23.0, 6)),
         "32x32": (np.linspace(1.9, 4.3, 33), np.linspace(20.0, 23.0, 33))}
LEVEL_WEIGHTS = np.array([0.55, 0.25, 0.15, 0.05])      # P_d = (the row's p_dla of _split_rows) x this
THRESHOLDS = dict(p_thresh_sample=1e-4, p_switch=0.25)


def standalone_case(S, seed=0):
    """Four levels of test_gpu_population's row kinds (fresh draws per level), random in-range base indices
    with some -1 and two indices past the end, samples inside the log N_HI range.  Built on the CPU alone."""
    rng = np.random.default_rng(9000 + 10 * S + seed)
    lls, ps = zip(*[_split_rows(S, rng) for _ in range(4)])
    ll = np.stack(lls)                                    # 4 x R x S
    R = ll.shape[1]
    P = LEVEL_WEIGHTS[:, None] * ps[0][None, :]
    base = rng.integers(0, S, (3, R, S)).astype(np.int32)
    base[rng.random(base.shape) < 0.06] = -1
    base[0, 0, S - 1], base[2, 1, 0] = S, S + 5            # outside [0, S): void, never read from
    min_z = np.linspace(2.0, 2.4, R)
    return dict(ll=ll, base=base, P=P, offset=rng.random(S), log_nhi=rng.uniform(20.0, 23.0, S), min_z=min_z,
                max_z=min_z + np.linspace(0.9, 1.8, R))


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("S", [1, 4, 63, 64, 65, 511, 512, 513, 1025])
def test_kernels_against_the_oracle(S, grid):
    c = standalone_case(S)
    ez, en = GRIDS[grid]
    nhi = 10.0 ** c["log_nhi"]
    R = c["ll"].shape[1]
    # a condition on the inputs: nothing close enough to a threshold or an edge for rounding to decide it
    dp, dx = LO.margins(c["ll"], c["base"], c["min_z"], c["max_z"], c["P"], c["offset"], c["log_nhi"], ez, en, **THRESHOLDS)
    print(f"S={S} {grid}: closest p to a threshold {dp:.2e}, closest coordinate to an edge {dx:.2e} (relative)")
    assert dp > 1e-9 and dx > 1e-9
    want_planes, count = LO.level_planes(c["ll"], c["base"], c["min_z"], c["max_z"], c["offset"], c["log_nhi"], nhi, ez, en)
    want_split = LO.level_split(c["ll"], c["base"], c["min_z"], c["max_z"], c["P"], c["offset"], c["log_nhi"], ez, en,
                                **THRESHOLDS)
    worst = 0.0
    for levels in (1, 2, 3, 4):
        ll, base, P = c["ll"][:levels], c["base"][:levels - 1] if levels > 1 else None, c["P"][:levels]
        planes = level_planes(ll, c["offset"], c["log_nhi"], nhi, c["min_z"], c["max_z"], ez, en, base_sample_inds=base)
        split = population_split_levels(ll, c["offset"], c["log_nhi"], c["min_z"], c["max_z"], P, ez, en,
                                        base_sample_inds=base, **THRESHOLDS)
        assert planes.shape == (R, levels, 5, ez.size - 1, en.size - 1)
        assert np.array_equal(split["population_level_large_inds"], want_split["population_level_large_inds"][:, :levels])
        assert np.array_equal(split["population_level_large_bins"], want_split["population_level_large_bins"][:, :levels])
        for d in range(levels):
            # a bin holds at most (d + 1) S non-negative terms, each pi = w / W with one exp and W a sum of S terms
            tol = ((d + 1) * S + 16) * 2.0 ** -52
            for got, want in ((planes[:, d], want_planes[:, d]),
                              (split["population_level_poisson"][:, d], want_split["population_level_poisson"][:, d]),
                              (split["population_level_large_probs"][:, d], want_split["population_level_large_probs"][:, d])):
                assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0, want == 0)   # membership
                ok = ~np.isnan(want) & (want != 0)
                if ok.any():
                    rel = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
                    worst = max(worst, float(rel.max() / tol))
                    assert np.all(rel <= tol), (levels, d)
    print(f"S={S} {grid}: worst error / bound {worst:.3f}")
    # the all-NaN rows (row 3 of every level) give nothing
    assert not planes[3].any() and not split["population_level_poisson"][3].any()
    assert (split["population_level_large_inds"][3] == -1).all() and np.isnan(split["population_level_large_probs"][3]).all()
    if S >= 511:
        assert (planes[:, :, 0] > 0).any(axis=(2, 3)).sum() >= 4 * (R - 1) - 2 and (split["population_level_large_inds"][1] >= 0).any()
        assert split["population_level_poisson"][0].any() and (count[:, 3].sum(axis=(1, 2)) < 4 * S).all()   # void chains exist
    # two launches are one launch, bit for bit; and so are two calls
    again = population_split_levels(ll, c["offset"], c["log_nhi"], c["min_z"], c["max_z"], P, ez, en, base_sample_inds=base,
                                    **THRESHOLDS)
    part = population_split_levels(ll[:, 2:], c["offset"], c["log_nhi"], c["min_z"][2:], c["max_z"][2:], P[:, 2:], ez, en,
                                   base_sample_inds=base[:, 2:], **THRESHOLDS)
    for key in SPLIT_KEYS:
        assert _same(split[key], again[key]) and _same(split[key][2:], part[key]), key
    assert _same(planes[2:], level_planes(ll[:, 2:], c["offset"], c["log_nhi"], nhi, c["min_z"][2:], c["max_z"][2:], ez, en,
                                          base_sample_inds=base[:, 2:]))


# ------------------------------------------------------------------- 2. the exact cases on the device
@pytest.mark.parametrize("D", [2, 4])
def test_exact_cases_on_the_device(D):
    c = exact_case(D)
    planes = level_planes(c["ll"], c["offset"], c["log_nhi"], c["nhi"], c["min_z"], c["max_z"], EXACT_Z_EDGES, EXACT_N_EDGES,
                          base_sample_inds=c["base"])
    split = population_split_levels(c["ll"], c["offset"], c["log_nhi"], c["min_z"], c["max_z"], c["P"], EXACT_Z_EDGES,
                                    EXACT_N_EDGES, base_sample_inds=c["base"], p_thresh_sample=EXACT_THRESH,
                                    p_switch=EXACT_SWITCH)
    check_exact(c, planes, split)


# ------------------------------------------------------------------- 3. reduction to what exists, bitwise
@pytest.mark.parametrize("S,grid", [pytest.param(S, grid, id=str(S) if grid == "7x5" else f"{S}-{grid}")
                                    for grid in ("7x5", "32x32") for S in (4, 255, 256, 257, 511, 512, 513, 1025)])
def test_level_one_is_the_existing_kernels(S, grid):
    """The level-1 and the level kernels are one body (csrc/row_posterior.h) at tiles of 512 and 256 samples: the
    sizes at which one of them ends a tile exactly, one short or one over; 32x32 is the LDS cap of both."""
    c = standalone_case(S, seed=1)
    ez, en = GRIDS[grid]
    nhi = 10.0 ** c["log_nhi"]
    planes = level_planes(c["ll"], c["offset"], c["log_nhi"], nhi, c["min_z"], c["max_z"], ez, en, base_sample_inds=c["base"])
    summ = posterior_summary(c["ll"], c["offset"], c["log_nhi"], nhi, c["min_z"], c["max_z"], base_sample_inds=c["base"],
                             z_edges=ez, log_nhi_edges=en)
    assert _same(planes[:, 0], summ["bin_planes"])
    p_dlas = c["P"][0] / LEVEL_WEIGHTS[0]
    one = population_split_levels(c["ll"][0], c["offset"], c["log_nhi"], c["min_z"], c["max_z"], p_dlas[None], ez, en, **THRESHOLDS)
    first = population_split(c["ll"][0], c["offset"], c["log_nhi"], c["min_z"], c["max_z"], p_dlas, ez, en, **THRESHOLDS)
    assert _same(one["population_level_poisson"][:, 0], first["population_poisson"])
    assert _same(one["population_level_large_inds"][:, 0], first["population_large_inds"])
    assert _same(one["population_level_large_probs"][:, 0], first["population_large_probs"])
    assert _same(one["population_level_large_bins"][:, 0, :, 0], first["population_large_bins"])
    assert (one["population_level_large_bins"][:, 0, :, 1:] == -1).all() and first["population_poisson"].any()


# ------------------------------------------------------------------- 4. MAP consistency
def test_single_sample_levels_land_on_the_map_pairs():
    """A level whose only finite sample is j*: pi = 1 there, so the sum-pi plane holds exactly 1.0 per pair in
    the bins of the MAP_z_dlas / MAP_log_nhis pairs the summaries report for that level."""
    S, D, R = 300, 4, 3
    rng = np.random.default_rng(41)
    ll = np.full((D, R, S), np.nan)
    stars = rng.integers(0, S, (D, R))
    for d in range(D):
        for r in range(R):
            ll[d, r, stars[d, r]] = -100.0 - d
    base = rng.integers(0, S, (D - 1, R, S)).astype(np.int32)
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)
    min_z, max_z = np.array([2.0, 2.1, 2.2]), np.array([3.5, 3.9, 4.1])
    ez, en = GRIDS["32x32"]
    planes = level_planes(ll, offset, log_nhi, 10.0 ** log_nhi, min_z, max_z, ez, en, base_sample_inds=base)
    summ = posterior_summary(ll, offset, log_nhi, 10.0 ** log_nhi, min_z, max_z, base_sample_inds=base)
    assert np.array_equal(summ["map_sample_inds"], stars)
    for d in range(D):
        for r in range(R):
            want = np.zeros((ez.size - 1, en.size - 1))
            z, n = summ["MAP_z_dlas"][d, r, :d + 1], summ["MAP_log_nhis"][d, r, :d + 1]
            assert not np.isnan(z).any()
            iz, inn = SO.bin_index(ez, z), SO.bin_index(en, n)
            inside = (iz >= 0) & (inn >= 0)
            np.add.at(want, (iz[inside], inn[inside]), 1.0)
            assert _same(planes[r, d, 0], want), (d, r)
    assert planes[:, :, 0].sum() >= 0.9 * R * 10


def test_void_chains_are_void_for_the_map_walk_and_the_sample_walk():
    """The MAP walk of posterior_summary and the per-sample walk of level_planes are one function
    (csrc/row_posterior.h walk_chain).  Hand-written base indices, one finite sample per (level, row): row 0 has
    complete chains; row 1's level-4 chain breaks at its deepest step (-1); row 2's first base index is S at every
    level >= 2.  The MAP pairs are NaN in exactly the (row, level, slot) where level_planes puts no mass, and
    finite where it puts 1.0."""
    S, D, R = 5, 4, 3
    ll = np.full((D, R, S), np.nan)
    for d in range(D):
        ll[d, :, d] = -50.0 - d                       # the only sample of level d + 1 is sample d
    base = np.empty((D - 1, R, S), dtype=np.int32)
    base[0, :], base[1, :], base[2, :] = [2, 3, 4, 0, 1], [1, 2, 3, 4, 0], [4, 0, 1, 2, 3]
    # row 0: 1 -> 3;  2 -> 3 -> 0;  3 -> 2 -> 3 -> 0
    base[2, 1, 3], base[1, 1, 0], base[0, 1, 4] = 0, 4, -1          # row 1, level 4: 3 -> 0 -> 4 -> void
    base[0, 2, 1] = base[1, 2, 2] = base[2, 2, 3] = S               # row 2: the first step leaves [0, S)
    chains = {(0, 1): [1, 3], (0, 2): [2, 3, 0], (0, 3): [3, 2, 3, 0], (1, 1): [1, 3], (1, 2): [2, 3, 0]}
    chains.update({(r, 0): [0] for r in range(R)})                   # every other (row, level) is void
    offset, log_nhi = np.array([0.1, 0.3, 0.5, 0.7, 0.9]), np.array([20.2, 20.8, 21.4, 22.0, 22.6])
    min_z, max_z = np.array([2.0, 2.1, 2.2]), np.array([3.5, 3.9, 4.1])
    ez, en = GRIDS["32x32"]
    planes = level_planes(ll, offset, log_nhi, 10.0 ** log_nhi, min_z, max_z, ez, en, base_sample_inds=base)
    summ = posterior_summary(ll, offset, log_nhi, 10.0 ** log_nhi, min_z, max_z, base_sample_inds=base)
    assert np.array_equal(summ["map_sample_inds"], np.repeat(np.arange(D)[:, None], R, axis=1))
    for d in range(D):
        for r in range(R):
            z, n = summ["MAP_z_dlas"][d, r], summ["MAP_log_nhis"][d, r]
            chain = chains.get((r, d), [])
            finite = np.arange(D) < len(chain)
            assert np.array_equal(~np.isnan(z), finite) and np.array_equal(~np.isnan(n), finite), (d, r)
            assert np.array_equal(n[finite], log_nhi[chain]), (d, r)
            want = np.zeros((ez.size - 1, en.size - 1))
            iz, inn = SO.bin_index(ez, z[finite]), SO.bin_index(en, n[finite])
            assert (iz >= 0).all() and (inn >= 0).all()                  # every absorber is inside the grid
            np.add.at(want, (iz, inn), 1.0)
            assert _same(planes[r, d, 0], want), (d, r)                  # mass 1.0 per pair; none where void
            assert planes[r, d, 0].sum() == len(chain)


# ------------------------------------------------------------------- 5. the engine
S_LEVEL = 333
# |device P_d - host P_d| / P_d.  Worst case by construction, as DESIGN.md section 15 derives it for p_no: on
# either side P_d = e_d / sum e_m carries one exp (1 ulp = 2^-52 relative at worst, both libraries), a sum of at
# most 6 non-negative terms (each with its own exp; 5 additions) and a quotient -- (2 + 2 + 5 + 1) 2^-53 relative
# each, 20 2^-53 between the two.  No subtraction follows, so the sub-DLA column adds nothing.
LEVEL_POSTERIOR_BOUND = 20 * 2.0 ** -53
# |sum_d P_d - p_dla| on the device: the exact quotients sum to 1; each of the <= 6 quotients rounds once (<= 2^-53
# absolute, P <= 1), the D - 1 <= 3 additions and the 1 - p_no (- p_lls) once each: 11 2^-53
SUM_BOUND = 11 * 2.0 ** -53


@pytest.mark.parametrize("D,sub", [(2, False), (4, False), (2, True), (4, True)])
def test_engine_levels(D, sub):
    k, Q = 4, 5
    model = syn.make_model(k=k)
    samples = syn.make_samples(S_LEVEL)
    packed = syn.pack_spectra(_spectra(model))
    params = set_parameters(k=k)
    lognhi, S = samples["log_nhi_samples"], S_LEVEL
    rng = np.random.default_rng(50 + D)
    forced = rng.integers(0, S, (D - 1, Q, S)).astype(np.int32)
    forced[rng.random(forced.shape) < 0.05] = -1
    skw = dict(sub_dla=samples["nhi_samples"] * 0.02) if sub else {}
    gkw = dict(log_nhi_samples=lognhi, z_edges=np.linspace(2.0, 4.0, 4), log_nhi_edges=np.linspace(20.0, 23.0, 3))
    with Engine(model, samples, params) as eng:
        first = eng.process_population(packed, D, base_sample_inds=forced, **skw)
        lld = first["log_likelihoods_dla"]
        shift = np.array([0.3, -1.1, 2.0, 0.0, -0.2])
        lp_no = np.full(Q, -0.25)
        lp_dla = np.stack([first["log_likelihoods_no_dla"] - np.nan_to_num(lld[d]) + shift - 0.4 * d for d in range(D)])
        lp_dla[:, 3] = -1.0                                 # the masked spectrum's evidences are NaN anyway
        pop = dict(z_edges=P_EDGES_Z, log_nhi_edges=P_EDGES_N, log_nhi_samples=lognhi, log_priors_no_dla=lp_no,
                   log_priors_dla=lp_dla)
        if sub:
            pop["log_priors_lls"] = first["log_likelihoods_no_dla"] - first["log_likelihoods_lls"] - 0.7
            pop["log_priors_lls"][3] = -2.0
        kw = dict(population=pop, base_sample_inds=forced, **gkw, **skw)
        plain = eng.process_population(packed, D, **kw)
        null = eng.process_levels(packed, D, levels=(), **kw)            # the levels pointer NULL
        assert list(plain) == list(null) and all(_same(plain[key], null[key]) for key in plain)
        eng.reset_stats()
        full = eng.process_levels(packed, D, **kw)
        stats = eng.level_population_stats()
        repeat = eng.process_levels(packed, D, **kw)
        again = eng.process_levels(packed, D, want_samples=False, **kw)
        dev = eng.process_levels(packed, D, memory="device", **kw)
        planes_only = eng.process_levels(packed, D, levels=("planes",), **kw)
        split_only = eng.process_levels(packed, D, population=pop, base_sample_inds=forced, **skw)
        # a separation no two absorbers of a sightline can have: level 2 is all NaN
        one = syn.pack_spectra(_spectra(model)[:1])
        far = eng.process_levels(one, D, population=dict(pop, log_priors_no_dla=lp_no[:1], log_priors_dla=lp_dla[:, :1],
                                                         **(dict(log_priors_lls=pop["log_priors_lls"][:1]) if sub else {})),
                                 base_sample_inds=forced[:, :1], min_z_separation=10.0, **gkw, **skw)
    assert stats["level_population_launches"] == 1 and stats["level_population_ms"] > 0
    for key in plain:                                       # every other result unchanged
        assert _same(plain[key], full[key]), key
    assert set(full) - set(plain) == set(LEVEL_KEYS)
    assert list(repeat) == list(full) and all(_same(full[key], repeat[key]) for key in full)      # a repeated call
    assert "sample_log_likelihoods_dla" not in again
    for other in (again, dev):
        for key in LEVEL_KEYS:
            assert _same(full[key], other[key]), key
    assert set(planes_only) - set(plain) == {"bin_planes_levels"} and _same(planes_only["bin_planes_levels"], full["bin_planes_levels"])
    assert "bin_planes_levels" not in split_only and all(_same(split_only[key], full[key]) for key in SPLIT_KEYS)
    assert _same(full["bin_planes_levels"][:, 0], full["bin_planes"])
    # ... and the engine's outputs are the stand-alone kernels on the rows, base indices and P_d it returned
    rows, base, P = full["sample_log_likelihoods_dla"], full["base_sample_inds"], full["population_level_posteriors"]
    assert rows.shape == (D, Q, S) and _same(base, forced) and P.shape == (D, Q)
    alone = population_split_levels(rows, samples["offset_samples"], lognhi, full["min_z_dlas"], full["max_z_dlas"], P,
                                    P_EDGES_Z, P_EDGES_N, base_sample_inds=base)
    for key in SPLIT_KEYS:
        assert _same(full[key], alone[key]), key
    assert _same(full["bin_planes_levels"], level_planes(rows, samples["offset_samples"], lognhi, samples["nhi_samples"],
                                                         full["min_z_dlas"], full["max_z_dlas"], gkw["z_edges"],
                                                         gkw["log_nhi_edges"], base_sample_inds=base))
    ok = np.array([True, True, True, False, True])
    assert np.isnan(P[:, 3]).all() and not np.isnan(P[:, ok]).any()
    assert not full["population_level_poisson"][3].any() and (full["population_level_large_inds"][3] == -1).all()
    assert full["population_level_poisson"][ok].any() and full["bin_planes_levels"][ok][:, D - 1, 0].any()
    # the posteriors: they sum with p_no (and p_lls) to 1, and agree with the host's expression
    p_dev = full["population_p_dlas"]
    gap = np.abs(P[:, ok].sum(axis=0) - p_dev[ok]).max()
    lp0 = lp_no + full["log_likelihoods_no_dla"]
    lpd = (lp_dla + lld).T
    if sub:
        host = PR.model_posteriors_sub(lp0, lpd, pop["log_priors_lls"] + full["log_likelihoods_lls"])[0][:, 1:1 + D].T
    else:
        host = PR.model_posteriors_multi(lp0, lpd)[0][:, 1:1 + D].T
    assert np.array_equal(host[:, ok] == 0, P[:, ok] == 0)
    nzp = (host != 0) & ok[None, :]
    rel = (np.abs(P[nzp] - host[nzp]) / host[nzp]).max()
    print(f"D={D} sub={sub}: P_d device vs host: max relative difference {rel / 2.0 ** -53:.2f} x 2^-53; "
          f"|sum P_d - p_dla| {gap / 2.0 ** -53:.2f} x 2^-53")
    assert rel <= LEVEL_POSTERIOR_BOUND and gap <= SUM_BOUND
    assert np.all((P[0, ok] > 0.005) & (P[0, ok] < 0.995))
    # the far-separated spectrum: P_2 = 0 and zero planes at level 2
    assert np.isnan(far["log_likelihoods_dla"][1, 0]) and far["population_level_posteriors"][1, 0] == 0.0
    assert not far["bin_planes_levels"][0, 1:].any() and not far["population_level_poisson"][0, 1:].any()
    assert (far["population_level_large_inds"][0, 1:] == -1).all() and far["bin_planes_levels"][0, 0].any()
    # any split into device batches
    with Engine(model, samples, params, max_batch_spectra=2) as eng:
        batched = eng.process_levels(packed, D, **kw)
    for key in full:
        assert _same(full[key], batched[key]), key


def test_level_argument_errors():
    model = syn.make_model(k=4)
    samples = syn.make_samples(64)
    packed = syn.pack_spectra([syn.make_spectrum(model, 0, n_target=220)])
    lognhi = samples["log_nhi_samples"]
    good = dict(z_edges=P_EDGES_Z, log_nhi_edges=P_EDGES_N, log_nhi_samples=lognhi, log_priors_no_dla=[-0.1],
                log_priors_dla=[-2.3])
    lib = L.load()
    with Engine(model, samples, set_parameters(k=4)) as eng:
        assert eng.process_levels(packed, 1, population=good)["population_level_poisson"].shape == (1, 1, 7, 5)
        _raises_einval(eng.process_levels, packed, 1, population=dict(good, p_switch=0.1))
        _raises_einval(eng.process_levels, packed, 1, population=dict(good, z_edges=P_EDGES_Z[::-1].copy()))
        for bad in (("planes",), ("split", "planes"), ("every",)):      # no grid here; an unknown half
            with pytest.raises(ValueError):
                eng.process_levels(packed, 1, population=good, levels=bad)
        with pytest.raises(ValueError):
            eng.process_levels(packed, 1, levels=("split",))
        # the library's own checks of the struct, which come before anything is read
        sp, md, rs = L.Spectra(), L.MultiDla(), L.ResultsMulti()
        buf = np.zeros(8)
        for lv in (L.LevelPopulation(memory=L.MEM_HOST),                                     # no array at all
                   L.LevelPopulation(memory=L.MEM_HOST, bin_planes=L.ptr(buf)),              # planes without a grid
                   L.LevelPopulation(memory=L.MEM_HOST, level_posteriors=L.ptr(buf)),        # split without a spec
                   L.LevelPopulation(memory=7, bin_planes=L.ptr(buf))):
            assert lib.gpdla_engine_process_levels(eng._h, C.byref(sp), C.byref(md), None, C.byref(rs), None, None, None,
                                                   None, None, C.byref(lv)) == L.GPDLA_EINVAL
        n = C.c_int64(0)
        assert lib.gpdla_engine_get_level_population_stats(eng._h, None, C.byref(n)) == L.GPDLA_EINVAL
    # the stand-alone calls
    ll = np.zeros((2, 1, 64))
    base = np.zeros((1, 1, 64), dtype=np.int32)
    args = (samples["offset_samples"], lognhi, [2.0], [4.0])
    _raises_einval(population_split_levels, ll, *args, [[0.5], [1.5]], P_EDGES_Z, P_EDGES_N, base_sample_inds=base)
    _raises_einval(population_split_levels, ll, *args, [[0.5], [0.5]], P_EDGES_Z, P_EDGES_N)              # no base indices
    _raises_einval(population_split_levels, ll, *args, [[0.5], [0.5]], P_EDGES_Z, P_EDGES_N, base_sample_inds=base, p_switch=0.1)
    _raises_einval(population_split_levels, np.zeros((5, 1, 64)), *args, np.full((5, 1), 0.1), P_EDGES_Z, P_EDGES_N,
                   base_sample_inds=np.zeros((4, 1, 64), dtype=np.int32))
    _raises_einval(level_planes, ll, samples["offset_samples"], lognhi, samples["nhi_samples"], [2.0], [4.0],
                   P_EDGES_Z[::-1].copy(), P_EDGES_N, base_sample_inds=base)
    _raises_einval(level_planes, ll, samples["offset_samples"], lognhi, samples["nhi_samples"], [2.0], [4.0],
                   np.linspace(2.0, 4.0, 34), np.linspace(20.0, 23.0, 33), base_sample_inds=base)


# ------------------------------------------------------------------- 6. process_qsos
def test_process_qsos_levels_on_the_device():
    """max_dlas = 3 with summaries, population, levels="all" and no sample arrays: ``catalog.line_density(levels=
    "all")`` equals the oracle's curve from the same run's sample arrays (interval integers equal, curves within
    1e-12 relative, DESIGN.md section 15's bar)."""
    k, D = 4, 3
    model = syn.make_model(k=k)
    samples = syn.make_samples(S_LEVEL)
    packed = syn.pack_spectra(_spectra(model)[:3])
    params = set_parameters(k=k)
    rng = np.random.default_rng(3)
    prior = dict(z_qsos=rng.uniform(2.0, 4.5, 400), dla_ind=rng.uniform(size=400) < 0.12)
    grid = dict(z_edges=np.linspace(2.0, 4.0, 4), log_nhi_edges=np.linspace(20.0, 23.0, 3))
    pop = dict(z_edges=P_EDGES_Z, log_nhi_edges=P_EDGES_N)
    kw = dict(params=params, max_dlas=D)
    plain = PR.process_qsos(model, samples, packed, prior, summaries=grid, population=pop, **kw)
    full = PR.process_qsos(model, samples, packed, prior, summaries=dict(grid, levels="all"),
                           population=dict(pop, levels="all"), **kw)
    lean = PR.process_qsos(model, samples, packed, prior, summaries=dict(grid, levels="all"),
                           population=dict(pop, levels="all"), save_samples=False, **kw)
    for key in plain:
        assert _same(plain[key], full[key]), key
    assert set(full) - set(plain) == set(PR.LEVEL_POPULATION_VARIABLES)
    assert "sample_log_likelihoods_dla" not in lean and "base_sample_inds" not in lean
    for key in lean:
        assert _same(lean[key], full[key]), key
    assert np.abs(lean["population_level_posteriors"] - np.asarray(lean["model_posteriors"])[:, 1:1 + D]).max() <= LEVEL_POSTERIOR_BOUND
    # the oracle on the kept run's arrays, with the P_d the device formed
    rows = np.ascontiguousarray(np.transpose(full["sample_log_likelihoods_dla"], (2, 0, 1)))
    base = np.ascontiguousarray(np.transpose(full["base_sample_inds"], (2, 0, 1))).astype(np.int64) - 1
    want = LO.level_split(rows, base, full["min_z_dlas"], full["max_z_dlas"], full["population_level_posteriors"].T,
                          samples["offset_samples"], samples["log_nhi_samples"], P_EDGES_Z, P_EDGES_N)
    ref = dict(lean, **LO.one_based(want))
    assert _same(lean["population_level_large_inds"], ref["population_level_large_inds"])
    assert _same(lean["population_level_large_bins"], ref["population_level_large_bins"])
    for axis in ("z", "log_nhi"):
        got_ci, want_ci = (CAT.confidence_intervals(o, axis=axis, levels="all") for o in (lean, ref))
        assert all(np.array_equal(a, b) for a, b in zip(got_ci, want_ci)), axis       # the interval integers
    got, ref_curve = CAT.line_density(lean, levels="all"), CAT.line_density(ref, levels="all")
    assert _same(got[0], ref_curve[0]) and got[1].size >= 3
    for a, b in zip(got[1:4], ref_curve[1:4]):
        assert a.shape == b.shape and np.all(np.abs(a - b) <= 1e-12 * np.abs(b))
    assert got[3].sum() > 0          # the 95 % band is not empty

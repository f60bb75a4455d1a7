"""Omega_DLA from the column density function, the parts that need no GPU: the lattice against an exact
enumeration, ``split_distributions_grid`` against ``split_distributions``, and ``total_column_intervals`` /
``omega_dla_cddf`` through their ``mixture=`` and ``pmf=`` hooks against the reference's own
``_get_omega_confidence_intervals`` (tests/golden/omega_cddf.npz, made by
tests/golden/make_omega_cddf_fixture.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import count_mixture_oracle as CO  # noqa: E402
import population_oracle as PO  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402
from test_population import golden_out, oracle_split  # noqa: E402

GOLDEN = Path(__file__).parent / "golden"
TIE_GUARD = 1e-9


def recurrence(lists):
    return [PO.recurrence_pmf(v) for v in lists]


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN / "population.npz")
    return g, golden_out(g, oracle_split(g)), np.load(GOLDEN / "omega_cddf.npz")


@pytest.fixture(scope="module")
def golden_curve(golden):
    """``omega_dla_cddf`` on the golden population variables with the numpy lattice, once."""
    g, out, ref = golden
    gaps = []
    got = CAT.omega_dla_cddf(out, hubble=float(ref["hubble"]), cells=int(ref["cells"]), pmf=recurrence,
                             mixture=CO.mixture(CO.numpy_chain, gaps))
    return got, gaps


def random_problem(rng, stages, cells):
    """At most 6 taps per stage with arbitrary positive values (the first 0, as a stage's first kept count),
    the lattice step and shifts formed as ``total_column_intervals`` forms them."""
    probs, values = [], []
    for _ in range(stages):
        n = int(rng.integers(2, 7))
        p = rng.uniform(0.05, 1.0, n)
        probs.append(p / p.sum() * rng.uniform(0.995, 1.0))         # cut tails: the mass is below 1
        values.append(np.concatenate([[0.0], np.sort(rng.uniform(0.3, 40.0, n - 1))]) * 10.0 ** rng.uniform(20, 22))
    step = sum(v[-1] for v in values) / (cells - 1 - stages)
    shifts = [np.rint(v / step).astype(np.int64) for v in values]
    return probs, values, step, shifts


@pytest.mark.parametrize("stages,cells,seed", [(1, 64, 0), (2, 257, 1), (3, 300, 2), (4, 150, 3), (4, 1000, 4), (3, 40, 5)])
def test_lattice_lower_quantiles_within_the_rounding_bound(stages, cells, seed):
    """Each stage moves an atom by at most h / 2 (rint), so the lattice's atoms are the exact ones each moved by
    at most stages h / 2 with the same probabilities, and the lower quantile is 1-Lipschitz under such a
    coupling.  1e-9 h on top covers the float64 quotient value / h."""
    rng = np.random.default_rng(20261021 + seed)
    probs, values, step, shifts = random_problem(rng, stages, cells)
    assert sum(int(s[-1]) for s in shifts) < cells
    pmf = CO.lattice_chain(list(zip(probs, shifts)), cells)
    lower, upper, mass, gap = CO.levels_of(pmf, CAT.MIXTURE_LEVELS)
    atoms, weights = CO.exact_atoms(probs, values)
    assert gap > TIE_GUARD
    assert abs(mass - weights.sum()) < 1e-12 and abs(mass - np.prod([p.sum() for p in probs])) < 1e-12
    for lam, cell in zip(CAT.MIXTURE_LEVELS, lower):
        want, tie = CO.lower_quantile(atoms, weights, lam)
        assert tie > TIE_GUARD
        print(f"level {lam:.3f}: lattice {cell * step:.6e} exact {want:.6e} bound {stages * step / 2:.3e}")
        assert abs(cell * step - want) <= stages * step / 2 + 1e-9 * step
    assert np.all(upper >= lower)


def test_oracle_conventions():
    """The upper cell is one occupied cell past the first cell above the level, clamped to the last occupied
    one, as ``catalog._interval`` returns it for counts; two taps may land on one cell."""
    pmf = CO.lattice_chain([([0.2, 0.3, 0.5], [0, 2, 5])], 8)
    assert np.array_equal(pmf, [0.2, 0, 0.3, 0, 0, 0.5, 0, 0])
    lower, upper, mass, _ = CO.levels_of(pmf, (0.1, 0.4, 0.6, 0.99))
    assert lower.tolist() == [0, 2, 5, 5] and upper.tolist() == [2, 5, 5, 5] and mass == 1.0
    # the same answers in atom indices from the interval function for counts (tails 0.4 / 0.6, then 0.1 / 0.9)
    atoms, cdf = np.array([0, 2, 5]), np.cumsum([0.2, 0.3, 0.5])
    low, high = CAT._interval(cdf, 0.2)
    assert (atoms[low], atoms[min(high, 2)]) == (lower[1], upper[2])
    low, high = CAT._interval(cdf, 0.8)
    assert (atoms[low], atoms[min(high, 2)]) == (lower[0], CO.levels_of(pmf, (0.9,))[1][0])
    both = CO.lattice_chain([([0.25, 0.25, 0.5], [1, 1, 3]), ([1.0], [2])], 8)
    assert np.array_equal(both, [0, 0, 0, 0.5, 0, 0.5, 0, 0])
    assert np.array_equal(CO.numpy_chain([([0.25, 0.25, 0.5], [1, 1, 3]), ([1.0], [2])], 8), both)
    empty = CO.levels_of(np.zeros(4), (0.5,))
    assert empty[0].tolist() == [0] and empty[1].tolist() == [0] and empty[2] == 0.0


def test_grid_split_collapses_to_the_axis_split(golden):
    """Summed over z, the grid's cells are ``split_distributions(axis="log_nhi")``: the same trials (as a
    multiset: the axis split orders a bin spectrum by spectrum across z) and the same Poisson mean, the nz
    per-cell ``fsum``s each rounded once where the axis split rounds once in all."""
    g, out, _ = golden
    for keep in (None, np.arange(g["p_dlas"].size) % 5 != 1):
        lists, means = CAT.split_distributions_grid(out, keep=keep)
        want_lists, want_means = CAT.split_distributions(out, keep=keep, axis="log_nhi")
        nz, nn = means.shape
        assert (nz, nn) == (g["z_edges"].size - 1, g["log_nhi_edges"].size - 1) and len(lists) == nz
        for b in range(nn):
            got = np.sort(np.concatenate([lists[z][b] for z in range(nz)]))
            assert np.array_equal(got, np.sort(want_lists[b])), b
        assert np.all(np.abs(means.sum(axis=0) - want_means) <= (nz + 1) * 2.0 ** -53 * want_means)
        # and over log N_HI, the z split
        z_lists, z_means = CAT.split_distributions(out, keep=keep, axis="z")
        for z in range(nz):
            assert np.array_equal(np.sort(np.concatenate(lists[z])), np.sort(z_lists[z])), z
        assert np.all(np.abs(means.sum(axis=1) - z_means) <= (nn + 1) * 2.0 ** -53 * z_means)
    assert sum(v.size for row in lists for v in row) > 8 and (means > 0).sum() > 20


def check_against_reference(got, g, ref):
    """``omega_dla_cddf``'s output against the reference's recorded levels, each within twice the deviation the
    fixture maker measured for it (tests/golden/make_omega_cddf_fixture.py: the reference merges atoms within
    1e-3 of each other and lumps 5e-4 of either tail after every bin, which this package's lattice does not
    reproduce); where the reference's level is 0 (no DLA at that level), 0."""
    zc, omega, o68, o95, xerrs = got
    ez = g["z_edges"]
    path = g["ref_path_bins"] > 0
    assert np.array_equal(zc, ((ez[1:] + ez[:-1]) / 2)[path])
    assert np.array_equal(xerrs[0], (zc - ez[:-1][path])) and np.array_equal(xerrs[1], ez[1:][path] - zc)
    want = float(ref["ref_conversion"]) * ref["ref_levels"][path] / g["ref_path_bins"][path, None]
    have = np.stack([omega, o68[:, 0], o68[:, 1], o95[:, 0], o95[:, 1]], axis=1)
    # the path lengths: scipy.integrate.quad's 1.5e-8 per contributing spectrum (test_population.QUAD_ABS_TOL)
    path_rtol = g["p_dlas"].size * 1.5e-8 / g["ref_path_bins"][path]
    bar = 2 * ref["measured_rel_dev"][None, :] + path_rtol[:, None]
    assert np.array_equal(have == 0, want == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want > 0, np.abs(have - want) / want, 0.0)
    print("largest relative deviation per level", rel.max(axis=0), "allowed", 2 * ref["measured_rel_dev"])
    assert np.all(rel <= bar)
    assert (want[:, 0] > 0).sum() >= 6 and (want[:, 3] > 0).any()         # not all trivial
    assert np.all(o95[:, 0] <= o68[:, 0]) and np.all(o68[:, 0] <= omega) and np.all(omega <= o68[:, 1]) and np.all(o68[:, 1] <= o95[:, 1])


def test_omega_dla_cddf_against_the_reference(golden, golden_curve):
    """Measured by the fixture maker at 2^20 cells, per level (median, low 68, high 68, low 95, high 95):
    1.33e-3, 4.5e-4, 2.93e-3, 7.8e-4, 3.83e-2 (the last in a bin whose upper 95 % end sits on the reference's
    lumped upper tail); asserted at twice that."""
    g, out, ref = golden
    got, gaps = golden_curve
    assert min(gaps) > TIE_GUARD
    assert np.all(ref["measured_rel_dev"] < 0.05) and int(ref["cells"]) == 2 ** 20
    check_against_reference(got, g, ref)


def test_total_column_intervals_against_the_reference(golden):
    """``total_column_intervals`` itself, in N_HI units, and its pieces: the step, a bin without stages."""
    g, out, ref = golden
    lists, means = CAT.split_distributions_grid(out)
    mid, l68, l95, steps = CAT.total_column_intervals(lists, means, g["log_nhi_edges"], cells=int(ref["cells"]), pmf=recurrence,
                                                      mixture=CO.mixture(CO.numpy_chain))
    have = np.stack([mid, l68[:, 0], l68[:, 1], l95[:, 0], l95[:, 1]], axis=1)
    want = ref["ref_levels"]
    assert np.array_equal(have == 0, want == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want > 0, np.abs(have - want) / want, 0.0)
    assert np.all(rel <= 2 * ref["measured_rel_dev"][None, :])
    assert np.all(steps > 0) and np.all(steps * int(ref["cells"]) > l95[:, 1] - l95[:, 0])
    # nothing at all in a bin: every quantity 0, no stage, step 0; the hook sees one problem without stages
    seen = []

    def hook(*args):
        seen.append(args)
        return CO.mixture()(*args)
    nn = g["log_nhi_edges"].size - 1
    none = CAT.total_column_intervals([[np.zeros(0)] * nn], np.zeros((1, nn)), g["log_nhi_edges"], pmf=recurrence, mixture=hook, cells=16)
    assert [v.tolist() for v in none] == [[0.0], [[0.0, 0.0]], [[0.0, 0.0]], [0.0]]
    assert seen[0][3].tolist() == [0, 0] and seen[0][0].size == 0
    # two certain DLAs in one bin and nothing else: the column is exactly twice that bin's centre
    sure = [[np.zeros(0)] * nn]
    sure[0][3] = np.array([1.0, 1.0])
    two = CAT.total_column_intervals(sure, np.zeros((1, nn)), g["log_nhi_edges"], pmf=recurrence, mixture=hook, cells=16)
    c3 = 10.0 ** ((g["log_nhi_edges"][3] + g["log_nhi_edges"][4]) / 2)
    assert two[0][0] == 2 * c3 and two[1].tolist() == [[2 * c3, 2 * c3]] and seen[1][0].size == 0


def test_bad_arguments(golden):
    g, out, _ = golden
    lists, means = CAT.split_distributions_grid(out)
    en = g["log_nhi_edges"]
    kw = dict(pmf=recurrence, mixture=CO.mixture(CO.numpy_chain), cells=4096)
    lists, means = lists[3:5], means[3:5]
    CAT.total_column_intervals(lists[:2], means[:2], en, **kw)
    for bad in (dict(cells=0), dict(cells=3), dict(cells=2.5), dict(tail_prob=0.0), dict(tail_prob=0.05), dict(tail_prob=np.nan)):
        with pytest.raises(ValueError):
            CAT.total_column_intervals(lists[:2], means[:2], en, **dict(kw, **bad))
    with pytest.raises(ValueError):
        CAT.total_column_intervals(lists[:2], means[:1], en, **kw)
    with pytest.raises(ValueError):
        CAT.total_column_intervals(lists[:2], means[:2], en[:-1], **kw)
    with pytest.raises(ValueError):
        CAT.total_column_intervals(lists[:2], means[:2], en[::-1], **kw)
    with pytest.raises(ValueError):
        CAT.total_column_intervals(lists[:2], -means[:2], en, **kw)
    with pytest.raises(ValueError):
        CAT.omega_dla_cddf(out, levels="second", **kw)
    with pytest.raises(ValueError):
        CAT.split_distributions_grid(dict(out, p_dlas=out["p_dlas"][:-1]))
    with pytest.raises(KeyError):
        CAT.split_distributions_grid(out, levels="all")        # the level variables are not in a level-1 run

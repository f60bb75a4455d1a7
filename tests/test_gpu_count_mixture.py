"""The count mixture on the GPU (csrc/count_mixture.hip): the stage, scan and search kernels against the
``fsum`` oracle (count_mixture_oracle.py) with identical shifts at every tile and tap-pass edge, determinism,
the argument checks, and ``catalog.omega_dla_cddf`` on the device path against the reference's recorded levels
(tests/golden/omega_cddf.npz) and on a multi-DLA run."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import count_mixture_oracle as CO  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import count_mixture, count_mixture_tiling  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402
from test_count_mixture import TIE_GUARD, check_against_reference, recurrence  # noqa: E402
from test_gpu_population import P_EDGES_N, P_EDGES_Z, _spectra  # noqa: E402
from test_population import golden_out, oracle_split  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"
LEVELS = np.array(CAT.MIXTURE_LEVELS)


def _raises_einval(fn, *a, **kw):
    with pytest.raises(L.GpdlaError) as ei:
        fn(*a, **kw)
    assert ei.value.code == L.GPDLA_EINVAL, ei.value


def _stage(rng, taps, reach, pin=True):
    """``taps`` taps with non-decreasing shifts in [0, reach] (the largest exactly ``reach`` if ``pin``) and
    probabilities summing to just below 1."""
    shifts = np.sort(rng.integers(0, reach + 1, taps))
    if pin:
        shifts[-1] = reach
    p = rng.uniform(0.2, 1.0, taps)
    return p / p.sum() * rng.uniform(0.999, 1.0), shifts.astype(np.int64)


def _problem(rng, taps_per_stage, cells):
    """Stages whose largest shifts sum to exactly cells - 1: the last cell is reached."""
    cuts = np.sort(rng.integers(0, cells, len(taps_per_stage) - 1))
    reach = np.diff(np.concatenate([[0], cuts, [cells - 1]]))
    return [_stage(rng, m, int(r)) for m, r in zip(taps_per_stage, reach)]


def problems_for(cells, tile, taps):
    """Every tap count at a pass edge as the first of two stages, then the special shapes, then ragged problems
    of 1, 2 and 5 stages."""
    rng = np.random.default_rng(77000 + cells)
    out = [_problem(rng, (m, 3), cells) for m in (1, taps - 1, taps, taps + 1, 2 * taps + 1)]
    out.append([(np.array([1.0]), np.array([0]))])                                        # identity
    out.append([(np.array([0.75]), np.array([cells - 1]))])                               # one tap on the last cell
    out.append([(np.array([0.25, 0.3, 0.45]), np.array([0, 0, cells - 1]))])              # two taps on one cell
    if cells > tile:                                                                      # shifts that straddle a tile edge
        edge = np.array([tile - 2, tile - 1, tile, tile, min(tile + 1, cells - 1)])
        rest = cells - 1 - int(edge[-1])
        out.append([_stage(rng, 4, rest), (np.full(5, 0.2), edge)])
        out.append([(np.full(5, 0.2), edge), _stage(rng, taps + 3, rest, pin=False)])
    out += [_problem(rng, (5,), cells), _problem(rng, (2, 7), cells), _problem(rng, (3, 1, taps + 2, 2, 4), cells)]
    return out


@pytest.fixture(scope="module")
def tiling():
    t = count_mixture_tiling()
    assert t["tile"] % 256 == 0 and t["taps"] >= 1 and t["max_levels"] >= LEVELS.size
    return t


@pytest.mark.parametrize("which", ["one", "tile-1", "tile", "tile+1", "2tile+1"])
def test_kernels_against_the_fsum_oracle(tiling, which):
    """Every cell within 2 sum_s m_s 2^-53 relative of the oracle's (a cell is a chain of m_s non-negative FMAs
    per stage, one rounding each, on inputs that carry the earlier stages' bound; the oracle rounds each product
    and each ``fsum`` once); every level's lower and upper cell equal, the oracle's cdf no closer than 1e-9 to a
    level; the mass within (2 cells + 2 sum m_s) 2^-53 (the scan and the oracle's cumsum each add at most ``cells``
    non-negative terms).  Then the batch's problems alone and the batch again: bitwise."""
    tile, taps = tiling["tile"], tiling["taps"]
    cells = dict(zip(("one", "tile-1", "tile", "tile+1", "2tile+1"), (1, tile - 1, tile, tile + 1, 2 * tile + 1)))[which]
    problems = problems_for(cells, tile, taps)
    args = CO.to_csr(problems)
    lower, upper, mass, pmf = count_mixture(*args, cells, LEVELS, return_pmf=True)
    assert pmf.shape == (len(problems), cells) and lower.shape == upper.shape == (len(problems), LEVELS.size)
    for p, stages in enumerate(problems):
        want = CO.lattice_chain(stages, cells)
        bound = 2 * sum(len(pr) for pr, _ in stages) * 2.0 ** -53
        assert np.array_equal(pmf[p] == 0, want == 0), p
        nz = want > 0
        rel = np.abs(pmf[p][nz] - want[nz]) / want[nz]
        print(f"cells {cells} problem {p}: max rel {rel.max():.3e} of {bound:.3e}")
        assert rel.max() <= bound, p
        lo, up, m, gap = CO.levels_of(want, LEVELS)
        assert gap > TIE_GUARD, (p, gap)
        assert np.array_equal(lower[p], lo) and np.array_equal(upper[p], up), p
        assert abs(mass[p] - m) <= (2 * cells + bound / 2.0 ** -53) * 2.0 ** -53 * m, p
    assert np.array_equal(pmf[5], np.eye(1, cells)[0]) and mass[5] == 1.0          # the identity leaves the delta
    again = count_mixture(*args, cells, LEVELS, return_pmf=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, (lower, upper, mass, pmf)))
    for p in (0, 4, len(problems) - 1, len(problems) - 3):                           # alone; a 5-stage and a 1-stage one
        alone = count_mixture(*CO.to_csr([problems[p]]), cells, LEVELS, return_pmf=True)
        assert all(np.array_equal(a[0], b[p]) for a, b in zip(alone, (lower, upper, mass, pmf))), p


def test_ragged_batch_and_no_stage(tiling):
    """Three problems of 1, 2 and 5 stages and one without any (the delta itself), in every order of the batch:
    each bitwise what it is alone; no levels asked."""
    cells = tiling["tile"] + 77
    rng = np.random.default_rng(5)
    problems = [_problem(rng, (4,), cells), _problem(rng, (3, 3), cells), _problem(rng, (2, 3, 1, 5, 2), cells), []]
    alone = [count_mixture(*CO.to_csr([pr]), cells, LEVELS, return_pmf=True) for pr in problems]
    assert alone[3][2][0] == 1.0 and np.array_equal(alone[3][3][0], np.eye(1, cells)[0])
    assert not alone[3][0].any() and not alone[3][1].any()
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 3, 0, 1]):
        got = count_mixture(*CO.to_csr([problems[i] for i in order]), cells, LEVELS, return_pmf=True)
        for slot, i in enumerate(order):
            assert all(np.array_equal(g[slot], a[0]) for g, a in zip(got, alone[i])), (order, i)
    lower, upper, mass = count_mixture(*CO.to_csr(problems), cells, np.zeros(0))
    assert lower.shape == (4, 0) and np.array_equal(mass, [a[2][0] for a in alone])
    empty = count_mixture(np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64), 8, LEVELS)
    assert empty[0].shape == (0, LEVELS.size) and empty[2].shape == (0,)


def test_bad_arguments_are_einval():
    ok = dict(probs=[0.5, 0.5, 1.0], shifts=[0, 3, 2], tap_offsets=[0, 2, 3], stage_offsets=[0, 2], cells=6, levels=[0.5])

    def call(**kw):
        a = dict(ok, **kw)
        return count_mixture(a["probs"], a["shifts"], a["tap_offsets"], a["stage_offsets"], a["cells"], a["levels"])
    lower, upper, mass = call()                                      # summed largest shifts 5 = cells - 1: allowed
    assert lower.tolist() == [[2]] and upper.tolist() == [[5]] and mass[0] == 1.0
    _raises_einval(call, shifts=[3, 0, 2])                           # decreasing within a stage
    _raises_einval(call, shifts=[-1, 3, 2])                          # negative
    _raises_einval(call, shifts=[0, 3, -2])
    for bad in (-0.25, np.nan, np.inf, -np.inf):
        _raises_einval(call, probs=[0.5, bad, 1.0])
    _raises_einval(call, tap_offsets=[0, 3, 3])                      # an empty stage
    _raises_einval(call, tap_offsets=[0, 0, 3])
    for cells in (0, -4):
        _raises_einval(call, cells=cells)
    _raises_einval(call, cells=5)                                    # the summed largest shifts reach cells
    _raises_einval(call, shifts=[0, 3, 3])
    for level in (0.0, 1.0, -0.5, 1.5, np.nan):
        _raises_einval(call, levels=[0.5, level])
    _raises_einval(call, levels=np.full(9, 0.5))                     # more than GPDLA_MIX_MAX_LEVELS
    with pytest.raises(ValueError):
        call(tap_offsets=[0, 2])
    with pytest.raises(ValueError):
        call(shifts=[0, 2 ** 31, 2])


def test_omega_dla_cddf_on_the_device_against_the_reference():
    """The golden population variables through the device pmf and the device lattice at the fixture's 2^20 cells:
    the reference's recorded levels at the recorded tolerance (test_count_mixture.check_against_reference), and
    the same cells as the numpy restatement of the lattice."""
    g = np.load(GOLDEN / "population.npz")
    ref = np.load(GOLDEN / "omega_cddf.npz")
    out = golden_out(g, oracle_split(g))
    kw = dict(hubble=float(ref["hubble"]), cells=int(ref["cells"]))
    got = CAT.omega_dla_cddf(out, **kw)
    check_against_reference(got, g, ref)
    assert len(L.last_call_kernel_ms()) == 3
    gaps = []
    want = CAT.omega_dla_cddf(out, pmf=recurrence, mixture=CO.mixture(CO.numpy_chain, gaps), **kw)
    assert min(gaps) > TIE_GUARD
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4]))
    keep = np.arange(g["p_dlas"].size) % 4 != 2                       # an SNR-style mask moves the curve
    cut = CAT.omega_dla_cddf(out, keep=keep, **kw)
    assert cut[1].shape == got[1].shape and not np.array_equal(cut[1], got[1])


def test_levels_all_on_a_multi_dla_run():
    """``levels="all"`` on a max_dlas = 2 run of a few synthetic spectra: ordered bands, the device lattice equal
    to the numpy restatement on the same lists; and on a max_dlas = 1 run (D = 1) bitwise the ``levels="first"``
    answer."""
    k = 4
    model = syn.make_model(k=k)
    samples = syn.make_samples(257)
    packed = syn.pack_spectra(_spectra(model))
    rng = np.random.default_rng(3)
    prior = dict(z_qsos=rng.uniform(2.0, 4.5, 400), dla_ind=rng.uniform(size=400) < 0.12)
    pop = dict(z_edges=P_EDGES_Z, log_nhi_edges=P_EDGES_N, levels="all")
    cells = 2 ** 14
    for D in (2, 1):
        out = PR.process_qsos(model, samples, packed, prior, params=set_parameters(k=k), max_dlas=D, population=pop,
                              save_samples=False)
        every = CAT.omega_dla_cddf(out, levels="all", cells=cells)
        zc, omega, o68, o95, _ = every
        assert zc.size >= 3 and (o95[:, 1] > 0).any()
        assert np.all(o95[:, 0] <= o68[:, 0]) and np.all(o68[:, 0] <= omega) and np.all(omega <= o68[:, 1]) and np.all(o68[:, 1] <= o95[:, 1])
        gaps = []
        want = CAT.omega_dla_cddf(out, levels="all", cells=cells, pmf=recurrence, mixture=CO.mixture(CO.numpy_chain, gaps))
        assert min(gaps) > TIE_GUARD
        assert all(np.array_equal(a, b) for a, b in zip(every[:4], want[:4])), D
        first = CAT.omega_dla_cddf(out, levels="first", cells=cells)
        if D == 1:
            assert all(np.array_equal(a, b) for a, b in zip(every[:4], first[:4]))
        else:
            assert first[1].shape == omega.shape

"""Population statistics on the GPU (csrc/population.hip): the Poisson-binomial pmf kernel against an exact
rational oracle and against the reference's recorded ``get_poisson_binomial_pdf``; the split kernel against
the numpy oracle (population_oracle.py) and, through catalog.py, against the reference's own numbers
(tests/golden/population.npz); the engine call (bitwise against the stand-alone kernel, batching, multi-DLA,
sub-DLA, the device's p_dla against the host's) and ``process_qsos(population=...)``."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import population_oracle as PO  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import Engine, poisson_binomial_pmf_csr, population_split, posterior_summary  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402
from test_population import (GOLDEN, check_curves_against_reference, check_split_against_reference, golden_out,  # noqa: E402
                             oracle_split, reference_lists)

pytestmark = pytest.mark.gpu
CHUNK = L.PMF_CHUNK
POP_KEYS = ("population_poisson", "population_large_inds", "population_large_probs", "population_large_bins")


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _raises_einval(fn, *a, **kw):
    with pytest.raises(L.GpdlaError) as ei:
        fn(*a, **kw)
    assert ei.value.code == L.GPDLA_EINVAL, ei.value


# ---------------------------------------------------------------------------------------- 1. the pmf
def _draw(rng, n, bits=None):
    """n probabilities in [0, 1] with exact 0.0, 1.0 and 0.25 among them; ``bits`` rounds them to a 2^-bits
    grid (still doubles; it keeps the exact oracle's integers short at the largest size)."""
    p = rng.random(n)
    if bits is not None:
        p = np.round(p * 2.0 ** bits) / 2.0 ** bits
    for k, v in zip(rng.permutation(n)[:3], (0.0, 1.0, 0.25)):
        p[k] = v
    return p


def _check_pmf(lists):
    """The lists as one CSR batch with an empty bin between the first two, against the exact product: every
    coefficient above the smallest normal within 4 (n + 1) 2^-53 (three roundings per factor inside a chunk,
    one more per factor and one per chunk in a fold step, all terms non-negative: DESIGN.md section 15); and
    every bin bitwise what it is alone."""
    lists = [lists[0], np.zeros(0)] + list(lists[1:])
    got = CAT.poisson_binomial_pmf(lists)
    for v, pmf in zip(lists, got):
        n = v.size
        assert pmf.shape == (n + 1,) and np.all(pmf >= 0)
        rel = PO.relative_errors(pmf, PO.exact_pmf(v))
        worst = np.nanmax(rel)
        print(f"n={n}: max rel err {worst / 2.0 ** -53:.1f} x 2^-53 (bound {4 * (n + 1)})")
        assert worst <= 4 * (n + 1) * 2.0 ** -53, n
        assert _same(CAT.poisson_binomial_pmf([v])[0], pmf), n
    assert _same(got[1], [1.0])


def test_pmf_exact_small_and_chunk_edges():
    rng = np.random.default_rng(11)
    _check_pmf([_draw(rng, n) if n >= 3 else rng.random(n) for n in (0, 1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1)])
    assert _same(CAT.poisson_binomial_pmf([[0.25, 1.0, 0.0]])[0], [0.0, 0.75, 0.25, 0.0])
    assert CAT.poisson_binomial_pmf([]) == []


def test_pmf_exact_three_chunks_and_a_remainder():
    rng = np.random.default_rng(12)
    _check_pmf([_draw(rng, 3 * CHUNK + 37, bits=20), _draw(rng, 5)])


def test_pmf_against_the_reference_pdf():
    """The reference's DFT result is only good to its own noise floor, which depends on the host's libm and
    long double: the fixture maker recorded its worst deviation from the exact pmf, and ten times that is
    allowed here (absolute)."""
    g = np.load(GOLDEN)
    for name in ("nhi", "z"):
        o, pdfs = g[f"ref_{name}_offsets"], g[f"ref_{name}_pdfs"]
        lists = reference_lists(g, name)
        flat = poisson_binomial_pmf_csr(g[f"ref_{name}_probs"], o)
        assert flat.shape == pdfs.shape
        dev = np.abs(flat - pdfs).max()
        print(f"{name}: max abs deviation from the reference {dev:.3e} (its own {g['ref_pdf_worst_abs_deviation']:.3e})")
        assert dev <= 10 * g["ref_pdf_worst_abs_deviation"]
        assert max(v.size for v in lists) >= 3


def test_pmf_argument_errors():
    for bad in ([0.5, -1e-300], [0.5, 1.0000000000000002], [np.nan], [np.inf]):
        _raises_einval(CAT.poisson_binomial_pmf, [bad])
    lib = L.load()
    p, out = np.array([0.5, 0.5]), np.zeros(4)
    for offsets in ([1, 2], [0, 2, 1]):
        o = np.array(offsets, dtype=np.int64)
        assert lib.gpdla_poisson_binomial_pmf_f64(0, L.ptr(p), L.ptr(o, np.ctypeslib.ctypes.c_int64), o.size - 1,
                                                  L.ptr(out)) == L.GPDLA_EINVAL


# ------------------------------------------------------------------------------- 2. the split kernel
Z_EDGES, N_EDGES = np.linspace(1.9, 4.3, 8), np.linspace(20.0, 23.0, 6)


def _split_rows(S, rng):
    """Rows and their p_dla: smooth (Poisson plane only), peaked (a few large samples), one with p_dla below
    the spectrum threshold, all NaN, 20 % NaN, and -- from S = 4 -- four equal finite samples with p_dla = 1."""
    smooth = rng.normal(0.0, 1.0, S)
    peaked = rng.normal(0.0, 1.0, S) - 8.0
    peaked[rng.permutation(S)[:min(3, S)]] = (1.0, 0.4, 0.1)[:min(3, S)]
    low = rng.normal(0.0, 2.0, S)
    allnan = np.full(S, np.nan)
    nans = rng.normal(0.0, 3.0, S)
    nans[rng.random(S) < 0.2] = np.nan
    nans[rng.integers(S)] = 2.0
    rows, p = [smooth, peaked, low, allnan, nans], [0.83, 0.9990234375, 0.04, 0.7, 0.61]
    if S >= 4:
        four = np.full(S, np.nan)
        four[np.sort(rng.permutation(S)[:4])] = -3.5
        rows.append(four)
        p.append(1.0)
    return np.stack(rows), np.array(p)


@pytest.mark.parametrize("S", [1, 4, 255, 256, 257, 513, 1000])
def test_split_kernel_alone(S):
    rng = np.random.default_rng(700 + S)
    ll, p_dlas = _split_rows(S, rng)
    R = ll.shape[0]
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)     # every sample inside the log N_HI range
    min_z = np.linspace(2.0, 2.4, R)
    max_z = min_z + np.linspace(0.9, 1.8, R)
    kw = dict(p_thresh_sample=1e-4, p_switch=0.25)
    want = PO.split_rows(ll, min_z, max_z, p_dlas, offset, log_nhi, Z_EDGES, N_EDGES, **kw)
    # a condition on the inputs: no p_j close enough to a threshold for rounding to decide its class
    for r in range(R):
        p = p_dlas[r] * PO.masses(ll[r])
        for level in (1e-4, 0.25):
            if not (S >= 4 and r == 5):
                assert np.abs(p / level - 1.0).min() > 1e-9
    got = population_split(ll, offset, log_nhi, min_z, max_z, p_dlas, Z_EDGES, N_EDGES, **kw)
    assert got["population_poisson"].shape == (R, 7, 5) and got["population_large_inds"].dtype == np.int32
    assert np.array_equal(got["population_large_inds"], want["population_large_inds"])
    assert np.array_equal(got["population_large_bins"], want["population_large_bins"])
    # pi = w / W with W a sum of S non-negative terms and one exp each: the bin planes' bound
    tol = (S + 16) * 2.0 ** -52
    for key in ("population_large_probs", "population_poisson"):
        g, w = got[key], want[key]
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g == 0, w == 0), key
        ok = ~np.isnan(w)
        assert np.all(np.abs(g[ok] - w[ok]) <= tol * np.abs(w[ok])), key
    assert not got["population_poisson"][3].any() and (got["population_large_inds"][3] == -1).all()    # all NaN
    assert np.isnan(got["population_large_probs"][3]).all() and (got["population_large_bins"][3] == -1).all()
    if S >= 255:
        assert got["population_poisson"][0].any() and (got["population_large_inds"][1] >= 0).any()
        assert got["population_poisson"][2].any()         # p_dla <= 0.05 is the host stage's filter, not the kernel's
    if S >= 4:   # four equal samples: pi = 0.25 exactly, all four large, in index order, nothing in the plane
        assert got["population_large_inds"][5].tolist() == np.flatnonzero(~np.isnan(ll[5])).tolist() + [-1] * 4
        assert np.all(got["population_large_probs"][5, :4] == 0.25) and not got["population_poisson"][5].any()
    # two launches are one launch, bit for bit; and so are two calls
    again = population_split(ll, offset, log_nhi, min_z, max_z, p_dlas, Z_EDGES, N_EDGES, **kw)
    a = population_split(ll[:2], offset, log_nhi, min_z[:2], max_z[:2], p_dlas[:2], Z_EDGES, N_EDGES, **kw)
    b = population_split(ll[2:], offset, log_nhi, min_z[2:], max_z[2:], p_dlas[2:], Z_EDGES, N_EDGES, **kw)
    for key in POP_KEYS:
        assert _same(got[key], again[key]), key
        assert _same(got[key], np.concatenate([a[key], b[key]])), key


def test_four_equal_samples_inside_the_grid():
    """Four equal finite samples, all inside the grid, p_dla = 1: pi = 0.25 exactly, so all four are kept
    exactly (p >= p_switch = 0.25), in index order, and the Poisson plane stays zero."""
    S = 40
    ll = np.full((1, S), np.nan)
    idx = [3, 17, 18, 39]
    ll[0, idx] = -1234.5
    offset, log_nhi = np.linspace(0.05, 0.95, S), np.linspace(20.1, 22.9, S)
    got = population_split(ll, offset, log_nhi, [2.0], [4.0], [1.0], Z_EDGES, N_EDGES)
    assert got["population_large_inds"][0].tolist() == idx + [-1] * 4
    assert got["population_large_probs"][0, :4].tolist() == [0.25] * 4 and np.isnan(got["population_large_probs"][0, 4:]).all()
    assert (got["population_large_bins"][0, :4] >= 0).all() and not got["population_poisson"].any()
    # eight samples of pi = 1/8 fill the list at p_switch = 1/8, the smallest the call accepts
    ll[0, :] = np.nan
    ll[0, ::5] = 0.0
    got = population_split(ll, offset, log_nhi, [2.0], [4.0], [1.0], Z_EDGES, N_EDGES, p_switch=0.125)
    assert got["population_large_inds"][0].tolist() == list(range(0, S, 5))
    args = (ll, offset, log_nhi, [2.0], [4.0], [1.0])
    _raises_einval(population_split, *args, Z_EDGES, N_EDGES, p_switch=0.1249)
    _raises_einval(population_split, *args, Z_EDGES, N_EDGES, p_thresh_sample=0.25)
    _raises_einval(population_split, *args, Z_EDGES, N_EDGES, p_thresh_sample=-1e-12)
    _raises_einval(population_split, *args, Z_EDGES[::-1].copy(), N_EDGES)
    _raises_einval(population_split, *args, np.linspace(2.0, 4.0, 34), np.linspace(20.0, 23.0, 33))
    _raises_einval(population_split, ll, offset, log_nhi, [2.0], [4.0], [1.5], Z_EDGES, N_EDGES)


def test_golden_reference_numbers():
    """The split kernel on the fixture's rows and the pmf kernel on its lists, through catalog.py, against
    executed reference code: the same trials in the same bins, values at the bar test_population.py measured
    for the oracle, every interval integer equal, f(N), dN/dX and Omega_DLA with their bands."""
    g = np.load(GOLDEN)
    got = population_split(g["sample_log_likelihoods"], g["offset_samples"], g["log_nhi_samples"], g["min_z_dlas"],
                           g["max_z_dlas"], g["p_dlas"], g["z_edges"], g["log_nhi_edges"])
    want = oracle_split(g)
    assert np.array_equal(got["population_large_inds"], want["population_large_inds"])
    assert np.array_equal(got["population_large_bins"], want["population_large_bins"])
    planes = posterior_summary(g["sample_log_likelihoods"], g["offset_samples"], g["log_nhi_samples"], g["nhi_samples"],
                               g["min_z_dlas"], g["max_z_dlas"], z_edges=g["z_edges"],
                               log_nhi_edges=g["log_nhi_edges"])["bin_planes"]
    out = golden_out(g, got, planes)
    worst = check_split_against_reference(g, out)
    print(f"kernel vs reference: max rel deviation {worst:.3e}")
    check_curves_against_reference(g, out, None)          # None: the device pmf


# ------------------------------------------------------------------------------------------ 3. engine
S_LEVEL = 257
P_EDGES_Z, P_EDGES_N = np.linspace(1.6, 4.6, 8), np.linspace(20.0, 23.0, 6)
MULTI_KEYS = ("log_likelihoods_no_dla", "log_likelihoods_dla", "min_z_dlas", "max_z_dlas", "num_pixels",
              "sample_log_likelihoods_dla")
# |device p_dla - host p_dla|.  Worst case by construction: each side's p_no = e_0 / sum e_m carries one exp
# (1 ulp = 2^-52 relative at worst, both libraries), a sum of at most 6 non-negative terms (each with its own
# exp) and a quotient -- (2 + 2 + 5 + 1) 2^-53 relative each, 20 2^-53 between them with p_no <= 1 -- and
# 1 - p_no (- p_lls, the same again) rounds once more on either side: 48 2^-53 in all.  Measured on the MI355X
# over the four engine cases below: 1.0 x 2^-53.  The bar is a few ulp over the
# measured value and inside the worst case.
P_DLA_BOUND = 8 * 2.0 ** -53


def _spectra(model):
    mk = dict(mask_fraction=0.05)
    return [syn.make_spectrum(model, 0, z_qso=2.6, n_target=300, **mk),
            syn.make_spectrum(model, 1, z_qso=3.1, n_target=None, **mk),
            syn.make_spectrum(model, 2, n_target=270, **mk),
            syn.make_spectrum(model, 3, n_target=300, mask_fraction=1.0),      # J = 0: NaN rows
            syn.make_spectrum(model, 4, z_qso=2.9, n_target=280, **mk)]


@pytest.mark.parametrize("D,sub", [(1, False), (2, False), (1, True), (2, True)])
def test_engine_population(D, sub):
    k = 4
    model = syn.make_model(k=k)
    samples = syn.make_samples(S_LEVEL)
    packed = syn.pack_spectra(_spectra(model))
    params = set_parameters(k=k)
    Q = 5
    lognhi = samples["log_nhi_samples"]
    skw = dict(sub_dla=samples["nhi_samples"] * 0.02) if sub else {}
    with Engine(model, samples, params) as eng:
        plain = eng.process_models(packed, D, **skw)
        null = eng.process_population(packed, D, population=None, **skw)
        for key in plain:                                   # both structs NULL: that call, bit for bit
            assert _same(plain[key], null[key]), key
        assert list(plain) == list(null)
        # priors that leave the models comparable, so p_dla is not just 0 or 1
        lld = plain["log_likelihoods_dla"]
        shift = np.array([0.3, -1.1, 2.0, 0.0, -0.2])
        lp_no = np.full(Q, -0.25)
        lp_dla = np.stack([plain["log_likelihoods_no_dla"] - lld[d] + shift - 0.4 * d for d in range(D)])
        lp_dla[:, 3] = -1.0                                 # the masked spectrum's evidences are NaN anyway
        pop = dict(z_edges=P_EDGES_Z, log_nhi_edges=P_EDGES_N, log_nhi_samples=lognhi, log_priors_no_dla=lp_no,
                   log_priors_dla=lp_dla)
        if sub:
            pop["log_priors_lls"] = plain["log_likelihoods_no_dla"] - plain["log_likelihoods_lls"] - 0.7
            pop["log_priors_lls"][3] = -2.0
        full = eng.process_population(packed, D, population=pop, **skw)
        again = eng.process_population(packed, D, population=pop, want_samples=False, **skw)
        dev = eng.process_population(packed, D, population=pop, memory="device", **skw)
        both = eng.process_population(packed, D, population=pop, log_nhi_samples=lognhi,
                                      z_edges=np.linspace(2.0, 4.0, 4), log_nhi_edges=np.linspace(20.0, 23.0, 3), **skw)
        stats = eng.population_stats()
    assert stats["population_launches"] == 4 and stats["population_ms"] > 0
    for key in plain:                                       # every other result unchanged
        assert _same(plain[key], full[key]), key
    assert set(full) - set(plain) == set(POP_KEYS) | {"population_p_dlas"}
    assert "sample_log_likelihoods_dla" not in again and both["bin_planes"].shape == (Q, 5, 3, 2)
    for other in (again, dev, both):
        for key in POP_KEYS + ("population_p_dlas",):
            assert _same(full[key], other[key]), key
    # ... and the population outputs are the stand-alone kernel on the rows and the p_dla the run returned
    p_dev = full["population_p_dlas"]
    rows = full["sample_log_likelihoods_dla"][0]
    ok = ~np.isnan(p_dev)
    assert ok.tolist() == [True, True, True, False, True]
    alone = population_split(rows[ok], samples["offset_samples"], lognhi, full["min_z_dlas"][ok], full["max_z_dlas"][ok],
                             p_dev[ok], P_EDGES_Z, P_EDGES_N)
    for key in POP_KEYS:
        assert _same(full[key][ok], alone[key]), key
        assert _same(full[key][3], np.zeros_like(full[key][3]) if key == "population_poisson" else
                     np.full_like(full[key][3], np.nan if key == "population_large_probs" else -1)), key
    assert full["population_poisson"][ok].any()
    # the device's p_dla against the host's expression on the same evidences
    lp0 = lp_no + full["log_likelihoods_no_dla"]
    lpd = (lp_dla + lld).T
    if sub:
        host = PR.model_posteriors_sub(lp0, lpd, pop["log_priors_lls"] + full["log_likelihoods_lls"])[3]
    else:
        host = PR.model_posteriors_multi(lp0, lpd)[2]
    diff = np.abs(p_dev[ok] - host[ok]).max()
    print(f"D={D} sub={sub}: p_dla device vs host: max abs difference {diff:.3e} ({diff / 2.0 ** -53:.1f} x 2^-53)")
    assert np.isnan(host[3]) and diff <= P_DLA_BOUND
    assert np.all((p_dev[ok] > 0.02) & (p_dev[ok] < 0.98))
    # any split into device batches
    with Engine(model, samples, params, max_batch_spectra=2) as eng:
        batched = eng.process_population(packed, D, population=pop, **skw)
    for key in MULTI_KEYS + POP_KEYS + ("population_p_dlas",):
        assert _same(full[key], batched[key]), key


def test_engine_population_argument_errors():
    model = syn.make_model(k=4)
    samples = syn.make_samples(64)
    packed = syn.pack_spectra([syn.make_spectrum(model, 0, n_target=220)])
    good = dict(z_edges=P_EDGES_Z, log_nhi_edges=P_EDGES_N, log_nhi_samples=samples["log_nhi_samples"],
                log_priors_no_dla=[-0.1], log_priors_dla=[-2.3])
    with Engine(model, samples, set_parameters(k=4)) as eng:
        assert eng.process_population(packed, 1, population=good)["population_poisson"].shape == (1, 7, 5)
        for change in (dict(p_switch=0.1), dict(p_thresh_sample=0.3), dict(z_edges=P_EDGES_Z[::-1].copy()),
                       dict(log_nhi_edges=[20.0, np.nan]), dict(z_edges=np.linspace(2, 4, 34), log_nhi_edges=np.linspace(20, 23, 33))):
            _raises_einval(eng.process_population, packed, 1, population=dict(good, **change))
        with pytest.raises(ValueError):
            eng.process_population(packed, 1, population=dict(good, bins=3))
        with pytest.raises(ValueError):
            eng.process_population(packed, 1, population=dict(good, log_priors_dla=[-2.3, -1.0]))
        with pytest.raises(ValueError):      # the sub-DLA model needs its prior
            eng.process_population(packed, 1, population=good, sub_dla=samples["nhi_samples"] * 0.02)


# ------------------------------------------------------------------------------- 4. process_qsos
def test_process_qsos_population_without_sample_arrays():
    """population with max_dlas = 2, summaries and save_samples=False: everything that was there is unchanged
    bit for bit, the population variables equal the stand-alone kernel on the kept run's rows, and the host's
    p_dlas agree with the device's."""
    k, D = 4, 2
    model = syn.make_model(k=k)
    samples = syn.make_samples(S_LEVEL)
    packed = syn.pack_spectra(_spectra(model)[:3])
    params = set_parameters(k=k)
    rng = np.random.default_rng(3)
    prior = dict(z_qsos=rng.uniform(2.0, 4.5, 400), dla_ind=rng.uniform(size=400) < 0.12)
    grid = dict(z_edges=np.linspace(2.0, 4.0, 4), log_nhi_edges=np.linspace(20.0, 23.0, 3))
    pop = dict(z_edges=P_EDGES_Z, log_nhi_edges=P_EDGES_N)
    kw = dict(params=params, max_dlas=D, summaries=grid)
    plain = PR.process_qsos(model, samples, packed, prior, **kw)
    full = PR.process_qsos(model, samples, packed, prior, population=pop, **kw)
    lean = PR.process_qsos(model, samples, packed, prior, population=pop, save_samples=False, **kw)
    one = PR.process_qsos(model, samples, packed, prior, params=params, population=pop)
    base = PR.process_qsos(model, samples, packed, prior, params=params)
    for key in plain:
        assert _same(plain[key], full[key]), key
    for key in base:
        assert _same(base[key], one[key]), key
    assert set(full) - set(plain) == set(one) - set(base) == set(PR.POPULATION_VARIABLES)
    assert "sample_log_likelihoods_dla" not in lean and "base_sample_inds" not in lean
    for key in lean:
        assert _same(lean[key], full[key]), key
    ok = ~np.isnan(full["population_p_dlas"])
    assert np.abs(full["population_p_dlas"][ok] - full["p_dlas"][ok]).max() <= P_DLA_BOUND
    alone = population_split(full["sample_log_likelihoods_dla"][:, :, 0], samples["offset_samples"], samples["log_nhi_samples"],
                             full["min_z_dlas"], full["max_z_dlas"], full["population_p_dlas"], P_EDGES_Z, P_EDGES_N)
    assert _same(lean["population_poisson"], alone["population_poisson"])
    assert _same(lean["population_large_inds"], alone["population_large_inds"] + 1.0)
    assert _same(lean["population_large_bins"], alone["population_large_bins"] + 1.0)
    assert _same(lean["population_large_probs"], alone["population_large_probs"])
    lists, means = CAT.split_distributions(lean, axis="z")
    assert len(lists) == 7 and means.shape == (7,)

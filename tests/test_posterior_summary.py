"""Posterior summaries, the parts that need no GPU: the numpy oracle (posterior_summary_oracle.py) and
``catalog.cddf_moments`` against the reference's own ``_get_z_nhi_hist`` / ``find_max_like`` numbers
(tests/golden/posterior_summary.npz, made by tests/golden/make_posterior_summary_fixture.py), the ASCII
catalogue's formats, and ``process_qsos(summaries=...)`` with an injected compute."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import multi_dla_oracle as MO  # noqa: E402
import posterior_summary_oracle as PO  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402
from gp_dla_detection_amd import matv73 as M  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402

GOLDEN = Path(__file__).parent / "golden" / "posterior_summary.npz"
# 10 x the largest relative deviation of oracle + cddf_moments from the reference's numbers, measured
# here at 1.34e-13 (the reference normalises with l - (log-mean-exp + log S), this package with w / W)
REFERENCE_BAR = 1.34e-12


def golden_planes(g, planes_of_row):
    return np.stack([planes_of_row(q) for q in range(g["sample_log_likelihoods"].shape[0])])


def check_against_reference(g, planes, bar=REFERENCE_BAR):
    """cddf_moments of ``planes`` against the reference's four histograms; returns the largest relative
    deviation."""
    worst = 0.0
    for moment in (False, True):
        means, variances = CAT.cddf_moments(planes, g["p_dlas"], moment=moment)
        assert means.shape == variances.shape == (6, 6)
        for nhi, axis in ((0, 1), (1, 0)):       # z histogram: summed over log N_HI, and the reverse
            ref = g[f"ref_nhi{nhi}_moment{int(moment)}"]
            for got, want in ((means.sum(axis=axis), ref[0]), (variances.sum(axis=axis), ref[1])):
                assert np.all(want > 0)
                rel = np.abs(got - want) / want
                print(f"nhi={nhi} moment={moment}: max rel deviation {rel.max():.3e}")
                worst = max(worst, float(rel.max()))
                assert rel.max() <= bar
    return worst


def test_oracle_and_moments_match_the_reference():
    """Measured: 1.34e-13 largest relative deviation over the 4 x 2 x 6 reference numbers; the bar is
    10 x that (REFERENCE_BAR), far below the 1e-9 ceiling.  The MAP pairs of the NaN-free rows equal
    find_max_like's bit for bit."""
    assert REFERENCE_BAR <= 1e-9
    g = np.load(GOLDEN)
    ll = g["sample_log_likelihoods"]
    planes = golden_planes(g, lambda q: PO.bin_planes(
        ll[q], g["min_z_dlas"][q], g["max_z_dlas"][q], g["offset_samples"], g["log_nhi_samples"], g["nhi_samples"],
        g["z_edges"], g["log_nhi_edges"])[0])
    worst = check_against_reference(g, planes)
    assert worst > 0      # not a tautology: two different normalisations
    _, _, z, n = PO.map_parameters(ll[None], None, g["min_z_dlas"], g["max_z_dlas"], g["offset_samples"],
                                   g["log_nhi_samples"])
    rows = g["map_rows"]
    assert np.array_equal(n[0, rows, 0], g["ref_max_like"][:, 0])
    assert np.array_equal(z[0, rows, 0], g["ref_max_like"][:, 1])
    assert np.isnan(z[0, :, 1:]).all()


def test_moments_filter_and_formula():
    rng = np.random.default_rng(2)
    planes = rng.uniform(0.0, 1.0, (5, 5, 2, 3))
    p = np.array([0.9, 0.05, 0.5, 0.04, 0.7])          # 0.05 itself is out: the reference's strict >
    keep = np.array([True, True, False, True, True])
    m, v = CAT.cddf_moments(planes, p, keep=keep)
    want_m = 0.9 * planes[0, 0] + 0.7 * planes[4, 0]
    want_v = (0.9 * planes[0, 0] - 0.81 * planes[0, 1]) + (0.7 * planes[4, 0] - 0.7 * 0.7 * planes[4, 1]) + want_m
    np.testing.assert_allclose(m, want_m, rtol=1e-15)
    np.testing.assert_allclose(v, want_v, rtol=1e-14)
    m2, v2 = CAT.cddf_moments(planes, p, keep=keep, moment=True)
    np.testing.assert_allclose(m2, 0.9 * planes[0, 2] + 0.7 * planes[4, 2], rtol=1e-15)
    np.testing.assert_allclose(v2, 0.9 * planes[0, 3] - 0.81 * planes[0, 4] + 0.7 * planes[4, 3] - 0.49 * planes[4, 4] + m2,
                               rtol=1e-14)
    m3, _ = CAT.cddf_moments(planes, p, p_thresh_spec=0.0)             # every spectrum passes the threshold
    np.testing.assert_allclose(m3, np.tensordot(p, planes[:, 0], axes=1), rtol=1e-15)
    with pytest.raises(ValueError):
        CAT.cddf_moments(planes[:, :4], p)


def test_oracle_edge_rules():
    assert PO.map_index([np.nan, 1.0, 3.0, 3.0, np.nan]) == 2          # the first maximum
    assert PO.map_index([np.nan, np.nan]) == -1
    assert PO.map_index([-np.inf, -np.inf]) == 0
    assert np.array_equal(PO.masses([-np.inf, -np.inf]), [0.0, 0.0])
    assert np.array_equal(PO.masses([np.nan, 0.0, np.nan, 0.0]), [0.0, 0.5, 0.0, 0.5])
    assert PO.bin_index([1.0, 2.0, 3.0], [0.5, 1.0, 1.5, 2.0, 3.0, np.nan]).tolist() == [-1, 0, 0, 1, -1, -1]
    base = np.array([[[1, -1, 0]], [[2, 0, 1]]])                        # levels 2 and 3 of one row
    ll = np.array([[[0.0, 1.0, 0.5]], [[0.0, 1.0, 2.0]], [[5.0, 1.0, 2.0]]])
    inds, mll, z, n = PO.map_parameters(ll, base, [2.0], [3.0], [0.0, 0.5, 1.0], [20.0, 21.0, 22.0])
    assert inds[:, 0].tolist() == [1, 2, 0] and mll[:, 0].tolist() == [1.0, 2.0, 5.0]
    assert np.array_equal(z[0, 0], [2.5, np.nan, np.nan, np.nan], equal_nan=True)
    assert np.array_equal(n[1, 0], [22.0, 20.0, np.nan, np.nan], equal_nan=True)      # level 2: sample 2 on base 0
    assert np.array_equal(z[2, 0], [2.0, 3.0, 2.0, np.nan], equal_nan=True)           # level 3: 0 -> 2 -> 0
    ll[2, 0, 0] = -1.0                                                               # MAP 2 -> base 1 -> -1
    assert np.isnan(PO.map_parameters(ll, base, [2.0], [3.0], [0.0, 0.5, 1.0], [20.0, 21.0, 22.0])[2][2]).all()


# ------------------------------------------------------------------------------------ ASCII catalogue
def test_ascii_catalog_formats(tmp_path):
    """Literal lines from generate_ascii_catalog.m's format strings: widths, signs, zero padding, the
    exponent rewrite (two digits -> three, three left alone), the four flag bits, the id-only prefix of
    a results line (the reference's line 57), NaN spelled as MATLAB spells it."""
    catalog = dict(thing_ids=np.array([12345, 987654321, 7]), sdss_names=np.array(["003712.49+001513.1  ", "J1", "x"], dtype=object),
                   plates=np.array([266, 7000, 1]), mjds=np.array([51630, 56789, 2]), fiber_ids=np.array([5, 1000, 3]),
                   ras=np.array([9.3020417, 187.5, 0.0]), decs=np.array([0.2536389, -5.25, 1.0]),
                   z_qsos=np.array([2.5, 3.12345, 0.5]), snrs=np.array([7.125, 123.45678, 0.0]),
                   filter_flags=np.array([0, 5, 10]))
    samples = dict(offset_samples=np.array([0.5, 0.123456789]), log_nhi_samples=np.array([20.123456789, 22.5]))
    out = dict(test_ind=np.array([True, False, True]), min_z_dlas=np.array([2.1, 0.3]), max_z_dlas=np.array([2.45, 0.49]),
               log_priors_no_dla=np.array([-0.105361, -0.5]), log_priors_dla=np.array([-2.302585, -12.25]),
               log_likelihoods_no_dla=np.array([-1234.5678, 1.5e-7]), log_likelihoods_dla=np.array([-1200.25, np.nan]),
               model_posteriors=np.array([[1.23456e-4, 0.999876544], [1.0, 2.5e-120]]),
               MAP_z_dlas=np.array([[2.25, np.nan], [np.nan, np.nan]]), MAP_log_nhis=np.array([[21.25, np.nan], [np.nan, np.nan]]))
    paths = CAT.write_ascii_catalog(str(tmp_path / "processed"), "dr12q", catalog, samples, out)
    assert [Path(p).name for p in paths] == ["dr12q_dla_samples.dat", "dr12q_spectra.dat", "dr12q_results.dat"]
    assert Path(paths[0]).read_text() == "0.500000 20.123457\n0.123457 22.500000\n"
    assert Path(paths[1]).read_text().splitlines() == [
        "000012345 003712.49+001513.1 0266 51630 0005 009.3020417 +00.2536389 2.5000 007.1250 0000",
        "987654321 J1                 7000 56789 1000 187.5000000 -05.2500000 3.1235 123.4568 1010",
        "000000007 x                  0001 00002 0003 000.0000000 +01.0000000 0.5000 000.0000 0101"]
    assert Path(paths[2]).read_text().splitlines() == [
        "000012345 2.1000 2.4500 -0.10536 -2.30259 -1.23457e+03 -1.20025e+03 1.23456e-004 9.99877e-001 2.2500 21.2500",
        "000000007 0.3000 0.4900 -0.50000 -12.25000  1.50000e-07          NaN 1.00000e+000 2.50000e-120    NaN     NaN"]


# ------------------------------------------------------------------------- process_qsos(summaries=...)
K, S, Q = 4, 24, 3
Z_EDGES, N_EDGES = np.linspace(1.5, 4.5, 4), np.linspace(20.0, 23.0, 3)


def summary_compute(calls):
    """A ``compute`` replacement: the multi-DLA oracle for the likelihoods, the summary oracle on its
    sample arrays for the rest, honouring the keywords process_qsos passes."""
    def compute(model, samples, packed, params, device=0, max_dlas=1, summaries=None, save_samples=True):
        calls.append(dict(max_dlas=max_dlas, summaries=summaries, save_samples=save_samples))
        res = MO.compute(model, samples, packed, params, device, max_dlas=max_dlas)
        if max_dlas == 1:
            sll, base = res["sample_log_likelihoods_dla"][None], None
        else:
            sll, base = res["sample_log_likelihoods_dla"], res["base_sample_inds"]
        if summaries is not None:
            inds, mll, z, n = PO.map_parameters(sll, base, res["min_z_dlas"], res["max_z_dlas"],
                                                samples["offset_samples"], samples["log_nhi_samples"])
            res.update(map_sample_inds=inds, map_log_likelihoods=mll, MAP_z_dlas=z[:, :, :max_dlas],
                       MAP_log_nhis=n[:, :, :max_dlas])
            if isinstance(summaries, dict):
                res["bin_planes"] = np.stack([PO.bin_planes(
                    sll[0, q], res["min_z_dlas"][q], res["max_z_dlas"][q], samples["offset_samples"],
                    samples["log_nhi_samples"], samples["nhi_samples"], summaries["z_edges"],
                    summaries["log_nhi_edges"])[0] for q in range(sll.shape[1])])
        if not save_samples:
            res.pop("sample_log_likelihoods_dla", None)
            res.pop("base_sample_inds", None)
        return res
    return compute


@pytest.fixture(scope="module")
def setup():
    model = syn.make_model(k=K)
    samples = syn.make_samples(S)
    spectra = [syn.make_spectrum(model, q, n_target=120, mask_fraction=0.05, dla_fraction=1.0) for q in range(Q)]
    rng = np.random.default_rng(5)
    prior = dict(z_qsos=rng.uniform(2.0, 4.5, 400), dla_ind=rng.uniform(size=400) < 0.12)
    return dict(model=model, samples=samples, packed=syn.pack_spectra(spectra), params=set_parameters(k=K), prior=prior)


def run(s, calls=None, **kw):
    calls = [] if calls is None else calls
    return PR.process_qsos(s["model"], s["samples"], s["packed"], s["prior"], params=s["params"],
                           compute=summary_compute(calls), **kw)


def test_process_qsos_default_is_unchanged(setup):
    """summaries=None: the compute replacement sees no new keyword and the output is today's, key for
    key and bit for bit (against the multi-DLA tests' own compute, which takes none of the keywords)."""
    s = setup
    for D in (1, 2):
        calls = []
        got = run(s, calls, max_dlas=D)
        want = PR.process_qsos(s["model"], s["samples"], s["packed"], s["prior"], params=s["params"], max_dlas=D,
                               compute=MO.compute)
        assert calls == [dict(max_dlas=D, summaries=None, save_samples=True)]
        assert list(got) == list(want)
        for key in want:
            assert np.array_equal(np.asarray(got[key]), np.asarray(want[key]), equal_nan=True), key
        assert not set(got) & set(PR.SUMMARY_VARIABLES)


@pytest.mark.parametrize("D", [1, 3])
def test_process_qsos_summaries(setup, tmp_path, D):
    s = setup
    grid = dict(z_edges=Z_EDGES, log_nhi_edges=N_EDGES)
    plain = run(s, max_dlas=D)
    calls = []
    out = run(s, calls, max_dlas=D, summaries=grid)
    assert calls[0]["summaries"] is grid and calls[0]["save_samples"] is True
    for key in plain:                                         # nothing that was there moves
        assert np.array_equal(np.asarray(out[key]), np.asarray(plain[key]), equal_nan=True), key
    assert set(out) - set(plain) == set(PR.SUMMARY_VARIABLES)
    assert out["MAP_z_dlas"].shape == out["MAP_log_nhis"].shape == out["map_sample_inds"].shape == (Q, D)
    assert out["bin_planes"].shape == (Q, 5, 3, 2)
    assert np.array_equal(out["bin_z_edges"], Z_EDGES) and np.array_equal(out["bin_log_nhi_edges"], N_EDGES)
    # level selection: the DLA model with the highest posterior gives the row, with that many pairs
    level = np.argmax(out["model_posteriors"][:, 1:], axis=1)
    sll = out["sample_log_likelihoods_dla"].reshape(Q, S, D)
    for q in range(Q):
        d = level[q]
        assert np.isfinite(out["MAP_z_dlas"][q, :d + 1]).all() and np.isnan(out["MAP_z_dlas"][q, d + 1:]).all()
        j = int(out["map_sample_inds"][q, d]) - 1             # 1-based in the output, like base_sample_inds
        assert j == PO.map_index(sll[q, :, d])
        assert out["MAP_log_nhis"][q, 0] == s["samples"]["log_nhi_samples"][j]
        assert out["MAP_z_dlas"][q, 0] == out["min_z_dlas"][q] + (out["max_z_dlas"][q] - out["min_z_dlas"][q]) * \
            s["samples"]["offset_samples"][j]
    assert out["map_sample_inds"].min() >= 1 and out["map_sample_inds"].dtype == np.float64
    # MAP only
    only = run(s, max_dlas=D, summaries=True)
    assert set(only) - set(plain) == {"MAP_z_dlas", "MAP_log_nhis", "map_sample_inds"}
    assert np.array_equal(only["MAP_z_dlas"], out["MAP_z_dlas"], equal_nan=True)
    # without the sample arrays: the same summaries, and a file that holds none
    calls = []
    lean = run(s, calls, max_dlas=D, summaries=grid, save_samples=False)
    assert calls[0]["save_samples"] is False
    assert set(out) - set(lean) == {"sample_log_likelihoods_dla"} | ({"base_sample_inds"} if D > 1 else set())
    for key in lean:
        assert np.array_equal(np.asarray(lean[key]), np.asarray(out[key]), equal_nan=True), key
    lean["test_ind"] = np.ones(Q, dtype=bool)
    path = tmp_path / "processed_qsos_lean.mat"
    PR.save_processed_qsos(str(path), lean)
    r = M.loadmat(str(path))
    assert "sample_log_likelihoods_dla" not in r and "base_sample_inds" not in r
    for key in ("log_likelihoods_dla", "model_posteriors", "p_dlas", "MAP_z_dlas", "MAP_log_nhis", "map_sample_inds",
                "bin_planes"):
        want = np.asarray(lean[key])
        assert np.array_equal(np.asarray(r[key]).reshape(want.shape), want, equal_nan=True), key
    assert r["bin_planes"].shape == (Q, 5, 3, 2)
    assert np.array_equal(np.ravel(r["bin_z_edges"]), Z_EDGES)


def test_summary_arguments(setup, tmp_path):
    s = setup
    with pytest.raises(ValueError):
        run(s, summaries=dict(z_edges=Z_EDGES))
    with pytest.raises(ValueError):
        run(s, summaries=dict(z_edges=Z_EDGES, log_nhi_edges=N_EDGES, bins=3))
    for kw in (dict(summaries=True), dict(save_samples=False)):
        with pytest.raises(NotImplementedError):
            PR.run_process_qsos(str(tmp_path), "dr12q", "a", "b", None, "dr12q", "dr12q", None, world=2, **kw)

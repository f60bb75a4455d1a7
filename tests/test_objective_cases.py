"""The objective's case table (tests/objective_cases.py) reaches what it is named for, its constants are
objective.hip's, its dense long-double reference is right on its own terms, and on every case judged by
that reference the double oracle agrees with it to a tenth of the GPU bars.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy.linalg import LinAlgError, cholesky
from scipy.stats import multivariate_normal

sys.path.insert(0, str(Path(__file__).parent))
import forest_training_oracle as FO  # noqa: E402
import objective_cases as OC  # noqa: E402
from oracle import gpdla_oracle as O  # noqa: E402

# a tenth of tests/test_training.py's bars (f rel 1e-11, g atol 1e-11 max|g|)
F_COND, G_COND = 1e-12, 1e-12


def _launches(cases):
    return [(c, d, l) for c in cases for d in [OC.case_decompose(c)] for l in d["launches"]]


# ------------------------------------------------------------------------------ the constants
def test_table_matches_the_source():
    assert OC.source_constants() == OC.TABLE_AS_SOURCE


def test_decompose_restates_the_partition():
    d = OC.decompose(11, 77, 20)
    assert (d["kb"], d["nxp"], d["nep"], d["ldw"], d["nss"], d["mt_rows"], d["kp"]) == (20, 256, 320, 96, 6, 80, 24)
    assert d["gram_steps"] == [2, 2, 1, 1]
    assert d["lds_bytes"] == 8 * (154 + 800 + 80 + 8 + 420) and not d["lds_opt_in"]
    (l,) = d["launches"]
    assert l["acc_chunks"] == [1, 1, 2, 1, 1, 2, 1, 2] and l["acc_nks"] == [1] * 8
    assert (l["rows"], l["padding_rows"], l["stale_rows"]) == (32, 21, 0)
    d = OC.decompose(70, 33, 8, batch=33)
    assert [l["nq"] for l in d["launches"]] == [33, 33, 4]
    assert [l["rows"] for l in d["launches"]] == [64, 64, 32]
    assert [l["stale_rows"] for l in d["launches"]] == [0, 0, 28]
    # the default launch size: all spectra while the workspace stays below 2^29 doubles
    assert OC.decompose(5000, 1217, 20)["batch"] == 5000
    assert OC.decompose(10 ** 6, 4096, 64)["batch"] == (1 << 29) // (2 * 4096 + 2 * 2176 + 5 * 4096 + 8)
    for nks, wave, want in ((0, 0, (0, 0)), (1, 0, (1, 0)), (1, 1, (0, 0)), (5, 0, (1, 1)), (5, 1, (1, 0)),
                            (9, 0, (2, 1)), (13, 0, (2, 2)), (17, 0, (3, 2))):
        got = OC._wave_pipeline(nks, wave)
        assert (got["trips"], got["second_halves"]) == want, (nks, wave)


# -------------------------------------------------------------------- what the case lists reach
def test_case_a_reaches_every_rank_bucket_from_both_sides():
    ranks = {c.k for c in OC.CASES_A if not c.lines}
    assert {1, OC.MAX_K} <= ranks
    for lo, kb in zip((0,) + OC.KB_LADDER, OC.KB_LADDER):
        inside = {k for k in ranks if OC.obj_kb(k) == kb}
        assert kb in inside, kb                               # k == KB: no zero padding
        assert any(k < kb for k in inside), kb                # k < KB: the padded copies matter
        assert lo + 1 in inside, kb                           # the first rank of the bucket
        if kb < OC.MAX_K:
            assert OC.obj_kb(kb + 1) != kb and kb + 1 in ranks
    assert {OC.obj_kb(c.k) for c in OC.CASES_A if c.lines == 31} == set(OC.KB_LADDER)
    assert {c.lines for c in OC.CASES_A if c.k == 20} == {0, 1, 2, 31}
    assert {OC.obj_kb(k) for k in OC.A_LOSS_RANKS} == set(OC.KB_LADDER)
    d = OC.decompose(OC.A_SPECTRA, OC.A_PIXELS, 20)
    assert all(OC.A_PIXELS % m for m in (4, 16, 32)) and d["ldw"] == 96
    assert d["gram_steps"] == [2, 2, 1, 1]                    # waves 0, 1 take two super-steps, 2, 3 one
    (l,) = d["launches"]
    assert {1, 2} == set(l["acc_chunks"])                     # unequal accumulate chunks, some of one spectrum


def test_case_b_reaches_every_pixel_edge_on_both_paths():
    for k in OC.B_RANKS:
        pixels = {c.P for c in OC.CASES_B if c.k == k}
        assert 1 in pixels
        for m in (4, 16, 32):
            assert {0, 1, m - 1} <= {P % m for P in pixels}, m
            assert any(P < m for P in pixels) and any(P > m for P in pixels)
        assert any(P < k for P in pixels) and any(P == 16 for P in pixels)
        steps = {tuple(OC.decompose(5, P, k)["gram_steps"]) for P in pixels}
        assert (1, 1, 0, 0) in steps and any(min(s) >= 2 for s in steps)     # idle waves, and two trips
    assert OC.decompose(5, 33, 20)["valu"] and not OC.decompose(5, 33, 40)["valu"]
    tiles = [OC.decompose(5, c.P, 40) for c in OC.CASES_B if c.k == 40]
    assert any(sum(d["mfma_tiles"]) == 1 and d["mfma_tail_pixels"] for d in tiles)    # P below one 16-pixel tile
    assert any(d["mfma_tiles"][3] == 0 for d in tiles) and any(d["mfma_tiles"][0] >= 2 for d in tiles)
    assert {d["mfma_tail_pixels"] for d in tiles} >= {0, 1, 15}
    assert {d["mt_rows"] - d["P"] for d in tiles} == {0, 1, 2, 3}


def test_limits_and_lds_opt_in():
    ds = [OC.case_decompose(c) for c in OC.ALL_CASES]
    assert {d["k"] for d in ds} >= {1, OC.MAX_K} and {d["P"] for d in ds} >= {1, OC.MAX_PIXELS}
    for valu in (True, False):
        assert {d["lds_opt_in"] for d in ds if d["valu"] == valu} == {True, False}, valu
    dd = {(c.P, c.k): OC.case_decompose(c) for c in OC.CASES_D}
    assert dd[4096, 64]["lds_bytes"] == 8 * (8192 + 8192 + 256 + 8) < 160 * 1024
    # 2 P doubles alone are 64 KiB at P = 4096: every P = 4096 case opts in, on the VALU path too
    assert dd[4096, 32]["lds_opt_in"] and dd[4096, 1]["lds_opt_in"] and dd[4096, 1]["valu"]
    # and 2 k^2 doubles are 64 KiB at k = 64: rank 64 opts in at any P; case A's rank 48 (same bucket) does not
    assert dd[1, 64]["lds_opt_in"] and not dd[1, 64]["valu"]
    assert not OC.decompose(11, 77, 48)["lds_opt_in"] and OC.decompose(11, 77, 48)["kb"] == 64
    assert all(OC.uses_dense(c) == (c.P <= 128) for c in OC.ALL_CASES)


def test_case_c_reaches_every_pipeline_and_sum_branch():
    one = _launches(OC.CASES_C)
    assert {c.Q for c in OC.CASES_C} >= {0, 1}
    assert OC.case_decompose(OC.CASES_C[0])["launches"] == []                # Q = 0: no launch at all
    chunks = [n for _, _, l in one for n in l["acc_chunks"]]
    assert 0 in chunks and 1 in chunks                                       # an empty accumulate chunk
    waves = [w for _, _, l in one for ws in l["acc_waves"] for w in ws]
    assert {0, 1} <= {w["trips"] for w in waves} and any(w["trips"] >= 2 for w in waves)
    assert any(w["trips"] == 1 and w["second_halves"] == 0 for w in waves)
    assert any(w["trips"] == 1 and w["second_halves"] == 1 for w in waves)
    assert any(w["trips"] >= 2 and w["second_halves"] == w["trips"] for w in waves)
    assert any(w["trips"] >= 2 and w["second_halves"] == w["trips"] - 1 for w in waves)
    # the second half first runs at Q = 137 (nks = 5); below it no wave of any chunk reaches it
    for c, _, l in one:
        ran = any(w["second_halves"] for ws in l["acc_waves"] for w in ws)
        assert ran == (c.Q >= 137), c
    nks = {c.Q: max(l["acc_nks"]) for c, _, l in one}
    assert (nks[33], nks[65], nks[137], nks[265], nks[409]) == (2, 3, 5, 9, 13) and nks[1031] > 16
    sums = [(b, t) for _, _, l in one for b, t in zip(l["sum_body"], l["sum_tail"])]
    assert any(b and t for b, t in sums) and any(b and not t for b, t in sums) and any(not b and t for b, t in sums)
    assert any(not b and not t for b, t in sums)
    for c, _, l in one:                                                      # only Q = 1031 runs the 16-deep body
        assert any(l["sum_body"]) == (c.Q == 1031), c


def test_case_c_launches():
    many = {c.batch: OC.case_decompose(c) for c in OC.CASES_C_LAUNCHES if not c.lines}
    assert [len(many[b]["launches"]) for b in (1, 5, 32, 33)] == [70, 14, 3, 3]
    assert [l["nq"] for l in many[32]["launches"]] == [32, 32, 6]            # no padding rows, then a ragged one
    assert many[32]["launches"][0]["padding_rows"] == 0
    last, before = many[33]["launches"][-1], many[33]["launches"][-2]
    assert (before["nq"], last["nq"]) == (33, 4) and last["rows"] == 32 and last["stale_rows"] == 28
    assert before["rows"] == 64 and before["padding_rows"] == 31
    forest = [c for c in OC.CASES_C_LAUNCHES if c.lines]
    assert len(forest) == 1 and len(OC.case_decompose(forest[0])["launches"]) > 1
    z = OC.case_problem(forest[0])["z_qsos"]
    assert np.unique(z).size == z.size                                       # a missing batch offset shows


# ---------------------------------------------------------------------------------- the inputs
def test_problem_rows():
    p = OC.problem(11, 77, 20, 100)
    nan = np.isnan(p["y"])
    assert nan[p["all_nan_row"]].all() and not nan[0].any()
    others = np.delete(nan, [0, p["all_nan_row"]], axis=0)
    assert 0.1 < others.mean() < 0.3 and others.any(axis=1).all()
    assert not np.isnan(OC.problem(2, 33, 8, 400)["y"]).any()
    # a row does not depend on how many spectra there are
    assert np.array_equal(OC.problem(9, 33, 8, 300)["lya"], OC.problem(33, 33, 8, 300)["lya"][:9])
    assert not OC.problem(3, 5, 2, 1)["x"].flags.writeable


def test_forest_problem_has_red_and_many_line_pixels():
    import sub_dla_forest_oracle as SO
    p = OC.problem(11, 77, 20, 100, forest=True)
    counts = set()
    for q in range(11):
        ok = ~np.isnan(p["y"][q])
        rest = p["lya"][q, ok] * FO.LAMBDA_1 / (1 + p["z_qsos"][q])
        counts |= {SO.active_lines(r, p["z_qsos"][q]) for r in rest}
        FO.series_terms(p["lya"][q, ok], p["z_qsos"][q], OC.TAU_0, OC.BETA, 31)      # asserts the edge guard
    assert {0, 1, 31} <= counts and len(counts) > 4


# -------------------------------------------------------------- the dense reference by itself
def test_dense_f_is_the_gaussian_nll():
    p = OC.loss_problem(8)
    f = OC.dense_spectrum(p["y"], p["lya"], p["nv"], p["M"], p["omega2"], OC.C_0, OC.TAU_0, OC.BETA)[0]
    sf = 1 - np.exp(-OC.TAU_0 * p["lya"] ** OC.BETA) + OC.C_0
    d = p["nv"] + p["omega2"] * sf ** 2
    ref = -multivariate_normal(np.zeros(p["y"].size), p["M"] @ p["M"].T + np.diag(d)).logpdf(p["y"])
    assert float(f) == pytest.approx(ref, rel=1e-12)


def test_dense_forest_terms_are_the_restatement():
    p = OC.loss_problem(8, forest=True)
    for L in (1, 2, 31):
        tau, tlog = OC.series_terms_ld(np.asarray(p["lya"], OC.LD), p["z_qso"], OC.LD(OC.TAU_0), OC.LD(OC.BETA), L)
        rt, rl = FO.series_terms(p["lya"], p["z_qso"], OC.TAU_0, OC.BETA, L)
        np.testing.assert_allclose(tau.astype(float), rt, rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(tlog.astype(float), rl, rtol=1e-13, atol=1e-300)
        assert (rt == 0).any() and (rt > 0).any()


@pytest.mark.parametrize("forest", [False, True])
def test_dense_gradient_matches_finite_differences(forest):
    """Central differences of the dense reference's own f in x = [M(:); log omega; log c0; log tau0; log beta]
    (h, rtol and atol of test_oracle_gradient_matches_finite_differences)."""
    n, k = 24, 3
    pr = OC.problem(1, n, k, 600, forest)
    y, lya, nv, x = pr["y"], pr["lya"], pr["nv"], pr["x"]
    z = pr["z_qsos"]

    def fg(x):
        f, g = OC.dense_objective(x, y, lya, nv, z, 31)
        return f, g

    _, g = fg(x)
    g = g.copy()
    t0, b = np.exp(x[-2]), np.exp(x[-1])
    g[-2] -= t0 * (t0 - 0.0023) / 0.0007 ** 2        # the priors enter g only (objective.m:59-71)
    g[-1] -= b * (b - 3.65) / 0.21 ** 2
    h = 1e-6
    fd = np.array([(fg(x + h * e)[0] - fg(x - h * e)[0]) / (2 * h) for e in np.eye(x.size)])
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-7)


def test_dense_objective_masks_sums_and_adds_priors():
    p = OC.problem(4, 12, 3, 601)
    x = p["x"].copy()
    x[-2:] = np.log([0.003, 3.5])
    f, g = OC.dense_objective(x, p["y"], p["lya"], p["nv"])
    fo, go = O.objective(x, p["y"], p["lya"], p["nv"])
    assert f == pytest.approx(fo, rel=1e-13)
    np.testing.assert_allclose(g, go, rtol=1e-9, atol=1e-12 * np.abs(go).max())
    f0, g0 = OC.dense_objective(x, np.full_like(p["y"], np.nan), p["lya"], p["nv"])
    assert f0 == 0 and not g0[:-2].any()
    assert g0[-2] == pytest.approx(0.003 * (0.003 - 0.0023) / 0.0007 ** 2, rel=1e-12)
    assert g0[-1] == pytest.approx(3.5 * (3.5 - 3.65) / 0.21 ** 2, rel=1e-12)


# ---------------------------------------------------------------- the condition on the inputs
def _condition(ref_f, ref_g, f, g, P, k, where):
    assert abs(f - ref_f) <= F_COND * max(abs(ref_f), 1.0), (where, f, ref_f)
    rb, gb = OC.blocks(ref_g, P, k), OC.blocks(g, P, k)
    for name in rb:
        if rb[name].size:
            err = np.abs(gb[name] - rb[name]).max()
            assert err <= G_COND * np.abs(rb[name]).max(), (where, name, err / np.abs(rb[name]).max())


# (Q = 0 has no spectrum to judge: its g is the two prior terms, which the GPU test forms itself)
DENSE_CASES = sorted({c._replace(batch=None) for c in OC.ALL_CASES if OC.uses_dense(c) and c.Q > 0})


@pytest.mark.parametrize("c", DENSE_CASES, ids=OC.case_id)
def test_oracle_agrees_with_the_dense_reference(c):
    """A condition on the inputs, not a measurement: where it fails the inputs are too ill-conditioned to
    judge a double-precision kernel with, and the inputs change, not the bar."""
    ref = OC.reference(c)
    assert ref["source"] == "dense"
    f, g = OC.oracle_objective(c)
    _condition(ref["f"], ref["g"], f, g, c.P, c.k, OC.case_id(c))


@pytest.mark.parametrize("forest", [False, True])
@pytest.mark.parametrize("k", OC.A_LOSS_RANKS)
def test_oracle_spectrum_loss_agrees_with_the_dense_reference(k, forest):
    p = OC.loss_problem(k, forest)
    ref = OC.loss_reference(k, forest)
    if forest:
        got = FO.spectrum_loss_forest(p["y"], p["lya"], p["nv"], p["M"], p["omega2"], OC.C_0, OC.TAU_0, OC.BETA,
                                      p["z_qso"], 31)
    else:
        got = O.spectrum_loss(p["y"], p["lya"], p["nv"], p["M"], p["omega2"], OC.C_0, OC.TAU_0, OC.BETA)
    g = np.concatenate([got[1].ravel(order="F"), got[2], got[3:]])
    rg = np.concatenate([ref[1].ravel(order="F"), ref[2], ref[3:]])
    _condition(ref[0], rg, got[0], g, OC.A_PIXELS, k, f"spectrum_loss k={k} forest={forest}")


def test_large_cases_fall_to_the_oracle():
    big = [c for c in OC.ALL_CASES if not OC.uses_dense(c)]
    assert {c.P for c in big} == {129, 255, 256, 257, 4096}
    assert OC.reference(OC.Case("B", 5, 129, 20, 0, None, 200))["source"] == "oracle"


# ------------------------------------------------------------------------------------- case E
def test_e4_pivot_is_refused_by_cholesky_and_the_good_point_is_ordinary():
    e = OC.e4_problem()
    Q, P, k = OC.E_SHAPE
    q = e["spectrum"]
    ind = ~np.isnan(e["y"][q])
    assert ind[OC.E4_PIXEL]

    def B(x):
        M = x[:P * k].reshape(P, k, order="F")[ind]
        sf = 1 - np.exp(-OC.TAU_0 * e["lya"][q, ind] ** OC.BETA) + OC.C_0
        d = e["nv"][q, ind] + np.exp(2 * x[P * k:P * (k + 1)])[ind] * sf ** 2
        return np.eye(k) + M.T @ (M / d[:, None]), d

    Bb, d = B(e["x_bad"])
    assert Bb[0, 0] < 0 and d[np.flatnonzero(ind) == OC.E4_PIXEL][0] < 0
    with pytest.raises(LinAlgError):
        cholesky(Bb, lower=False)
    Bg, d = B(e["x_good"])
    assert d.min() > 0
    cholesky(Bg, lower=False)
    f, g = O.objective(e["x_good"], e["y"], e["lya"], e["nv"])
    fd, gd = OC.dense_objective(e["x_good"], e["y"], e["lya"], e["nv"])
    _condition(fd, gd, f, g, P, k, "E4 good point")

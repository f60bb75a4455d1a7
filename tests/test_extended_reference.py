"""The extended-precision references of tests/extended_reference.py, pinned on the CPU before they
judge a kernel (tests/test_gpu_standalone_edges.py): against scipy's dense density, against both
oracles over every shape the GPU sweep uses, and against the exact power-of-two scaling law.  Every
test prints the worst deviation it measured before it asserts."""
import numpy as np
import pytest
from scipy.stats import multivariate_normal

import extended_reference as X
from oracle import cpu_ref
from oracle import gpdla_oracle as O


def _rel(got, ref):
    return abs(float(got) - float(ref)) / max(1.0, abs(float(ref)))


def test_long_double_is_extended():
    X.require_extended_precision()
    assert np.finfo(np.longdouble).nmant >= 63


def test_log_mvnpdf_ld_matches_dense_scipy():
    worst = 0.0
    for n, k in ((50, 3), (300, 20), (129, 64)):
        y, mu, M, d = X.mvn_case(n, k)
        ref = multivariate_normal(mu, M @ M.T + np.diag(d)).logpdf(y)
        err = abs(float(X.log_mvnpdf_ld(y, mu, M, d)) - ref) / abs(ref)
        worst = max(worst, err)
        assert err < 1e-9, (n, k, err)
    print(f"log_mvnpdf_ld vs scipy dense: worst relative deviation {worst:.2e}")


@pytest.fixture(scope="module")
def ld_values():
    """log_mvnpdf_ld over MVN_SHAPES, computed once for the two oracle comparisons."""
    return {nk: X.log_mvnpdf_ld(*X.mvn_case(*nk)) for nk in X.MVN_SHAPES}


@pytest.mark.parametrize("which", ["python_oracle", "cpp_oracle"])
def test_log_mvnpdf_ld_matches_the_oracles(ld_values, which):
    fn = O.log_mvnpdf_low_rank if which == "python_oracle" else cpu_ref.log_mvnpdf_low_rank
    assert len(X.MVN_SHAPES) == 576
    worst, at = 0.0, None
    for nk in X.MVN_SHAPES:
        err = _rel(fn(*X.mvn_case(*nk)), ld_values[nk])
        if err > worst:
            worst, at = err, nk
    print(f"{which} vs log_mvnpdf_ld over {len(X.MVN_SHAPES)} cases: worst {worst:.2e} at (n, k) = {at}")
    assert worst <= 1e-12, (which, worst, at)


@pytest.mark.parametrize("n,k", X.SCALE_SHAPES)
def test_log_mvnpdf_ld_power_of_two_scaling(n, k):
    """(s y, s mu, s M, s^2 d) with s = 2^e is exact, and shifts the log density by -n e ln 2."""
    base_case = X.mvn_case(n, k)
    base = X.log_mvnpdf_ld(*base_case)
    ln2 = np.log(np.longdouble(2))
    for e in X.SCALE_EXPONENTS:
        scaled_case = X.mvn_scaled(base_case, e)
        assert all(np.all(np.isfinite(a)) and np.all(a != 0) for a in scaled_case)
        scaled = X.log_mvnpdf_ld(*scaled_case)
        dev = abs(float(scaled - (base - np.longdouble(n) * np.longdouble(e) * ln2)))
        orc = abs(float(O.log_mvnpdf_low_rank(*scaled_case)) - float(scaled)) / abs(float(scaled))
        print(f"(n, k, e) = ({n}, {k}, {e}): scaling law off by {dev:.2e}, python oracle vs ld {orc:.2e}")
        assert dev < 1e-11, (n, k, e, dev)
        assert orc <= 1e-12, (n, k, e, orc)


def test_log_mean_exp_ld():
    rng = np.random.default_rng(5)
    row = -4000 + 30 * rng.standard_normal(1025)
    ref = np.logaddexp.reduce(row) - np.log(row.size)
    assert abs(float(X.log_mean_exp_ld(row)) - ref) < 1e-12 * abs(ref)
    assert float(X.log_mean_exp_ld([-1234.5])) == -1234.5
    assert float(X.log_mean_exp_ld([-7.0] * 4096)) == -7.0


def test_cpp_voigt_matches_the_python_oracle_at_the_tile_edges():
    """The two restatements of voigt.c:253-304 at the shapes of the GPU edge sweep, with the bars the
    GPU comparison uses: the reference alone must sit far inside them."""
    worst_abs = worst_rel = 0.0
    for n_padded in X.VOIGT_N_PADDED:
        lam = X.voigt_grid(n_padded)
        for nl in X.VOIGT_NUM_LINES:
            for z, N in X.voigt_absorbers(lam):
                ref = O.voigt_mex(lam, z, N, nl)
                got = cpu_ref.voigt(lam, z, N, nl)
                assert got.shape == ref.shape == (n_padded - 6,)
                worst_abs = max(worst_abs, float(np.max(np.abs(got - ref))))
                big = ref > 1e-200
                if big.any():
                    worst_rel = max(worst_rel, float(np.max(np.abs(got[big] - ref[big]) / ref[big])))
    print(f"cpu_ref.voigt vs voigt_mex: worst absolute {worst_abs:.2e}, worst relative {worst_rel:.2e}")
    assert worst_abs < 1e-12
    assert worst_rel < 1e-9

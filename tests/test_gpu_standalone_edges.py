"""The stand-alone MEX drop-ins and the evidence reduction at the edges of their kernels.

* ``gpdla_log_mvnpdf_low_rank_f64`` (mvn_single_kernel): every rank 1..64 -- ranks >= 22 are the
  ones that use the Gram / u slots j >= 1 of a thread, rank 64 column 64 of the D^-1 M tile and the
  65 x 66 augmented Cholesky -- at n below, at and one past the 64-row chunk, against the
  long-double reference of tests/extended_reference.py; power-of-two scaled inputs; invalid data
  (reported, never returned); the host argument limits; the MATLAB gateway at rank 64.
* ``gpdla_voigt_f64`` / ``gpdla_voigt_batch_f64`` (voigt_batch_kernel): n_out = 1, 2, 3, 255-257 and
  512-514 around the 256-output tile with its 6-pixel halo, seven line counts, absorbers at both ends
  and the middle of the grid; a batch larger than one tile, against single calls.
* the staging buffer both share (standalone_bufs, csrc/engine.hip): calls of different sizes
  interleaved, bit for bit.
* ``reduce_kernel`` through Engine.process: S at the boundaries of its 4 x 1,024 unrolled loop and its
  tail, against the long-double log-mean-exp of the device's own sample row.

The bars are the project's existing ones for each entry point (tests/test_gpu_parity.py:47-49,67;
tests/test_gpu_baseline_configs.py:77); every test prints the worst deviation it measured before it
asserts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import extended_reference as X  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import Engine, log_mvnpdf_low_rank, voigt, voigt_batch  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def require_device():
    lib = L.load()
    assert lib.gpdla_device_count() > 0, "no HIP device: GPU tests must run on the MI355X box"


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _mvn_abi(y, mu, M, d, n=None, k=None):
    """gpdla_log_mvnpdf_low_rank_f64 itself: (return code, *out); *out starts as a finite sentinel."""
    y, mu, d = (np.ascontiguousarray(a, dtype=np.float64) for a in (y, mu, d))
    M = np.asarray(M, dtype=np.float64)
    Mf = np.ascontiguousarray(M.ravel(order="F"))
    out = np.full(1, 12345.0)
    rc = L.load().gpdla_log_mvnpdf_low_rank_f64(L.ptr(y), L.ptr(mu), L.ptr(Mf), L.ptr(d),
                                                M.shape[0] if n is None else n,
                                                M.shape[1] if k is None else k, L.ptr(out))
    return rc, float(out[0])


def _rel(got, ref):
    return abs(float(got) - float(ref)) / max(1.0, abs(float(ref)))


# ============================================================================== log_mvnpdf_low_rank
@pytest.fixture(scope="module")
def mvn_worst():
    """Worst relative deviation of the rank sweep and where; reported when the module is done."""
    worst = {"err": 0.0, "at": None, "cases": 0}
    yield worst
    print(f"\nlog_mvnpdf_low_rank vs long double over {worst['cases']} cases: worst relative deviation "
          f"{worst['err']:.3e} at (n, k) = {worst['at']}")


@pytest.mark.parametrize("k", range(1, 65))
def test_log_mvnpdf_every_rank_at_the_chunk_edges(k, mvn_worst):
    """All of MVN_SHAPES: |got - ref| <= 1e-10 max(1, |ref|) against log_mvnpdf_ld."""
    shapes = [nk for nk in X.MVN_SHAPES if nk[1] == k]
    assert [n for n, _ in shapes] == list(X.MVN_NS)
    errs = {}
    for n, _ in shapes:
        case = X.mvn_case(n, k)
        rc, got = _mvn_abi(*case)
        assert rc == L.GPDLA_OK, (n, k, rc)
        errs[n] = _rel(got, X.log_mvnpdf_ld(*case))
        mvn_worst["cases"] += 1
        if errs[n] >= mvn_worst["err"]:
            mvn_worst["err"], mvn_worst["at"] = errs[n], (n, k)
    n_worst = max(errs, key=errs.get)
    print(f"k = {k}: worst relative deviation {errs[n_worst]:.3e} at n = {n_worst}")
    assert all(e <= 1e-10 for e in errs.values()), (k, errs)


@pytest.mark.parametrize("n,k", [(257, 64), (1, 64)])
def test_log_mvnpdf_repeat_calls_same_bits(n, k):
    case = X.mvn_case(n, k)
    first = log_mvnpdf_low_rank(*case)
    assert np.isfinite(first)
    assert _bits(log_mvnpdf_low_rank(*case)) == _bits(first)


@pytest.mark.parametrize("e", X.SCALE_EXPONENTS)
@pytest.mark.parametrize("n,k", X.SCALE_SHAPES)
def test_log_mvnpdf_power_of_two_scaled_inputs(n, k, e):
    """(s y, s mu, s M, s^2 d), s = 2^e: Gram, u and the quadratic form are unchanged, sum log d moves
    by 2 n e ln 2; nothing may overflow on the way, and no call may report GPDLA_ENUMERIC."""
    scaled = X.mvn_scaled(X.mvn_case(n, k), e)
    rc, got = _mvn_abi(*scaled)
    ref = X.log_mvnpdf_ld(*scaled)
    print(f"(n, k, e) = ({n}, {k}, {e}): rc {rc}, relative deviation {_rel(got, ref):.3e}")
    assert rc == L.GPDLA_OK, (n, k, e, rc)
    assert _rel(got, ref) <= 1e-10, (n, k, e, got, float(ref))


def _poison(case, what, i):
    y, mu, M, d = (a.copy() for a in case)
    if what == "y_nan":
        y[i] = np.nan
    else:
        d[i] = {"d_zero": 0.0, "d_negative": -1.0, "d_nan": np.nan}[what]
    return y, mu, M, d


@pytest.mark.parametrize("i", [0, 63, 64, 128])
@pytest.mark.parametrize("what", ["d_zero", "d_negative", "d_nan", "y_nan"])
def test_log_mvnpdf_invalid_data_is_reported(what, i):
    """A non-positive or NaN d[i], or a NaN y[i], on either side of the 64-row chunk edge and at both
    ends: GPDLA_ENUMERIC with *out = NaN through the C ABI, GpdlaNumericError through the binding,
    and the valid case afterwards gives the bits it gave before (a failed call leaves nothing
    behind in the staging buffer or the status word)."""
    good = X.mvn_case(129, 22)
    before = log_mvnpdf_low_rank(*good)
    assert np.isfinite(before)
    bad = _poison(good, what, i)
    rc, out = _mvn_abi(*bad)
    assert rc == L.GPDLA_ENUMERIC, (what, i, rc, out)
    assert np.isnan(out), (what, i, out)
    assert _bits(log_mvnpdf_low_rank(*good)) == _bits(before)
    with pytest.raises(L.GpdlaNumericError):
        log_mvnpdf_low_rank(*bad)
    assert _bits(log_mvnpdf_low_rank(*good)) == _bits(before)


def test_log_mvnpdf_argument_limits():
    """Host checks (no kernel runs): k = 65 is unsupported, n = 0 or k = 0 invalid."""
    y, mu, M, d = X.mvn_case(5, 65)
    assert _mvn_abi(y, mu, M, d)[0] == L.GPDLA_EUNSUPPORTED
    with pytest.raises(L.GpdlaError) as ei:
        log_mvnpdf_low_rank(y, mu, M, d)
    assert ei.value.code == L.GPDLA_EUNSUPPORTED
    y, mu, M, d = X.mvn_case(5, 2)
    assert _mvn_abi(y, mu, M, d, n=0)[0] == L.GPDLA_EINVAL
    assert _mvn_abi(y, mu, M, d, k=0)[0] == L.GPDLA_EINVAL
    assert _mvn_abi(y, mu, M, d)[0] == L.GPDLA_OK


def test_mvn_gateway_at_rank_64():
    """log_mvnpdf_low_rank_mex (matlab/log_mvnpdf_low_rank_mex.c, through the in-process MEX runtime of
    tests/test_matlab_gateways.py) at the largest rank the drop-in takes, n one past a 64-row chunk:
    the binding's bits, and within the entry point's 1e-10 bar of the long-double reference."""
    from test_matlab_gateways import MOCK, Gateway
    assert (MOCK / "liblog_mvnpdf_low_rank_mex_mock.so").exists(), "the MEX mocks are built by build()"
    y, mu, M, d = X.mvn_case(129, 64)
    (got,) = Gateway("log_mvnpdf_low_rank_mex")(1, y, mu, M, d)
    assert got.shape == (1, 1)
    assert got[0, 0] == log_mvnpdf_low_rank(y, mu, M, d)
    ref = float(X.log_mvnpdf_ld(y, mu, M, d))
    assert abs(got[0, 0] - ref) <= 1e-10 * max(1, abs(ref))


# ============================================================================ voigt / voigt_batch
@pytest.fixture(scope="module")
def voigt_worst():
    worst = {"abs": 0.0, "abs_at": None, "rel": 0.0, "rel_at": None, "cases": 0}
    yield worst
    print(f"\nvoigt vs voigt_mex over {worst['cases']} calls: worst absolute deviation {worst['abs']:.3e} at "
          f"(n_padded, num_lines, absorber) = {worst['abs_at']}, worst relative {worst['rel']:.3e} at {worst['rel_at']}")


@pytest.mark.parametrize("n_padded", X.VOIGT_N_PADDED)
def test_voigt_at_the_tile_edges(n_padded, voigt_worst):
    """n_out = n_padded - 6 of 1, 2, 3, 255-257, 512-514, every line count of the list, absorbers at
    the blue end, the middle and the red end, against oracle.gpdla_oracle.voigt_mex."""
    from oracle import gpdla_oracle as O
    lam = X.voigt_grid(n_padded)
    w_abs = w_rel = 0.0
    for nl in X.VOIGT_NUM_LINES:
        for a, (z, N) in enumerate(X.voigt_absorbers(lam)):
            ref = O.voigt_mex(lam, z, N, nl)
            got = voigt(lam, z, N, nl)
            assert got.shape == ref.shape == (n_padded - 6,)
            e_abs = float(np.max(np.abs(got - ref)))
            big = ref > 1e-200
            e_rel = float(np.max(np.abs(got[big] - ref[big]) / ref[big])) if big.any() else 0.0
            w_abs, w_rel = max(w_abs, e_abs), max(w_rel, e_rel)
            voigt_worst["cases"] += 1
            if e_abs >= voigt_worst["abs"]:
                voigt_worst["abs"], voigt_worst["abs_at"] = e_abs, (n_padded, nl, a)
            if e_rel >= voigt_worst["rel"]:
                voigt_worst["rel"], voigt_worst["rel_at"] = e_rel, (n_padded, nl, a)
            assert e_abs < 1e-12, (n_padded, nl, a, e_abs)
            assert e_rel < 1e-9, (n_padded, nl, a, e_rel)
    print(f"n_padded = {n_padded}: worst absolute {w_abs:.3e}, worst relative {w_rel:.3e}")


@pytest.mark.parametrize("count", [1, 2, 257])
def test_voigt_batch_equals_single_calls(count):
    """One block per (z, N): a batch of more blocks than a tile has outputs, bit for bit the single
    calls, checked at both sides of row 256."""
    lam = X.voigt_grid(263)
    absorbers = X.voigt_absorbers(lam)
    zs = np.array([absorbers[i % 3][0] for i in range(count)])
    Ns = np.array([absorbers[i % 3][1] for i in range(count)])
    batch = voigt_batch(lam, zs, Ns, 3)
    assert batch.shape == (count, 257)
    single = [voigt(lam, z, N, 3) for z, N in absorbers]
    assert not np.array_equal(single[0], single[1]) and not np.array_equal(single[1], single[2])
    for row in range(count):                            # rows 0, 1, 255, 256 and all between
        np.testing.assert_array_equal(batch[row], single[row % 3], err_msg=f"row {row}")


def test_voigt_batch_of_none_is_empty():
    lam = X.voigt_grid(263)
    out = voigt_batch(lam, np.zeros(0), np.zeros(0), 3)
    assert out.shape == (0, 257) and out.size == 0


def test_voigt_argument_limits():
    lib = L.load()
    lam = X.voigt_grid(263)
    out = np.full(257, 7.0)
    z, N = 2.1, 1e20
    assert lib.gpdla_voigt_f64(L.ptr(lam), 6, z, N, 3, L.ptr(out)) == L.GPDLA_EINVAL
    for nl in (0, 32):
        assert lib.gpdla_voigt_f64(L.ptr(lam), 263, z, N, nl, L.ptr(out)) == L.GPDLA_EINVAL
        with pytest.raises(L.GpdlaError) as ei:
            voigt(lam, z, N, nl)
        assert ei.value.code == L.GPDLA_EINVAL
    zs, Ns = np.array([z]), np.array([N])
    assert lib.gpdla_voigt_batch_f64(L.ptr(lam), 6, L.ptr(zs), L.ptr(Ns), 1, 3, L.ptr(out)) == L.GPDLA_EINVAL
    assert np.all(out == 7.0)                           # refused calls write nothing
    assert lib.gpdla_voigt_f64(L.ptr(lam), 7, z, N, 3, L.ptr(out)) == L.GPDLA_OK
    assert out[0] != 7.0 and np.all(out[1:] == 7.0)     # n_padded = 7 writes its one output only


# ======================================================================== the shared staging buffer
def test_interleaved_sizes_through_the_shared_staging_buffer():
    """Both entry points stage through one per-device buffer that only grows: large and small calls of
    both, forwards, backwards and forwards again, each equal to its first value bit for bit."""
    lam263 = X.voigt_grid(263)
    ab = X.voigt_absorbers(lam263)
    zs = np.array([ab[i % 3][0] for i in range(257)])
    Ns = np.array([ab[i % 3][1] for i in range(257)])
    lam520, lam7 = X.voigt_grid(520), X.voigt_grid(7)
    calls = [
        lambda: np.array([log_mvnpdf_low_rank(*X.mvn_case(257, 64))]),
        lambda: voigt(lam520, *X.voigt_absorbers(lam520)[1], 31),
        lambda: np.array([log_mvnpdf_low_rank(*X.mvn_case(1, 1))]),
        lambda: voigt(lam7, *X.voigt_absorbers(lam7)[1], 31),
        lambda: voigt_batch(lam263, zs, Ns, 3),
        lambda: np.array([log_mvnpdf_low_rank(*X.mvn_case(129, 40))]),
    ]
    first = [c() for c in calls]
    assert all(np.all(np.isfinite(f)) for f in first)
    order = list(range(len(calls)))
    for sweep in (order[::-1], order):
        for i in sweep:
            np.testing.assert_array_equal(_bits(calls[i]()), _bits(first[i]), err_msg=f"call {i}")


# ================================================================= reduce_kernel via Engine.process
@pytest.fixture(scope="module")
def reduce_inputs():
    """Two short usable spectra of different length and one with nothing in range.  One and two pixels
    on purpose: with tens of pixels a row spans hundreds of e-folds and all but a handful of its
    samples could be dropped from the sum unnoticed; over one pixel every sample counts (checked
    in the test)."""
    model = syn.make_model(k=4)
    base = syn.make_spectrum(model, 0, z_qso=2.8, n_target=None, mask_fraction=0.1)
    spectra = []
    for npx in (1, 2):
        sl = slice(100, 100 + npx)
        spectra.append({k: (v[sl] if isinstance(v, np.ndarray) else v) for k, v in base.items()})
        spectra[-1]["pixel_mask"] = np.zeros(npx, dtype=bool)
    empty = dict(base)
    empty["z_qso"] = 9.5
    spectra.append(empty)
    return model, syn.pack_spectra(spectra)


@pytest.fixture(scope="module")
def reduce_worst():
    worst = {"err": 0.0, "at": None}
    yield worst
    print(f"\nlog-mean-exp vs long double: worst relative deviation {worst['err']:.3e} at (S, row) = {worst['at']}")


@pytest.mark.parametrize("S", [1, 1023, 1024, 1025, 3072, 3073, 4095, 4096, 4097, 8193])
def test_log_mean_exp_at_the_loop_boundaries(S, reduce_inputs, reduce_worst):
    """S on both sides of every boundary of the reduction's loops (a thread enters the 4-way unrolled
    loop when tid + 3072 < S; the tail strides by 1,024).  The reference is formed from the device's
    own sample row, so this judges the reduction alone."""
    model, packed = reduce_inputs
    samples = syn.make_samples(S)
    params = set_parameters(k=4)
    with Engine(model, samples, params) as eng:
        out = eng.process(packed)
    with Engine(model, samples, params, max_batch_spectra=1) as eng:
        split = eng.process(packed)
    sll, lld = out["sample_log_likelihoods_dla"], out["log_likelihoods_dla"]
    assert sll.shape == (3, S)
    for q in (0, 1):
        assert np.all(np.isfinite(sll[q]))
        ref = X.log_mean_exp_ld(sll[q])
        err = _rel(lld[q], ref)
        print(f"S = {S}, row {q}: relative deviation {err:.3e}")
        if err >= reduce_worst["err"]:
            reduce_worst["err"], reduce_worst["at"] = err, (S, q)
        assert err <= 1e-12, (S, q, lld[q], float(ref))
    assert not np.array_equal(sll[0], sll[1])
    # the sweep can see any single sample go missing: each one's share of row 0's mean is at least
    # 1,000 bars (measured on the host oracle: 1.4e-8 of the mean at S = 8193, the bar 3.9e-12)
    ref0 = X.log_mean_exp_ld(sll[0])
    share = np.exp(sll[0].astype(np.longdouble) - ref0) / S
    assert float(share.min()) >= 1000 * 1e-12 * max(1.0, abs(float(ref0))), (S, float(share.min()))
    assert np.isnan(lld[2]) and np.all(np.isnan(sll[2]))
    for key in ("log_likelihoods_dla", "sample_log_likelihoods_dla", "log_likelihoods_no_dla"):
        np.testing.assert_array_equal(split[key], out[key], err_msg=key)

"""The training objective (csrc/objective.hip) at every rank bucket, pixel tile, pipeline and sum edge and
on its API branches, through training.objective / Objective / spectrum_loss, plain and with the forest.

The inputs and where each lands in the kernels' partition arithmetic come from tests/objective_cases.py;
tests/test_objective_cases.py checks on the CPU that they reach what they are named for and that the double
oracle agrees with the dense long-double reference to a tenth of the bars used here.

  A  k = 1 .. 64 on both sides of every obj_kb bucket edge (P = 77, Q = 11), the forest objective on one
     rank per bucket, spectrum_loss (omega2 passed in, Q = 1) on one rank per bucket
  B  P = 1 .. 257 around every multiple of 4, 16 and 32, P < k included, at k = 20 (VALU) and 40 (matrix cores)
  C  Q = 0 .. 1031 in one launch, then 70 spectra in launches of 1, 5, 32 and 33 (plain) and 33 (forest)
  D  (P, k) = (4096, 64), (4096, 32), (4096, 1), (1, 64)
  E  device-resident data, g = NULL, the GPDLA_EINVAL ladder, GPDLA_ENUMERIC and the handle after it

Reference: the dense long-double one up to P = 128, oracle.gpdla_oracle / forest_training_oracle above.
Bars (tests/test_training.py's): objective f rel 1e-11, g rtol 1e-8 / atol 1e-11 max|g|; spectrum_loss f rel
1e-11, dM and d log omega rtol 1e-9 / atol 1e-12 max, scalars rel 1e-9 / abs 1e-12; between launch
splittings f rel 1e-13, g rtol 1e-11 / atol 1e-13 max|g|.  Every case is evaluated twice on one handle
(bitwise equal).  The worst errors per family (f relative; each gradient block relative to its own largest
entry) are printed when the module is done.
"""
import ctypes as C
import json
import math
import sys
import time
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).parent))
import objective_cases as OC  # noqa: E402

from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import training as T  # noqa: E402

WORST = {}      # family -> {f, dM, dlog_omega, scalars}: worst error seen


@pytest.fixture(scope="module", autouse=True)
def require_device():
    lib = L.load()
    assert lib.gpdla_device_count() > 0, "no HIP device: GPU tests must run on the MI355X box"
    t0 = time.perf_counter()
    yield
    worst = {fam: {n: float(f"{v:.3e}") for n, v in sorted(w.items())} for fam, w in sorted(WORST.items())}
    print("\nobjective edges, worst errors: " + json.dumps(worst))
    print(f"objective edges, module wall time: {time.perf_counter() - t0:.1f} s")


def _record(family, f, fr, g, gr, P, k):
    w = WORST.setdefault(family, {})
    w["f"] = max(w.get("f", 0.0), abs(f - fr) / max(abs(fr), 1.0))
    gb, rb = OC.blocks(g, P, k), OC.blocks(gr, P, k)
    for name in rb:
        scale = np.abs(rb[name]).max() if rb[name].size else 0.0
        if scale > 0:
            w[name] = max(w.get(name, 0.0), float(np.abs(gb[name] - rb[name]).max() / scale))


def _evaluate(p, k, lines=0, times=1):
    """(f, g) of ``times`` evaluations on one handle."""
    with T.Objective(p["y"], p["lya"], p["nv"], k, z_qsos=p["z_qsos"] if lines else None,
                     num_forest_lines=lines or None) as obj:
        return [obj(p["x"]) for _ in range(times)]


def _assert_objective(family, f, g, ref, P, k, where):
    fr, gr = ref["f"], ref["g"]
    _record(family, f, fr, g, gr, P, k)
    assert np.isfinite(f) and np.all(np.isfinite(g)), where
    assert f == pytest.approx(fr, rel=1e-11), where
    np.testing.assert_allclose(g, gr, rtol=1e-8, atol=1e-11 * np.abs(gr).max(), err_msg=where)


def _family(c):
    return f"{c.family} {'forest' if c.lines else 'plain'} vs {OC.reference(c)['source']}"


def _check_case(c):
    p, ref, where = OC.case_problem(c), OC.reference(c), OC.case_id(c)
    (f, g), (f2, g2) = _evaluate(p, c.k, c.lines, times=2)
    assert f == f2 and np.array_equal(g, g2), where
    _assert_objective(_family(c), f, g, ref, c.P, c.k, where)
    # the all-NaN spectrum adds exactly 0 to f: with at most one spectrum per sum chunk (Q <= 64, one launch)
    # f is the spectra's values added in order, so taking a zero out leaves it bit for bit
    dead = p["all_nan_row"]
    if dead is not None and c.Q <= OC.SUM_CHUNKS:
        ((fw, _),) = _evaluate(OC.without_row(p, dead), c.k, c.lines)
        assert fw == f, where
    return f, g


# -------------------------------------------------------------------------------------- case A
@pytest.mark.parametrize("c", OC.CASES_A, ids=OC.case_id)
def test_every_rank_bucket_and_edge(c):
    _check_case(c)


@pytest.mark.parametrize("forest", [False, True], ids=["plain", "forest"])
@pytest.mark.parametrize("k", OC.A_LOSS_RANKS)
def test_spectrum_loss_on_every_bucket(k, forest):
    """omega2 is passed in (objective_omega2_kernel does not run), Q = 1, no NaN."""
    p, ref = OC.loss_problem(k, forest), OC.loss_reference(k, forest)
    extra = dict(z_qso=p["z_qso"], num_forest_lines=31) if forest else {}
    got = T.spectrum_loss(p["y"], p["lya"], p["nv"], p["M"], p["omega2"], OC.C_0, OC.TAU_0, OC.BETA, **extra)
    flat = lambda r: np.concatenate([r[1].ravel(order="F"), r[2], r[3:]])      # noqa: E731
    _record(f"A spectrum_loss {'forest' if forest else 'plain'} vs dense", got[0], ref[0], flat(got), flat(ref),
            OC.A_PIXELS, k)
    assert got[0] == pytest.approx(ref[0], rel=1e-11)
    np.testing.assert_allclose(got[1], ref[1], rtol=1e-9, atol=1e-12 * np.abs(ref[1]).max())
    np.testing.assert_allclose(got[2], ref[2], rtol=1e-9, atol=1e-12 * np.abs(ref[2]).max())
    for a, r in zip(got[3:], ref[3:]):
        assert a == pytest.approx(r, rel=1e-9, abs=1e-12)


# -------------------------------------------------------------------------------------- case B
@pytest.mark.parametrize("c", OC.CASES_B, ids=OC.case_id)
def test_every_pixel_edge_on_both_paths(c):
    _check_case(c)


# -------------------------------------------------------------------------------------- case C
@pytest.mark.parametrize("c", [c for c in OC.CASES_C if c.Q > 0], ids=OC.case_id)
def test_every_spectrum_count_in_one_launch(c):
    _check_case(c)


def _priors(x):
    """objective.m:59-71 as gpdla_objective_eval forms them (libm's exp, the same products)."""
    t0, b = math.exp(x[-2]), math.exp(x[-1])
    return (t0 * (t0 - OC.TAU_0_MU) / (OC.TAU_0_SIGMA * OC.TAU_0_SIGMA),
            b * (b - OC.BETA_MU) / (OC.BETA_SIGMA * OC.BETA_SIGMA))


def test_no_spectra():
    """Q = 0: no launch; f = 0, a zero gradient but for the two prior terms.  At the drawn x the scalars sit
    on the prior means and the terms are rounding residue: one ulp of tau_0 = exp(x) moves tau_0 (tau_0 - mu) /
    sigma^2 by 0.0023 x 4.3e-19 / 4.9e-7 = 2e-15 and one ulp of beta moves its term by 3.65 x 4.4e-16 / 0.0441
    = 3.7e-14, hence abs 1e-13 there; off the means the terms are compared relatively (1e-12, the bar of
    test_oracle_objective_sums_spectra_and_adds_priors_to_g_only)."""
    c = OC.CASES_C[0]
    assert c.Q == 0
    p = OC.case_problem(c)
    n = c.P * (c.k + 1)
    x_off = p["x"].copy()
    x_off[-2:] = np.log([0.003, 3.5])
    with T.Objective(p["y"], p["lya"], p["nv"], c.k) as obj:
        for x, tol in ((p["x"], dict(abs=1e-13)), (x_off, dict(rel=1e-12))):
            (f, g), (f2, g2) = obj(x), obj(x)
            assert f == 0.0 and f2 == 0.0 and np.array_equal(g, g2)
            assert not g[:n].any() and g[n] == 0.0
            assert g[n + 1] == pytest.approx(_priors(x)[0], **tol) and g[n + 2] == pytest.approx(_priors(x)[1], **tol)
    assert g[n + 1] == pytest.approx(0.003 * 0.0007 / 0.0007 ** 2, rel=1e-9)


def test_an_all_nan_spectrum_alone_is_zero():
    p = OC.problem(3, OC.C_PIXELS, OC.C_RANK, 300)
    q = p["all_nan_row"]
    only = dict(p, Q=1, y=p["y"][q:q + 1], lya=p["lya"][q:q + 1], nv=p["nv"][q:q + 1])
    ((f, g),) = _evaluate(only, OC.C_RANK)
    n = OC.C_PIXELS * (OC.C_RANK + 1)
    assert f == 0.0 and not g[:n + 1].any()


_one_launch = {}


def _one_launch_result(c):
    key = c._replace(batch=None)
    if key not in _one_launch:
        _one_launch[key] = _evaluate(OC.case_problem(c), c.k, c.lines)[0]
    return _one_launch[key]


@pytest.mark.parametrize("c", OC.CASES_C_LAUNCHES, ids=OC.case_id)
def test_launch_splittings(c, monkeypatch):
    """GPDLA_OBJECTIVE_BATCH = 33: launches of 33, 33 and 4, the last one's 32-spectrum tile holding the
    operand rows of the launch before; the forest case moves the z_QSO array with the batch."""
    f1, g1 = _one_launch_result(c)
    monkeypatch.setenv("GPDLA_OBJECTIVE_BATCH", str(c.batch))
    fb, gb = _check_case(c)
    scale = np.abs(g1).max()
    w = WORST.setdefault("C launches vs one launch", {})
    w["f"] = max(w.get("f", 0.0), abs(fb - f1) / max(abs(f1), 1.0))
    w["g"] = max(w.get("g", 0.0), float(np.abs(gb - g1).max() / scale))
    assert fb == pytest.approx(f1, rel=1e-13)
    np.testing.assert_allclose(gb, g1, rtol=1e-11, atol=1e-13 * scale)


# -------------------------------------------------------------------------------------- case D
@pytest.mark.parametrize("c", OC.CASES_D, ids=OC.case_id)
def test_documented_limits(c):
    _check_case(c)


# -------------------------------------------------------------------------------------- case E
def _create(Q, P, k, y, lya, nv, memory, out="handle", device=0):
    """gpdla_objective_create as called from C -> (rc, handle value)."""
    h = C.c_void_p(1)          # not NULL going in: the call must clear it
    rc = L.load().gpdla_objective_create(device, Q, P, k, y, lya, nv, memory, C.byref(h) if out == "handle" else None)
    return rc, h.value


def _eval_raw(h, x, want_g=True):
    f = np.full(1, np.nan)
    g = np.full(x.size, np.nan) if want_g else None
    rc = L.load().gpdla_objective_eval(h, L.ptr(x), L.ptr(f), L.ptr(g))
    return rc, float(f[0]), g


def _e_problem():
    Q, P, k = OC.E_SHAPE
    return OC.problem(Q, P, k, 500)


def test_device_resident_data_and_null_gradient():
    """E1: GPDLA_MEM_DEVICE data (the handle borrows it) gives what the host-memory handle gives, bit for
    bit; E2: g = NULL gives the same f."""
    Q, P, k = OC.E_SHAPE
    p = _e_problem()
    ((fh, gh),) = _evaluate(p, k)
    bufs = [L.DeviceArray.from_numpy(p[name]) for name in ("y", "lya", "nv")]
    try:
        rc, h = _create(Q, P, k, *[L.dev_ptr(b.ptr) for b in bufs], L.MEM_DEVICE)
        assert rc == L.GPDLA_OK and h
        try:
            rc, fd, gd = _eval_raw(C.c_void_p(h), p["x"])
            assert rc == L.GPDLA_OK
            rc, fn, _ = _eval_raw(C.c_void_p(h), p["x"], want_g=False)
            assert rc == L.GPDLA_OK
        finally:
            L.load().gpdla_objective_destroy(C.c_void_p(h))
        # the data outlives the handle that borrowed it
        assert np.array_equal(bufs[0].numpy(), p["y"], equal_nan=True)
    finally:
        for b in bufs:
            b.free()
    assert fd == fh and np.array_equal(gd, gh) and fn == fh
    _assert_objective("E plain vs dense", fd, gd, OC.reference(OC.Case("E", Q, P, k, 0, None, 500)), P, k, "E1")


def test_argument_errors():
    """E3: every refusal of gpdla_objective_create leaves a null handle; gpdla_objective_eval refuses a null x
    or f."""
    Q, P, k = OC.E_SHAPE
    p = _e_problem()
    data = [L.ptr(p[name]) for name in ("y", "lya", "nv")]
    for what, args in (("k = 0", (Q, P, 0, *data, L.MEM_HOST)), ("k = 65", (Q, P, OC.MAX_K + 1, *data, L.MEM_HOST)),
                       ("P = 0", (Q, 0, k, *data, L.MEM_HOST)), ("P = 4097", (Q, OC.MAX_PIXELS + 1, k, *data, L.MEM_HOST)),
                       ("Q = -1", (-1, P, k, *data, L.MEM_HOST)), ("memory kind", (Q, P, k, *data, 7)),
                       ("null y", (Q, P, k, None, data[1], data[2], L.MEM_HOST)),
                       ("null lya", (Q, P, k, data[0], None, data[2], L.MEM_HOST)),
                       ("null noise", (Q, P, k, data[0], data[1], None, L.MEM_HOST))):
        rc, h = _create(*args)
        assert rc == L.GPDLA_EINVAL and h is None, what
    rc, _ = _create(Q, P, k, *data, L.MEM_HOST, out=None)
    assert rc == L.GPDLA_EINVAL
    rc, h = _create(Q, P, k, *data, L.MEM_HOST)
    assert rc == L.GPDLA_OK and h
    try:
        f, g = np.empty(1), np.empty(p["x"].size)
        lib = L.load()
        assert lib.gpdla_objective_eval(C.c_void_p(h), None, L.ptr(f), L.ptr(g)) == L.GPDLA_EINVAL
        assert lib.gpdla_objective_eval(C.c_void_p(h), L.ptr(p["x"]), None, L.ptr(g)) == L.GPDLA_EINVAL
        assert lib.gpdla_objective_eval(None, L.ptr(p["x"]), L.ptr(f), L.ptr(g)) == L.GPDLA_EINVAL
        rc, fv, _ = _eval_raw(C.c_void_p(h), p["x"])                          # and the handle still works
        assert rc == L.GPDLA_OK and np.isfinite(fv)
    finally:
        L.load().gpdla_objective_destroy(C.c_void_p(h))


def test_non_positive_pivot_is_reported_and_leaves_nothing_behind():
    """E4: a spectrum whose B has a negative first pivot (tests/test_objective_cases.py: scipy's cholesky
    refuses the same B) returns GPDLA_ENUMERIC; the handle then evaluates a point where the covariance is
    positive definite bit for bit as a fresh handle does, and to the bars."""
    Q, P, k = OC.E_SHAPE
    e = OC.e4_problem()
    with T.Objective(e["y"], e["lya"], e["nv"], k) as obj:
        with pytest.raises(L.GpdlaNumericError) as err:
            obj(e["x_bad"])
        assert err.value.code == L.GPDLA_ENUMERIC
        f, g = obj(e["x_good"])
    with T.Objective(e["y"], e["lya"], e["nv"], k) as fresh:
        f2, g2 = fresh(e["x_good"])
    assert f == f2 and np.array_equal(g, g2)
    fr, gr = OC.dense_objective(e["x_good"], e["y"], e["lya"], e["nv"])
    _assert_objective("E plain vs dense", f, g, dict(f=fr, g=gr), P, k, "E4 good point")

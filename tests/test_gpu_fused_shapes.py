"""The fused fp64 sweep (kernels.hip prep_kernel<K>, likelihood_kernel<K, NL>) at every pixel count,
rank, line placement and block edge, against the oracle.

The inputs and where each lands in the kernel's decomposition come from tests/fused_shape_cases.py;
tests/test_fused_shape_cases.py checks on the CPU that they reach what they are named for.

  A  J = 1..100 pixels on the shipped three-line kernel at rank 12 (odd tile count) and 20 (even):
     every chunk count 1..7, every phase of the 5-unrolled chunk loop and its wrap, every J mod 4 and
     L mod 4; the same batch plus J = 127..257 on the int8 fused path against the fp64 one.
  B  every compiled rank (and 11, zero-padded into 12) x {3, 2} lines x both absorption modes.
  C  Lyman-line centres on every padded index of a 22- and an 85-pixel spectrum, in every Voigt zone:
     every (segment, chunk step, phase) and every window-prologue position in a core zone.
  D  masks on segment edges, an all-masked spectrum between usable ones, out-of-range pixels in front.
  E  S + 1 lanes around the 64-sample block (the null model last in a block, alone in a block, one
     past that) x spectrum counts around the grid's padding to a multiple of 8.

Error: max |got - want| / max(|want|, 1).  Bars (the suite's regression bars): 1e-9 for the fused fp64
path against oracle/gpdla_oracle.py process_spectrum, 1e-11 between the fused and the panel-GEMM fp64
paths, I8_TOL of test_gpu_i8.py for the int8 fused path against the fp64 one.
"""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).parent))
import fused_shape_cases as F  # noqa: E402
from test_gpu_i8 import I8_TOL  # noqa: E402

from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import Engine  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402
from oracle import gpdla_oracle as O  # noqa: E402

ORACLE_TOL = 1e-9
PANEL_TOL = 1e-11
KEYS = ("sample_log_likelihoods_dla", "log_likelihoods_no_dla", "log_likelihoods_dla")
WORST = {}      # case -> worst error seen, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def require_device():
    lib = L.load()
    assert lib.gpdla_device_count() > 0, "no HIP device: GPU tests must run on the MI355X box"
    yield
    print("\nfused shapes, worst errors: " + json.dumps({k: float(f"{v:.3e}") for k, v in sorted(WORST.items())}))


# the oracle results, once per module (fused_shape_cases memoises them and hands them out read-only)
@pytest.fixture(scope="module")
def oracle_a():
    return {k: F.case_a_oracle(k) for k in (12, 20)}


@pytest.fixture(scope="module")
def oracle_b():
    return {(k, nl, mode): F.case_b_oracle(k, nl, mode) for k in F.B_RANKS for nl in F.B_LINES for mode in F.B_MODES}


@pytest.fixture(scope="module")
def oracle_c():
    return {J: F.case_c_oracle(J) for J in F.C_PIXELS}


@pytest.fixture(scope="module")
def oracle_d():
    return {(J, mode): F.case_d_oracle(J, mode) for J in F.D_PIXELS for mode in F.B_MODES}


@pytest.fixture(scope="module")
def oracle_e():
    return F.case_e_oracle()


def _run(k, samples, spectra, path="fused", max_batch_spectra=0, **params):
    with Engine(F.model(k), samples, set_parameters(k=k, **params), path=path,
                max_batch_spectra=max_batch_spectra) as eng:
        return eng.process(syn.pack_spectra(spectra))


def _row_errors(got, want, rows=slice(None)):
    """Per spectrum, the worst error over the per-sample, null and evidence outputs (inf where an
    output is not finite)."""
    errs = []
    for key in KEYS:
        g, w = np.asarray(got[key], float)[rows], np.asarray(want[key], float)
        e = np.abs(g - w) / np.maximum(np.abs(w), 1.0)
        e = np.where(np.isfinite(g), e, np.inf)
        errs.append(e.max(axis=1) if e.ndim == 2 else e)
    return np.max(errs, axis=0)


def _record(case, errs):
    WORST[case] = max(WORST.get(case, 0.0), float(np.max(errs)))


def _shape_name(k, J):
    d = F.decompose(int(J))
    return f"(k={k}, J={d['J']}, L={d['L']}, nchunks={d['nchunks']})"


# -------------------------------------------------------------------------------------- case A
@pytest.mark.parametrize("k", [12, 20])
def test_every_pixel_count_on_the_three_line_kernel(oracle_a, k):
    """J = 1..100 in one batch, 65 samples (the null model alone in the second block)."""
    out = _run(k, syn.make_samples(F.A_SAMPLES), F.case_a_spectra(k))
    np.testing.assert_array_equal(out["num_pixels"], F.A_PIXELS)
    errs = _row_errors(out, oracle_a[k])
    _record(f"A fused k={k}", errs)
    print(f"case A k={k}: worst {errs.max():.3e} at J={F.A_PIXELS[int(errs.argmax())]}")
    bad = [f"{_shape_name(k, J)}: {e:.3e}" for J, e in zip(F.A_PIXELS, errs) if not e < ORACLE_TOL]
    assert not bad, "\n".join(bad)


def test_every_pixel_count_on_the_int8_fused_path():
    """The same batch and J = 127..257 (convert_i8_kernel's 16-step chunks: ceil(L / 16) up to 5) on
    fused_i8 against the fp64 fused kernel."""
    k, samples, spectra = 20, syn.make_samples(F.A_SAMPLES), F.case_a_spectra(20, F.A_PIXELS_I8)
    ref = _run(k, samples, spectra)
    out = _run(k, samples, spectra, path="fused_i8")
    np.testing.assert_array_equal(out["num_pixels"], F.A_PIXELS_I8)
    errs = _row_errors(out, ref)
    _record("A fused_i8 vs fused", errs)
    print(f"case A i8: worst {errs.max():.3e} at J={F.A_PIXELS_I8[int(errs.argmax())]}")
    bad = [f"{_shape_name(k, J)}: {e:.3e}" for J, e in zip(F.A_PIXELS_I8, errs) if not e < I8_TOL]
    assert not bad, "\n".join(bad)


# -------------------------------------------------------------------------------------- case B
@pytest.mark.parametrize("mode", F.B_MODES)
@pytest.mark.parametrize("num_lines", F.B_LINES)
@pytest.mark.parametrize("k", F.B_RANKS)
def test_every_rank_line_count_and_mode(oracle_b, k, num_lines, mode):
    """likelihood_kernel<K, 3> and <K, 0> of every compiled K (k = 11 runs on 12, zero-padded), pixel
    counts around 4, 16 and 64 with 10% masked pixels from J = 5 on."""
    samples, spectra = syn.make_samples(F.B_SAMPLES), F.case_b_spectra(k)
    ref = oracle_b[k, num_lines, mode]
    out = _run(k, samples, spectra, num_lines=num_lines, absorption_mode=mode)
    np.testing.assert_array_equal(out["num_pixels"], ref["num_pixels"])
    swept = [F.kernel_positions(n, m, mode) for n, m in zip(ref["num_pixels"], ref["m"])]
    errs = _row_errors(out, ref)
    _record(f"B fused lines={num_lines}", errs)
    bad = [f"{_shape_name(k, J)} lines={num_lines} {mode}: {e:.3e}" for J, e in zip(swept, errs) if not e < ORACLE_TOL]
    assert not bad, "\n".join(bad)
    if num_lines == 3 and mode == "reference":
        gemm = _run(k, samples, spectra, path="panel_gemm")
        errs = _row_errors(out, gemm)
        _record("B fused vs panel_gemm", errs)
        bad = [f"{_shape_name(k, J)} vs panel_gemm: {e:.3e}" for J, e in zip(swept, errs) if not e < PANEL_TOL]
        assert not bad, "\n".join(bad)


# -------------------------------------------------------------------------------------- case C
def _centre_names(c, failing):
    """The failing samples by where their line centre sits: (line, padded index, dx, (g, tt, phase))."""
    s = c["samples"]
    names = sorted({(int(s["line"][i]), int(s["index"][i]), float(s["dx"][i]),
                     F.centre_slot(c["J"], int(s["index"][i]))) for i in failing})
    slots = sorted({n[3] for n in names if n[3] is not None})
    all_tt = [(F.centre_slot(c["J"], int(i)) or (None, None))[1] for i in s["index"]]
    by_tt = {tt: f"{sum(all_tt[i] == tt for i in failing)}/{all_tt.count(tt)}" for tt in (None, 0, 1, 2, 3)}
    return (f"{len(failing)} samples; failing/all by the centre's chunk step (None: prologue of segment 0): {by_tt}; "
            f"centre slots (g, tt, phase): {slots}; first (line, index, dx, slot): {names[:12]}")


@pytest.mark.parametrize("J", F.C_PIXELS)
def test_line_centres_at_every_slot_of_a_short_spectrum(oracle_c, J):
    """Every padded index 0 .. J + 5 carries the centre of each of the three lines of some sample, and
    one at dx = 4.5, -8.9, 9.1, -20, 31.9, -32.1 and 40 Doppler units from it, at N_HI = 1e20 and
    10^22.5.  The offsets are NOT restricted to [0, 1]: on a spectrum this short the Ly-beta and
    Ly-gamma centres (and most Ly-alpha ones) need offsets far outside it; the engine takes any finite
    offset and the oracle applies the same affine z_DLA = zmin + (zmax - zmin) offset.  J = 22 is
    L = 6 in segments of Ls = 8 rows (two neutral rows inside every segment), J = 85 is L = 22, six
    chunks: all five phases and the wrap."""
    c = F.case_c(J)
    ref = oracle_c[J]
    out = _run(F.C_RANK, c["samples"], [c["spec"]])
    i8 = _run(F.C_RANK, c["samples"], [c["spec"]], path="fused_i8")
    # per sample first (a non-finite value counts as an infinite error), so that a failure names the
    # slots its line centres sit on; then all three outputs
    for name, got, want, tol in (("fused", out, ref, ORACLE_TOL), ("fused_i8 vs fused", i8, out, I8_TOL)):
        g, w = got["sample_log_likelihoods_dla"][0], want["sample_log_likelihoods_dla"][0]
        err = np.where(np.isfinite(g), np.abs(g - w) / np.maximum(np.abs(w), 1.0), np.inf)
        print(f"case C J={J} {name}: worst {err.max():.3e}")
        failing = np.flatnonzero(~(err < tol))
        assert failing.size == 0, f"{name}: {_centre_names(c, failing)}"
        for key in KEYS:
            assert np.all(np.isfinite(got[key])), (name, key)
        errs = _row_errors(got, want)
        _record(f"C {name} J={J}", errs)
        assert errs[0] < tol, name


# -------------------------------------------------------------------------------------- case D
@pytest.mark.parametrize("mode", F.B_MODES)
@pytest.mark.parametrize("J", F.D_PIXELS)
def test_masks_on_segment_edges(oracle_d, J, mode):
    """All patterns in one batch: the all-masked spectrum gives NaN in all three outputs and leaves its
    neighbours (the rows before and after it) as the oracle has them."""
    spectra = F.case_d_spectra(J)
    out = _run(F.D_RANK, syn.make_samples(F.D_SAMPLES), spectra, absorption_mode=mode)
    dead = F.D_PATTERNS.index("all_masked")
    usable = [q for q in range(len(F.D_PATTERNS)) if q != dead]
    assert 0 < dead < len(F.D_PATTERNS) - 1
    np.testing.assert_array_equal(out["num_pixels"], [F.case_d_expected(J, p)[0] for p in F.D_PATTERNS])
    for key in KEYS:
        assert np.all(np.isnan(out[key][dead])), key
    errs = _row_errors(out, oracle_d[J, mode], rows=usable)
    _record("D fused", errs)
    bad = [f"{F.D_PATTERNS[q]} J={J} {mode}: {e:.3e}" for q, e in zip(usable, errs) if not e < ORACLE_TOL]
    assert not bad, "\n".join(bad)


# -------------------------------------------------------------------------------------- case E
def _e_runs(S, Q):
    """The batch of Q spectra at S samples; the 9-spectrum batch (an unusable spectrum in the middle)
    also in device batches of 2."""
    samples, spectra = syn.make_samples(S), F.case_e_spectra(Q)
    runs = [("one batch", _run(F.E_RANK, samples, spectra))]
    if Q == 9:
        runs.append(("batches of 2", _run(F.E_RANK, samples, spectra, max_batch_spectra=2)))
    return runs


@pytest.fixture(scope="module")
def e_full():
    return {Q: _e_runs(max(F.E_SAMPLES), Q)[0][1] for Q in F.E_SPECTRA}


@pytest.mark.parametrize("S", F.E_SAMPLES)
def test_block_and_grid_edges(oracle_e, e_full, S):
    """S + 1 lanes per spectrum in blocks of 64: S = 63 puts the null model in the last lane of a
    block, 64 alone in a block of its own, 65 one past that (and likewise 15..17 within a wave's 16
    and 127..129).  Q = 1, 3, 8, 9 spectra make grids of Q ceil((S + 1) / 64) blocks padded to a
    multiple of 8 for the XCD remap.  Every value agrees with the oracle, and, each sample's arithmetic
    being independent of the lanes around it (engine.hip), every run's first S columns and nulls are
    bitwise those of the S = 129 run."""
    for Q in F.E_SPECTRA:
        usable = [q for q in range(Q) if not (Q == 9 and q == F.E_UNUSABLE)]
        want = dict(sample_log_likelihoods_dla=oracle_e["sample_log_likelihoods_dla"][usable, :S],
                    log_likelihoods_no_dla=oracle_e["log_likelihoods_no_dla"][usable],
                    log_likelihoods_dla=np.array([O.log_mean_exp(oracle_e["sample_log_likelihoods_dla"][q, :S])
                                                  for q in usable]))
        full = e_full[Q]
        for name, out in _e_runs(S, Q):
            where = f"S={S} Q={Q} {name}"
            assert out["sample_log_likelihoods_dla"].shape == (Q, S), where
            errs = _row_errors(out, want, rows=usable)
            _record("E fused", errs)
            bad = [f"{where} q={q}: {e:.3e}" for q, e in zip(usable, errs) if not e < ORACLE_TOL]
            assert not bad, "\n".join(bad)
            nulls = np.abs(out["log_likelihoods_no_dla"][usable] - want["log_likelihoods_no_dla"])
            assert np.all(nulls < ORACLE_TOL * np.maximum(np.abs(want["log_likelihoods_no_dla"]), 1.0)), where
            if Q == 9:
                for key in KEYS:
                    assert np.all(np.isnan(out[key][F.E_UNUSABLE])), (where, key)
            assert np.array_equal(out["sample_log_likelihoods_dla"], full["sample_log_likelihoods_dla"][:, :S],
                                  equal_nan=True), where
            assert np.array_equal(out["log_likelihoods_no_dla"], full["log_likelihoods_no_dla"], equal_nan=True), where


# ---------------------------------------------------------------------------- offset validation
def test_non_finite_offsets_rejected():
    """NaN and +-inf offsets are refused at engine creation (GPDLA_EINVAL, naming the index) before the
    samples are sorted by offset; finite offsets outside [0, 1] are accepted."""
    model = F.model(20)
    base = syn.make_samples(16)
    for bad in (np.nan, np.inf, -np.inf):
        off = base["offset_samples"].copy()
        off[5] = bad
        with pytest.raises(L.GpdlaError, match=r"offset_samples\[5\]"):
            Engine(model, dict(base, offset_samples=off), set_parameters(k=20))
    off = base["offset_samples"].copy()
    off[5], off[6] = -0.5, 1.5
    spec = F.short_spectrum(20, 0, 40)
    with Engine(model, dict(base, offset_samples=off), set_parameters(k=20)) as eng:
        out = eng.process(syn.pack_spectra([spec]))
    ref = F.oracle(spec, 20, dict(base, offset_samples=off))
    assert np.all(np.isfinite(out["sample_log_likelihoods_dla"]))
    err = np.abs(out["sample_log_likelihoods_dla"][0] - ref["sample_log_likelihoods_dla"])
    assert np.all(err < ORACLE_TOL * np.maximum(np.abs(ref["sample_log_likelihoods_dla"]), 1.0))

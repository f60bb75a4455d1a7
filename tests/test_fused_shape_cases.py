"""The inputs of tests/test_gpu_fused_shapes.py land where they claim (CPU, oracle only).

A green device run means something only if its inputs reach the branches they are named for: every
chunk count, phase and L mod 4 of the fused sweep (case A), a line centre in every Voigt zone at
every slot and window-prologue position (case C), the (n, m) of every mask pattern (case D), and
finite oracle results for every spectrum meant to be usable.  These are conditions on the inputs,
computed from the kernel's decomposition (tests/fused_shape_cases.py), not on any kernel output.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import fused_shape_cases as F  # noqa: E402

from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from oracle import gpdla_oracle as O  # noqa: E402

KEYS = ("sample_log_likelihoods_dla", "log_likelihoods_no_dla", "log_likelihoods_dla")


def _finite(ref):
    return all(np.all(np.isfinite(ref[k])) for k in KEYS)


# -------------------------------------------------------------------------------------- case A
def _pixel_sweep_gaps(pixels):
    """What a pixel-count list leaves uncovered of: nchunks 1..7, at each nchunks >= 2 every J mod 4,
    and at each nchunks 2..6 every L mod 4 (nchunks = 7 is L = 25..28, i.e. J = 97..112: a sweep that
    ends at J = 100 reaches it at L = 25 only, with every J mod 4)."""
    decs = [F.decompose(J) for J in pixels]
    gaps = [("nchunks", nc) for nc in range(1, 8) if nc not in {d["nchunks"] for d in decs}]
    for nc in range(2, 8):
        here = [d for d in decs if d["nchunks"] == nc]
        if nc < 7:
            gaps += [("L mod 4", nc, r) for r in range(4) if r not in {d["L"] % 4 for d in here}]
        gaps += [("J mod 4", nc, r) for r in range(4) if r not in {d["J"] % 4 for d in here}]
    return gaps


def test_pixel_sweep_reaches_every_chunk_count_phase_and_remainder():
    assert _pixel_sweep_gaps(F.A_PIXELS) == []
    phases = {F.position(p, J)["phase"] for J in F.A_PIXELS for p in range(J)}
    assert phases == set(range(F.UNROLL))
    # the wrap into a second round of the 5-unroll: chunks 5 and 6 run in phases 0 and 1 again
    chunks = {F.position(p, J)["c"] for J in F.A_PIXELS for p in range(J)}
    assert {5, 6} <= chunks
    # the check is a real one: without the longest spectra nchunks = 6, 7 (J = 81..100) are missed
    assert ("nchunks", 7) in _pixel_sweep_gaps(range(1, 81))
    assert ("nchunks", 6) in _pixel_sweep_gaps(range(1, 81))


def test_pixel_sweep_spectra_have_the_pixel_counts_they_are_named_for():
    for J, spec in zip(F.A_PIXELS_I8, F.case_a_spectra(20, F.A_PIXELS_I8)):
        assert F.count_pixels(spec) == (J, J)
    nch16 = [(F.decompose(J)["L"] + 15) // 16 for J in F.A_PIXELS_I8[len(F.A_PIXELS):]]
    assert nch16 == [2, 2, 3, 3, 4, 5]


@pytest.mark.parametrize("k", [12, 20])
def test_pixel_sweep_oracle_is_finite_and_near_the_lines(k):
    ref = F.case_a_oracle(k)
    assert _finite(ref)
    np.testing.assert_array_equal(ref["num_pixels"], F.A_PIXELS)
    # Ly-alpha of the samples crosses the pixels: at J = 100 a good share of the (sample, padded pixel)
    # pairs lies inside the fix-up zone and inside the core
    spec = F.case_a_spectra(k)[-1]
    prep = O.prepare_spectrum(spec["wavelengths"], spec["flux"], spec["noise_variance"], spec["pixel_mask"],
                              spec["z_qso"], F.model(k))
    samples = syn.make_samples(F.A_SAMPLES)
    z = prep["zmin"] + (prep["zmax"] - prep["zmin"]) * samples["offset_samples"]
    ax = np.abs(F.doppler_x(prep["padded"], z)).min(axis=2)
    assert np.count_nonzero(ax < F.OUTER_X) > 500 and np.count_nonzero(ax < F.CORE_X) > 100


# -------------------------------------------------------------------------------------- case B
@pytest.mark.parametrize("k", F.B_RANKS)
def test_rank_sweep_oracle_is_finite(k):
    for nl in F.B_LINES:
        for mode in F.B_MODES:
            ref = F.case_b_oracle(k, nl, mode)
            assert _finite(ref), (k, nl, mode)
            np.testing.assert_array_equal(ref["m"], F.B_PIXELS)
            assert np.all(ref["num_pixels"] >= 1)
    # masks are present from J = 5 on, so the two modes sweep different position counts
    ref = F.case_b_oracle(k, 3, "reference")
    assert np.any(ref["num_pixels"] < ref["m"])


# -------------------------------------------------------------------------------------- case C
ZONES = ((0.0, F.CORE_X), (F.CORE_X, F.OUTER_X), (F.OUTER_X, 40.0))


def _centre_gaps(c):
    """Padded indices x lines with no sample on the centre (|x| < 1e-3), or none in some zone."""
    ax = np.abs(c["x"])                                        # [s, i, j]
    gaps = [("centre", i, j) for i, j in zip(*np.nonzero(~np.any(ax < 1e-3, axis=0)))]
    for lo, hi in ZONES:
        inside = np.any((ax > lo) & (ax < hi) & (ax >= 1e-3), axis=0)
        gaps += [((lo, hi), i, j) for i, j in zip(*np.nonzero(~inside))]
    return gaps


def _core_coverage(c):
    """(segment, chunk step, phase) triples and window-prologue (segment, position) pairs that lie in
    the core zone of some sample and line, from the decomposition of where each padded index is
    evaluated."""
    J = c["J"]
    core_at = np.any(np.abs(c["x"]) < F.CORE_X, axis=(0, 2))   # per padded index
    triples = set()
    for p in range(J):
        d = F.position(p, J)
        if core_at[d["padded_index"]]:
            triples.add((d["g"], d["tt"], d["phase"]))
    prologue = {(g, i) for g in range(1, 4) for i, idx in enumerate(F.prologue_indices(J, g)) if core_at[idx]}
    return triples, prologue


@pytest.mark.parametrize("J", F.C_PIXELS)
def test_line_centres_reach_every_index_zone_slot_and_prologue(J):
    c = F.case_c(J)
    assert c["padded"].size == J + 6
    assert np.all(np.isfinite(c["samples"]["offset_samples"]))
    # on a spectrum this short most centres need an offset outside [0, 1]
    off = c["samples"]["offset_samples"]
    assert np.count_nonzero((off < 0) | (off > 1)) > off.size // 2
    assert _centre_gaps(c) == []
    triples, prologue = _core_coverage(c)
    assert triples == F.slot_triples(J)
    assert prologue == {(g, i) for g in range(1, 4) for i in range(6)}
    d = F.decompose(J)
    if J == 22:
        assert (d["L"], d["Ls"]) == (6, 8)            # two neutral rows inside every segment
    else:
        assert (d["L"], d["nchunks"]) == (22, 6)      # all five phases plus the wrap
        assert {t[2] for t in triples} == set(range(5))
    assert _finite(F.case_c_oracle(J))


def test_line_centre_coverage_needs_the_centred_samples():
    """The coverage above is a real check: without the dx = 0 samples no index carries a centre."""
    c = F.case_c(22, tuple(dx for dx in F.C_DX if dx != 0.0))
    gaps = _centre_gaps(c)
    assert len([g for g in gaps if g[0] == "centre"]) == (22 + 6) * F.LINES


# -------------------------------------------------------------------------------------- case D
@pytest.mark.parametrize("J", F.D_PIXELS)
def test_mask_patterns_yield_their_pixel_counts(J):
    spectra = F.case_d_spectra(J)
    for pattern, spec in zip(F.D_PATTERNS, spectra):
        want = F.case_d_expected(J, pattern)
        assert F.count_pixels(spec) == want, pattern
        if pattern == "all_masked":
            assert want[0] == 0
            assert F.kernel_positions(*want, "reference") == F.kernel_positions(*want, "unmasked") == 0
            continue
        for mode in F.B_MODES:
            prep = O.prepare_spectrum(spec["wavelengths"], spec["flux"], spec["noise_variance"],
                                      spec["pixel_mask"], spec["z_qso"], F.model(F.D_RANK), mode)
            assert (prep["n"], prep["m"]) == want, (pattern, mode)
            # reference mode keeps the first n profile values, unmasked mode those of the unmasked pixels
            assert prep["absorption_index"].size == want[0]
    blue = spectra[F.D_PATTERNS.index("blue_prepended")]
    rest = blue["wavelengths"] / (1 + blue["z_qso"])
    assert np.all(rest[:5] < O.MIN_LAMBDA) and np.all(rest[5:] >= O.MIN_LAMBDA) and rest.size == J + 5
    for mode in F.B_MODES:
        ref = F.case_d_oracle(J, mode)
        assert _finite(ref), mode
        assert ref["num_pixels"].size == len(F.D_PATTERNS) - 1


# -------------------------------------------------------------------------------------- case E
def test_block_edge_samples_are_prefixes_and_the_oracle_is_finite():
    big = syn.make_samples(max(F.E_SAMPLES))
    for S in F.E_SAMPLES:
        small = syn.make_samples(S)
        for key in ("offset_samples", "nhi_samples"):
            np.testing.assert_array_equal(small[key], big[key][:S])
    # the null model (lane S) on the last lane of a block, alone in a block, and one past that
    assert {(S + 1) % 64 for S in F.E_SAMPLES} >= {0, 1, 2}
    assert _finite(F.case_e_oracle())
    nine = F.case_e_spectra(9)
    assert F.count_pixels(nine[F.E_UNUSABLE]) == (0, 0)
    assert all(F.count_pixels(s) == (F.E_PIXELS, F.E_PIXELS) for q, s in enumerate(nine) if q != F.E_UNUSABLE)

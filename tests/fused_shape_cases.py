"""Inputs that pin the fused fp64 sweep (kernels.hip prep_kernel<K> / likelihood_kernel<K, NL>) at
every pixel count, rank and block edge, with the place each input takes in the kernel's decomposition.

The sweep splits a spectrum's J pixel-order positions (J = n in the "reference" absorption mode, m in
"unmasked") into 4 segments of L = ceil(J / 4) steps; a segment runs in nchunks = ceil(L / 4) chunks of
4 steps (rows t >= L of the last chunk are neutral), the chunk loop is unrolled by 5 over a ring of ten
window registers, so chunk c runs in phase c % 5.  Position p is segment g = p // L, step t = p % L,
chunk c = t // 4, chunk step tt = t % 4; the raw profile evaluated at that slot is the one at padded
index p + 6, and segment g's window prologue holds padded indices g L .. g L + 5.

Cases (tests/test_fused_shape_cases.py checks on the CPU that they land where they claim;
tests/test_gpu_fused_shapes.py runs them on the device):

  A  every pixel count 1..100 (plus a few longer ones for the int8 conversion's 16-step chunks)
  B  every compiled rank x line count {3, 2} x absorption mode, pixel counts around 4, 16 and 64
  C  Lyman-line centres on every padded index of a short spectrum, in every Voigt zone
  D  masks on segment edges
  E  sample counts around the 64-sample block, spectrum counts around the 8-XCD grid padding

The oracle results are computed once per process (lru_cache) and returned read-only.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from gp_dla_detection_amd import parameters as P
from gp_dla_detection_amd import synthetic as syn
from oracle import gpdla_oracle as O

Z_QSO = 2.9
CHUNK_STEPS = 4          # kChunkSteps
UNROLL = 5               # phases of the chunk loop
CORE_X, OUTER_X = 9.0, 32.0   # kCoreX, kOuterX: core | inner wing | outer wing, in Doppler units
LINES = 3


# ------------------------------------------------------------------------------- decomposition
def decompose(J: int) -> dict:
    """L, nchunks and the padded segment stride Ls of a spectrum with J pixel-order positions."""
    L = (J + 3) // 4
    nchunks = (L + CHUNK_STEPS - 1) // CHUNK_STEPS
    return dict(J=J, L=L, nchunks=nchunks, Ls=nchunks * CHUNK_STEPS)


def position(p: int, J: int) -> dict:
    """Where pixel-order position p of a J-position spectrum sits in the sweep."""
    L = decompose(J)["L"]
    g, t = divmod(p, L)
    c, tt = divmod(t, CHUNK_STEPS)
    return dict(g=g, t=t, c=c, tt=tt, phase=c % UNROLL, padded_index=p + 6)


def slot_triples(J: int) -> set:
    """Every (segment, chunk step, phase) that holds a pixel of a J-position spectrum."""
    return {(d["g"], d["tt"], d["phase"]) for d in (position(p, J) for p in range(J))}


def prologue_indices(J: int, g: int) -> range:
    L = decompose(J)["L"]
    return range(g * L, g * L + 6)


def kernel_positions(n: int, m: int, mode: str) -> int:
    """prep_kernel's J: unmasked in-range pixels (reference mode) or in-range pixels (unmasked mode)."""
    return 0 if n == 0 or m == 0 else (n if mode == "reference" else m)


def count_pixels(spec: dict) -> tuple:
    """(n, m) of process_qsos.m:104-111: unmasked in-range and in-range pixel counts."""
    rest = spec["wavelengths"] / (1 + spec["z_qso"])
    inr = (rest >= P.MIN_LAMBDA) & (rest <= P.MAX_LAMBDA)
    return int(np.count_nonzero(inr & ~np.asarray(spec["pixel_mask"], bool))), int(np.count_nonzero(inr))


# ------------------------------------------------------------------------------------- helpers
def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)
    return x


@lru_cache(maxsize=None)
def model(k: int) -> dict:
    return _freeze(syn.make_model(k=k, seed=500 + k))


def short_spectrum(k: int, q: int, J: int, mask_fraction: float = 0.0, z_qso: float = Z_QSO) -> dict:
    """J in-range pixels at the red end of the modelled range and one out-of-range pixel (no DLA is
    injected: the generator's z_DLA range is empty on a spectrum this short)."""
    return syn.make_spectrum(model(k), q, z_qso=z_qso, n_target=J, mask_fraction=mask_fraction,
                             dla_fraction=0.0)


def oracle(spec: dict, k: int, samples: dict, num_lines: int = 3, mode: str = "reference") -> dict:
    return O.process_spectrum(spec["wavelengths"], spec["flux"], spec["noise_variance"], spec["pixel_mask"],
                              spec["z_qso"], model(k), samples["offset_samples"], samples["nhi_samples"],
                              num_lines=num_lines, absorption_mode=mode)


def stack(refs: list) -> dict:
    """Per-spectrum oracle results as the engine's arrays."""
    return _freeze(dict(
        sample_log_likelihoods_dla=np.stack([r["sample_log_likelihoods_dla"] for r in refs]),
        log_likelihoods_no_dla=np.array([r["log_likelihood_no_dla"] for r in refs]),
        log_likelihoods_dla=np.array([r["log_likelihood_dla"] for r in refs]),
        num_pixels=np.array([r["n"] for r in refs]), m=np.array([r["m"] for r in refs])))


# -------------------------------------------------------------------------------------- case A
A_PIXELS = tuple(range(1, 101))
A_PIXELS_I8 = A_PIXELS + (127, 128, 129, 192, 193, 257)   # convert_i8_kernel: ceil(L / 16) = 2 2 3 3 4 5
A_SAMPLES = 65


def case_a_spectra(k: int, pixels=A_PIXELS) -> list:
    return [short_spectrum(k, J, J) for J in pixels]


@lru_cache(maxsize=None)
def case_a_oracle(k: int) -> dict:
    samples = syn.make_samples(A_SAMPLES)
    return stack([oracle(s, k, samples) for s in case_a_spectra(k)])


# -------------------------------------------------------------------------------------- case B
B_RANKS = (4, 8, 10, 11, 12, 16, 20, 24)      # 11: the zero-padded entry into rank 12
B_LINES = (3, 2)
B_MODES = ("reference", "unmasked")
B_PIXELS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 80, 81, 97)
B_SAMPLES = 40


def case_b_spectra(k: int) -> list:
    return [short_spectrum(k, 1000 + J, J, mask_fraction=0.1 if J >= 5 else 0.0) for J in B_PIXELS]


@lru_cache(maxsize=None)
def case_b_oracle(k: int, num_lines: int, mode: str) -> dict:
    samples = syn.make_samples(B_SAMPLES)
    return stack([oracle(s, k, samples, num_lines, mode) for s in case_b_spectra(k)])


# -------------------------------------------------------------------------------------- case C
C_PIXELS = (22, 85)     # L = 6 (Ls = 8: two neutral rows per segment); L = 22 (6 chunks: 5 phases + wrap)
C_DX = (0.0, 4.5, -8.9, 9.1, -20.0, 31.9, -32.1, 40.0)
C_NHI = (1e20, 10.0 ** 22.5)
C_RANK = 20
C_OVER = O.C_CGS / (O.SIGMA * np.sqrt(2.0))      # x = C_OVER (lam / (lam_j (1 + z)) - 1)


def doppler_x(padded: np.ndarray, z: np.ndarray) -> np.ndarray:
    """x[s, i, j]: distance of padded wavelength i from line j of an absorber at z[s], Doppler units."""
    lam_j = O.TRANSITION_WAVELENGTHS[:LINES] * 1e8
    return C_OVER * (padded[None, :, None] / (lam_j[None, None, :] * (1.0 + z[:, None, None])) - 1.0)


def centred_samples(prep: dict, dxs=C_DX) -> dict:
    """Offsets putting line j's centre at padded wavelength i shifted by dx Doppler units, for every
    padded index, line, dx and column density -- built as test_gpu_line_centres._centred_samples does,
    but not restricted to offsets in [0, 1]: on a spectrum this short the Ly-beta and Ly-gamma centres
    need offsets far outside it.  The engine takes any finite offset, and the oracle applies the same
    affine z_DLA = zmin + (zmax - zmin) offset."""
    padded, zmin, zmax = prep["padded"], prep["zmin"], prep["zmax"]
    offs, nhis, meta = [], [], []
    for j in range(LINES):
        lam_j = O.TRANSITION_WAVELENGTHS[j] * 1e8
        for i in range(padded.size):
            for dx in dxs:
                z = padded[i] / (lam_j * (1.0 + dx / C_OVER)) - 1.0
                off = (z - zmin) / (zmax - zmin)
                for N in C_NHI:
                    offs.append(off)
                    nhis.append(N)
                    meta.append((j, i, dx))
    nhis = np.array(nhis)
    return dict(offset_samples=np.array(offs), nhi_samples=nhis, log_nhi_samples=np.log10(nhis),
                line=np.array([m[0] for m in meta]), index=np.array([m[1] for m in meta]),
                dx=np.array([m[2] for m in meta]))


@lru_cache(maxsize=None)
def case_c(J: int, dxs=C_DX) -> dict:
    """The spectrum, its samples, x[s, i, j] as the kernels see it and the oracle's results."""
    spec = short_spectrum(C_RANK, 2000 + J, J)
    prep = O.prepare_spectrum(spec["wavelengths"], spec["flux"], spec["noise_variance"], spec["pixel_mask"],
                              spec["z_qso"], model(C_RANK))
    samples = centred_samples(prep, dxs)
    z = prep["zmin"] + (prep["zmax"] - prep["zmin"]) * samples["offset_samples"]
    return _freeze(dict(spec=spec, samples=samples, padded=prep["padded"], x=doppler_x(prep["padded"], z), J=J))


@lru_cache(maxsize=None)
def case_c_oracle(J: int) -> dict:
    c = case_c(J)
    return stack([oracle(c["spec"], C_RANK, c["samples"])])


def centre_slot(J: int, index: int):
    """(g, tt, phase) of the slot that evaluates padded index `index`, None for the first six (they
    are only ever evaluated in segment 0's prologue)."""
    if index < 6:
        return None
    d = position(index - 6, J)
    return d["g"], d["tt"], d["phase"]


# -------------------------------------------------------------------------------------- case D
D_PIXELS = (37, 64)
D_RANK = 20
D_SAMPLES = 40
D_PATTERNS = ("first_pixel", "last_pixel", "first_segment", "last_segment", "all_but_one", "alternate",
              "all_masked", "blue_prepended")
D_Z_BLUE = 3.0     # 911.75 (1 + z) = 3647 A: the blue edge of the modelled range inside the array


def blue_edge_spectrum(k: int, q: int, J: int, extra: int = 5, z_qso: float = D_Z_BLUE) -> dict:
    """`extra` out-of-range pixels, then J in-range ones from the blue edge of the modelled range up:
    the in-range index of a pixel is its array index minus `extra`."""
    rng = np.random.default_rng(7000 + q)
    mdl = model(k)
    bottom = np.log10(P.MIN_LAMBDA * (1 + z_qso))
    lam = 10.0 ** (bottom + P.PIXEL_SPACING * (np.arange(-extra, J) + 0.5))
    rest = lam / (1 + z_qso)
    mu = np.interp(rest, mdl["rest_wavelengths"], mdl["mu"])
    noise = rng.uniform(0.01, 0.09, lam.size)
    flux = mu + 0.2 * rng.standard_normal(lam.size) + np.sqrt(noise) * rng.standard_normal(lam.size)
    return dict(wavelengths=lam, flux=flux, noise_variance=noise, pixel_mask=np.zeros(lam.size, dtype=bool),
                z_qso=float(z_qso))


def case_d_expected(J: int, pattern: str) -> tuple:
    """The (n, m) a pattern is named for."""
    L = decompose(J)["L"]
    n = dict(first_pixel=J - 1, last_pixel=J - 1, first_segment=J - L, last_segment=3 * L, all_but_one=1,
             alternate=(J + 1) // 2, all_masked=0, blue_prepended=J)[pattern]
    return n, J


def case_d_spectrum(J: int, pattern: str) -> dict:
    """Masks placed on the segment edges of the unmasked-mode decomposition (L = ceil(m / 4))."""
    if pattern == "blue_prepended":
        return blue_edge_spectrum(D_RANK, J, J)
    spec = short_spectrum(D_RANK, 3000 + J, J)
    L = decompose(J)["L"]
    mask = np.zeros(J + 1, dtype=bool)      # pixel J is the out-of-range one
    if pattern == "first_pixel":
        mask[0] = True
    elif pattern == "last_pixel":
        mask[J - 1] = True
    elif pattern == "first_segment":
        mask[:L] = True
    elif pattern == "last_segment":
        mask[3 * L:J] = True
    elif pattern == "all_but_one":
        mask[:J] = True
        mask[J // 2] = False
    elif pattern == "alternate":
        mask[1:J:2] = True
    elif pattern == "all_masked":
        mask[:J] = True
    else:
        raise ValueError(pattern)
    spec["pixel_mask"] = mask
    return spec


def case_d_spectra(J: int) -> list:
    return [case_d_spectrum(J, p) for p in D_PATTERNS]


@lru_cache(maxsize=None)
def case_d_oracle(J: int, mode: str) -> dict:
    """Oracle rows of the usable patterns, in D_PATTERNS order without "all_masked"."""
    samples = syn.make_samples(D_SAMPLES)
    return stack([oracle(s, D_RANK, samples, mode=mode)
                  for s, p in zip(case_d_spectra(J), D_PATTERNS) if p != "all_masked"])


# -------------------------------------------------------------------------------------- case E
E_SAMPLES = (15, 16, 17, 63, 64, 65, 127, 128, 129)
E_SPECTRA = (1, 3, 8, 9)
E_PIXELS = 40
E_RANK = 20
E_UNUSABLE = 4          # the middle spectrum of the 9-spectrum batch


def case_e_spectra(Q: int) -> list:
    spectra = [short_spectrum(E_RANK, 4000 + q, E_PIXELS) for q in range(Q)]
    if Q == 9:
        spectra[E_UNUSABLE] = dict(spectra[E_UNUSABLE], z_qso=9.5)     # nothing in range
    return spectra


@lru_cache(maxsize=None)
def case_e_oracle() -> dict:
    """All 9 spectra (usable, i.e. before the z_qso = 9.5 replacement) at S = 129; make_samples(S) is a
    prefix of make_samples(129), so columns :S serve every smaller S."""
    samples = syn.make_samples(max(E_SAMPLES))
    spectra = [short_spectrum(E_RANK, 4000 + q, E_PIXELS) for q in range(max(E_SPECTRA))]
    return stack([oracle(s, E_RANK, samples) for s in spectra])

"""Plain extended-precision (x87 80-bit ``np.longdouble``) references for the stand-alone entry points
and the evidence reduction, and the one input generator their tests share.  Host only.

* ``log_mvnpdf_ld``    log_mvnpdf_low_rank.m:5-33 with every operation in long double;
* ``log_mean_exp_ld``  process_qsos.m:202-209, max + log(sum exp(row - max) / S), in long double;
* ``mvn_case``         the regime of tests/golden/make_golden.py:golden_mvn, seeded from [seed, n, k];
* ``MVN_SHAPES``       every rank 1..64 at the edges of the kernel's 64-row chunk;
* the voigt shape list (tile edges of the 256-output tile with its 6-pixel halo).

tests/test_extended_reference.py pins these against scipy and both oracles before they judge a
kernel (tests/test_gpu_standalone_edges.py)."""
import numpy as np

LD = np.longdouble


def require_extended_precision():
    """The references are only references with a 64-bit significand: fail loudly without one."""
    assert np.finfo(LD).nmant >= 63, (
        f"np.longdouble has a {np.finfo(LD).nmant}-bit mantissa here: the extended-precision references "
        "need the x87 80-bit format")


def _cholesky_lower_ld(B):
    """L with L L' = B (long double; numpy.linalg has no long-double path)."""
    k = B.shape[0]
    Lo = np.zeros((k, k), dtype=LD)
    for j in range(k):
        v = B[j, j] - Lo[j, :j] @ Lo[j, :j]
        assert v > 0, f"B is not positive definite at pivot {j}"
        Lo[j, j] = np.sqrt(v)
        if j + 1 < k:
            Lo[j + 1:, j] = (B[j + 1:, j] - Lo[j + 1:, :j] @ Lo[j, :j]) / Lo[j, j]
    return Lo


def log_mvnpdf_ld(y, mu, M, d):
    """log N(y; mu, M M' + diag d) by the formula of log_mvnpdf_low_rank.m:5-33:
    B = I + M' D^-1 M = L L', L t = M' D^-1 r, and
    -0.5 (r' D^-1 r - t't + sum log d + 2 sum log L_pp + n log 2 pi)."""
    require_extended_precision()
    M = np.asarray(M, dtype=np.float64)
    if M.ndim == 1:
        M = M[:, None]
    M = M.astype(LD)
    r = np.asarray(y, dtype=np.float64).astype(LD) - np.asarray(mu, dtype=np.float64).astype(LD)
    d = np.asarray(d, dtype=np.float64).astype(LD)
    n, k = M.shape
    d_inv = LD(1) / d
    DM = d_inv[:, None] * M
    B = M.T @ DM
    B[np.diag_indices(k)] += LD(1)
    Lo = _cholesky_lower_ld(B)
    u = DM.T @ r
    t = np.zeros(k, dtype=LD)
    for p in range(k):                                  # forward substitution L t = u
        t[p] = (u[p] - Lo[p, :p] @ t[:p]) / Lo[p, p]
    log_2pi = np.log(LD(8) * np.arctan(LD(1)))
    quad = r @ (d_inv * r) - t @ t
    log_det = np.sum(np.log(d)) + LD(2) * np.sum(np.log(np.diag(Lo)))
    return LD(-0.5) * (quad + log_det + LD(n) * log_2pi)


def log_mean_exp_ld(row):
    """max + log(sum exp(row - max) / S) in long double (process_qsos.m:202-209)."""
    require_extended_precision()
    row = np.asarray(row, dtype=np.float64).astype(LD)
    mx = np.max(row)
    return mx + np.log(np.sum(np.exp(row - mx)) / LD(row.size))


# ------------------------------------------------------------------------------ log_mvnpdf inputs
def mvn_case(n, k, seed=0):
    """(y, mu, M, d) in the regime of golden_mvn (B well conditioned).  Column c of M is scaled by
    1 + c / 8, so no two Gram entries are alike and a swapped (row, column) cannot cancel."""
    rng = np.random.default_rng([seed, n, k])
    M = 0.05 * rng.standard_normal((n, k)) * (1 + np.arange(k) / 8)
    mu = 1 + 0.1 * rng.standard_normal(n)
    d = rng.uniform(0.01, 0.2, n)
    y = mu + M @ rng.standard_normal(k) + np.sqrt(d) * rng.standard_normal(n)
    return y, mu, M, d


MVN_NS = (1, 2, 63, 64, 65, 67, 128, 129, 257)
MVN_SHAPES = [(n, k) for k in range(1, 65) for n in MVN_NS]

# power-of-two scaling (y, mu, M, d) -> (s y, s mu, s M, s^2 d), s = 2^e: exact in binary floating
# point, and log p(scaled) = log p(base) - n e ln 2
SCALE_SHAPES = ((65, 22), (257, 64), (3, 64))
SCALE_EXPONENTS = (-400, 400)


def mvn_scaled(case, e):
    y, mu, M, d = case
    return np.ldexp(y, e), np.ldexp(mu, e), np.ldexp(M, e), np.ldexp(d, 2 * e)


# ----------------------------------------------------------------------------------- voigt inputs
VOIGT_N_PADDED = (7, 8, 9, 261, 262, 263, 518, 519, 520)    # n_out = 1, 2, 3, 255-257, 512-514
VOIGT_NUM_LINES = (1, 2, 3, 4, 16, 30, 31)
LYA = 1215.6701


def voigt_grid(n_padded):
    return 10 ** (np.log10(911.75 * 3.56) + 0.003 + 1e-4 * np.arange(n_padded))


def voigt_absorbers(lam):
    """(z, N) at the blue end, the middle and the red end of the grid."""
    z_min, z_max = lam.min() / LYA - 1, lam.max() / LYA - 1
    return ((z_min, 1e20), (0.5 * (z_min + z_max), 10 ** 21.3), (z_max, 1e23))

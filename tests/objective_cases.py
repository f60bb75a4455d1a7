"""Inputs that pin the training objective (csrc/objective.hip) at every rank bucket, tile and sum edge,
with the place each input takes in the kernels' partition arithmetic, and a dense long-double reference.

One evaluation is, per launch of ``batch`` spectra: a pixel kernel (one block per spectrum), the Gram GEMM
(32-spectrum x 64-entry tiles; four waves take every fourth 16-pixel super-step of the ``ldw`` = P rounded
up to 32 operand row), ``objective_spectrum_kernel<KB>`` (KB = the ``obj_kb`` bucket of the rank; up to
KB = 32 the per-pixel sums run unguarded over zero-padded copies of B^-1 and C y, KB = 64 runs 16-pixel
tiles on the matrix cores), the dM GEMM (``objective_accum_kernel``: 8 spectrum chunks, each walked in steps
of 4 spectra by 4 waves through a two-stage software pipeline) and the sums of d log omega and the scalars
(``objective_chunk_sum_kernel``: 64 spectrum chunks, a 16-deep unrolled body and a scalar tail).
``decompose`` restates that arithmetic; the constants it uses are compared with the source by
tests/test_objective_cases.py (``source_constants``).

Cases (tests/test_objective_cases.py checks on the CPU that they land where they claim;
tests/test_gpu_objective_edges.py runs them on the device):

  A  every rank bucket from both sides of every edge, k = 1 and 64; P = 77, Q = 11; the forest objective
     on one rank per bucket
  B  pixel counts around 4, 16, 32, 64, 128 and 256 (P < k included) on the VALU (k = 20) and the
     matrix-core (k = 40) path
  C  spectrum counts 0 .. 1031 in one launch (every pipeline and sum-loop trip count), then 70 spectra in
     launches of 1, 5, 32 and 33
  D  the documented limits: P = 4096 and k = 64, alone and together
  E  the API branches (device-resident data, g = NULL, the argument errors, the non-positive pivot)

The reference (``dense_spectrum`` / ``dense_objective``) is the negative log likelihood and its gradient
from the dense covariance K = M M' + diag(d) in ``np.longdouble``: a hand-written Cholesky for log det K and
K^-1, no Woodbury identity, the per-pixel pow / exp / log in long double as well.  It is used up to
P = DENSE_MAX_PIXELS; above that the double oracle (oracle.gpdla_oracle / forest_training_oracle) stands in,
which the CPU test pins to the dense reference on every case that uses the latter.  References are computed
once per process and handed out read-only.
"""
from __future__ import annotations

import re
from collections import namedtuple
from functools import lru_cache
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parents[1] / "gp_dla_detection_amd" / "csrc" / "objective.hip"

# ------------------------------------------------------------------------------------ the table
MAX_K = 64                       # kObjMaxK
MAX_PIXELS = 4096                # kObjMaxPixels
KB_LADDER = (8, 16, 20, 24, 32, 64)   # obj_kb
VALU_MAX_KB = 32                 # above it pass 6 runs on the matrix cores and Bp / sp do not exist
SCALARS = 8                      # kObjScalars
ROW_PAD = 32                     # obj_ldw: operand rows are P rounded up to this (= the dM GEMM's pixel tile)
ENTRY_TILE = 64                  # entries per GEMM tile; nxp and g's tile are multiples of it
SPECTRUM_TILE = 32               # spectra per Gram tile
PIXEL_STEP = 16                  # pixels per Gram super-step, and per matrix-core tile of pass 6
GRAM_WAVES = 4
MT_ROW_PAD = 4                   # MT has 4 ceil(P / 4) rows
ACC_CHUNKS = 8                   # spectrum chunks of objective_accum_kernel
ACC_STEP = 4                     # spectra per K step
ACC_WAVES = 4
ACC_STRIDE = 8                   # K steps per trip of a wave's pipelined loop (two stages of ACC_WAVES)
SUM_CHUNKS = 64                  # kSumChunks
SUM_DEPTH = 16                   # kD, the unrolled body of objective_chunk_sum_kernel
LDS_OPT_IN = 65536               # dynamic LDS above this is opted into per kernel
WORKSPACE_SHIFT = 29             # spectra per launch <= 2^29 / per_q doubles
DENSE_MAX_PIXELS = 128

C_0, TAU_0, BETA = 0.1, 0.0023, 3.65
TAU_0_MU, TAU_0_SIGMA, BETA_MU, BETA_SIGMA = 0.0023, 0.0007, 3.65, 0.21     # objective.m:59-71


def source_constants() -> dict:
    """The same constants read from objective.hip."""
    s = SRC.read_text()

    def one(pattern):
        m = re.findall(pattern, s)
        assert len(set(m)) == 1, (pattern, m)
        return m[0]

    ladder = one(r"constexpr int obj_kb\(int k\) \{\s*return ([^;]+);")
    steps = re.findall(r"k <= (\d+) \? (\d+)", ladder)
    assert all(a == b for a, b in steps), ladder
    nxp = one(r"obj_nxp\(int k\) \{ return \(k \* \(k \+ 1\) / 2 \+ (\d+)\) / (\d+) \* (\d+); \}")
    ldw = one(r"obj_ldw\(int64_t P\) \{ return \(int\)\(\(P \+ (\d+)\) / (\d+) \* (\d+)\); \}")
    acc = one(r"s0 = a\.nq \* chunk / (\d+), s1 = a\.nq \* \(chunk \+ 1\) / (\d+);")
    mt = one(r"mt_rows = (\d+) \* \(\(P \+ (\d+)\) / (\d+)\);")
    assert "(2 * P + 2 * k * k + 4 * k + 8 + (kb <= 32 ? kb * kb + kb : 0)) * sizeof(double)" in s
    assert "per_q = 2 * ldw + 2 * nep + 5 * num_pixels + kObjScalars;" in s
    assert "const int n16p = (P + 15) / 16;" in s and "for (int pt = wave; pt < n16p; pt += 4)" in s
    assert "for (int ss = wave; ss < a.nss; ss += 4)" in s
    return dict(
        MAX_K=int(one(r"constexpr int kObjMaxK = (\d+);")),
        MAX_PIXELS=int(one(r"constexpr int kObjMaxPixels = (\d+);")),
        KB_LADDER=tuple(int(a) for a, _ in steps) + (int(re.search(r": (\d+)$", ladder).group(1)),),
        VALU_MAX_KB=int(one(r"if constexpr \(KB <= (\d+)\)")),
        VALU_MAX_KB_LDS=int(one(r"\(kb <= (\d+) \? kb \* kb \+ kb : 0\)")),
        SCALARS=int(one(r"constexpr int kObjScalars = (\d+);")),
        ROW_PAD=tuple(int(v) for v in ldw),
        ENTRY_TILE=tuple(int(v) for v in nxp) + (int(one(r"obj_nep\(int k\) \{ return obj_nxp\(k\) \+ (\d+); \}")),),
        SPECTRUM_TILE=int(one(r"const int64_t s0 = (\d+) \* \(int64_t\)st;")),
        PIXEL_STEP=int(one(r"gm\.nss = ldw / (\d+);")),
        MT_ROW_PAD=tuple(int(v) for v in mt),
        ACC_CHUNKS=tuple(int(v) for v in acc) + (int(one(r"const int chunk = blockIdx\.x & (\d+),")) + 1,),
        ACC_STEP=tuple(int(v) for v in one(r"nks = \(s1 - s0 \+ (\d+)\) / (\d+);")),
        ACC_STRIDE=int(one(r"for \(int64_t ks = wave; ks < nks; ks \+= (\d+)\)")),
        ACC_HALF=tuple(int(v) for v in one(r"load\(ks \+ (\d+), A1, B1\);\s*mma\(A0, B0\);\s*if \(ks \+ (\d+) < nks\) \{"
                                           r"\s*load\(ks \+ \d+, A0, B0\);\s*mma\(A1, B1\);")),
        SUM_CHUNKS=int(one(r"constexpr int kSumChunks = (\d+);")),
        SUM_DEPTH=int(one(r"constexpr int kD = (\d+);")),
        LDS_OPT_IN=int(one(r"if \(shm > (\d+)\)")),
        WORKSPACE_SHIFT=int(one(r"\(1LL << (\d+)\) / per_q")),
    )


TABLE_AS_SOURCE = dict(
    MAX_K=MAX_K, MAX_PIXELS=MAX_PIXELS, KB_LADDER=KB_LADDER, VALU_MAX_KB=VALU_MAX_KB, VALU_MAX_KB_LDS=VALU_MAX_KB,
    SCALARS=SCALARS, ROW_PAD=(ROW_PAD - 1, ROW_PAD, ROW_PAD), ENTRY_TILE=(ENTRY_TILE - 1,) + (ENTRY_TILE,) * 3,
    SPECTRUM_TILE=SPECTRUM_TILE, PIXEL_STEP=PIXEL_STEP, MT_ROW_PAD=(MT_ROW_PAD, MT_ROW_PAD - 1, MT_ROW_PAD),
    ACC_CHUNKS=(ACC_CHUNKS,) * 3, ACC_STEP=(ACC_STEP - 1, ACC_STEP), ACC_STRIDE=ACC_STRIDE,
    ACC_HALF=(ACC_WAVES, ACC_WAVES), SUM_CHUNKS=SUM_CHUNKS, SUM_DEPTH=SUM_DEPTH, LDS_OPT_IN=LDS_OPT_IN,
    WORKSPACE_SHIFT=WORKSPACE_SHIFT)


# ------------------------------------------------------------------------------- decomposition
def obj_kb(k: int) -> int:
    return next(kb for kb in KB_LADDER if k <= kb)


def _split(n: int, chunks: int) -> list:
    return [n * (c + 1) // chunks - n * c // chunks for c in range(chunks)]


def _wave_pipeline(nks: int, wave: int) -> dict:
    """One wave's pipelined loop over a chunk of nks K steps: its trips, and how many ran the second half."""
    ks = range(wave, nks, ACC_STRIDE)
    return dict(trips=len(ks), second_halves=sum(1 for s in ks if s + ACC_WAVES < nks))


def decompose(Q: int, P: int, k: int, batch: int | None = None) -> dict:
    """Where a Q-spectrum, P-pixel, rank-k evaluation lands in objective.hip's partition arithmetic
    (``batch``: GPDLA_OBJECTIVE_BATCH)."""
    assert 1 <= k <= MAX_K and 1 <= P <= MAX_PIXELS and Q >= 0
    kb = obj_kb(k)
    nxp = (k * (k + 1) // 2 + ENTRY_TILE - 1) // ENTRY_TILE * ENTRY_TILE
    nep = nxp + ENTRY_TILE
    ldw = (P + ROW_PAD - 1) // ROW_PAD * ROW_PAD
    nss = ldw // PIXEL_STEP
    lds = 8 * (2 * P + 2 * k * k + 4 * k + 8 + (kb * kb + kb if kb <= VALU_MAX_KB else 0))
    per_q = 2 * ldw + 2 * nep + 5 * P + SCALARS
    b = max(1, min(max(Q, 1), (1 << WORKSPACE_SHIFT) // per_q))
    if batch:
        b = min(b, int(batch))
    launches, prev = [], 0
    for q0 in range(0, Q, b):
        nq = min(b, Q - q0)
        rows = (nq + SPECTRUM_TILE - 1) // SPECTRUM_TILE * SPECTRUM_TILE
        acc = _split(nq, ACC_CHUNKS)
        sums = _split(nq, SUM_CHUNKS)
        launches.append(dict(
            q0=q0, nq=nq, rows=rows, padding_rows=rows - nq,
            stale_rows=max(0, min(prev, rows) - nq),      # padding rows that hold the previous launch's operands
            acc_chunks=acc, acc_nks=[(n + ACC_STEP - 1) // ACC_STEP for n in acc],
            acc_waves=[[_wave_pipeline((n + ACC_STEP - 1) // ACC_STEP, w) for w in range(ACC_WAVES)] for n in acc],
            sum_chunks=sums, sum_body=[n // SUM_DEPTH for n in sums], sum_tail=[n % SUM_DEPTH for n in sums]))
        prev = nq
    return dict(
        Q=Q, P=P, k=k, kb=kb, valu=kb <= VALU_MAX_KB, pad_ranks=kb - k, nxp=nxp, nep=nep, ldw=ldw, nss=nss,
        gram_steps=[len(range(w, nss, GRAM_WAVES)) for w in range(GRAM_WAVES)],
        mfma_tiles=[len(range(w, (P + PIXEL_STEP - 1) // PIXEL_STEP, GRAM_WAVES)) for w in range(GRAM_WAVES)],
        mfma_tail_pixels=P % PIXEL_STEP, mt_rows=MT_ROW_PAD * ((P + MT_ROW_PAD - 1) // MT_ROW_PAD),
        kp=4 * ((kb + 4) // 4), lds_bytes=lds, lds_opt_in=lds > LDS_OPT_IN, batch=b, launches=launches)


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


def blocks(g, P: int, k: int) -> dict:
    """The gradient's blocks: dM, d log omega, and the three scalars."""
    g = np.asarray(g)
    return dict(dM=g[:P * k], dlog_omega=g[P * k:P * (k + 1)], scalars=g[P * (k + 1):])


def _line_tables():
    import sub_dla_forest_oracle as SO
    return SO.LINE_WAVELENGTHS, SO.LINE_STRENGTHS


# -------------------------------------------------------------------------------------- inputs
def _row(seed: int, P: int, k: int, q: int) -> tuple:
    """Spectrum q of the (seed, P, k) stream: the same row whatever Q is."""
    rng = np.random.default_rng([seed, P, k, 1, q])
    y = 0.3 * rng.standard_normal(P)
    lya = rng.uniform(2.5, 4.5, P)
    nv = rng.uniform(0.01, 0.1, P)
    hole = rng.uniform(size=P) < 0.2
    z_qso = rng.uniform(3.0, 4.0) - 1.0           # 1 + z_QSO inside the range of 1 + z_Lya
    return y, lya, nv, hole, z_qso


def _off_the_edges(lya, z_qso):
    """Move any pixel within 1e-6 (relative) of a line's edge lambda_i (1 + z_QSO) 1e-5 away from it."""
    lam_i, _ = _line_tables()
    edges = lam_i * (1 + z_qso) / lam_i[0]
    for _ in range(4):
        gap = np.abs(lya[:, None] - edges[None, :]) / edges[None, :]
        near = gap.min(axis=1) < 1e-6
        if not near.any():
            break
        lya = np.where(near, lya * (1 + 1e-5), lya)
    return lya


@lru_cache(maxsize=None)
def problem(Q: int, P: int, k: int, seed: int, forest: bool = False) -> dict:
    """x = [M(:); log omega; log c_0; log tau_0; log beta] and the Q x P training matrices, in the ranges of
    tests/test_training.py.  From Q = 3 on about 20 % of the pixels are NaN, spectrum Q // 2 is NaN
    throughout and spectrum 0 has no NaN.  ``forest``: one z_QSO per spectrum with 1 + z_QSO in 3..4, so
    pixels above it are redward of Lya (no active line) and those far below it have all 31."""
    rng = np.random.default_rng([seed, P, k, 0])
    M = 0.3 * rng.standard_normal((P, k))
    log_omega = 0.5 * np.log(rng.uniform(0.01, 0.05, P))
    x = np.concatenate([M.ravel(order="F"), log_omega, np.log([C_0, TAU_0, BETA])])
    y, lya, nv = (np.empty((Q, P)) for _ in range(3))
    z = np.empty(Q)
    for q in range(Q):
        y[q], lya[q], nv[q], hole, z[q] = _row(seed, P, k, q)
        if forest:
            lya[q] = _off_the_edges(lya[q], z[q])
        if Q >= 3:
            if q == Q // 2:
                y[q] = np.nan
            elif q != 0:
                y[q, hole] = np.nan
    return _freeze(dict(Q=Q, P=P, k=k, x=x, y=y, lya=lya, nv=nv, z_qsos=z if forest else None,
                        all_nan_row=Q // 2 if Q >= 3 else None))


# ------------------------------------------------------------------------- the dense reference
LD = np.longdouble
LOG_2PI_LD = np.log(8 * np.arctan(LD(1)))


def cholesky_ld(K):
    """Lower Cholesky factor of K (long double), column by column."""
    n = K.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        s = K[j, j] - L[j, :j] @ L[j, :j]
        if not s > 0:
            raise np.linalg.LinAlgError("dense reference: covariance not positive definite")
        L[j, j] = np.sqrt(s)
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def lower_inverse_ld(L):
    """L^-1 by forward substitution, row by row."""
    n = L.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        X[i, i] = 1 / L[i, i]
        if i:
            X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
    return X


def series_terms_ld(lya_1pz, z_qso, tau_0, beta, num_lines):
    """(sum_i t_i, sum_i t_i log(1 + z_i)) of forest_training_oracle.series_terms, in long double."""
    lam_i, c_i = _line_tables()
    lam = lya_1pz * LD(lam_i[0])
    tau = np.zeros(lam.shape, dtype=LD)
    tlog = np.zeros(lam.shape, dtype=LD)
    for i in range(num_lines):
        li = LD(lam_i[i])
        zi = (lam - li) / li
        on = zi <= LD(z_qso)
        base = np.where(on, 1 + zi, LD(1))
        t = np.where(on, tau_0 * LD(c_i[i]) * base ** beta, LD(0))
        tau = tau + t
        tlog = tlog + t * np.log(base)
    return tau, tlog


def dense_spectrum(y, lya_1pz, noise_variance, M, omega2, c_0, tau_0, beta, z_qso=None, num_lines=31):
    """spectrum_loss.m's six outputs from the dense n x n covariance, in long double; no NaN in y."""
    y, lya, nv, om2 = (np.asarray(v, dtype=LD) for v in (y, lya_1pz, noise_variance, omega2))
    M = np.asarray(M, dtype=LD)
    c_0, tau_0, beta = LD(c_0), LD(tau_0), LD(beta)
    n, k = M.shape
    if z_qso is None:
        tau = tau_0 * lya ** beta
        tlog = tau * np.log(lya)
    else:
        tau, tlog = series_terms_ld(lya, z_qso, tau_0, beta, num_lines)
    absorb = np.exp(-tau)
    sf = 1 - absorb + c_0
    an = om2 * sf * sf
    d = nv + an
    K = M @ M.T
    K[np.diag_indices(n)] += d
    L = cholesky_ld(K)
    Li = lower_inverse_ld(L)
    Kinv = Li.T @ Li
    a = Kinv @ y
    dk = np.diag(Kinv).copy()
    f = (y @ a + 2 * np.sum(np.log(np.diag(L))) + n * LOG_2PI_LD) / 2
    dM = -(np.outer(a, a @ M) - Kinv @ M)
    dlo = -(an * (a * a - dk))
    out = [f, dM, dlo]
    for da in (c_0 * om2 * sf, om2 * sf * tau * absorb, om2 * sf * absorb * beta * tlog):
        out.append(-(a * da) @ a + dk @ da)
    return tuple(out)


_SPECTRA = {}     # per-spectrum dense results: the cases of one (P, k) stream share their rows


def dense_objective(x, y, lya, nv, z_qsos=None, num_lines=31):
    """objective.m on the dense reference: NaN pixels masked, the spectra summed, the two prior terms added
    to the gradient; (f, g) rounded to double once at the end."""
    Q, P = y.shape
    k = (x.size - 3) // P - 1
    xl = np.asarray(x, dtype=LD)
    M = xl[:P * k].reshape(P, k, order="F")
    om2 = np.exp(2 * xl[P * k:P * (k + 1)])
    c_0, tau_0, beta = np.exp(xl[-3]), np.exp(xl[-2]), np.exp(xl[-1])
    f = LD(0)
    dM = np.zeros((P, k), dtype=LD)
    dlo = np.zeros(P, dtype=LD)
    sc = np.zeros(3, dtype=LD)
    xkey = hash(np.asarray(x).tobytes())
    for q in range(Q):
        ind = ~np.isnan(y[q])
        if not ind.any():
            continue
        z = None if z_qsos is None else float(z_qsos[q])
        key = (xkey, y[q].tobytes(), lya[q].tobytes(), nv[q].tobytes(), z, num_lines if z is not None else 0)
        if key not in _SPECTRA:
            _SPECTRA[key] = dense_spectrum(y[q, ind], lya[q, ind], nv[q, ind], M[ind], om2[ind], c_0, tau_0, beta,
                                           z, num_lines)
        tf, tdM, tdo, tc, tt, tb = _SPECTRA[key]
        f += tf
        dM[ind] += tdM
        dlo[ind] += tdo
        sc += np.array([tc, tt, tb], dtype=LD)
    sc[1] += tau_0 * (tau_0 - LD(TAU_0_MU)) / (LD(TAU_0_SIGMA) * LD(TAU_0_SIGMA))
    sc[2] += beta * (beta - LD(BETA_MU)) / (LD(BETA_SIGMA) * LD(BETA_SIGMA))
    g = np.concatenate([dM.ravel(order="F"), dlo, sc])
    return float(f), g.astype(np.float64)


# --------------------------------------------------------------------------------------- cases
Case = namedtuple("Case", "family Q P k lines batch seed")      # lines = 0: the Lya-only objective


def case_id(c: Case) -> str:
    s = f"{c.family}-Q{c.Q}-P{c.P}-k{c.k}"
    if c.lines:
        s += f"-L{c.lines}"
    if c.batch:
        s += f"-batch{c.batch}"
    return s


A_RANKS = (1, 2, 7, 8, 9, 15, 16, 17, 19, 20, 21, 23, 24, 25, 31, 32, 33, 48, 63, 64)
A_PIXELS, A_SPECTRA = 77, 11
A_FOREST = ((8, 31), (16, 31), (20, 31), (24, 31), (32, 31), (64, 31), (20, 1), (20, 2))   # (k, lines)
A_LOSS_RANKS = (8, 16, 20, 24, 32, 64)       # spectrum_loss: one rank per bucket
CASES_A = tuple(Case("A", A_SPECTRA, A_PIXELS, k, 0, None, 100) for k in A_RANKS) + tuple(
    Case("A", A_SPECTRA, A_PIXELS, k, L, None, 100) for k, L in A_FOREST)

B_PIXELS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
B_RANKS, B_SPECTRA = (20, 40), 5
CASES_B = tuple(Case("B", B_SPECTRA, P, k, 0, None, 200) for k in B_RANKS for P in B_PIXELS)

C_PIXELS, C_RANK = 33, 8
C_SPECTRA = (0, 1, 7, 8, 9, 33, 65, 137, 265, 409, 1031)
C_LAUNCH_SPECTRA, C_BATCHES = 70, (1, 5, 32, 33)
C_FOREST_BATCH = 33
CASES_C = tuple(Case("C", Q, C_PIXELS, C_RANK, 0, None, 300) for Q in C_SPECTRA)
CASES_C_LAUNCHES = tuple(Case("C", C_LAUNCH_SPECTRA, C_PIXELS, C_RANK, 0, b, 300) for b in C_BATCHES) + (
    Case("C", C_LAUNCH_SPECTRA, C_PIXELS, C_RANK, 31, C_FOREST_BATCH, 300),)

D_SHAPES = ((4096, 64), (4096, 32), (4096, 1), (1, 64))
CASES_D = tuple(Case("D", 2, P, k, 0, None, 400) for P, k in D_SHAPES)

ALL_CASES = CASES_A + CASES_B + CASES_C + CASES_C_LAUNCHES + CASES_D


def case_problem(c: Case) -> dict:
    return problem(c.Q, c.P, c.k, c.seed, bool(c.lines))


def case_decompose(c: Case) -> dict:
    return decompose(c.Q, c.P, c.k, c.batch)


def uses_dense(c: Case) -> bool:
    return c.P <= DENSE_MAX_PIXELS


def oracle_objective(c: Case) -> tuple:
    """The double-precision restatement (oracle.gpdla_oracle.objective / forest_training_oracle)."""
    from oracle import gpdla_oracle as O
    p = case_problem(c)
    if c.lines:
        import forest_training_oracle as FO
        return FO.objective_forest(p["x"], p["y"], p["lya"], p["nv"], p["z_qsos"], c.lines)
    return O.objective(p["x"], p["y"], p["lya"], p["nv"])


@lru_cache(maxsize=None)
def _reference(Q, P, k, lines, seed) -> dict:
    c = Case("", Q, P, k, lines, None, seed)
    p = case_problem(c)
    if uses_dense(c):
        f, g = dense_objective(p["x"], p["y"], p["lya"], p["nv"], p["z_qsos"], lines or 31)
        return _freeze(dict(f=f, g=g, source="dense"))
    f, g = oracle_objective(c)
    return _freeze(dict(f=float(f), g=np.asarray(g, dtype=np.float64), source="oracle"))


def reference(c: Case) -> dict:
    """f and g of the case (the launch splitting does not enter), computed once per process, read-only."""
    return _reference(c.Q, c.P, c.k, c.lines, c.seed)


def without_row(p: dict, q: int) -> dict:
    """The problem with spectrum q taken out."""
    keep = np.arange(p["Q"]) != q
    return dict(p, Q=p["Q"] - 1, y=p["y"][keep], lya=p["lya"][keep], nv=p["nv"][keep],
                z_qsos=None if p["z_qsos"] is None else p["z_qsos"][keep])


# ---------------------------------------------------------------------- spectrum_loss (case A)
@lru_cache(maxsize=None)
def loss_problem(k: int, forest: bool = False) -> dict:
    """One spectrum without NaN at P = A_PIXELS: spectrum_loss's own arguments (omega2, not log omega)."""
    p = problem(1, A_PIXELS, k, 150, forest)
    P = A_PIXELS
    return _freeze(dict(y=p["y"][0], lya=p["lya"][0], nv=p["nv"][0], M=p["x"][:P * k].reshape(P, k, order="F"),
                        omega2=np.exp(2 * p["x"][P * k:P * (k + 1)]), z_qso=float(p["z_qsos"][0]) if forest else None))


@lru_cache(maxsize=None)
def loss_reference(k: int, forest: bool = False, num_lines: int = 31) -> tuple:
    p = loss_problem(k, forest)
    out = dense_spectrum(p["y"], p["lya"], p["nv"], p["M"], p["omega2"], C_0, TAU_0, BETA, p["z_qso"], num_lines)
    return _freeze((float(out[0]), out[1].astype(np.float64), out[2].astype(np.float64)) + tuple(float(v) for v in out[3:]))


# ------------------------------------------------------------------------------ case E inputs
E_SHAPE = (9, 33, 8)         # Q, P, k of the API cases
E4_PIXEL = 5


def e4_problem() -> dict:
    """A non-positive first pivot: pixel E4_PIXEL of spectrum 1 carries a negative noise variance.  At
    ``x_bad`` (the problem's x with M[E4_PIXEL, 0] = 10) that pixel's d = nv + omega^2 sf^2 is negative and
    B[0][0] = 1 + sum_i M_i0^2 / d_i < 0; at ``x_good`` (log omega = 1 there, M as drawn) d is positive,
    the covariance is positive definite and the objective is the ordinary one."""
    Q, P, k = E_SHAPE
    p = problem(Q, P, k, 500)
    nv = p["nv"].copy()
    y = p["y"].copy()
    y[1, E4_PIXEL] = 0.1                            # (in use whatever the holes are)
    nv[1, E4_PIXEL] = -0.05
    x_bad, x_good = p["x"].copy(), p["x"].copy()
    x_bad[0 * P + E4_PIXEL] = 10.0
    x_good[P * k + E4_PIXEL] = 1.0
    return _freeze(dict(p, y=y, nv=nv, x_bad=x_bad, x_good=x_good, spectrum=1))


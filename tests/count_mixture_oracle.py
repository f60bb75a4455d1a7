"""Oracles for the count mixture (csrc/count_mixture.hip, catalog.total_column_intervals), numpy and
``math.fsum`` only:

``lattice_chain``   the chain of sparse convolutions with given shifts, every cell the ``fsum`` of its terms
``numpy_chain``     the same chain as the device orders it (per tap, ascending, one multiply and one add per cell),
                    vectorised over the cells: the restatement the measurement script times and the reference
                    fixture is made with
``levels_of``       the lower and upper cells of a lattice and how close its cdf comes to a level
``mixture``         either chain behind the ``mixture=`` hook of ``catalog.total_column_intervals``
``exact_atoms``     every outcome of a small problem with its exact value, and ``lower_quantile`` of them."""
import itertools
import math
from fractions import Fraction

import numpy as np


def _live(stages, upto):
    return 1 + sum(int(np.max(s)) for _, s in stages[:upto])


def lattice_chain(stages, cells: int) -> np.ndarray:
    """``stages``: [(probs, shifts), ...].  next[g] = fsum_i(p_i cur[g - shift_i]) from delta at cell 0."""
    cur = np.zeros(cells)
    cur[0] = 1.0
    for n, (probs, shifts) in enumerate(stages):
        probs, shifts = np.asarray(probs, dtype=np.float64), np.asarray(shifts, dtype=np.int64)
        live = min(cells, _live(stages, n + 1))
        terms = np.zeros((live, probs.size))
        for i, (p, s) in enumerate(zip(probs, shifts)):
            if s < live:
                terms[s:, i] = p * cur[:live - s]
        nxt = np.zeros(cells)
        nxt[:live] = [math.fsum(row) for row in terms]
        cur = nxt
    return cur


def numpy_chain(stages, cells: int) -> np.ndarray:
    cur = np.zeros(cells)
    cur[0] = 1.0
    for n, (probs, shifts) in enumerate(stages):
        live = min(cells, _live(stages, n + 1))
        nxt = np.zeros(cells)
        for p, s in zip(np.asarray(probs, dtype=np.float64), np.asarray(shifts, dtype=np.int64)):
            if s < live:
                nxt[s:live] += p * cur[:live - s]
        cur = nxt
    return cur


def levels_of(pmf, levels):
    """(lower cells, upper cells, mass, the smallest distance of a cdf value from a level): lower = the first
    cell with cdf >= level; upper = the first occupied cell strictly above the first with cdf > level; either the
    last occupied cell where there is none, 0 for a lattice without mass."""
    pmf = np.asarray(pmf, dtype=np.float64)
    cdf = np.cumsum(pmf)
    occupied = np.flatnonzero(pmf > 0)
    end = int(occupied[-1]) if occupied.size else 0
    lower, upper = [], []
    for lam in levels:
        at = np.flatnonzero(cdf >= lam)
        lower.append(int(at[0]) if at.size else end)
        over = np.flatnonzero(cdf > lam)
        nxt = occupied[occupied > over[0]] if over.size else occupied[:0]
        upper.append(int(nxt[0]) if nxt.size else end)
    gap = float(np.abs(cdf[:, None] - np.asarray(levels, dtype=np.float64)[None, :]).min()) if len(levels) else np.inf
    return np.array(lower, dtype=np.int32), np.array(upper, dtype=np.int32), float(cdf[-1]), gap


def split_csr(probs, shifts, tap_offsets, stage_offsets):
    """The CSR arguments of ``engine.count_mixture`` as a list of problems, each a list of (probs, shifts)."""
    return [[(np.asarray(probs)[tap_offsets[s]:tap_offsets[s + 1]], np.asarray(shifts)[tap_offsets[s]:tap_offsets[s + 1]])
             for s in range(stage_offsets[p], stage_offsets[p + 1])] for p in range(len(stage_offsets) - 1)]


def to_csr(problems):
    """The inverse of ``split_csr``: (probs, shifts, tap_offsets, stage_offsets)."""
    stages = [st for prob in problems for st in prob]
    tap_offsets = np.concatenate([[0], np.cumsum([len(p) for p, _ in stages])]).astype(np.int64)
    stage_offsets = np.concatenate([[0], np.cumsum([len(prob) for prob in problems])]).astype(np.int64)
    probs = np.concatenate([np.asarray(p, dtype=np.float64) for p, _ in stages]) if stages else np.zeros(0)
    shifts = np.concatenate([np.asarray(s, dtype=np.int64) for _, s in stages]) if stages else np.zeros(0, dtype=np.int64)
    return probs, shifts, tap_offsets, stage_offsets


def mixture(chain=lattice_chain, gaps=None):
    """A ``mixture=`` hook; ``gaps`` (a list) collects every problem's distance of its cdf from a level."""
    def run(probs, shifts, tap_offsets, stage_offsets, cells, levels):
        got = [levels_of(chain(stages, cells), levels) for stages in split_csr(probs, shifts, tap_offsets, stage_offsets)]
        if gaps is not None:
            gaps.extend(g[3] for g in got)
        return (np.array([g[0] for g in got]).reshape(len(got), -1), np.array([g[1] for g in got]).reshape(len(got), -1),
                np.array([g[2] for g in got]))
    return run


def exact_atoms(stages, values):
    """Every outcome of a small problem: ``stages`` the tap probabilities per stage, ``values`` each tap's exact
    value.  Returns (values ascending, probabilities), the value sums and probability products formed in
    rationals and rounded once."""
    atoms = {}
    taps = [[(Fraction(float(v)), Fraction(float(p))) for p, v in zip(ps, vs)] for ps, vs in zip(stages, values)]
    for combo in itertools.product(*taps):
        v, p = sum(c[0] for c in combo), math.prod(c[1] for c in combo)
        atoms[v] = atoms.get(v, 0) + p
    keys = sorted(atoms)
    return np.array([float(k) for k in keys]), np.array([float(atoms[k]) for k in keys])


def lower_quantile(values, probs, level):
    """(the smallest value whose cumulative probability reaches ``level`` -- the last value if none does -- and
    the distance of the cumulative probabilities from ``level``)."""
    cdf = np.cumsum(probs)
    at = np.flatnonzero(cdf >= level)
    return float(values[at[0]] if at.size else values[-1]), float(np.abs(cdf - level).min())

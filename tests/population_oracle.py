"""Numpy / exact-arithmetic oracles of the population statistics (csrc/population.hip, DESIGN.md section
15): the split of the level-1 masses p_dla pi_j into a Poisson plane and the list of large probabilities,
and the Poisson-binomial pmf, exactly (rational arithmetic) and in double by the kernel's recurrence."""
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).parent))
import posterior_summary_oracle as PO  # noqa: E402

MAX_LARGE = 8


masses = PO.masses   # pi_j exactly as the summaries define it


def split(ll, min_z, max_z, p_dla, offset, log_nhi, z_edges, n_edges, p_thresh_sample=1e-4, p_switch=0.25):
    """One row: (nz x nn Poisson plane summed in sample order, indices / probabilities / flat bins of the
    samples with p >= p_switch inside the grid, by increasing index)."""
    nz, nn = len(z_edges) - 1, len(n_edges) - 1
    p = p_dla * masses(ll)
    iz = PO.bin_index(z_edges, PO.sample_z(min_z, max_z, offset))
    inn = PO.bin_index(n_edges, log_nhi)
    inside = (iz >= 0) & (inn >= 0)
    plane = np.zeros((nz, nn))
    inds, probs, bins = [], [], []
    for j in np.flatnonzero(inside):
        if p[j] >= p_switch:
            inds.append(j); probs.append(p[j]); bins.append(iz[j] * nn + inn[j])
        elif p_thresh_sample < p[j] < p_switch:
            plane[iz[j], inn[j]] += p[j]
    return plane, np.array(inds, dtype=np.int64), np.array(probs), np.array(bins, dtype=np.int64)


def split_rows(ll, min_z, max_z, p_dlas, offset, log_nhi, z_edges, n_edges, **kw):
    """``split`` over rows, in the kernel's output layout (unused slots -1 / NaN / -1)."""
    ll = np.atleast_2d(ll)
    R = ll.shape[0]
    plane = np.zeros((R, len(z_edges) - 1, len(n_edges) - 1))
    inds, bins = np.full((R, MAX_LARGE), -1, dtype=np.int32), np.full((R, MAX_LARGE), -1, dtype=np.int32)
    probs = np.full((R, MAX_LARGE), np.nan)
    for r in range(R):
        plane[r], i, p, b = split(ll[r], min_z[r], max_z[r], p_dlas[r], offset, log_nhi, z_edges, n_edges, **kw)
        assert i.size <= MAX_LARGE
        inds[r, :i.size], probs[r, :i.size], bins[r, :i.size] = i, p, b
    return dict(population_poisson=plane, population_large_inds=inds, population_large_probs=probs,
                population_large_bins=bins)


def exact_pmf(probs):
    """The coefficients of prod_j (1 - p_j + p_j x), exactly: (numerators, E) with coefficient k equal to
    numerators[k] / 2^E.  Doubles are dyadic rationals, so the rational product runs on Python integers over
    a common power-of-two denominator (2^e per factor) instead of reduced ``fractions.Fraction`` terms, which
    compute the same numbers far more slowly."""
    fr = [Fraction(float(p)) for p in probs]
    e = max([f.denominator.bit_length() - 1 for f in fr], default=0)
    one = 1 << e
    coef = [1]
    for f in fr:
        m = int(f * one)
        q = one - m
        new = [0] * (len(coef) + 1)
        for k, c in enumerate(coef):
            new[k] += c * q
            new[k + 1] += c * m
        coef = new
    return coef, e * len(fr)


def exact_fractions(probs):
    """``exact_pmf`` as a list of Fractions (small lists)."""
    coef, E = exact_pmf(probs)
    return [Fraction(c, 1 << E) for c in coef]


def relative_errors(got, exact):
    """|got - exact| / exact per coefficient as floats, in integer arithmetic; coefficients below the smallest
    normal are left out (NaN)."""
    coef, E = exact
    out = np.full(len(coef), np.nan)
    for k, (g, c) in enumerate(zip(got, coef)):
        if (c << 1022) < (1 << E):
            continue
        gn, gd = float(g).as_integer_ratio()
        out[k] = abs((gn << E) - c * gd) / (c * gd)
    return out


def absolute_errors(got, exact):
    """|got - exact| per coefficient as floats."""
    coef, E = exact
    out = np.empty(len(coef))
    for k, (g, c) in enumerate(zip(got, coef)):
        gn, gd = float(g).as_integer_ratio()
        out[k] = abs((gn << E) - c * gd) / (gd << E)
    return out


def recurrence_pmf(probs):
    """The kernel's recurrence in double, one list (a CPU stand-in for the device pmf in the host tests)."""
    pmf = np.ones(1)
    for p in np.asarray(probs, dtype=np.float64).ravel():
        new = np.zeros(pmf.size + 1)
        new[:-1] = pmf * (1.0 - p)
        new[1:] += pmf * p
        pmf = new
    return pmf

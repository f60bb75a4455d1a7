"""numpy / math.fsum restatement of the population statistics over every multi-DLA level (include/gpdla.h
"Population statistics over every multi-DLA level", csrc/level_population.hip), the
reference the kernel tests compare against.  Sums go through math.fsum (exactly rounded), everything else is
plain float64 arithmetic in the order the header states it.  The level posteriors P_d are an input."""
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).parent))
import posterior_summary_oracle as PO  # noqa: E402

MAX_LARGE = 8
MAX_DLAS = 4
PLANES = 5

masses = PO.masses   # pi_{d,j} exactly as the level-1 reductions define it, on level d's row


def chains(base, row, level, S):
    """The absorbers of every sample of ``level`` (1-based) of one row: (S x level sample indices -- slot 0 the
    sample itself, then its base chain -- and the S flags of an unbroken chain).  ``base`` is (levels - 1) x
    rows x S, 0-based, -1 = none; a chain that meets -1 or an index outside [0, S) is void."""
    slots = np.zeros((S, level), dtype=np.int64)
    ok = np.ones(S, dtype=bool)
    slots[:, 0] = np.arange(S)
    for i in range(1, level):
        prev = slots[:, i - 1]
        nxt = np.asarray(base[level - 1 - i][row], dtype=np.int64)[np.where(ok, prev, 0)]
        ok &= (nxt >= 0) & (nxt < S)
        slots[:, i] = np.where(ok, nxt, 0)
    return slots, ok


def slot_bins(slots, ok, min_z, max_z, offset, log_nhi, z_edges, n_edges):
    """S x level flat bins (iz nn + in) of the slots, -1 outside the grid and for void chains."""
    nn = len(n_edges) - 1
    iz = PO.bin_index(z_edges, PO.sample_z(min_z, max_z, np.asarray(offset, dtype=np.float64)[slots]))
    inn = PO.bin_index(n_edges, np.asarray(log_nhi, dtype=np.float64)[slots])
    return np.where((iz >= 0) & (inn >= 0) & ok[:, None], iz * nn + inn, -1)


def level_planes(ll, base, min_z, max_z, offset, log_nhi, nhi, z_edges, n_edges):
    """ll: levels x rows x S.  Returns (rows x levels x 5 x nz x nn planes -- sum pi, pi^2, N pi, N^2 pi,
    N^2 pi^2 over the (sample, slot) pairs of each bin, N the slot's column density -- and the rows x levels x
    nz x nn pair counts)."""
    ll = np.asarray(ll, dtype=np.float64)
    levels, rows, S = ll.shape
    nz, nn = len(z_edges) - 1, len(n_edges) - 1
    nhi = np.asarray(nhi, dtype=np.float64)
    out = np.zeros((rows, levels, PLANES, nz, nn))
    count = np.zeros((rows, levels, nz, nn), dtype=np.int64)
    for r in range(rows):
        for d in range(1, levels + 1):
            pi = masses(ll[d - 1, r])
            slots, ok = chains(base, r, d, S)
            flat = slot_bins(slots, ok, min_z[r], max_z[r], offset, log_nhi, z_edges, n_edges)
            N = nhi[slots]
            p = np.broadcast_to(pi[:, None], N.shape)
            npi = N * p
            terms = (p, p * p, npi, N * npi, npi * npi)
            for b in np.unique(flat[flat >= 0]):
                sel = flat == b                       # row-major: (sample, slot) order
                count[r, d - 1, b // nn, b % nn] = int(sel.sum())
                for k in range(PLANES):
                    out[r, d - 1, k, b // nn, b % nn] = math.fsum(terms[k][sel])
    return out, count


def level_split(ll, base, min_z, max_z, level_posteriors, offset, log_nhi, z_edges, n_edges, p_thresh_sample=1e-4,
                p_switch=0.25):
    """ll: levels x rows x S, level_posteriors: levels x rows.  The kernel's outputs in its layout (unused
    entries -1 / NaN / -1): with p = P_d pi_{d,j}, a sample with p >= p_switch and a slot inside the grid goes
    to the exact list (index, p, one bin per slot); otherwise, with p_thresh_sample < p < p_switch, p is added
    to the Poisson-plane bin of each of its slots."""
    ll = np.asarray(ll, dtype=np.float64)
    levels, rows, S = ll.shape
    P = np.asarray(level_posteriors, dtype=np.float64).reshape(levels, rows)
    nz, nn = len(z_edges) - 1, len(n_edges) - 1
    plane = np.zeros((rows, levels, nz, nn))
    inds = np.full((rows, levels, MAX_LARGE), -1, dtype=np.int32)
    probs = np.full((rows, levels, MAX_LARGE), np.nan)
    bins = np.full((rows, levels, MAX_LARGE, MAX_DLAS), -1, dtype=np.int32)
    for r in range(rows):
        for d in range(1, levels + 1):
            p = P[d - 1, r] * masses(ll[d - 1, r])
            slots, ok = chains(base, r, d, S)
            flat = slot_bins(slots, ok, min_z[r], max_z[r], offset, log_nhi, z_edges, n_edges)
            inside = (flat >= 0).any(axis=1)
            with np.errstate(invalid="ignore"):
                large = inside & (p >= p_switch)
                small = inside & (p > p_thresh_sample) & (p < p_switch)
            js = np.flatnonzero(large)
            assert js.size <= MAX_LARGE
            inds[r, d - 1, :js.size], probs[r, d - 1, :js.size] = js, p[js]
            bins[r, d - 1, :js.size, :d] = flat[js]
            terms = {}
            for j in np.flatnonzero(small):
                for b in flat[j]:
                    if b >= 0:
                        terms.setdefault(int(b), []).append(p[j])
            for b, v in terms.items():
                plane[r, d - 1, b // nn, b % nn] = math.fsum(v)
    return dict(population_level_poisson=plane, population_level_large_inds=inds, population_level_large_probs=probs,
                population_level_large_bins=bins)


def margins(ll, base, min_z, max_z, level_posteriors, offset, log_nhi, z_edges, n_edges, p_thresh_sample=1e-4,
            p_switch=0.25):
    """How far the case is from a decision the device could take the other way: (the smallest relative distance
    of any p = P_d pi_{d,j} > 0 to p_thresh_sample or p_switch, the smallest relative distance of any slot
    coordinate -- z or log N_HI of an unbroken chain with pi > 0 -- to a grid edge).  inf where there is none."""
    ll = np.asarray(ll, dtype=np.float64)
    levels, rows, S = ll.shape
    P = np.asarray(level_posteriors, dtype=np.float64).reshape(levels, rows)
    ez, en = np.asarray(z_edges, dtype=np.float64), np.asarray(n_edges, dtype=np.float64)
    offset, log_nhi = np.asarray(offset, dtype=np.float64), np.asarray(log_nhi, dtype=np.float64)
    dp, dx = math.inf, math.inf
    for r in range(rows):
        for d in range(1, levels + 1):
            pi = masses(ll[d - 1, r])
            p = P[d - 1, r] * pi
            for t in (p_thresh_sample, p_switch):
                v = p[(p > 0) & np.isfinite(p)]
                if v.size and t > 0:
                    dp = min(dp, float(np.abs(v - t).min() / t))
            slots, ok = chains(base, r, d, S)
            use = ok & (pi > 0)
            if use.any():
                z = PO.sample_z(min_z[r], max_z[r], offset[slots[use]]).ravel()
                n = log_nhi[slots[use]].ravel()
                for x, e in ((z, ez), (n, en)):
                    dx = min(dx, float((np.abs(x[:, None] - e[None, :]) / np.abs(e[None, :])).min()))
    return dp, dx


def expected_counts(planes, level_posteriors):
    """sum_d P_d sum_{(j, slot) in b} pi_{d,j}: rows x nz x nn, from ``level_planes``'s sum-pi planes and
    levels x rows posteriors (NaN rows give 0)."""
    planes = np.asarray(planes, dtype=np.float64)
    P = np.nan_to_num(np.asarray(level_posteriors, dtype=np.float64).reshape(planes.shape[1], planes.shape[0]).T)
    return np.einsum("rd,rdzn->rzn", P, planes[:, :, 0])


def one_based(split):
    """The kernel-layout arrays of a level split as ``process_qsos`` saves them (1-based doubles, 0 = none)."""
    out = dict(split)
    for key in ("population_level_large_inds", "population_level_large_bins"):
        out[key] = np.asarray(split[key]).astype(np.float64) + 1.0
    return out

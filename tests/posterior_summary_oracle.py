"""numpy restatement of the posterior summaries (include/gpdla.h "Posterior summaries"), the reference
the kernel tests compare against.  Sums go through math.fsum (exactly rounded), everything else is plain
float64 arithmetic in the order the header states it."""
import math

import numpy as np

PLANES = 5
MAX_DLAS = 4


def map_index(l):
    """Smallest index attaining the maximum over the non-NaN entries (nanmax's first maximum,
    generate_ascii_catalog.m:73), -1 if every entry is NaN."""
    l = np.asarray(l, dtype=np.float64)
    ok = ~np.isnan(l)
    if not ok.any():
        return -1
    return int(np.flatnonzero(ok & (l == l[ok].max()))[0])


def sample_z(min_z, max_z, offsets):
    """z = min_z + (max_z - min_z) * offset, each operation rounded (numpy never fuses)."""
    return np.float64(min_z) + (np.float64(max_z) - np.float64(min_z)) * np.asarray(offsets, dtype=np.float64)


def masses(l):
    """pi_j = w_j / W with w_j = exp(l_j - max), NaN -> 0; all 0 if W is 0 or not finite."""
    l = np.asarray(l, dtype=np.float64)
    j = map_index(l)
    if j < 0:
        return np.zeros(l.size)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp(l - l[j])
    w[np.isnan(l)] = 0.0
    W = math.fsum(w) if not np.isnan(w).any() else float("nan")
    if not (W > 0.0 and W < math.inf):
        return np.zeros(l.size)
    return w / W


def bin_index(edges, x):
    """i with edges[i] <= x < edges[i + 1], -1 outside (and for NaN)."""
    edges = np.asarray(edges, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    i = np.searchsorted(edges, x, side="right") - 1
    with np.errstate(invalid="ignore"):
        inside = (x >= edges[0]) & (x < edges[-1])
    return np.where(inside, i, -1)


def bin_planes(l, min_z, max_z, offsets, log_nhi, nhi, z_edges, log_nhi_edges):
    """(5, nz, nn): sum pi, pi^2, N pi, N^2 pi, N^2 pi^2 per bin, and the per-bin sample counts."""
    nz, nn = len(z_edges) - 1, len(log_nhi_edges) - 1
    pi = masses(l)
    nhi = np.asarray(nhi, dtype=np.float64)
    iz = bin_index(z_edges, sample_z(min_z, max_z, offsets))
    inn = bin_index(log_nhi_edges, log_nhi)
    out = np.zeros((PLANES, nz, nn))
    count = np.zeros((nz, nn), dtype=np.int64)
    npi = nhi * pi
    terms = (pi, pi * pi, npi, nhi * npi, npi * npi)
    flat = np.where((iz >= 0) & (inn >= 0), iz * nn + inn, -1)
    order = np.argsort(flat, kind="stable")                 # each bin's samples, in index order
    bounds = np.searchsorted(flat[order], np.arange(nz * nn + 1))
    for b in range(nz * nn):
        sel = order[bounds[b]:bounds[b + 1]]
        count[b // nn, b % nn] = sel.size
        for p in range(PLANES):
            out[p, b // nn, b % nn] = math.fsum(terms[p][sel])
    return out, count


def map_parameters(ll, base, min_z, max_z, offsets, log_nhi):
    """ll: levels x rows x S, base: (levels - 1) x rows x S (0-based, -1 = none).  Returns
    (inds, map_ll, z, n): levels x rows and levels x rows x MAX_DLAS, unused / broken chains NaN."""
    ll = np.asarray(ll, dtype=np.float64)
    levels, rows, S = ll.shape
    inds = np.full((levels, rows), -1, dtype=np.int32)
    mll = np.full((levels, rows), np.nan)
    z = np.full((levels, rows, MAX_DLAS), np.nan)
    n = np.full((levels, rows, MAX_DLAS), np.nan)
    offsets = np.asarray(offsets, dtype=np.float64)
    log_nhi = np.asarray(log_nhi, dtype=np.float64)
    for d in range(levels):
        for r in range(rows):
            j = map_index(ll[d, r])
            inds[d, r] = j
            if j < 0:
                continue
            mll[d, r] = ll[d, r, j]
            chain = [j]
            for i in range(d):
                b = int(base[d - 1 - i][r][chain[-1]])
                if b < 0 or b >= S:
                    chain = None
                    break
                chain.append(b)
            if chain is None:
                continue
            zs = sample_z(min_z[r], max_z[r], offsets[chain])
            z[d, r, :len(chain)] = zs
            n[d, r, :len(chain)] = log_nhi[chain]
    return inds, mll, z, n

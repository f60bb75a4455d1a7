"""numpy restatement of the posterior intervals (include/gpdla.h "Posterior intervals"), the reference the
kernel tests compare against.  Every cdf and moment goes through math.fsum (exactly rounded, so independent of
the order of the terms); the quantiles come from a stable argsort by value."""
import math

import numpy as np

MAX_DLAS = 4
DEFAULT_LEVELS = (0.025, 0.16, 0.5, 0.84, 0.975)


def sample_z(min_z, max_z, offsets):
    """z = min_z + (max_z - min_z) * offset, each operation rounded (numpy never fuses)."""
    with np.errstate(invalid="ignore"):
        return np.float64(min_z) + (np.float64(max_z) - np.float64(min_z)) * np.asarray(offsets, dtype=np.float64)


def row_masses(l):
    """(pi, m, usable): pi_j = w_j / W with w_j = exp(l_j - m), NaN -> 0, m the maximum over the non-NaN entries;
    usable is False (and pi all 0) if there is no such entry or W is 0 or not finite."""
    l = np.asarray(l, dtype=np.float64)
    ok = ~np.isnan(l)
    if not ok.any():
        return np.zeros(l.size), math.nan, False
    m = float(l[ok].max())
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp(l - m)
    w[~ok] = 0.0
    W = math.fsum(w) if not np.isnan(w).any() else math.nan
    if not (W > 0.0 and W < math.inf):
        return np.zeros(l.size), m, False
    return w / W, m, True


def chains(base, d, r, S):
    """The chains of every sample of row r at level d + 1: c (d + 1) x S (c[0] = the sample, then the base
    indices) and which are valid; base is (levels - 1) x rows x S, 0-based, anything outside [0, S) void."""
    c = np.zeros((d + 1, S), dtype=np.int64)
    c[0] = np.arange(S)
    ok = np.ones(S, dtype=bool)
    for i in range(d):
        b = np.asarray(base[d - 1 - i][r], dtype=np.int64)[c[i]]
        ok &= (b >= 0) & (b < S)
        c[i + 1] = np.where(ok, b, 0)
    return c, ok


def mass_at_or_below(x, pi, v, strict=False):
    """F(v) = sum of pi_j over x_j <= v (strict: x_j < v), exactly rounded."""
    sel = (x < v) if strict else (x <= v)
    return math.fsum(pi[sel])


def quantile(x, pi, level):
    """(x*, T): the smallest value of x whose cumulative mass F(x*) reaches level * T, T = fsum(pi); NaN if T is 0."""
    T = math.fsum(pi)
    if not T > 0.0:
        return math.nan, T
    order = np.argsort(x, kind="stable")
    xs, ps = x[order], pi[order]
    last = np.flatnonzero(np.append(xs[1:] != xs[:-1], True))     # the last entry of each distinct value
    cum = np.cumsum(ps)[last]                                     # approximate F per distinct value
    target = level * T
    tol = 4.0 * x.size * 2.0 ** -52 * T
    lo = int(np.searchsorted(cum, target - tol, side="left"))     # F(lo - 1) < target for sure
    hi = min(int(np.searchsorted(cum, target + tol, side="left")), last.size - 1)   # F(hi) >= target for sure
    while lo < hi:                                                # F is monotone: bisect with the exact sums
        mid = (lo + hi) // 2
        if math.fsum(ps[:last[mid] + 1]) >= target:
            hi = mid
        else:
            lo = mid + 1
    return float(xs[last[lo]]), T


def quantile_dense(x, pi, level):
    """The same by brute force: every value tried as x*, F formed afresh for each."""
    T = math.fsum(pi)
    if not T > 0.0:
        return math.nan
    best = math.nan
    for v in np.unique(x):
        if math.fsum(pi[x <= v]) >= level * T:
            best = float(v)
            break
    return best


def slot_values(c, u, min_z, max_z, offsets, log_nhi):
    return sample_z(min_z, max_z, np.asarray(offsets, dtype=np.float64)[c[u]]), np.asarray(log_nhi, dtype=np.float64)[c[u]]


def z_range_ok(min_z, max_z):
    return bool(np.isfinite(min_z) and np.isfinite(max_z) and max_z >= min_z)


def intervals(ll, base, min_z, max_z, offsets, log_nhi, levels=DEFAULT_LEVELS, lr_delta=2.0, quantiles=True):
    """ll: levels x rows x S, base: (levels - 1) x rows x S.  Returns the arrays of Engine.process_intervals
    (D x rows x D [x 2 | x L], lr_counts D x rows); ``quantiles=False`` leaves the quantiles NaN."""
    ll = np.asarray(ll, dtype=np.float64)
    if ll.ndim == 2:
        ll = ll[None]
    D, R, S = ll.shape
    levels = np.asarray(levels, dtype=np.float64)
    slot = (D, R, D)
    out = dict(z_dla_means=np.full(slot, np.nan), z_dla_sds=np.full(slot, np.nan), log_nhi_means=np.full(slot, np.nan),
               log_nhi_sds=np.full(slot, np.nan), z_dla_lr_ranges=np.full(slot + (2,), np.nan),
               log_nhi_lr_ranges=np.full(slot + (2,), np.nan), z_dla_quantiles=np.full(slot + (levels.size,), np.nan),
               log_nhi_quantiles=np.full(slot + (levels.size,), np.nan), lr_counts=np.zeros((D, R), dtype=np.int32))
    names = ("z_dla", "log_nhi")
    for d in range(D):
        for r in range(R):
            l = ll[d, r]
            pi, m, usable = row_masses(l)
            if not usable:
                continue
            c, ok = chains(base, d, r, S)
            thr = m - np.float64(lr_delta)
            with np.errstate(invalid="ignore"):
                inside = ok & (l > thr)
            out["lr_counts"][d, r] = int(inside.sum())
            T = math.fsum(pi[ok])
            for u in range(d + 1):
                xs = slot_values(c, u, min_z[r], max_z[r], offsets, log_nhi)
                for p, x in enumerate(xs):
                    if p == 0 and not z_range_ok(min_z[r], max_z[r]):
                        continue
                    if inside.any():
                        out[names[p] + "_lr_ranges"][d, r, u] = x[inside].min(), x[inside].max()
                    if T > 0.0:
                        mean = math.fsum(pi[ok] * x[ok]) / T
                        out[names[p] + "_means"][d, r, u] = mean
                        out[names[p] + "_sds"][d, r, u] = math.sqrt(math.fsum(pi[ok] * (x[ok] - mean) ** 2) / T)
                        if quantiles:
                            for k, lv in enumerate(levels):
                                out[names[p] + "_quantiles"][d, r, u, k] = quantile(x[ok], pi[ok], lv)[0]
    return out

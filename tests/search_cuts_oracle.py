"""numpy / math.fsum restatement of the search cuts (include/gpdla.h "Search cuts", csrc/search_cuts.hip,
DESIGN.md section 22): the proximity-zone cut (calc_cddf.py ``lowzcut``) and the noisy-pixel cut
(``filter_noisy_pixels``).  Every expression is plain float64 arithmetic in the order the header states it; the
path's terms are added with math.fsum (exactly rounded) and X is ``catalog.absorption_distance``."""
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).parent))
import level_population_oracle as LO  # noqa: E402
import posterior_summary_oracle as PO  # noqa: E402
from gp_dla_detection_amd.catalog import absorption_distance  # noqa: E402

LYA = 1215.67


def _on(x):
    return x is not None and not (isinstance(x, float) and math.isnan(x))


def spectrum_cut(wavelengths, noise_variance, min_z, max_z, proximity_zone=None, noise_thresh=None):
    """(good flags of the n selected pixels in pixel order, z_upper) of one spectrum."""
    w = np.asarray(wavelengths, dtype=np.float64).ravel()
    v = np.asarray(noise_variance, dtype=np.float64).ravel()
    min_z, max_z = float(min_z), float(max_z)
    with np.errstate(invalid="ignore"):
        sel = (LYA * (1.0 + min_z) < w) & (w < LYA * (1.0 + max_z))
        good = (v[sel] < noise_thresh) if _on(noise_thresh) else np.ones(int(sel.sum()), dtype=bool)
    z_upper = max_z
    if _on(proximity_zone):
        zu = max_z - proximity_zone
        z_upper = min_z if min_z > zu else zu
    return good, z_upper


def bitmap(goods):
    """The CSR bitmap of a list of good-flag vectors, each spectrum's stretch ``words_q`` words long: (offsets
    [Q + 1], uint32 words).  ``goods`` is a list of (flags, words_q)."""
    off = np.zeros(len(goods) + 1, dtype=np.int64)
    words = []
    for q, (g, nw) in enumerate(goods):
        wq = np.zeros(nw, dtype=np.uint32)
        for i in np.flatnonzero(g):
            wq[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
        words.append(wq)
        off[q + 1] = off[q] + nw
    return off, (np.concatenate(words) if words else np.zeros(0, dtype=np.uint32))


def zz(min_z, max_z, n):
    """zz[i] = min_z + (span i) / (n - 1), each operation rounded on its own (n >= 2)."""
    span = max_z - min_z
    return min_z + (span * np.arange(n, dtype=np.float64)) / float(n - 1)


def path_terms(good, min_z, max_z, z_upper, z_lo, z_hi, pixel_cut, omega_m=0.279):
    """The terms of one spectrum's path in [z_lo, z_hi] (a list, empty: no contribution)."""
    n = len(good)
    if not (min_z < z_hi and z_upper > z_lo):
        return []
    pmin, pmax = max(z_lo, min_z), min(z_hi, z_upper)
    X = lambda z: float(absorption_distance(z, omega_m))   # noqa: E731
    if not pixel_cut or (n >= 1 and bool(np.all(good))):
        return [X(pmax) - X(pmin)]
    if n < 2:
        return []
    z = zz(min_z, max_z, n)
    inside = good & (z >= pmin)
    terms = []
    for i in range(n - 1):
        if not (inside[i] and (i == 0 or not inside[i - 1]) and z[i] <= pmax):
            continue
        bad = np.flatnonzero(~good[i + 1:])
        e = i + 1 + int(bad[0]) if bad.size else None
        top = X(z[e - 1]) if e is not None and z[e] < pmax else X(pmax)
        terms.append(top - X(z[i]))
    return terms


def path_columns(good, min_z, max_z, z_upper, z_edges, pixel_cut, omega_m=0.279):
    """(nz + 1 path values -- each bin, then the whole extent -- and the number of terms of each)."""
    e = np.asarray(z_edges, dtype=np.float64)
    spans = [(e[c], e[c + 1]) for c in range(e.size - 1)] + [(e[0], e[-1])]
    terms = [path_terms(good, min_z, max_z, z_upper, lo, hi, pixel_cut, omega_m) for lo, hi in spans]
    return np.array([math.fsum(t) for t in terms]), np.array([len(t) for t in terms])


def search_cuts(wavelengths, noise_variance, min_z, max_z, proximity_zone=None, noise_thresh=None, z_edges_summary=None,
                z_edges_population=None, omega_m=0.279):
    """``engine.search_cuts``'s dict, plus ``terms_summary`` / ``terms_population`` (the number of path terms
    behind each value, for the error bound) and ``goods`` (the per-spectrum flag vectors)."""
    Q = len(wavelengths)
    goods, zus = [], np.zeros(Q)
    for q in range(Q):
        g, zus[q] = spectrum_cut(wavelengths[q], noise_variance[q], min_z[q], max_z[q], proximity_zone, noise_thresh)
        goods.append(g)
    off, words = bitmap([(g, (np.size(wavelengths[q]) + 31) // 32) for q, g in enumerate(goods)])
    out = dict(cut_proximity_zone=float(proximity_zone) if _on(proximity_zone) else math.nan,
               cut_noise_thresh=float(noise_thresh) if _on(noise_thresh) else math.nan, cut_z_uppers=zus,
               cut_pixel_counts=np.array([len(g) for g in goods], dtype=np.int32), cut_bitmap_offsets=off,
               cut_bitmap_words=words, goods=goods)
    for name, edges in (("summary", z_edges_summary), ("population", z_edges_population)):
        if edges is None:
            continue
        cols = [path_columns(goods[q], float(min_z[q]), float(max_z[q]), zus[q], edges, _on(noise_thresh), omega_m)
                for q in range(Q)]
        out["cut_path_" + name] = np.array([c[0] for c in cols]).reshape(Q, -1)
        out["terms_" + name] = np.array([c[1] for c in cols]).reshape(Q, -1)
    return out


def slot_kept(z, min_z, max_z, z_upper, good, proximity, pixel_cut):
    """Whether absorber slots at redshifts ``z`` (any shape) pass the cuts of their spectrum."""
    z = np.asarray(z, dtype=np.float64)
    keep = np.ones(z.shape, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        if proximity:
            keep &= z < z_upper
        if pixel_cut:
            n = len(good)
            span = max_z - min_z
            f = ((z - min_z) / span) * float(n)
            ok = (f > -1.0) & (f < float(n)) & (span != 0.0)
            idx = np.where(ok, f, 0.0).astype(np.int64)          # truncation toward zero
            keep &= ok & (np.asarray(good, dtype=bool)[idx] if n else np.zeros(z.shape, dtype=bool))
    return keep


def kept_samples(cuts, min_z, max_z, offset):
    """rows x S flags of the sample redshifts, from a ``search_cuts`` dict of this module."""
    prox, pix = _on(cuts["cut_proximity_zone"]), _on(cuts["cut_noise_thresh"])
    off = np.asarray(offset, dtype=np.float64)
    return np.stack([slot_kept(PO.sample_z(min_z[r], max_z[r], off), min_z[r], max_z[r], cuts["cut_z_uppers"][r],
                               cuts["goods"][r], prox, pix) for r in range(len(min_z))])


def _row_log_nhi(kept_row, log_nhi):
    """A row's log N_HI samples with NaN where the cuts drop the sample's slot: a NaN belongs to no bin
    (posterior_summary_oracle.bin_index), and nothing else reads the value."""
    return np.where(kept_row, np.asarray(log_nhi, dtype=np.float64), np.nan)


def level_planes(cuts, ll, base, min_z, max_z, offset, log_nhi, nhi, z_edges, n_edges):
    """level_population_oracle.level_planes under the cuts, row by row."""
    ll = np.asarray(ll, dtype=np.float64)
    kept = kept_samples(cuts, min_z, max_z, offset)
    parts = [LO.level_planes(ll[:, r:r + 1], None if base is None else np.asarray(base)[:, r:r + 1], min_z[r:r + 1],
                             max_z[r:r + 1], offset, _row_log_nhi(kept[r], log_nhi), nhi, z_edges, n_edges)
             for r in range(ll.shape[1])]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def level_split(cuts, ll, base, min_z, max_z, level_posteriors, offset, log_nhi, z_edges, n_edges, **thresholds):
    """level_population_oracle.level_split under the cuts, row by row."""
    ll = np.asarray(ll, dtype=np.float64)
    P = np.asarray(level_posteriors, dtype=np.float64).reshape(ll.shape[0], ll.shape[1])
    kept = kept_samples(cuts, min_z, max_z, offset)
    parts = [LO.level_split(ll[:, r:r + 1], None if base is None else np.asarray(base)[:, r:r + 1], min_z[r:r + 1],
                            max_z[r:r + 1], P[:, r:r + 1], offset, _row_log_nhi(kept[r], log_nhi), z_edges, n_edges,
                            **thresholds) for r in range(ll.shape[1])]
    return {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}


def margins(cuts, min_z, max_z, offset):
    """How far any sample is from a cut decision rounding could take the other way: (the smallest |z - z_upper|,
    the smallest distance of ((z - min_z) / span) n to an integer); inf where a cut is off."""
    prox, pix = _on(cuts["cut_proximity_zone"]), _on(cuts["cut_noise_thresh"])
    off = np.asarray(offset, dtype=np.float64)
    dz, di = math.inf, math.inf
    for r in range(len(min_z)):
        z = PO.sample_z(min_z[r], max_z[r], off)
        if prox:
            dz = min(dz, float(np.abs(z - cuts["cut_z_uppers"][r]).min()))
        n = len(cuts["goods"][r])
        if pix and n and max_z[r] != min_z[r]:
            f = ((z - min_z[r]) / (max_z[r] - min_z[r])) * n
            di = min(di, float(np.abs(f - np.rint(f)).min()))
    return dz, di

"""Host oracles of the bootstrap and SNR kernels (csrc/bootstrap.hip, csrc/snr.hip), in Python integers and
numpy: Philox4x64-10, the draw rule of include/gpdla.h "Bootstrap sample errors", the rows and sums through
``catalog.cddf_moments`` on gathered spectra (``math.fsum`` for the exact sums), and ``find_snr``
(calc_cddf.py:906-924) with every dtype explicit."""
import math

import numpy as np

from gp_dla_detection_amd import catalog as CAT

MASK = (1 << 64) - 1
M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B


def philox4x64_10(counter, key):
    """Salmon et al. 2011 (Random123 philox4x64, 10 rounds): four 64-bit words from a four-word counter and a
    two-word key."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 64) ^ c1 ^ k0, p1 & MASK, (p0 >> 64) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def seed_words(seed):
    """The key of ``engine._bootstrap_spec``: an integer below 2^128 as (low, high) words, or the pair itself."""
    if isinstance(seed, (int, np.integer)):
        return int(seed) & MASK, int(seed) >> 64
    return int(seed[0]), int(seed[1])


def draws(replica: int, seed, stratum_offsets, members):
    """The spectra replica ``replica`` draws, in draw order: draw g = word g & 3 of counter (g >> 2, 0, replica, 0);
    with s its stratum, members[offsets[s] + mulhi64(word, n_s)]."""
    key = seed_words(seed)
    so = [int(v) for v in stratum_offsets]
    out = []
    s, words = 0, None
    for g in range(so[-1]):
        if g & 3 == 0 or words is None:
            words = philox4x64_10((g >> 2, 0, replica, 0), key)
        while g >= so[s + 1]:
            s += 1
        n = so[s + 1] - so[s]
        out.append(int(members[so[s] + ((words[g & 3] * n) >> 64)]))
    return out


def counts(Q: int, replicas: int, seed, stratum_offsets=None, members=None, first_replica: int = 0):
    """replicas x Q int32 multiplicities."""
    if members is None:
        stratum_offsets, members = [0, Q], np.arange(Q)
    c = np.zeros((replicas, Q), dtype=np.int32)
    for b in range(replicas):
        np.add.at(c[b], draws(first_replica + b, seed, stratum_offsets, members), 1)
    return c


def rows(planes, p_dlas, keep=None, p_thresh_spec=0.05, level_posteriors=None):
    """Q x 4 nz nn: numpy's own ``p * planes[a]`` and ``p * planes[b] - p * p * planes[c]`` of ``cddf_moments``
    (levels: from zeros, ``+=`` per level ascending, NaN P_d skipped, as ``_cddf_moments_levels``), zeros for
    the spectra it skips."""
    planes = np.asarray(planes, dtype=np.float64)
    p = np.asarray(p_dlas, dtype=np.float64).ravel()
    Q = planes.shape[0]
    nb = planes.shape[-1] * planes.shape[-2]
    use = p > p_thresh_spec
    if keep is not None:
        use &= np.asarray(keep, dtype=bool).ravel()
    out = np.zeros((Q, 4 * nb))
    for q in np.flatnonzero(use):
        for mom, (a, b, c) in enumerate(((CAT.PLANE_PI, CAT.PLANE_PI, CAT.PLANE_PI2),
                                         (CAT.PLANE_NPI, CAT.PLANE_N2PI, CAT.PLANE_N2PI2))):
            if level_posteriors is None:
                m = p[q] * planes[q, a]
                v = p[q] * planes[q, b] - p[q] * p[q] * planes[q, c]
            else:
                P = np.asarray(level_posteriors, dtype=np.float64).reshape(Q, -1)
                pl = planes[q] if planes.ndim == 5 else planes[q][None]
                m, v = np.zeros(planes.shape[-2:]), np.zeros(planes.shape[-2:])
                for d in range(pl.shape[0]):
                    if np.isnan(P[q, d]):
                        continue
                    m += P[q, d] * pl[d, a]
                    v += P[q, d] * pl[d, b] - P[q, d] * P[q, d] * pl[d, c]
            out[q, 2 * mom * nb:(2 * mom + 1) * nb] = m.ravel()
            out[q, (2 * mom + 1) * nb:(2 * mom + 2) * nb] = v.ravel()
    return out


def exact_sums(cnt, r):
    """(counts @ rows, sum_q |counts rows|), every entry the exact sum rounded once (``math.fsum``).  A count
    times a double need not be a double, so each row value is cut into its top 26 significand bits and the
    (exact) rest, at most 27 bits and of the same sign: with counts below 2^20 both partial products are exact,
    and the sum of their magnitudes is the term's."""
    cnt = np.asarray(cnt, dtype=np.int64)
    r = np.asarray(r, dtype=np.float64)
    assert cnt.min() >= 0 and cnt.max() < 1 << 20
    B, N = cnt.shape[0], r.shape[1]
    m, e = np.frexp(r)
    r_hi = np.ldexp(np.trunc(np.ldexp(m, 26)), e - 26)
    r_lo = r - r_hi
    got, mag = np.zeros((B, N)), np.zeros((B, N))
    for b in range(B):
        nzq = np.flatnonzero(cnt[b])
        c = cnt[b, nzq].astype(np.float64)[:, None]
        t_hi, t_lo = c * r_hi[nzq], c * r_lo[nzq]
        for n in range(N):
            terms = t_hi[:, n].tolist() + t_lo[:, n].tolist()
            got[b, n] = math.fsum(terms)
            mag[b, n] = math.fsum(abs(t) for t in terms)
    return got, mag


def sums_via_cddf_moments(planes, p_dlas, level_posteriors, keep, p_thresh_spec, path, replicas, first_replica, seed,
                          stratum_offsets, members):
    """The ``sums=`` callable of ``catalog.bootstrap_moments`` on the host, the parent commit's only route:
    ``catalog.cddf_moments`` on each replica's gathered spectra (its variances minus its means are the variance
    terms) and the path columns summed over the gathered spectra with ``math.fsum``."""
    planes = np.asarray(planes, dtype=np.float64)
    nz, nn = planes.shape[-2:]
    nb = nz * nn
    out = np.zeros((replicas, 4 * nb + nz + 1))
    kept = None if keep is None else np.asarray(keep, dtype=bool).ravel()
    for b in range(replicas):
        idx = np.array(draws(first_replica + b, seed, stratum_offsets, members), dtype=np.int64)
        kw = dict(keep=None if kept is None else kept[idx], p_thresh_spec=p_thresh_spec)
        if level_posteriors is not None:
            kw.update(levels="all", level_posteriors=np.asarray(level_posteriors)[idx])
        for mom in (0, 1):
            m, v = CAT.cddf_moments(planes[idx], np.asarray(p_dlas)[idx], moment=bool(mom), **kw)
            out[b, 2 * mom * nb:(2 * mom + 1) * nb] = m.ravel()
            out[b, (2 * mom + 1) * nb:(2 * mom + 2) * nb] = (v - m).ravel()
        for c in range(nz + 1):
            out[b, 4 * nb + c] = math.fsum(np.asarray(path)[idx, c].tolist())
    return out


def sums_all_ones(planes, p_dlas, level_posteriors, keep, p_thresh_spec, path, replicas, **_):
    """A ``sums=`` callable whose every replica is the sample itself (all counts 1), summed exactly."""
    r = np.hstack([rows(planes, p_dlas, keep, p_thresh_spec, level_posteriors), np.asarray(path)])
    got, _mag = exact_sums(np.ones((1, r.shape[0]), dtype=np.int64), r)
    return np.repeat(got, replicas, axis=0)


def find_snr(wavelengths, flux, noise_variance, max_z, norm=None):
    """calc_cddf.py:906-924 with explicit classes: both comparisons in double, the floor value formed in double
    and rounded to the cells' class, the ratio, numpy's median and the reciprocal in the cells' class."""
    w = np.asarray(wavelengths)
    dt = np.float32 if w.dtype == np.float32 else np.float64
    sel = w.astype(np.float64) > 1215.67 * (1.0 + float(max_z))
    f = np.array(np.asarray(flux, dtype=dt)[sel], dtype=dt)
    nv = np.asarray(noise_variance, dtype=dt)[sel]
    with np.errstate(all="ignore"):
        if norm is not None:
            f[f.astype(np.float64) / float(norm) < 0.1] = dt(float(norm) * 0.1)
        else:
            f[f.astype(np.float64) < 0.1] = dt(0.1)
        ratio = (np.sqrt(nv) / np.abs(f)).astype(dt)
        assert ratio.dtype == dt
        if ratio.size == 0 or np.isnan(ratio).any():
            return dt(np.nan)
        s = np.sort(ratio)
        n = s.size
        med = s[n // 2] if n % 2 else dt((s[n // 2 - 1] + s[n // 2]) / dt(2))
        return dt(dt(1) / med)

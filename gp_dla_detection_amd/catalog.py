"""The last stage after ``process_qsos``: the ASCII DLA catalogue (generate_ascii_catalog.m) and the
binned population moments (CDDF_analysis/calc_cddf.py ``_get_z_nhi_hist``), both from the posterior
summaries the engine reduces on the device (``Engine.process_summaries``, ``process_qsos(summaries=...)``)
instead of the Q x S sample array, and the population curves with their confidence bands -- f(N), dN/dX,
Omega_DLA (calc_cddf.py) -- from the population variables (``process_qsos(population=...)``), Omega_DLA both as
the moment estimator (``omega_dla``) and from the column density function with its posterior bands
(``omega_dla_cddf``)."""
from __future__ import annotations

import os
import re

import numpy as np

# bin_planes' second axis (include/gpdla.h GPDLA_SUMMARY_PLANES)
PLANE_PI, PLANE_PI2, PLANE_NPI, PLANE_N2PI, PLANE_N2PI2 = range(5)


LEVELS = ("first", "all")


def _check_levels(levels: str) -> bool:
    """True for ``levels="all"`` (every absorber of every multi-DLA level), False for "first" (today's
    level-1 statistics)."""
    if levels not in LEVELS:
        raise ValueError(f"levels must be one of {LEVELS}")
    return levels == "all"


def cddf_moments(bin_planes, p_dlas, keep=None, p_thresh_spec: float = 0.05, moment: bool = False,
                 levels: str = "first", level_posteriors=None):
    """``_get_z_nhi_hist`` (calc_cddf.py:829-870) on the whole (z, log N_HI) grid at once: the expected
    number of DLAs per bin (``moment``: the expected column density) and its variance, the Poisson-binomial
    sum over spectra plus the Poisson sampling term.

    ``bin_planes`` is Q x 5 x nz x nn, ``p_dlas`` the Q model posteriors of at least one DLA.  Spectra
    with ``p_dla <= p_thresh_spec`` (calc_cddf.py:286 ``filter_dla_spectra``) or ``keep`` false (its SNR /
    condition mask) contribute nothing.  With pi the normalised sample masses of a spectrum and p its p_dla,

        means     = sum_q p A              variances = sum_q (p B - p^2 C) + means
        (A, B, C) = (sum pi, sum pi, sum pi^2)               or, with ``moment``,
                    (sum N pi, sum N^2 pi, sum N^2 pi^2)

    which is sum w p pi and sum w^2 (1 - p pi) p pi over a bin's samples (w = 1 or N).  Returns
    (means, variances), each nz x nn; the reference's one-dimensional histograms are their sums over the
    other axis (dN/dX and Omega_DLA over log N_HI, the CDDF over z).

    ``levels="all"`` counts every absorber of every level of a multi-DLA run:
    ``bin_planes`` is then ``bin_planes_levels``, Q x D x 5 x nz x nn (a Q x 5 x nz x nn array counts as D = 1),
    ``level_posteriors`` the Q x D posteriors P_d of exactly d DLAs (``model_posteriors[:, 1:1 + D]``; for D = 1
    it defaults to ``p_dlas``), and

        means = sum_q sum_d P_d A_d          variances = sum_q sum_d (P_d B_d - P_d^2 C_d) + means

    with level d's planes, every (level, sample, slot) one Bernoulli trial of probability P_d pi_{d,j}.  The
    spectrum filter stays ``p_dlas > p_thresh_spec`` and ``keep``."""
    if _check_levels(levels):
        return _cddf_moments_levels(bin_planes, p_dlas, keep, p_thresh_spec, moment, level_posteriors)
    planes = np.asarray(bin_planes, dtype=np.float64)
    if planes.ndim != 4 or planes.shape[1] != 5:
        raise ValueError("bin_planes must be Q x 5 x nz x nn")
    p = np.asarray(p_dlas, dtype=np.float64).ravel()
    if p.size != planes.shape[0]:
        raise ValueError("one p_dla per spectrum")
    use = p > p_thresh_spec
    if keep is not None:
        use &= np.asarray(keep, dtype=bool).ravel()
    a, b, c = (PLANE_NPI, PLANE_N2PI, PLANE_N2PI2) if moment else (PLANE_PI, PLANE_PI, PLANE_PI2)
    means = np.zeros(planes.shape[2:])
    variances = np.zeros(planes.shape[2:])
    for q in np.flatnonzero(use):      # spectrum by spectrum, as the reference accumulates
        means += p[q] * planes[q, a]
        variances += p[q] * planes[q, b] - p[q] * p[q] * planes[q, c]
    variances += means
    return means, variances


def _cddf_moments_levels(bin_planes, p_dlas, keep, p_thresh_spec, moment, level_posteriors):
    """``cddf_moments(levels="all")``."""
    planes = np.asarray(bin_planes, dtype=np.float64)
    if planes.ndim == 4:
        planes = planes[:, None]
    if planes.ndim != 5 or planes.shape[2] != 5:
        raise ValueError("bin_planes must be Q x D x 5 x nz x nn")
    Q, D = planes.shape[:2]
    p = np.asarray(p_dlas, dtype=np.float64).ravel()
    if p.size != Q:
        raise ValueError("one p_dla per spectrum")
    if level_posteriors is None:
        if D != 1:
            raise ValueError("levels='all' with D > 1 needs level_posteriors (Q x D)")
        P = p[:, None]
    else:
        P = np.asarray(level_posteriors, dtype=np.float64).reshape(Q, -1)
        if P.shape[1] != D:
            raise ValueError("level_posteriors must be Q x D")
    use = p > p_thresh_spec
    if keep is not None:
        use &= np.asarray(keep, dtype=bool).ravel()
    a, b, c = (PLANE_NPI, PLANE_N2PI, PLANE_N2PI2) if moment else (PLANE_PI, PLANE_PI, PLANE_PI2)
    means = np.zeros(planes.shape[3:])
    variances = np.zeros(planes.shape[3:])
    for q in np.flatnonzero(use):      # spectrum by spectrum, level ascending
        for d in range(D):
            if np.isnan(P[q, d]):
                continue
            means += P[q, d] * planes[q, d, a]
            variances += P[q, d] * planes[q, d, b] - P[q, d] * P[q, d] * planes[q, d, c]
    variances += means
    return means, variances


def poisson_binomial_pmf(probs_per_bin, device: int = 0) -> list:
    """The Poisson-binomial pmf of each trial list, on the device (gpdla_poisson_binomial_pmf_f64): for a list
    of n probabilities the n + 1 coefficients of prod_j (1 - p_j + p_j x), i.e. Pr(k successes).  It stands
    where the reference calls ``get_poisson_binomial_pdf`` (calc_cddf.py:1021-1044), but as a product of
    polynomials with non-negative coefficients instead of a characteristic-function DFT, so the tails keep a
    relative accuracy.  An empty list gives ``[1.0]`` (:1024-1025).  Returns one array per list."""
    from .engine import poisson_binomial_pmf_csr
    lists = [np.ascontiguousarray(p, dtype=np.float64).ravel() for p in probs_per_bin]
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([p.size for p in lists], out=offsets[1:])
    flat = poisson_binomial_pmf_csr(np.concatenate(lists) if lists else np.zeros(0), offsets, device=device)
    return [flat[offsets[b] + b: offsets[b + 1] + b + 1].copy() for b in range(len(lists))]


def _population(out):
    """The population variables of ``process_qsos(population=...)`` in working form: (Q x nz x nn Poisson
    plane, Q x 8 0-based sample indices with -1 = none, probabilities, 0-based flat bins, nz, nn)."""
    plane = np.asarray(out["population_poisson"], dtype=np.float64)
    if plane.ndim != 3:
        raise ValueError("population_poisson must be Q x nz x nn")
    Q, nz, nn = plane.shape
    inds = np.asarray(out["population_large_inds"], dtype=np.float64).reshape(Q, -1).astype(np.int64) - 1
    bins = np.asarray(out["population_large_bins"], dtype=np.float64).reshape(Q, -1).astype(np.int64) - 1
    probs = np.asarray(out["population_large_probs"], dtype=np.float64).reshape(Q, -1)
    return plane, inds, probs, bins, nz, nn


def _population_levels(out):
    """The LEVEL_POPULATION_VARIABLES of the split (``process_qsos(population=dict(..., levels="all"))``) in
    working form: (Q x D x nz x nn Poisson planes, Q x D x 8 0-based sample indices with -1 = none,
    probabilities, Q x D x 8 x 4 0-based flat bins, nz, nn)."""
    plane = np.asarray(out["population_level_poisson"], dtype=np.float64)
    if plane.ndim != 4:
        raise ValueError("population_level_poisson must be Q x D x nz x nn")
    Q, D, nz, nn = plane.shape
    inds = np.asarray(out["population_level_large_inds"], dtype=np.float64).reshape(Q, D, -1).astype(np.int64) - 1
    probs = np.asarray(out["population_level_large_probs"], dtype=np.float64).reshape(Q, D, -1)
    bins = np.asarray(out["population_level_large_bins"], dtype=np.float64).reshape(Q, D, inds.shape[2], -1).astype(np.int64) - 1
    return plane, inds, probs, bins, nz, nn


def split_distributions(out, keep=None, p_thresh_spec: float = 0.05, axis: str = "log_nhi", levels: str = "first"):
    """``_split_distributions_single`` (calc_cddf.py:724-778) from the population variables the engine reduced
    (``process_qsos(population=...)``): per bin of ``axis`` -- ``"log_nhi"`` for the CDDF (the grid collapsed
    over z, ``nhi=True``) or ``"z"`` for dN/dX (collapsed over log N_HI) -- the probabilities kept exactly
    (p >= p_switch; spectrum by spectrum and in sample order within one, the order the reference appends
    them in, :771-773) and the mean of the Poisson approximation to the rest (:767-769,774; summed with
    ``math.fsum`` as there).  Spectra with ``p_dla <= p_thresh_spec`` (:732, ``filter_dla_spectra``) or
    ``keep`` false contribute nothing.  Returns (list of probability arrays, array of Poisson means).

    ``levels="all"`` reads the LEVEL_POPULATION_VARIABLES instead: every (level, sample,
    slot) is one trial of probability P_d pi_{d,j} in the slot's bin, the lists built spectrum by spectrum, level
    ascending, sample index ascending, slot ascending, and the Poisson mean of a bin the ``fsum`` over every
    level's plane entries.  The spectrum filter is the same."""
    import math
    if axis not in ("log_nhi", "z"):
        raise ValueError("axis must be 'log_nhi' or 'z'")
    if _check_levels(levels):
        return _split_distributions_levels(out, keep, p_thresh_spec, axis)
    plane, inds, probs, bins, nz, nn = _population(out)
    p = np.asarray(out["p_dlas"], dtype=np.float64).ravel()
    if p.size != plane.shape[0]:
        raise ValueError("one p_dla per spectrum")
    use = p > p_thresh_spec
    if keep is not None:
        use &= np.asarray(keep, dtype=bool).ravel()
    nb = nn if axis == "log_nhi" else nz
    lists = [[] for _ in range(nb)]
    small = [[] for _ in range(nb)]
    for q in np.flatnonzero(use):
        for slot in np.flatnonzero(inds[q] >= 0):          # increasing sample index
            b = bins[q, slot] % nn if axis == "log_nhi" else bins[q, slot] // nn
            lists[b].append(probs[q, slot])
        for b in range(nb):
            part = plane[q, :, b] if axis == "log_nhi" else plane[q, b, :]
            small[b].extend(part[part > 0].tolist())
    return [np.array(v, dtype=np.float64) for v in lists], np.array([math.fsum(v) for v in small])


def _split_distributions_levels(out, keep, p_thresh_spec, axis):
    """``split_distributions(levels="all")``."""
    import math
    plane, inds, probs, bins, nz, nn = _population_levels(out)
    Q, D = plane.shape[:2]
    p = np.asarray(out["p_dlas"], dtype=np.float64).ravel()
    if p.size != Q:
        raise ValueError("one p_dla per spectrum")
    use = p > p_thresh_spec
    if keep is not None:
        use &= np.asarray(keep, dtype=bool).ravel()
    nb = nn if axis == "log_nhi" else nz
    lists = [[] for _ in range(nb)]
    small = [[] for _ in range(nb)]
    for q in np.flatnonzero(use):
        for d in range(D):
            for entry in np.flatnonzero(inds[q, d] >= 0):      # increasing sample index
                for fb in bins[q, d, entry]:                   # slot ascending
                    if fb >= 0:
                        lists[fb % nn if axis == "log_nhi" else fb // nn].append(probs[q, d, entry])
            for b in range(nb):
                part = plane[q, d, :, b] if axis == "log_nhi" else plane[q, d, b, :]
                small[b].extend(part[part > 0].tolist())
    return [np.array(v, dtype=np.float64) for v in lists], np.array([math.fsum(v) for v in small])


def _interval(cdf, level: float, offset: int = 0):
    """``interval`` (calc_cddf.py:986-1005; the branch it always takes): the first index at or above the
    lower tail and one past the first index above the upper one; a cdf that never exceeds the upper level
    gives its length, without the offset, as there (:1003)."""
    cdf = np.asarray(cdf)
    if cdf.size == 1:
        return offset, offset
    low, high = offset, 1 + offset
    down = np.flatnonzero(cdf < 0.5 - level / 2)
    if down.size:
        low += int(down[-1]) + 1
    up = np.flatnonzero(cdf > 0.5 + level / 2)
    high = high + int(up[0]) if up.size else int(cdf.size)
    return low, high


def count_intervals(pmf, poisson_mean: float):
    """``_get_combined_levels`` and ``pdf_confidence`` (calc_cddf.py:780-798, 1007-1019): the pmf of the
    exactly kept trials convolved with the Poisson pmf of mean ``poisson_mean``, both cut to their central
    1 - 1e-4 (:789-796; a zero mean leaves the pmf alone, :784-785), then the count at which the cdf reaches
    one half and the 68 % and 95 % intervals.  Returns (count, (low68, high68), (low95, high95)), integers."""
    import math
    pmf = np.asarray(pmf, dtype=np.float64).ravel()
    offset = 0
    if poisson_mean != 0.0:
        from scipy.stats import poisson
        weak = poisson(poisson_mean)
        plow, phigh = (int(v) for v in weak.interval(1 - 1e-4))
        dlow, dhigh = _interval(np.cumsum(pmf), 1 - 1e-4)
        top = min(dhigh + 1, pmf.size)
        pmf = np.array([math.fsum(weak.pmf(n - i) * pmf[i] for i in range(dlow, top))
                        for n in range(plow + dlow, phigh + dhigh + 1)])
        offset = plow + dlow
    cdf = np.cumsum(pmf)
    return _interval(cdf, 0.0, offset)[0], _interval(cdf, 0.68, offset), _interval(cdf, 0.95, offset)


def confidence_intervals(out, keep=None, p_thresh_spec: float = 0.05, axis: str = "log_nhi", device: int = 0, pmf=None,
                         levels: str = "first"):
    """``_get_confidence_intervals`` (calc_cddf.py:800-827): ``split_distributions``, the device pmf of every
    bin's exact list and ``count_intervals``.  ``pmf(lists)`` replaces the device call (tests, as ``compute``
    does for ``process_qsos``).  ``levels`` as in ``split_distributions``.  Returns (counts [nb], intervals68
    [nb x 2], intervals95 [nb x 2])."""
    lists, means = split_distributions(out, keep, p_thresh_spec, axis, levels)
    pmfs = poisson_binomial_pmf(lists, device=device) if pmf is None else pmf(lists)
    got = [count_intervals(one, mean) for one, mean in zip(pmfs, means)]
    return (np.array([g[0] for g in got]), np.array([g[1] for g in got]).reshape(-1, 2),
            np.array([g[2] for g in got]).reshape(-1, 2))


def absorption_distance(z, omega_m: float = 0.279):
    """X(z) with dX = (1 + z)^2 H_0 / H(z) dz (calc_cddf.py:1058-1063, flat LCDM without radiation, :978-984):
    the integrand has the antiderivative 2 sqrt(Omega_m (1 + z)^3 + 1 - Omega_m) / (3 Omega_m)."""
    z = np.asarray(z, dtype=np.float64)
    return 2.0 * np.sqrt(omega_m * (1.0 + z) ** 3 + (1.0 - omega_m)) / (3.0 * omega_m)


def path_length(z_lo: float, z_hi: float, min_z_dlas, max_z_dlas, keep=None, omega_m: float = 0.279) -> float:
    """The absorption path searched between ``z_lo`` and ``z_hi`` (calc_cddf.py:334-385 without pixel
    filtering): every spectrum with ``keep`` true (the reference's SNR / condition mask, :347; no p_dla cut)
    whose search range overlaps the interval (:355) contributes X(min(z_hi, max_z)) - X(max(z_lo, min_z)).
    Vectorised over spectra.  No quadrature: the antiderivative is closed (``absorption_distance``), so a
    spectrum's term is exact to a few ulp of X (< 4e-15 absolute below z = 7), where the reference's ``quad``
    stops at 1.5e-8 per integral."""
    import math
    if not z_lo < z_hi:
        raise ValueError("z_lo must be below z_hi")
    zmin = np.asarray(min_z_dlas, dtype=np.float64).ravel()
    zmax = np.asarray(max_z_dlas, dtype=np.float64).ravel()
    use = (zmin < z_hi) & (zmax > z_lo)
    if keep is not None:
        use &= np.asarray(keep, dtype=bool).ravel()
    hi, lo = np.minimum(z_hi, zmax[use]), np.maximum(z_lo, zmin[use])
    return math.fsum(absorption_distance(hi, omega_m) - absorption_distance(lo, omega_m))


def cut_path_columns(out, grid: str, keep=None, omega_m: float = 0.279):
    """The per-spectrum path columns a run under the search cuts stored (``process_qsos(cuts=...)``; DESIGN.md
    section 22) for ``grid`` ("summary": ``cut_path_summary`` on ``bin_z_edges``; "population":
    ``cut_path_population`` on ``population_z_edges``), Q x (nz + 1) -- each z bin, then the whole extent -- with the
    rows ``keep`` drops zeroed: what takes ``path_columns``'s place, so that cut planes never meet an uncut path.
    None for an ``out`` without the cut variables.  ValueError when the run stored no path for the grid, or stored
    it for another ``omega_m``."""
    if "cut_z_uppers" not in out:
        return None
    key = "cut_path_" + grid
    if key not in out:
        raise ValueError(f"the run was cut but holds no {key}: its planes cannot be paired with an uncut path")
    if "cut_omega_m" in out and float(np.ravel(out["cut_omega_m"])[0]) != float(omega_m):
        raise ValueError(f"the stored cut path is for omega_m = {float(np.ravel(out['cut_omega_m'])[0])}, not {omega_m}")
    cols = np.array(out[key], dtype=np.float64)
    if keep is not None:
        cols[~np.asarray(keep, dtype=bool).ravel()] = 0.0
    return cols


def _bin_paths(out, grid: str, z_edges, keep, omega_m):
    """(the path of every bin of ``z_edges``, the path of their whole extent): ``path_length``, or for a run under
    the search cuts the ``fsum`` of the stored columns of ``grid``."""
    import math
    ez = np.asarray(z_edges, dtype=np.float64).ravel()
    cols = cut_path_columns(out, grid, keep, omega_m)
    if cols is None:
        zmin, zmax = out["min_z_dlas"], out["max_z_dlas"]
        return (np.array([path_length(a, b, zmin, zmax, keep, omega_m) for a, b in zip(ez[:-1], ez[1:])]),
                path_length(ez[0], ez[-1], zmin, zmax, keep, omega_m))
    if cols.ndim != 2 or cols.shape[1] != ez.size:
        raise ValueError(f"cut_path_{grid} must hold {ez.size} columns")
    sums = np.array([math.fsum(cols[:, c]) for c in range(ez.size)])
    return sums[:-1], float(sums[-1])


def column_density_function(out, keep=None, p_thresh_spec: float = 0.05, omega_m: float = 0.279, device: int = 0,
                            pmf=None, levels: str = "first"):
    """f(N) = n_DLA / dN / dX (calc_cddf.py:440-464) on the population grid of ``out``: the log N_HI bins are
    ``population_log_nhi_edges`` and the redshift range its whole z extent; ``levels="all"`` counts every
    absorber of every multi-DLA level (``split_distributions``).  Returns (bin centres in log N_HI,
    f(N), its 68 % band [nn x 2], its 95 % band, (lower, upper) bin half-widths in N_HI).  For an ``out`` of a
    run under the search cuts the path is the stored cut one (``cut_path_columns``), here and in ``line_density``,
    ``omega_dla``, ``omega_dla_cddf``, ``bootstrap_moments`` and ``sample_errors``."""
    ez = np.asarray(out["population_z_edges"], dtype=np.float64).ravel()
    en = np.asarray(out["population_log_nhi_edges"], dtype=np.float64).ravel()
    n, l68, l95 = confidence_intervals(out, keep, p_thresh_spec, "log_nhi", device, pmf, levels)
    dX = _bin_paths(out, "population", ez, keep, omega_m)[1]
    dN = 10.0 ** en[1:] - 10.0 ** en[:-1]
    cent = (en[1:] + en[:-1]) / 2.0
    xerrs = (10.0 ** cent - 10.0 ** en[:-1], 10.0 ** en[1:] - 10.0 ** cent)
    return cent, n / dX / dN, l68 / dX / dN[:, None], l95 / dX / dN[:, None], xerrs


def line_density(out, keep=None, p_thresh_spec: float = 0.05, omega_m: float = 0.279, device: int = 0, pmf=None,
                 levels: str = "first"):
    """dN/dX per redshift bin (calc_cddf.py:490-507) on the population grid of ``out``: the bins are
    ``population_z_edges`` and the column densities its whole log N_HI extent; bins without path are dropped
    (:500); ``levels`` as in ``column_density_function``.  Returns (bin centres, dN/dX, 68 % band, 95 % band,
    (lower, upper) half-widths)."""
    ez = np.asarray(out["population_z_edges"], dtype=np.float64).ravel()
    n, l68, l95 = confidence_intervals(out, keep, p_thresh_spec, "z", device, pmf, levels)
    dX = _bin_paths(out, "population", ez, keep, omega_m)[0]
    ii = dX > 0
    cent = (ez[1:] + ez[:-1]) / 2.0
    xerrs = (cent[ii] - ez[:-1][ii], ez[1:][ii] - cent[ii])
    return cent[ii], n[ii] / dX[ii], l68[ii] / dX[ii, None], l95[ii] / dX[ii, None], xerrs


PROTON_MASS_G = 1.67262178e-24        # calc_cddf.py:651
H100_PER_S = 3.2407789e-18            # 100 km/s/Mpc in 1/s (:655)
LIGHT_CM_PER_S = 2.99e10              # :657, the reference's own rounding
GRAVITY_CGS = 6.674e-8                # :1070


def rho_crit(hubble: float = 0.7) -> float:
    """Critical density at z = 0 in g cm^-3 (calc_cddf.py:1065-1072)."""
    import math
    return 3.0 * (H100_PER_S * hubble) ** 2 / (8.0 * math.pi * GRAVITY_CGS)


def omega_dla(out, keep=None, p_thresh_spec: float = 0.05, hubble: float = 0.7, omega_m: float = 0.279,
              levels: str = "first"):
    """Omega_DLA per redshift bin by summing column densities (calc_cddf.py:638-662), the moment version:
    ``cddf_moments(moment=True)`` on the summary grid of ``out`` (``bin_planes`` with ``bin_z_edges``; every
    log N_HI bin of it counts) over the path lengths, in the reference's units -- m_p H_0 / (c rho_crit), with
    rho_crit at the reference's default h = 0.7 whatever ``hubble`` is (:658 calls it without the argument).
    ``levels="all"`` sums ``bin_planes_levels`` with the level posteriors ``model_posteriors[:, 1:1 + D]``
    (``cddf_moments``).  Returns (bin centres, Omega_DLA, its standard deviation, the z edges)."""
    ez = np.asarray(out["bin_z_edges"], dtype=np.float64).ravel()
    if _check_levels(levels):
        planes = np.asarray(out["bin_planes_levels"], dtype=np.float64)
        post = np.asarray(out["model_posteriors"], dtype=np.float64)
        means, variances = cddf_moments(planes, out["p_dlas"], keep, p_thresh_spec, moment=True, levels="all",
                                        level_posteriors=post.reshape(planes.shape[0], -1)[:, 1:1 + planes.shape[1]])
    else:
        means, variances = cddf_moments(out["bin_planes"], out["p_dlas"], keep, p_thresh_spec, moment=True)
    mean, variance = means.sum(axis=1), variances.sum(axis=1)
    dX = _bin_paths(out, "summary", ez, keep, omega_m)[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        conversion = PROTON_MASS_G * (H100_PER_S * hubble) / LIGHT_CM_PER_S / dX / rho_crit()
    return (ez[1:] + ez[:-1]) / 2.0, mean * conversion, np.sqrt(variance) * conversion, ez


def split_distributions_grid(out, keep=None, p_thresh_spec: float = 0.05, levels: str = "first"):
    """``_split_distributions_single(..., nhi=True)`` (calc_cddf.py:724-778) once per redshift bin of the
    population grid, as ``_get_omega_confidence_intervals`` asks for it (:568): for every (z bin, log N_HI bin)
    cell the probabilities kept exactly and the mean of the Poisson approximation to the rest.  The population
    variables, the spectrum filter, the order of a list (spectrum by spectrum, in sample order within one;
    ``levels="all"``: level, sample, slot ascending) and the ``fsum`` of a cell's Poisson terms over the spectra
    are ``split_distributions``'s.  Returns (lists[z][n], each an array; means, nz x nn)."""
    import math
    all_levels = _check_levels(levels)
    plane, inds, probs, bins, nz, nn = _population_levels(out) if all_levels else _population(out)
    Q = plane.shape[0]
    p = np.asarray(out["p_dlas"], dtype=np.float64).ravel()
    if p.size != Q:
        raise ValueError("one p_dla per spectrum")
    use = p > p_thresh_spec
    if keep is not None:
        use &= np.asarray(keep, dtype=bool).ravel()
    lists = [[[] for _ in range(nn)] for _ in range(nz)]
    small = [[[] for _ in range(nn)] for _ in range(nz)]
    for q in np.flatnonzero(use):
        if all_levels:
            for d in range(plane.shape[1]):
                for entry in np.flatnonzero(inds[q, d] >= 0):      # increasing sample index
                    for fb in bins[q, d, entry]:                   # slot ascending
                        if fb >= 0:
                            lists[fb // nn][fb % nn].append(probs[q, d, entry])
                for iz, ib in zip(*np.nonzero(plane[q, d] > 0)):
                    small[iz][ib].append(plane[q, d, iz, ib])
        else:
            for slot in np.flatnonzero(inds[q] >= 0):              # increasing sample index
                lists[bins[q, slot] // nn][bins[q, slot] % nn].append(probs[q, slot])
            for iz, ib in zip(*np.nonzero(plane[q] > 0)):
                small[iz][ib].append(plane[q, iz, ib])
    return ([[np.array(v, dtype=np.float64) for v in row] for row in lists],
            np.array([[math.fsum(v) for v in row] for row in small]).reshape(nz, nn))


MIXTURE_LEVELS = (0.5, 0.5 - 0.68 / 2, 0.5 + 0.68 / 2, 0.5 - 0.95 / 2, 0.5 + 0.95 / 2)   # interval's own expressions (:996,999)


def _column_stages(pmfs, means, atoms, tail_prob):
    """One redshift bin's stages for ``total_column_intervals``: per log N_HI bin the Poisson-binomial pmf of
    the exact list and the Poisson pmf of the rest, each cut to its central 1 - ``tail_prob`` as
    ``_get_combined_levels`` cuts them (calc_cddf.py:789-796), in ascending column density.  A stage that is
    exactly [1.0] (no exact trial, or a zero mean, :784-785) is dropped.  Returns (base, span, stages): the
    column of every stage's first kept count, the summed column of the kept spans, and per stage
    (probabilities, columns relative to the first kept count)."""
    from scipy.stats import poisson
    base, span, stages = 0.0, 0.0, []
    for pmf, mean, atom in zip(pmfs, means, atoms):
        pmf = np.asarray(pmf, dtype=np.float64).ravel()
        dlow, dhigh = _interval(np.cumsum(pmf), 1 - tail_prob)
        top = min(dhigh + 1, pmf.size)
        kept = [(dlow, pmf[dlow:top])]
        if mean != 0.0:
            plow, phigh = (int(v) for v in poisson.interval(1 - tail_prob, mean))
            kept.append((plow, poisson.pmf(np.arange(plow, phigh + 1), mean)))
        for first, prob in kept:
            base += first * atom
            if prob.size == 1 and prob[0] == 1.0:
                continue
            span += (prob.size - 1) * atom
            stages.append((prob, np.arange(prob.size, dtype=np.float64) * atom))
    return base, span, stages


def total_column_intervals(lists, means, log_nhi_edges, tail_prob: float = 1e-4, cells: int = 2 ** 20, device: int = 0,
                           pmf=None, mixture=None):
    """``_get_omega_confidence_intervals`` (calc_cddf.py:562-636) for every redshift bin at once: the
    distribution of the total column T = sum_b n_b c_b, c_b = 10^(centre of log N_HI bin b) (:576), where n_b is
    the sum of bin b's exact trials and a Poisson count, and the columns at which its cdf passes one half and
    the 68 % and 95 % levels.  ``lists`` and ``means`` are ``split_distributions_grid``'s.

    The reference multiplies lists of (value, probability) atoms out, merging atoms within 1e-3 of each other
    and lumping 5e-4 of either tail after every bin (:599-630).  Here T lives on a lattice of ``cells`` entries:
    every bin contributes two stages (``_column_stages``), the lattice covers the summed kept spans with step h,
    a count k_rel above a stage's first kept one shifts by rint(k_rel c_b / h) cells (formed here in float64, so
    the device and every oracle share the assignment), and the device convolves the stages one after the other
    (``engine.count_mixture``).  Each stage moves an atom by at most h / 2.  The levels are
    read off the unnormalised cdf, as the reference does.  The reference's ``tophat_prior`` branch (off by
    default) is left out.

    ``pmf(lists)`` replaces ``poisson_binomial_pmf`` and ``mixture(probs, shifts, tap_offsets, stage_offsets,
    cells, levels)`` -> (lower, upper, mass) the device convolution (tests).  Returns (median [nz], 68 % pair
    [nz x 2], 95 % pair [nz x 2], lattice step [nz]) in N_HI units; a bin without any stage has step 0."""
    en = np.asarray(log_nhi_edges, dtype=np.float64).ravel()
    means = np.asarray(means, dtype=np.float64)
    nn = en.size - 1
    if nn < 1 or means.ndim != 2 or means.shape[1] != nn or len(lists) != means.shape[0] or any(len(r) != nn for r in lists):
        raise ValueError("lists must be nz x nn arrays and means nz x nn, for the nn + 1 log_nhi_edges")
    if not (np.all(np.isfinite(en)) and np.all(np.diff(en) > 0)):
        raise ValueError("log_nhi_edges must be finite and strictly increasing")
    if not 0.0 < tail_prob < 0.05:
        raise ValueError("tail_prob must lie in (0, 0.05): the 95 % levels are read off what is kept")
    if not (np.all(np.isfinite(means)) and np.all(means >= 0)):
        raise ValueError("means must be finite and >= 0")
    if int(cells) != cells or cells < 1:
        raise ValueError("cells must be a positive integer")
    cells, nz = int(cells), means.shape[0]
    atoms = 10.0 ** ((en[1:] + en[:-1]) / 2.0)
    flat = [np.asarray(v, dtype=np.float64).ravel() for row in lists for v in row]
    pmfs = poisson_binomial_pmf(flat, device=device) if pmf is None else pmf(flat)
    bases, steps = np.zeros(nz), np.zeros(nz)
    probs, shifts, tap_offsets, stage_offsets = [], [], [0], [0]
    for iz in range(nz):
        bases[iz], span, stages = _column_stages(pmfs[iz * nn:(iz + 1) * nn], means[iz], atoms, tail_prob)
        # every stage's largest shift rounds up by at most a half, so this step keeps their sum below cells
        room = cells - 1 - len(stages)
        if stages and room < 1:
            raise ValueError(f"cells = {cells} leaves no lattice for the {len(stages)} stages of redshift bin {iz}")
        if stages:
            steps[iz] = span / room
        for prob, columns in stages:
            probs.append(prob)
            shifts.append(np.rint(columns / steps[iz]).astype(np.int64) if span > 0 else np.zeros(prob.size, dtype=np.int64))
            tap_offsets.append(tap_offsets[-1] + prob.size)
        stage_offsets.append(stage_offsets[-1] + len(stages))
    probs = np.concatenate(probs) if probs else np.zeros(0)
    shifts = np.concatenate(shifts) if shifts else np.zeros(0, dtype=np.int64)
    args = (probs, shifts, np.array(tap_offsets, dtype=np.int64), np.array(stage_offsets, dtype=np.int64), cells,
            np.array(MIXTURE_LEVELS))
    if mixture is None:
        from .engine import count_mixture
        lower, upper, _ = count_mixture(*args, device=device)
    else:
        lower, upper, _ = mixture(*args)
    lower, upper = (np.asarray(v, dtype=np.float64).reshape(nz, len(MIXTURE_LEVELS)) for v in (lower, upper))
    value = lambda cell: bases + cell * steps     # noqa: E731
    return (value(lower[:, 0]), np.stack([value(lower[:, 1]), value(upper[:, 2])], axis=1),
            np.stack([value(lower[:, 3]), value(upper[:, 4])], axis=1), steps)


def omega_dla_cddf(out, keep=None, p_thresh_spec: float = 0.05, hubble: float = 0.7, omega_m: float = 0.279,
                   levels: str = "first", tail_prob: float = 1e-4, cells: int = 2 ** 20, device: int = 0, pmf=None,
                   mixture=None):
    """Omega_DLA per redshift bin from the column density function, with its 68 % and 95 % Bayesian bands
    (calc_cddf.py:521-560, the curve ``plot_omega_dla`` draws): ``split_distributions_grid`` on the population
    grid of ``out``, ``total_column_intervals`` for the bins with path, and the conversion m_p H_0 / (c rho_crit)
    over the path -- here rho_crit does take ``hubble`` (:542), unlike ``omega_dla``.  ``keep`` is the SNR / z_QSO
    mask, ``levels="all"`` counts every absorber of every multi-DLA level; ``tail_prob``, ``cells``, ``pmf`` and
    ``mixture`` as in ``total_column_intervals``.  Bins without path are dropped (:546).  Returns (bin centres,
    Omega_DLA, 68 % band [n x 2], 95 % band [n x 2], (lower, upper) bin half-widths)."""
    ez = np.asarray(out["population_z_edges"], dtype=np.float64).ravel()
    en = np.asarray(out["population_log_nhi_edges"], dtype=np.float64).ravel()
    lists, means = split_distributions_grid(out, keep, p_thresh_spec, levels)
    dX = _bin_paths(out, "population", ez, keep, omega_m)[0]
    ii = np.flatnonzero(dX > 0)
    mid, l68, l95, _ = total_column_intervals([lists[i] for i in ii], means[ii], en, tail_prob, cells, device, pmf, mixture)
    conversion = PROTON_MASS_G / LIGHT_CM_PER_S * (H100_PER_S * hubble) / rho_crit(hubble)
    cent = (ez[1:] + ez[:-1]) / 2.0
    xerrs = (cent[ii] - ez[:-1][ii], ez[1:][ii] - cent[ii])
    return cent[ii], conversion * mid / dX[ii], conversion * l68 / dX[ii, None], conversion * l95 / dX[ii, None], xerrs


def bootstrap_strata(min_z_dlas, max_z_dlas, num_strata: int = 9, min_per_stratum: int = 10):
    """The redshift strata ``resample`` draws within (calc_cddf.py:139-156), so that a replica keeps the rare
    high-redshift sightlines: ``num_strata + 1`` linearly spaced edges between ``newmin`` and ``newmax`` --
    ``newmax`` from max(max_z) - 0.2 down in steps of 0.2 until ``min_per_stratum`` spectra lie above it,
    ``newmin`` from min(min_z) + 0.2 up in steps of 0.2 while fewer than ``min_per_stratum`` spectra have
    ``max_z <= newmin`` (the reference's own loop, :145, counts ``min_z > newmin`` and cannot end once entered)
    -- the first edge then replaced by min(min_z) and the last by max(max_z), and spectrum q in the stratum with
    ``zm < max_z[q] <= zp``.  Spectra with a NaN range, or a ``max_z`` at or below the first edge, are in none.
    A stratum below ``min_per_stratum`` raises ``ValueError``, as the reference asserts (:153).  Returns CSR:
    (stratum_offsets [num_strata + 1] int64, members int32, ascending within a stratum)."""
    zmin = np.asarray(min_z_dlas, dtype=np.float64).ravel()
    zmax = np.asarray(max_z_dlas, dtype=np.float64).ravel()
    if zmin.size != zmax.size:
        raise ValueError("one search range per spectrum")
    if num_strata < 1 or min_per_stratum < 1:
        raise ValueError("num_strata and min_per_stratum must be positive")
    ok = ~(np.isnan(zmin) | np.isnan(zmax))
    if np.count_nonzero(ok) < min_per_stratum:
        raise ValueError(f"{np.count_nonzero(ok)} spectra with a search range: fewer than min_per_stratum = {min_per_stratum}")
    lo, hi = float(zmin[ok].min()), float(zmax[ok].max())
    with np.errstate(invalid="ignore"):
        newmax = hi - 0.2
        while np.count_nonzero(zmax > newmax) < min_per_stratum:
            newmax -= 0.2
        newmin = lo + 0.2
        while np.count_nonzero(zmax <= newmin) < min_per_stratum:
            newmin += 0.2
        edges = np.linspace(newmin, newmax, num_strata + 1)
        edges[-1], edges[0] = hi, lo
        groups = [np.flatnonzero((zmax > zm) & (zmax <= zp)) for zm, zp in zip(edges[:-1], edges[1:])]
    for s, g in enumerate(groups):
        if g.size < min_per_stratum:
            raise ValueError(f"stratum {s} ({edges[s]:.3f} < max_z <= {edges[s + 1]:.3f}) holds {g.size} spectra: "
                             f"fewer than min_per_stratum = {min_per_stratum}")
    offsets = np.zeros(num_strata + 1, dtype=np.int64)
    np.cumsum([g.size for g in groups], out=offsets[1:])
    return offsets, np.concatenate(groups).astype(np.int32)


def path_columns(z_edges, min_z_dlas, max_z_dlas, keep=None, omega_m: float = 0.279) -> np.ndarray:
    """Every spectrum's own term of ``path_length``, Q x (nz + 1): one column per bin of ``z_edges`` and one for
    its whole range, 0 where the search range misses the interval or ``keep`` is false (no p_dla cut,
    calc_cddf.py:347) -- the same ``absorption_distance`` expressions, so a column's ``fsum`` is ``path_length``."""
    ez = np.asarray(z_edges, dtype=np.float64).ravel()
    zmin = np.asarray(min_z_dlas, dtype=np.float64).ravel()
    zmax = np.asarray(max_z_dlas, dtype=np.float64).ravel()
    kept = np.ones(zmin.size, dtype=bool) if keep is None else np.asarray(keep, dtype=bool).ravel()
    cols = np.zeros((zmin.size, ez.size))
    with np.errstate(invalid="ignore"):
        for c, (z_lo, z_hi) in enumerate(list(zip(ez[:-1], ez[1:])) + [(ez[0], ez[-1])]):
            use = (zmin < z_hi) & (zmax > z_lo) & kept
            hi, lo = np.minimum(z_hi, zmax[use]), np.maximum(z_lo, zmin[use])
            cols[use, c] = absorption_distance(hi, omega_m) - absorption_distance(lo, omega_m)
    return cols


def _first_column(v) -> np.ndarray:
    """MATLAB's x(i) on a Q x D array: column 1."""
    v = np.asarray(v, dtype=np.float64)
    return v.reshape(v.shape[0], -1)[:, 0] if v.ndim > 1 else v


def bootstrap_moments(out, replicas: int, seed, keep=None, strata="auto", levels: str = "first", device: int = 0,
                      sums=None, p_thresh_spec: float = 0.05, omega_m: float = 0.279, first_replica: int = 0) -> dict:
    """``resample`` (calc_cddf.py:126-156) and the sums behind ``line_density`` / ``omega_dla`` for ``replicas``
    bootstrap replicas of the sightlines of ``out`` (``process_qsos(summaries=...)``) at once, on the device: the
    per-spectrum terms of ``cddf_moments`` (``engine.bootstrap_rows``) with the ``path_columns`` appended, then
    the stratified draws and the product counts x rows (``engine.bootstrap``).

    ``seed`` is the 128-bit Philox key; replica r is the same whatever else the call holds.  ``strata`` is
    ``"auto"`` (``bootstrap_strata`` of the search ranges), ``None`` (one stratum of all spectra) or a
    (stratum_offsets, members) pair.  Only full-size replicas are drawn: a stratum draws as many sightlines as
    it holds.  ``levels="all"`` uses ``bin_planes_levels`` with ``model_posteriors[:, 1:1 + D]``.

    ``sums(planes=, p_dlas=, level_posteriors=, keep=, p_thresh_spec=, path=, replicas=, first_replica=, seed=,
    stratum_offsets=, members=)`` replaces the device (tests; it returns the replicas x N sums, N = 4 nz nn +
    nz + 1 in the order means, variance terms, moment means, moment variance terms, path per bin, whole path).

    Returns per replica ``means``, ``variances``, ``moment_means``, ``moment_variances`` (B x nz x nn; what
    ``cddf_moments`` returns), ``path`` (B x nz) and ``path_total`` (B)."""
    from . import engine as E
    all_levels = _check_levels(levels)
    p = np.asarray(out["p_dlas"], dtype=np.float64).ravel()
    zmin, zmax = _first_column(out["min_z_dlas"]), _first_column(out["max_z_dlas"])
    if all_levels:
        planes = np.asarray(out["bin_planes_levels"], dtype=np.float64)
        if planes.ndim == 4:
            planes = planes[:, None]
        P = np.asarray(out["model_posteriors"], dtype=np.float64).reshape(planes.shape[0], -1)[:, 1:1 + planes.shape[1]]
    else:
        planes, P = np.asarray(out["bin_planes"], dtype=np.float64), None
    Q = planes.shape[0]
    nz, nn = planes.shape[-2:]
    nb = nz * nn
    if isinstance(strata, str):
        if strata != "auto":
            raise ValueError("strata must be 'auto', None or (stratum_offsets, members)")
        strata = bootstrap_strata(zmin, zmax)
    so, mem = (np.array([0, Q], dtype=np.int64), np.arange(Q, dtype=np.int32)) if strata is None else strata
    path = cut_path_columns(out, "summary", keep, omega_m)
    if path is None:
        path = path_columns(out["bin_z_edges"], zmin, zmax, keep, omega_m)
    elif path.shape != (Q, nz + 1):
        raise ValueError(f"cut_path_summary must be {(Q, nz + 1)}")
    if sums is not None:
        got = np.asarray(sums(planes=planes, p_dlas=p, level_posteriors=P, keep=keep, p_thresh_spec=p_thresh_spec, path=path,
                              replicas=replicas, first_replica=first_replica, seed=seed, stratum_offsets=so, members=mem),
                         dtype=np.float64)
    else:
        rows = E.bootstrap_rows(planes, p, keep, p_thresh_spec, P, columns=4 * nb + nz + 1, device=device)
        rows[:, 4 * nb:] = path
        got = E.bootstrap(rows, replicas, seed, so, mem, first_replica, device=device)
    if got.shape != (replicas, 4 * nb + nz + 1):
        raise ValueError(f"sums must be {(replicas, 4 * nb + nz + 1)}")
    B = got.shape[0]
    means, moments = got[:, :nb].reshape(B, nz, nn), got[:, 2 * nb:3 * nb].reshape(B, nz, nn)
    return dict(means=means, variances=got[:, nb:2 * nb].reshape(B, nz, nn) + means, moment_means=moments,
                moment_variances=got[:, 3 * nb:4 * nb].reshape(B, nz, nn) + moments,
                path=got[:, 4 * nb:4 * nb + nz].copy(), path_total=got[:, 4 * nb + nz].copy())


def sample_errors(out, replicas: int = 1000, seed=0, keep=None, strata="auto", levels: str = "first", device: int = 0,
                  sums=None, p_thresh_spec: float = 0.05, hubble: float = 0.7, omega_m: float = 0.279) -> dict:
    """``get_sample_errors`` (calc_cddf.py:162-184): the spread of dN/dX and Omega_DLA over bootstrap replicas
    of the sightline sample, per z bin of the summary grid of ``out``.  dN/dX of a replica is
    ``means.sum(-1) / path`` and Omega_DLA the moment estimator of ``omega_dla`` (``moment_means.sum(-1)`` times
    its conversion at the replica's own path; in ``omega_dla``'s units, where the reference multiplies by 1000
    and uses ``omega_dla_cddf``); a replica without path in a bin is NaN there and the percentiles ignore it.
    Bins whose full-sample path is 0 are dropped, as in ``line_density``.

    Returns ``z`` (bin centres), and for ``dndx`` and ``omega`` the reference's five products:
    ``<name>_median`` (``dndx_sample`` / ``omega_sample``), ``<name>_68`` (2 x bins: the 84th and the 16th
    percentile, the reference's order, :179) and ``<name>_95`` (97.5th and 2.5th); also the replica arrays
    ``dndx_replicas`` / ``omega_replicas`` (B x bins).  The arguments are ``bootstrap_moments``'s."""
    import warnings
    bm = bootstrap_moments(out, replicas, seed, keep, strata, levels, device, sums, p_thresh_spec, omega_m)
    ez = np.asarray(out["bin_z_edges"], dtype=np.float64).ravel()
    full = _bin_paths(dict(out, min_z_dlas=_first_column(out["min_z_dlas"]), max_z_dlas=_first_column(out["max_z_dlas"])),
                      "summary", ez, keep, omega_m)[0]
    ii = full > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        dX = np.where(bm["path"] > 0, bm["path"], np.nan)
        dndx = bm["means"].sum(axis=-1) / dX
        conversion = PROTON_MASS_G * (H100_PER_S * hubble) / LIGHT_CM_PER_S / dX / rho_crit()
        omega = bm["moment_means"].sum(axis=-1) * conversion
    res = dict(z=((ez[1:] + ez[:-1]) / 2.0)[ii])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # a bin without path in every replica: all NaN
        for name, v in (("dndx", dndx[:, ii]), ("omega", omega[:, ii])):
            res[f"{name}_median"] = np.nanmedian(v, axis=0)
            res[f"{name}_68"] = np.array((np.nanpercentile(v, 100 - 32 / 2, axis=0), np.nanpercentile(v, 32 / 2, axis=0)))
            res[f"{name}_95"] = np.array((np.nanpercentile(v, 100 - 5 / 2, axis=0), np.nanpercentile(v, 5 / 2, axis=0)))
            res[f"{name}_replicas"] = v
    return res


def search_cuts(preloaded, out, z_edges=None, proximity_zone=0.1, noise_thresh=None, population_z_edges=None,
                omega_m: float = 0.279, device: int = 0) -> dict:
    """``lowzcut`` / ``filter_noisy_pixels`` of every searched spectrum on the device, stand-alone
    (``engine.search_cuts``), in the manner of ``compute_snrs``: ``preloaded`` holds the cells
    ``all_wavelengths`` and ``all_noise_variance`` (converted to float64), ``out`` the ``min_z_dlas`` /
    ``max_z_dlas`` of the searched spectra and, when the cells cover the whole catalogue, ``test_ind``.
    ``z_edges`` / ``population_z_edges`` ask for the path columns of a summary / population grid.  Returns
    ``engine.search_cuts``'s dict."""
    from .engine import search_cuts as device_search_cuts
    zmin, zmax = _first_column(out["min_z_dlas"]), _first_column(out["max_z_dlas"])
    cells = [list(preloaded[k]) for k in ("all_wavelengths", "all_noise_variance")]
    if "test_ind" in out and len(cells[0]) != zmax.size:
        ti = np.asarray(out["test_ind"]).ravel()
        sel = np.flatnonzero(ti) if ti.dtype == bool else ti.astype(np.int64)
        cells = [[c[i] for i in sel] for c in cells]
    if len(cells[0]) != zmax.size:
        raise ValueError("the preloaded cells and max_z_dlas disagree on the number of spectra")
    cells = [[np.asarray(c, dtype=np.float64).ravel() for c in lst] for lst in cells]
    return device_search_cuts(cells[0], cells[1], zmin, zmax, proximity_zone, noise_thresh, z_edges, population_z_edges,
                              omega_m, device)


def compute_snrs(preloaded, out, device: int = 0) -> np.ndarray:
    """``compute_all_snrs`` (calc_cddf.py:959-976): ``find_snr`` of every searched spectrum, on the device
    (``engine.spectrum_snrs``) -- the number behind the ``keep`` masks of the functions above (e.g.
    ``keep = snrs > 4``).  ``preloaded`` holds the cells ``all_wavelengths``, ``all_flux``,
    ``all_noise_variance`` and, if present, ``all_normalizers``; ``out`` the ``max_z_dlas`` of the searched
    spectra and, when the cells cover the whole catalogue, ``test_ind`` (a boolean mask or 0-based indices, as in
    ``write_ascii_catalog``).  float32 cells give float32 SNRs, anything else float64."""
    from .engine import spectrum_snrs
    zmax = _first_column(out["max_z_dlas"])
    cells = [list(preloaded[k]) for k in ("all_wavelengths", "all_flux", "all_noise_variance")]
    norm = preloaded.get("all_normalizers") if hasattr(preloaded, "get") else None
    norm = None if norm is None else np.asarray(norm, dtype=np.float64).ravel()
    if "test_ind" in out and len(cells[0]) != zmax.size:
        ti = np.asarray(out["test_ind"]).ravel()
        sel = np.flatnonzero(ti) if ti.dtype == bool else ti.astype(np.int64)
        cells = [[c[i] for i in sel] for c in cells]
        norm = None if norm is None else norm[sel]
    if len(cells[0]) != zmax.size:
        raise ValueError("the preloaded cells and max_z_dlas disagree on the number of spectra")
    return spectrum_snrs(*cells, zmax, norm, device=device)


def _fmt(spec: str, value) -> str:
    """C / MATLAB fprintf of one number; MATLAB spells the non-finite values NaN, Inf, -Inf."""
    if isinstance(value, (float, np.floating)) and not np.isfinite(value):
        # blank-padded whatever the zero flag says, as C does
        flags, width = re.match(r"%([-+0 ]*)(\d*)", spec).groups()
        text = "NaN" if np.isnan(value) else ("-Inf" if value < 0 else ("+Inf" if "+" in flags else "Inf"))
        return text.ljust(int(width or 0)) if "-" in flags else text.rjust(int(width or 0))
    return spec % value


def _exp3(value: float) -> str:
    """generate_ascii_catalog.m:67-70: %0.5e with a two-digit exponent widened to three."""
    return re.sub(r"e([+-])(\d\d)$", r"e\g<1>0\2", _fmt("%0.5e", float(value)))


def write_ascii_catalog(directory: str, test_set_name: str, catalog: dict, samples: dict, out: dict) -> list:
    """generate_ascii_catalog.m: ``<test_set_name>_dla_samples.dat``, ``_spectra.dat`` and
    ``_results.dat`` in ``directory``, field for field in the reference's formats (including the
    three-digit exponent of the two model posteriors, :67-70).

    ``catalog`` holds the release catalogue's vectors (thing_ids, sdss_names, plates, mjds, fiber_ids,
    ras, decs, z_qsos, snrs, filter_flags), ``samples`` the DLA samples and ``out`` the variables of
    ``process_qsos(..., summaries=...)`` with ``test_ind``.  The MAP pair of the last two columns comes
    from ``MAP_z_dlas`` / ``MAP_log_nhis`` (the first pair of each row: the MAP sample's own DLA), not from
    the sample array, which need not exist; a multi-DLA run's Q x D arrays contribute their first column,
    as MATLAB's linear index ``(i)`` does.

    Line 57 of the reference passes one argument to the two-conversion format ``'%09i %-18s '``.  MATLAB
    stops at the first conversion without data, so a results line starts with the 9-digit thing_id and one
    space, and no name; this does the same.  Returns the three paths."""
    os.makedirs(directory, exist_ok=True)
    paths = [os.path.join(directory, f"{test_set_name}_{kind}.dat") for kind in ("dla_samples", "spectra", "results")]
    off = np.asarray(samples["offset_samples"], dtype=np.float64).ravel()
    lognhi = np.asarray(samples["log_nhi_samples"], dtype=np.float64).ravel()
    with open(paths[0], "w") as f:
        for o, n in zip(off, lognhi):
            f.write(_fmt("%06f", o) + " " + _fmt("%09f", n) + "\n")

    def col(key, dtype=np.float64):
        return np.asarray(catalog[key], dtype=dtype).ravel()
    thing_ids, plates, mjds, fibers = (col(k, np.int64) for k in ("thing_ids", "plates", "mjds", "fiber_ids"))
    flags = col("filter_flags", np.int64)
    ras, decs, z_qsos, snrs = (col(k) for k in ("ras", "decs", "z_qsos", "snrs"))
    names = [str(s).rstrip() for s in np.asarray(catalog["sdss_names"], dtype=object).ravel()]
    with open(paths[1], "w") as f:
        for i in range(z_qsos.size):
            f.write("%09d %-18s %04d %05d %04d " % (thing_ids[i], names[i], plates[i], mjds[i], fibers[i]) +
                    " ".join([_fmt("%011.7f", ras[i]), _fmt("%+011.7f", decs[i]), _fmt("%06.4f", z_qsos[i]),
                              _fmt("%08.4f", snrs[i])]) +
                    " %d%d%d%d\n" % tuple((int(flags[i]) >> b) & 1 for b in range(4)))

    ti = np.asarray(out["test_ind"]).ravel()
    searched = np.flatnonzero(ti) if ti.dtype == bool else ti.astype(np.int64)

    def first(key):    # MATLAB's x(i) on a Q x D array: column 1
        v = np.asarray(out[key], dtype=np.float64)
        return v.reshape(v.shape[0], -1)[:, 0] if v.ndim > 1 else v
    zmin, zmax, lp_no, lp_dla, ll_no, ll_dla = (first(k) for k in (
        "min_z_dlas", "max_z_dlas", "log_priors_no_dla", "log_priors_dla", "log_likelihoods_no_dla",
        "log_likelihoods_dla"))
    post = np.asarray(out["model_posteriors"], dtype=np.float64)
    map_z, map_n = first("MAP_z_dlas"), first("MAP_log_nhis")
    with open(paths[2], "w") as f:
        for i, ci in enumerate(searched):
            f.write("%09d " % thing_ids[ci])
            f.write(" ".join([_fmt("%06.4f", zmin[i]), _fmt("%06.4f", zmax[i]), _fmt("%8.5f", lp_no[i]),
                              _fmt("%8.5f", lp_dla[i]), _fmt("%12.5e", ll_no[i]), _fmt("%12.5e", ll_dla[i]),
                              _exp3(post[i, 0]), _exp3(post[i, 1])]) + " ")
            f.write(_fmt("%06.4f", map_z[i]) + " " + _fmt("%07.4f", map_n[i]) + "\n")
    return paths


# ------------------------------------------------------------------------------- posterior intervals
def _interval_array(out, key, tail_dims: int) -> np.ndarray:
    """An INTERVAL_VARIABLES array of ``process_qsos(intervals=...)``, or of its file as ``matv73.loadmat`` reads it
    back: Q x D x 4 and ``tail_dims`` further axes."""
    if key not in out:
        raise ValueError(f"the run has no {key}: process_qsos(intervals=...) writes it")
    v = np.asarray(out[key], dtype=np.float64)
    if v.ndim != 3 + tail_dims or v.shape[2] != 4:
        raise ValueError(f"{key} must be Q x D x 4" + " x n" * tail_dims)
    return v


def find_delta_nhi(out) -> np.ndarray:
    """DLACatalogue.find_delta_NHI (calc_cddf.py:872-878) per searched spectrum: the range of log N_HI over the
    samples of the first DLA model whose likelihood is within e^-lr_delta of the maximum -- hi - lo of level 1,
    slot 0 of ``log_nhi_lr_ranges`` (NaN for a spectrum without such a sample)."""
    r = _interval_array(out, "log_nhi_lr_ranges", 1)
    return r[:, 0, 0, 1] - r[:, 0, 0, 0]


def find_delta_z(out) -> np.ndarray:
    """DLACatalogue.find_delta_z (calc_cddf.py:880-886): the same for z_DLA, from ``z_dla_lr_ranges``."""
    r = _interval_array(out, "z_dla_lr_ranges", 1)
    return r[:, 0, 0, 1] - r[:, 0, 0, 0]


ABSORBER_FIELDS = ("spectrum", "level", "absorber", "map_z_dla", "map_log_nhi", "z_dla_mean", "z_dla_sd",
                   "log_nhi_mean", "log_nhi_sd", "z_dla_lr_lo", "z_dla_lr_hi", "log_nhi_lr_lo", "log_nhi_lr_hi")


def absorber_table(out) -> dict:
    """One record per (spectrum, absorber) of each spectrum's best DLA level -- the level d with the highest
    model posterior, as ``MAP_z_dlas`` takes it, giving d records -- as a dict of equal-length columns:

    ``spectrum`` (0-based row of the run), ``level`` (d, 1-based), ``absorber`` (slot, 0 = the sample's own),
    ``map_z_dla`` / ``map_log_nhi`` (the MAP pair), ``z_dla_quantiles`` / ``log_nhi_quantiles`` (records x L, at
    ``interval_levels``, also returned), ``z_dla_mean`` / ``_sd``, ``log_nhi_mean`` / ``_sd`` and the
    likelihood-ratio ranges ``z_dla_lr_lo`` / ``_hi``, ``log_nhi_lr_lo`` / ``_hi``.  ``out`` holds the variables
    of ``process_qsos(..., intervals=...)``."""
    zq, nq = _interval_array(out, "z_dla_quantiles", 1), _interval_array(out, "log_nhi_quantiles", 1)
    Q, D = zq.shape[:2]
    post = np.asarray(out["model_posteriors"], dtype=np.float64).reshape(Q, -1)[:, 1:1 + D]
    level = np.argmax(np.where(np.isnan(post), -np.inf, post), axis=1) if Q else np.zeros(0, dtype=np.int64)
    map_z = np.asarray(out["MAP_z_dlas"], dtype=np.float64).reshape(Q, -1)
    map_n = np.asarray(out["MAP_log_nhis"], dtype=np.float64).reshape(Q, -1)
    q = np.repeat(np.arange(Q), level + 1)
    u = np.concatenate([np.arange(d + 1) for d in level]) if Q else np.zeros(0, dtype=np.int64)
    d = level[q]
    pick = lambda key, tail: _interval_array(out, key, tail)[q, d, u]   # noqa: E731
    zr, nr = pick("z_dla_lr_ranges", 1), pick("log_nhi_lr_ranges", 1)
    return dict(spectrum=q, level=d + 1, absorber=u, map_z_dla=map_z[q, u], map_log_nhi=map_n[q, u],
                z_dla_quantiles=zq[q, d, u], log_nhi_quantiles=nq[q, d, u],
                z_dla_mean=pick("z_dla_means", 0), z_dla_sd=pick("z_dla_sds", 0),
                log_nhi_mean=pick("log_nhi_means", 0), log_nhi_sd=pick("log_nhi_sds", 0),
                z_dla_lr_lo=zr[:, 0], z_dla_lr_hi=zr[:, 1], log_nhi_lr_lo=nr[:, 0], log_nhi_lr_hi=nr[:, 1],
                interval_levels=np.asarray(out["interval_levels"], dtype=np.float64).ravel())


def write_absorber_catalog(directory: str, test_set_name: str, catalog: dict, out: dict) -> str:
    """``<test_set_name>_absorbers.dat`` in ``directory``: ``absorber_table(out)`` with one line per record --
    the 9-digit thing_id (``catalog['thing_ids']`` at ``out['test_ind']``, as ``write_ascii_catalog`` resolves
    it), level and absorber slot (1-based), the MAP pair, then for z_DLA and log N_HI in turn the quantiles in
    level order, mean, sd and the likelihood-ratio range; a header line names the columns.  z in %06.4f and
    log N_HI in %07.4f like the results file, the sds in %.4e.  Returns the path."""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, f"{test_set_name}_absorbers.dat")
    t = absorber_table(out)
    thing_ids = np.asarray(catalog["thing_ids"], dtype=np.int64).ravel()
    ti = np.asarray(out["test_ind"]).ravel()
    searched = np.flatnonzero(ti) if ti.dtype == bool else ti.astype(np.int64)
    levels = t["interval_levels"]
    names = ["thing_id", "level", "absorber", "map_z_dla", "map_log_nhi"]
    for prefix in ("z_dla", "log_nhi"):
        names += [f"{prefix}_q{lv:g}" for lv in levels] + [f"{prefix}_mean", f"{prefix}_sd", f"{prefix}_lr_lo", f"{prefix}_lr_hi"]
    with open(path, "w") as f:
        f.write("# " + " ".join(names) + "\n")
        for i in range(t["spectrum"].size):
            f.write("%09d %d %d " % (thing_ids[searched[t["spectrum"][i]]], t["level"][i], t["absorber"][i] + 1))
            fields = [_fmt("%06.4f", t["map_z_dla"][i]), _fmt("%07.4f", t["map_log_nhi"][i])]
            for prefix, spec in (("z_dla", "%06.4f"), ("log_nhi", "%07.4f")):
                fields += [_fmt(spec, v) for v in t[prefix + "_quantiles"][i]]
                fields += [_fmt(spec, t[prefix + "_mean"][i]), _fmt("%.4e", t[prefix + "_sd"][i]),
                           _fmt(spec, t[prefix + "_lr_lo"][i]), _fmt(spec, t[prefix + "_lr_hi"][i])]
            f.write(" ".join(fields) + "\n")
    return path


# ------------------------------------------------------------------------------------------ model spectra
# what Engine.model_spectra returns, under the names an output dictionary carries them by
MODEL_SPECTRA_KEYS = dict(offsets="model_offsets", pixel_inds="model_pixel_inds", absorption="model_absorption",
                          model_mean="model_mean", continuum="model_continuum", continuum_sd="model_continuum_sd",
                          log_likelihoods="model_log_likelihoods", chi2="model_chi2", num_pixels="model_num_pixels")


def model_spectra_variables(result: dict) -> dict:
    """``Engine.model_spectra``'s result under the ``model_*`` names the helpers below read."""
    return {new: result[old] for old, new in MODEL_SPECTRA_KEYS.items()}


def model_spectrum(out: dict, q: int, wavelengths=None) -> dict:
    """Spectrum ``q``'s slices of the flat ``model_*`` arrays: ``pixel_inds`` (within the spectrum), ``absorption``,
    ``model_mean``, ``continuum``, ``continuum_sd``, the posterior absorbed fit ``fit`` = absorption * continuum,
    the scalars ``chi2``, ``log_likelihood``, ``num_pixels`` and, with the spectrum's own ``wavelengths``, those at
    ``pixel_inds``."""
    off = np.asarray(out["model_offsets"], dtype=np.int64)
    if not 0 <= q < off.size - 1:
        raise IndexError(f"spectrum {q} outside 0..{off.size - 2}")
    sl = slice(int(off[q]), int(off[q + 1]))
    r = dict(pixel_inds=np.asarray(out["model_pixel_inds"])[sl], absorption=np.asarray(out["model_absorption"])[sl],
             model_mean=np.asarray(out["model_mean"])[sl], continuum=np.asarray(out["model_continuum"])[sl],
             continuum_sd=np.asarray(out["model_continuum_sd"])[sl], chi2=float(np.asarray(out["model_chi2"])[q]),
             log_likelihood=float(np.asarray(out["model_log_likelihoods"])[q]),
             num_pixels=int(np.asarray(out["model_num_pixels"])[q]))
    r["fit"] = r["absorption"] * r["continuum"]
    if wavelengths is not None:
        r["wavelengths"] = np.asarray(wavelengths, dtype=np.float64)[r["pixel_inds"]]
    return r


def dla_pixel_mask(out: dict, min_transmission: float = 0.8) -> np.ndarray:
    """Flat bool array over the ``model_*`` pixels: True where the absorbers transmit less than
    ``min_transmission`` (the cores a Lyman-alpha forest analysis masks).  NaN absorption is not masked."""
    if not 0.0 <= min_transmission <= 1.0:
        raise ValueError("min_transmission must lie in [0, 1]")
    with np.errstate(invalid="ignore"):
        return np.asarray(out["model_absorption"], dtype=np.float64) < min_transmission


def wing_correction(out: dict, min_transmission: float = 0.8) -> np.ndarray:
    """1 / absorption where ``dla_pixel_mask`` is False (the factor that divides the damping wings out of the
    flux), NaN where it is True."""
    a = np.asarray(out["model_absorption"], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(dla_pixel_mask(out, min_transmission), np.nan, 1.0 / a)


def fit_quality(out: dict) -> dict:
    """Per spectrum ``reduced_chi2`` = chi2 / n and ``z_score`` = (chi2 - n) / sqrt(2 n): under the model chi2 =
    r'K^-1 r is chi-squared with n degrees of freedom (mean n, variance 2 n), so z_score is its standardised
    residual -- near 0 for a sightline the model describes, many units above it for one it cannot (a BAL, a bad
    reduction).  NaN for a spectrum without pixels."""
    chi2 = np.asarray(out["model_chi2"], dtype=np.float64)
    n = np.asarray(out["model_num_pixels"], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(reduced_chi2=np.where(n > 0, chi2 / n, np.nan),
                    z_score=np.where(n > 0, (chi2 - n) / np.sqrt(2 * n), np.nan))

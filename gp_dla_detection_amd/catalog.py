"""The last stage after ``process_qsos``: the ASCII DLA catalogue (generate_ascii_catalog.m) and the
binned population moments (CDDF_analysis/calc_cddf.py ``_get_z_nhi_hist``), both from the posterior
summaries the engine reduces on the device (``Engine.process_summaries``, ``process_qsos(summaries=...)``)
instead of the Q x S sample array."""
from __future__ import annotations

import os
import re

import numpy as np

# bin_planes' second axis (include/gpdla.h GPDLA_SUMMARY_PLANES)
PLANE_PI, PLANE_PI2, PLANE_NPI, PLANE_N2PI, PLANE_N2PI2 = range(5)


def cddf_moments(bin_planes, p_dlas, keep=None, p_thresh_spec: float = 0.05, moment: bool = False):
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
    other axis (dN/dX and Omega_DLA over log N_HI, the CDDF over z)."""
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

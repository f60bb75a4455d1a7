"""Python handle on the native engine (``gpdla_engine_*`` in include/gpdla.h)."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import _lib as L
from .parameters import Parameters, set_parameters


def _model_struct(model: dict, keep: list) -> L.Model:
    lam = np.ascontiguousarray(model["rest_wavelengths"], dtype=np.float64).ravel()
    mu = np.ascontiguousarray(model["mu"], dtype=np.float64).ravel()
    M = np.asfortranarray(model["M"], dtype=np.float64)
    lom = np.ascontiguousarray(model["log_omega"], dtype=np.float64).ravel()
    if M.shape[0] != lam.size or mu.size != lam.size or lom.size != lam.size:
        raise ValueError("model arrays disagree on the rest-grid size")
    Mflat = M.ravel(order="F")  # MATLAB column-major
    keep += [lam, mu, Mflat, lom]
    return L.Model(num_rest=lam.size, k=M.shape[1], rest_wavelengths=L.ptr(lam), mu=L.ptr(mu),
                   M=L.ptr(Mflat), log_omega=L.ptr(lom), log_c_0=float(np.ravel(model["log_c_0"])[0]),
                   log_tau_0=float(np.ravel(model["log_tau_0"])[0]),
                   log_beta=float(np.ravel(model["log_beta"])[0]))


_PATHS = {"auto": L.PATH_AUTO, "fused": L.PATH_FUSED, "panel_gemm": L.PATH_PANEL_GEMM,
          "fused_i8": L.PATH_FUSED_I8, "panel_gemm_i8": L.PATH_PANEL_GEMM_I8,
          "panel_gemm_i8_24": L.PATH_PANEL_GEMM_I8_24}


# what the forest's mean flux multiplies -> the scope code of gpdla_engine_set_forest_scoped
MEAN_FLUX_SCOPES = {"mu": 0, "mu_M": 1, "all": 2}


def mean_flux_scope_code(scope, mean_flux) -> int:
    """The code of a ``mean_flux_scope`` name; ValueError for an unknown name and for a scope other than
    "mu" without ``mean_flux`` (there is no mean flux to multiply by)."""
    if not isinstance(scope, str) or scope not in MEAN_FLUX_SCOPES:
        raise ValueError(f"mean_flux_scope must be one of {list(MEAN_FLUX_SCOPES)}, not {scope!r}")
    if scope != "mu" and not mean_flux:
        raise ValueError(f"mean_flux_scope={scope!r} needs mean_flux=True")
    return MEAN_FLUX_SCOPES[scope]


def _params_struct(p: Parameters, max_batch_spectra: int = 0, path: str = "auto") -> L.Params:
    return L.Params(num_lines=p.num_lines, width=p.width, pixel_spacing=p.pixel_spacing,
                    min_lambda=p.min_lambda, max_lambda=p.max_lambda,
                    lya_wavelength=p.lya_wavelength, lyman_limit=p.lyman_limit,
                    min_z_cut=p.min_z_cut, max_z_cut=p.max_z_cut,
                    absorption_mode=(L.ABSORPTION_REFERENCE if p.absorption_mode == "reference"
                                     else L.ABSORPTION_UNMASKED),
                    max_batch_spectra=max_batch_spectra, path=_PATHS[path])


# relative guard band of model_capacities' rest-wavelength test: far above the rounding of lambda / (1 + z)
# (a few 1e-16), far below a pixel (2.3e-4)
MODEL_CAPACITY_GUARD = 1e-12


def model_capacities(packed: dict, params: Parameters) -> np.ndarray:
    """An upper bound [Q] on each spectrum's likelihood pixels: its pixels with min_lambda (1 - g) <= lambda /
    (1 + z_qso) <= max_lambda (1 + g), g = MODEL_CAPACITY_GUARD, the mask ignored.  The device's own test is
    the same without the guard band, so however the division rounds, n <= capacity."""
    offsets = np.asarray(packed["offsets"], dtype=np.int64)
    wl = np.asarray(packed["wavelengths"], dtype=np.float64)
    zq = np.asarray(packed["z_qsos"], dtype=np.float64)
    caps = np.zeros(offsets.size - 1, dtype=np.int64)
    lo, hi = params.min_lambda * (1 - MODEL_CAPACITY_GUARD), params.max_lambda * (1 + MODEL_CAPACITY_GUARD)
    for q in range(caps.size):
        rest = wl[offsets[q]:offsets[q + 1]] / (1 + zq[q])
        caps[q] = np.count_nonzero((rest >= lo) & (rest <= hi))
    return caps


def _absorber_arrays(Q: int, z_dlas, log_nhis, counts):
    """[Q][4] NaN-padded z and log N_HI and the int32 counts of Engine.model_spectra; ValueError for a shape that
    does not fit or a count outside 0..4."""
    z, n = np.asarray(z_dlas, dtype=np.float64), np.asarray(log_nhis, dtype=np.float64)
    z = z.reshape(Q, -1) if z.size else np.zeros((Q, 0))
    n = n.reshape(Q, -1) if n.size else np.zeros((Q, 0))
    if z.shape != n.shape or z.shape[1] > L.MAX_DLAS:
        raise ValueError(f"z_dlas and log_nhis must both be [Q][<= {L.MAX_DLAS}]")
    z4, n4 = np.full((Q, L.MAX_DLAS), np.nan), np.full((Q, L.MAX_DLAS), np.nan)
    z4[:, :z.shape[1]] = z
    n4[:, :n.shape[1]] = n
    if counts is None:
        ok = np.isfinite(z4) & np.isfinite(n4)
        cnt = np.where(ok.all(axis=1), L.MAX_DLAS, np.argmin(ok, axis=1)).astype(np.int32)
    else:
        cnt = np.ascontiguousarray(counts, dtype=np.int32).ravel()
        if cnt.size != Q or np.any(cnt < 0) or np.any(cnt > np.minimum(L.MAX_DLAS, max(z.shape[1], 0))):
            raise ValueError(f"counts must be Q integers in 0..{L.MAX_DLAS} and within the rows given")
    return z4, n4, cnt


def compact_model_spectra(cap_offsets, num_pixels, pixel_inds, arrays: dict) -> dict:
    """The capacity-CSR of gpdla_engine_model_spectra squeezed to n_q values per spectrum: ``offsets`` [Q + 1]
    and every flat array with its first num_pixels[q] values of each spectrum's stretch."""
    npix = np.asarray(num_pixels, dtype=np.int64)
    off = np.zeros(npix.size + 1, dtype=np.int64)
    np.cumsum(npix, out=off[1:])
    take = np.concatenate([cap_offsets[q] + np.arange(npix[q]) for q in range(npix.size)] or
                          [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    out = dict(offsets=off, pixel_inds=np.asarray(pixel_inds)[take])
    for key, arr in arrays.items():
        out[key] = np.asarray(arr)[take]
    return out


def host_empty(shape: tuple, dtype=np.float64) -> np.ndarray:
    """An uninitialised host array for outputs the engine writes in full: the 13 GB full-DR12Q Q x S
    sample array is not NaN-filled first (a whole extra pass over it; the D2H copies touch each page
    once).  From 256 MB up it is an anonymous map advised for transparent huge pages where the host
    enables them (fewer first-touch faults)."""
    import math
    import mmap
    nbytes = math.prod(shape) * np.dtype(dtype).itemsize
    if nbytes < (1 << 28):
        return np.empty(shape, dtype=dtype)
    m = mmap.mmap(-1, nbytes, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
    try:
        m.madvise(mmap.MADV_HUGEPAGE)
    except (AttributeError, OSError):  # no THP on this host: plain pages
        pass
    return np.frombuffer(m, dtype=dtype).reshape(shape)


class Engine:
    """One engine per device: resident model, DLA samples and line-profile tables.

    ``path``: "auto" (fused single-kernel sweep for ranks 1..24 -- compiled for 4 8 10 12 16 20 24, a
    rank in between runs on the next one with M zero-padded, exactly -- else the panel-GEMM path),
    "fused", or "panel_gemm" (weights kernel + dgemm + batched LDL^T; ranks 1..64)."""

    def __init__(self, model: dict, samples: dict, params: Parameters | None = None,
                 device: int = 0, max_batch_spectra: int = 0, path: str = "auto"):
        self.lib = L.load()
        self.params = params or set_parameters(k=np.asarray(model["M"]).shape[1])
        if self.params.k != np.asarray(model["M"]).shape[1]:
            raise ValueError("params.k disagrees with the model's M")
        keep: list = []
        ms = _model_struct(model, keep)
        off = np.ascontiguousarray(samples["offset_samples"], dtype=np.float64).ravel()
        nhi = np.ascontiguousarray(samples["nhi_samples"], dtype=np.float64).ravel()
        if off.size != nhi.size:
            raise ValueError("offset_samples and nhi_samples differ in length")
        ss = L.Samples(num_samples=off.size, offset_samples=L.ptr(off), nhi_samples=L.ptr(nhi))
        if path not in _PATHS:
            raise ValueError(f"path must be one of {sorted(_PATHS)}")
        ps = _params_struct(self.params, max_batch_spectra, path)
        h = C.c_void_p()
        L.check(self.lib.gpdla_engine_create(device, C.byref(ms), C.byref(ss), C.byref(ps), C.byref(h)))
        self._h = h
        self.num_samples = off.size
        self.device = device

    # -------------------------------------------------------------------------------- host path
    def process(self, packed: dict, want_samples: bool = True, raise_numeric: bool = False,
                timings: dict | None = None) -> dict:
        """Run the hot path on CSR-packed host spectra (see synthetic.pack_spectra).  ``timings``
        (optional) receives the host output allocation and the engine call times."""
        t0 = time.perf_counter()
        offsets = np.ascontiguousarray(packed["offsets"], dtype=np.int64)
        Q = offsets.size - 1
        wl = np.ascontiguousarray(packed["wavelengths"], dtype=np.float64)
        fl = np.ascontiguousarray(packed["flux"], dtype=np.float64)
        nv = np.ascontiguousarray(packed["noise_variance"], dtype=np.float64)
        mk = np.ascontiguousarray(packed["pixel_mask"], dtype=np.uint8)
        zq = np.ascontiguousarray(packed["z_qsos"], dtype=np.float64)
        if not (wl.size == fl.size == nv.size == mk.size and offsets[-1] <= wl.size and zq.size == Q):
            raise ValueError("inconsistent spectra arrays")
        out = dict(log_likelihoods_no_dla=np.full(Q, np.nan), log_likelihoods_dla=np.full(Q, np.nan),
                   min_z_dlas=np.full(Q, np.nan), max_z_dlas=np.full(Q, np.nan),
                   num_pixels=np.zeros(Q, dtype=np.int32))
        if want_samples:  # every row is written by the engine (NaN rows for unusable spectra)
            out["sample_log_likelihoods_dla"] = host_empty((Q, self.num_samples))
        sp = L.Spectra(memory=L.MEM_HOST, num_spectra=Q, offsets=L.ptr(offsets, C.c_int64),
                       wavelengths=L.ptr(wl), flux=L.ptr(fl), noise_variance=L.ptr(nv),
                       pixel_mask=L.ptr(mk, C.c_uint8), z_qsos=L.ptr(zq))
        sll = out.get("sample_log_likelihoods_dla")
        rs = L.Results(memory=L.MEM_HOST, log_likelihoods_no_dla=L.ptr(out["log_likelihoods_no_dla"]),
                       sample_log_likelihoods_dla=L.ptr(sll), sample_ld=self.num_samples,
                       log_likelihoods_dla=L.ptr(out["log_likelihoods_dla"]),
                       min_z_dlas=L.ptr(out["min_z_dlas"]), max_z_dlas=L.ptr(out["max_z_dlas"]),
                       num_pixels=L.ptr(out["num_pixels"], C.c_int32))
        t1 = time.perf_counter()
        rc = self.lib.gpdla_engine_process(self._h, C.byref(sp), C.byref(rs))
        if timings is not None:
            timings["host_alloc_s"] = t1 - t0
            timings["engine_process_s"] = time.perf_counter() - t1
        if rc == L.GPDLA_ENUMERIC and not raise_numeric:
            out["numeric_warning"] = self.lib.gpdla_last_error().decode()
        else:
            L.check(rc)
        return out

    # ------------------------------------------------------------------------------ multi-DLA
    def default_resample_uniforms(self, max_dlas: int) -> np.ndarray:
        """The (max_dlas - 1) x S uniforms of the level resamplers when the caller gives none: the
        RR2-scrambled Halton dimensions after the samples' own bases 2 and 3, from point 1."""
        from .dla_samples import halton_rr2
        if max_dlas <= 1:
            return np.zeros((0, self.num_samples))
        pts = halton_rr2(self.num_samples, bases=(5, 7, 11)[:max_dlas - 1], start=1, device=self.device)
        return np.ascontiguousarray(pts.T)

    def process_multi(self, packed: dict, max_dlas: int, resample_uniforms=None, base_sample_inds=None,
                      want_samples: bool = True, min_z_separation: float | None = None,
                      occam_log_penalty: float | None = None, raise_numeric: bool = False,
                      memory: str = "host") -> dict:
        """The multi-DLA search (gpdla_engine_process_multi): up to ``max_dlas`` (1..4) DLAs per
        sightline on the fused fp64 path.  Level d's sample j carries its own DLA and those of the base
        sample drawn for it from the level-(d-1) posterior with ``resample_uniforms[d-2, j]``
        ((max_dlas - 1) x S in [0, 1); default ``default_resample_uniforms``).  ``base_sample_inds``
        ((max_dlas - 1) x Q x S, 0-based, -1 = none) replaces the resampler (tests, replaying a saved run).
        Returns ``log_likelihoods_dla`` (D x Q), ``sample_log_likelihoods_dla`` (D x Q x S),
        ``base_sample_inds`` ((D - 1) x Q x S int32, -1 = none) and the per-spectrum vectors of
        ``process``.  ``memory="device"`` routes inputs and results through device buffers (same values)."""
        return self._run_multi(packed, max_dlas, resample_uniforms, base_sample_inds, want_samples,
                               min_z_separation, occam_log_penalty, raise_numeric, memory, None)

    def process_summaries(self, packed: dict, max_dlas: int, log_nhi_samples, z_edges=None, log_nhi_edges=None,
                          want_samples: bool = False, **kwargs) -> dict:
        """``process_multi`` (its keyword arguments pass through; ``max_dlas`` 1..4) with the posterior
        summaries reduced on the device (gpdla_engine_process_summaries), so the D x Q x S sample array need
        not leave it (``want_samples=False``, the default here).  ``log_nhi_samples`` are the engine's
        samples' log10 N_HI.  Besides ``process_multi``'s arrays:

        ``map_sample_inds`` (D x Q int32)  first maximum over the non-NaN samples of each level, -1 = none
        ``map_log_likelihoods`` (D x Q)    that maximum (NaN)
        ``MAP_z_dlas`` / ``MAP_log_nhis`` (D x Q x D)  level d's d (z_DLA, log N_HI) pairs: the MAP sample's
                                           own, then its base chain's; unused slots NaN
        ``bin_planes`` (Q x 5 x nz x nn)   with ``z_edges`` (nz + 1) and ``log_nhi_edges`` (nn + 1): the
                                           level-1 normalised sample masses summed per bin as sum pi, pi^2,
                                           N pi, N^2 pi, N^2 pi^2 (``catalog.cddf_moments`` consumes them)
        Repeated calls and any ``max_batch_spectra`` give bitwise equal summaries."""
        if (z_edges is None) != (log_nhi_edges is None):
            raise ValueError("z_edges and log_nhi_edges go together")
        lognhi = np.ascontiguousarray(log_nhi_samples, dtype=np.float64).ravel()
        if lognhi.size != self.num_samples:
            raise ValueError("one log_nhi sample per engine sample")
        summary = dict(log_nhi=lognhi,
                       z_edges=None if z_edges is None else np.ascontiguousarray(z_edges, dtype=np.float64).ravel(),
                       n_edges=None if log_nhi_edges is None else np.ascontiguousarray(log_nhi_edges, dtype=np.float64).ravel())
        order = ("resample_uniforms", "base_sample_inds", "min_z_separation", "occam_log_penalty", "raise_numeric", "memory")
        unknown = set(kwargs) - set(order)
        if unknown:
            raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
        return self._run_multi(packed, max_dlas, kwargs.get("resample_uniforms"), kwargs.get("base_sample_inds"),
                               want_samples, kwargs.get("min_z_separation"), kwargs.get("occam_log_penalty"),
                               kwargs.get("raise_numeric", False), kwargs.get("memory", "host"), summary)

    def process_intervals(self, packed: dict, max_dlas: int, log_nhi_samples, levels=None, lr_delta: float = 2.0,
                          z_edges=None, log_nhi_edges=None, want_samples: bool = False, **kwargs) -> dict:
        """``process_summaries`` (same arguments, same outputs bit for bit) with the posterior intervals of
        every absorber of every level reduced on the device as well (gpdla_engine_process_intervals).
        ``levels`` are up to 8 quantile levels strictly inside (0, 1), increasing (default
        ``DEFAULT_INTERVAL_LEVELS``); ``lr_delta`` > 0 the likelihood-ratio depth.  Besides the summaries, with
        L = len(levels) and slot u of level d its u-th absorber (own first, then the base chain's):

        ``z_dla_quantiles`` / ``log_nhi_quantiles`` (D x Q x D x L)  the smallest slot value whose cumulative
                                           posterior mass reaches level x total: bitwise a sample value
        ``z_dla_means`` / ``_sds``, ``log_nhi_means`` / ``_sds`` (D x Q x D)  posterior mean and sd
        ``z_dla_lr_ranges`` / ``log_nhi_lr_ranges`` (D x Q x D x 2)  min and max over the samples with
                                           l > max l - lr_delta; ``lr_counts`` (D x Q int32) how many those are
        ``interval_levels`` (L), ``lr_delta``  the arguments as used
        Unused slots, and rows without a usable weight sum, are NaN (count 0).  Repeated calls, any
        ``max_batch_spectra`` and either ``memory`` give bitwise equal results."""
        if (z_edges is None) != (log_nhi_edges is None):
            raise ValueError("z_edges and log_nhi_edges go together")
        lognhi = np.ascontiguousarray(log_nhi_samples, dtype=np.float64).ravel()
        if lognhi.size != self.num_samples:
            raise ValueError("one log_nhi sample per engine sample")
        summary = dict(log_nhi=lognhi,
                       z_edges=None if z_edges is None else np.ascontiguousarray(z_edges, dtype=np.float64).ravel(),
                       n_edges=None if log_nhi_edges is None else np.ascontiguousarray(log_nhi_edges, dtype=np.float64).ravel())
        order = ("resample_uniforms", "base_sample_inds", "min_z_separation", "occam_log_penalty", "raise_numeric", "memory")
        unknown = set(kwargs) - set(order)
        if unknown:
            raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
        intervals = dict(log_nhi=lognhi, levels=_interval_levels(levels), lr_delta=float(lr_delta))
        return self._run_multi(packed, max_dlas, kwargs.get("resample_uniforms"), kwargs.get("base_sample_inds"),
                               want_samples, kwargs.get("min_z_separation"), kwargs.get("occam_log_penalty"),
                               kwargs.get("raise_numeric", False), kwargs.get("memory", "host"), summary,
                               intervals=intervals)

    def interval_stats(self) -> dict:
        """gpdla_engine_get_interval_stats: cumulative ms and count of the interval launches."""
        ms, n = C.c_double(0.0), C.c_int64(0)
        L.check(self.lib.gpdla_engine_get_interval_stats(self._h, C.byref(ms), C.byref(n)))
        return dict(interval_ms=ms.value, interval_launches=n.value)

    def summary_stats(self) -> dict:
        """gpdla_engine_get_summary_stats: cumulative ms and count of the summary launches."""
        ms, n = C.c_double(0.0), C.c_int64(0)
        L.check(self.lib.gpdla_engine_get_summary_stats(self._h, C.byref(ms), C.byref(n)))
        return dict(summary_ms=ms.value, summary_launches=n.value)

    def _run_multi(self, packed, max_dlas, resample_uniforms, base_sample_inds, want_samples, min_z_separation,
                   occam_log_penalty, raise_numeric, memory, summary, sub=None, models=False, population=None,
                   levels=None, intervals=None, cuts=None, model_spectra=None) -> dict:
        """process_multi / process_summaries / process_models / process_population: ``summary`` is None or
        the samples' log N_HI and the grid; ``sub`` None or the sub-DLA column densities (``nhi``) and, for the
        MAP outputs, their log10 (``log_nhi``); ``models`` routes the call through gpdla_engine_process_models,
        ``models="population"`` through gpdla_engine_process_population with ``population`` None (both structs
        NULL) or the normalised dict of ``process_population``; ``levels`` (with ``models="population"``) routes
        it through gpdla_engine_process_levels with the halves it names ("planes", "split"); ``intervals`` (with
        ``summary`` alone) routes it through gpdla_engine_process_intervals: the samples' log N_HI, ``levels`` and
        ``lr_delta``; ``cuts`` (with ``models="population"``) routes it through gpdla_engine_process_cuts: the
        normalised dict of ``process_cuts``."""
        D, S = int(max_dlas), self.num_samples
        offsets = np.ascontiguousarray(packed["offsets"], dtype=np.int64)
        Q = offsets.size - 1
        wl = np.ascontiguousarray(packed["wavelengths"], dtype=np.float64)
        fl = np.ascontiguousarray(packed["flux"], dtype=np.float64)
        nv = np.ascontiguousarray(packed["noise_variance"], dtype=np.float64)
        mk = np.ascontiguousarray(packed["pixel_mask"], dtype=np.uint8)
        zq = np.ascontiguousarray(packed["z_qsos"], dtype=np.float64)
        if not (wl.size == fl.size == nv.size == mk.size and offsets[-1] <= wl.size and zq.size == Q):
            raise ValueError("inconsistent spectra arrays")
        Dc = min(max(D, 1), L.MAX_DLAS)   # array sizes for an out-of-range D (the library rejects it)
        forced = None
        if base_sample_inds is not None:
            forced = np.ascontiguousarray(base_sample_inds, dtype=np.int32)
            if forced.shape != (Dc - 1, Q, S):
                raise ValueError(f"base_sample_inds must be {(Dc - 1, Q, S)}")
        u = None
        if resample_uniforms is not None:
            u = np.ascontiguousarray(resample_uniforms, dtype=np.float64)
            if u.shape != (Dc - 1, S):
                raise ValueError(f"resample_uniforms must be {(Dc - 1, S)}")
        elif forced is None and 1 < D <= L.MAX_DLAS:
            u = self.default_resample_uniforms(D)
        from .parameters import kms_to_z
        md = L.MultiDla(max_dlas=D,
                        min_z_separation=kms_to_z(3000) if min_z_separation is None else float(min_z_separation),
                        occam_log_penalty=float(np.log(S)) if occam_log_penalty is None else float(occam_log_penalty),
                        resample_uniforms=L.ptr(u) if u is not None and u.size else None,
                        forced_base_inds=L.ptr(forced, C.c_int32) if forced is not None and forced.size else None)
        out = dict(log_likelihoods_no_dla=np.full(Q, np.nan), log_likelihoods_dla=np.full((Dc, Q), np.nan),
                   min_z_dlas=np.full(Q, np.nan), max_z_dlas=np.full(Q, np.nan),
                   num_pixels=np.zeros(Q, dtype=np.int32), max_dlas=D)
        if want_samples:
            out["sample_log_likelihoods_dla"] = np.full((Dc, Q, S), np.nan)
            out["base_sample_inds"] = np.full((Dc - 1, Q, S), -1, dtype=np.int32)
        spec = None
        if summary is not None:
            ez, en = summary["z_edges"], summary["n_edges"]
            nz, nn = (0, 0) if ez is None else (ez.size - 1, en.size - 1)
            spec = L.SummarySpec(log_nhi_samples=L.ptr(summary["log_nhi"]), num_z_bins=nz, num_nhi_bins=nn,
                                 z_edges=L.ptr(ez), log_nhi_edges=L.ptr(en))
            sout = dict(map_sample_inds=np.full((Dc, Q), -1, dtype=np.int32), map_log_likelihoods=np.full((Dc, Q), np.nan),
                        map_z_dlas=np.full((Dc, Q, L.MAX_DLAS), np.nan), map_log_nhis=np.full((Dc, Q, L.MAX_DLAS), np.nan))
            if ez is not None:
                sout["bin_planes"] = np.zeros((Q, L.SUMMARY_PLANES, max(nz, 0), max(nn, 0)))

        ispec, iout = None, {}
        if intervals is not None:
            if spec is None or sub is not None or models or population is not None or levels:
                raise ValueError("intervals go with the summaries alone")
            lv_q = intervals["levels"]
            nlq = min(lv_q.size, L.INTERVAL_MAX_LEVELS)
            ispec = L.IntervalSpec(log_nhi_samples=L.ptr(intervals["log_nhi"]), lr_delta=intervals["lr_delta"],
                                   num_levels=lv_q.size)
            for i in range(nlq):
                ispec.levels[i] = lv_q[i]
            slot = (Dc, Q, L.MAX_DLAS)
            iout = dict(z_dla_means=np.full(slot, np.nan), z_dla_sds=np.full(slot, np.nan),
                        log_nhi_means=np.full(slot, np.nan), log_nhi_sds=np.full(slot, np.nan),
                        z_dla_lr_ranges=np.full(slot + (2,), np.nan), log_nhi_lr_ranges=np.full(slot + (2,), np.nan),
                        z_dla_quantiles=np.full(slot + (max(nlq, 1),), np.nan),
                        log_nhi_quantiles=np.full(slot + (max(nlq, 1),), np.nan),
                        lr_counts=np.zeros((Dc, Q), dtype=np.int32))

        mlev = mres = None
        if model_spectra is not None:
            if spec is None or sub is not None or models or population is not None or levels or cuts is not None:
                raise ValueError("model_spectra goes with the summaries and intervals (not sub_dla, population, levels or cuts)")
            caps = model_spectra["capacities"]
            m_cap = np.zeros(Q + 1, dtype=np.int64)
            np.cumsum(caps, out=m_cap[1:])
            tot = max(int(m_cap[-1]), 1)
            m_pix = np.full(tot, -1, dtype=np.int32)
            m_arr = {k: np.full(tot, np.nan) for k in ("absorption", "model_mean", "continuum", "continuum_sd")}
            m_q = dict(chi2=np.full(Q, np.nan), log_likelihoods=np.full(Q, np.nan), num_pixels=np.zeros(Q, dtype=np.int32),
                       levels=np.full(Q, -1, dtype=np.int32))
            m_given, m_lp = model_spectra["levels"], model_spectra["log_priors_dla"]
            mlev = L.ModelLevels(level_mode=L.MODEL_LEVEL_BEST if m_given is None else L.MODEL_LEVEL_GIVEN,
                                 levels=L.ptr(m_given, C.c_int32), log_priors_dla=L.ptr(m_lp))
            mres = L.ModelSpectra(memory=L.MEM_HOST, cap_offsets=L.ptr(m_cap, C.c_int64), pixel_inds=L.ptr(m_pix, C.c_int32),
                                  absorption=L.ptr(m_arr["absorption"]), model_mean=L.ptr(m_arr["model_mean"]),
                                  continuum_mean=L.ptr(m_arr["continuum"]), continuum_sd=L.ptr(m_arr["continuum_sd"]),
                                  chi2=L.ptr(m_q["chi2"]), log_likelihoods=L.ptr(m_q["log_likelihoods"]),
                                  num_pixels=L.ptr(m_q["num_pixels"], C.c_int32), levels=L.ptr(m_q["levels"], C.c_int32))

        def results_intervals(mem, get):
            return L.Intervals(memory=mem, z_means=get("z_dla_means"), z_sds=get("z_dla_sds"),
                               log_nhi_means=get("log_nhi_means"), log_nhi_sds=get("log_nhi_sds"),
                               z_lr_ranges=get("z_dla_lr_ranges"), log_nhi_lr_ranges=get("log_nhi_lr_ranges"),
                               z_quantiles=get("z_dla_quantiles"), log_nhi_quantiles=get("log_nhi_quantiles"),
                               lr_counts=get("lr_counts", C.c_int32))

        subs, subout = None, {}
        if sub is not None:
            subs = L.SubDla(nhi_samples=L.ptr(sub["nhi"]))
            subout = dict(log_likelihoods_lls=np.full(Q, np.nan))
            if want_samples:
                subout["sample_log_likelihoods_lls"] = np.full((Q, S), np.nan)
            if spec is not None and sub.get("log_nhi") is not None:
                subout.update(map_sample_ind_lls=np.full(Q, -1, dtype=np.int32), map_log_likelihood_lls=np.full(Q, np.nan),
                              MAP_z_lls=np.full(Q, np.nan), MAP_log_nhi_lls=np.full(Q, np.nan))

        pspec, pout = None, {}
        if population is not None:
            pz, pn = population["z_edges"], population["log_nhi_edges"]
            lp_no, lp_dla, lp_lls = population["log_priors_no_dla"], population["log_priors_dla"], population["log_priors_lls"]
            if lp_no.shape != (Q,) or lp_dla.shape != (Dc, Q) or (lp_lls is not None and lp_lls.shape != (Q,)):
                raise ValueError(f"population priors must be {(Q,)}, {(Dc, Q)} and {(Q,)}")
            if sub is not None and lp_lls is None:
                raise ValueError("population with the sub-DLA model needs log_priors_lls")
            pspec = L.PopulationSpec(log_nhi_samples=L.ptr(population["log_nhi"]), num_z_bins=pz.size - 1,
                                     num_nhi_bins=pn.size - 1, z_edges=L.ptr(pz), log_nhi_edges=L.ptr(pn),
                                     p_thresh_sample=population["p_thresh_sample"], p_switch=population["p_switch"],
                                     p_thresh_spec=population["p_thresh_spec"], log_priors_no_dla=L.ptr(lp_no),
                                     log_priors_dla=L.ptr(lp_dla), log_priors_lls=L.ptr(lp_lls))
            pout = dict(population_poisson=np.zeros((Q, max(pz.size - 1, 0), max(pn.size - 1, 0))),
                        population_large_inds=np.full((Q, L.POPULATION_MAX_LARGE), -1, dtype=np.int32),
                        population_large_probs=np.full((Q, L.POPULATION_MAX_LARGE), np.nan),
                        population_large_bins=np.full((Q, L.POPULATION_MAX_LARGE), -1, dtype=np.int32),
                        population_p_dlas=np.full(Q, np.nan))

        lvout = {}
        if levels:
            if "planes" in levels:
                if spec is None or "bin_planes" not in sout:
                    raise ValueError("the level planes need a summary grid")
                lvout["bin_planes_levels"] = np.zeros((Q, Dc) + sout["bin_planes"].shape[1:])
            if "split" in levels:
                if pspec is None:
                    raise ValueError("the level split needs population")
                NL = L.POPULATION_MAX_LARGE
                lvout.update(population_level_posteriors=np.full((Dc, Q), np.nan),
                             population_level_poisson=np.zeros((Q, Dc) + pout["population_poisson"].shape[1:]),
                             population_level_large_inds=np.full((Q, Dc, NL), -1, dtype=np.int32),
                             population_level_large_probs=np.full((Q, Dc, NL), np.nan),
                             population_level_large_bins=np.full((Q, Dc, NL, L.MAX_DLAS), -1, dtype=np.int32))

        cspec, cout = None, {}
        if cuts is not None:
            if intervals is not None or sub is not None:
                raise ValueError("cuts do not cover the interval outputs or the sub-DLA model")
            ces = summary["z_edges"] if summary is not None else None
            cep = population["z_edges"] if population is not None else None
            if ces is None and cep is None:
                raise ValueError("cuts need a summary grid or population")
            cspec = L.SearchCuts(proximity_zone=cuts["proximity_zone"], noise_thresh=cuts["noise_thresh"],
                                 omega_m=cuts["omega_m"], num_z_bins_summary=0 if ces is None else ces.size - 1,
                                 z_edges_summary=L.ptr(ces), num_z_bins_population=0 if cep is None else cep.size - 1,
                                 z_edges_population=L.ptr(cep))
            cout = dict(cut_z_uppers=np.full(Q, np.nan), cut_pixel_counts=np.zeros(Q, dtype=np.int32),
                        cut_bitmap_offsets=np.zeros(Q + 1, dtype=np.int64),
                        cut_bitmap_words=np.zeros(max(int(((np.diff(offsets) + 31) // 32).sum()), 1), dtype=np.uint32))
            if ces is not None:
                cout["cut_path_summary"] = np.zeros((Q, ces.size))
            if cep is not None:
                cout["cut_path_population"] = np.zeros((Q, cep.size))

        def results_cuts(mem, get):
            if cspec is None:
                return None
            return L.SearchCutResults(memory=mem, z_uppers=get("cut_z_uppers"), pixel_counts=get("cut_pixel_counts", C.c_int32),
                                      bitmap_offsets=get("cut_bitmap_offsets", C.c_int64),
                                      bitmap_words=get("cut_bitmap_words", C.c_uint32), path_summary=get("cut_path_summary"),
                                      path_population=get("cut_path_population"))

        def results_levels(mem, get):
            if not lvout:
                return None
            return L.LevelPopulation(memory=mem, level_posteriors=get("population_level_posteriors"),
                                     bin_planes=get("bin_planes_levels"), poisson_plane=get("population_level_poisson"),
                                     large_inds=get("population_level_large_inds", C.c_int32),
                                     large_probs=get("population_level_large_probs"),
                                     large_bins=get("population_level_large_bins", C.c_int32))

        def results_pop(mem, get):
            if pspec is None:
                return None
            return L.Population(memory=mem, poisson_plane=get("population_poisson"),
                                large_inds=get("population_large_inds", C.c_int32),
                                large_probs=get("population_large_probs"),
                                large_bins=get("population_large_bins", C.c_int32), p_dlas=get("population_p_dlas"))

        def results_sub(mem, get):
            if sub is None:
                return None
            return L.ResultsSub(memory=mem, log_likelihoods_lls=get("log_likelihoods_lls"),
                                sample_log_likelihoods_lls=get("sample_log_likelihoods_lls"), sample_ld=S,
                                log_nhi_samples=L.ptr(sub.get("log_nhi")),
                                map_sample_inds=get("map_sample_ind_lls", C.c_int32),
                                map_log_likelihoods=get("map_log_likelihood_lls"), map_z_lls=get("MAP_z_lls"),
                                map_log_nhi_lls=get("MAP_log_nhi_lls"))

        def call(sp, rs, sm, rsub=None, rpop=None, rlv=None, riv=None, rcut=None):
            if mlev is not None:
                return self.lib.gpdla_engine_process_spectra_models(
                    self._h, C.byref(sp), C.byref(md), C.byref(rs), C.byref(spec), C.byref(sm),
                    C.byref(ispec) if ispec is not None else None, C.byref(riv) if riv is not None else None,
                    C.byref(mlev), C.byref(mres))
            if cspec is not None:
                return self.lib.gpdla_engine_process_cuts(
                    self._h, C.byref(sp), C.byref(md), C.byref(subs) if subs is not None else None, C.byref(rs),
                    C.byref(rsub) if rsub is not None else None, C.byref(spec) if spec is not None else None,
                    C.byref(sm) if sm is not None else None, C.byref(pspec) if pspec is not None else None,
                    C.byref(rpop) if rpop is not None else None, C.byref(rlv) if rlv is not None else None,
                    C.byref(cspec), C.byref(rcut))
            if ispec is not None:
                return self.lib.gpdla_engine_process_intervals(self._h, C.byref(sp), C.byref(md), C.byref(rs),
                                                               C.byref(spec), C.byref(sm), C.byref(ispec), C.byref(riv))
            if levels is not None:
                return self.lib.gpdla_engine_process_levels(
                    self._h, C.byref(sp), C.byref(md), C.byref(subs) if subs is not None else None, C.byref(rs),
                    C.byref(rsub) if rsub is not None else None, C.byref(spec) if spec is not None else None,
                    C.byref(sm) if sm is not None else None, C.byref(pspec) if pspec is not None else None,
                    C.byref(rpop) if rpop is not None else None, C.byref(rlv) if rlv is not None else None)
            if models == "population":
                return self.lib.gpdla_engine_process_population(
                    self._h, C.byref(sp), C.byref(md), C.byref(subs) if subs is not None else None, C.byref(rs),
                    C.byref(rsub) if rsub is not None else None, C.byref(spec) if spec is not None else None,
                    C.byref(sm) if sm is not None else None, C.byref(pspec) if pspec is not None else None,
                    C.byref(rpop) if rpop is not None else None)
            if models:
                return self.lib.gpdla_engine_process_models(
                    self._h, C.byref(sp), C.byref(md), C.byref(subs) if subs is not None else None, C.byref(rs),
                    C.byref(rsub) if rsub is not None else None, C.byref(spec) if spec is not None else None,
                    C.byref(sm) if sm is not None else None)
            if spec is None:
                return self.lib.gpdla_engine_process_multi(self._h, C.byref(sp), C.byref(md), C.byref(rs))
            return self.lib.gpdla_engine_process_summaries(self._h, C.byref(sp), C.byref(md), C.byref(rs),
                                                           C.byref(spec), C.byref(sm))
        sm = None
        if memory == "host":
            sp = L.Spectra(memory=L.MEM_HOST, num_spectra=Q, offsets=L.ptr(offsets, C.c_int64),
                           wavelengths=L.ptr(wl), flux=L.ptr(fl), noise_variance=L.ptr(nv),
                           pixel_mask=L.ptr(mk, C.c_uint8), z_qsos=L.ptr(zq))
            sll, base = out.get("sample_log_likelihoods_dla"), out.get("base_sample_inds")
            rs = L.ResultsMulti(memory=L.MEM_HOST, log_likelihoods_no_dla=L.ptr(out["log_likelihoods_no_dla"]),
                                log_likelihoods_dla=L.ptr(out["log_likelihoods_dla"]),
                                sample_log_likelihoods_dla=L.ptr(sll), sample_ld=S,
                                base_sample_inds=L.ptr(base, C.c_int32) if base is not None and base.size else None,
                                min_z_dlas=L.ptr(out["min_z_dlas"]), max_z_dlas=L.ptr(out["max_z_dlas"]),
                                num_pixels=L.ptr(out["num_pixels"], C.c_int32))
            if spec is not None:
                pl = sout.get("bin_planes")
                sm = L.Summaries(memory=L.MEM_HOST, map_sample_inds=L.ptr(sout["map_sample_inds"], C.c_int32),
                                 map_log_likelihoods=L.ptr(sout["map_log_likelihoods"]),
                                 map_z_dlas=L.ptr(sout["map_z_dlas"]), map_log_nhis=L.ptr(sout["map_log_nhis"]),
                                 bin_planes=L.ptr(pl) if pl is not None and pl.size else None)
            rc = call(sp, rs, sm, results_sub(L.MEM_HOST, lambda k, t=C.c_double: L.ptr(subout.get(k), t)),
                      results_pop(L.MEM_HOST, lambda k, t=C.c_double: L.ptr(pout[k], t) if pout[k].size else None),
                      results_levels(L.MEM_HOST, lambda k, t=C.c_double: L.ptr(lvout[k], t) if k in lvout and lvout[k].size else None),
                      results_intervals(L.MEM_HOST, lambda k, t=C.c_double: L.ptr(iout[k], t) if iout[k].size else None)
                      if ispec is not None else None,
                      results_cuts(L.MEM_HOST, lambda k, t=C.c_double: L.ptr(cout[k], t) if k in cout and cout[k].size else None))
        elif memory == "device":
            dev = {k: L.DeviceArray.from_numpy(v, self.device) for k, v in
                   dict(wl=wl, fl=fl, nv=nv, mk=mk, zq=zq).items()}
            dout = {k: L.DeviceArray(self.device, v.shape, v.dtype) for k, v in out.items()
                    if isinstance(v, np.ndarray) and v.size}
            sp = L.Spectra(memory=L.MEM_DEVICE, num_spectra=Q, offsets=L.ptr(offsets, C.c_int64),
                           wavelengths=L.dev_ptr(dev["wl"].ptr), flux=L.dev_ptr(dev["fl"].ptr),
                           noise_variance=L.dev_ptr(dev["nv"].ptr), pixel_mask=L.dev_ptr(dev["mk"].ptr, C.c_uint8),
                           z_qsos=L.dev_ptr(dev["zq"].ptr))

            def dptr(key, ctype=C.c_double):
                return L.dev_ptr(dout[key].ptr, ctype) if key in dout else None
            rs = L.ResultsMulti(memory=L.MEM_DEVICE, log_likelihoods_no_dla=dptr("log_likelihoods_no_dla"),
                                log_likelihoods_dla=dptr("log_likelihoods_dla"),
                                sample_log_likelihoods_dla=dptr("sample_log_likelihoods_dla"), sample_ld=S,
                                base_sample_inds=dptr("base_sample_inds", C.c_int32),
                                min_z_dlas=dptr("min_z_dlas"), max_z_dlas=dptr("max_z_dlas"),
                                num_pixels=dptr("num_pixels", C.c_int32))
            dsum = {}
            if spec is not None:
                dsum = {k: L.DeviceArray(self.device, v.shape, v.dtype) for k, v in sout.items() if v.size}

                def sptr(key, ctype=C.c_double):
                    return L.dev_ptr(dsum[key].ptr, ctype) if key in dsum else None
                sm = L.Summaries(memory=L.MEM_DEVICE, map_sample_inds=sptr("map_sample_inds", C.c_int32),
                                 map_log_likelihoods=sptr("map_log_likelihoods"), map_z_dlas=sptr("map_z_dlas"),
                                 map_log_nhis=sptr("map_log_nhis"), bin_planes=sptr("bin_planes"))
            dsub = {k: L.DeviceArray(self.device, v.shape, v.dtype) for k, v in subout.items() if v.size}
            dpop = {k: L.DeviceArray(self.device, v.shape, v.dtype) for k, v in pout.items() if v.size}
            dlv = {k: L.DeviceArray(self.device, v.shape, v.dtype) for k, v in lvout.items() if v.size}
            div = {k: L.DeviceArray(self.device, v.shape, v.dtype) for k, v in iout.items() if v.size}
            dcut = {k: L.DeviceArray(self.device, v.shape, v.dtype) for k, v in cout.items()}   # (empty arrays too: non-null)
            rc = call(sp, rs, sm, results_sub(L.MEM_DEVICE, lambda k, t=C.c_double: L.dev_ptr(dsub[k].ptr, t) if k in dsub else None),
                      results_pop(L.MEM_DEVICE, lambda k, t=C.c_double: L.dev_ptr(dpop[k].ptr, t) if k in dpop else None),
                      results_levels(L.MEM_DEVICE, lambda k, t=C.c_double: L.dev_ptr(dlv[k].ptr, t) if k in dlv else None),
                      results_intervals(L.MEM_DEVICE, lambda k, t=C.c_double: L.dev_ptr(div[k].ptr, t) if k in div else None)
                      if ispec is not None else None,
                      results_cuts(L.MEM_DEVICE, lambda k, t=C.c_double: L.dev_ptr(dcut[k].ptr, t) if k in dcut else None))
            if rc in (L.GPDLA_OK, L.GPDLA_ENUMERIC):
                for k, d in dlv.items():
                    lvout[k] = d.numpy()
                for k, d in div.items():
                    iout[k] = d.numpy()
                for k, d in dcut.items():
                    cout[k] = d.numpy()
                for k, d in dpop.items():
                    pout[k] = d.numpy()
                for k, d in dout.items():
                    out[k] = d.numpy()
                for k, d in dsum.items():
                    sout[k] = d.numpy()
                for k, d in dsub.items():
                    subout[k] = d.numpy()
            for d in list(dev.values()) + list(dout.values()) + list(dsum.values()) + list(dsub.values()) + list(dpop.values()) + list(dlv.values()) + list(div.values()) + list(dcut.values()):
                d.free()
        else:
            raise ValueError("memory must be 'host' or 'device'")
        if rc == L.GPDLA_ENUMERIC and not raise_numeric:
            out["numeric_warning"] = self.lib.gpdla_last_error().decode()
        else:
            L.check(rc)
        if spec is not None:
            out["map_sample_inds"], out["map_log_likelihoods"] = sout["map_sample_inds"], sout["map_log_likelihoods"]
            out["MAP_z_dlas"] = np.ascontiguousarray(sout["map_z_dlas"][:, :, :Dc])
            out["MAP_log_nhis"] = np.ascontiguousarray(sout["map_log_nhis"][:, :, :Dc])
            if "bin_planes" in sout:
                out["bin_planes"] = sout["bin_planes"]
        out.update(subout)
        out.update(pout)
        out.update(lvout)
        if cspec is not None:
            cout["cut_bitmap_words"] = cout["cut_bitmap_words"][:int(cout["cut_bitmap_offsets"][-1])]
            out.update(cout, cut_proximity_zone=float(cuts["proximity_zone"]), cut_noise_thresh=float(cuts["noise_thresh"]))
        if mlev is not None:
            ms = compact_model_spectra(m_cap, m_q["num_pixels"], m_pix, m_arr)
            out.update(model_offsets=ms["offsets"], model_pixel_inds=ms["pixel_inds"], model_absorption=ms["absorption"],
                       model_mean=ms["model_mean"], model_continuum=ms["continuum"], model_continuum_sd=ms["continuum_sd"],
                       model_levels=m_q["levels"], model_log_likelihoods=m_q["log_likelihoods"], model_chi2=m_q["chi2"],
                       model_num_pixels=m_q["num_pixels"])
        if ispec is not None:
            for key, v in iout.items():   # the C arrays are GPDLA_MAX_DLAS slots wide
                out[key] = v if key == "lr_counts" else np.ascontiguousarray(v[:, :, :Dc])
            out["interval_levels"], out["lr_delta"] = intervals["levels"].copy(), float(intervals["lr_delta"])
        return out

    # --------------------------------------------------------------------- sub-DLA model and forest
    def set_forest(self, forest=None, *, num_forest_lines: int = 31, variance_series: bool = True,
                   mean_flux: bool = True, mean_flux_tau_0: float = 0.0023, mean_flux_beta: float = 3.65,
                   mean_flux_scope: str = "mu") -> None:
        """The Lyman-series forest of every later ``process*`` call (gpdla_engine_set_forest_scoped).
        ``forest`` is None (the Lya-only null model, as before), True (the keyword defaults: 31 lines, both
        parts, Kim et al. 2007's mean flux) or a dict of those keywords.  ``variance_series``: omega^2 sums
        the series with the model's tau_0, beta, c_0; ``mean_flux``: mu is multiplied by
        F = exp(-sum_i tau_0 c_i (1 + z_i)^beta) for every model.  ``mean_flux_scope`` says what else F
        multiplies (``MEAN_FLUX_SCOPES``): "mu" nothing (the default), "mu_M" the rows of M, "all" the rows
        of M and omega^2 (by F^2) -- the model ``learn_qso_model(forest=dict(mean_flux=True))`` learns;
        other than "mu" it needs ``mean_flux`` (ValueError).  Fused fp64 path only."""
        if forest is None or forest is False:
            L.check(self.lib.gpdla_engine_set_forest(self._h, None))
            return
        kw = dict(num_forest_lines=num_forest_lines, variance_series=variance_series, mean_flux=mean_flux,
                  mean_flux_tau_0=mean_flux_tau_0, mean_flux_beta=mean_flux_beta, mean_flux_scope=mean_flux_scope)
        if isinstance(forest, dict):
            unknown = set(forest) - set(kw)
            if unknown:
                raise TypeError(f"unexpected forest settings {sorted(unknown)}")
            kw.update(forest)
        scope = mean_flux_scope_code(kw["mean_flux_scope"], kw["mean_flux"])
        fs = L.Forest(num_forest_lines=int(kw["num_forest_lines"]), variance_series=int(bool(kw["variance_series"])),
                      mean_flux=int(bool(kw["mean_flux"])), mean_flux_tau_0=float(kw["mean_flux_tau_0"]),
                      mean_flux_beta=float(kw["mean_flux_beta"]))
        L.check(self.lib.gpdla_engine_set_forest_scoped(self._h, C.byref(fs), scope))

    def process_models(self, packed: dict, max_dlas: int = 1, sub_dla=None, log_nhi_samples=None, z_edges=None,
                       log_nhi_edges=None, sub_dla_log_nhi=None, want_samples: bool = True, **kwargs) -> dict:
        """``process_multi`` -- or, with ``log_nhi_samples`` (and optionally the grid), ``process_summaries`` --
        plus the sub-DLA model (gpdla_engine_process_models).  ``sub_dla``: S column densities (cm^-2) in the
        engine's sample order; sample j is one absorber at the engine's own z_j with that column density.
        Adds ``log_likelihoods_lls`` (Q; log-mean-exp, any NaN -> NaN), ``sample_log_likelihoods_lls`` (Q x S,
        with ``want_samples``) and, with summaries, ``map_sample_ind_lls`` (Q int32, -1 = none),
        ``map_log_likelihood_lls``, ``MAP_z_lls`` and ``MAP_log_nhi_lls`` (Q; ``sub_dla_log_nhi`` defaults to
        log10 of ``sub_dla``).  Every other array is the plain call's, bit for bit; ``sub_dla=None`` is
        exactly that call."""
        return self._process_models(packed, max_dlas, sub_dla, log_nhi_samples, z_edges, log_nhi_edges, sub_dla_log_nhi,
                                    want_samples, True, None, kwargs)

    def _process_models(self, packed, max_dlas, sub_dla, log_nhi_samples, z_edges, log_nhi_edges, sub_dla_log_nhi,
                        want_samples, entry, population, kwargs, levels=None, cuts=None) -> dict:
        """``process_models`` / ``process_population`` / ``process_levels``: ``entry``, ``population`` and
        ``levels`` are ``_run_multi``'s ``models``, ``population`` and ``levels``."""
        if (z_edges is None) != (log_nhi_edges is None):
            raise ValueError("z_edges and log_nhi_edges go together")
        if z_edges is not None and log_nhi_samples is None:
            raise ValueError("a summary grid needs log_nhi_samples")
        summary = None
        if log_nhi_samples is not None:
            lognhi = np.ascontiguousarray(log_nhi_samples, dtype=np.float64).ravel()
            if lognhi.size != self.num_samples:
                raise ValueError("one log_nhi sample per engine sample")
            summary = dict(log_nhi=lognhi,
                           z_edges=None if z_edges is None else np.ascontiguousarray(z_edges, dtype=np.float64).ravel(),
                           n_edges=None if log_nhi_edges is None else np.ascontiguousarray(log_nhi_edges, dtype=np.float64).ravel())
        sub = None
        if sub_dla is not None:
            nhi = np.ascontiguousarray(sub_dla, dtype=np.float64).ravel()
            if nhi.size != self.num_samples:
                raise ValueError("one sub-DLA column density per engine sample")
            sub = dict(nhi=nhi, log_nhi=None)
            if summary is not None:
                with np.errstate(divide="ignore", invalid="ignore"):
                    ln = np.log10(nhi) if sub_dla_log_nhi is None else np.ascontiguousarray(sub_dla_log_nhi, dtype=np.float64).ravel()
                if ln.size != nhi.size:
                    raise ValueError("one sub_dla_log_nhi per sub-DLA sample")
                sub["log_nhi"] = np.ascontiguousarray(ln)
        order = ("resample_uniforms", "base_sample_inds", "min_z_separation", "occam_log_penalty", "raise_numeric", "memory")
        unknown = set(kwargs) - set(order)
        if unknown:
            raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
        return self._run_multi(packed, max_dlas, kwargs.get("resample_uniforms"), kwargs.get("base_sample_inds"),
                               want_samples, kwargs.get("min_z_separation"), kwargs.get("occam_log_penalty"),
                               kwargs.get("raise_numeric", False), kwargs.get("memory", "host"), summary, sub, entry,
                               population, levels, cuts=cuts)

    def process_population(self, packed: dict, max_dlas: int = 1, population=None, sub_dla=None, log_nhi_samples=None,
                           z_edges=None, log_nhi_edges=None, sub_dla_log_nhi=None, want_samples: bool = True,
                           **kwargs) -> dict:
        """``process_models`` (its arguments pass through) plus the population statistics reduced on the device
        (gpdla_engine_process_population).  ``population`` is a dict of ``z_edges``,
        ``log_nhi_edges`` (a grid of its own, independent of a summary grid), ``log_nhi_samples`` (the engine's
        samples' log10 N_HI), ``log_priors_no_dla`` (Q), ``log_priors_dla`` (D x Q, or Q for D = 1),
        ``log_priors_lls`` (Q, with ``sub_dla``) and optionally ``p_thresh_sample`` (1e-4), ``p_switch`` (0.25),
        ``p_thresh_spec`` (0.05).  Adds, with p_j = p_dla pi_j over the level-1 samples of a spectrum,

        ``population_p_dlas`` (Q)               the p_dla the device formed from the evidences and the priors
        ``population_poisson`` (Q x nz x nn)    per bin, sum of p_j with p_thresh_sample < p_j < p_switch
        ``population_large_inds`` / ``_probs`` / ``_bins`` (Q x 8)   the samples with p_j >= p_switch in a bin,
                                                 by increasing index (0-based), p_j and bin iz nn + in; unused
                                                 slots -1 / NaN / -1
        ``population=None`` is ``process_models``, bit for bit.  Repeated calls and any ``max_batch_spectra``
        give bitwise equal outputs."""
        return self._process_models(packed, max_dlas, sub_dla, log_nhi_samples, z_edges, log_nhi_edges, sub_dla_log_nhi,
                                    want_samples, "population", self._population_dict(population), kwargs)

    def _population_dict(self, population):
        """``process_population``'s ``population`` in ``_run_multi``'s working form (None stays None)."""
        pop = None
        if population is not None:
            known = {"z_edges", "log_nhi_edges", "log_nhi_samples", "log_priors_no_dla", "log_priors_dla",
                     "log_priors_lls", "p_thresh_sample", "p_switch", "p_thresh_spec"}
            if not isinstance(population, dict) or set(population) - known:
                raise ValueError(f"population must be a dict of {sorted(known)}")
            missing = {"z_edges", "log_nhi_edges", "log_nhi_samples", "log_priors_no_dla", "log_priors_dla"} - set(population)
            if missing:
                raise ValueError(f"population lacks {sorted(missing)}")

            def vec(key):
                return None if population.get(key) is None else np.ascontiguousarray(population[key], dtype=np.float64).ravel()
            lognhi = vec("log_nhi_samples")
            if lognhi.size != self.num_samples:
                raise ValueError("one log_nhi sample per engine sample")
            lp_dla = np.ascontiguousarray(population["log_priors_dla"], dtype=np.float64)
            if lp_dla.ndim == 1:
                lp_dla = lp_dla[None]
            pop = dict(log_nhi=lognhi, z_edges=vec("z_edges"), log_nhi_edges=vec("log_nhi_edges"),
                       log_priors_no_dla=vec("log_priors_no_dla"), log_priors_dla=lp_dla, log_priors_lls=vec("log_priors_lls"),
                       p_thresh_sample=float(population.get("p_thresh_sample", 1e-4)),
                       p_switch=float(population.get("p_switch", 0.25)),
                       p_thresh_spec=float(population.get("p_thresh_spec", 0.05)))
            if pop["z_edges"].size < 1 or pop["log_nhi_edges"].size < 1:
                raise ValueError("population edges must not be empty")
        return pop

    def process_levels(self, packed: dict, max_dlas: int = 1, population=None, sub_dla=None, log_nhi_samples=None,
                       z_edges=None, log_nhi_edges=None, sub_dla_log_nhi=None, want_samples: bool = True,
                       levels=None, **kwargs) -> dict:
        """``process_population`` (its arguments pass through; every array of it comes back bit for bit) plus
        the population statistics over every level of the multi-DLA search (gpdla_engine_process_levels;
        DESIGN.md section 18): sample j of level d carries d absorbers, its own and those of its base chain, and
        each is binned with the sample's normalised mass pi_{d,j}.  ``levels`` names the halves wanted,
        ``("planes", "split")``; the default is every half the call has the inputs for (a summary grid,
        ``population``), and ``levels=()`` is ``process_population`` itself.  Adds

        ``bin_planes_levels`` (Q x D x 5 x nz x nn)        "planes": per level, ``bin_planes``'s five sums over the
                                                           (sample, slot) pairs of each bin of the summary grid
        ``population_level_posteriors`` (D x Q)            "split": P_d, the posterior of exactly d DLAs
        ``population_level_poisson`` (Q x D x nz x nn)     per level ``population_poisson`` with p = P_d pi_{d,j},
                                                           added to the bin of every slot of the sample
        ``population_level_large_inds`` / ``_probs`` (Q x D x 8), ``_bins`` (Q x D x 8 x 4)   the samples with
                                                           p >= p_switch and a slot inside the grid: index, p and
                                                           one bin per slot (-1 outside the grid or beyond d)
        Level 1 of the planes is ``bin_planes`` bit for bit."""
        have = (("planes",) if z_edges is not None else ()) + (("split",) if population is not None else ())
        halves = have if levels is None else tuple(levels)
        if set(halves) - {"planes", "split"}:
            raise ValueError("levels names 'planes' and / or 'split'")
        return self._process_models(packed, max_dlas, sub_dla, log_nhi_samples, z_edges, log_nhi_edges, sub_dla_log_nhi,
                                    want_samples, "population", self._population_dict(population), kwargs,
                                    levels=halves)

    def process_cuts(self, packed: dict, max_dlas: int = 1, cuts=None, population=None, log_nhi_samples=None,
                     z_edges=None, log_nhi_edges=None, want_samples: bool = True, levels=(), **kwargs) -> dict:
        """``process_levels`` (its arguments pass through, without the sub-DLA model; ``levels=()`` by default, i.e.
        ``process_population``) under the search cuts (gpdla_engine_process_cuts).  ``cuts``
        is a dict of ``proximity_zone`` and ``noise_thresh`` (either None for off, not both) and optionally
        ``omega_m`` (0.279).  Every grid reduction of the call -- ``bin_planes``, ``population_*``,
        ``bin_planes_levels``, ``population_level_*`` -- drops the absorber slots in the proximity zone or on a
        noisy pixel; every other array is unchanged bit for bit.  Adds ``cut_proximity_zone`` / ``cut_noise_thresh``
        (NaN = off), ``cut_z_uppers`` (Q), ``cut_pixel_counts`` (Q), the good-pixel bitmap ``cut_bitmap_offsets``
        (Q + 1) / ``cut_bitmap_words``, and the path columns ``cut_path_summary`` (Q x (nz + 1), with a summary
        grid) and ``cut_path_population`` (with ``population``): each z bin, then the grid's whole extent.
        ``cuts=None`` is ``process_levels``, bit for bit."""
        have = (("planes",) if z_edges is not None else ()) + (("split",) if population is not None else ())
        halves = have if levels is None else tuple(levels)
        if set(halves) - {"planes", "split"}:
            raise ValueError("levels names 'planes' and / or 'split'")
        return self._process_models(packed, max_dlas, None, log_nhi_samples, z_edges, log_nhi_edges, None, want_samples,
                                    "population", self._population_dict(population), kwargs, levels=halves,
                                    cuts=normalise_cuts(cuts))

    # --------------------------------------------------------------------------- model spectra
    def model_spectra(self, packed: dict, z_dlas, log_nhis, counts=None, nhis=None, capacities=None) -> dict:
        """gpdla_engine_model_spectra: the model of the given absorbers on every spectrum's likelihood pixels,
        without a search.  ``z_dlas`` / ``log_nhis`` are [Q][<= 4] (NaN-padded rows are fine with ``counts``);
        ``counts`` [Q] defaults to the number of leading finite pairs of each row; ``nhis`` (optional) gives the
        column densities themselves instead of 10**log_nhis.  Returns the compacted CSR: ``offsets`` [Q + 1],
        ``pixel_inds`` (index within the spectrum), ``absorption``, ``model_mean``, ``continuum``,
        ``continuum_sd`` (flat), and ``chi2``, ``log_likelihoods``, ``num_pixels`` per spectrum.  The posterior
        absorbed fit is absorption * continuum.  ``capacities`` [Q] overrides the per-spectrum capacity
        (default: ``model_capacities``); a spectrum over its capacity raises GpdlaError, whose ``partial``
        attribute holds the result with that spectrum empty."""
        offsets = np.ascontiguousarray(packed["offsets"], dtype=np.int64)
        Q = offsets.size - 1
        wl = np.ascontiguousarray(packed["wavelengths"], dtype=np.float64)
        fl = np.ascontiguousarray(packed["flux"], dtype=np.float64)
        nv = np.ascontiguousarray(packed["noise_variance"], dtype=np.float64)
        mk = np.ascontiguousarray(packed["pixel_mask"], dtype=np.uint8)
        zq = np.ascontiguousarray(packed["z_qsos"], dtype=np.float64)
        if not (wl.size == fl.size == nv.size == mk.size and offsets[-1] <= wl.size and zq.size == Q):
            raise ValueError("inconsistent spectra arrays")
        z4, n4, cnt = _absorber_arrays(Q, z_dlas, log_nhis, counts)
        lin = None
        if nhis is not None:
            lin = np.full((Q, L.MAX_DLAS), np.nan)
            src = np.asarray(nhis, dtype=np.float64).reshape(Q, -1)
            lin[:, :src.shape[1]] = src
        caps = model_capacities(packed, self.params) if capacities is None else np.asarray(capacities, dtype=np.int64)
        if caps.shape != (Q,) or np.any(caps < 0):
            raise ValueError("capacities must be Q non-negative integers")
        cap_off = np.zeros(Q + 1, dtype=np.int64)
        np.cumsum(caps, out=cap_off[1:])
        tot = max(int(cap_off[-1]), 1)
        pix = np.full(tot, -1, dtype=np.int32)
        arrs = {k: np.full(tot, np.nan) for k in ("absorption", "model_mean", "continuum", "continuum_sd")}
        chi2, ll, npix = np.full(Q, np.nan), np.full(Q, np.nan), np.zeros(Q, dtype=np.int32)
        sp = L.Spectra(memory=L.MEM_HOST, num_spectra=Q, offsets=L.ptr(offsets, C.c_int64),
                       wavelengths=L.ptr(wl), flux=L.ptr(fl), noise_variance=L.ptr(nv),
                       pixel_mask=L.ptr(mk, C.c_uint8), z_qsos=L.ptr(zq))
        ab = L.ModelAbsorbers(counts=L.ptr(cnt, C.c_int32), z_dlas=L.ptr(z4), log_nhis=L.ptr(n4), nhis=L.ptr(lin))
        rs = L.ModelSpectra(memory=L.MEM_HOST, cap_offsets=L.ptr(cap_off, C.c_int64), pixel_inds=L.ptr(pix, C.c_int32),
                            absorption=L.ptr(arrs["absorption"]), model_mean=L.ptr(arrs["model_mean"]),
                            continuum_mean=L.ptr(arrs["continuum"]), continuum_sd=L.ptr(arrs["continuum_sd"]),
                            chi2=L.ptr(chi2), log_likelihoods=L.ptr(ll), num_pixels=L.ptr(npix, C.c_int32))
        rc = self.lib.gpdla_engine_model_spectra(self._h, C.byref(sp), C.byref(ab), C.byref(rs))
        written = rc in (L.GPDLA_OK, L.GPDLA_ENUMERIC) or (rc == L.GPDLA_EINVAL and np.any(npix > caps))
        out = None
        if written:
            out = compact_model_spectra(cap_off, np.where(npix > caps, 0, npix), pix, arrs)
            out.update(chi2=chi2, log_likelihoods=ll, num_pixels=npix)
        if rc == L.GPDLA_ENUMERIC:
            out["numeric_warning"] = self.lib.gpdla_last_error().decode()
        elif rc != L.GPDLA_OK:
            try:
                L.check(rc)
            except L.GpdlaError as err:
                err.partial = out
                raise
        return out

    def process_model_spectra(self, packed: dict, max_dlas: int, log_nhi_samples, level="best", log_priors_dla=None,
                              z_edges=None, log_nhi_edges=None, want_samples: bool = False, intervals=None,
                              **kwargs) -> dict:
        """``process_summaries`` -- with ``intervals`` (True, or dict(levels=..., lr_delta=...)) ``process_intervals``
        -- (same arguments, same outputs bit for bit) plus the model spectra of each
        spectrum's level, rendered per device batch on the panel the sweeps just used
        (gpdla_engine_process_spectra_models).  ``level``: "best" (the DLA level 1..max_dlas with the highest model
        posterior, taken on the device from the evidences and ``log_priors_dla`` (max_dlas x Q; not needed with
        max_dlas = 1): the level ``catalog.absorber_table`` takes), an integer 0..max_dlas for every spectrum (0: the
        null model) or Q of them.  Adds ``model_offsets`` (Q + 1), ``model_pixel_inds``, ``model_absorption``,
        ``model_mean``, ``model_continuum``, ``model_continuum_sd`` (flat, CSR by ``model_offsets``),
        ``model_levels``, ``model_log_likelihoods``, ``model_chi2`` and ``model_num_pixels`` (Q); bitwise what
        ``model_spectra`` gives for the level's ``MAP_z_dlas`` / ``MAP_log_nhis``."""
        if (z_edges is None) != (log_nhi_edges is None):
            raise ValueError("z_edges and log_nhi_edges go together")
        lognhi = np.ascontiguousarray(log_nhi_samples, dtype=np.float64).ravel()
        if lognhi.size != self.num_samples:
            raise ValueError("one log_nhi sample per engine sample")
        Q, D = np.asarray(packed["offsets"]).size - 1, int(max_dlas)
        given = lp = None
        if isinstance(level, str):
            if level != "best":
                raise ValueError(f"level must be 'best', an integer 0..max_dlas or Q of them, not {level!r}")
            if D > 1:
                if log_priors_dla is None:
                    raise ValueError("level='best' with max_dlas > 1 needs log_priors_dla (max_dlas x Q)")
                lp = np.ascontiguousarray(log_priors_dla, dtype=np.float64)
                if lp.shape != (D, Q):
                    raise ValueError(f"log_priors_dla must be {(D, Q)}")
        else:
            lv = np.asarray(level)
            if lv.dtype.kind not in "iu" or lv.shape not in ((), (Q,)) or np.any(lv < 0) or np.any(lv > D):
                raise ValueError(f"level must be 'best', an integer 0..{D} or {Q} of them")
            given = np.ascontiguousarray(np.broadcast_to(lv, (Q,)), dtype=np.int32)
        summary = dict(log_nhi=lognhi,
                       z_edges=None if z_edges is None else np.ascontiguousarray(z_edges, dtype=np.float64).ravel(),
                       n_edges=None if log_nhi_edges is None else np.ascontiguousarray(log_nhi_edges, dtype=np.float64).ravel())
        order = ("resample_uniforms", "base_sample_inds", "min_z_separation", "occam_log_penalty", "raise_numeric", "memory")
        unknown = set(kwargs) - set(order)
        if unknown:
            raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
        ms = dict(levels=given, log_priors_dla=lp, capacities=model_capacities(packed, self.params))
        ivs = None
        if intervals is not None and intervals is not False:
            ivd = {} if intervals is True else dict(intervals)
            if set(ivd) - {"levels", "lr_delta"}:
                raise ValueError("intervals must be True or dict(levels=..., lr_delta=...)")
            ivs = dict(log_nhi=lognhi, levels=_interval_levels(ivd.get("levels")), lr_delta=float(ivd.get("lr_delta", 2.0)))
        return self._run_multi(packed, max_dlas, kwargs.get("resample_uniforms"), kwargs.get("base_sample_inds"),
                               want_samples, kwargs.get("min_z_separation"), kwargs.get("occam_log_penalty"),
                               kwargs.get("raise_numeric", False), kwargs.get("memory", "host"), summary, intervals=ivs,
                               model_spectra=ms)

    def model_spectra_stats(self) -> dict:
        """gpdla_engine_get_model_spectra_stats: cumulative ms and count of the model-spectra launches."""
        ms, n = C.c_double(0.0), C.c_int64(0)
        L.check(self.lib.gpdla_engine_get_model_spectra_stats(self._h, C.byref(ms), C.byref(n)))
        return dict(model_spectra_ms=ms.value, model_spectra_launches=n.value)

    def cut_stats(self) -> dict:
        """gpdla_engine_get_cut_stats: cumulative ms and count of the search-cut launches."""
        ms, n = C.c_double(0.0), C.c_int64(0)
        L.check(self.lib.gpdla_engine_get_cut_stats(self._h, C.byref(ms), C.byref(n)))
        return dict(cut_ms=ms.value, cut_launches=n.value)

    def level_population_stats(self) -> dict:
        """gpdla_engine_get_level_population_stats: cumulative ms and count of the level-population launches."""
        ms, n = C.c_double(0.0), C.c_int64(0)
        L.check(self.lib.gpdla_engine_get_level_population_stats(self._h, C.byref(ms), C.byref(n)))
        return dict(level_population_ms=ms.value, level_population_launches=n.value)

    def population_stats(self) -> dict:
        """gpdla_engine_get_population_stats: cumulative ms and count of the population launches."""
        ms, n = C.c_double(0.0), C.c_int64(0)
        L.check(self.lib.gpdla_engine_get_population_stats(self._h, C.byref(ms), C.byref(n)))
        return dict(population_ms=ms.value, population_launches=n.value)

    def model_stats(self) -> dict:
        """gpdla_engine_get_model_stats: cumulative ms / launches of the forest kernel, the sub-DLA sweeps and
        the sub-DLA log-mean-exp + MAP launches."""
        s = L.ModelStats()
        L.check(self.lib.gpdla_engine_get_model_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in L.ModelStats._fields_}

    def multi_stats(self) -> dict:
        """gpdla_engine_get_multi_stats: per-level likelihood ms / launches, resample and reduce ms."""
        s = L.MultiStats()
        L.check(self.lib.gpdla_engine_get_multi_stats(self._h, C.byref(s)))
        return dict(level_ms=list(s.level_ms), level_launches=list(s.level_launches),
                    resample_ms=s.resample_ms, resample_launches=s.resample_launches,
                    multi_reduce_ms=s.multi_reduce_ms, multi_reduce_launches=s.multi_reduce_launches)

    # ------------------------------------------------------------------------- device path
    def process_device(self, offsets: np.ndarray, wl_ptr: int, flux_ptr: int, noise_ptr: int,
                       mask_ptr: int, z_ptr: int, ll_null_ptr: int, ll_dla_ptr: int,
                       sample_ptr: int | None = None, sample_ld: int = 0,
                       zmin_ptr: int | None = None, zmax_ptr: int | None = None,
                       npix_ptr: int | None = None) -> None:
        """Enqueue the hot path on device-resident inputs/outputs (raw device addresses).
        ``offsets`` is host int64 [Q+1].  Returns after enqueueing; call ``synchronize()``."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self._keep_offsets = offsets
        Q = offsets.size - 1
        sp = L.Spectra(memory=L.MEM_DEVICE, num_spectra=Q, offsets=L.ptr(offsets, C.c_int64),
                       wavelengths=L.dev_ptr(wl_ptr), flux=L.dev_ptr(flux_ptr),
                       noise_variance=L.dev_ptr(noise_ptr), pixel_mask=L.dev_ptr(mask_ptr, C.c_uint8),
                       z_qsos=L.dev_ptr(z_ptr))
        rs = L.Results(memory=L.MEM_DEVICE, log_likelihoods_no_dla=L.dev_ptr(ll_null_ptr),
                       sample_log_likelihoods_dla=L.dev_ptr(sample_ptr), sample_ld=sample_ld or self.num_samples,
                       log_likelihoods_dla=L.dev_ptr(ll_dla_ptr), min_z_dlas=L.dev_ptr(zmin_ptr),
                       max_z_dlas=L.dev_ptr(zmax_ptr), num_pixels=L.dev_ptr(npix_ptr, C.c_int32))
        L.check(self.lib.gpdla_engine_process(self._h, C.byref(sp), C.byref(rs)))

    def synchronize(self) -> None:
        L.check(self.lib.gpdla_engine_synchronize(self._h))

    def set_stream(self, stream_handle: int | None) -> None:
        """Order the engine's kernels on an external hipStream_t handle (e.g. torch's
        ``current_stream().cuda_stream``).  Handle 0 is the null stream (torch's default stream,
        gpdla_engine_use_null_stream), since the C ABI reads a NULL handle as "restore".  None restores
        the engine's own stream, as ``restore_stream()`` does; before round 6, 0 meant "restore" too, so a
        caller passing 0 for that now gets the null stream -- a warning says so."""
        if stream_handle == 0:
            import warnings
            warnings.warn("Engine.set_stream(0) selects the null stream (torch's default stream); use "
                          "restore_stream() or set_stream(None) for the engine's own stream", stacklevel=2)
            L.check(self.lib.gpdla_engine_use_null_stream(self._h))
        elif stream_handle is None:
            self.restore_stream()
        else:
            L.check(self.lib.gpdla_engine_set_stream(self._h, C.c_void_p(stream_handle)))

    def restore_stream(self) -> None:
        """Back to the engine's own (non-blocking) stream."""
        L.check(self.lib.gpdla_engine_set_stream(self._h, C.c_void_p(0)))

    def set_panel_streams(self, n: int) -> None:
        """Panel-GEMM paths: spectra of a batch alternate over n (1..4) compute streams."""
        L.check(self.lib.gpdla_engine_set_panel_streams(self._h, int(n)))

    def stats(self) -> dict:
        s = L.Stats()
        L.check(self.lib.gpdla_engine_get_stats(self._h, C.byref(s)))
        return {name: getattr(s, name) for name, _ in L.Stats._fields_}

    def reset_stats(self) -> None:
        L.check(self.lib.gpdla_engine_reset_stats(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.lib.gpdla_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def resample(log_likelihoods, uniforms, device: int = 0) -> np.ndarray:
    """The multi-DLA resampler alone (gpdla_resample_f64): for each row of S log likelihoods, the
    index of the smallest i whose weight prefix sum exceeds ``uniforms[j]`` times the total (weights
    exp(l - max), NaN -> 0); -1 throughout a row without a finite positive total.  int32, rows x S."""
    ll = np.ascontiguousarray(np.atleast_2d(log_likelihoods), dtype=np.float64)
    u = np.ascontiguousarray(uniforms, dtype=np.float64).ravel()
    rows, S = ll.shape
    if u.size != S:
        raise ValueError("one uniform per sample")
    out = np.empty((rows, S), dtype=np.int32)
    L.check(L.load().gpdla_resample_f64(device, L.ptr(ll), rows, S, S, L.ptr(u), L.ptr(out, C.c_int32)))
    return out


DEFAULT_INTERVAL_LEVELS = (0.025, 0.16, 0.5, 0.84, 0.975)


def _interval_levels(levels) -> np.ndarray:
    """The quantile levels as the library takes them (it validates their values and their number)."""
    lv = np.ascontiguousarray(DEFAULT_INTERVAL_LEVELS if levels is None else levels, dtype=np.float64).ravel()
    return lv


def posterior_intervals(log_likelihoods, offset_samples, log_nhi_samples, min_z, max_z, base_sample_inds=None,
                        levels=None, lr_delta: float = 2.0, device: int = 0) -> dict:
    """The interval kernel alone (gpdla_posterior_intervals_f64) on host arrays, with ``posterior_summary``'s
    inputs: ``log_likelihoods`` rows x S or levels x rows x S, ``base_sample_inds`` (levels - 1) x rows x S.
    Returns ``Engine.process_intervals``'s interval arrays."""
    ll = np.ascontiguousarray(log_likelihoods, dtype=np.float64)
    if ll.ndim == 2:
        ll = ll[None]
    if ll.ndim != 3:
        raise ValueError("log_likelihoods must be rows x S or levels x rows x S")
    nlv, rows, S = ll.shape
    off = np.ascontiguousarray(offset_samples, dtype=np.float64).ravel()
    lognhi = np.ascontiguousarray(log_nhi_samples, dtype=np.float64).ravel()
    zmin = np.ascontiguousarray(np.broadcast_to(np.asarray(min_z, dtype=np.float64), (rows,)))
    zmax = np.ascontiguousarray(np.broadcast_to(np.asarray(max_z, dtype=np.float64), (rows,)))
    if not off.size == lognhi.size == S:
        raise ValueError("sample arrays must have S entries")
    base = None
    if base_sample_inds is not None:
        base = np.ascontiguousarray(base_sample_inds, dtype=np.int32)
        if base.shape != (max(nlv - 1, 0), rows, S):
            raise ValueError(f"base_sample_inds must be {(nlv - 1, rows, S)}")
    lv = _interval_levels(levels)
    nlq = min(lv.size, L.INTERVAL_MAX_LEVELS)
    ispec = L.IntervalSpec(log_nhi_samples=L.ptr(lognhi), lr_delta=float(lr_delta), num_levels=lv.size)
    for i in range(nlq):
        ispec.levels[i] = lv[i]
    Lc = min(max(nlv, 1), L.MAX_DLAS)
    slot = (nlv, rows, L.MAX_DLAS)
    o = dict(z_dla_means=np.full(slot, np.nan), z_dla_sds=np.full(slot, np.nan), log_nhi_means=np.full(slot, np.nan),
             log_nhi_sds=np.full(slot, np.nan), z_dla_lr_ranges=np.full(slot + (2,), np.nan),
             log_nhi_lr_ranges=np.full(slot + (2,), np.nan), z_dla_quantiles=np.full(slot + (max(nlq, 1),), np.nan),
             log_nhi_quantiles=np.full(slot + (max(nlq, 1),), np.nan), lr_counts=np.zeros((nlv, rows), dtype=np.int32))
    iv = L.Intervals(memory=L.MEM_HOST, z_means=L.ptr(o["z_dla_means"]), z_sds=L.ptr(o["z_dla_sds"]),
                     log_nhi_means=L.ptr(o["log_nhi_means"]), log_nhi_sds=L.ptr(o["log_nhi_sds"]),
                     z_lr_ranges=L.ptr(o["z_dla_lr_ranges"]), log_nhi_lr_ranges=L.ptr(o["log_nhi_lr_ranges"]),
                     z_quantiles=L.ptr(o["z_dla_quantiles"]), log_nhi_quantiles=L.ptr(o["log_nhi_quantiles"]),
                     lr_counts=L.ptr(o["lr_counts"], C.c_int32))
    L.check(L.load().gpdla_posterior_intervals_f64(
        device, L.ptr(ll), rows, S, S, L.ptr(off), L.ptr(lognhi), L.ptr(zmin), L.ptr(zmax),
        L.ptr(base, C.c_int32) if base is not None and base.size else None, nlv, C.byref(ispec), C.byref(iv)))
    out = {k: (v if k == "lr_counts" else np.ascontiguousarray(v[:, :, :Lc])) for k, v in o.items()}
    out["interval_levels"], out["lr_delta"] = lv.copy(), float(lr_delta)
    return out


def posterior_summary(log_likelihoods, offset_samples, log_nhi_samples, nhi_samples, min_z, max_z,
                      base_sample_inds=None, z_edges=None, log_nhi_edges=None, device: int = 0) -> dict:
    """The summary kernel alone (gpdla_posterior_summary_f64) on host arrays: ``log_likelihoods`` is
    rows x S (one level) or levels x rows x S, ``base_sample_inds`` (levels - 1) x rows x S (0-based,
    -1 = none), ``min_z`` / ``max_z`` one per row.  Returns ``Engine.process_summaries``'s summary arrays
    (``map_sample_inds``, ``map_log_likelihoods``, ``MAP_z_dlas``, ``MAP_log_nhis`` and, with a grid,
    ``bin_planes``)."""
    ll = np.ascontiguousarray(log_likelihoods, dtype=np.float64)
    if ll.ndim == 2:
        ll = ll[None]
    if ll.ndim != 3:
        raise ValueError("log_likelihoods must be rows x S or levels x rows x S")
    levels, rows, S = ll.shape
    off = np.ascontiguousarray(offset_samples, dtype=np.float64).ravel()
    lognhi = np.ascontiguousarray(log_nhi_samples, dtype=np.float64).ravel()
    nhi = np.ascontiguousarray(nhi_samples, dtype=np.float64).ravel()
    zmin = np.ascontiguousarray(np.broadcast_to(np.asarray(min_z, dtype=np.float64), (rows,)))
    zmax = np.ascontiguousarray(np.broadcast_to(np.asarray(max_z, dtype=np.float64), (rows,)))
    if not off.size == lognhi.size == nhi.size == S:
        raise ValueError("sample arrays must have S entries")
    base = None
    if base_sample_inds is not None:
        base = np.ascontiguousarray(base_sample_inds, dtype=np.int32)
        if base.shape != (max(levels - 1, 0), rows, S):
            raise ValueError(f"base_sample_inds must be {(levels - 1, rows, S)}")
    if (z_edges is None) != (log_nhi_edges is None):
        raise ValueError("z_edges and log_nhi_edges go together")
    ez = None if z_edges is None else np.ascontiguousarray(z_edges, dtype=np.float64).ravel()
    en = None if log_nhi_edges is None else np.ascontiguousarray(log_nhi_edges, dtype=np.float64).ravel()
    nz, nn = (0, 0) if ez is None else (ez.size - 1, en.size - 1)
    spec = L.SummarySpec(log_nhi_samples=L.ptr(lognhi), num_z_bins=nz, num_nhi_bins=nn, z_edges=L.ptr(ez),
                         log_nhi_edges=L.ptr(en))
    Lc = min(max(levels, 1), L.MAX_DLAS)
    ind = np.full((levels, rows), -1, dtype=np.int32)
    mll = np.full((levels, rows), np.nan)
    mz = np.full((levels, rows, L.MAX_DLAS), np.nan)
    mn = np.full((levels, rows, L.MAX_DLAS), np.nan)
    planes = None if ez is None else np.zeros((rows, L.SUMMARY_PLANES, max(nz, 0), max(nn, 0)))
    L.check(L.load().gpdla_posterior_summary_f64(
        device, L.ptr(ll), rows, S, S, L.ptr(off), L.ptr(lognhi), L.ptr(nhi), L.ptr(zmin), L.ptr(zmax),
        L.ptr(base, C.c_int32) if base is not None and base.size else None, levels, C.byref(spec),
        L.ptr(ind, C.c_int32), L.ptr(mll), L.ptr(mz), L.ptr(mn),
        L.ptr(planes) if planes is not None and planes.size else None))
    out = dict(map_sample_inds=ind, map_log_likelihoods=mll, MAP_z_dlas=np.ascontiguousarray(mz[:, :, :Lc]),
               MAP_log_nhis=np.ascontiguousarray(mn[:, :, :Lc]))
    if planes is not None:
        out["bin_planes"] = planes
    return out


def population_split(log_likelihoods, offset_samples, log_nhi_samples, min_z, max_z, p_dlas, z_edges, log_nhi_edges,
                     p_thresh_sample: float = 1e-4, p_switch: float = 0.25, device: int = 0) -> dict:
    """The split kernel alone (gpdla_population_split_f64) on host arrays: ``log_likelihoods`` rows x S (level
    1), ``min_z`` / ``max_z`` / ``p_dlas`` one per row.  Returns ``Engine.process_population``'s
    ``population_poisson``, ``population_large_inds`` / ``_probs`` / ``_bins``."""
    ll = np.ascontiguousarray(np.atleast_2d(log_likelihoods), dtype=np.float64)
    if ll.ndim != 2:
        raise ValueError("log_likelihoods must be rows x S")
    rows, S = ll.shape
    off = np.ascontiguousarray(offset_samples, dtype=np.float64).ravel()
    lognhi = np.ascontiguousarray(log_nhi_samples, dtype=np.float64).ravel()
    if not off.size == lognhi.size == S:
        raise ValueError("sample arrays must have S entries")
    zmin, zmax, p = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (rows,)))
                     for v in (min_z, max_z, p_dlas))
    ez = np.ascontiguousarray(z_edges, dtype=np.float64).ravel()
    en = np.ascontiguousarray(log_nhi_edges, dtype=np.float64).ravel()
    nz, nn = ez.size - 1, en.size - 1
    spec = L.PopulationSpec(log_nhi_samples=L.ptr(lognhi), num_z_bins=nz, num_nhi_bins=nn, z_edges=L.ptr(ez),
                            log_nhi_edges=L.ptr(en), p_thresh_sample=float(p_thresh_sample), p_switch=float(p_switch),
                            p_thresh_spec=0.05, log_priors_no_dla=None, log_priors_dla=None, log_priors_lls=None)
    NL = L.POPULATION_MAX_LARGE
    plane = np.zeros((rows, max(nz, 1), max(nn, 1)))
    inds, bins = np.full((rows, NL), -1, dtype=np.int32), np.full((rows, NL), -1, dtype=np.int32)
    probs = np.full((rows, NL), np.nan)
    L.check(L.load().gpdla_population_split_f64(
        device, L.ptr(ll), rows, S, S, L.ptr(off), L.ptr(lognhi), L.ptr(zmin), L.ptr(zmax), L.ptr(p), C.byref(spec),
        L.ptr(plane), L.ptr(inds, C.c_int32), L.ptr(probs), L.ptr(bins, C.c_int32)))
    return dict(population_poisson=plane, population_large_inds=inds, population_large_probs=probs,
                population_large_bins=bins)


def _level_rows(log_likelihoods, offset_samples, log_nhi_samples, min_z, max_z, base_sample_inds):
    """The arguments the two stand-alone level kernels share, as contiguous arrays."""
    ll = np.ascontiguousarray(log_likelihoods, dtype=np.float64)
    if ll.ndim == 2:
        ll = ll[None]
    if ll.ndim != 3:
        raise ValueError("log_likelihoods must be rows x S or levels x rows x S")
    levels, rows, S = ll.shape
    off = np.ascontiguousarray(offset_samples, dtype=np.float64).ravel()
    lognhi = np.ascontiguousarray(log_nhi_samples, dtype=np.float64).ravel()
    if not off.size == lognhi.size == S:
        raise ValueError("sample arrays must have S entries")
    zmin = np.ascontiguousarray(np.broadcast_to(np.asarray(min_z, dtype=np.float64), (rows,)))
    zmax = np.ascontiguousarray(np.broadcast_to(np.asarray(max_z, dtype=np.float64), (rows,)))
    base = None
    if base_sample_inds is not None:
        base = np.ascontiguousarray(base_sample_inds, dtype=np.int32)
        if base.shape != (max(levels - 1, 0), rows, S):
            raise ValueError(f"base_sample_inds must be {(levels - 1, rows, S)}")
    return ll, off, lognhi, zmin, zmax, base


def normalise_cuts(cuts):
    """``cuts`` of ``Engine.process_cuts`` / ``process_qsos`` as floats with NaN for off (None stays None).
    ValueError for anything but a dict of ``proximity_zone``, ``noise_thresh`` (and ``omega_m``), for both off, and
    for a negative or non-finite proximity zone."""
    if cuts is None:
        return None
    known = {"proximity_zone", "noise_thresh", "omega_m"}
    if not isinstance(cuts, dict) or set(cuts) - known:
        raise ValueError(f"cuts must be a dict of {sorted(known)}")
    pz, nt = cuts.get("proximity_zone"), cuts.get("noise_thresh")
    pz = np.nan if pz is None else float(pz)
    nt = np.nan if nt is None else float(nt)
    if np.isnan(pz) and np.isnan(nt):
        raise ValueError("cuts with both proximity_zone and noise_thresh off")
    if not np.isnan(pz) and not (0.0 <= pz < np.inf):
        raise ValueError("proximity_zone must be finite and >= 0")
    om = float(cuts.get("omega_m", 0.279))
    if not 0.0 < om <= 1.0:
        raise ValueError("omega_m must lie in (0, 1]")
    return dict(proximity_zone=pz, noise_thresh=nt, omega_m=om)


def search_cuts(wavelengths, noise_variance, min_z, max_z, proximity_zone=None, noise_thresh=None,
                z_edges_summary=None, z_edges_population=None, omega_m: float = 0.279, device: int = 0) -> dict:
    """gpdla_search_cuts_f64: the proximity-zone and noisy-pixel cuts of every spectrum (include/gpdla.h "Search
    cuts").  The two cell lists hold one vector per spectrum (taken as float64); ``None`` turns a cut off.
    Returns ``cut_proximity_zone`` / ``cut_noise_thresh`` (NaN = off), ``cut_z_uppers`` [Q], ``cut_pixel_counts``
    [Q], the good-pixel bitmap ``cut_bitmap_offsets`` [Q + 1] / ``cut_bitmap_words`` (uint32), and per grid
    given ``cut_path_summary`` / ``cut_path_population`` [Q x (nz + 1)]: the path of each z bin, then of the
    grid's whole extent.  The dict is what ``level_planes`` / ``population_split_levels`` take as ``cuts``."""
    cells = [list(wavelengths), list(noise_variance)]
    Q = len(cells[0])
    if len(cells[1]) != Q:
        raise ValueError("one cell per spectrum in each list")
    offsets = np.zeros(Q + 1, dtype=np.int64)
    np.cumsum([np.size(c) for c in cells[0]], out=offsets[1:])
    flat = []
    for lst in cells:
        if any(np.size(c) != offsets[q + 1] - offsets[q] for q, c in enumerate(lst)):
            raise ValueError("a spectrum's two vectors differ in length")
        flat.append(np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float64).ravel() for c in lst])
                                         if Q else np.zeros(0)))
    zmin = np.ascontiguousarray(min_z, dtype=np.float64).ravel()
    zmax = np.ascontiguousarray(max_z, dtype=np.float64).ravel()
    if zmin.size != Q or zmax.size != Q:
        raise ValueError("one min_z and max_z per spectrum")
    pz = np.nan if proximity_zone is None else float(proximity_zone)
    nt = np.nan if noise_thresh is None else float(noise_thresh)
    edges = [None if e is None else np.ascontiguousarray(e, dtype=np.float64).ravel()
             for e in (z_edges_summary, z_edges_population)]
    nzs = [0 if e is None else e.size - 1 for e in edges]
    paths = [None if e is None else np.zeros((Q, max(nz, 0) + 1)) for e, nz in zip(edges, nzs)]
    spec = L.SearchCuts(proximity_zone=pz, noise_thresh=nt, omega_m=float(omega_m), num_z_bins_summary=nzs[0],
                        z_edges_summary=L.ptr(edges[0]), num_z_bins_population=nzs[1],
                        z_edges_population=L.ptr(edges[1]))
    z_uppers = np.zeros(Q)
    counts = np.zeros(Q, dtype=np.int32)
    woff = np.zeros(Q + 1, dtype=np.int64)
    words = np.zeros(int(((np.diff(offsets) + 31) // 32).sum()) if Q else 0, dtype=np.uint32)
    res = L.SearchCutResults(memory=L.MEM_HOST, z_uppers=L.ptr(z_uppers), pixel_counts=L.ptr(counts, C.c_int32),
                             bitmap_offsets=L.ptr(woff, C.c_int64), bitmap_words=L.ptr(words, C.c_uint32),
                             path_summary=L.ptr(paths[0]), path_population=L.ptr(paths[1]))
    L.check(L.load().gpdla_search_cuts_f64(device, Q, L.ptr(offsets, C.c_int64), L.ptr(flat[0]), L.ptr(flat[1]), L.ptr(zmin),
                                           L.ptr(zmax), C.byref(spec), C.byref(res)))
    out = dict(cut_proximity_zone=pz, cut_noise_thresh=nt, cut_z_uppers=z_uppers, cut_pixel_counts=counts,
               cut_bitmap_offsets=woff, cut_bitmap_words=words)
    if paths[0] is not None:
        out["cut_path_summary"] = paths[0]
    if paths[1] is not None:
        out["cut_path_population"] = paths[1]
    return out


def _sample_cuts(cuts, rows: int):
    """gpdla_sample_cuts from ``search_cuts``'s dict, and the arrays it points to."""
    prox = not np.isnan(cuts["cut_proximity_zone"])
    pix = not np.isnan(cuts["cut_noise_thresh"])
    zu = np.ascontiguousarray(cuts["cut_z_uppers"], dtype=np.float64).ravel() if prox else None
    cnt = np.ascontiguousarray(cuts["cut_pixel_counts"], dtype=np.int32).ravel() if pix else None
    woff = np.ascontiguousarray(cuts["cut_bitmap_offsets"], dtype=np.int64).ravel() if pix else None
    words = np.ascontiguousarray(cuts["cut_bitmap_words"], dtype=np.uint32).ravel() if pix else None
    if (zu is not None and zu.size != rows) or (cnt is not None and (cnt.size != rows or woff.size != rows + 1)):
        raise ValueError("cuts must hold one entry per row")
    spec = L.SampleCuts(z_uppers=L.ptr(zu), pixel_counts=L.ptr(cnt, C.c_int32), bitmap_offsets=L.ptr(woff, C.c_int64),
                        bitmap_words=L.ptr(words, C.c_uint32))
    return spec, (zu, cnt, woff, words)


def level_planes(log_likelihoods, offset_samples, log_nhi_samples, nhi_samples, min_z, max_z, z_edges, log_nhi_edges,
                 base_sample_inds=None, device: int = 0, cuts=None) -> np.ndarray:
    """The level-planes kernel alone (gpdla_level_planes_f64) on host arrays, with ``posterior_summary``'s
    inputs: ``log_likelihoods`` levels x rows x S, ``base_sample_inds`` (levels - 1) x rows x S (0-based, -1 =
    none).  Returns ``bin_planes_levels``, rows x levels x 5 x nz x nn.  ``cuts`` (``search_cuts``'s dict, one
    entry per row) applies the sample tests of the search cuts (gpdla_level_planes_cut_f64)."""
    ll, off, lognhi, zmin, zmax, base = _level_rows(log_likelihoods, offset_samples, log_nhi_samples, min_z, max_z,
                                                    base_sample_inds)
    levels, rows, S = ll.shape
    nhi = np.ascontiguousarray(nhi_samples, dtype=np.float64).ravel()
    if nhi.size != S:
        raise ValueError("sample arrays must have S entries")
    ez = np.ascontiguousarray(z_edges, dtype=np.float64).ravel()
    en = np.ascontiguousarray(log_nhi_edges, dtype=np.float64).ravel()
    nz, nn = ez.size - 1, en.size - 1
    spec = L.SummarySpec(log_nhi_samples=L.ptr(lognhi), num_z_bins=nz, num_nhi_bins=nn, z_edges=L.ptr(ez),
                         log_nhi_edges=L.ptr(en))
    planes = np.zeros((rows, levels, L.SUMMARY_PLANES, max(nz, 1), max(nn, 1)))
    bp = L.ptr(base, C.c_int32) if base is not None and base.size else None
    if cuts is None:
        L.check(L.load().gpdla_level_planes_f64(
            device, L.ptr(ll), rows, S, S, L.ptr(off), L.ptr(lognhi), L.ptr(nhi), L.ptr(zmin), L.ptr(zmax), bp, levels,
            C.byref(spec), L.ptr(planes)))
    else:
        cspec, _hold = _sample_cuts(cuts, rows)
        L.check(L.load().gpdla_level_planes_cut_f64(
            device, L.ptr(ll), rows, S, S, L.ptr(off), L.ptr(lognhi), L.ptr(nhi), L.ptr(zmin), L.ptr(zmax), bp, levels,
            C.byref(spec), C.byref(cspec), L.ptr(planes)))
    return planes


def population_split_levels(log_likelihoods, offset_samples, log_nhi_samples, min_z, max_z, level_posteriors, z_edges,
                            log_nhi_edges, base_sample_inds=None, p_thresh_sample: float = 1e-4,
                            p_switch: float = 0.25, device: int = 0, cuts=None) -> dict:
    """The level-split kernel alone (gpdla_population_split_levels_f64) on host arrays: ``log_likelihoods``
    levels x rows x S, ``base_sample_inds`` (levels - 1) x rows x S, ``level_posteriors`` levels x rows (an
    input).  Returns ``Engine.process_levels``'s ``population_level_poisson`` (rows x levels x nz x nn),
    ``population_level_large_inds`` / ``_probs`` (rows x levels x 8) and ``_bins`` (rows x levels x 8 x 4).
    ``cuts`` as in ``level_planes`` (gpdla_population_split_levels_cut_f64)."""
    ll, off, lognhi, zmin, zmax, base = _level_rows(log_likelihoods, offset_samples, log_nhi_samples, min_z, max_z,
                                                    base_sample_inds)
    levels, rows, S = ll.shape
    P = np.ascontiguousarray(level_posteriors, dtype=np.float64).reshape(-1, rows) if rows else np.zeros((levels, 0))
    if P.shape != (levels, rows):
        raise ValueError(f"level_posteriors must be {(levels, rows)}")
    ez = np.ascontiguousarray(z_edges, dtype=np.float64).ravel()
    en = np.ascontiguousarray(log_nhi_edges, dtype=np.float64).ravel()
    nz, nn = ez.size - 1, en.size - 1
    spec = L.PopulationSpec(log_nhi_samples=L.ptr(lognhi), num_z_bins=nz, num_nhi_bins=nn, z_edges=L.ptr(ez),
                            log_nhi_edges=L.ptr(en), p_thresh_sample=float(p_thresh_sample), p_switch=float(p_switch),
                            p_thresh_spec=0.05, log_priors_no_dla=None, log_priors_dla=None, log_priors_lls=None)
    NL = L.POPULATION_MAX_LARGE
    plane = np.zeros((rows, levels, max(nz, 1), max(nn, 1)))
    inds = np.full((rows, levels, NL), -1, dtype=np.int32)
    bins = np.full((rows, levels, NL, L.MAX_DLAS), -1, dtype=np.int32)
    probs = np.full((rows, levels, NL), np.nan)
    bp = L.ptr(base, C.c_int32) if base is not None and base.size else None
    outs = (L.ptr(plane), L.ptr(inds, C.c_int32), L.ptr(probs), L.ptr(bins, C.c_int32))
    if cuts is None:
        L.check(L.load().gpdla_population_split_levels_f64(
            device, L.ptr(ll), rows, S, S, L.ptr(off), L.ptr(lognhi), L.ptr(zmin), L.ptr(zmax), bp, levels, L.ptr(P),
            C.byref(spec), *outs))
    else:
        cspec, _hold = _sample_cuts(cuts, rows)
        L.check(L.load().gpdla_population_split_levels_cut_f64(
            device, L.ptr(ll), rows, S, S, L.ptr(off), L.ptr(lognhi), L.ptr(zmin), L.ptr(zmax), bp, levels, L.ptr(P),
            C.byref(spec), C.byref(cspec), *outs))
    return dict(population_level_poisson=plane, population_level_large_inds=inds, population_level_large_probs=probs,
                population_level_large_bins=bins)


def _bootstrap_spec(Q: int, replicas: int, seed, first_replica: int, stratum_offsets, members):
    """gpdla_bootstrap_spec and the arrays it points to.  ``seed`` is an integer below 2^128 (key words
    seed mod 2^64, seed >> 64) or a pair of 64-bit words; ``stratum_offsets`` / ``members`` None: one stratum
    of all Q spectra."""
    if isinstance(seed, (int, np.integer)):
        seed = (int(seed) & (2 ** 64 - 1), int(seed) >> 64)
    k0, k1 = (int(s) for s in seed)
    if not (0 <= k0 < 2 ** 64 and 0 <= k1 < 2 ** 64):
        raise ValueError("seed must fit 128 bits")
    if members is None:
        stratum_offsets, members = [0, Q], np.arange(Q)
    so = np.ascontiguousarray(stratum_offsets, dtype=np.int64).ravel()
    mem = np.ascontiguousarray(members, dtype=np.int32).ravel()
    if so.size < 2 or so[-1] != mem.size:
        raise ValueError("stratum_offsets must have num_strata + 1 entries ending at len(members)")
    spec = L.BootstrapSpec(seed=(C.c_uint64 * 2)(k0, k1), num_replicas=int(replicas), first_replica=int(first_replica),
                           num_strata=so.size - 1, stratum_offsets=L.ptr(so, C.c_int64), members=L.ptr(mem, C.c_int32))
    return spec, (so, mem)


def bootstrap_counts(Q: int, replicas: int, seed, stratum_offsets=None, members=None, first_replica: int = 0,
                     device: int = 0) -> np.ndarray:
    """gpdla_bootstrap_counts_i32: the multiplicities of ``replicas`` stratified bootstrap replicas of Q
    spectra, replicas x Q int32 (the draw rule is in include/gpdla.h "Bootstrap sample errors")."""
    spec, _hold = _bootstrap_spec(Q, replicas, seed, first_replica, stratum_offsets, members)
    counts = np.empty((max(int(replicas), 0), max(int(Q), 0)), dtype=np.int32)
    L.check(L.load().gpdla_bootstrap_counts_i32(device, int(Q), C.byref(spec), L.ptr(counts, C.c_int32)))
    return counts


def bootstrap_rows(bin_planes, p_dlas, keep=None, p_thresh_spec: float = 0.05, level_posteriors=None, columns: int = 0,
                   device: int = 0) -> np.ndarray:
    """gpdla_bootstrap_rows_f64: per spectrum the four planes ``catalog.cddf_moments`` accumulates -- p A and
    p B - p p C for ``moment=False``, then for ``moment=True`` -- as Q x max(columns, 4 nz nn); the columns past
    4 nz nn are left 0 for the caller (the path terms).  ``bin_planes`` is Q x 5 x nz x nn, or with
    ``level_posteriors`` (Q x D) Q x D x 5 x nz x nn, the row then the sum over the levels."""
    planes = np.ascontiguousarray(bin_planes, dtype=np.float64)
    if level_posteriors is None:
        if planes.ndim != 4 or planes.shape[1] != L.SUMMARY_PLANES:
            raise ValueError("bin_planes must be Q x 5 x nz x nn")
        Q, D, P = planes.shape[0], 1, None
    else:
        if planes.ndim == 4:
            planes = planes[:, None]
        if planes.ndim != 5 or planes.shape[2] != L.SUMMARY_PLANES:
            raise ValueError("bin_planes must be Q x D x 5 x nz x nn")
        Q, D = planes.shape[:2]
        P = np.ascontiguousarray(level_posteriors, dtype=np.float64).reshape(Q, -1)
        if P.shape[1] != D:
            raise ValueError("level_posteriors must be Q x D")
    nz, nn = planes.shape[-2:]
    p = np.ascontiguousarray(p_dlas, dtype=np.float64).ravel()
    if p.size != Q:
        raise ValueError("one p_dla per spectrum")
    k = None if keep is None else np.ascontiguousarray(np.asarray(keep, dtype=bool).ravel(), dtype=np.uint8)
    if k is not None and k.size != Q:
        raise ValueError("one keep flag per spectrum")
    ld = max(int(columns), 4 * nz * nn)
    rows = np.zeros((Q, ld))
    L.check(L.load().gpdla_bootstrap_rows_f64(device, L.ptr(planes), D, L.ptr(p), L.ptr(P), L.ptr(k, C.c_uint8), Q, nz, nn,
                                              float(p_thresh_spec), L.ptr(rows), ld))
    return rows


def bootstrap_sums(counts, rows, device: int = 0) -> np.ndarray:
    """gpdla_bootstrap_sums_f64: ``counts @ rows`` (replicas x Q int32 by Q x N) on the f64 matrix cores, in a
    reduction order over the spectra that is the same for every replica of every call."""
    c = np.ascontiguousarray(counts, dtype=np.int32)
    r = np.ascontiguousarray(rows, dtype=np.float64)
    if c.ndim != 2 or r.ndim != 2 or c.shape[1] != r.shape[0]:
        raise ValueError("counts must be replicas x Q and rows Q x N")
    sums = np.empty((c.shape[0], r.shape[1]))
    L.check(L.load().gpdla_bootstrap_sums_f64(device, L.ptr(c, C.c_int32), L.ptr(r), c.shape[0], c.shape[1], r.shape[1],
                                              L.ptr(sums)))
    return sums


def bootstrap(rows, replicas: int, seed, stratum_offsets=None, members=None, first_replica: int = 0,
              device: int = 0) -> np.ndarray:
    """gpdla_bootstrap_f64: the draws and the sums in one call, the counts never leaving the device; bit for
    bit ``bootstrap_sums(bootstrap_counts(...), rows)``.  Returns replicas x N."""
    r = np.ascontiguousarray(rows, dtype=np.float64)
    if r.ndim != 2:
        raise ValueError("rows must be Q x N")
    spec, _hold = _bootstrap_spec(r.shape[0], replicas, seed, first_replica, stratum_offsets, members)
    sums = np.empty((max(int(replicas), 0), r.shape[1]))
    L.check(L.load().gpdla_bootstrap_f64(device, L.ptr(r), r.shape[0], r.shape[1], C.byref(spec), L.ptr(sums)))
    return sums


def spectrum_snrs(wavelengths, flux, noise_variance, max_z_dlas, normalizers=None, device: int = 0) -> np.ndarray:
    """gpdla_spectrum_snrs_f32 / _f64: ``find_snr`` (calc_cddf.py:906-924) of every spectrum.  The three cell
    lists hold one vector per spectrum, all float32 (the f32 call, float32 result) or anything else (taken as
    float64)."""
    cells = [list(wavelengths), list(flux), list(noise_variance)]
    Q = len(cells[0])
    if not (len(cells[1]) == len(cells[2]) == Q):
        raise ValueError("one cell per spectrum in each list")
    single = Q > 0 and all(np.asarray(c).dtype == np.float32 for lst in cells for c in lst)
    dt, ct = (np.float32, C.c_float) if single else (np.float64, C.c_double)
    offsets = np.zeros(Q + 1, dtype=np.int64)
    np.cumsum([np.size(c) for c in cells[0]], out=offsets[1:])
    flat = []
    for lst in cells:
        if any(np.size(c) != offsets[q + 1] - offsets[q] for q, c in enumerate(lst)):
            raise ValueError("a spectrum's three vectors differ in length")
        flat.append(np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=dt).ravel() for c in lst])
                                         if Q else np.zeros(0, dtype=dt)))
    zmax = np.ascontiguousarray(max_z_dlas, dtype=np.float64).ravel()
    norm = None if normalizers is None else np.ascontiguousarray(normalizers, dtype=np.float64).ravel()
    if zmax.size != Q or (norm is not None and norm.size != Q):
        raise ValueError("one max_z_dla (and normalizer) per spectrum")
    snrs = np.empty(Q, dtype=dt)
    fn = L.load().gpdla_spectrum_snrs_f32 if single else L.load().gpdla_spectrum_snrs_f64
    L.check(fn(device, Q, L.ptr(offsets, C.c_int64), L.ptr(flat[0], ct), L.ptr(flat[1], ct), L.ptr(flat[2], ct), L.ptr(zmax),
               L.ptr(norm), L.ptr(snrs, ct)))
    return snrs


def poisson_binomial_pmf_csr(probs, offsets, device: int = 0) -> np.ndarray:
    """gpdla_poisson_binomial_pmf_f64: the coefficients of prod_j (1 - p_j + p_j x) of every bin of a CSR
    trial list, concatenated (bin b at ``offsets[b] + b``, ``n_b + 1`` values)."""
    p = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    o = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
    if o.size < 1 or o[-1] != p.size:
        raise ValueError("offsets must have nbins + 1 entries ending at len(probs)")
    out = np.empty(p.size + o.size - 1)
    L.check(L.load().gpdla_poisson_binomial_pmf_f64(device, L.ptr(p), L.ptr(o, C.c_int64), o.size - 1, L.ptr(out)))
    return out


def count_mixture_tiling() -> dict:
    """GPDLA_MIX_TILE, GPDLA_MIX_TAPS and GPDLA_MIX_MAX_LEVELS of the loaded library (``tile``, ``taps``,
    ``max_levels``)."""
    v = [C.c_int32() for _ in range(3)]
    L.check(L.load().gpdla_count_mixture_tiling(*(C.byref(x) for x in v)))
    return dict(zip(("tile", "taps", "max_levels"), (x.value for x in v)))


def count_mixture(probs, shifts, tap_offsets, stage_offsets, cells: int, levels, device: int = 0, return_pmf: bool = False):
    """gpdla_count_mixture_f64: per problem (CSR ``stage_offsets`` over stages, ``tap_offsets`` over taps) the
    chain of sparse convolutions next[g] = sum_i probs_i cur[g - shifts_i] on a lattice of ``cells`` entries
    from delta at cell 0, then per level the first cell with cdf >= level (``lower``) and the first occupied
    cell strictly above the first with cdf > level (``upper``).  Returns (lower [P x L] int32, upper, mass [P])
    and, with ``return_pmf``, the final lattices [P x cells]."""
    p = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    raw = np.asarray(shifts).ravel()
    if raw.size and (raw.min() < -2 ** 31 or raw.max() >= 2 ** 31):
        raise ValueError("shifts must fit 32 bits")
    sh = np.ascontiguousarray(raw, dtype=np.int32)
    to = np.ascontiguousarray(tap_offsets, dtype=np.int64).ravel()
    so = np.ascontiguousarray(stage_offsets, dtype=np.int64).ravel()
    lam = np.ascontiguousarray(levels, dtype=np.float64).ravel()
    if so.size < 1 or to.size != so[-1] + 1 or to[-1] != p.size or sh.size != p.size:
        raise ValueError("stage_offsets must have problems + 1 entries ending at the number of stages, tap_offsets "
                         "stages + 1 entries ending at len(probs) == len(shifts)")
    P = so.size - 1
    lower, upper = np.zeros((P, lam.size), dtype=np.int32), np.zeros((P, lam.size), dtype=np.int32)
    mass = np.zeros(P)
    pmf = np.empty((P, int(cells))) if return_pmf and cells >= 1 else None
    L.check(L.load().gpdla_count_mixture_f64(device, L.ptr(p), L.ptr(sh, C.c_int32), L.ptr(to, C.c_int64), L.ptr(so, C.c_int64),
                                             P, int(cells), L.ptr(lam), lam.size, L.ptr(lower, C.c_int32),
                                             L.ptr(upper, C.c_int32), L.ptr(mass), L.ptr(pmf)))
    return (lower, upper, mass, pmf) if return_pmf else (lower, upper, mass)


def forest_optical_depth(wavelengths, z_qso, tau_0, beta, num_forest_lines=31, device: int = 0) -> np.ndarray:
    """sum_i tau_0 c_i (1 + z_i)^beta [z_i <= z_qso] over the first ``num_forest_lines`` Lyman-series lines at
    the observed ``wavelengths`` (gpdla_forest_f64: the device function the engine's forest kernel calls)."""
    wl = np.ascontiguousarray(wavelengths, dtype=np.float64).ravel()
    out = np.empty(wl.size)
    L.check(L.load().gpdla_forest_f64(device, L.ptr(wl), wl.size, float(z_qso), float(tau_0), float(beta),
                                      int(num_forest_lines), L.ptr(out)))
    return out


def voigt(lambdas, z, N, num_lines=31) -> np.ndarray:
    """MEX ``voigt(lambdas, z, N, num_lines)`` (voigt.c:253-304) on the GPU."""
    lib = L.load()
    lam = np.ascontiguousarray(lambdas, dtype=np.float64).ravel()
    out = np.empty(lam.size - 6)
    L.check(lib.gpdla_voigt_f64(L.ptr(lam), lam.size, float(z), float(N), int(num_lines), L.ptr(out)))
    return out


def voigt_batch(lambdas, zs, Ns, num_lines=31) -> np.ndarray:
    lib = L.load()
    lam = np.ascontiguousarray(lambdas, dtype=np.float64).ravel()
    zs = np.ascontiguousarray(zs, dtype=np.float64).ravel()
    Ns = np.ascontiguousarray(Ns, dtype=np.float64).ravel()
    out = np.empty((zs.size, lam.size - 6))
    L.check(lib.gpdla_voigt_batch_f64(L.ptr(lam), lam.size, L.ptr(zs), L.ptr(Ns), zs.size,
                                      int(num_lines), L.ptr(out)))
    return out


def log_mvnpdf_low_rank(y, mu, M, d) -> float:
    """``log_mvnpdf_low_rank(y, mu, M, d)`` (log_mvnpdf_low_rank.m:5-33) on the GPU."""
    lib = L.load()
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    mu = np.ascontiguousarray(mu, dtype=np.float64).ravel()
    d = np.ascontiguousarray(d, dtype=np.float64).ravel()
    M = np.asarray(M, dtype=np.float64)
    if M.ndim == 1:
        M = M[:, None]
    n, k = M.shape
    Mf = np.asfortranarray(M).ravel(order="F")
    out = np.empty(1)
    L.check(lib.gpdla_log_mvnpdf_low_rank_f64(L.ptr(y), L.ptr(mu), L.ptr(Mf), L.ptr(d), n, k, L.ptr(out)))
    return float(out[0])

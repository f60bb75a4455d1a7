"""Time the posterior intervals (gpdla_engine_process_intervals) on BASELINE configs[1]'s shape: 1,024 synthetic
spectra x 10^4 DLA samples, n = 800, k = 20, the five default quantile levels, at max_dlas = 1 and 4, device-resident
inputs, host results, no sample buffers.  Per case: warm-up calls, then ``reps`` timed calls, each giving the
interval launches' time (gpdla_engine_get_interval_stats, HIP events), the level sweeps' time of the same call
(gpdla_engine_get_multi_stats, every level) and the call's wall time.  gpdla_engine_process_summaries -- the call
the intervals are added to, unchanged by them -- is timed at the same shape in the same run, alternating with the
interval call, so the wall-time cost is read off one run on one device.  Prints one JSON line and, with --out,
writes it.  There is no bar: the share of the sweeps is reported.

    python tools/bench_intervals.py [--spectra 1024] [--samples 10000] [--k 20] [--reps 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import DEFAULT_INTERVAL_LEVELS, Engine  # noqa: E402
from gp_dla_detection_amd.parameters import kms_to_z, set_parameters  # noqa: E402


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(mean=float(v.mean()), min=float(v.min()), max=float(v.max()), std=float(v.std()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectra", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--z-bins", type=int, default=12)
    ap.add_argument("--nhi-bins", type=int, default=30)
    ap.add_argument("--max-dlas", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Q, S, dev = a.spectra, a.samples, 0
    model = syn.make_model(k=a.k)
    samples = syn.make_samples(S)
    packed = syn.pack_spectra([syn.make_spectrum(model, q) for q in range(Q)])
    offsets = np.ascontiguousarray(packed["offsets"], dtype=np.int64)
    t = {key: L.DeviceArray.from_numpy(packed[key], device=dev)
         for key in ("wavelengths", "flux", "noise_variance", "pixel_mask", "z_qsos")}
    sp = L.Spectra(memory=L.MEM_DEVICE, num_spectra=Q, offsets=L.ptr(offsets, C.c_int64),
                   wavelengths=L.dev_ptr(t["wavelengths"].ptr), flux=L.dev_ptr(t["flux"].ptr),
                   noise_variance=L.dev_ptr(t["noise_variance"].ptr),
                   pixel_mask=L.dev_ptr(t["pixel_mask"].ptr, C.c_uint8), z_qsos=L.dev_ptr(t["z_qsos"].ptr))
    lognhi = np.ascontiguousarray(samples["log_nhi_samples"], dtype=np.float64)
    ez, en = np.linspace(1.5, 5.5, a.z_bins + 1), np.linspace(20.0, 23.0, a.nhi_bins + 1)
    spec = L.SummarySpec(log_nhi_samples=L.ptr(lognhi), num_z_bins=a.z_bins, num_nhi_bins=a.nhi_bins,
                         z_edges=L.ptr(ez), log_nhi_edges=L.ptr(en))
    levels = np.asarray(DEFAULT_INTERVAL_LEVELS)
    ispec = L.IntervalSpec(log_nhi_samples=L.ptr(lognhi), lr_delta=2.0, num_levels=levels.size)
    for i, lv in enumerate(levels):
        ispec.levels[i] = lv
    rec = dict(what="gpdla_engine_process_intervals: interval launches vs the level sweeps of the same call (HIP events), "
                    "wall time against gpdla_engine_process_summaries in the same run; no sample buffers",
               spectra=Q, samples=S, k=a.k, grid=[a.z_bins, a.nhi_bins], levels=levels.tolist(), lr_delta=2.0, reps=a.reps,
               warmup=a.warmup, runs={})
    with Engine(model, samples, set_parameters(k=a.k), device=dev) as eng:
        for D in a.max_dlas:
            u = eng.default_resample_uniforms(D)
            md = L.MultiDla(max_dlas=D, min_z_separation=kms_to_z(3000), occam_log_penalty=float(np.log(S)),
                            resample_uniforms=L.ptr(u) if u.size else None, forced_base_inds=None)
            null, lld = np.empty(Q), np.empty((D, Q))
            ind, mll = np.empty((D, Q), np.int32), np.empty((D, Q))
            mz, mn = np.empty((D, Q, L.MAX_DLAS)), np.empty((D, Q, L.MAX_DLAS))
            planes = np.empty((Q, L.SUMMARY_PLANES, a.z_bins, a.nhi_bins))
            sm = L.Summaries(memory=L.MEM_HOST, map_sample_inds=L.ptr(ind, C.c_int32), map_log_likelihoods=L.ptr(mll),
                             map_z_dlas=L.ptr(mz), map_log_nhis=L.ptr(mn), bin_planes=L.ptr(planes))
            rs = L.ResultsMulti(memory=L.MEM_HOST, log_likelihoods_no_dla=L.ptr(null), log_likelihoods_dla=L.ptr(lld),
                                sample_log_likelihoods_dla=None, sample_ld=S, base_sample_inds=None, min_z_dlas=None,
                                max_z_dlas=None, num_pixels=None)
            slot = (D, Q, L.MAX_DLAS)
            io = dict(z_means=np.empty(slot), z_sds=np.empty(slot), log_nhi_means=np.empty(slot), log_nhi_sds=np.empty(slot),
                      z_lr_ranges=np.empty(slot + (2,)), log_nhi_lr_ranges=np.empty(slot + (2,)),
                      z_quantiles=np.empty(slot + (levels.size,)), log_nhi_quantiles=np.empty(slot + (levels.size,)))
            counts = np.empty((D, Q), np.int32)
            iv = L.Intervals(memory=L.MEM_HOST, lr_counts=L.ptr(counts, C.c_int32), **{k_: L.ptr(v) for k_, v in io.items()})

            def summaries():
                rc = eng.lib.gpdla_engine_process_summaries(eng._h, C.byref(sp), C.byref(md), C.byref(rs), C.byref(spec),
                                                            C.byref(sm))
                if rc != L.GPDLA_ENUMERIC:
                    L.check(rc)

            def intervals():
                rc = eng.lib.gpdla_engine_process_intervals(eng._h, C.byref(sp), C.byref(md), C.byref(rs), C.byref(spec),
                                                            C.byref(sm), C.byref(ispec), C.byref(iv))
                if rc != L.GPDLA_ENUMERIC:
                    L.check(rc)

            for _ in range(a.warmup):
                summaries()
                intervals()
            i_ms, sweep_ms, s_ms, wall_i, wall_s = [], [], [], [], []
            for _ in range(a.reps):          # alternating, so a drift of the device shows in both
                eng.reset_stats()
                t0 = time.perf_counter()
                summaries()
                wall_s.append((time.perf_counter() - t0) * 1e3)
                lld_s, planes_s = lld.copy(), planes.copy()
                eng.reset_stats()
                t0 = time.perf_counter()
                intervals()
                wall_i.append((time.perf_counter() - t0) * 1e3)
                i_ms.append(eng.interval_stats()["interval_ms"])
                s_ms.append(eng.summary_stats()["summary_ms"])
                sweep_ms.append(float(np.sum(eng.multi_stats()["level_ms"][:D])))
            live = np.isfinite(io["log_nhi_quantiles"][:, :, 0, 2])
            rec["runs"][str(D)] = dict(
                interval_ms=spread(i_ms), level_sweeps_ms=spread(sweep_ms), summary_ms=spread(s_ms),
                interval_over_sweeps=float(np.mean(i_ms) / np.mean(sweep_ms)),
                wall_ms_with_intervals=spread(wall_i), wall_ms_summaries_only=spread(wall_s),
                wall_ratio=float(np.mean(wall_i) / np.mean(wall_s)),
                other_outputs_bitwise_equal=bool(np.array_equal(lld, lld_s, equal_nan=True) and
                                                 np.array_equal(planes, planes_s, equal_nan=True)),
                rows_with_intervals=int(live.sum()), rows=int(live.size),
                median_log_nhi_width_68=float(np.nanmedian(io["log_nhi_quantiles"][0, :, 0, 3] - io["log_nhi_quantiles"][0, :, 0, 1])),
                mean_lr_count_level1=float(counts[0].mean()))
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

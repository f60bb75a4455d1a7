"""Time the posterior summaries (gpdla_engine_process_summaries) on BASELINE configs[1]'s shape: 1,024
synthetic spectra x 10^4 DLA samples, n = 800, k = 20, a 12 x 30 (z, log N_HI) grid, at max_dlas = 1 and
4, device-resident inputs, host results -- once with the sample buffers (the D x Q x S array and the base
indices copied out) and once without (evidences and summaries only).  Per case: warm-up calls, then
``reps`` timed calls, each giving the summary launches' time (gpdla_engine_get_summary_stats, HIP
events), the level-1 likelihood time of the same call (gpdla_engine_get_multi_stats) and the call's wall
time.  The same engine's plain gpdla_engine_process is timed in the same run; ``--bench-likelihood-ms``
records the figure bench.py printed for the commit being compared against.  Prints one JSON line and,
with --out, writes it.  The design target it checks: summaries under 5 % of the level-1 likelihood time.

    python tools/bench_summaries.py [--spectra 1024] [--samples 10000] [--k 20] [--reps 5] [--out FILE]
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
from gp_dla_detection_amd.engine import Engine  # noqa: E402
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
    ap.add_argument("--bench-likelihood-ms", type=float, default=None,
                    help="bench.py's likelihood ms per step of the commit compared against (recorded as given)")
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
    rec = dict(what="gpdla_engine_process_summaries: summary launches vs the level-1 likelihood sweep (HIP events), "
                    "wall time with and without the sample buffers", spectra=Q, samples=S, k=a.k, grid=[a.z_bins, a.nhi_bins],
               reps=a.reps, warmup=a.warmup, bench_py_likelihood_ms_per_step=a.bench_likelihood_ms, runs={})
    o_null, o_n = L.DeviceArray(dev, Q, np.float64), L.DeviceArray(dev, Q, np.int32)
    o_dla, o_s = L.DeviceArray(dev, Q, np.float64), L.DeviceArray(dev, (Q, S), np.float64)
    with Engine(model, samples, set_parameters(k=a.k), device=dev) as eng:
        def plain():
            eng.process_device(offsets, t["wavelengths"].ptr, t["flux"].ptr, t["noise_variance"].ptr,
                               t["pixel_mask"].ptr, t["z_qsos"].ptr, o_null.ptr, o_dla.ptr, o_s.ptr, S, npix_ptr=o_n.ptr)
            eng.synchronize()

        for _ in range(a.warmup + 1):
            plain()
        ms = []
        for _ in range(a.reps):
            eng.reset_stats()
            plain()
            ms.append(eng.stats()["likelihood_ms"])
        rec["process_likelihood_ms"] = spread(ms)
        rec["n_mean"] = float(np.mean(o_n.numpy()))
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
            run, keep = {}, {}
            for label, with_samples in (("with_sample_buffers", True), ("summaries_only", False)):
                sll = np.empty((D, Q, S)) if with_samples else None
                base = np.empty((max(D - 1, 1), Q, S), np.int32) if with_samples and D > 1 else None
                rs = L.ResultsMulti(memory=L.MEM_HOST, log_likelihoods_no_dla=L.ptr(null), log_likelihoods_dla=L.ptr(lld),
                                    sample_log_likelihoods_dla=L.ptr(sll), sample_ld=S,
                                    base_sample_inds=L.ptr(base, C.c_int32), min_z_dlas=None, max_z_dlas=None,
                                    num_pixels=None)

                def call():
                    rc = eng.lib.gpdla_engine_process_summaries(eng._h, C.byref(sp), C.byref(md), C.byref(rs),
                                                                C.byref(spec), C.byref(sm))
                    if rc != L.GPDLA_ENUMERIC:
                        L.check(rc)

                for _ in range(a.warmup):
                    call()
                s_ms, l1_ms, wall = [], [], []
                for _ in range(a.reps):
                    eng.reset_stats()
                    t0 = time.perf_counter()
                    call()
                    wall.append((time.perf_counter() - t0) * 1e3)
                    s_ms.append(eng.summary_stats()["summary_ms"])
                    l1_ms.append(eng.multi_stats()["level_ms"][0])
                keep[label] = (ind.copy(), planes.copy(), lld.copy())
                run[label] = dict(summary_ms=spread(s_ms), level1_likelihood_ms=spread(l1_ms), wall_ms=spread(wall),
                                  summary_over_level1=float(np.mean(s_ms) / np.mean(l1_ms)),
                                  output_bytes=int(sum(x.nbytes for x in (sll, base) if x is not None)))
            a_, b_ = keep["with_sample_buffers"], keep["summaries_only"]
            run["bitwise_equal_with_and_without_samples"] = bool(all(
                np.array_equal(x, y, equal_nan=True) for x, y in zip(a_, b_)))
            run["mass_in_grid_mean"] = float(np.nanmean(planes[:, 0].sum(axis=(1, 2))))
            run["under_5_percent_of_level1"] = bool(run["summaries_only"]["summary_over_level1"] < 0.05)
            rec["runs"][str(D)] = run
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""Time the multi-DLA search (gpdla_engine_process_multi) on BASELINE configs[1]'s shape: 1,024
synthetic spectra x 10^4 DLA samples, n = 800, k = 20, for max_dlas = 1..4, device-resident inputs and
evidences only (no sample array leaves the device).  Per max_dlas: warm-up calls, then ``reps`` timed
calls, each read back through gpdla_engine_get_multi_stats (HIP events): per-level likelihood ms and the
resample ms, with their run-to-run spread; the same engine's plain gpdla_engine_process is timed in
the same run.  Prints one JSON line and, with --out, writes it.

    python tools/bench_multi_dla.py [--spectra 1024] [--samples 10000] [--k 20] [--reps 10] [--out FILE]
"""
import argparse
import ctypes as C
import json
import sys
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-dlas", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Q, S, dev = a.spectra, a.samples, 0
    model = syn.make_model(k=a.k)
    samples = syn.make_samples(S)
    packed = syn.pack_spectra([syn.make_spectrum(model, q) for q in range(Q)])
    offsets = np.ascontiguousarray(packed["offsets"], dtype=np.int64)
    t = {key: L.DeviceArray.from_numpy(packed[key], device=dev)
         for key in ("wavelengths", "flux", "noise_variance", "pixel_mask", "z_qsos")}
    o_null, o_n = L.DeviceArray(dev, Q, np.float64), L.DeviceArray(dev, Q, np.int32)
    o_dla = L.DeviceArray(dev, (a.max_dlas, Q), np.float64)
    o_s = L.DeviceArray(dev, (Q, S), np.float64)          # plain process only
    sp = L.Spectra(memory=L.MEM_DEVICE, num_spectra=Q, offsets=L.ptr(offsets, C.c_int64),
                   wavelengths=L.dev_ptr(t["wavelengths"].ptr), flux=L.dev_ptr(t["flux"].ptr),
                   noise_variance=L.dev_ptr(t["noise_variance"].ptr),
                   pixel_mask=L.dev_ptr(t["pixel_mask"].ptr, C.c_uint8), z_qsos=L.dev_ptr(t["z_qsos"].ptr))
    rs = L.ResultsMulti(memory=L.MEM_DEVICE, log_likelihoods_no_dla=L.dev_ptr(o_null.ptr),
                        log_likelihoods_dla=L.dev_ptr(o_dla.ptr), sample_log_likelihoods_dla=None, sample_ld=S,
                        base_sample_inds=None, min_z_dlas=None, max_z_dlas=None,
                        num_pixels=L.dev_ptr(o_n.ptr, C.c_int32))
    rec = dict(what="gpdla_engine_process_multi, per-level kernel ms (HIP events)", spectra=Q, samples=S, k=a.k,
               reps=a.reps, warmup=a.warmup, runs={})
    with Engine(model, samples, set_parameters(k=a.k), device=dev) as eng:
        def plain():
            eng.process_device(offsets, t["wavelengths"].ptr, t["flux"].ptr, t["noise_variance"].ptr,
                               t["pixel_mask"].ptr, t["z_qsos"].ptr, o_null.ptr, o_dla.ptr, o_s.ptr, S, npix_ptr=o_n.ptr)
            eng.synchronize()

        for _ in range(a.warmup):
            plain()
        ms = []
        for _ in range(a.reps):
            eng.reset_stats()
            plain()
            ms.append(eng.stats()["likelihood_ms"])
        rec["process_likelihood_ms"] = spread(ms)
        rec["n_mean"] = float(np.mean(o_n.numpy()))
        for D in range(1, a.max_dlas + 1):
            u = eng.default_resample_uniforms(D)
            md = L.MultiDla(max_dlas=D, min_z_separation=kms_to_z(3000), occam_log_penalty=float(np.log(S)),
                            resample_uniforms=L.ptr(u) if u.size else None, forced_base_inds=None)

            def multi():
                rc = eng.lib.gpdla_engine_process_multi(eng._h, C.byref(sp), C.byref(md), C.byref(rs))
                if rc != L.GPDLA_ENUMERIC:
                    L.check(rc)

            for _ in range(a.warmup):
                multi()
            levels, res, red = [], [], []
            for _ in range(a.reps):
                eng.reset_stats()
                multi()
                st = eng.multi_stats()
                levels.append(st["level_ms"][:D])
                res.append(st["resample_ms"])
                red.append(st["multi_reduce_ms"])
            levels = np.asarray(levels)
            lld = o_dla.numpy()[:D]
            rec["runs"][str(D)] = dict(level_ms=[spread(levels[:, d]) for d in range(D)], resample_ms=spread(res),
                                       multi_reduce_ms=spread(red),
                                       finite_evidences=[int(np.isfinite(lld[d]).sum()) for d in range(D)])
        # the plain call once more, after the deepest run (separates drift of the box from the call)
        ms = []
        for _ in range(a.reps):
            eng.reset_stats()
            plain()
            ms.append(eng.stats()["likelihood_ms"])
        rec["process_likelihood_ms_after"] = spread(ms)
    # the two statements to check: level 1 is gpdla_engine_process's kernel (equal within the run's
    # spread), and level d costs at most d x level 1 -- per max_dlas, each against its own call's level 1
    p = rec["process_likelihood_ms"]
    rec["level1_vs_process"], rec["level_over_level1"], rec["level_d_at_most_d_times_level1"] = {}, {}, {}
    for D, run in rec["runs"].items():
        l1 = run["level_ms"][0]
        sp_ms = max(l1["max"] - l1["min"], p["max"] - p["min"])
        rec["level1_vs_process"][D] = dict(diff_ms=l1["mean"] - p["mean"], spread_ms=sp_ms,
                                           within_spread=bool(abs(l1["mean"] - p["mean"]) <= sp_ms))
        rec["level_over_level1"][D] = [lv["mean"] / l1["mean"] for lv in run["level_ms"]]
        rec["level_d_at_most_d_times_level1"][D] = [bool(lv["mean"] <= (d + 1) * l1["mean"])
                                                    for d, lv in enumerate(run["level_ms"])]
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""Time the level-population launches (gpdla_engine_process_levels) on BASELINE configs[1]'s shape: 1,024
synthetic spectra x 10^4 DLA samples, n = 800, k = 20, device-resident inputs and outputs (no sample array
leaves the device), on the reference's grid (12 z bins x 27 log N_HI bins) for both the planes and the split,
at max_dlas = 2, 3, 4.  Warm-up calls, then ``reps`` timed calls per max_dlas, each read back through the
engine's HIP-event accounting: the level planes + level posteriors + level split launches (one span) against
the sum of the level sweeps of the same call (gpdla_engine_get_multi_stats), next to the existing level-1
summary and population launches; mean with max - min.  Prints one JSON line and, with --out, writes it.

    python tools/bench_population_levels.py [--spectra 1024] [--samples 10000] [--k 20] [--reps 10] [--out FILE]
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
    return dict(mean=float(v.mean()), min=float(v.min()), max=float(v.max()), std=float(v.std()),
                max_minus_min=float(v.max() - v.min()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectra", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-dlas", type=int, nargs="+", default=[2, 3, 4])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Q, S, dev = a.spectra, a.samples, 0
    model = syn.make_model(k=a.k)
    samples = syn.make_samples(S)
    packed = syn.pack_spectra([syn.make_spectrum(model, q) for q in range(Q)])
    offsets = np.ascontiguousarray(packed["offsets"], dtype=np.int64)
    t = {key: L.DeviceArray.from_numpy(packed[key], device=dev)
         for key in ("wavelengths", "flux", "noise_variance", "pixel_mask", "z_qsos")}
    ez, en = np.linspace(2.0, 4.0, 13), np.linspace(20.3, 23.0, 28)
    nz, nn, NL, MD = ez.size - 1, en.size - 1, L.POPULATION_MAX_LARGE, L.MAX_DLAS
    lognhi = np.ascontiguousarray(samples["log_nhi_samples"], dtype=np.float64)
    sp = L.Spectra(memory=L.MEM_DEVICE, num_spectra=Q, offsets=L.ptr(offsets, C.c_int64),
                   wavelengths=L.dev_ptr(t["wavelengths"].ptr), flux=L.dev_ptr(t["flux"].ptr),
                   noise_variance=L.dev_ptr(t["noise_variance"].ptr),
                   pixel_mask=L.dev_ptr(t["pixel_mask"].ptr, C.c_uint8), z_qsos=L.dev_ptr(t["z_qsos"].ptr))
    rec = dict(what="gpdla_engine_process_levels: level planes + posteriors + split launches vs the sum of the level "
                    "sweeps of the same call (HIP events, ms)",
               spectra=Q, samples=S, k=a.k, reps=a.reps, warmup=a.warmup, grid=[nz, nn], max_dlas={})
    with Engine(model, samples, set_parameters(k=a.k), device=dev) as eng:
        for D in a.max_dlas:
            def arr(shape, dtype=np.float64):
                return L.DeviceArray(dev, shape, dtype)
            o = dict(null=arr(Q), npix=arr(Q, np.int32), dla=arr((D, Q)), mi=arr((D, Q), np.int32), ml=arr((D, Q)),
                     mz=arr((D, Q, MD)), mn=arr((D, Q, MD)), planes=arr((Q, 5, nz, nn)), plane=arr((Q, nz, nn)),
                     li=arr((Q, NL), np.int32), lp=arr((Q, NL)), lb=arr((Q, NL), np.int32), p=arr(Q),
                     vpost=arr((D, Q)), vplanes=arr((Q, D, 5, nz, nn)), vplane=arr((Q, D, nz, nn)),
                     vli=arr((Q, D, NL), np.int32), vlp=arr((Q, D, NL)), vlb=arr((Q, D, NL, MD), np.int32))

            def dp(key, ctype=C.c_double):
                return L.dev_ptr(o[key].ptr, ctype)
            rs = L.ResultsMulti(memory=L.MEM_DEVICE, log_likelihoods_no_dla=dp("null"), log_likelihoods_dla=dp("dla"),
                                sample_log_likelihoods_dla=None, sample_ld=S, base_sample_inds=None, min_z_dlas=None,
                                max_z_dlas=None, num_pixels=dp("npix", C.c_int32))
            u = eng.default_resample_uniforms(D)
            md = L.MultiDla(max_dlas=D, min_z_separation=kms_to_z(3000), occam_log_penalty=float(np.log(S)),
                            resample_uniforms=L.ptr(u), forced_base_inds=None)
            ss = L.SummarySpec(log_nhi_samples=L.ptr(lognhi), num_z_bins=nz, num_nhi_bins=nn, z_edges=L.ptr(ez),
                               log_nhi_edges=L.ptr(en))
            sm = L.Summaries(memory=L.MEM_DEVICE, map_sample_inds=dp("mi", C.c_int32), map_log_likelihoods=dp("ml"),
                             map_z_dlas=dp("mz"), map_log_nhis=dp("mn"), bin_planes=dp("planes"))
            lp_no = np.full(Q, np.log(0.9))
            lp_dla = np.ascontiguousarray(np.tile(np.log([0.1 ** d - 0.1 ** (d + 1) for d in range(1, D)] + [0.1 ** D]), (Q, 1)).T)
            ps = L.PopulationSpec(log_nhi_samples=L.ptr(lognhi), num_z_bins=nz, num_nhi_bins=nn, z_edges=L.ptr(ez),
                                  log_nhi_edges=L.ptr(en), p_thresh_sample=1e-4, p_switch=0.25, p_thresh_spec=0.05,
                                  log_priors_no_dla=L.ptr(lp_no), log_priors_dla=L.ptr(lp_dla), log_priors_lls=None)
            po = L.Population(memory=L.MEM_DEVICE, poisson_plane=dp("plane"), large_inds=dp("li", C.c_int32),
                              large_probs=dp("lp"), large_bins=dp("lb", C.c_int32), p_dlas=dp("p"))
            lv = L.LevelPopulation(memory=L.MEM_DEVICE, level_posteriors=dp("vpost"), bin_planes=dp("vplanes"),
                                   poisson_plane=dp("vplane"), large_inds=dp("vli", C.c_int32), large_probs=dp("vlp"),
                                   large_bins=dp("vlb", C.c_int32))

            def call(on):
                rc = eng.lib.gpdla_engine_process_levels(eng._h, C.byref(sp), C.byref(md), None, C.byref(rs), None, C.byref(ss),
                                                         C.byref(sm), C.byref(ps), C.byref(po), C.byref(lv) if on else None)
                if rc != L.GPDLA_ENUMERIC:
                    L.check(rc)

            for _ in range(a.warmup):
                call(True)
            cols = {key: [] for key in ("sweeps_ms", "level_population_ms", "summary_ms", "population_ms", "sweeps_ms_without")}
            for _ in range(a.reps):
                for on in (False, True):
                    eng.reset_stats()
                    call(on)
                    ms, lst = eng.multi_stats(), eng.level_population_stats()
                    assert lst["level_population_launches"] == (1 if on else 0)
                    sweeps = float(sum(ms["level_ms"][:D]))
                    if on:
                        cols["sweeps_ms"].append(sweeps)
                        cols["level_population_ms"].append(lst["level_population_ms"])
                        cols["summary_ms"].append(eng.summary_stats()["summary_ms"])
                        cols["population_ms"].append(eng.population_stats()["population_ms"])
                    else:
                        cols["sweeps_ms_without"].append(sweeps)
            r = {key: spread(v) for key, v in cols.items()}
            r["level_ms"] = [float(x) for x in ms["level_ms"][:D]]
            r["level_population_over_sweeps"] = r["level_population_ms"]["mean"] / r["sweeps_ms"]["mean"]
            P = o["vpost"].numpy()
            r["finite_level_posteriors"] = int(np.isfinite(P).sum())
            r["mean_level_posteriors"] = [float(np.nanmean(P[d])) for d in range(D)]
            r["large_samples"] = [int((o["vli"].numpy()[:, d] >= 0).sum()) for d in range(D)]
            r["poisson_mass"] = [float(o["vplane"].numpy()[:, d].sum()) for d in range(D)]
            r["plane_mass"] = [float(o["vplanes"].numpy()[:, d, 0].sum()) for d in range(D)]
            r["level1_planes_equal_bin_planes"] = bool(np.array_equal(o["vplanes"].numpy()[:, 0], o["planes"].numpy()))
            rec["max_dlas"][str(D)] = r
            for v in o.values():
                v.free()
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

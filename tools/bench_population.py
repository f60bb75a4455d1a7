"""Time the population launches (gpdla_engine_process_population) on BASELINE configs[1]'s shape: 1,024
synthetic spectra x 10^4 DLA samples, n = 800, k = 20, max_dlas = 1, device-resident inputs and outputs (no
sample array leaves the device), on the reference's grid (12 z bins x 27 log N_HI bins).  Warm-up calls, then
``reps`` timed calls with and without the population structs, alternating, each read back through the
engine's HIP-event accounting: the posterior + split launches against the level-1 sweep of the same call, and
the level-1 sweep of the calls without them (the call as it was before); mean with max - min.  Then the
Poisson-binomial pmf kernel at one bin of ``--trials`` trials (gpdla_last_call_kernel_ms: the chunk launch
and the fold launches).  Prints one JSON line and, with --out, writes it.

    python tools/bench_population.py [--spectra 1024] [--samples 10000] [--k 20] [--reps 10] [--out FILE]
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
from gp_dla_detection_amd.engine import Engine, poisson_binomial_pmf_csr  # noqa: E402
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
    ap.add_argument("--trials", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Q, S, dev = a.spectra, a.samples, 0
    model = syn.make_model(k=a.k)
    samples = syn.make_samples(S)
    packed = syn.pack_spectra([syn.make_spectrum(model, q) for q in range(Q)])
    offsets = np.ascontiguousarray(packed["offsets"], dtype=np.int64)
    t = {key: L.DeviceArray.from_numpy(packed[key], device=dev)
         for key in ("wavelengths", "flux", "noise_variance", "pixel_mask", "z_qsos")}
    o_null, o_n, o_dla = L.DeviceArray(dev, Q, np.float64), L.DeviceArray(dev, Q, np.int32), L.DeviceArray(dev, (1, Q), np.float64)
    ez, en = np.linspace(2.0, 4.0, 13), np.linspace(20.3, 23.0, 28)
    NL = L.POPULATION_MAX_LARGE
    o_plane = L.DeviceArray(dev, (Q, ez.size - 1, en.size - 1), np.float64)
    o_li, o_lb = L.DeviceArray(dev, (Q, NL), np.int32), L.DeviceArray(dev, (Q, NL), np.int32)
    o_lp, o_p = L.DeviceArray(dev, (Q, NL), np.float64), L.DeviceArray(dev, Q, np.float64)
    sp = L.Spectra(memory=L.MEM_DEVICE, num_spectra=Q, offsets=L.ptr(offsets, C.c_int64),
                   wavelengths=L.dev_ptr(t["wavelengths"].ptr), flux=L.dev_ptr(t["flux"].ptr),
                   noise_variance=L.dev_ptr(t["noise_variance"].ptr),
                   pixel_mask=L.dev_ptr(t["pixel_mask"].ptr, C.c_uint8), z_qsos=L.dev_ptr(t["z_qsos"].ptr))
    rs = L.ResultsMulti(memory=L.MEM_DEVICE, log_likelihoods_no_dla=L.dev_ptr(o_null.ptr),
                        log_likelihoods_dla=L.dev_ptr(o_dla.ptr), sample_log_likelihoods_dla=None, sample_ld=S,
                        base_sample_inds=None, min_z_dlas=None, max_z_dlas=None,
                        num_pixels=L.dev_ptr(o_n.ptr, C.c_int32))
    md = L.MultiDla(max_dlas=1, min_z_separation=kms_to_z(3000), occam_log_penalty=float(np.log(S)),
                    resample_uniforms=None, forced_base_inds=None)
    lognhi = np.ascontiguousarray(samples["log_nhi_samples"], dtype=np.float64)
    lp_no, lp_dla = np.full(Q, np.log(0.9)), np.full(Q, np.log(0.1))
    ps = L.PopulationSpec(log_nhi_samples=L.ptr(lognhi), num_z_bins=ez.size - 1, num_nhi_bins=en.size - 1,
                          z_edges=L.ptr(ez), log_nhi_edges=L.ptr(en), p_thresh_sample=1e-4, p_switch=0.25,
                          p_thresh_spec=0.05, log_priors_no_dla=L.ptr(lp_no), log_priors_dla=L.ptr(lp_dla),
                          log_priors_lls=None)
    po = L.Population(memory=L.MEM_DEVICE, poisson_plane=L.dev_ptr(o_plane.ptr), large_inds=L.dev_ptr(o_li.ptr, C.c_int32),
                      large_probs=L.dev_ptr(o_lp.ptr), large_bins=L.dev_ptr(o_lb.ptr, C.c_int32), p_dlas=L.dev_ptr(o_p.ptr))
    rec = dict(what="gpdla_engine_process_population: posterior + split launches vs the level-1 sweep (HIP events, ms); "
                    "gpdla_poisson_binomial_pmf_f64 at one bin",
               spectra=Q, samples=S, k=a.k, reps=a.reps, warmup=a.warmup, grid=[ez.size - 1, en.size - 1])
    with Engine(model, samples, set_parameters(k=a.k), device=dev) as eng:
        def call(on):
            rc = eng.lib.gpdla_engine_process_population(eng._h, C.byref(sp), C.byref(md), None, C.byref(rs), None, None,
                                                         None, C.byref(ps) if on else None, C.byref(po) if on else None)
            if rc != L.GPDLA_ENUMERIC:
                L.check(rc)

        for _ in range(a.warmup):
            call(False)
            call(True)
        cols = {key: [] for key in ("level1_ms_without", "level1_ms_with", "population_ms")}
        for _ in range(a.reps):
            for on in (False, True):
                eng.reset_stats()
                call(on)
                st, pst = eng.stats(), eng.population_stats()
                assert st["sample_evals"] == Q * S and pst["population_launches"] == (1 if on else 0)
                cols["level1_ms_with" if on else "level1_ms_without"].append(st["likelihood_ms"])
                if on:
                    cols["population_ms"].append(pst["population_ms"])
        rec.update({key: spread(v) for key, v in cols.items()})
        rec["population_over_level1"] = rec["population_ms"]["mean"] / rec["level1_ms_without"]["mean"]
        p = o_p.numpy()
        rec["finite_p_dlas"] = int(np.isfinite(p).sum())
        rec["spectra_above_p_thresh_spec"] = int((p > 0.05).sum())
        rec["large_samples"] = int((o_li.numpy() >= 0).sum())
        rec["poisson_mass"] = float(o_plane.numpy().sum())
        rec["n_mean"] = float(np.mean(o_n.numpy()))
    rng = np.random.default_rng(1)
    probs = rng.uniform(0.25, 1.0, a.trials)
    off = np.array([0, a.trials], dtype=np.int64)
    chunk, fold = [], []
    for i in range(a.warmup + a.reps):
        pmf = poisson_binomial_pmf_csr(probs, off, device=dev)
        ms = L.last_call_kernel_ms()
        if i >= a.warmup:
            chunk.append(ms[0])
            fold.append(ms[1] if len(ms) > 1 else 0.0)
    rec["pmf"] = dict(trials=a.trials, chunk=L.PMF_CHUNK, chunk_launch_ms=spread(chunk), fold_launches_ms=spread(fold),
                      fold_launches=max(0, -(-a.trials // L.PMF_CHUNK) - 1),
                      total_ms=spread(np.asarray(chunk) + np.asarray(fold)), sum_minus_one=float(pmf.sum() - 1.0))
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

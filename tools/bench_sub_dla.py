"""Time the sub-DLA sweep and the forest kernel (gpdla_engine_process_models, gpdla_engine_set_forest) on
BASELINE configs[1]'s shape: 1,024 synthetic spectra x 10^4 DLA samples, n = 800, k = 20, max_dlas = 1,
device-resident inputs and evidences only (no sample array leaves the device).  Warm-up calls, then
``reps`` timed calls with the forest on and the sub-DLA model on, each read back through the engine's
HIP-event accounting: the sub-DLA sweep against the level-1 sweep of the same call, and the forest kernel
against prep_ms of the same call; mean with max - min.  The same calls without the forest are timed in the
same run (the sweep itself does not depend on it).  Prints one JSON line and, with --out, writes it.

With --scope (mu_M or all) the arms are instead the forest under mean_flux_scope "mu" (the baseline) and
under that scope, alternated twice within the run.  forest_ms then sums forest_kernel and
forest_covariance_kernel (two launches per batch); the new launch's time is reported as the difference
of the arms' forest_ms means, next to prep_ms and the level-1 and sub-DLA sweeps of both arms.

    python tools/bench_sub_dla.py [--spectra 1024] [--samples 10000] [--k 20] [--reps 10] [--scope all] [--out FILE]
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import dla_samples as DS  # noqa: E402
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
    ap.add_argument("--scope", default=None, choices=("mu_M", "all"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Q, S, dev = a.spectra, a.samples, 0
    model = syn.make_model(k=a.k)
    samples = syn.make_samples(S)
    sub_nhi = np.ascontiguousarray(DS.sub_dla_samples(S, u=syn.halton(S, 3))["lls_nhi_samples"])
    packed = syn.pack_spectra([syn.make_spectrum(model, q) for q in range(Q)])
    offsets = np.ascontiguousarray(packed["offsets"], dtype=np.int64)
    t = {key: L.DeviceArray.from_numpy(packed[key], device=dev)
         for key in ("wavelengths", "flux", "noise_variance", "pixel_mask", "z_qsos")}
    o_null, o_n = L.DeviceArray(dev, Q, np.float64), L.DeviceArray(dev, Q, np.int32)
    o_dla, o_sub = L.DeviceArray(dev, (1, Q), np.float64), L.DeviceArray(dev, Q, np.float64)
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
    sub = L.SubDla(nhi_samples=L.ptr(sub_nhi))
    rsub = L.ResultsSub(memory=L.MEM_DEVICE, log_likelihoods_lls=L.dev_ptr(o_sub.ptr), sample_ld=S)
    rec = dict(what="gpdla_engine_process_models: sub-DLA sweep vs level 1, forest kernel vs prep (HIP events, ms)",
               spectra=Q, samples=S, k=a.k, reps=a.reps, warmup=a.warmup, runs={})
    with Engine(model, samples, set_parameters(k=a.k), device=dev) as eng:
        def call():
            rc = eng.lib.gpdla_engine_process_models(eng._h, C.byref(sp), C.byref(md), C.byref(sub), C.byref(rs),
                                                     C.byref(rsub), None, None)
            if rc != L.GPDLA_ENUMERIC:
                L.check(rc)

        arms = (("forest_off", None), ("forest_on", True), ("forest_off_after", None))
        if a.scope:
            mu, scoped = dict(mean_flux_scope="mu"), dict(mean_flux_scope=a.scope)
            arms = (("scope_mu", mu), (f"scope_{a.scope}", scoped), ("scope_mu_again", mu), (f"scope_{a.scope}_again", scoped))
            rec["scope"] = a.scope
        for name, forest in arms:
            launches = 0 if not forest else 2 if forest is not True and forest["mean_flux_scope"] != "mu" else 1
            eng.set_forest(forest)
            for _ in range(a.warmup):
                call()
            cols = {key: [] for key in ("level1_ms", "sub_dla_ms", "sub_dla_reduce_ms", "prep_ms", "forest_ms", "reduce_ms")}
            for _ in range(a.reps):
                eng.reset_stats()
                call()
                st, ms = eng.stats(), eng.model_stats()
                cols["level1_ms"].append(st["likelihood_ms"])
                cols["prep_ms"].append(st["prep_ms"])
                cols["reduce_ms"].append(st["reduce_ms"])
                for key in ("sub_dla_ms", "sub_dla_reduce_ms", "forest_ms"):
                    cols[key].append(ms[key])
                assert st["sample_evals"] == Q * S and ms["sub_dla_launches"] == 1
                assert ms["forest_launches"] == launches
            run = {key: spread(v) for key, v in cols.items()}
            ratios = np.asarray(cols["sub_dla_ms"]) / np.asarray(cols["level1_ms"])
            l1, sd = run["level1_ms"], run["sub_dla_ms"]
            sp_ms = max(l1["max_minus_min"], sd["max_minus_min"])
            run["sub_dla_over_level1"] = dict(mean=sd["mean"] / l1["mean"], per_call=spread(ratios),
                                              diff_ms=sd["mean"] - l1["mean"], spread_ms=sp_ms,
                                              within_spread=bool(abs(sd["mean"] - l1["mean"]) <= sp_ms))
            if forest:
                run["forest_over_prep"] = run["forest_ms"]["mean"] / run["prep_ms"]["mean"]
                run["forest_over_level1"] = run["forest_ms"]["mean"] / l1["mean"]
            run["finite_sub_evidences"] = int(np.isfinite(o_sub.numpy()).sum())
            run["finite_dla_evidences"] = int(np.isfinite(o_dla.numpy()).sum())
            rec["runs"][name] = run
        if a.scope:
            runs, sc = rec["runs"], f"scope_{a.scope}"
            mean2 = lambda arm, key: 0.5 * (runs[arm][key]["mean"] + runs[arm + "_again"][key]["mean"])  # noqa: E731
            cov = mean2(sc, "forest_ms") - mean2("scope_mu", "forest_ms")
            rec["covariance_kernel"] = dict(ms=cov, over_prep=cov / mean2("scope_mu", "prep_ms"),
                                            over_level1=cov / mean2("scope_mu", "level1_ms"))
            for key in ("level1_ms", "sub_dla_ms"):
                diff = mean2(sc, key) - mean2("scope_mu", key)
                sp_ms = max(runs[arm][key]["max_minus_min"] for arm in runs)
                rec[key + "_scope_minus_mu"] = dict(diff_ms=diff, spread_ms=sp_ms, within_spread=bool(abs(diff) <= sp_ms))
        rec["n_mean"] = float(np.mean(o_n.numpy()))
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

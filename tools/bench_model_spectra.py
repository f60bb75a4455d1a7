"""Time the model-spectra launch (gpdla_engine_model_spectra).

Part 1, BASELINE configs[1]'s shape: 1,024 synthetic spectra x 10^4 DLA samples, n = 800, k = 20.  Per repetition the
level-1 sweep (gpdla_engine_process, no sample array) and the model-spectra call with 1 and with 4 absorbers per
spectrum run on the same engine; each is read back through the engine's HIP-event accounting, so the model launch
is compared with the sweep the same engine just ran.  ``reps`` repetitions after ``warmup``.

Part 1b, the same launch inside the search call (Engine.process_model_spectra, level="best", device-resident
spectra) at max_dlas 1 and 4, against the level-1 sweep and all sweeps of that call.

Part 2, the stand-alone entry at ``--survey-spectra`` spectra (the part-1 spectra repeated): kernel time by HIP
events, the call's wall time, and the achieved bytes per second against the panel bytes the kernel must read (two
passes over n rows of Layout<k>::kRow doubles: 1,920 B per row at k = 20).

    python tools/bench_model_spectra.py [--reps 5] [--survey-spectra 8192] [--out FILE]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import Engine  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(mean=float(v.mean()), min=float(v.min()), max=float(v.max()), std=float(v.std()))


def panel_row_bytes(k: int) -> int:
    """Layout<k>::kRow doubles (csrc/internal.h), in bytes."""
    tiles = (k * (k + 1) // 2 + 3) // 4 + (k + 3) // 4
    return 8 * 4 * (((tiles + 2) + 1) & ~1)


def absorbers(Q: int, count: int, z_lo, z_hi):
    f = np.array([0.2, 0.45, 0.6, 0.85])[:count]
    z = z_lo[:, None] + (z_hi - z_lo)[:, None] * f[None, :]
    return z, np.tile(np.array([20.5, 21.0, 20.3, 21.5])[:count], (Q, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectra", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--survey-spectra", type=int, default=8192)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Q, S = a.spectra, a.samples
    model = syn.make_model(k=a.k)
    samples = syn.make_samples(S)
    spectra = [syn.make_spectrum(model, q) for q in range(Q)]
    packed = syn.pack_spectra(spectra)
    rec = dict(what="gpdla_engine_model_spectra: the model launch vs the level-1 sweep on the same engine (HIP events, ms)",
               spectra=Q, samples=S, k=a.k, pixels=int(packed["offsets"][-1]), reps=a.reps, warmup=a.warmup,
               panel_row_bytes=panel_row_bytes(a.k))
    cols = dict(sweep_ms=[], model_ms_1=[], model_ms_4=[])
    with Engine(model, samples, set_parameters(k=a.k)) as eng:
        for i in range(a.warmup + a.reps):
            eng.reset_stats()
            sweep = eng.process(packed, want_samples=False)
            sweep_ms = eng.stats()["likelihood_ms"]
            ms = {}
            for count in (1, 4):
                eng.reset_stats()
                z, ln = absorbers(Q, count, sweep["min_z_dlas"], sweep["max_z_dlas"])
                out = eng.model_spectra(packed, z, ln)
                ms[count] = eng.model_spectra_stats()["model_spectra_ms"]
            if i >= a.warmup:
                cols["sweep_ms"].append(sweep_ms)
                cols["model_ms_1"].append(ms[1])
                cols["model_ms_4"].append(ms[4])
        n_total = int(out["num_pixels"].sum())
        rec["likelihood_pixels"] = n_total
        rec.update({key: spread(v) for key, v in cols.items()})
        must_read = 2.0 * n_total * panel_row_bytes(a.k)
        for count in (1, 4):
            best = rec[f"model_ms_{count}"]["min"]
            rec[f"model_over_sweep_{count}"] = rec[f"model_ms_{count}"]["mean"] / rec["sweep_ms"]["mean"]
            rec[f"gb_per_s_{count}"] = must_read / (best * 1e-3) / 1e9
        rec["mean_reduced_chi2"] = float(np.nanmean(out["chi2"] / out["num_pixels"]))

        # ---- the launch inside the search call (gpdla_engine_process_spectra_models), against that call's sweeps
        lp = np.log(np.full((4, Q), 0.1))
        for D in (1, 4):
            sw, ml, tot = [], [], []
            for i in range(a.warmup + a.reps):
                eng.reset_stats()
                eng.process_model_spectra(packed, D, samples["log_nhi_samples"], level="best", log_priors_dla=lp[:D],
                                          memory="device")
                if i >= a.warmup:
                    lv = eng.multi_stats()["level_ms"]
                    sw.append(lv[0]); tot.append(float(np.sum(lv[:D]))); ml.append(eng.model_spectra_stats()["model_spectra_ms"])
            rec[f"search_max_dlas_{D}"] = dict(level1_sweep_ms=spread(sw), all_sweeps_ms=spread(tot), model_ms=spread(ml),
                                               model_over_level1_sweep=float(np.mean(ml) / np.mean(sw)),
                                               model_over_all_sweeps=float(np.mean(ml) / np.mean(tot)))

        # ---- the stand-alone entry at survey scale
        reps = max(1, a.survey_spectra // Q)
        big = syn.pack_spectra(spectra * reps)
        Qs = Q * reps
        z, ln = absorbers(Qs, 1, np.tile(sweep["min_z_dlas"], reps), np.tile(sweep["max_z_dlas"], reps))
        kernel, wall = [], []
        for _ in range(3):
            eng.reset_stats()
            t0 = time.perf_counter()
            res = eng.model_spectra(big, z, ln)
            wall.append((time.perf_counter() - t0) * 1e3)
            kernel.append(eng.model_spectra_stats()["model_spectra_ms"])
        nb = 2.0 * int(res["num_pixels"].sum()) * panel_row_bytes(a.k)
        rec["survey"] = dict(spectra=Qs, absorbers=1, kernel_ms=spread(kernel), call_wall_ms=spread(wall),
                             prep_ms=eng.stats()["prep_ms"], panel_bytes_read=nb, gb_per_s=nb / (min(kernel) * 1e-3) / 1e9)
    print(json.dumps(rec))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

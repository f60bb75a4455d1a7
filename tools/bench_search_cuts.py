"""Time the search cuts (gpdla_engine_process_cuts, gpdla_search_cuts_f64).

Part 1, BASELINE configs[1]'s shape: 1,024 synthetic spectra x 10^4 DLA samples, n = 800, k = 20, max_dlas = 1,
device-resident spectra, no sample array, the reference's grid (12 z bins x 27 log N_HI bins) for the summaries,
the population split and the level halves.  ``reps`` calls with and without ``cuts`` alternate; each is read back
through the engine's HIP-event accounting: the cut launch, and the summary, population and level launches with
and without the cuts, against the level-1 sweep of the same call.

Part 2, the kernel alone at survey scale: ``--survey-spectra`` spectra of ``--survey-pixels`` pixels (DR12Q is
162,861 x about 4,600), the Lya range a fifth of each, random noise with a quarter of the pixels noisy, both path
grids; kernel time by HIP events (gpdla_last_call_kernel_ms) against the bytes it must read (16 B per pixel).

    python tools/bench_search_cuts.py [--reps 10] [--survey-spectra 16384] [--out FILE]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import Engine, search_cuts  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402


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
    ap.add_argument("--survey-spectra", type=int, default=16384)
    ap.add_argument("--survey-pixels", type=int, default=4600)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Q, S = a.spectra, a.samples
    model = syn.make_model(k=a.k)
    samples = syn.make_samples(S)
    packed = syn.pack_spectra([syn.make_spectrum(model, q) for q in range(Q)])
    ez, en = np.linspace(2.0, 4.0, 13), np.linspace(20.3, 23.0, 28)
    lognhi = samples["log_nhi_samples"]
    pop = dict(z_edges=ez, log_nhi_edges=en, log_nhi_samples=lognhi, log_priors_no_dla=np.full(Q, np.log(0.9)),
               log_priors_dla=np.full((1, Q), np.log(0.1)))
    kw = dict(population=pop, log_nhi_samples=lognhi, z_edges=ez, log_nhi_edges=en, want_samples=False, memory="device",
              levels=None)
    thresh = float(np.quantile(packed["noise_variance"], 0.75))
    cuts = dict(proximity_zone=0.1, noise_thresh=thresh)
    rec = dict(what="gpdla_engine_process_cuts: the cut launch and the grid reductions with / without cuts vs the level-1 "
                    "sweep of the same call (HIP events, ms)", spectra=Q, samples=S, k=a.k, grid=[ez.size - 1, en.size - 1],
               pixels=int(packed["offsets"][-1]), reps=a.reps, warmup=a.warmup, cuts=cuts)
    keys = ("sweep_ms", "cut_ms", "summary_ms", "population_ms", "level_population_ms")
    cols = {on: {key: [] for key in keys} for on in (False, True)}
    with Engine(model, samples, set_parameters(k=a.k)) as eng:
        for i in range(a.warmup + a.reps):
            for on in (False, True):
                eng.reset_stats()
                out = eng.process_cuts(packed, 1, cuts=cuts if on else None, **kw)
                if i < a.warmup:
                    continue
                c = cols[on]
                c["sweep_ms"].append(eng.multi_stats()["level_ms"][0])
                c["cut_ms"].append(eng.cut_stats()["cut_ms"])
                c["summary_ms"].append(eng.summary_stats()["summary_ms"])
                c["population_ms"].append(eng.population_stats()["population_ms"])
                c["level_population_ms"].append(eng.level_population_stats()["level_population_ms"])
                if on:
                    rec["plane_mass_cut"] = float(out["bin_planes"][:, 0].sum())
                    rec["mean_pixel_count"] = float(out["cut_pixel_counts"].mean())
                    rec["path_total_cut"] = float(out["cut_path_summary"][:, -1].sum())
                else:
                    rec["plane_mass_uncut"] = float(out["bin_planes"][:, 0].sum())
    rec["without_cuts"] = {key: spread(v) for key, v in cols[False].items()}
    rec["with_cuts"] = {key: spread(v) for key, v in cols[True].items()}
    rec["cut_over_sweep"] = rec["with_cuts"]["cut_ms"]["mean"] / rec["with_cuts"]["sweep_ms"]["mean"]

    # ---- the kernel alone at survey scale
    Qs, n = a.survey_spectra, a.survey_pixels
    rng = np.random.default_rng(0)
    zmin = rng.uniform(2.0, 2.6, Qs)
    zmax = zmin + rng.uniform(0.5, 1.2, Qs)
    lo, hi = 1215.67 * (1.0 + zmin), 1215.67 * (1.0 + zmax)
    frac = np.linspace(-1.0, 4.0, n)              # a fifth of the pixels inside the Lya range
    wl = [lo[q] + (hi[q] - lo[q]) * frac for q in range(Qs)]
    nv = list(rng.random((Qs, n)))
    times = []
    for _ in range(3):
        res = search_cuts(wl, nv, zmin, zmax, 0.1, 0.75, ez, ez)
        times.append(L.last_call_kernel_ms()[0])
    bytes_read = 16.0 * Qs * n
    rec["survey"] = dict(spectra=Qs, pixels_per_spectrum=n, pixels=Qs * n, mean_pixel_count=float(res["cut_pixel_counts"].mean()),
                         kernel_ms=spread(times), bytes_read=bytes_read,
                         gb_per_s=bytes_read / (min(times) * 1e-3) / 1e9)
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

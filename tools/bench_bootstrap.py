"""Time the bootstrap sample errors (csrc/bootstrap.hip, catalog.sample_errors) at the DR12Q shape: Q = 162,861
sightlines, the reference's 18 x 30 summary grid (N = 4 nz nn + nz + 1 = 2,179 columns with the path terms),
B = 1,000 replicas, on synthetic summary planes.  Records

* the kernel time of every stage from gpdla_last_call_kernel_ms (HIP events): the rows launches (the call keeps
  its first 8 spans; their mean times the launch count is quoted as the stage's time and marked an estimate),
  then over ``reps`` calls of the one-call pipeline the draws, the product and the split-K reduction;
* the product's rate, 2 B Q N flop over its time, and that as a fraction of the 78.6 TF/s FP64 matrix peak;
* the wall time of the whole ``catalog.sample_errors`` call (host checks, copies and percentiles included);
* as the baseline the only route before this kernel: ``catalog.cddf_moments`` (both moments) and the path sums
  on gathered indices, timed for ``--baseline-replicas`` replicas and quoted per replica.

Prints one JSON line and, with --out, writes it.

    python tools/bench_bootstrap.py [--spectra 162861] [--nz 18] [--nn 30] [--replicas 1000] [--out FILE]
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402
from gp_dla_detection_amd import engine as E  # noqa: E402

FP64_PEAK_TFLOPS = 78.6


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(mean=float(v.mean()), min=float(v.min()), max=float(v.max()), max_minus_min=float(v.max() - v.min()))


def synthetic_out(Q, nz, nn, seed=7):
    """Summary variables of Q sightlines: one in ten carries a DLA's worth of mass, spread over a few bins."""
    rng = np.random.default_rng(seed)
    planes = np.zeros((Q, 5, nz, nn))
    hit = np.flatnonzero(rng.random(Q) < 0.1)
    for q in hit:
        iz, inn = rng.integers(0, nz, 4), rng.integers(0, nn, 4)
        mass = rng.dirichlet(np.ones(4))
        N = 10.0 ** rng.uniform(20.3, 22.0, 4)
        planes[q, :, iz, inn] = np.stack([mass, mass ** 2, N * mass, N ** 2 * mass, N ** 2 * mass ** 2], axis=1)
    p = np.where(np.isin(np.arange(Q), hit), rng.uniform(0.3, 1.0, Q), rng.uniform(0.0, 0.04, Q))
    zmax = np.where(rng.random(Q) < 0.97, rng.uniform(2.1, 3.6, Q), rng.uniform(3.6, 5.5, Q))   # a thin high-z tail
    zmin = np.maximum(1.96, zmax - rng.uniform(0.3, 1.2, Q))
    return dict(bin_planes=planes, p_dlas=p, min_z_dlas=zmin, max_z_dlas=zmax, bin_z_edges=np.linspace(2.0, 5.6, nz + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectra", type=int, default=162861)
    ap.add_argument("--nz", type=int, default=18)
    ap.add_argument("--nn", type=int, default=30)
    ap.add_argument("--replicas", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-replicas", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Q, nz, nn, B = a.spectra, a.nz, a.nn, a.replicas
    nb = nz * nn
    N = 4 * nb + nz + 1
    out = synthetic_out(Q, nz, nn)
    so, mem = CAT.bootstrap_strata(out["min_z_dlas"], out["max_z_dlas"])
    rec = dict(what="bootstrap sample errors: kernel ms per stage (HIP events), the product's FP64 rate, the wall time of "
                    "catalog.sample_errors, and the host route per replica",
               spectra=Q, grid=[nz, nn], columns=N, replicas=B, reps=a.reps, strata=[int(v) for v in np.diff(so)],
               tiling=L.bootstrap_tiling(), fp64_peak_tflops=FP64_PEAK_TFLOPS)

    t0 = time.perf_counter()
    rows = E.bootstrap_rows(out["bin_planes"], out["p_dlas"], None, 0.05, None, columns=N)
    rec["rows_call_wall_s"] = time.perf_counter() - t0
    ms = L.last_call_kernel_ms()
    launches = -(-Q // max(1, (64 << 20) // (5 * nb * 8)))
    rec["rows"] = dict(launches=launches, first_spans_ms=ms, kernel_ms_estimate=float(np.mean(ms)) * launches,
                       note="estimate: mean of the recorded spans times the launch count")
    rows[:, 4 * nb:] = CAT.path_columns(out["bin_z_edges"], out["min_z_dlas"], out["max_z_dlas"])

    stages = {k: [] for k in ("draws_ms", "product_ms", "reduction_ms")}
    walls = []
    for i in range(a.reps + 1):
        t0 = time.perf_counter()
        sums = E.bootstrap(rows, B, 2020, so, mem)
        wall = time.perf_counter() - t0
        ms = L.last_call_kernel_ms()
        chunks = len(ms) // 3
        if i:                                   # the first call warms up
            walls.append(wall)
            for j, k in enumerate(stages):
                stages[k].append(sum(ms[3 * c + j] for c in range(chunks)))
    rec.update({k: spread(v) for k, v in stages.items()})
    rec["pipeline_call_wall_s"] = spread(walls)
    flop = 2.0 * B * Q * N
    tf = flop / (rec["product_ms"]["mean"] * 1e-3) / 1e12
    rec["product"] = dict(flop=flop, tflops=tf, fraction_of_fp64_peak=tf / FP64_PEAK_TFLOPS)
    rec["checksum"] = float(sums[:, 4 * nb + nz].mean())
    del rows, sums

    t0 = time.perf_counter()
    se = CAT.sample_errors(out, replicas=B, seed=2020, strata=(so, mem))
    rec["sample_errors_wall_s"] = time.perf_counter() - t0
    rec["bins_with_path"] = int(se["z"].size)
    rec["dndx_median"] = [float(v) for v in se["dndx_median"]]

    # the route before: gather, then cddf_moments and the path sums on the gathered sightlines
    rng = np.random.default_rng(5)
    path = CAT.path_columns(out["bin_z_edges"], out["min_z_dlas"], out["max_z_dlas"])
    per = []
    for _ in range(a.baseline_replicas):
        t0 = time.perf_counter()
        idx = mem[rng.integers(0, mem.size, mem.size)]
        planes, p = out["bin_planes"][idx], out["p_dlas"][idx]
        for moment in (False, True):
            CAT.cddf_moments(planes, p, moment=moment)
        for c in range(nz + 1):
            math.fsum(path[idx, c].tolist())
        per.append(time.perf_counter() - t0)
    rec["host_route"] = dict(replicas_timed=a.baseline_replicas, seconds_per_replica=spread(per),
                             note="catalog.cddf_moments on gathered indices; per replica, not extrapolated")
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

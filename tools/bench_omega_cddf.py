"""Time Omega_DLA from the column density function (csrc/count_mixture.hip, catalog.omega_dla_cddf) at a
DR12Q-like load: the reference's 18 x 30 (z, log N_HI) grid, per-cell exact lists and Poisson means drawn so that
a cell at the low-N end counts 10^2 - 10^3 absorbers and the counts fall as N^-1.6 from there.  Records

* the stages: per redshift bin their number, the taps, and the cells that can be non-zero at the end;
* the kernel times of gpdla_count_mixture_f64 from gpdla_last_call_kernel_ms (HIP events) over ``reps`` calls
  after a warm-up: all stage launches, the scan, the search; the tap-cell products per second of the stage
  launches (one FMA and one 8-byte read each); and the wall time of the call (allocation, memset, copies);
* the kernel times of the Poisson-binomial pmf call that feeds it, and the wall time of the whole
  ``catalog.total_column_intervals``;
* the same arithmetic in numpy (tests/count_mixture_oracle.numpy_chain, one vector multiply-add per tap over the
  live cells, then cumsum and searchsorted-style level lookups), one process per redshift bin on ``--workers``
  processes, run before the device is touched: the wall time of the pool and every bin's own time;
* the tile and tap constants of the library that was timed, and that both runs return the same cells.

Prints one JSON line and, with --out, writes it.

    python tools/bench_omega_cddf.py [--nz 18] [--nn 30] [--cells 1048576] [--reps 5] [--workers 16] [--host-only] [--out FILE]
"""
import argparse
import json
import sys
import time
from multiprocessing import get_context
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import count_mixture_oracle as CO  # noqa: E402
import population_oracle as PO  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(mean=float(v.mean()), min=float(v.min()), max=float(v.max()), max_minus_min=float(v.max() - v.min()))


def synthetic_grid(nz, nn, seed=11):
    """Per cell an expected count A_z 10^(-1.6 (log N - 20.3)) with A_z in 10^2 .. 10^3 (fewer towards high z), a
    fifth of it (at most 400 trials) as exact trials with p in [0.25, 1), the rest as the Poisson mean."""
    rng = np.random.default_rng(seed)
    en = np.linspace(20.3, 23.0, nn + 1)
    cent = (en[1:] + en[:-1]) / 2
    amp = 10.0 ** np.linspace(3.0, 2.0, nz)
    lists, means = [], np.zeros((nz, nn))
    for iz in range(nz):
        row = []
        for b in range(nn):
            count = amp[iz] * 10.0 ** (-1.6 * (cent[b] - cent[0])) * rng.uniform(0.8, 1.25)
            trials = int(min(400, rng.poisson(count / 5 / 0.625)))
            row.append(rng.uniform(0.25, 1.0, trials))
            means[iz, b] = max(count - row[-1].sum(), 0.0)
        lists.append(row)
    return lists, means, en


def numpy_problem(job):
    stages, cells, levels = job
    t0 = time.perf_counter()
    got = CO.levels_of(CO.numpy_chain(stages, cells), levels)
    return got[0], got[1], got[2], time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nz", type=int, default=18)
    ap.add_argument("--nn", type=int, default=30)
    ap.add_argument("--cells", type=int, default=2 ** 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--host-only", action="store_true", help="the load and the numpy restatement, no device")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lists, means, en = synthetic_grid(a.nz, a.nn)
    captured = []

    def capture(*args):
        captured.append(args)
        P = len(args[3]) - 1
        return np.zeros((P, len(args[5])), dtype=np.int32), np.zeros((P, len(args[5])), dtype=np.int32), np.ones(P)
    CAT.total_column_intervals(lists, means, en, cells=a.cells, pmf=lambda ls: [PO.recurrence_pmf(v) for v in ls], mixture=capture)
    probs, shifts, tap_off, stage_off, cells, levels = captured[0]
    problems = CO.split_csr(probs, shifts, tap_off, stage_off)
    live = [1 + sum(int(s[-1]) for _, s in pr) for pr in problems]
    products = 0
    for pr in problems:
        reach = 1
        for p, s in pr:
            reach += int(s[-1])
            products += int(np.clip(reach - s, 0, None).sum())      # tap i touches the cells shift_i .. reach - 1
    rec = dict(what="omega_dla_cddf at a DR12Q-like load: kernel ms of gpdla_count_mixture_f64 (HIP events), its wall time, "
                    "the pmf call before it, catalog.total_column_intervals end to end, and the numpy restatement",
               grid=[a.nz, a.nn], cells=cells, reps=a.reps,
               expected_count_low_n=[float(means[iz, 0] + lists[iz][0].sum()) for iz in range(a.nz)],
               exact_trials=int(sum(v.size for row in lists for v in row)),
               stages_per_problem=[len(pr) for pr in problems], taps_per_problem=[int(sum(len(p) for p, _ in pr)) for pr in problems],
               largest_stage_taps=int(np.diff(tap_off).max()), live_cells_per_problem=live, tap_cell_products=products)

    # numpy first: the pool forks before this process opens the device
    jobs = [(pr, cells, levels) for pr in problems]
    t0 = time.perf_counter()
    with get_context("fork").Pool(min(a.workers, len(jobs))) as pool:
        host = pool.map(numpy_problem, jobs, chunksize=1)
    rec["numpy"] = dict(workers=min(a.workers, len(jobs)), wall_s=time.perf_counter() - t0,
                        seconds_per_problem=[float(h[3]) for h in host], sum_of_problems_s=float(sum(h[3] for h in host)),
                        note="count_mixture_oracle.numpy_chain + levels_of, one process per redshift bin")

    if a.host_only:
        print(json.dumps(rec))
        return
    from gp_dla_detection_amd import _lib as L
    from gp_dla_detection_amd import engine as E
    rec["tiling"] = E.count_mixture_tiling()
    spans, walls = [], []
    for i in range(a.reps + 1):
        t0 = time.perf_counter()
        lower, upper, mass = E.count_mixture(probs, shifts, tap_off, stage_off, cells, levels)
        wall = time.perf_counter() - t0
        if i:                                   # the first call warms up
            walls.append(wall)
            spans.append(L.last_call_kernel_ms())
    spans = np.array(spans)
    rec.update(stages_ms=spread(spans[:, 0]), scan_ms=spread(spans[:, 1]), search_ms=spread(spans[:, 2]),
               kernels_ms=spread(spans.sum(axis=1)), count_mixture_call_wall_s=spread(walls))
    rec["stage_rate"] = dict(products_per_s=products / (rec["stages_ms"]["mean"] * 1e-3),
                             read_gb_per_s=8.0 * products / (rec["stages_ms"]["mean"] * 1e-3) / 1e9,
                             note="one fp64 FMA and one 8-byte read (L2 / LDS-staged tap aside) per product")
    rec["same_cells_as_numpy"] = bool(all(np.array_equal(lower[p], host[p][0]) and np.array_equal(upper[p], host[p][1])
                                          for p in range(len(problems))))
    rec["mass"] = spread(mass)
    flat = [v for row in lists for v in row]
    CAT.poisson_binomial_pmf(flat)
    t0 = time.perf_counter()
    CAT.poisson_binomial_pmf(flat)
    rec["pmf_call"] = dict(wall_s=time.perf_counter() - t0, kernel_ms=L.last_call_kernel_ms())
    t0 = time.perf_counter()
    mid, l68, l95, steps = CAT.total_column_intervals(lists, means, en, cells=a.cells)
    rec["total_column_intervals_wall_s"] = time.perf_counter() - t0
    rec["median_total_column"] = [float(v) for v in mid]
    rec["lattice_step_over_median"] = float((steps / mid).max())
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

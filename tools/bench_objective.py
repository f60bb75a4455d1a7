"""Time the GPU training objective (objective.m) on a DR9-training-set-sized synthetic problem:
Q spectra x 1217 rest pixels, k = 20, ~30% missing pixels.  Prints one JSON line.

    python tools/bench_objective.py [Q P k reps] [--forest [--lines L] [--rounds R]]

--forest: the Lyman-series forest in the objective.  The pixels then sit on the rest
grid of quasars at z_QSO in 2.2..4.5 (so the number of absorbing lines runs from 31 at the blue end to 0
redward of Lya, as in a training set), and the Lya-only objective is timed on the same data in the same
process, the two alternating for R rounds of `reps` evaluations; medians and the rounds are reported."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gp_dla_detection_amd import training as T  # noqa: E402


def _time(obj, x, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        f, g = obj(x)
    return (time.perf_counter() - t0) / reps, f


def main(Q=5000, P=1217, k=20, reps=5, forest=False, lines=31, rounds=5):
    rng = np.random.default_rng(3)
    y = 0.3 * rng.standard_normal((Q, P))
    y[rng.uniform(size=y.shape) < 0.3] = np.nan
    lya = rng.uniform(2.5, 4.5, (Q, P))
    nv = rng.uniform(0.01, 0.1, (Q, P))
    x = np.concatenate([0.05 * rng.standard_normal(P * k), np.log(0.15) + 0.1 * rng.standard_normal(P),
                        [np.log(0.1), np.log(0.0023), np.log(3.65)]])
    flops = Q * np.mean((~np.isnan(y[:64])).sum(axis=1)) * (k * (k + 1) + 4 * k * k + 8 * k)
    if not forest:
        with T.Objective(y, lya, nv, k) as obj:
            obj(x)
            dt, f = _time(obj, x, reps)
        print(json.dumps(dict(what="objective.m f+g on the GPU", spectra=Q, pixels=P, k=k, ms_per_eval=dt * 1e3,
                              spectra_per_s=Q / dt, approx_gflops=flops / dt / 1e9, f=f)))
        return
    z = rng.uniform(2.2, 4.5, Q)
    rest = np.linspace(911.75, 1215.75, P)
    lya = rest[None, :] * (1 + z[:, None]) / 1215.6701
    with T.Objective(y, lya, nv, k) as obj:
        obj(x)
        obj.set_forest(z, lines)
        obj(x)
        off, on = [], []
        for _ in range(rounds):
            obj.set_forest(None)
            dt, f_off = _time(obj, x, reps)
            off.append(dt * 1e3)
            obj.set_forest(z, lines)
            dt, f = _time(obj, x, reps)
            on.append(dt * 1e3)
    dt = float(np.median(on)) * 1e-3
    print(json.dumps(dict(what="objective.m f+g on the GPU, Lyman-series forest in the objective", spectra=Q, pixels=P,
                          k=k, num_forest_lines=lines, ms_per_eval=dt * 1e3, ms_per_eval_lya_only=float(np.median(off)),
                          rounds_ms=[round(v, 4) for v in on], rounds_ms_lya_only=[round(v, 4) for v in off],
                          spectra_per_s=Q / dt, approx_gflops=flops / dt / 1e9, f=f, f_lya_only=f_off)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shape", nargs="*", type=int, help="Q P k reps (defaults 5000 1217 20 5)")
    ap.add_argument("--forest", action="store_true")
    ap.add_argument("--lines", type=int, default=31)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    main(*a.shape, forest=a.forest, lines=a.lines, rounds=a.rounds)

"""Posterior intervals, the parts that need no GPU: the fsum oracle (posterior_intervals_oracle.py) against a
brute-force dense version and against the reference's own ``find_delta_NHI`` / ``find_delta_z`` numbers
(tests/golden/posterior_intervals.npz, made by tests/golden/make_posterior_intervals_fixture.py),
``process_qsos(intervals=...)`` with an injected compute, the catalogue functions, the keyword validation and
the dynamic-LDS carve of the kernel."""
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import posterior_intervals_oracle as IO  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402
from gp_dla_detection_amd import matv73 as M  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402
from test_posterior_summary import summary_compute  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).parent / "golden" / "posterior_intervals.npz"


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ------------------------------------------------------------------------------------------- oracle
def dense_intervals(l, c, ok, min_z, max_z, offsets, log_nhi, levels, lr_delta):
    """One (row, level) by brute force, sample by sample: per slot and parameter (lo, hi, mean, sd, quantiles)."""
    S = l.size
    pi, m, usable = IO.row_masses(l)     # the masses are the definition both share; everything after them is redone
    if not usable:
        return None
    valid = [j for j in range(S) if ok[j]]
    inside = [j for j in valid if l[j] > m - lr_delta]
    T = math.fsum(pi[j] for j in valid)
    out = {"count": len(inside)}
    for u in range(c.shape[0]):
        for p in range(2):
            x = [float(np.float64(min_z) + (np.float64(max_z) - np.float64(min_z)) * np.float64(offsets[c[u, j]])) if p == 0
                 else float(log_nhi[c[u, j]]) for j in range(S)]
            lo = min((x[j] for j in inside), default=math.nan)
            hi = max((x[j] for j in inside), default=math.nan)
            if not T > 0.0:
                out[(u, p)] = (lo, hi, math.nan, math.nan, [math.nan] * len(levels))
                continue
            mean = math.fsum(np.float64(pi[j]) * np.float64(x[j]) for j in valid) / T
            var = math.fsum(np.float64(pi[j]) * ((np.float64(x[j]) - mean) * (np.float64(x[j]) - mean)) for j in valid) / T
            qs = []
            for lv in levels:
                best = math.nan
                for v in sorted(set(x[j] for j in valid)):
                    if math.fsum(pi[j] for j in valid if x[j] <= v) >= lv * T:
                        best = v
                        break
                qs.append(best)
            out[(u, p)] = (lo, hi, mean, math.sqrt(var), qs)
    return out


def test_oracle_against_brute_force():
    rng = np.random.default_rng(3)
    S, R, D = 23, 5, 3
    ll = rng.normal(0.0, 2.0, (D, R, S))
    ll[rng.random(ll.shape) < 0.15] = np.nan
    ll[1, 2] = np.nan                                   # unusable
    ll[0, 3] = -np.inf                                  # unusable: exp(-inf + inf)
    ll[2, 4] = 0.0                                      # flat: the 0.5 quantile sits on a step of the cdf
    base = rng.integers(-1, S + 1, (D - 1, R, S))       # -1 and S are void
    base[:, 4] = rng.integers(0, 3, (D - 1, S))         # repeated bases: ties in every deeper slot
    offsets = np.round(rng.random(S), 1)                # ties
    log_nhi = np.round(rng.uniform(20.0, 23.0, S), 1)
    min_z, max_z = rng.uniform(2.0, 2.5, R), rng.uniform(2.6, 4.0, R)
    levels = (0.025, 0.5, 0.975)
    got = IO.intervals(ll, base, min_z, max_z, offsets, log_nhi, levels, 1.25)
    seen = 0
    for d in range(D):
        for r in range(R):
            c, ok = IO.chains(base, d, r, S)
            want = dense_intervals(ll[d, r], c, ok, min_z[r], max_z[r], offsets, log_nhi, levels, 1.25)
            if want is None:
                assert got["lr_counts"][d, r] == 0
                for key in got:
                    if key != "lr_counts":
                        assert np.isnan(got[key][d, r]).all(), (key, d, r)
                continue
            assert got["lr_counts"][d, r] == want["count"]
            for u in range(d + 1):
                for p, name in enumerate(("z_dla", "log_nhi")):
                    lo, hi, mean, sd, qs = want[(u, p)]
                    assert _same(got[name + "_lr_ranges"][d, r, u], [lo, hi]), (name, d, r, u)
                    assert _same(got[name + "_means"][d, r, u], mean) and _same(got[name + "_sds"][d, r, u], sd)
                    assert _same(got[name + "_quantiles"][d, r, u], qs), (name, d, r, u)
                    seen += not math.isnan(mean)
            assert np.isnan(got["z_dla_means"][d, r, d + 1:]).all()
    assert seen > 40
    x, pi = np.array([1.0, 2.0, 2.0, 3.0]), np.array([0.25, 0.25, 0.25, 0.25])
    assert [IO.quantile(x, pi, lv)[0] for lv in (0.25, 0.26, 0.75, 0.76)] == [1.0, 2.0, 2.0, 3.0]   # the step itself counts
    assert IO.quantile_dense(x, pi, 0.75) == 2.0 and math.isnan(IO.quantile(x, 0.0 * pi, 0.5)[0])


def test_oracle_matches_the_reference():
    """hi - lo of level 1, slot 0 equals the reference's find_delta_NHI / find_delta_z bit for bit: both form z with
    a separately rounded product and sum.  The fixture holds a row with one sample inside the range (width 0) and
    rows with many; its generator asserted that no sample lies within 1e-9 of the threshold."""
    g = np.load(GOLDEN)
    ll = g["sample_log_likelihoods"]
    got = IO.intervals(ll[None], None, g["min_z_dlas"], g["max_z_dlas"], g["offset_samples"], g["log_nhi_samples"],
                       quantiles=False)
    nr, zr = got["log_nhi_lr_ranges"][0, :, 0], got["z_dla_lr_ranges"][0, :, 0]
    assert np.array_equal(nr[:, 1] - nr[:, 0], g["ref_delta_nhi"]) and np.array_equal(zr[:, 1] - zr[:, 0], g["ref_delta_z"])
    assert np.array_equal(got["lr_counts"][0], g["lr_counts"])
    assert (g["lr_counts"] == 1).any() and (g["lr_counts"] >= 3).any()
    assert (g["ref_delta_nhi"][g["lr_counts"] == 1] == 0.0).all() and (g["ref_delta_nhi"][g["lr_counts"] >= 3] > 0.0).all()
    assert np.abs(ll - (ll.max(axis=1) - 2.0)[:, None]).min() > 1e-9


# ------------------------------------------------------------------------- process_qsos(intervals=...)
K, S, Q = 4, 24, 3
Z_EDGES, N_EDGES = np.linspace(1.5, 4.5, 4), np.linspace(20.0, 23.0, 3)


def interval_compute(calls):
    """A ``compute`` replacement: test_posterior_summary.py's for everything process_qsos had, the interval oracle
    on its sample arrays for the rest."""
    def compute(model, samples, packed, params, device=0, max_dlas=1, summaries=None, save_samples=True, intervals=None):
        calls.append(dict(max_dlas=max_dlas, summaries=summaries, save_samples=save_samples, intervals=intervals))
        res = summary_compute([])(model, samples, packed, params, device, max_dlas=max_dlas, summaries=summaries)
        if intervals is not None:
            sll = res["sample_log_likelihoods_dla"][None] if max_dlas == 1 else res["sample_log_likelihoods_dla"]
            res.update(IO.intervals(sll, res.get("base_sample_inds"), res["min_z_dlas"], res["max_z_dlas"],
                                    samples["offset_samples"], samples["log_nhi_samples"], intervals["levels"],
                                    intervals["lr_delta"]))
        if not save_samples:
            res.pop("sample_log_likelihoods_dla", None)
            res.pop("base_sample_inds", None)
        return res
    return compute


@pytest.fixture(scope="module")
def setup():
    model = syn.make_model(k=K)
    samples = syn.make_samples(S)
    spectra = [syn.make_spectrum(model, q, n_target=120, mask_fraction=0.05, dla_fraction=1.0) for q in range(Q)]
    rng = np.random.default_rng(5)
    prior = dict(z_qsos=rng.uniform(2.0, 4.5, 400), dla_ind=rng.uniform(size=400) < 0.12)
    return dict(model=model, samples=samples, packed=syn.pack_spectra(spectra), params=set_parameters(k=K), prior=prior)


def run(s, calls=None, **kw):
    calls = [] if calls is None else calls
    return PR.process_qsos(s["model"], s["samples"], s["packed"], s["prior"], params=s["params"],
                           compute=interval_compute(calls), **kw)


@pytest.mark.parametrize("D", [1, 3])
def test_process_qsos_intervals(setup, tmp_path, D):
    s = setup
    grid = dict(z_edges=Z_EDGES, log_nhi_edges=N_EDGES)
    calls = []
    plain = run(s, calls, max_dlas=D, summaries=grid)
    assert calls[0]["intervals"] is None                      # without the keyword the compute call is as before
    out = run(s, calls, max_dlas=D, summaries=grid, intervals=True)
    assert np.array_equal(calls[1]["intervals"]["levels"], (0.025, 0.16, 0.5, 0.84, 0.975)) and calls[1]["intervals"]["lr_delta"] == 2.0
    for key in plain:                                         # nothing that was there moves
        assert _same(out[key], plain[key]), key
    assert set(out) - set(plain) == set(PR.INTERVAL_VARIABLES)
    assert out["z_dla_quantiles"].shape == out["log_nhi_quantiles"].shape == (Q, D, 4, 5)
    assert out["z_dla_means"].shape == out["log_nhi_sds"].shape == (Q, D, 4)
    assert out["z_dla_lr_ranges"].shape == (Q, D, 4, 2) and out["lr_counts"].shape == (Q, D)
    assert out["lr_counts"].dtype == np.float64 and out["lr_delta"] == 2.0
    for d in range(D):                                        # level d + 1 has d + 1 absorbers, the rest is NaN
        assert np.isfinite(out["log_nhi_means"][:, d, :d + 1]).all() and np.isnan(out["log_nhi_means"][:, d, d + 1:]).all()
    q50 = out["log_nhi_quantiles"][:, 0, 0]
    assert np.all(np.diff(q50, axis=1) >= 0) and np.all(np.isin(q50, s["samples"]["log_nhi_samples"]))
    # implied summaries (the MAP pairs), other levels, no sample arrays
    only = run(s, max_dlas=D, intervals=dict(levels=[0.5], lr_delta=0.5))
    assert {"MAP_z_dlas", "MAP_log_nhis", "map_sample_inds"} <= set(only) and "bin_planes" not in only
    assert only["z_dla_quantiles"].shape == (Q, D, 4, 1) and np.all(only["lr_counts"] <= out["lr_counts"])
    assert _same(only["z_dla_quantiles"][..., 0], out["z_dla_quantiles"][..., 2])
    lean = run(s, max_dlas=D, summaries=grid, intervals=True, save_samples=False)
    assert "sample_log_likelihoods_dla" not in lean
    for key in lean:
        assert _same(lean[key], out[key]), key
    # the file, and the catalogue functions on what was read back
    lean["test_ind"] = np.array([True, False, True, True])
    path = tmp_path / "processed_qsos_intervals.mat"
    PR.save_processed_qsos(str(path), lean)
    r = M.loadmat(str(path))
    for key in PR.INTERVAL_VARIABLES:
        assert _same(np.asarray(r[key]).reshape(np.shape(lean[key])), lean[key]), key
    assert r["z_dla_quantiles"].shape == (Q, D, 4, 5)
    plain["test_ind"] = lean["test_ind"]
    PR.save_processed_qsos(str(tmp_path / "plain.mat"), plain)
    assert not set(M.loadmat(str(tmp_path / "plain.mat"))) & set(PR.INTERVAL_VARIABLES)
    lr = out["log_nhi_lr_ranges"][:, 0, 0]
    assert _same(CAT.find_delta_nhi(r), lr[:, 1] - lr[:, 0])
    zr = out["z_dla_lr_ranges"][:, 0, 0]
    assert _same(CAT.find_delta_z(r), zr[:, 1] - zr[:, 0]) and np.all(CAT.find_delta_z(out) >= 0)
    sll = out["sample_log_likelihoods_dla"].reshape(Q, S, D)[:, :, 0]
    for q in range(Q):                                        # the reference's two lines, spelled out
        keep = sll[q] > np.nanmax(sll[q]) - 2
        nv = s["samples"]["log_nhi_samples"][keep]
        assert CAT.find_delta_nhi(out)[q] == nv.max() - nv.min()
    table = CAT.absorber_table(r)
    level = np.argmax(out["model_posteriors"][:, 1:1 + D], axis=1)
    assert table["spectrum"].tolist() == [q for q in range(Q) for _ in range(level[q] + 1)]
    assert table["absorber"].tolist() == [u for q in range(Q) for u in range(level[q] + 1)]
    assert np.array_equal(table["level"], level[table["spectrum"]] + 1)
    n = table["spectrum"].size
    for key in CAT.ABSORBER_FIELDS:
        assert table[key].shape == (n,), key
    assert table["z_dla_quantiles"].shape == (n, 5) and np.array_equal(table["interval_levels"], out["interval_levels"])
    for i in range(n):
        q, d, u = table["spectrum"][i], table["level"][i] - 1, table["absorber"][i]
        assert table["map_z_dla"][i] == out["MAP_z_dlas"][q, u] and table["map_log_nhi"][i] == out["MAP_log_nhis"][q, u]
        assert _same(table["log_nhi_quantiles"][i], out["log_nhi_quantiles"][q, d, u])
        assert table["z_dla_sd"][i] == out["z_dla_sds"][q, d, u] and table["log_nhi_lr_hi"][i] == out["log_nhi_lr_ranges"][q, d, u, 1]
    catalog = dict(thing_ids=np.array([11, 22, 33, 44]))
    dat = CAT.write_absorber_catalog(str(tmp_path / "cat"), "dr12q", catalog, r)
    lines = Path(dat).read_text().splitlines()
    assert Path(dat).name == "dr12q_absorbers.dat" and len(lines) == n + 1
    assert lines[0].split()[:6] == ["#", "thing_id", "level", "absorber", "map_z_dla", "map_log_nhi"]
    assert len(lines[0].split()) - 1 == len(lines[1].split()) == 5 + 2 * (5 + 4)
    ids = [11, 33, 44]                                        # test_ind resolves the searched spectra
    for i, line in enumerate(lines[1:]):
        f = line.split()
        assert f[0] == "%09d" % ids[table["spectrum"][i]] and int(f[1]) == table["level"][i] and int(f[2]) == table["absorber"][i] + 1
        assert f[3] == "%06.4f" % table["map_z_dla"][i] and f[7] == "%06.4f" % table["z_dla_quantiles"][i, 2]
        assert f[10] == "%06.4f" % table["z_dla_mean"][i] and f[11] == "%.4e" % table["z_dla_sd"][i]
        assert f[-1] == "%07.4f" % table["log_nhi_lr_hi"][i]


def test_catalog_functions_need_the_interval_variables(setup):
    plain = run(setup, summaries=True)
    for fn in (CAT.find_delta_nhi, CAT.find_delta_z, CAT.absorber_table):
        with pytest.raises(ValueError, match="intervals"):
            fn(plain)
    with pytest.raises(ValueError):
        CAT.find_delta_z(dict(z_dla_lr_ranges=np.zeros((3, 1, 2, 2))))


def test_interval_arguments(setup):
    s = setup
    bad = [dict(levels=[0.5, 0.5]), dict(levels=[0.6, 0.4]), dict(levels=[0.0, 0.5]), dict(levels=[0.5, 1.0]),
           dict(levels=[np.nan]), dict(levels=[]), dict(levels=np.linspace(0.1, 0.9, 9)), dict(lr_delta=0.0),
           dict(lr_delta=-2.0), dict(lr_delta=np.inf), dict(lr_delta=np.nan), dict(quantiles=[0.5]), [0.5], "yes"]
    for ivs in bad:
        with pytest.raises(ValueError):
            run(s, intervals=ivs)
    assert "z_dla_quantiles" not in run(s, intervals=False) and "z_dla_quantiles" not in run(s, intervals=None)
    assert run(s, intervals=dict(levels=np.linspace(0.1, 0.9, 8)))["z_dla_quantiles"].shape == (Q, 1, 4, 8)
    pop = dict(z_edges=Z_EDGES, log_nhi_edges=N_EDGES)
    with pytest.raises(ValueError, match="population"):
        run(s, intervals=True, population=pop)
    with pytest.raises(ValueError, match="sub_dla"):
        run(s, intervals=True, sub_dla=True)
    with pytest.raises(ValueError, match="levels='all'"):
        run(s, intervals=True, max_dlas=2, summaries=dict(z_edges=Z_EDGES, log_nhi_edges=N_EDGES, levels="all"))


# ------------------------------------------------------------------------------------------ LDS carve
PROGRAM = r"""
#include <cstdio>
#include "row_posterior.h"
using namespace gpdla;
int main() {
  const long sizes[] = {1, 2, 1024, 1025, 2048, 2049, 10000, 1 << 18, (1 << 18) + 1, 1 << 19, (1 << 19) + 1, 1 << 20};
  for (long S : sizes)
    for (int nq = 1; nq <= 8; ++nq)
      std::printf("%ld %d %d %d %d %zu\n", S, nq, interval_shift(S), interval_group(interval_shift(S), nq),
                  interval_cells(S, nq), interval_lds(S, nq).total);
  return 0;
}
"""


def up16(x):
    return (x + 15) & ~15


def interval_lds(S, nq):
    """The carve laid out by hand: 4 waves, 2 parameters x 4 slots x 12 results, 8 quantile levels, a tile of 512."""
    s = 0
    while (S - 1) >> s >= 1024:
        s += 1
    group = min(nq, max(2048 >> s, 1))
    cells = max(((S - 1) >> s) + 1, (group << s) if s else 0)
    o = 0
    for size in [4 * 8, 4 * 4, 2 * 4 * 12 * 8, 2 * 8 * 8, 2 * 8 * 8, 8 * 8, 2 * 8 * 4, 2 * 8 * 4, 2 * 8 * 4, 4,
                 2 * cells * 8, 512 * 8, 512 * 4, 512 * 4]:
        o = up16(o + size)
    return s, group, cells, o


def test_interval_carve_totals(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = tmp_path / "interval_lds.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "interval_lds"
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O0", f"-I{ROOT / 'gp_dla_detection_amd' / 'csrc'}",
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        S_, nq, s, group, cells, total = map(int, line.split())
        got[(S_, nq)] = (s, group, cells, total)
    assert len(got) == 12 * 8
    for (S_, nq), v in got.items():
        assert v == interval_lds(S_, nq), (S_, nq)
        assert v[3] <= 64 * 1024
        assert v[0] == 0 or v[1] << v[0] <= 2048
    # the shift steps where the issue's sizes say, and the figures the sources quote
    assert [got[(n, 5)][0] for n in (1024, 1025, 2048, 2049, 10000, 1 << 20)] == [0, 1, 1, 2, 4, 10]
    assert got[(1 << 20, 8)][:3] == (10, 2, 2048) and got[(1 << 18, 8)][:3] == (8, 8, 2048)
    assert got[(10000, 5)][3] == 19536 and got[(1024, 5)][3] == 25920
    assert max(v[3] for v in got.values()) == got[(1 << 20, 8)][3] == 42304

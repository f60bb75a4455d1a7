"""Bootstrap sample errors and per-spectrum SNRs on the GPU (csrc/bootstrap.hip, csrc/snr.hip) against the host
oracles of bootstrap_oracle.py: the draws integer for integer, the f64 matrix-core product against the exact
sums at every tile, stage, slice and chunk edge (read from the library, gpdla_bootstrap_tiling), the rows and
the SNRs bit for bit, the one-call pipeline against its two halves, ``catalog.sample_errors`` on a synthetic
``process_qsos(summaries=...)`` run against the injected host route, and every GPDLA_EINVAL."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import bootstrap_oracle as BO  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402
from gp_dla_detection_amd import engine as E  # noqa: E402
from gp_dla_detection_amd import process as PR  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402
from test_bootstrap import synthetic_out  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def _tiling():
    return L.bootstrap_tiling()


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _raises_einval(fn, *a, **kw):
    with pytest.raises(L.GpdlaError) as ei:
        fn(*a, **kw)
    assert ei.value.code == L.GPDLA_EINVAL, ei.value


# ------------------------------------------------------------------------------------------ 1. counts
# strata of 1..5 members (the four-words-per-counter edge), starting at positions 1, 3, 6, 10 (no multiple of
# 4 but 0), over 20 spectra of which 5 are in no stratum
SMALL_SO = np.array([0, 1, 3, 6, 10, 15])
SMALL_MEM = np.array([19, 4, 11, 0, 7, 8, 2, 5, 13, 17, 1, 3, 9, 12, 18])


@pytest.mark.parametrize("case", ["one", "small", "many"])
def test_counts_equal_the_oracle(case):
    if case == "one":
        Q, so, mem, B = 37, None, None, 5
    elif case == "small":
        Q, so, mem, B = 20, SMALL_SO, SMALL_MEM, 9
    else:
        rng = np.random.default_rng(4)
        Q = 1500
        mem = np.sort(rng.permutation(Q)[:1301])
        so, B = np.array([0, 257, 258, 1027, 1301]), 3
    seed = (0x9e3779b97f4a7c15, 0x0123456789abcdef)
    got = E.bootstrap_counts(Q, B, seed, so, mem)
    assert got.dtype == np.int32 and _same(got, BO.counts(Q, B, seed, so, mem))
    members = np.arange(Q) if mem is None else mem
    offs = [0, Q] if so is None else so
    assert np.all(got.sum(axis=1) == len(members))
    for s in range(len(offs) - 1):
        assert np.all(got[:, members[offs[s]:offs[s + 1]]].sum(axis=1) == offs[s + 1] - offs[s])
    assert np.all(got[:, np.setdiff1d(np.arange(Q), members)] == 0)
    # a split by first_replica is the one call; an integer seed is its two words
    parts = [E.bootstrap_counts(Q, 2, seed, so, mem), E.bootstrap_counts(Q, B - 2, seed, so, mem, first_replica=2)]
    assert _same(np.vstack(parts), got)
    assert _same(E.bootstrap_counts(Q, 1, seed[0] + (seed[1] << 64), so, mem), got[:1])


def test_counts_over_more_than_one_device_chunk():
    B = _tiling()["max_chunk"] + 1
    got = E.bootstrap_counts(20, B, 77, SMALL_SO, SMALL_MEM, first_replica=5)
    assert _same(got, BO.counts(20, B, 77, SMALL_SO, SMALL_MEM, first_replica=5))


# -------------------------------------------------------------------------------------------- 2. sums
def _operands(rng, M, N, K):
    """Counts 0..3, most of them 0 or 1, and signed rows over twelve decades."""
    cnt = rng.choice(np.arange(4, dtype=np.int32), size=(M, K), p=[0.45, 0.4, 0.1, 0.05])
    rows = rng.standard_normal((K, N)) * 10.0 ** rng.uniform(-6, 6, (K, N))
    return cnt, rows


def _edge_sizes():
    t = _tiling()
    around = lambda v: [v - 1, v, v + 1]
    ms = [1] + around(t["tile_m"]) + around(t["max_chunk"])
    ns = [1] + around(t["tile_n"])
    ks = [1] + around(t["stage_k"]) + around(t["k_slice"])
    base = (3, 5, 7)
    return ([(m, base[1], base[2]) for m in ms] + [(base[0], n, base[2]) for n in ns] + [(base[0], base[1], k) for k in ks] +
            [(t["tile_m"] + 1, t["tile_n"] + 1, 2 * t["stage_k"] + 1)])


def test_sums_at_every_edge_within_the_summation_bound():
    """|got - exact| <= (K + 2) 2^-53 sum_q |count row| per entry: K - 1 additions and one rounding per fused
    term in any order, and the exact sum's own rounding."""
    rng = np.random.default_rng(21)
    sizes = _edge_sizes()
    assert len(set(sizes)) == len(sizes) >= 15
    for M, N, K in sizes:
        cnt, rows = _operands(rng, M, N, K)
        got = E.bootstrap_sums(cnt, rows)
        exact, mag = BO.exact_sums(cnt, rows)
        worst = np.max(np.abs(got - exact) / np.where(mag > 0, mag, 1.0))
        print(f"M={M} N={N} K={K}: worst error {worst / U:.2f} x 2^-53 of the magnitude sum (bound {K + 2})")
        assert got.shape == (M, N) and np.all(np.abs(got - exact) <= (K + 2) * U * mag), (M, N, K)


def test_sums_identity_zero_rows_and_repeats():
    t = _tiling()
    rng = np.random.default_rng(22)
    K, N = t["tile_m"] + 2, t["tile_n"] + 3
    rows = rng.standard_normal((K, N)) * 10.0 ** rng.uniform(-3, 3, (K, N))       # asymmetric
    assert _same(E.bootstrap_sums(np.eye(K, dtype=np.int32), rows), rows)         # one term each: exact
    ones = E.bootstrap_sums(np.ones((1, K), dtype=np.int32), rows)
    exact, mag = BO.exact_sums(np.ones((1, K), dtype=np.int64), rows)
    assert np.all(np.abs(ones - exact) <= (K + 2) * U * mag)
    cnt, _ = _operands(rng, 5, N, K)
    cnt[2] = 0
    got = E.bootstrap_sums(cnt, rows)
    assert np.all(got[2] == 0.0) and not np.signbit(got[2]).any()
    assert _same(E.bootstrap_sums(cnt, rows), got)


def test_a_replicas_sums_do_not_depend_on_its_company():
    """Alone, in the middle of a batch, across a device chunk, with other replicas around it: bit for bit."""
    t = _tiling()
    rng = np.random.default_rng(23)
    M, N, K = t["tile_m"] + 40, 37, t["k_slice"] + t["stage_k"] + 3              # two slices
    cnt, rows = _operands(rng, M, N, K)
    full = E.bootstrap_sums(cnt, rows)
    pick = t["tile_m"] + 9
    assert _same(E.bootstrap_sums(cnt[pick:pick + 1], rows), full[pick:pick + 1])
    assert _same(E.bootstrap_sums(cnt[100:pick + 5], rows), full[100:pick + 5])
    assert _same(E.bootstrap_sums(cnt[::-1], rows), full[::-1])
    M2 = t["max_chunk"] + 3                                                       # two device chunks
    cnt2, rows2 = _operands(rng, M2, 9, 50)
    full2 = E.bootstrap_sums(cnt2, rows2)
    assert _same(E.bootstrap_sums(cnt2[M2 - 2:], rows2), full2[M2 - 2:])
    assert _same(E.bootstrap_sums(cnt2[5:t["max_chunk"]], rows2), full2[5:t["max_chunk"]])


# -------------------------------------------------------------------------------------------- 3. rows
@pytest.mark.parametrize("grid", [(4, 5), (18, 30)])
def test_rows_bitwise_first_level(grid):
    out = synthetic_out(seed=31, Q=70, nz=grid[0], nn=grid[1])
    Q, p = 70, out["p_dlas"]
    keep = np.arange(Q) % 4 != 2
    p[9] = 0.05                                        # at the threshold: dropped (strict >)
    p[11] = np.nextafter(0.05, 1.0)
    for kp, thresh in ((None, 0.05), (keep, 0.05), (keep, 0.4)):
        got = E.bootstrap_rows(out["bin_planes"], p, kp, thresh)
        want = BO.rows(out["bin_planes"], p, kp, thresh)
        assert got.shape == want.shape and _same(got, want)
        assert np.all(got[5] == 0.0) and np.all(got[9] == 0.0) and (thresh > 0.05 or np.any(got[11] != 0.0))
        assert kp is None or np.all(got[2] == 0.0)
    wide = E.bootstrap_rows(out["bin_planes"], p, keep, columns=want.shape[1] + 6)
    assert _same(wide[:, :want.shape[1]], BO.rows(out["bin_planes"], p, keep)) and np.all(wide[:, want.shape[1]:] == 0.0)


@pytest.mark.parametrize("D", [1, 2, 4])
def test_rows_bitwise_all_levels(D):
    out = synthetic_out(seed=32, Q=50, nz=3, nn=7, D=D)
    P = out["model_posteriors"][:, 1:1 + D].copy()
    P[11, D - 1] = np.nan                              # a NaN level posterior is skipped, the others count
    keep = np.arange(50) % 5 != 0
    got = E.bootstrap_rows(out["bin_planes_levels"], out["p_dlas"], keep, 0.05, P)
    assert _same(got, BO.rows(out["bin_planes_levels"], out["p_dlas"], keep, 0.05, P))
    assert np.all(got[5] == 0.0) and (D == 1 or np.any(got[11] != 0.0))


def test_rows_over_more_than_one_device_chunk():
    """450 spectra of 4 levels on a 32 x 32 grid: more than one 64 MiB chunk of planes."""
    out = synthetic_out(seed=33, Q=450, nz=32, nn=32, D=4)
    P = out["model_posteriors"][:, 1:]
    got = E.bootstrap_rows(out["bin_planes_levels"], out["p_dlas"], None, 0.05, P)
    assert _same(got, BO.rows(out["bin_planes_levels"], out["p_dlas"], None, 0.05, P))


# ---------------------------------------------------------------------------------------- 4. pipeline
def test_one_call_is_counts_then_sums():
    t = _tiling()
    rng = np.random.default_rng(41)
    Q = 1500
    mem = np.sort(rng.permutation(Q)[:1301])
    so = np.array([0, 257, 258, 1027, 1301])
    rows = rng.standard_normal((Q, 131)) * 10.0 ** rng.uniform(-3, 3, (Q, 131))
    for B, first in ((7, 0), (t["tile_m"] + 1, 1000)):
        got = E.bootstrap(rows, B, 99, so, mem, first_replica=first)
        assert _same(got, E.bootstrap_sums(E.bootstrap_counts(Q, B, 99, so, mem, first_replica=first), rows))
    small = rows[:20, :11]
    B = t["max_chunk"] + 2                                                        # two device chunks
    got = E.bootstrap(small, B, 5, SMALL_SO, SMALL_MEM)
    ms = L.last_call_kernel_ms()
    assert _same(got, E.bootstrap_sums(BO.counts(20, B, 5, SMALL_SO, SMALL_MEM), small))
    assert len(ms) == 6 and all(v >= 0.0 for v in ms)                             # draws, product, reduction per chunk


def test_sample_errors_on_a_processed_run():
    """``process_qsos(summaries=...)`` on 200 synthetic sightlines, then 64 replicas on the device against the
    host route (``cddf_moments`` on gathered spectra).  All terms of the compared sums are non-negative, so the
    bound of test_sums_... is relative: a device sum is within (Q + 2) u of exact, a host one within Q u (numpy's
    sequential adds), the sum over a bin's nn columns adds nn u on each side, the path is (Q + 2) u against fsum's
    one, and the ratio and the conversion's five operations one each: (3 Q + 2 nn + 20) u of the value; the
    percentiles interpolate between order statistics with weights that sum to one (two more roundings)."""
    k, Q, S, B = 4, 200, 256, 64
    model = syn.make_model(k=k)
    samples = syn.make_samples(S)
    packed = syn.pack_spectra(syn.make_dr12q_like_spectra(model, Q))
    rng = np.random.default_rng(3)
    prior = dict(z_qsos=rng.uniform(2.0, 4.5, 400), dla_ind=rng.uniform(size=400) < 0.12)
    grid = dict(z_edges=np.linspace(1.8, 4.6, 6), log_nhi_edges=np.linspace(20.0, 23.0, 4))
    out = PR.process_qsos(model, samples, packed, prior, params=set_parameters(k=k), summaries=grid, save_samples=False)
    snr_keep = np.arange(Q) % 9 != 4
    strata = CAT.bootstrap_strata(out["min_z_dlas"], out["max_z_dlas"], num_strata=4)
    kw = dict(replicas=B, seed=2020, keep=snr_keep, strata=strata)
    dev = CAT.sample_errors(out, **kw)
    host = CAT.sample_errors(out, sums=BO.sums_via_cddf_moments, **kw)
    nn = 3
    tol = (3 * Q + 2 * nn + 20) * U
    assert dev["z"].size >= 3 and _same(dev["z"], host["z"])
    for name in ("dndx", "omega"):
        d, h = dev[f"{name}_replicas"], host[f"{name}_replicas"]
        assert d.shape == (B, dev["z"].size) and _same(np.isnan(d), np.isnan(h))
        ok = ~np.isnan(h)
        worst = np.max(np.abs(d[ok] - h[ok]) / np.where(h[ok] != 0, np.abs(h[ok]), 1.0))
        print(f"{name}: worst replica deviation {worst / U:.1f} x 2^-53 (bound {tol / U:.0f})")
        assert np.all(np.abs(d[ok] - h[ok]) <= tol * np.abs(h[ok])) and np.all(h[ok] >= 0) and np.ptp(h[ok]) > 0
        for key in (f"{name}_median", f"{name}_68", f"{name}_95"):
            assert np.all(np.abs(dev[key] - host[key]) <= (tol + 2 * U) * np.abs(host[key])), key
        assert np.all(dev[f"{name}_95"][0] >= dev[f"{name}_68"][0]) and np.all(dev[f"{name}_68"][1] >= dev[f"{name}_95"][1])
    # the replica sums behind them, and a replica alone
    bm = CAT.bootstrap_moments(out, B, 2020, keep=snr_keep, strata=strata)
    one = CAT.bootstrap_moments(out, 1, 2020, keep=snr_keep, strata=strata, first_replica=17)
    for key in bm:
        assert _same(one[key][0], bm[key][17]), key


# --------------------------------------------------------------------------------------------- 5. SNR
def _snr_case(rng, dt, n_set, n_below, zmax, special=None):
    """A spectrum with n_below pixels at or blueward of the Lyman-alpha edge of zmax and n_set redward."""
    edge = 1215.67 * (1.0 + zmax)
    w = np.concatenate([edge - 1.0 - np.sort(rng.random(n_below))[::-1] * 500.0, edge + 0.5 + np.sort(rng.random(n_set)) * 60.0])
    n = n_set + n_below
    flux = rng.normal(1.0, 0.8, n)
    nv = rng.random(n) * 0.3 + 1e-3
    if special == "ties" and n_set >= 4:
        flux[n_below:] = np.where(np.arange(n_set) % 2, 0.5, 2.0)
        nv[n_below:] = 0.25
    if special == "inf" and n_set:
        nv[n_below + n_set // 2] = np.inf
    if special == "nan" and n_set:
        flux[n_below + n_set // 3] = np.nan
    if special == "nan_below" and n_below:
        flux[0] = np.nan                                # outside the set: ignored
    if special == "negative" and n_set:
        flux[n_below:] = -np.abs(flux[n_below:]) * 3.0
    return w.astype(dt), flux.astype(dt), nv.astype(dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("with_norm", [False, True])
def test_snrs_bitwise(dt, with_norm):
    rng = np.random.default_rng(51)
    cases = [(n, nb, None) for n in (0, 1, 2, 3, 63, 64, 65, 257, 1025) for nb in (0, 41)]
    cases += [(n, 7, sp) for n in (4, 10, 11, 64) for sp in ("ties", "inf", "nan", "nan_below", "negative")]
    zs = rng.uniform(2.0, 5.0, len(cases))
    cells = [_snr_case(rng, dt, n, nb, z, sp) for (n, nb, sp), z in zip(cases, zs)]
    norm = rng.uniform(0.5, 20.0, len(cases)) if with_norm else None
    got = E.spectrum_snrs([c[0] for c in cells], [c[1] for c in cells], [c[2] for c in cells], zs, norm)
    want = np.array([BO.find_snr(*c, z, None if norm is None else norm[i]) for i, (c, z) in enumerate(zip(cells, zs))], dtype=dt)
    assert got.dtype == dt and _same(got, want), np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    for i, (n, nb, sp) in enumerate(cases):
        assert np.isnan(got[i]) == (n == 0 or sp == "nan"), (n, nb, sp)
    # an infinite ratio in the middle of the order: only where it is the median does the SNR fall to 0
    assert np.all(got[~np.isnan(got)] >= 0)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_snr_wavelength_edge_is_strict(dt):
    """A pixel exactly at 1215.67 (1 + max_z) is out; the next representable wavelength is in."""
    zmax, w0 = None, None
    for cand in np.arange(4000.0, 4400.0, 0.25):       # exactly representable in float32
        z = cand / 1215.67 - 1.0
        if 1215.67 * (1.0 + z) == cand:
            zmax, w0 = z, dt(cand)
            break
    assert zmax is not None
    w = np.array([w0 - dt(1), w0, np.nextafter(w0, dt(np.inf)), w0 + dt(1)], dtype=dt)
    flux, nv = np.array([1, 1, 2, 4], dtype=dt), np.array([100, 100, 1, 1], dtype=dt)
    got = E.spectrum_snrs([w, w[:2]], [flux, flux[:2]], [nv, nv[:2]], [zmax, zmax])
    assert got.dtype == dt and got[0] == BO.find_snr(w, flux, nv, zmax) == dt(1) / dt(0.375) and np.isnan(got[1])


def test_compute_snrs_and_save(tmp_path):
    rng = np.random.default_rng(53)
    cells = [_snr_case(rng, np.float32, 40 + q, 300, 2.5 + 0.1 * q) for q in range(6)]
    pre = dict(all_wavelengths=[c[0] for c in cells], all_flux=[c[1] for c in cells], all_noise_variance=[c[2] for c in cells],
               all_normalizers=rng.uniform(1.0, 5.0, 6))
    test_ind = np.array([True, False, True, True, False, True])
    zmax = (2.5 + 0.1 * np.arange(6))[test_ind]
    snrs = CAT.compute_snrs(pre, dict(max_z_dlas=zmax, test_ind=test_ind))
    want = [BO.find_snr(*cells[q], 2.5 + 0.1 * q, pre["all_normalizers"][q]) for q in np.flatnonzero(test_ind)]
    assert snrs.dtype == np.float32 and _same(snrs, np.array(want, dtype=np.float32))
    PR.save_snrs(str(tmp_path / "snrs.mat"), snrs)
    from gp_dla_detection_amd.matv73 import loadmat
    back = loadmat(str(tmp_path / "snrs.mat"))["snrs"]
    assert back.shape == (1, 4) and back.dtype == np.float32 and _same(back.ravel(), snrs)


# ------------------------------------------------------------------------------------------ 6. EINVAL
def test_argument_errors():
    rows = np.ones((6, 3))
    so, mem = [0, 2, 6], [0, 1, 2, 3, 4, 5]
    for fn in (lambda **kw: E.bootstrap_counts(6, kw.pop("replicas", 2), 1, kw.get("so", so), kw.get("mem", mem)),
               lambda **kw: E.bootstrap(rows, kw.pop("replicas", 2), 1, kw.get("so", so), kw.get("mem", mem))):
        fn()
        _raises_einval(fn, replicas=0)
        _raises_einval(fn, mem=[0, 1, 2, 3, 4, 6])             # outside 0..Q-1
        _raises_einval(fn, mem=[0, 1, 2, 3, 4, -1])
        _raises_einval(fn, mem=[0, 1, 2, 3, 4, 1])             # listed twice
        _raises_einval(fn, so=[0, 2, 2, 6])                    # an empty stratum
        _raises_einval(fn, so=[0, 6, 6])
    _raises_einval(E.bootstrap_counts, 0, 2, 1, [0, 1], [0])   # Q < 1
    _raises_einval(E.bootstrap_counts, 6, 2, 1, so, mem, first_replica=-1)
    _raises_einval(E.bootstrap, np.ones((0, 3)), 2, 1, [0, 1], [0])
    cnt = np.ones((2, 6), dtype=np.int32)
    E.bootstrap_sums(cnt, rows)
    _raises_einval(E.bootstrap_sums, np.ones((0, 6), dtype=np.int32), rows)       # B < 1
    _raises_einval(E.bootstrap_sums, np.ones((2, 0), dtype=np.int32), np.ones((0, 3)))
    bad = cnt.copy()
    bad[1, 4] = -1
    _raises_einval(E.bootstrap_sums, bad, rows)
    for v in (np.nan, np.inf, -np.inf):
        r = rows.copy()
        r[5, 2] = v
        _raises_einval(E.bootstrap_sums, cnt, r)
        _raises_einval(E.bootstrap, r, 2, 1, so, mem)
    assert b"rows[5][2]" in L.load().gpdla_last_error()
    planes, p = np.ones((3, 5, 2, 2)), np.full(3, 0.5)
    E.bootstrap_rows(planes, p)
    lib = L.load()
    out = np.zeros((3, 16))
    args = lambda D=1, Q=3, nz=2, nn=2, ld=16: (0, L.ptr(planes), D, L.ptr(p), None, None, Q, nz, nn, 0.05, L.ptr(out), ld)
    assert lib.gpdla_bootstrap_rows_f64(*args()) == L.GPDLA_OK
    for kw in (dict(D=2), dict(D=0), dict(Q=0), dict(nz=0), dict(nz=64, nn=64), dict(ld=15)):
        assert lib.gpdla_bootstrap_rows_f64(*args(**kw)) == L.GPDLA_EINVAL, kw
    w = [np.linspace(4000, 9000, 10)]
    E.spectrum_snrs(w, w, w, [2.0])
    off = np.array([0, 5, 3], dtype=np.int64)
    x, z, s = np.ones(5), np.ones(2), np.ones(2)
    c64 = np.ctypeslib.ctypes.c_int64
    assert lib.gpdla_spectrum_snrs_f64(0, 2, L.ptr(off, c64), L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(z), None, L.ptr(s)) == L.GPDLA_EINVAL
    assert lib.gpdla_spectrum_snrs_f64(0, 0, L.ptr(off, c64), L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(z), None, L.ptr(s)) == L.GPDLA_EINVAL

"""Posterior summaries on the GPU (csrc/posterior_summary.hip) against the numpy oracle
(posterior_summary_oracle.py): the kernel alone over sizes, row shapes and grids, the base chains, the
reference's own numbers (tests/golden/posterior_summary.npz), the engine call (bitwise against the
standalone kernel, batching, repeats, memory spaces, with and without the sample buffers) and the
argument errors."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import posterior_summary_oracle as PO  # noqa: E402
from gp_dla_detection_amd import _lib as L  # noqa: E402
from gp_dla_detection_amd import synthetic as syn  # noqa: E402
from gp_dla_detection_amd.engine import Engine, posterior_summary  # noqa: E402
from gp_dla_detection_amd.parameters import set_parameters  # noqa: E402
from test_posterior_summary import GOLDEN, check_against_reference  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---------------------------------------------------------------------------------- 1. kernel alone
ROWS = ("flat", "spike", "two", "last", "pow2", "allnan", "neginf", "nans", "wide", "smooth")


def _rows(S, rng):
    flat = np.zeros(S)
    spike = np.full(S, -np.inf)
    spike[S // 3] = 5.0
    two = rng.normal(0.0, 1.0, S) - 10.0
    two[S // 5] = two[(4 * S) // 5] = 2.5                # two equal maxima: the first wins
    last = rng.normal(0.0, 1.0, S)
    last[S - 1] = 9.0
    # 0 / 1 weights with NaNs, the finite count a power of two: pi = 2^-k, every sum exact
    P = 1 << (S.bit_length() - 1)
    if P == S and S > 1:
        P //= 2
    pow2 = np.full(S, np.nan)
    pow2[rng.permutation(S)[:P]] = 2.0
    allnan = np.full(S, np.nan)
    neginf = np.full(S, -np.inf)
    nans = rng.normal(0.0, 3.0, S)
    nans[rng.random(S) < 0.2] = np.nan
    nans[rng.integers(S)] = 1.0
    wide = -1e5 * rng.random(S)                          # dynamic range 1e5 in l
    smooth = rng.normal(0.0, 1.0, S)
    return np.stack([flat, spike, two, last, pow2, allnan, neginf, nans, wide, smooth]), P


def _grids(S, log_nhi):
    """(name, z_edges, log_nhi_edges): 1x1, 6x1, 1x6, 7x5, the 32x32 cap, and one covering part of the
    samples whose inner and upper log N_HI edges are sample values (an edge value belongs to the bin it
    opens; the grid's last edge is outside)."""
    z_lo, z_hi, n_lo, n_hi = 1.7, 4.6, 19.9, 23.1
    full = lambda nz, nn: (np.linspace(z_lo, z_hi, nz + 1), np.linspace(n_lo, n_hi, nn + 1))  # noqa: E731
    inner = np.sort(log_nhi[(log_nhi > 20.6) & (log_nhi < 21.6)])
    mid, top = (inner[inner.size // 3], inner[-1]) if inner.size >= 2 else (21.0, 21.7)
    return [("1x1",) + full(1, 1), ("6x1",) + full(6, 1), ("1x6",) + full(1, 6), ("7x5",) + full(7, 5),
            ("32x32",) + full(32, 32), ("partial", np.array([2.5, 2.8, 3.2]), np.array([20.5, mid, top]))]


@pytest.mark.parametrize("S", [1, 63, 64, 65, 333, 1025, 10000])
def test_kernel_alone(S):
    rng = np.random.default_rng(300 + S)
    ll, P = _rows(S, rng)
    R = ll.shape[0]
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)
    # N_HI to 8 significant bits: with pi a power of two, N pi, N^2 pi and N^2 pi^2 then sum exactly in
    # any order (36-bit terms over a 2^10 range, 10^4 of them), so the pow2 row is bitwise on every plane
    m, e = np.frexp(10.0 ** log_nhi)
    nhi = np.ldexp(np.round(m * 256.0) / 256.0, e)
    min_z = np.linspace(1.8, 2.6, R)
    max_z = min_z + np.linspace(0.4, 1.9, R)
    want_ind, want_ll, want_z, want_n = PO.map_parameters(ll[None], None, min_z, max_z, offset, log_nhi)
    only = posterior_summary(ll, offset, log_nhi, nhi, min_z, max_z)          # MAP only: no grid
    assert "bin_planes" not in only and only["map_sample_inds"].dtype == np.int32
    tol = (S + 16) * 2.0 ** -52
    for name, ez, en in _grids(S, log_nhi):
        got = posterior_summary(ll, offset, log_nhi, nhi, min_z, max_z, z_edges=ez, log_nhi_edges=en)
        for key in ("map_sample_inds", "map_log_likelihoods", "MAP_z_dlas", "MAP_log_nhis"):
            assert _same(got[key], only[key]), (name, key)
        assert np.array_equal(got["map_sample_inds"], want_ind)
        assert _same(got["map_log_likelihoods"], want_ll)
        assert _same(got["MAP_z_dlas"], want_z[:, :, :1]) and _same(got["MAP_log_nhis"], want_n[:, :, :1])
        planes = got["bin_planes"]
        assert planes.shape == (R, 5, ez.size - 1, en.size - 1)
        worst = 0.0
        for r, rname in enumerate(ROWS):
            want, count = PO.bin_planes(ll[r], min_z[r], max_z[r], offset, log_nhi, nhi, ez, en)
            if rname in ("allnan", "neginf"):
                assert not planes[r].any(), (name, rname)
                continue
            assert not planes[r][:, count == 0].any(), (name, rname, "empty bins are exactly 0")
            if rname == "pow2":      # membership through sum pi: finite samples per bin, exactly
                fin = ~np.isnan(ll[r])
                iz = PO.bin_index(ez, PO.sample_z(min_z[r], max_z[r], offset))
                inn = PO.bin_index(en, log_nhi)
                members = np.zeros(count.shape)
                np.add.at(members, (iz[fin & (iz >= 0) & (inn >= 0)], inn[fin & (iz >= 0) & (inn >= 0)]), 1.0)
                assert np.array_equal(planes[r, 0] * P, members), (name, "membership")
                assert np.array_equal(planes[r], want), (name, "pow2 planes bitwise")
                continue
            if rname in ("flat", "spike"):
                assert np.array_equal(planes[r, 0] > 0, want[0] > 0), (name, rname, "membership")
            err = np.abs(planes[r] - want)
            assert np.all(err <= tol * np.abs(want)), (name, rname, float((err / np.maximum(np.abs(want), 1e-300)).max()))
            nz = want != 0
            if nz.any():
                worst = max(worst, float((err[nz] / np.abs(want[nz])).max()))
        print(f"S={S} grid {name}: max rel err {worst:.3g} (bound {tol:.3g})")
    assert want_ind[0].tolist() == [0, S // 3, S // 5, S - 1, int(np.flatnonzero(~np.isnan(ll[4]))[0]), -1, 0,
                                    want_ind[0, 7], want_ind[0, 8], want_ind[0, 9]]
    assert np.isnan(only["map_log_likelihoods"][0, 5]) and np.isnan(only["MAP_z_dlas"][0, 5]).all()
    assert only["map_log_likelihoods"][0, 6] == -np.inf and np.isfinite(only["MAP_z_dlas"][0, 6, 0])


def test_row_stride_and_repeat():
    """Two calls are bitwise equal, and a row's outputs do not depend on the rows around it."""
    S = 1025
    rng = np.random.default_rng(9)
    ll = rng.normal(0.0, 2.0, (7, S))
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)
    nhi = 10.0 ** log_nhi
    min_z, max_z = np.linspace(2.0, 2.5, 7), np.linspace(3.0, 4.2, 7)
    ez, en = np.linspace(2.0, 4.0, 8), np.linspace(20.0, 23.0, 6)
    a = posterior_summary(ll, offset, log_nhi, nhi, min_z, max_z, z_edges=ez, log_nhi_edges=en)
    b = posterior_summary(ll, offset, log_nhi, nhi, min_z, max_z, z_edges=ez, log_nhi_edges=en)
    c = posterior_summary(ll[2:5], offset, log_nhi, nhi, min_z[2:5], max_z[2:5], z_edges=ez, log_nhi_edges=en)
    for key in a:
        assert _same(a[key], b[key]), key
        axis = 0 if key == "bin_planes" else 1
        assert _same(np.take(a[key], [2, 3, 4], axis=axis), c[key]), key


# ------------------------------------------------------------------------------------------ 2. chains
@pytest.mark.parametrize("levels", [3, 4])
def test_chains(levels):
    S, R = 333, 6
    rng = np.random.default_rng(40 + levels)
    ll = rng.normal(0.0, 2.0, (levels, R, S))
    ll[rng.random(ll.shape) < 0.1] = np.nan
    ll[levels - 1, 4] = np.nan                                   # no MAP sample at the deepest level of row 4
    base = rng.integers(0, S, (levels - 1, R, S)).astype(np.int32)
    base[rng.random(base.shape) < 0.3] = -1
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)
    min_z, max_z = rng.uniform(1.9, 2.4, R), rng.uniform(2.9, 4.3, R)
    want_ind, want_ll, want_z, want_n = PO.map_parameters(ll, base, min_z, max_z, offset, log_nhi)
    broken = np.isnan(want_z[:, :, 0]) & (want_ind >= 0)
    assert broken[1:].any() and (~np.isnan(want_z[levels - 1, :, levels - 1])).any()   # both outcomes occur
    got = posterior_summary(ll, offset, log_nhi, 10.0 ** log_nhi, min_z, max_z, base_sample_inds=base)
    assert np.array_equal(got["map_sample_inds"], want_ind) and _same(got["map_log_likelihoods"], want_ll)
    assert got["MAP_z_dlas"].shape == (levels, R, levels)
    assert _same(got["MAP_z_dlas"], want_z[:, :, :levels]) and _same(got["MAP_log_nhis"], want_n[:, :, :levels])
    # the kernel's own slots beyond the level count stay NaN (the C arrays are GPDLA_MAX_DLAS wide)
    for d in range(levels):
        assert np.isnan(got["MAP_z_dlas"][d, :, d + 1:]).all()


# ------------------------------------------------------------------------------------------ 3. golden
def test_golden_reference_numbers():
    """The kernel on the fixture's rows, through catalog.cddf_moments, against the reference's
    _get_z_nhi_hist numbers at the bar test_posterior_summary.py measured for the oracle; the MAP pairs
    against find_max_like bit for bit."""
    g = np.load(GOLDEN)
    got = posterior_summary(g["sample_log_likelihoods"], g["offset_samples"], g["log_nhi_samples"], g["nhi_samples"],
                            g["min_z_dlas"], g["max_z_dlas"], z_edges=g["z_edges"], log_nhi_edges=g["log_nhi_edges"])
    worst = check_against_reference(g, got["bin_planes"])
    print(f"kernel vs reference: max rel deviation {worst:.3e}")
    rows = g["map_rows"]
    assert np.array_equal(got["MAP_log_nhis"][0, rows, 0], g["ref_max_like"][:, 0])
    assert np.array_equal(got["MAP_z_dlas"][0, rows, 0], g["ref_max_like"][:, 1])


# ------------------------------------------------------------------------------------------ 4. engine
S_LEVEL = 333
Z_EDGES, N_EDGES = np.linspace(1.6, 4.6, 8), np.linspace(20.0, 23.0, 6)
SUMMARY_KEYS = ("map_sample_inds", "map_log_likelihoods", "MAP_z_dlas", "MAP_log_nhis", "bin_planes")
MULTI_KEYS = ("log_likelihoods_no_dla", "log_likelihoods_dla", "min_z_dlas", "max_z_dlas", "num_pixels")


def _spectra(model):
    mk = dict(mask_fraction=0.05)
    return [syn.make_spectrum(model, 0, z_qso=2.6, n_target=300, **mk),
            syn.make_spectrum(model, 1, z_qso=3.1, n_target=None, **mk),
            syn.make_spectrum(model, 2, n_target=270, **mk),
            syn.make_spectrum(model, 3, n_target=300, mask_fraction=1.0)]      # J = 0: NaN rows


@pytest.mark.parametrize("k,D", [(4, 1), (4, 3), (20, 1), (20, 3)])
def test_engine_summaries(k, D):
    model = syn.make_model(k=k)
    samples = syn.make_samples(S_LEVEL)
    packed = syn.pack_spectra(_spectra(model))
    params = set_parameters(k=k)
    lognhi = samples["log_nhi_samples"]
    kw = dict(z_edges=Z_EDGES, log_nhi_edges=N_EDGES)
    with Engine(model, samples, params) as eng:
        plain = eng.process_multi(packed, D)
        full = eng.process_summaries(packed, D, lognhi, want_samples=True, **kw)
        lean = eng.process_summaries(packed, D, lognhi, **kw)
        again = eng.process_summaries(packed, D, lognhi, **kw)
        dev = eng.process_summaries(packed, D, lognhi, memory="device", **kw)
        only = eng.process_summaries(packed, D, lognhi)
        stats = eng.summary_stats()
    assert stats["summary_launches"] == 5 and stats["summary_ms"] > 0
    # process_multi's outputs are what they are without summaries
    for key in MULTI_KEYS + ("sample_log_likelihoods_dla", "base_sample_inds"):
        assert _same(full[key], plain[key]), key
    assert "sample_log_likelihoods_dla" not in lean and "base_sample_inds" not in lean
    for other in (lean, again, dev):
        for key in MULTI_KEYS + SUMMARY_KEYS:
            assert _same(full[key], other[key]), key
    assert "bin_planes" not in only
    for key in SUMMARY_KEYS[:4]:
        assert _same(full[key], only[key]), key
    # ... and the summaries are the standalone kernel on the arrays the same run returned
    alone = posterior_summary(full["sample_log_likelihoods_dla"], samples["offset_samples"], lognhi, samples["nhi_samples"],
                              full["min_z_dlas"], full["max_z_dlas"],
                              base_sample_inds=full["base_sample_inds"] if D > 1 else None, **kw)
    for key in SUMMARY_KEYS:
        assert _same(full[key], alone[key]), key
    assert full["MAP_z_dlas"].shape == (D, 4, D) and full["bin_planes"].shape == (4, 5, 7, 5)
    assert (full["map_sample_inds"][:, :3] >= 0).all() and (full["map_sample_inds"][:, 3] == -1).all()
    assert np.isnan(full["MAP_z_dlas"][:, 3]).all() and not full["bin_planes"][3].any()
    mass = full["bin_planes"][:3, 0].sum(axis=(1, 2))
    assert np.all((mass > 0) & (mass < 1 + 1e-12))
    # any split into device batches
    for mb in (1, 3):
        with Engine(model, samples, params, max_batch_spectra=mb) as eng:
            batched = eng.process_summaries(packed, D, lognhi, **kw)
        for key in MULTI_KEYS + SUMMARY_KEYS:
            assert _same(full[key], batched[key]), (mb, key)


# ------------------------------------------------------------------------------------------ 5. errors
def _raises_einval(fn, *a, **kw):
    with pytest.raises(L.GpdlaError) as ei:
        fn(*a, **kw)
    assert ei.value.code == L.GPDLA_EINVAL, ei.value


def test_argument_errors():
    S = 64
    rng = np.random.default_rng(1)
    ll = rng.normal(size=(2, S))
    offset, log_nhi = rng.random(S), rng.uniform(20.0, 23.0, S)
    nhi = 10.0 ** log_nhi
    args = (ll, offset, log_nhi, nhi, [2.0, 2.1], [3.0, 3.1])
    ez, en = np.linspace(2.0, 4.0, 5), np.linspace(20.0, 23.0, 4)
    bad_grids = [
        (np.array([2.0, 3.0, 3.0, 4.0]), en),              # not strictly increasing
        (ez[::-1].copy(), en),
        (ez, np.array([20.0, np.nan, 23.0])),              # non-finite
        (ez, np.array([20.0, 21.0, np.inf])),
        (np.linspace(2.0, 4.0, 34), np.linspace(20.0, 23.0, 33)),   # 33 x 32 bins: above the cap
        (np.array([2.0]), en),                             # nz = 0 with nn = 3
        (ez, np.array([20.0])),
    ]
    for bz, bn in bad_grids:
        _raises_einval(posterior_summary, *args, z_edges=bz, log_nhi_edges=bn)
    ok = posterior_summary(*args, z_edges=np.linspace(2.0, 4.0, 33), log_nhi_edges=np.linspace(20.0, 23.0, 33))
    assert ok["bin_planes"].shape == (2, 5, 32, 32)        # the cap itself is fine
    _raises_einval(posterior_summary, np.zeros((2, 2, S)), *args[1:])          # two levels without base indices

    model = syn.make_model(k=8)
    samples = syn.make_samples(S)
    packed = syn.pack_spectra([syn.make_spectrum(model, 0, n_target=220)])
    with Engine(model, samples, set_parameters(k=8)) as eng:
        for bz, bn in bad_grids:
            _raises_einval(eng.process_summaries, packed, 1, samples["log_nhi_samples"], z_edges=bz, log_nhi_edges=bn)
        _raises_einval(eng.process_summaries, packed, 0, samples["log_nhi_samples"])
        good = eng.process_summaries(packed, 1, samples["log_nhi_samples"], z_edges=ez, log_nhi_edges=en)
        assert good["bin_planes"].shape == (1, 5, 4, 3)
        # null required arrays, straight at the C ABI
        lib = eng.lib
        offsets = np.ascontiguousarray(packed["offsets"], dtype=np.int64)
        arrs = {key: np.ascontiguousarray(packed[key], dtype=np.float64) for key in
                ("wavelengths", "flux", "noise_variance", "z_qsos")}
        mask = np.ascontiguousarray(packed["pixel_mask"], dtype=np.uint8)
        sp = L.Spectra(memory=L.MEM_HOST, num_spectra=1, offsets=L.ptr(offsets, C.c_int64),
                       wavelengths=L.ptr(arrs["wavelengths"]), flux=L.ptr(arrs["flux"]),
                       noise_variance=L.ptr(arrs["noise_variance"]), pixel_mask=L.ptr(mask, C.c_uint8),
                       z_qsos=L.ptr(arrs["z_qsos"]))
        md = L.MultiDla(max_dlas=1, min_z_separation=0.01, occam_log_penalty=0.0, resample_uniforms=None,
                        forced_base_inds=None)
        null, dla = np.zeros(1), np.zeros(1)
        rs = L.ResultsMulti(memory=L.MEM_HOST, log_likelihoods_no_dla=L.ptr(null), log_likelihoods_dla=L.ptr(dla),
                            sample_log_likelihoods_dla=None, sample_ld=S, base_sample_inds=None, min_z_dlas=None,
                            max_z_dlas=None, num_pixels=None)
        lognhi = np.ascontiguousarray(samples["log_nhi_samples"], dtype=np.float64)
        ind, mll, mz, mn = np.zeros(1, np.int32), np.zeros(1), np.zeros(4), np.zeros(4)
        planes = np.zeros((1, 5, 4, 3))

        def call(spec_kw=None, sum_kw=None, spec=True, sums=True):
            skw = dict(log_nhi_samples=L.ptr(lognhi), num_z_bins=4, num_nhi_bins=3, z_edges=L.ptr(ez), log_nhi_edges=L.ptr(en))
            skw.update(spec_kw or {})
            mkw = dict(memory=L.MEM_HOST, map_sample_inds=L.ptr(ind, C.c_int32), map_log_likelihoods=L.ptr(mll),
                       map_z_dlas=L.ptr(mz), map_log_nhis=L.ptr(mn), bin_planes=L.ptr(planes))
            mkw.update(sum_kw or {})
            s_, m_ = L.SummarySpec(**skw), L.Summaries(**mkw)
            return lib.gpdla_engine_process_summaries(eng._h, C.byref(sp), C.byref(md), C.byref(rs),
                                                      C.byref(s_) if spec else None, C.byref(m_) if sums else None)
        assert call() == L.GPDLA_OK
        assert _same(planes, good["bin_planes"])
        assert call(spec=False) == L.GPDLA_EINVAL and call(sums=False) == L.GPDLA_EINVAL
        for key in ("log_nhi_samples", "z_edges", "log_nhi_edges"):
            assert call(spec_kw={key: None}) == L.GPDLA_EINVAL, key
        for key in ("map_sample_inds", "map_log_likelihoods", "map_z_dlas", "map_log_nhis", "bin_planes"):
            assert call(sum_kw={key: None}) == L.GPDLA_EINVAL, key


# ------------------------------------------------------------------------------- 6. process_qsos
def test_four_dla_run_without_sample_arrays(tmp_path):
    """max_dlas = 4 with save_samples=False: the file holds evidences, posteriors, MAP parameters and
    bin planes, and no sample array; the summaries equal those of the run that keeps the arrays."""
    from gp_dla_detection_amd import matv73 as M
    from gp_dla_detection_amd import process as PR
    k, D = 20, 4
    model = syn.make_model(k=k)
    samples = syn.make_samples(S_LEVEL)
    packed = syn.pack_spectra(_spectra(model)[:3])
    params = set_parameters(k=k)
    grid = dict(z_edges=Z_EDGES, log_nhi_edges=N_EDGES)
    lean = PR.process_qsos(model, samples, packed, params=params, max_dlas=D, summaries=grid, save_samples=False)
    full = PR.process_qsos(model, samples, packed, params=params, max_dlas=D, summaries=grid)
    plain = PR.process_qsos(model, samples, packed, params=params, max_dlas=D)
    assert "sample_log_likelihoods_dla" not in lean and "base_sample_inds" not in lean
    assert full["sample_log_likelihoods_dla"].shape == (3, S_LEVEL, D)
    for key in lean:
        assert _same(lean[key], full[key]), key
    for key in plain:
        assert _same(plain[key], full[key]), key
    assert lean["MAP_z_dlas"].shape == lean["MAP_log_nhis"].shape == lean["map_sample_inds"].shape == (3, D)
    level = np.argmax(lean["model_posteriors"][:, 1:], axis=1)
    for q in range(3):
        assert np.isfinite(lean["MAP_z_dlas"][q, :level[q] + 1]).all() and np.isnan(lean["MAP_z_dlas"][q, level[q] + 1:]).all()
        j = int(lean["map_sample_inds"][q, level[q]]) - 1
        assert j == PO.map_index(full["sample_log_likelihoods_dla"][q, :, level[q]])
        assert lean["MAP_log_nhis"][q, 0] == samples["log_nhi_samples"][j]
    lean["test_ind"] = np.ones(3, dtype=bool)
    path = tmp_path / "processed_qsos_lean.mat"
    PR.save_processed_qsos(str(path), lean)
    r = M.loadmat(str(path))
    assert not {"sample_log_likelihoods_dla", "base_sample_inds"} & set(r)
    assert r["log_likelihoods_dla"].shape == (3, D) and r["model_posteriors"].shape == (3, 1 + D)
    assert r["bin_planes"].shape == (3, 5, 7, 5) and r["MAP_z_dlas"].shape == (3, D)
    assert _same(r["bin_planes"], lean["bin_planes"]) and _same(r["MAP_log_nhis"], lean["MAP_log_nhis"])
    one = PR.process_qsos(model, samples, packed, params=params, summaries=True)       # max_dlas = 1, MAP only
    assert one["MAP_z_dlas"].shape == (3, 1) and one["log_likelihoods_dla"].shape == (3,) and "bin_planes" not in one

"""Bootstrap sample errors on the host (catalog.bootstrap_strata / bootstrap_moments / sample_errors with the
numpy oracle injected through ``sums=``; no GPU): the Philox oracle against its published vector and numpy's
generator, the strata, and the estimators built from the replica sums."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).parent))
import bootstrap_oracle as BO  # noqa: E402
from gp_dla_detection_amd import catalog as CAT  # noqa: E402


def synthetic_out(seed=3, Q=120, nz=4, nn=5, D=1, z_lo=2.0, z_hi=4.0):
    """The variables of a ``process_qsos(summaries=...)`` run that the bootstrap reads, drawn at random: planes of
    the five masses, posteriors (some below the 0.05 cut, one NaN), search ranges that miss some bins."""
    rng = np.random.default_rng(seed)
    planes = rng.random((Q, D, 5, nz, nn)) * np.array([1.0, 1.0, 1e20, 1e40, 1e40])[None, None, :, None, None]
    post = rng.dirichlet(np.ones(D + 1), size=Q)
    post[::7] = np.array([0.97] + [0.03 / D] * D)
    post[5, 1] = np.nan
    p = 1.0 - post[:, 0]
    p[5] = np.nan
    zmin = z_lo + 0.8 * (z_hi - z_lo) * rng.random(Q)
    zmax = zmin + 0.05 + (z_hi - zmin) * rng.random(Q)
    out = dict(bin_planes=planes[:, 0].copy(), p_dlas=p, model_posteriors=post, min_z_dlas=zmin, max_z_dlas=zmax,
               bin_z_edges=np.linspace(z_lo - 0.5, z_hi + 0.5, nz + 1), bin_planes_levels=planes)
    return out


# -------------------------------------------------------------------------------------------- Philox
def test_philox_known_answer():
    """Random123's kat_vectors: philox4x64 10 rounds, counter 0, key 0."""
    assert BO.philox4x64_10((0, 0, 0, 0), (0, 0)) == (0x16554d9eca36314c, 0xdb20fe9d672d0fdc, 0xd7e772cee186176b,
                                                       0x7e68b68aec7ba23b)


def test_philox_matches_numpy_generator():
    """numpy's Philox increments its counter before the first block: random_raw(4) at counter c is the
    function at c + 1."""
    for c, k in (((0, 0, 0, 0), (0, 0)), ((5, 0, 77, 0), (0x0123456789abcdef, 0xfedcba9876543210)),
                 ((2 ** 64 - 2, 3, 2 ** 63, 9), (1, 2 ** 64 - 1))):
        raw = np.random.Philox(counter=np.array(c, dtype=np.uint64), key=np.array(k, dtype=np.uint64)).random_raw(4)
        assert tuple(int(v) for v in raw) == BO.philox4x64_10((c[0] + 1,) + c[1:], k)


def test_draw_rule_counts():
    so, mem = [0, 3, 8], np.array([7, 1, 4, 0, 2, 9, 5, 3])
    c = BO.counts(10, 6, 12345, so, mem)
    assert c.dtype == np.int32 and c.shape == (6, 10)
    assert np.all(c.sum(axis=1) == 8) and np.all(c[:, [7, 1, 4]].sum(axis=1) == 3) and np.all(c[:, [6, 8]] == 0)
    assert np.array_equal(BO.counts(10, 2, 12345, so, mem, first_replica=3), c[3:5])
    assert len({tuple(r) for r in c}) > 1


# -------------------------------------------------------------------------------------------- strata
def test_strata_edges_and_membership():
    rng = np.random.default_rng(0)
    zmax = np.concatenate([2.0 + 2.0 * rng.random(400), [4.9, 5.3, 5.9]])     # a thin high-redshift tail
    zmin = zmax - 0.5 - rng.random(zmax.size)
    zmax[17] = zmin[17] = np.nan
    so, mem = CAT.bootstrap_strata(zmin, zmax)
    assert so.dtype == np.int64 and mem.dtype == np.int32 and so.shape == (10,) and so[0] == 0 and so[-1] == mem.size
    assert np.unique(mem).size == mem.size and 17 not in mem
    # the widening loops, restated
    newmax = np.nanmax(zmax) - 0.2
    while np.sum(zmax > newmax) < 10:
        newmax -= 0.2
    newmin = np.nanmin(zmin) + 0.2
    while np.sum(zmax <= newmin) < 10:
        newmin += 0.2
    assert newmax < np.nanmax(zmax) - 0.2 - 1e-9, "the upper loop must have run"
    assert newmin > np.nanmin(zmin) + 0.2 + 1e-9, "the lower loop must have run"
    edges = np.linspace(newmin, newmax, 10)
    edges[0], edges[-1] = np.nanmin(zmin), np.nanmax(zmax)
    for s in range(9):
        g = mem[so[s]:so[s + 1]]
        assert g.size >= 10 and np.all(np.diff(g) > 0)
        assert np.all((zmax[g] > edges[s]) & (zmax[g] <= edges[s + 1]))
    assert np.nanargmax(zmax) in mem[so[8]:]                       # the last edge is max(max_z), inclusive
    outside = np.setdiff1d(np.arange(zmax.size), mem)
    assert all(not (zmax[q] > edges[0]) for q in outside)          # NaN, or at or below the first edge


def test_strata_too_small_raises():
    rng = np.random.default_rng(1)
    zmax = 2.0 + 2.0 * rng.random(60)
    with pytest.raises(ValueError, match="min_per_stratum"):
        CAT.bootstrap_strata(zmax - 1.0, zmax, num_strata=9, min_per_stratum=10)
    with pytest.raises(ValueError, match="min_per_stratum"):
        CAT.bootstrap_strata(zmax[:5] - 1.0, zmax[:5])
    so, mem = CAT.bootstrap_strata(zmax - 1.0, zmax, num_strata=2, min_per_stratum=10)
    assert so.size == 3 and np.unique(mem).size == mem.size


def test_strata_none_is_one_stratum_of_everything():
    out = synthetic_out(Q=40)
    seen = {}

    def spy(**kw):
        seen.update(kw)
        return BO.sums_all_ones(**kw)
    CAT.bootstrap_moments(out, 2, 9, strata=None, sums=spy)
    assert list(seen["stratum_offsets"]) == [0, 40] and np.array_equal(seen["members"], np.arange(40))
    with pytest.raises(ValueError):
        CAT.bootstrap_moments(out, 2, 9, strata="none", sums=spy)


# ------------------------------------------------------------------------------------ the estimators
def _close(a, b, n):
    """Within n roundings of the larger magnitude (two summation orders of n non-negative terms)."""
    a, b = np.asarray(a), np.asarray(b)
    assert np.all(np.abs(a - b) <= n * 2.0 ** -53 * np.maximum(np.abs(a), np.abs(b))), np.abs(a - b).max()


@pytest.mark.parametrize("keep_some", [False, True])
def test_all_ones_replica_is_the_full_sample(keep_some):
    out = synthetic_out()
    Q = out["p_dlas"].size
    keep = (np.arange(Q) % 3 != 1) if keep_some else None
    bm = CAT.bootstrap_moments(out, 3, 1, keep=keep, strata=None, sums=BO.sums_all_ones)
    for mom, (mk, vk) in enumerate((("means", "variances"), ("moment_means", "moment_variances"))):
        m, v = CAT.cddf_moments(out["bin_planes"], out["p_dlas"], keep, moment=bool(mom))
        for b in range(3):
            _close(bm[mk][b], m, Q + 1)
            _close(bm[vk][b], v, 4 * Q + 4)       # a difference of sums: bounded by the terms' magnitudes below
    ez = out["bin_z_edges"]
    want = [CAT.path_length(a, b, out["min_z_dlas"], out["max_z_dlas"], keep) for a, b in zip(ez[:-1], ez[1:])]
    assert np.array_equal(bm["path"][0], want)                      # fsum both ways: identical
    assert bm["path_total"][0] == CAT.path_length(ez[0], ez[-1], out["min_z_dlas"], out["max_z_dlas"], keep)
    # sample_errors: every replica is the sample, so every percentile is the full-sample estimate
    se = CAT.sample_errors(out, replicas=3, seed=1, keep=keep, strata=None, sums=BO.sums_all_ones)
    z, om, _sd, _ez = CAT.omega_dla(out, keep)
    ii = np.array(want) > 0
    assert np.array_equal(se["z"], z[ii])
    for key in ("omega_median", "omega_68", "omega_95"):
        _close(np.broadcast_to(om[ii], np.shape(se[key])), se[key], Q + 4)
    m, _v = CAT.cddf_moments(out["bin_planes"], out["p_dlas"], keep)
    _close(se["dndx_median"], (m.sum(axis=1) / np.array(want))[ii], Q + 4)
    assert se["dndx_68"].shape == se["omega_95"].shape == (2, ii.sum())


def test_variance_terms_bounded_by_their_magnitudes():
    """The variance columns are differences; their agreement is checked against the sum of magnitudes."""
    out = synthetic_out(seed=8)
    r = BO.rows(out["bin_planes"], out["p_dlas"])
    got, mag = BO.exact_sums(np.ones((1, r.shape[0]), dtype=np.int64), r)
    assert np.all(np.abs(got[0] - r.sum(axis=0)) <= (r.shape[0] + 2) * 2.0 ** -53 * mag[0])


def test_filters_drop_spectra():
    out = synthetic_out()
    Q = out["p_dlas"].size
    r = BO.rows(out["bin_planes"], out["p_dlas"], keep=np.arange(Q) % 2 == 0, p_thresh_spec=0.3)
    dropped = ~((out["p_dlas"] > 0.3) & (np.arange(Q) % 2 == 0))
    assert dropped[5] and np.all(r[dropped] == 0.0) and np.all(np.abs(r[~dropped]).sum(axis=1) > 0)
    cols = CAT.path_columns(out["bin_z_edges"], out["min_z_dlas"], out["max_z_dlas"], keep=np.arange(Q) % 2 == 0)
    assert np.all(cols[1::2] == 0.0) and np.all(cols[::2, -1] > 0)       # no p_dla cut on the path
    hi = CAT.bootstrap_moments(out, 2, 4, strata=None, sums=BO.sums_via_cddf_moments, p_thresh_spec=0.3)
    lo = CAT.bootstrap_moments(out, 2, 4, strata=None, sums=BO.sums_via_cddf_moments)
    assert np.all(hi["means"] <= lo["means"]) and np.any(hi["means"] < lo["means"])
    assert np.array_equal(hi["path"], lo["path"])


def test_gathered_route_equals_the_multiplicity_route():
    """cddf_moments on gathered spectra (the parent's route) against counts x rows summed exactly."""
    out = synthetic_out(Q=150)
    so, mem = CAT.bootstrap_strata(out["min_z_dlas"], out["max_z_dlas"], num_strata=3)
    bm = CAT.bootstrap_moments(out, 4, (7, 11), strata=(so, mem), sums=BO.sums_via_cddf_moments)
    cnt = BO.counts(150, 4, (7, 11), so, mem)
    assert np.all(cnt.sum(axis=1) == mem.size)
    r = np.hstack([BO.rows(out["bin_planes"], out["p_dlas"]),
                   CAT.path_columns(out["bin_z_edges"], out["min_z_dlas"], out["max_z_dlas"])])
    got, mag = BO.exact_sums(cnt, r)
    nb = 20
    assert np.all(np.abs(bm["means"].reshape(4, -1) - got[:, :nb]) <= 152 * 2.0 ** -53 * mag[:, :nb])
    assert np.all(np.abs(bm["moment_means"].reshape(4, -1) - got[:, 2 * nb:3 * nb]) <= 152 * 2.0 ** -53 * mag[:, 2 * nb:3 * nb])
    assert np.array_equal(bm["path"], got[:, 4 * nb:4 * nb + 4])


def test_levels_all_with_one_level_is_first():
    out = synthetic_out()
    out["p_dlas"] = out["model_posteriors"][:, 1].copy()              # D = 1: P_1 is p_dla
    out["p_dlas"][5] = np.nan
    a = CAT.bootstrap_moments(out, 3, 2, strata=None, sums=BO.sums_via_cddf_moments)
    b = CAT.bootstrap_moments(out, 3, 2, strata=None, sums=BO.sums_via_cddf_moments, levels="all")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    with pytest.raises(ValueError):
        CAT.bootstrap_moments(out, 3, 2, strata=None, sums=BO.sums_via_cddf_moments, levels="some")


def test_zero_path_is_nan_and_ignored():
    out = synthetic_out(Q=60, nz=5, z_lo=2.0, z_hi=3.0)
    out["bin_z_edges"] = np.array([0.5, 1.0, 2.2, 2.8, 3.6, 9.0])       # bin 0: no path in the full sample
    out["max_z_dlas"] = np.minimum(out["max_z_dlas"], 3.5)
    out["max_z_dlas"][0] = 4.0                                         # the only sightline reaching bin 4
    se = CAT.sample_errors(out, replicas=40, seed=5, strata=None, sums=BO.sums_via_cddf_moments)
    assert se["z"].size == 4 and se["z"][0] == 1.6
    last = se["dndx_replicas"][:, -1]
    assert np.isnan(last).any() and not np.isnan(last).all()           # replicas that never drew sightline 0
    assert np.isfinite(se["dndx_median"]).all() and np.isfinite(se["omega_95"]).all()
    assert np.all(se["dndx_68"][0] >= se["dndx_median"]) and np.all(se["dndx_median"] >= se["dndx_68"][1])
    assert np.all(se["omega_95"][0] >= se["omega_68"][0]) and np.all(se["omega_68"][1] >= se["omega_95"][1])


def test_find_snr_oracle_against_the_reference_expression():
    """The dtype-explicit restatement agrees with find_snr's own lines (calc_cddf.py:914-924) in float64, where
    numpy's promotion rules leave nothing to choose."""
    rng = np.random.default_rng(2)
    w = np.sort(3600.0 + 6000.0 * rng.random(300))
    flux, nv, zmax, norm = rng.normal(1.0, 1.0, 300), rng.random(300) + 0.01, 5.1, 2.5
    for nm in (norm, None):
        ipix = np.where(w > 1215.67 * (1 + zmax))
        f = np.array(flux)[ipix]
        if nm is not None:
            f[np.where(f / nm < 0.1)] = nm * 0.1
        else:
            f[np.where(f < 0.1)] = 0.1
        assert BO.find_snr(w, flux, nv, zmax, nm) == 1 / np.median(np.sqrt(nv[ipix]) / np.abs(f))
    assert np.isnan(BO.find_snr(w, flux, nv, 9.0)) and BO.find_snr(w.astype(np.float32), flux, nv, 5.1).dtype == np.float32

"""``process_qsos`` mirror (process_qsos.m:1-249) over the native engine.

The MATLAB script reads seven workspace variables and four ``.mat`` files, loops over spectra
and saves ``processed_qsos_<test_set>.mat``.  Here the same steps are one function call:

    params = set_parameters()
    out = process_qsos(model, samples, spectra, prior, params=params, test_ind=...)
    save_processed_qsos(path, out)

``spectra`` is the preloaded_qsos content: either a list of dicts (``wavelengths``, ``flux``,
``noise_variance``, ``pixel_mask``, ``z_qso``) or CSR arrays from ``synthetic.pack_spectra``.
The likelihood of every (spectrum, DLA sample) pair, the null model and the log-mean-exp run on
the GPU (libgpdla.so); priors and posteriors are O(Q) host bookkeeping (process_qsos.m:4-27,
122-132, 222-232).
"""
from __future__ import annotations

import os

import numpy as np

from . import parameters as P
from .engine import Engine, mean_flux_scope_code
from .parameters import Parameters, set_parameters
from .synthetic import pack_spectra


def filter_prior_dlas(prior_z_qsos, prior_dla_ind, prior_z_dlas):
    """process_qsos.m:20-25: drop prior DLAs whose Lya lies below the QSO's Lyman limit."""
    dla_ind = np.array(prior_dla_ind, dtype=bool).copy()
    for i in np.flatnonzero(dla_ind):
        zd = np.atleast_1d(np.asarray(prior_z_dlas[i], dtype=np.float64))
        # MATLAB `if` on a vector is true only if every element is true
        if zd.size and np.all(P.observed_wavelengths(P.LYA_WAVELENGTH, zd)
                              < P.observed_wavelengths(P.LYMAN_LIMIT, prior_z_qsos[i])):
            dla_ind[i] = False
    return dla_ind


def dla_priors(z_qsos, prior_z_qsos, prior_dla_ind, prior_z_qso_increase=P.PRIOR_Z_QSO_INCREASE):
    """process_qsos.m:122-132, vectorised with a sorted prior catalogue."""
    pz = np.asarray(prior_z_qsos, dtype=np.float64)
    order = np.argsort(pz, kind="stable")
    pz_sorted = pz[order]
    dla_cum = np.concatenate([[0], np.cumsum(np.asarray(prior_dla_ind, dtype=bool)[order])])
    cut = np.searchsorted(pz_sorted, np.asarray(z_qsos, dtype=np.float64) + prior_z_qso_increase, side="left")
    num_quasars = cut.astype(np.float64)
    num_dlas = dla_cum[cut].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        log_priors_dla = np.log(num_dlas) - np.log(num_quasars)
        log_priors_no_dla = np.log(num_quasars - num_dlas) - np.log(num_quasars)
    return log_priors_no_dla, log_priors_dla


def model_posteriors(log_posteriors_no_dla, log_posteriors_dla):
    """process_qsos.m:222-232."""
    lp = np.stack([log_posteriors_no_dla, log_posteriors_dla], axis=1)
    mx = np.max(lp, axis=1, keepdims=True)
    post = np.exp(lp - mx)
    post = post / np.sum(post, axis=1, keepdims=True)
    p_no = post[:, 0]
    return post, p_no, 1 - p_no


def multi_dla_priors(z_qsos, prior_z_qsos, prior_dla_ind, max_dlas: int = 1,
                     prior_z_qso_increase=P.PRIOR_Z_QSO_INCREASE, sub_dla_prior_ratio=None):
    """Model priors of the multi-DLA search: with p = M / N of process_qsos.m:123-127, no DLA has prior
    1 - p, exactly d DLAs p^d - p^(d+1) for d < max_dlas and p^max_dlas for d = max_dlas (they sum to 1).
    Returns (log_priors_no_dla [Q], log_priors_dla [Q x max_dlas]); for max_dlas = 1 these are
    ``dla_priors``'s two arrays, bit for bit.

    With ``sub_dla_prior_ratio`` r = Z_sub / Z_DLA (dla_samples.sub_dla_prior_ratio) the sub-DLA model has
    prior r p, the DLA priors are unchanged and no absorber has 1 - p - r p (log -inf where that is <= 0);
    a third array, log_priors_lls [Q], is returned."""
    if not 1 <= max_dlas <= 4:
        raise ValueError("max_dlas must be 1..4")
    lp_no, lp1 = dla_priors(z_qsos, prior_z_qsos, prior_dla_ind, prior_z_qso_increase)
    if max_dlas == 1:
        lp_dla = lp1[:, None]
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.exp(lp1)
            cols = [np.log(p ** d - p ** (d + 1)) for d in range(1, max_dlas)] + [np.log(p ** max_dlas)]
        lp_dla = np.stack(cols, axis=1)
    if sub_dla_prior_ratio is None:
        return lp_no, lp_dla
    lp_no, lp_sub = sub_dla_priors(np.exp(lp1), sub_dla_prior_ratio)
    return lp_no, lp_dla, lp_sub


def sub_dla_priors(p, sub_dla_prior_ratio):
    """(log Pr(no absorber), log Pr(sub-DLA)) for the DLA prior p: Pr(sub-DLA) = r p and Pr(none) =
    1 - p - r p, whose log is -inf where that is <= 0."""
    r = float(sub_dla_prior_ratio)
    if not (np.isfinite(r) and r >= 0):
        raise ValueError("sub_dla_prior_ratio must be finite and >= 0")
    p = np.asarray(p, dtype=np.float64)
    none = 1 - p - r * p
    with np.errstate(divide="ignore", invalid="ignore"):
        lp_no = np.where(none > 0, np.log(np.where(none > 0, none, 1.0)), -np.inf)
        lp_no = np.where(np.isnan(none), np.nan, lp_no)
        lp_sub = np.log(r * p)
    return lp_no, lp_sub


def model_posteriors_multi(log_posteriors_no_dla, log_posteriors_dla):
    """process_qsos.m:222-232 over 1 + D models: ``log_posteriors_dla`` is Q x D.  A level d >= 2 whose
    evidence is NaN (no finite sample below it) enters with posterior 0."""
    lp_dla = np.array(log_posteriors_dla, dtype=np.float64)
    lp_dla[:, 1:] = np.where(np.isnan(lp_dla[:, 1:]), -np.inf, lp_dla[:, 1:])
    lp = np.concatenate([np.asarray(log_posteriors_no_dla, dtype=np.float64)[:, None], lp_dla], axis=1)
    mx = np.max(lp, axis=1, keepdims=True)
    post = np.exp(lp - mx)
    post = post / np.sum(post, axis=1, keepdims=True)
    p_no = post[:, 0]
    return post, p_no, 1 - p_no


def model_posteriors_sub(log_posteriors_no_dla, log_posteriors_dla, log_posteriors_lls):
    """``model_posteriors_multi`` with the sub-DLA model as one more column, placed LAST: Q x (1 + D + 1),
    so column d still reads "exactly d DLAs" (calc_cddf.py:67).  Returns (model_posteriors, p_no_dlas, p_lls,
    p_dlas) with p_dlas = 1 - p_no_dlas - p_lls."""
    lp_dla = np.array(log_posteriors_dla, dtype=np.float64)
    if lp_dla.ndim == 1:
        lp_dla = lp_dla[:, None]
    lp_dla[:, 1:] = np.where(np.isnan(lp_dla[:, 1:]), -np.inf, lp_dla[:, 1:])
    lp = np.concatenate([np.asarray(log_posteriors_no_dla, dtype=np.float64)[:, None], lp_dla,
                         np.asarray(log_posteriors_lls, dtype=np.float64)[:, None]], axis=1)
    mx = np.max(lp, axis=1, keepdims=True)
    post = np.exp(lp - mx)
    post = post / np.sum(post, axis=1, keepdims=True)
    p_no, p_lls = post[:, 0], post[:, -1]
    return post, p_no, p_lls, 1 - p_no - p_lls


def _sub_dla_spec(sub_dla, samples: dict, device: int = 0):
    """``sub_dla`` of process_qsos -> None (off) or dict(nhi, log_nhi, ratio).  True takes the default samples
    (dla_samples.sub_dla_samples: uniform over 19.5..20 on the DLA samples' own Halton points, on the device)
    or the ``lls_log_nhi_samples`` ``samples`` holds, and the prior ratio from ``samples['sub_dla_prior_ratio']``
    or ``samples['fit']``.  A dict gives ``lls_log_nhi_samples`` (or ``lls_nhi_samples``) and / or
    ``sub_dla_prior_ratio`` itself."""
    if sub_dla is None or sub_dla is False:
        return None
    given = {} if sub_dla is True else sub_dla
    if not isinstance(given, dict) or set(given) - {"lls_log_nhi_samples", "lls_nhi_samples", "sub_dla_prior_ratio"}:
        raise ValueError("sub_dla must be None, True or dict(lls_log_nhi_samples=..., sub_dla_prior_ratio=...)")
    S = np.asarray(samples["nhi_samples"]).size
    src = given if ("lls_log_nhi_samples" in given or "lls_nhi_samples" in given) else samples
    if "lls_log_nhi_samples" in src:
        log_nhi = np.ascontiguousarray(src["lls_log_nhi_samples"], dtype=np.float64).ravel()
        nhi = (np.ascontiguousarray(src["lls_nhi_samples"], dtype=np.float64).ravel() if "lls_nhi_samples" in src
               else 10.0 ** log_nhi)
    elif "lls_nhi_samples" in src:
        nhi = np.ascontiguousarray(src["lls_nhi_samples"], dtype=np.float64).ravel()
        with np.errstate(divide="ignore", invalid="ignore"):
            log_nhi = np.log10(nhi)
    else:
        from .dla_samples import sub_dla_samples
        d = sub_dla_samples(S, device=device)
        log_nhi, nhi = d["lls_log_nhi_samples"], d["lls_nhi_samples"]
    if nhi.size != S or log_nhi.size != S:
        raise ValueError("one sub-DLA column density per DLA sample")
    if not np.all(np.isfinite(nhi) & (nhi > 0)):
        raise ValueError("sub-DLA column densities must be finite and > 0")
    if "sub_dla_prior_ratio" in given:
        ratio = float(np.ravel(given["sub_dla_prior_ratio"])[0])
    elif "sub_dla_prior_ratio" in samples:
        ratio = float(np.ravel(samples["sub_dla_prior_ratio"])[0])
    elif "fit" in samples:
        from .dla_samples import sub_dla_prior_ratio
        ratio = sub_dla_prior_ratio(samples["fit"])
    else:
        raise ValueError("sub_dla needs sub_dla_prior_ratio (or samples['fit'] to derive it from)")
    if not (np.isfinite(ratio) and ratio >= 0):
        raise ValueError("sub_dla_prior_ratio must be finite and >= 0")
    return dict(nhi=nhi, log_nhi=log_nhi, ratio=ratio)


FOREST_DEFAULTS = dict(num_forest_lines=31, variance_series=True, mean_flux=True, mean_flux_tau_0=0.0023,
                       mean_flux_beta=3.65,   # Kim et al. 2007's mean flux
                       mean_flux_scope="mu")  # what the mean flux multiplies (engine.MEAN_FLUX_SCOPES)


def _forest_spec(forest):
    """``forest`` of process_qsos -> None (off) or the full settings dict (True = FOREST_DEFAULTS).
    ValueError for an unknown ``mean_flux_scope`` and for one other than "mu" with ``mean_flux=False``."""
    if forest is None or forest is False:
        return None
    given = {} if forest is True else forest
    if not isinstance(given, dict) or set(given) - set(FOREST_DEFAULTS):
        raise ValueError(f"forest must be None, True or a dict of {sorted(FOREST_DEFAULTS)}")
    f = dict(FOREST_DEFAULTS, **given)
    if not 1 <= int(f["num_forest_lines"]) <= 31:
        raise ValueError("num_forest_lines must be 1..31")
    if not (np.isfinite(f["mean_flux_tau_0"]) and f["mean_flux_tau_0"] >= 0 and np.isfinite(f["mean_flux_beta"])):
        raise ValueError("mean_flux_tau_0 must be finite and >= 0, mean_flux_beta finite")
    mean_flux_scope_code(f["mean_flux_scope"], f["mean_flux"])
    return f


def _scope_variables(forest) -> dict:
    """MEAN_FLUX_SCOPE_VARIABLES of a run or a learned model: nothing under the default scope."""
    code = mean_flux_scope_code(forest["mean_flux_scope"], forest["mean_flux"])
    return dict(mean_flux_scope=float(code)) if code else {}


def _select(spectra, test_ind):
    if isinstance(spectra, dict) and "offsets" in spectra:
        packed = spectra
        if test_ind is None:
            return packed
        idx = np.flatnonzero(np.asarray(test_ind)) if np.asarray(test_ind).dtype == bool else np.asarray(test_ind)
        lst = []
        for q in idx:
            a, b = packed["offsets"][q], packed["offsets"][q + 1]
            lst.append(dict(wavelengths=packed["wavelengths"][a:b], flux=packed["flux"][a:b],
                            noise_variance=packed["noise_variance"][a:b],
                            pixel_mask=packed["pixel_mask"][a:b], z_qso=packed["z_qsos"][q]))
        return pack_spectra(lst)
    lst = list(spectra)
    if test_ind is not None:
        ti = np.asarray(test_ind)
        idx = np.flatnonzero(ti) if ti.dtype == bool else ti
        lst = [lst[i] for i in idx]
    return pack_spectra(lst)


def _summary_grid(summaries):
    """``summaries`` of process_qsos -> None (off) or (z_edges, log_nhi_edges), both None for MAP only.  The
    dict may also hold ``levels`` ("first", the default, or "all": ``_summary_levels``), which needs the grid."""
    if summaries is None or summaries is False:
        return None
    if summaries is True:
        return None, None
    if not isinstance(summaries, dict) or set(summaries) - {"z_edges", "log_nhi_edges", "levels"}:
        raise ValueError("summaries must be None, True or dict(z_edges=..., log_nhi_edges=..., levels=...)")
    if summaries.get("levels", "first") not in LEVELS:
        raise ValueError(f"summaries levels must be one of {LEVELS}")
    ez, en = summaries.get("z_edges"), summaries.get("log_nhi_edges")
    if (ez is None) != (en is None):
        raise ValueError("summaries needs both z_edges and log_nhi_edges, or neither")
    if ez is None:
        if summaries.get("levels", "first") == "all":
            raise ValueError("summaries levels='all' needs z_edges and log_nhi_edges")
        return None, None
    return np.ascontiguousarray(ez, dtype=np.float64).ravel(), np.ascontiguousarray(en, dtype=np.float64).ravel()


LEVELS = ("first", "all")    # which levels the binned masses / the population split count


def _summary_levels(summaries) -> bool:
    """True when ``summaries`` asks for the binned masses of every level (``levels="all"``)."""
    return _summary_grid(summaries) is not None and isinstance(summaries, dict) and summaries.get("levels") == "all"


POPULATION_DEFAULTS = dict(p_thresh_sample=1e-4, p_switch=0.25)   # calc_cddf.py:47,50
POPULATION_MAX_LARGE = 8     # include/gpdla.h GPDLA_POPULATION_MAX_LARGE
POPULATION_MAX_BINS = 1024   # GPDLA_SUMMARY_MAX_BINS


def _population_spec(population):
    """``population`` of process_qsos -> None (off) or dict(z_edges, log_nhi_edges, p_thresh_sample, p_switch),
    checked as the library checks them; with ``levels="all"`` (every level of the multi-DLA search, not the
    first alone) the dict also holds ``levels``."""
    if population is None or population is False:
        return None
    keys = {"z_edges", "log_nhi_edges", "levels"} | set(POPULATION_DEFAULTS)
    if not isinstance(population, dict) or set(population) - keys:
        raise ValueError(f"population must be None or a dict of {sorted(keys)}")
    if "z_edges" not in population or "log_nhi_edges" not in population:
        raise ValueError("population needs z_edges and log_nhi_edges")
    pop = dict(POPULATION_DEFAULTS)
    for key in POPULATION_DEFAULTS:
        if key in population:
            pop[key] = float(population[key])
    for key in ("z_edges", "log_nhi_edges"):
        e = np.ascontiguousarray(population[key], dtype=np.float64).ravel()
        if e.size < 2 or not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
            raise ValueError(f"population {key} must be at least two finite, strictly increasing edges")
        pop[key] = e
    if (pop["z_edges"].size - 1) * (pop["log_nhi_edges"].size - 1) > POPULATION_MAX_BINS:
        raise ValueError(f"population grid exceeds {POPULATION_MAX_BINS} bins")
    if not (np.isfinite(pop["p_switch"]) and pop["p_switch"] >= 1.0 / POPULATION_MAX_LARGE):
        raise ValueError(f"p_switch must be finite and >= 1/{POPULATION_MAX_LARGE}")
    if not 0.0 <= pop["p_thresh_sample"] < pop["p_switch"]:
        raise ValueError("p_thresh_sample must lie in [0, p_switch)")
    if population.get("levels", "first") not in LEVELS:
        raise ValueError(f"population levels must be one of {LEVELS}")
    if population.get("levels") == "all":
        pop["levels"] = "all"
    return pop


def _model_log_priors(z_qsos, prior: dict | None, params: Parameters, max_dlas: int, sub=None):
    """The log priors ``_finish`` will write, before the compute call (they depend on z_QSO and the prior
    catalogue alone): (log_priors_no_dla [Q], log_priors_dla [D x Q], log_priors_lls [Q] or None), by the same
    expressions as ``_finish`` / ``_finish_multi`` / ``_finish_sub``."""
    Q, D = np.asarray(z_qsos).size, int(max_dlas)
    if prior is not None:
        dla_ind = filter_prior_dlas(prior["z_qsos"], prior["dla_ind"], prior.get("z_dlas", [None] * len(prior["z_qsos"])))
        if D > 1:
            lp_no, lp_dla = multi_dla_priors(z_qsos, prior["z_qsos"], dla_ind, D, params.prior_z_qso_increase)
        else:
            lp_no, lp_dla = dla_priors(z_qsos, prior["z_qsos"], dla_ind, params.prior_z_qso_increase)
            lp_dla = lp_dla[:, None]
        p = np.exp(dla_priors(z_qsos, prior["z_qsos"], dla_ind, params.prior_z_qso_increase)[1])
    elif D > 1:
        lp_no = np.full(Q, np.log(1 - 0.5))
        lp_dla = np.tile(np.log([0.5 ** d - 0.5 ** (d + 1) for d in range(1, D)] + [0.5 ** D]), (Q, 1))
        p = np.full(Q, 0.5)
    else:
        lp_no, lp_dla, p = np.full(Q, np.log(0.5)), np.full((Q, 1), np.log(0.5)), np.full(Q, 0.5)
    lp_lls = None
    if sub is not None:
        lp_no, lp_lls = sub_dla_priors(p, sub["ratio"])
    return lp_no, np.ascontiguousarray(np.asarray(lp_dla, dtype=np.float64).T), lp_lls


def _interval_spec(intervals):
    """``intervals`` of process_qsos -> None (off) or dict(levels, lr_delta): True takes the defaults
    (engine.DEFAULT_INTERVAL_LEVELS, lr_delta = 2).  The levels are up to 8 numbers strictly inside (0, 1),
    strictly increasing; lr_delta is finite and > 0."""
    if intervals is None or intervals is False:
        return None
    given = {} if intervals is True else intervals
    if not isinstance(given, dict) or set(given) - {"levels", "lr_delta"}:
        raise ValueError("intervals must be None, True or dict(levels=..., lr_delta=...)")
    from .engine import DEFAULT_INTERVAL_LEVELS
    levels = np.asarray(given.get("levels", DEFAULT_INTERVAL_LEVELS), dtype=np.float64).ravel()
    lr_delta = float(given.get("lr_delta", 2.0))
    if not 1 <= levels.size <= 8:
        raise ValueError("intervals levels: 1 to 8 quantile levels")
    if not (np.all(levels > 0.0) and np.all(levels < 1.0)):
        raise ValueError("intervals levels must lie strictly inside (0, 1)")
    if not np.all(np.diff(levels) > 0.0):
        raise ValueError("intervals levels must be strictly increasing")
    if not (np.isfinite(lr_delta) and lr_delta > 0.0):
        raise ValueError("intervals lr_delta must be finite and > 0")
    return dict(levels=levels, lr_delta=lr_delta)


def _compute_kwargs(max_dlas: int, summaries, save_samples: bool, sub=None, forest=None, population=None,
                    intervals=None, cuts=None) -> dict:
    """What a ``compute`` replacement is told beyond the five positional arguments: only what differs
    from the plain single-DLA call, so existing replacements keep working.  ``sub_dla`` is the normalised
    dict(nhi, log_nhi, ratio), ``forest`` the full settings dict, ``population`` the normalised dict of
    ``_population_spec`` with the log priors of ``_model_log_priors`` added, ``cuts`` the dict of
    ``engine.normalise_cuts`` (NaN = off)."""
    kw = {}
    if cuts is not None:
        kw["cuts"] = cuts
    if population is not None:
        kw["population"] = population
    if sub is not None:
        kw["sub_dla"] = sub
    if forest is not None:
        kw["forest"] = forest
    if max_dlas > 1:
        kw["max_dlas"] = max_dlas
    if _summary_grid(summaries) is not None:
        kw["summaries"] = summaries
    if not save_samples:
        kw["save_samples"] = False
    if intervals is not None:
        kw["intervals"] = intervals
    return kw


def _engine_compute(model: dict, samples: dict, packed: dict, params: Parameters, device: int = 0,
                    engine: Engine | None = None, max_dlas: int = 1, summaries=None, save_samples: bool = True,
                    timings: dict | None = None, sub_dla=None, forest=None, population=None, intervals=None,
                    cuts=None, model_spectra=None) -> dict:
    """The hot path on the GPU: per-spectrum null / sample / DLA log likelihoods and z ranges; with
    ``max_dlas`` > 1 every level of the multi-DLA search (Engine.process_multi's arrays); with
    ``summaries`` the posterior summaries as well (Engine.process_summaries), the sample arrays only if
    ``save_samples``.  ``sub_dla`` (the normalised dict of ``_sub_dla_spec``) adds the sub-DLA model's arrays
    (Engine.process_models); ``forest`` (the settings dict) is set on the engine for this call and cleared
    after it.  ``population`` (the dict ``_compute_kwargs`` documents) adds Engine.process_population's arrays;
    ``levels="all"`` in either dict routes the call through Engine.process_levels for that half.  ``intervals``
    (the dict of ``_interval_spec``; with ``summaries`` alone) adds Engine.process_intervals's arrays.  ``cuts``
    (the dict of ``engine.normalise_cuts``) routes the call through Engine.process_cuts: the grid reductions
    under the search cuts, and the cut variables."""
    grid = _summary_grid(summaries)
    halves = (("planes",) if _summary_levels(summaries) else ()) + \
             (("split",) if population is not None and population.get("levels") == "all" else ())
    eng = engine or Engine(model, samples, params, device=device)
    try:
        if forest is not None:
            eng.set_forest(forest)
        if model_spectra is not None:   # (with the summaries alone: process_qsos has checked)
            if "log_nhi_samples" not in samples:
                raise ValueError("model_spectra needs samples['log_nhi_samples']")
            res = eng.process_model_spectra(packed, max_dlas, samples["log_nhi_samples"], level=model_spectra["level"],
                                            log_priors_dla=model_spectra["log_priors_dla"],
                                            z_edges=grid[0] if grid else None, log_nhi_edges=grid[1] if grid else None,
                                            want_samples=save_samples,
                                            intervals=None if intervals is None else dict(levels=intervals["levels"],
                                                                                          lr_delta=intervals["lr_delta"]))
            if max_dlas == 1:   # Engine.process's shapes: no level axis, no multi-DLA variables
                res["log_likelihoods_dla"] = res["log_likelihoods_dla"][0]
                if "sample_log_likelihoods_dla" in res:
                    res["sample_log_likelihoods_dla"] = res["sample_log_likelihoods_dla"][0]
                res.pop("base_sample_inds", None)
                res.pop("max_dlas", None)
            return res
        if cuts is not None:
            if "log_nhi_samples" not in samples:
                raise ValueError("cuts need samples['log_nhi_samples']")
            popd = None
            if population is not None:
                popd = {k: v for k, v in population.items() if k != "levels"}
                popd["log_nhi_samples"] = samples["log_nhi_samples"]
            res = eng.process_cuts(
                packed, max_dlas, cuts={k: (None if np.isnan(v) else v) for k, v in cuts.items()}, population=popd,
                log_nhi_samples=samples["log_nhi_samples"] if grid is not None else None,
                z_edges=grid[0] if grid is not None else None, log_nhi_edges=grid[1] if grid is not None else None,
                want_samples=save_samples, levels=halves)
            if max_dlas == 1:   # Engine.process's shapes: no level axis, no multi-DLA variables
                res["log_likelihoods_dla"] = res["log_likelihoods_dla"][0]
                if "sample_log_likelihoods_dla" in res:
                    res["sample_log_likelihoods_dla"] = res["sample_log_likelihoods_dla"][0]
                res.pop("base_sample_inds", None)
                res.pop("max_dlas", None)
            return res
        if halves:
            if "log_nhi_samples" not in samples:
                raise ValueError("levels='all' needs samples['log_nhi_samples']")
            popd = None
            if population is not None:
                popd = {k: v for k, v in population.items() if k != "levels"}
                popd["log_nhi_samples"] = samples["log_nhi_samples"]
            res = eng.process_levels(
                packed, max_dlas, population=popd, sub_dla=None if sub_dla is None else sub_dla["nhi"],
                log_nhi_samples=samples["log_nhi_samples"] if grid is not None else None,
                z_edges=grid[0] if grid is not None else None, log_nhi_edges=grid[1] if grid is not None else None,
                sub_dla_log_nhi=None if sub_dla is None else sub_dla["log_nhi"], want_samples=save_samples,
                levels=halves)
            if max_dlas == 1:   # Engine.process's shapes: no level axis, no multi-DLA variables
                res["log_likelihoods_dla"] = res["log_likelihoods_dla"][0]
                if "sample_log_likelihoods_dla" in res:
                    res["sample_log_likelihoods_dla"] = res["sample_log_likelihoods_dla"][0]
                res.pop("base_sample_inds", None)
                res.pop("max_dlas", None)
            return res
        if population is not None:
            if "log_nhi_samples" not in samples:
                raise ValueError("population needs samples['log_nhi_samples']")
            res = eng.process_population(
                packed, max_dlas, population=dict(population, log_nhi_samples=samples["log_nhi_samples"]),
                sub_dla=None if sub_dla is None else sub_dla["nhi"],
                log_nhi_samples=samples["log_nhi_samples"] if grid is not None else None,
                z_edges=grid[0] if grid is not None else None, log_nhi_edges=grid[1] if grid is not None else None,
                sub_dla_log_nhi=None if sub_dla is None else sub_dla["log_nhi"], want_samples=save_samples)
            if max_dlas == 1:   # Engine.process's shapes: no level axis, no multi-DLA variables
                res["log_likelihoods_dla"] = res["log_likelihoods_dla"][0]
                if "sample_log_likelihoods_dla" in res:
                    res["sample_log_likelihoods_dla"] = res["sample_log_likelihoods_dla"][0]
                res.pop("base_sample_inds", None)
                res.pop("max_dlas", None)
            return res
        if sub_dla is not None:
            if grid is not None and "log_nhi_samples" not in samples:
                raise ValueError("summaries need samples['log_nhi_samples']")
            res = eng.process_models(packed, max_dlas, sub_dla=sub_dla["nhi"],
                                     log_nhi_samples=samples["log_nhi_samples"] if grid is not None else None,
                                     z_edges=grid[0] if grid is not None else None,
                                     log_nhi_edges=grid[1] if grid is not None else None,
                                     sub_dla_log_nhi=sub_dla["log_nhi"], want_samples=save_samples)
            if max_dlas == 1:   # Engine.process's shapes: no level axis, no multi-DLA variables
                res["log_likelihoods_dla"] = res["log_likelihoods_dla"][0]
                if "sample_log_likelihoods_dla" in res:
                    res["sample_log_likelihoods_dla"] = res["sample_log_likelihoods_dla"][0]
                res.pop("base_sample_inds", None)
                res.pop("max_dlas", None)
            return res
        if grid is not None:
            if "log_nhi_samples" not in samples:
                raise ValueError("summaries need samples['log_nhi_samples']")
            if intervals is not None:
                res = eng.process_intervals(packed, max_dlas, samples["log_nhi_samples"], levels=intervals["levels"],
                                            lr_delta=intervals["lr_delta"], z_edges=grid[0], log_nhi_edges=grid[1],
                                            want_samples=save_samples)
            else:
                res = eng.process_summaries(packed, max_dlas, samples["log_nhi_samples"], z_edges=grid[0],
                                            log_nhi_edges=grid[1], want_samples=save_samples)
            if max_dlas == 1:   # Engine.process's shapes: no level axis, no multi-DLA variables
                res["log_likelihoods_dla"] = res["log_likelihoods_dla"][0]
                if "sample_log_likelihoods_dla" in res:
                    res["sample_log_likelihoods_dla"] = res["sample_log_likelihoods_dla"][0]
                res.pop("base_sample_inds", None)
                res.pop("max_dlas", None)
            return res
        if max_dlas > 1:
            return eng.process_multi(packed, max_dlas, want_samples=save_samples)
        return eng.process(packed, want_samples=save_samples, **(dict(timings=timings) if timings is not None else {}))
    finally:
        if forest is not None and engine is not None:
            eng.set_forest(None)
        if engine is None:
            eng.close()


def _finish_multi(res: dict, z_qsos, prior: dict | None, params: Parameters, metadata: dict | None,
                  max_dlas: int) -> dict:
    """``_finish`` for max_dlas > 1, in MATLAB shapes: ``res`` holds Engine.process_multi's arrays
    (D x Q evidences, D x Q x S sample rows, (D - 1) x Q x S 0-based base indices)."""
    Q, D = np.asarray(z_qsos).size, int(max_dlas)
    lld = np.ascontiguousarray(np.asarray(res["log_likelihoods_dla"], dtype=np.float64).T)       # Q x D
    if lld.shape != (Q, D):
        raise ValueError(f"log_likelihoods_dla must be {(D, Q)} for max_dlas={D}")
    out = dict(
        min_z_dlas=res["min_z_dlas"], max_z_dlas=res["max_z_dlas"],
        log_likelihoods_no_dla=res["log_likelihoods_no_dla"], log_likelihoods_dla=lld,
        num_pixels=res["num_pixels"], num_lines=params.num_lines, max_z_cut=params.max_z_cut,
        prior_z_qso_increase=params.prior_z_qso_increase, max_dlas=D)
    if "sample_log_likelihoods_dla" in res:                                  # Q x S x D
        out["sample_log_likelihoods_dla"] = np.ascontiguousarray(
            np.transpose(np.asarray(res["sample_log_likelihoods_dla"]), (1, 2, 0)))
    if "base_sample_inds" in res:   # 1-based doubles, 0 = none: Q x S for D = 2, Q x S x (D - 1) beyond
        b = np.transpose(np.asarray(res["base_sample_inds"]), (1, 2, 0)).astype(np.float64) + 1.0
        out["base_sample_inds"] = np.ascontiguousarray(b[:, :, 0] if D == 2 else b)
    if prior is not None:
        dla_ind = filter_prior_dlas(prior["z_qsos"], prior["dla_ind"], prior.get("z_dlas", [None] * len(prior["z_qsos"])))
        lp_no, lp_dla = multi_dla_priors(z_qsos, prior["z_qsos"], dla_ind, D, params.prior_z_qso_increase)
    else:
        p = 0.5
        lp_no = np.full(Q, np.log(1 - p))
        lp_dla = np.tile(np.log([p ** d - p ** (d + 1) for d in range(1, D)] + [p ** D]), (Q, 1))
    out["log_priors_no_dla"], out["log_priors_dla"] = lp_no, lp_dla
    out["log_posteriors_no_dla"] = lp_no + out["log_likelihoods_no_dla"]
    out["log_posteriors_dla"] = lp_dla + lld
    post, p_no, p_dla = model_posteriors_multi(out["log_posteriors_no_dla"], out["log_posteriors_dla"])
    out["model_posteriors"], out["p_no_dlas"], out["p_dlas"] = post, p_no, p_dla
    if "numeric_warning" in res:
        out["numeric_warning"] = res["numeric_warning"]
    for key, val in (metadata or {}).items():
        out[key] = val
    return out


def _finish_summaries(out: dict, res: dict, summaries, max_dlas: int) -> dict:
    """Add the summary variables to the saved ones.  ``res`` holds Engine.process_summaries's arrays
    (D x Q MAP indices, D x Q x D MAP pairs, Q x 5 x nz x nn planes).  ``MAP_z_dlas`` / ``MAP_log_nhis``
    (Q x D, the names of Ho et al.'s files) are those of the DLA model with the highest posterior -- level
    d's d pairs, the rest NaN; ``map_sample_inds`` (Q x D) keeps every level's MAP sample, 1-based with
    0 = none like ``base_sample_inds``."""
    grid = _summary_grid(summaries)
    D = int(max_dlas)
    post = np.asarray(out["model_posteriors"], dtype=np.float64)[:, 1:1 + D]
    Q = post.shape[0]
    level = np.argmax(np.where(np.isnan(post), -np.inf, post), axis=1) if Q else np.zeros(0, dtype=np.int64)
    for key in ("MAP_z_dlas", "MAP_log_nhis"):
        v = np.asarray(res[key], dtype=np.float64)
        if v.shape != (D, Q, D):
            raise ValueError(f"{key} must be {(D, Q, D)}")
        out[key] = np.ascontiguousarray(v[level, np.arange(Q), :])
    ind = np.asarray(res["map_sample_inds"])
    if ind.shape != (D, Q):
        raise ValueError(f"map_sample_inds must be {(D, Q)}")
    out["map_sample_inds"] = np.ascontiguousarray(ind.T.astype(np.float64) + 1.0)
    if grid[0] is not None:
        out["bin_planes"] = np.asarray(res["bin_planes"], dtype=np.float64)
        out["bin_z_edges"], out["bin_log_nhi_edges"] = grid
    return out


def _finish_intervals(out: dict, res: dict, ivs: dict, max_dlas: int) -> dict:
    """Add INTERVAL_VARIABLES to the saved ones.  ``res`` holds Engine.process_intervals's arrays (D x Q x D
    [x 2 | x L] per absorber slot, D x Q counts); the saved ones are spectrum-major and 4 slots wide whatever D
    is: Q x D x 4 [x 2 | x L], unused slots NaN, ``lr_counts`` Q x D doubles."""
    D, L = int(max_dlas), ivs["levels"].size
    Q = np.asarray(out["log_likelihoods_no_dla"]).size
    tails = dict(z_dla_quantiles=(L,), log_nhi_quantiles=(L,), z_dla_means=(), z_dla_sds=(), log_nhi_means=(),
                 log_nhi_sds=(), z_dla_lr_ranges=(2,), log_nhi_lr_ranges=(2,))
    for key, tail in tails.items():
        v = np.asarray(res[key], dtype=np.float64)
        if v.shape != (D, Q, D) + tail:
            raise ValueError(f"{key} must be {(D, Q, D) + tail}")
        wide = np.full((Q, D, 4) + tail, np.nan)
        wide[:, :, :D] = np.swapaxes(v, 0, 1)
        out[key] = wide
    cnt = np.asarray(res["lr_counts"])
    if cnt.shape != (D, Q):
        raise ValueError(f"lr_counts must be {(D, Q)}")
    out["lr_counts"] = np.ascontiguousarray(cnt.T.astype(np.float64))
    out["interval_levels"], out["lr_delta"] = ivs["levels"].copy(), float(ivs["lr_delta"])
    return out


def _finish_sub(out: dict, res: dict, z_qsos, prior: dict | None, params: Parameters, sub: dict) -> dict:
    """The sub-DLA model on top of ``_finish``'s variables: Pr(sub-DLA) = r p, Pr(no absorber) = 1 - p - r p
    (the DLA priors stay), ``model_posteriors`` gains a LAST column and ``p_dlas`` = 1 - p_no_dlas - p_lls."""
    Q = np.asarray(out["log_likelihoods_no_dla"]).size
    ll_lls = np.asarray(res["log_likelihoods_lls"], dtype=np.float64).ravel()
    if ll_lls.size != Q:
        raise ValueError(f"log_likelihoods_lls must have {Q} entries")
    if prior is None:
        p = np.full(Q, 0.5)
    else:   # p = M / N as multi_dla_priors forms it
        dla_ind = filter_prior_dlas(prior["z_qsos"], prior["dla_ind"], prior.get("z_dlas", [None] * len(prior["z_qsos"])))
        p = np.exp(dla_priors(z_qsos, prior["z_qsos"], dla_ind, params.prior_z_qso_increase)[1])
    lp_no, lp_sub = sub_dla_priors(p, sub["ratio"])
    out["log_priors_no_dla"], out["log_priors_lls"] = lp_no, lp_sub
    out["log_likelihoods_lls"] = ll_lls
    out["log_posteriors_no_dla"] = lp_no + out["log_likelihoods_no_dla"]
    out["log_posteriors_lls"] = lp_sub + ll_lls
    post, p_no, p_lls, p_dla = model_posteriors_sub(out["log_posteriors_no_dla"], out["log_posteriors_dla"],
                                                    out["log_posteriors_lls"])
    out["model_posteriors"], out["p_no_dlas"], out["p_lls"], out["p_dlas"] = post, p_no, p_lls, p_dla
    if "sample_log_likelihoods_lls" in res:
        out["sample_log_likelihoods_lls"] = np.asarray(res["sample_log_likelihoods_lls"], dtype=np.float64)
    out["lls_log_nhi_samples"] = sub["log_nhi"]
    out["sub_dla_prior_ratio"] = float(sub["ratio"])
    for key in ("MAP_z_lls", "MAP_log_nhi_lls"):
        if key in res:
            out[key] = np.asarray(res[key], dtype=np.float64)
    return out


def _finish_population(out: dict, res: dict, pop: dict) -> dict:
    """Add POPULATION_VARIABLES to the saved ones.  ``res`` holds Engine.process_population's arrays; the
    sample indices and the flat bins (iz nn + in) become 1-based doubles with 0 = none, like
    ``base_sample_inds``."""
    Q = np.asarray(out["log_likelihoods_no_dla"]).size
    nz, nn = pop["z_edges"].size - 1, pop["log_nhi_edges"].size - 1
    plane = np.asarray(res["population_poisson"], dtype=np.float64)
    if plane.shape != (Q, nz, nn):
        raise ValueError(f"population_poisson must be {(Q, nz, nn)}")
    out["population_poisson"] = plane
    for key in ("population_large_inds", "population_large_bins"):
        v = np.asarray(res[key])
        if v.shape != (Q, POPULATION_MAX_LARGE):
            raise ValueError(f"{key} must be {(Q, POPULATION_MAX_LARGE)}")
        out[key] = v.astype(np.float64) + 1.0
    out["population_large_probs"] = np.asarray(res["population_large_probs"], dtype=np.float64)
    out["population_p_dlas"] = np.asarray(res["population_p_dlas"], dtype=np.float64)
    out["population_z_edges"], out["population_log_nhi_edges"] = pop["z_edges"], pop["log_nhi_edges"]
    out["population_p_thresh_sample"], out["population_p_switch"] = pop["p_thresh_sample"], pop["p_switch"]
    return out


def _finish_cuts(out: dict, res: dict, cuts: dict, summaries, pop: dict | None) -> dict:
    """Add CUT_VARIABLES to the saved ones.  ``res`` holds Engine.process_cuts's arrays; a threshold that is off
    is saved as NaN, and a path array only with its grid."""
    Q = np.asarray(out["log_likelihoods_no_dla"]).size
    out["cut_proximity_zone"], out["cut_noise_thresh"] = float(cuts["proximity_zone"]), float(cuts["noise_thresh"])
    out["cut_omega_m"] = float(cuts["omega_m"])
    out["cut_z_uppers"] = np.asarray(res["cut_z_uppers"], dtype=np.float64).reshape(Q)
    out["cut_pixel_counts"] = np.asarray(res["cut_pixel_counts"], dtype=np.float64).reshape(Q)
    grid = _summary_grid(summaries)
    for key, edges in (("cut_path_summary", None if grid is None else grid[0]),
                       ("cut_path_population", None if pop is None else pop["z_edges"])):
        if edges is None:
            continue
        v = np.asarray(res[key], dtype=np.float64)
        if v.shape != (Q, np.size(edges)):
            raise ValueError(f"{key} must be {(Q, np.size(edges))}")
        out[key] = v
    return out


def _finish_levels(out: dict, res: dict, summaries, pop: dict | None, max_dlas: int) -> dict:
    """Add the LEVEL_POPULATION_VARIABLES a ``levels="all"`` run produced.  ``res`` holds Engine.process_levels's
    arrays; the level posteriors become Q x D, the sample indices and the flat bins 1-based doubles with
    0 = none, like ``population_large_inds``."""
    Q, D = np.asarray(out["log_likelihoods_no_dla"]).size, int(max_dlas)
    if _summary_levels(summaries):
        ez, en = _summary_grid(summaries)
        planes = np.asarray(res["bin_planes_levels"], dtype=np.float64)
        if planes.shape != (Q, D, 5, ez.size - 1, en.size - 1):
            raise ValueError(f"bin_planes_levels must be {(Q, D, 5, ez.size - 1, en.size - 1)}")
        out["bin_planes_levels"] = planes
    if pop is not None and pop.get("levels") == "all":
        nz, nn = pop["z_edges"].size - 1, pop["log_nhi_edges"].size - 1
        shapes = dict(population_level_posteriors=(D, Q), population_level_poisson=(Q, D, nz, nn),
                      population_level_large_inds=(Q, D, POPULATION_MAX_LARGE),
                      population_level_large_probs=(Q, D, POPULATION_MAX_LARGE),
                      population_level_large_bins=(Q, D, POPULATION_MAX_LARGE, 4))
        for key, shape in shapes.items():
            v = np.asarray(res[key])
            if v.shape != shape:
                raise ValueError(f"{key} must be {shape}")
            if key in ("population_level_large_inds", "population_level_large_bins"):
                v = v.astype(np.float64) + 1.0
            out[key] = np.ascontiguousarray(v.T if key == "population_level_posteriors" else v, dtype=np.float64)
    return out


def _finish(res: dict, z_qsos, prior: dict | None, params: Parameters, metadata: dict | None,
            max_dlas: int = 1, summaries=None, sub=None, forest=None) -> dict:
    """process_qsos.m:122-132, 150-155, 202-232: priors, posteriors and the saved scalars."""
    if forest is not None:
        out = _finish(res, z_qsos, prior, params, metadata, max_dlas, summaries, sub)
        out.update(num_forest_lines=int(forest["num_forest_lines"]), forest_variance_series=bool(forest["variance_series"]),
                   forest_mean_flux=bool(forest["mean_flux"]), mean_flux_tau_0=float(forest["mean_flux_tau_0"]),
                   mean_flux_beta=float(forest["mean_flux_beta"]), **_scope_variables(forest))
        return out
    if _summary_grid(summaries) is not None:
        return _finish_summaries(_finish(res, z_qsos, prior, params, metadata, max_dlas, None, sub), res, summaries, max_dlas)
    if sub is not None:
        return _finish_sub(_finish(res, z_qsos, prior, params, metadata, max_dlas), res, z_qsos, prior, params, sub)
    if max_dlas > 1:
        return _finish_multi(res, z_qsos, prior, params, metadata, max_dlas)
    Q = np.asarray(z_qsos).size
    out = dict(
        min_z_dlas=res["min_z_dlas"], max_z_dlas=res["max_z_dlas"],
        log_likelihoods_no_dla=res["log_likelihoods_no_dla"],
        log_likelihoods_dla=res["log_likelihoods_dla"], num_pixels=res["num_pixels"],
        num_lines=params.num_lines, max_z_cut=params.max_z_cut,
        prior_z_qso_increase=params.prior_z_qso_increase)
    if "sample_log_likelihoods_dla" in res:
        out["sample_log_likelihoods_dla"] = res["sample_log_likelihoods_dla"]
    if prior is not None:
        dla_ind = filter_prior_dlas(prior["z_qsos"], prior["dla_ind"], prior.get("z_dlas", [None] * len(prior["z_qsos"])))
        lp_no, lp_dla = dla_priors(z_qsos, prior["z_qsos"], dla_ind, params.prior_z_qso_increase)
    else:
        lp_no, lp_dla = np.full(Q, np.log(0.5)), np.full(Q, np.log(0.5))
    out["log_priors_no_dla"], out["log_priors_dla"] = lp_no, lp_dla
    out["log_posteriors_no_dla"] = lp_no + out["log_likelihoods_no_dla"]      # process_qsos.m:154-155
    out["log_posteriors_dla"] = lp_dla + out["log_likelihoods_dla"]           # process_qsos.m:211-212
    post, p_no, p_dla = model_posteriors(out["log_posteriors_no_dla"], out["log_posteriors_dla"])
    out["model_posteriors"], out["p_no_dlas"], out["p_dlas"] = post, p_no, p_dla
    if "numeric_warning" in res:
        out["numeric_warning"] = res["numeric_warning"]
    for key, val in (metadata or {}).items():
        out[key] = val
    return out


def process_qsos(model: dict, samples: dict, spectra, prior: dict | None = None,
                 params: Parameters | None = None, test_ind=None, engine: Engine | None = None,
                 device: int = 0, metadata: dict | None = None, max_dlas: int = 1, compute=None,
                 summaries=None, save_samples: bool = True, sub_dla=None, forest=None, population=None,
                 intervals=None, cuts=None, model_spectra=None) -> dict:
    """Run the DLA search (process_qsos.m:88-232) and return the saved variables.  ``max_dlas`` > 1
    (up to 4) runs the multi-DLA search: ``log_likelihoods_dla`` / ``log_priors_dla`` /
    ``log_posteriors_dla`` become Q x D, ``model_posteriors`` Q x (1 + D), ``sample_log_likelihoods_dla``
    Q x S x D, and ``base_sample_inds`` (1-based, 0 = none; Q x S for D = 2, else Q x S x (D - 1)) and
    ``max_dlas`` are added.  ``compute(model, samples, packed, params, device, max_dlas=D)`` replaces the
    engine (tests) and returns Engine.process / process_multi's arrays.

    ``summaries`` (True, or ``dict(z_edges=..., log_nhi_edges=...)`` for the binned masses too) has the
    engine reduce the posterior summaries on the device (Engine.process_summaries; ``samples`` must hold
    ``log_nhi_samples``) and adds ``MAP_z_dlas`` / ``MAP_log_nhis`` (Q x D: the pairs of the DLA model with
    the highest posterior), ``map_sample_inds`` (Q x D, 1-based, 0 = none) and, with a grid,
    ``bin_planes`` (Q x 5 x nz x nn), ``bin_z_edges`` and ``bin_log_nhi_edges`` (catalog.py consumes
    them).  ``save_samples=False`` runs the engine without the sample buffers: the output then has no
    ``sample_log_likelihoods_dla`` and no ``base_sample_inds``.  A ``compute`` replacement receives
    ``summaries=`` / ``save_samples=False`` as keywords when they are set.

    ``sub_dla`` (True, or ``dict(lls_log_nhi_samples=..., sub_dla_prior_ratio=...)``; see ``_sub_dla_spec``)
    adds the sub-DLA model of Ho, Bird & Garnett 2020: one absorber at the engine's own z_j with column
    density N^sub_j.  The output gains SUB_DLA_VARIABLES, ``model_posteriors`` a LAST column for it,
    ``log_priors_no_dla`` becomes log(1 - p - r p) and ``p_dlas`` = 1 - p_no_dlas - p_lls.  ``forest`` (True, or
    a dict overriding FOREST_DEFAULTS) makes the null model sum the Lyman series in omega^2
    (``variance_series``) and suppress mu by the mean flux (``mean_flux``), for every model; the output
    records FOREST_VARIABLES.  Its ``mean_flux_scope`` says what the mean flux F multiplies: "mu" (the
    default) mu alone, "mu_M" also the rows of M (the lineage's inference), "all" also omega^2 (by F^2) --
    the model ``learn_qso_model(forest=dict(mean_flux=True))`` learns; other than "mu" the output also
    records MEAN_FLUX_SCOPE_VARIABLES (1 or 2).  Both run on the fused fp64 path only; without them every
    variable is as before, bit for bit.  A ``compute`` replacement receives ``sub_dla=`` (dict(nhi, log_nhi, ratio)) and
    ``forest=`` (the full settings) when they are set.

    ``population`` (``dict(z_edges=..., log_nhi_edges=..., p_thresh_sample=1e-4, p_switch=0.25)``) has the
    engine reduce what the reference's confidence intervals need (calc_cddf.py ``_split_distributions_single``;
    Engine.process_population): the priors are then computed before the compute call and handed to it, and the
    output gains POPULATION_VARIABLES (catalog.py's ``split_distributions`` and the functions after it consume
    them).  It combines with every other keyword; without it every variable is as before, bit for bit.  A
    ``compute`` replacement receives ``population=`` (the edges, the thresholds and ``log_priors_no_dla`` [Q],
    ``log_priors_dla`` [D x Q], ``log_priors_lls`` [Q] or None) only when it is set.

    ``levels="all"`` inside ``summaries`` (with a grid) and / or ``population`` counts every absorber of every
    level of the multi-DLA search instead of the level-1 samples alone (Engine.process_levels; DESIGN.md
    section 18): sample j of level d carries d absorbers, its own and its base chain's.  Every variable above
    is still written, bit for bit; the output gains ``bin_planes_levels`` (Q x D x 5 x nz x nn) from
    ``summaries`` and, from ``population``, ``population_level_posteriors`` (Q x D: Pr(exactly d DLAs)),
    ``population_level_poisson`` (Q x D x nz x nn), ``population_level_large_inds`` / ``_probs`` (Q x D x 8) and
    ``population_level_large_bins`` (Q x D x 8 x 4; indices and bins 1-based, 0 = none) --
    LEVEL_POPULATION_VARIABLES, which catalog.py's functions read with ``levels="all"``.  The default
    ``levels="first"`` is the run without the key.  A ``compute`` replacement finds ``levels="all"`` inside the
    ``summaries`` / ``population`` dicts it already gets.

    ``intervals`` (True, or ``dict(levels=..., lr_delta=...)``; see ``_interval_spec``) has the engine reduce
    credible intervals for every absorber of every level (Engine.process_intervals) and
    adds INTERVAL_VARIABLES: ``z_dla_quantiles`` / ``log_nhi_quantiles`` (Q x D x 4 x L: level d's absorber
    slot u, own first and then the base chain's, unused slots NaN), ``z_dla_means`` / ``_sds`` and
    ``log_nhi_means`` / ``_sds`` (Q x D x 4), ``z_dla_lr_ranges`` / ``log_nhi_lr_ranges`` (Q x D x 4 x 2: the
    reference's find_delta_z / find_delta_NHI are hi - lo of level 1, slot 0), ``lr_counts`` (Q x D),
    ``interval_levels`` (L) and ``lr_delta``.  It runs with the summaries -- without ``summaries`` it implies
    ``summaries=True`` (the MAP pairs) -- and composes with ``max_dlas``, a summary grid, ``forest`` and
    ``save_samples=False``.  With ``population``, ``sub_dla`` or ``levels="all"`` it raises ValueError: those
    calls do not carry the interval launches (the sub-DLA model has no intervals yet).  Without the keyword
    every variable is as before, bit for bit.  A ``compute`` replacement receives ``intervals=`` (dict(levels,
    lr_delta)) when it is set.

    ``cuts`` (``dict(proximity_zone=0.1, noise_thresh=0.25)``, either None for off; optionally ``omega_m``) applies
    the reference's ``lowzcut`` and ``filter_noisy_pixels`` (Engine.process_cuts) inside every
    grid reduction of the call -- ``bin_planes``, the POPULATION_VARIABLES and, with ``levels="all"``, the
    LEVEL_POPULATION_VARIABLES -- and adds CUT_VARIABLES: the thresholds (NaN = off), ``cut_z_uppers`` and
    ``cut_pixel_counts`` (Q) and the per-spectrum path columns ``cut_path_summary`` / ``cut_path_population``
    (Q x (nz + 1): each z bin of the grid, then its whole extent), which catalog.py's population functions then use
    in place of the uncut path.  It needs a summary grid or ``population`` (ValueError otherwise, and for both
    thresholds None); with ``intervals`` or ``sub_dla`` it raises ValueError: the cuts do not cover the interval
    outputs or the sub-DLA model.  Every variable that is not a grid reduction is as before, bit for bit, and so
    is everything without the keyword.  A ``compute`` replacement receives ``cuts=`` (dict(proximity_zone,
    noise_thresh, omega_m), NaN = off) and returns the ``cut_*`` arrays of Engine.process_cuts.

    ``model_spectra`` (True, or ``dict(level=...)``) renders the model on the pixels per device batch, on the panel
    the sweeps just used (Engine.process_model_spectra): ``level`` "best" (default: the DLA level with the highest
    model posterior, the one ``MAP_z_dlas`` takes), an integer 0..max_dlas (0: the null model) or Q of them.  The
    output and the file gain MODEL_SPECTRA_VARIABLES.  It implies ``summaries=True`` and composes with ``max_dlas``,
    a summary grid, ``intervals``, ``forest`` and ``save_samples=False``; with ``sub_dla``, ``population``,
    ``cuts``, summaries ``levels="all"`` or a ``compute`` replacement it raises ValueError.  Without the keyword
    every variable and the file are as before, bit for bit."""
    if not 1 <= int(max_dlas) <= 4:
        raise ValueError("max_dlas must be 1..4")
    msp = _model_spectra_spec(model_spectra)
    if msp is not None:
        for name, val in (("sub_dla", sub_dla), ("population", population), ("cuts", cuts)):
            if val is not None and val is not False:
                raise ValueError(f"model_spectra does not combine with {name} in the same call")
        if compute is not None:
            raise ValueError("model_spectra does not combine with a compute replacement")
        if _summary_levels(summaries):
            raise ValueError("model_spectra does not combine with summaries levels='all'")
        if _summary_grid(summaries) is None:
            summaries = True
    from .engine import normalise_cuts
    cts = normalise_cuts(cuts)
    if cts is not None:
        if intervals is not None and intervals is not False:
            raise ValueError("cuts do not combine with intervals: the interval outputs are not cut")
        if sub_dla is not None and sub_dla is not False:
            raise ValueError("cuts do not combine with sub_dla: the sub-DLA model is not cut")
        if _summary_grid(summaries) is None and (population is None or population is False):
            raise ValueError("cuts need a summary grid or population: there is no grid reduction to cut")
    ivs = _interval_spec(intervals)
    if ivs is not None:
        if population is not None and population is not False:
            raise ValueError("intervals do not combine with population: run the population statistics in a call of their own")
        if sub_dla is not None and sub_dla is not False:
            raise ValueError("intervals do not combine with sub_dla: the sub-DLA model has no intervals")
        if _summary_levels(summaries):
            raise ValueError("intervals do not combine with summaries levels='all'")
        if _summary_grid(summaries) is None:
            summaries = True
    pop = _population_spec(population)
    params = params or set_parameters(k=np.asarray(model["M"]).shape[1])
    sub, fst = _sub_dla_spec(sub_dla, samples, device), _forest_spec(forest)
    packed = _select(spectra, test_ind)
    popkw = None
    if pop is not None:
        lp_no, lp_dla, lp_lls = _model_log_priors(packed["z_qsos"], prior, params, max_dlas, sub)
        popkw = dict(pop, log_priors_no_dla=lp_no, log_priors_dla=lp_dla, log_priors_lls=lp_lls)
    if msp is not None:
        lv = msp["level"]
        if not isinstance(lv, str):
            lv = np.asarray(lv)
            if lv.dtype.kind not in "iu" or lv.shape not in ((), (packed["z_qsos"].size,)) or np.any(lv < 0) or np.any(lv > max_dlas):
                raise ValueError(f"model_spectra level must be 'best', an integer 0..{int(max_dlas)} or one per spectrum")
        msp = dict(level=lv, log_priors_dla=_model_log_priors(packed["z_qsos"], prior, params, max_dlas)[1])
    if compute is not None:
        res = compute(model, samples, packed, params, device,
                      **_compute_kwargs(max_dlas, summaries, save_samples, sub, fst, popkw, ivs, cts))
    else:
        res = _engine_compute(model, samples, packed, params, device, engine, max_dlas, summaries, save_samples,
                              sub_dla=sub, forest=fst, population=popkw, intervals=ivs, cuts=cts,
                              model_spectra=msp)
    if not save_samples:
        res = {k: v for k, v in res.items() if k not in ("sample_log_likelihoods_dla", "base_sample_inds",
                                                         "sample_log_likelihoods_lls")}
    out = _finish(res, packed["z_qsos"], prior, params, metadata, max_dlas, summaries, sub, fst)
    if ivs is not None:
        _finish_intervals(out, res, ivs, max_dlas)
    if pop is not None:
        _finish_population(out, res, pop)
    _finish_levels(out, res, summaries, pop, max_dlas)
    if cts is not None:
        _finish_cuts(out, res, cts, summaries, pop)
    if msp is not None:
        for key in MODEL_SPECTRA_VARIABLES:
            out[key] = res[key]
    if test_ind is not None:
        out["test_ind"] = np.asarray(test_ind)
    return out


def _model_spectra_spec(model_spectra):
    """None, or dict(level=...) of process_qsos(model_spectra=...); ValueError for anything else."""
    if model_spectra is None or model_spectra is False:
        return None
    if model_spectra is True:
        return dict(level="best")
    if not isinstance(model_spectra, dict) or set(model_spectra) - {"level"}:
        raise ValueError("model_spectra must be None, True or dict(level=...)")
    level = model_spectra.get("level", "best")
    if isinstance(level, str) and level != "best":
        raise ValueError(f"model_spectra level must be 'best', an integer or one per spectrum, not {level!r}")
    return dict(level=level)


# what a run with the model spectra saves besides (process_qsos(model_spectra=...)); catalog.py reads them.  The
# per-pixel arrays are flat, CSR by model_offsets (Q + 1); the rest is per spectrum
MODEL_SPECTRA_VARIABLES = ("model_offsets", "model_pixel_inds", "model_absorption", "model_mean", "model_continuum",
                           "model_continuum_sd", "model_levels", "model_log_likelihoods", "model_chi2",
                           "model_num_pixels")
# names of process_qsos.m:235-243, in order
PROCESSED_VARIABLES = ("training_release", "training_set_name", "dla_catalog_name", "prior_ind",
                       "release", "test_set_name", "test_ind", "prior_z_qso_increase", "max_z_cut",
                       "num_lines", "min_z_dlas", "max_z_dlas", "log_priors_no_dla", "log_priors_dla",
                       "log_likelihoods_no_dla", "sample_log_likelihoods_dla", "log_likelihoods_dla",
                       "log_posteriors_no_dla", "log_posteriors_dla", "model_posteriors", "p_no_dlas",
                       "p_dlas")
# what a multi-DLA run (max_dlas > 1) saves besides; calc_cddf.py:112-115,225 reads base_sample_inds
MULTI_DLA_VARIABLES = ("base_sample_inds", "max_dlas")
# what a run with summaries saves besides (process_qsos(summaries=...)); catalog.py reads them
SUMMARY_VARIABLES = ("MAP_z_dlas", "MAP_log_nhis", "map_sample_inds", "bin_planes", "bin_z_edges",
                     "bin_log_nhi_edges")
# what a run with the sub-DLA model saves besides (process_qsos(sub_dla=...)), in the lineage's naming
# (Ho, Bird & Garnett's files call the sub-DLA model "lls"); the MAP pair only with summaries
SUB_DLA_VARIABLES = ("log_priors_lls", "log_likelihoods_lls", "log_posteriors_lls", "p_lls",
                     "sample_log_likelihoods_lls", "lls_log_nhi_samples", "sub_dla_prior_ratio", "MAP_z_lls",
                     "MAP_log_nhi_lls")
# what a run with the Lyman-series forest records (process_qsos(forest=...))
FOREST_VARIABLES = ("num_forest_lines", "forest_variance_series", "forest_mean_flux", "mean_flux_tau_0",
                    "mean_flux_beta")
# ... and, only when forest["mean_flux_scope"] is not "mu", what the mean flux multiplied: 1 mu and M,
# 2 mu, M and omega^2 (a double; files of the default scope have no such variable)
MEAN_FLUX_SCOPE_VARIABLES = ("mean_flux_scope",)
# what a run with the population statistics saves besides (process_qsos(population=...)); catalog.py reads them
POPULATION_VARIABLES = ("population_poisson", "population_large_inds", "population_large_probs",
                        "population_large_bins", "population_p_dlas", "population_z_edges",
                        "population_log_nhi_edges", "population_p_thresh_sample", "population_p_switch")
# what ``levels="all"`` in ``summaries`` (the first) / ``population`` (the rest) saves besides: the reductions
# over every absorber of every multi-DLA level; catalog.py reads them with levels="all"
LEVEL_POPULATION_VARIABLES = ("bin_planes_levels", "population_level_posteriors", "population_level_poisson",
                              "population_level_large_inds", "population_level_large_probs",
                              "population_level_large_bins")
# what a run with the posterior intervals saves besides (process_qsos(intervals=...)); catalog.py reads them
INTERVAL_VARIABLES = ("z_dla_quantiles", "log_nhi_quantiles", "interval_levels", "z_dla_means", "z_dla_sds",
                      "log_nhi_means", "log_nhi_sds", "z_dla_lr_ranges", "log_nhi_lr_ranges", "lr_counts", "lr_delta")
# what a run under the search cuts saves besides (process_qsos(cuts=...)): the thresholds (NaN = off), the upper
# ends and pixel counts, and the per-spectrum path columns catalog.py reads in place of the uncut path
CUT_VARIABLES = ("cut_proximity_zone", "cut_noise_thresh", "cut_omega_m", "cut_z_uppers", "cut_pixel_counts",
                 "cut_path_summary", "cut_path_population")


def save_processed_qsos(path: str, out: dict, format: str = "v7.3") -> dict:
    """``save(filename, variables_to_save{:}, '-v7.3')`` (process_qsos.m:235-249).

    MATLAB shapes: Q-vectors are Q x 1 columns, ``sample_log_likelihoods_dla`` is Q x S,
    ``model_posteriors`` Q x 2, strings are char rows, ``test_ind``/``prior_ind`` logical.  The
    default container is v7.3 (HDF5, matv73.py): what the reference writes and what
    calc_cddf.py reads with h5py (Q-vectors as (1, Q), the sample array as (S, Q)); it has no
    per-variable size limit and streams the sample array into the file.  ``format="v5"`` writes
    a scipy MATLAB v5 file instead (each variable must then stay under 2 GB).

    A multi-DLA run (``max_dlas`` = D > 1) also writes MULTI_DLA_VARIABLES, and its arrays have the
    shapes ``process_qsos`` documents: h5py then sees ``sample_log_likelihoods_dla`` as (D, S, Q) --
    ``[0]`` the first DLA, ``[1]`` the second, calc_cddf.py:89-90,107 -- and ``base_sample_inds`` as
    (S, Q) for D = 2.  The 3-D array is written in one piece (not streamed).

    A run with summaries also writes the SUMMARY_VARIABLES it produced; one with ``save_samples=False``
    has no sample array (and no ``base_sample_inds``) to write.  A run with ``sub_dla`` writes the
    SUB_DLA_VARIABLES (``model_posteriors`` is then Q x (1 + D + 1), the sub-DLA column last, so h5py's
    ``model_posteriors[2]`` still reads "exactly two DLAs", calc_cddf.py:67), one with ``forest`` the
    FOREST_VARIABLES (and, with a ``mean_flux_scope`` other than "mu", MEAN_FLUX_SCOPE_VARIABLES), one
    with ``population`` the POPULATION_VARIABLES, one with ``levels="all"`` the LEVEL_POPULATION_VARIABLES
    (h5py sees ``bin_planes_levels`` as (nn, nz, 5, D, Q)), one with ``intervals`` the INTERVAL_VARIABLES, one
    with ``cuts`` the CUT_VARIABLES."""
    mat = {}
    multi = int(np.ravel(out.get("max_dlas", 1))[0]) > 1
    for key in (PROCESSED_VARIABLES + (MULTI_DLA_VARIABLES if multi else ()) + SUMMARY_VARIABLES + SUB_DLA_VARIABLES +
                FOREST_VARIABLES + MEAN_FLUX_SCOPE_VARIABLES + POPULATION_VARIABLES + LEVEL_POPULATION_VARIABLES +
                INTERVAL_VARIABLES + CUT_VARIABLES + MODEL_SPECTRA_VARIABLES):
        if key not in out:
            continue
        v = out[key]
        if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool):
            v = np.float64(v)          # MATLAB numeric literals are double (num_lines = 3)
        elif isinstance(v, (bool, np.bool_)) and key in FOREST_VARIABLES:
            v = np.float64(v)          # the two forest flags: 0 / 1
        mat[key] = v
    if format == "v7.3":
        from .matv73 import savemat73
        return savemat73(path, mat)
    elif format == "v5":
        from scipy.io import savemat
        mat = {k: (v[:, None] if isinstance(v, np.ndarray) and v.ndim == 1 else v) for k, v in mat.items()}
        savemat(path, mat, do_compression=False, oned_as="column")
        return {}
    raise ValueError("format must be 'v7.3' or 'v5'")


# ------------------------------------------------------------------------------ file-level driver
def processed_directory(base_directory: str, release: str) -> str:
    """set_parameters.m:85-86."""
    return f"{base_directory}/{release}/processed"


class _MatMap:
    def __init__(self, d: dict):
        self._d = d

    def __call__(self, key):
        v = self._d[key]
        if isinstance(v, np.ndarray) and v.dtype != object and v.ndim == 2 and 1 in v.shape:
            return v.ravel()
        if isinstance(v, np.ndarray) and v.dtype == object:
            return list(v.ravel(order="F"))
        return v


def evaluate_index(expr, **names) -> np.ndarray:
    """``if (ischar(ind)) ind = eval(ind); end`` (process_qsos.m:7-9,53-55).  A boolean/integer
    array passes through; a callable gets the named structs; a string is parsed as the
    reference's MATLAB index expression (``&``, ``|``, ``~``, ``==``, ``~=``, field access and
    containers.Map lookup, README.md:242-253) by the restricted evaluator in index_expr.py --
    never by Python's ``eval``."""
    if callable(expr):
        return np.asarray(expr(**names))
    if isinstance(expr, str):
        from .index_expr import evaluate_index_string
        return evaluate_index_string(expr, **names)
    return np.asarray(expr)


def _as_list(cells) -> list:
    if isinstance(cells, np.ndarray) and cells.dtype == object:
        return [np.asarray(c).ravel() for c in cells.ravel(order="F")]
    return [np.asarray(c).ravel() for c in cells]


def load_model(path: str) -> dict:
    """process_qsos.m:29-35 (learned_qso_model_<training_set_name>.mat)."""
    from .matv73 import loadmat
    d = loadmat(path, ["rest_wavelengths", "mu", "M", "log_omega", "log_c_0", "log_tau_0", "log_beta"])
    out = {k: np.asarray(d[k], dtype=np.float64).ravel() for k in ("rest_wavelengths", "mu", "log_omega")}
    out["M"] = np.asfortranarray(np.asarray(d["M"], dtype=np.float64))
    for k in ("log_c_0", "log_tau_0", "log_beta"):
        out[k] = float(np.asarray(d[k]).ravel()[0])
    return out


def load_dla_samples(path: str) -> dict:
    """process_qsos.m:37-40 (dla_samples.mat)."""
    from .matv73 import loadmat
    d = loadmat(path, ["offset_samples", "log_nhi_samples", "nhi_samples", "lls_log_nhi_samples", "sub_dla_prior_ratio"])
    out = {k: np.asarray(v, dtype=np.float64).ravel() for k, v in d.items()}
    if "sub_dla_prior_ratio" in out:
        out["sub_dla_prior_ratio"] = float(out["sub_dla_prior_ratio"][0])
    return out


def save_dla_samples(path: str, samples: dict, **extra) -> None:
    """dla_samples.mat (generate_dla_samples.m:59-63): the sample vectors are MATLAB 1 x S rows
    (h5py sees (S, 1); calc_cddf.py:121-123 reads ``[:, 0]``)."""
    from .matv73 import savemat73
    var = {k: np.asarray(samples[k], dtype=np.float64).reshape(1, -1)
           for k in ("offset_samples", "log_nhi_samples", "nhi_samples", "lls_log_nhi_samples") if k in samples}
    if "sub_dla_prior_ratio" in samples:   # the sub-DLA model's two entries travel with the samples
        var["sub_dla_prior_ratio"] = np.float64(samples["sub_dla_prior_ratio"])
    var.update(extra)
    savemat73(path, var)


def save_snrs(path: str, snrs) -> None:
    """The SNR file of ``compute_all_snrs`` (calc_cddf.py:968-970; ``catalog.compute_snrs``): one v7.3 variable
    ``snrs``, a MATLAB 1 x Q row in the SNRs' own class (h5py sees (Q, 1), like the processed file's vectors;
    the reference's own file holds a rank-1 dataset, which MATLAB's container has no form for)."""
    from .matv73 import savemat73
    v = np.asarray(snrs)
    savemat73(path, {"snrs": (v if v.dtype == np.float32 else v.astype(np.float64)).reshape(1, -1)})


def load_preloaded_qsos(path: str, test_ind=None) -> list[dict]:
    """process_qsos.m:45-60 (preloaded_qsos.mat cells, selected by test_ind); z_QSO is attached
    by the caller from the catalogue.  v7.3 files decode only the selected cells."""
    from .matv73 import MatFile, is_matv73, loadmat
    keys = ("all_wavelengths", "all_flux", "all_noise_variance", "all_pixel_mask")
    if is_matv73(path):
        with MatFile(path) as mf:
            n = mf.cell_count("all_wavelengths")
            idx = _indices(test_ind, n)
            cols = {k: [np.asarray(c).ravel() for c in mf.cell_elements(k, idx)] for k in keys}
    else:
        d = loadmat(path, list(keys))
        full = {k: _as_list(d[k]) for k in d}
        idx = _indices(test_ind, len(full["all_wavelengths"]))
        cols = {k: [full[k][i] for i in idx] for k in keys}
    return [dict(wavelengths=w, flux=f, noise_variance=v, pixel_mask=m.astype(bool))
            for w, f, v, m in zip(cols["all_wavelengths"], cols["all_flux"], cols["all_noise_variance"],
                                  cols["all_pixel_mask"])]


def load_preloaded_qsos_packed(path: str, test_ind=None) -> dict:
    """``pack_spectra(load_preloaded_qsos(path, test_ind))`` without z_qsos (the caller attaches
    them from the catalogue): the engine's CSR arrays straight from the file, with the cells of a
    v7.3 file read in bulk (matv73.MatFile.cell_vectors) rather than decoded one by one."""
    from .matv73 import MatFile, is_matv73
    if not is_matv73(path):
        lst = load_preloaded_qsos(path, test_ind)
        if not lst:
            return dict(offsets=np.zeros(1, np.int64), wavelengths=np.zeros(0), flux=np.zeros(0),
                        noise_variance=np.zeros(0), pixel_mask=np.zeros(0, np.uint8))
        out = pack_spectra([dict(s, z_qso=0.0) for s in lst])
        del out["z_qsos"]
        return out
    keys = (("wavelengths", "all_wavelengths", np.float64), ("flux", "all_flux", np.float64),
            ("noise_variance", "all_noise_variance", np.float64), ("pixel_mask", "all_pixel_mask", np.bool_))
    out = {}
    with MatFile(path) as mf:
        idx = _indices(test_ind, mf.cell_count("all_wavelengths"))
        lengths = None
        for key, var, dt in keys:
            out[key], n = mf.cell_vectors(var, idx, dt)
            if lengths is None:
                lengths = n
            elif not np.array_equal(n, lengths):
                q = int(np.flatnonzero(n != lengths)[0])
                raise ValueError(f"preloaded_qsos: spectrum {int(idx[q])} has {int(lengths[q])} wavelengths "
                                 f"but {int(n[q])} entries in {var}")
    out["pixel_mask"] = out["pixel_mask"].view(np.uint8)   # 0 / 1, as pack_spectra of the bool masks
    out["offsets"] = np.zeros(idx.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=out["offsets"][1:])
    return out


def _indices(sel, n: int) -> np.ndarray:
    if sel is None:
        return np.arange(n)
    sel = np.asarray(sel)
    return np.flatnonzero(sel) if sel.dtype == bool else sel.astype(np.int64)


def run_process_qsos(base_directory: str, training_release: str, training_set_name: str,
                     dla_catalog_name: str, prior_ind, release: str, test_set_name: str, test_ind,
                     params: Parameters | None = None, device: int = 0, save: bool = True,
                     rank: int = 0, world: int = 1, compute=None, timings: dict | None = None,
                     chunk_rows: int | None = None, max_dlas: int = 1, summaries=None,
                     save_samples: bool = True, sub_dla=None, forest=None, population=None,
                     model_spectra=None) -> dict:
    """The whole ``process_qsos`` script (process_qsos.m:1-249) on files laid out as the reference
    lays them out (set_parameters.m:79-86):

      <base>/<training_release>/processed/catalog.mat                  (prior catalogue)
      <base>/<training_release>/processed/learned_qso_model_<set>.mat
      <base>/<training_release>/processed/dla_samples.mat
      <base>/<release>/processed/catalog.mat, preloaded_qsos.mat
      -> <base>/<release>/processed/processed_qsos_<test_set_name>.mat  (v7.3)

    ``prior_ind`` / ``test_ind`` are the reference's index expressions (strings such as
    ``'(catalog.filter_flags == 0)'``), callables or boolean arrays.  The catalogue's
    containers.Map variables (los_inds, dla_inds, z_dlas) are read as structs keyed by catalogue
    name (MATLAB's MCOS Map objects are opaque outside MATLAB, SURVEY.md 7 viii).

    Multi-GPU (``world`` > 1; one process per GPU with a torch.distributed process group already
    initialised, gloo suffices): rank r decodes and evaluates only its contiguous shard of the
    test spectra on ``device``.  The Q x S sample array is a chunked HDF5 dataset whose chunks
    are blocks of whole rows (``matv73.auto_chunk_rows`` spectra each, ~4 MB), and the shards are
    whole chunk blocks, LPT-balanced on the expected pixel count of each block (``shard.py``), so
    ranks get equal sweep work and each writes only whole chunks of its own.  Rank 0 gathers the
    per-spectrum scalars (not the sample arrays), computes priors and posteriors, and writes the
    file with the sample array deferred; every rank then pwrites its own chunks (disjoint 4 KiB-
    aligned ranges of the one file), so the 13 GB full-DR12Q array is never gathered.
    ``compute(model, samples, packed, params, device) -> dict`` replaces the engine (tests);
    ``chunk_rows`` overrides the sharded file's rows per chunk (tests).
    ``timings`` (a dict) receives this rank's wall seconds per phase: load (the four input files,
    process_qsos.m:1-63), compute (the engine, :88-212) and write (priors / posteriors and the
    v7.3 file, :222-249).
    Rank 0 returns the saved scalars; other ranks their local results.
    ``max_dlas`` > 1 runs the multi-DLA search (see ``process_qsos``) on one GPU only: the sharded
    writer is 2-D, so ``world`` > 1 raises NotImplementedError.
    ``summaries`` / ``save_samples`` as in ``process_qsos`` (the file then holds the SUMMARY_VARIABLES and,
    with ``save_samples=False``, no sample array), on one GPU only as well.
    ``sub_dla`` / ``forest`` as in ``process_qsos``: ``sub_dla`` on one GPU only (``world`` > 1 raises
    NotImplementedError: its arrays are not gathered); ``forest`` alone passes through to every rank's
    engine.  ``population`` as in ``process_qsos``, on one GPU only (``world`` > 1 raises NotImplementedError:
    its arrays are not gathered); ``levels="all"`` in either dict likewise."""
    if model_spectra is not None and model_spectra is not False:
        raise ValueError("model_spectra is not covered by run_process_qsos (nor by its multi-GPU split): "
                         "call process_qsos and save_processed_qsos")
    import time
    if not 1 <= int(max_dlas) <= 4:
        raise ValueError("max_dlas must be 1..4")
    pop = _population_spec(population)
    if pop is not None and world > 1:
        raise NotImplementedError("population with world > 1: the population arrays are not gathered")
    if max_dlas > 1 and world > 1:
        raise NotImplementedError("max_dlas > 1 with world > 1: the sharded writer takes the 2-D sample array only")
    if (_summary_grid(summaries) is not None or not save_samples) and world > 1:
        raise NotImplementedError("summaries / save_samples=False with world > 1: the summaries are not gathered")
    if sub_dla is not None and sub_dla is not False and world > 1:
        raise NotImplementedError("sub_dla with world > 1: the sub-DLA arrays are not gathered")
    _forest_spec(forest)    # bad settings (an unknown mean_flux_scope, ...) before any file is opened
    from .matv73 import LazyArray, LazyMat, auto_chunk_rows, is_matv73, loadmat, write_chunks
    from .shard import block_lpt_shards, expected_pixels, merge_shards
    compute = compute or _engine_compute
    tm = timings if timings is not None else {}
    t_start = time.perf_counter()
    tdir, rdir = processed_directory(base_directory, training_release), processed_directory(base_directory, release)
    prior_catalog = loadmat(f"{tdir}/catalog.mat")
    pind = evaluate_index(prior_ind, prior_catalog=prior_catalog, dla_catalog_name=dla_catalog_name).astype(bool).ravel()
    pz = np.asarray(prior_catalog["z_qsos"], dtype=np.float64).ravel()[pind]
    pdla = np.asarray(_MatMap(prior_catalog["dla_inds"])(dla_catalog_name)).astype(bool).ravel()[pind]
    z_dlas_all = _MatMap(prior_catalog["z_dlas"])(dla_catalog_name)
    pzd = [z_dlas_all[i] for i in np.flatnonzero(pind)]
    model = load_model(f"{tdir}/learned_qso_model_{training_set_name}.mat")
    samples = load_dla_samples(f"{tdir}/dla_samples.mat")
    params = params or set_parameters(k=np.asarray(model["M"]).shape[1])
    sub, fst = _sub_dla_spec(sub_dla, samples, device), _forest_spec(forest)
    # the release catalogue: only what test_ind names, and z_qsos, is decoded (not its z_dlas cells)
    catalog = LazyMat(f"{rdir}/catalog.mat") if is_matv73(f"{rdir}/catalog.mat") else loadmat(f"{rdir}/catalog.mat")
    side = f"{rdir}/catalog_filter_flags.mat"
    if os.path.exists(side):
        # preload_qsos's filter_flags when catalog.mat could not take them in place (ingest.py:
        # a catalog holding MATLAB objects is never rewritten): the sidecar supersedes the stale copy
        catalog["filter_flags"] = loadmat(side)["filter_flags"]
    tind = evaluate_index(test_ind, catalog=catalog).astype(bool).ravel()
    tidx = np.flatnonzero(tind)
    z_all = np.asarray(catalog["z_qsos"], dtype=np.float64).ravel()[tidx]
    if isinstance(catalog, LazyMat):
        catalog.close()
    S = np.asarray(samples["nhi_samples"]).size
    if not chunk_rows:
        chunk_rows = auto_chunk_rows(S, 8, tidx.size)
        if world > 1:
            # at least ~4 blocks per rank, so a small Q still spreads over every rank (every rank
            # derives the same value from Q and world before the file exists)
            chunk_rows = max(1, min(chunk_rows, -(-tidx.size // (4 * world) // 8) * 8 or 8))
    shards = block_lpt_shards(expected_pixels(z_all), chunk_rows, world)
    mine = shards[rank]
    packed = load_preloaded_qsos_packed(f"{rdir}/preloaded_qsos.mat", tidx[mine])
    packed["z_qsos"] = np.ascontiguousarray(z_all[mine], dtype=np.float64)
    popkw = None
    if pop is not None:
        lp_no, lp_dla, lp_lls = _model_log_priors(z_all[mine], dict(z_qsos=pz, dla_ind=pdla, z_dlas=pzd), params, max_dlas, sub)
        popkw = dict(pop, log_priors_no_dla=lp_no, log_priors_dla=lp_dla, log_priors_lls=lp_lls)
    t_load = time.perf_counter()
    tm["load_s"] = t_load - t_start
    if compute is _engine_compute:  # the compute phase split: engine creation, then the batches
        eng = Engine(model, samples, params, device=device)
        tm["engine_create_s"] = time.perf_counter() - t_load
        try:
            res = _engine_compute(model, samples, packed, params, device, eng, max_dlas, summaries, save_samples,
                                  timings=tm, sub_dla=sub, forest=fst, population=popkw)
        finally:
            eng.close()
    else:
        res = compute(model, samples, packed, params, device,
                      **_compute_kwargs(max_dlas, summaries, save_samples, sub, fst, popkw))
    if not save_samples:
        res = {k: v for k, v in res.items() if k not in ("sample_log_likelihoods_dla", "base_sample_inds",
                                                         "sample_log_likelihoods_lls")}
    t_comp = time.perf_counter()
    tm["compute_s"] = t_comp - t_load
    meta = dict(training_release=training_release, training_set_name=training_set_name,
                dla_catalog_name=dla_catalog_name, prior_ind=pind, release=release,
                test_set_name=test_set_name)
    prior = dict(z_qsos=pz, dla_ind=pdla, z_dlas=pzd)
    path = f"{rdir}/processed_qsos_{test_set_name}.mat"
    if world == 1:
        out = _finish(res, z_all, prior, params, meta, max_dlas, summaries, sub, fst)
        if pop is not None:
            _finish_population(out, res, pop)
        _finish_levels(out, res, summaries, pop, max_dlas)
        out["test_ind"] = tind
        if save:
            save_processed_qsos(path, out)
        tm["write_s"] = time.perf_counter() - t_comp
        return out
    import torch.distributed as dist
    small = {k: v for k, v in res.items() if k != "sample_log_likelihoods_dla"}
    gathered = [None] * world if rank == 0 else None
    dist.gather_object(small, gathered, dst=0)
    region = [None]
    if rank == 0:
        merged = merge_shards(tidx.size, shards, gathered)
        # GPDLA_ENUMERIC on any rank (its likelihoods are NaN): keep every rank's report
        warns = [f"rank {r}: {g['numeric_warning']}" for r, g in enumerate(gathered) if g.get("numeric_warning")]
        if warns:
            merged["numeric_warning"] = "; ".join(warns)
        out = _finish(merged, z_all, prior, params, meta, forest=fst)
        out["test_ind"] = tind
        if save:   # deferred, chunked by the rows the shards were cut on
            out["sample_log_likelihoods_dla"] = LazyArray((tidx.size, S), np.float64, chunk_rows=chunk_rows)
            region[0] = save_processed_qsos(path, out)["sample_log_likelihoods_dla"]
            del out["sample_log_likelihoods_dla"]
    if save:
        dist.broadcast_object_list(region, src=0)
        # this rank's chunks, straight into the file (page cache; no msync, as matv73): one call per
        # run of consecutive blocks
        sll = np.asarray(res["sample_log_likelihoods_dla"])
        breaks = np.flatnonzero(np.diff(mine) != 1) + 1
        for lo, hi in zip(np.r_[0, breaks], np.r_[breaks, mine.size]):
            if hi > lo:
                write_chunks(path, region[0], sll[lo:hi], row0=int(mine[lo]))
        dist.barrier()
    tm["write_s"] = time.perf_counter() - t_comp
    return out if rank == 0 else res



"""Run the reference's own ``_get_omega_confidence_intervals`` (CDDF_analysis/calc_cddf.py:562-636) on the exact
lists and Poisson means this package splits a redshift bin into.  Used by
tests/golden/make_omega_cddf_fixture.py; never runs where the reference is absent.

calc_cddf.py imports h5py at module level but the function needs no file, so a stub module stands in for it;
the catalogue is made with ``object.__new__`` (its constructor opens files) with ``tophat_prior`` off, its
default (:69), and ``_split_distributions`` is replaced by one that hands back the given lists."""
import sys
import types
import warnings

import numpy as np

sys.dont_write_bytecode = True   # never write __pycache__ into the read-only reference tree


def load_reference(ref_cddf: str):
    warnings.filterwarnings("ignore")
    if not hasattr(np, "bool"):
        np.bool = bool  # calc_cddf.py:84 uses the alias numpy 1.24 removed
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    import matplotlib
    matplotlib.use("Agg")
    if ref_cddf not in sys.path:
        sys.path.insert(0, ref_cddf)
    import calc_cddf
    return calc_cddf


def reference_intervals(ref_cddf: str, lists, means, log_nhi_edges):
    """One redshift bin: ``lists`` the nn exact lists, ``means`` the nn Poisson means.  Returns the reference's
    (median, (low68, high68), (low95, high95)) in N_HI units."""
    calc_cddf = load_reference(ref_cddf)
    cat = object.__new__(calc_cddf.DLACatalogue)
    cat.tophat_prior = False

    def split(q_bins, **kw):
        assert kw.get("nhi") is True and len(q_bins) == len(lists) + 1
        # a list of per-spectrum arrays, as calc_cddf.py:773 appends them; one array holds them all (:1026)
        return [[np.asarray(v, dtype=np.float64)] if len(v) else [] for v in lists], np.asarray(means, dtype=np.float64)
    cat._split_distributions = split
    like, l68, l95 = cat._get_omega_confidence_intervals(lnhi_bins=np.asarray(log_nhi_edges, dtype=np.float64), lred=0.0, ured=0.0)
    return float(like), (float(l68[0]), float(l68[1])), (float(l95[0]), float(l95[1]))


def reference_conversion(ref_cddf: str, hubble: float) -> float:
    """calc_cddf.py:532-542."""
    calc_cddf = load_reference(ref_cddf)
    return 1.67262178e-24 / 2.99e10 * (3.2407789e-18 * hubble) / calc_cddf.rho_crit(hubble)

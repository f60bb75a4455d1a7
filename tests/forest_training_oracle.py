"""Numpy restatement of the training objective with the Lyman-series forest in it (DESIGN.md section 16;
Ho, Bird & Garnett 2020, arXiv:2003.11036): oracle.gpdla_oracle.spectrum_loss / objective term for term,
with the optical depth of spectrum_loss.m:23 replaced by the series sum of sub_dla_forest_oracle.forest_tau
at lambda = lya_1pz lambda_1 and the spectrum's own z_QSO, and the mean-flux step of the training
preparation.

  tau      = sum_i t_i,   t_i = tau_0 c_i (1 + z_i)^beta [z_i <= z_QSO]
  d tau / d log tau_0 = tau,   d tau / d log beta = beta sum_i t_i log(1 + z_i)

f is discontinuous in lya_1pz where a pixel crosses a line's edge lambda_i (1 + z_QSO); the gradient is
with respect to the parameters at fixed pixels, so no pixel may sit on an edge to rounding (asserted).
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

import sub_dla_forest_oracle as SO
from oracle import gpdla_oracle as O

LAMBDA_1 = SO.LINE_WAVELENGTHS[0]
EDGE_GUARD = 1e-9          # relative distance a used pixel keeps from every line's edge


def series_terms(lya_1pz, z_qso, tau_0, beta, num_lines=31):
    """(sum_i t_i, sum_i t_i log(1 + z_i)) per pixel; the second as the explicit line sum."""
    lya_1pz = np.asarray(lya_1pz, dtype=np.float64)
    lam = lya_1pz * LAMBDA_1
    edges = SO.LINE_WAVELENGTHS[:num_lines] * (1 + z_qso)
    gap = np.abs(lam[:, None] - edges[None, :]) / edges[None, :]
    assert gap.size == 0 or gap.min() > EDGE_GUARD, "a pixel sits on a line's edge: f is discontinuous there"
    tau = SO.forest_tau(lam, z_qso, tau_0, beta, num_lines)
    tlog = np.zeros(lam.shape)
    for i in range(num_lines):
        zi = (lam - SO.LINE_WAVELENGTHS[i]) / SO.LINE_WAVELENGTHS[i]
        on = zi <= z_qso
        base = np.where(on, 1 + zi, 1.0)
        tlog = tlog + np.where(on, tau_0 * SO.LINE_STRENGTHS[i] * base ** beta * np.log(base), 0.0)
    return tau, tlog


def spectrum_loss_forest(y, lya_1pz, noise_variance, M, omega2, c_0, tau_0, beta, z_qso, num_lines=31):
    n, k = M.shape                                                               # :20
    optical_depth, depth_log = series_terms(lya_1pz, z_qso, tau_0, beta, num_lines)   # :23, summed over the series
    absorption = np.exp(-optical_depth)                                          # :24
    scaling_factor = 1 - absorption + c_0                                        # :27
    absorption_noise = omega2 * scaling_factor ** 2                              # :28
    d = noise_variance + absorption_noise                                        # :30
    d_inv = 1 / d                                                                # :32
    D_inv_y = d_inv * y                                                          # :33
    D_inv_M = d_inv[:, None] * M                                                 # :34
    B = M.T @ D_inv_M                                                            # :41
    B[np.diag_indices(k)] += 1                                                   # :42
    L = cholesky(B, lower=False)                                                 # :43
    C = solve_triangular(L, solve_triangular(L, D_inv_M.T, trans='T', lower=False),
                         lower=False)                                            # :45
    K_inv_y = D_inv_y - D_inv_M @ (C @ y)                                        # :47
    log_det_K = np.sum(np.log(d)) + 2 * np.sum(np.log(np.diag(L)))               # :49
    nlog_p = 0.5 * (y @ K_inv_y + log_det_K + n * O.LOG_2PI)                     # :53
    K_inv_M = D_inv_M - D_inv_M @ (C @ M)                                        # :56
    dM = -(np.outer(K_inv_y, K_inv_y @ M) - K_inv_M)                             # :57
    diag_K_inv = d_inv - np.sum(C * D_inv_M.T, axis=0)                           # :60
    dlog_omega = -(absorption_noise * (K_inv_y ** 2 - diag_K_inv))               # :63
    da = c_0 * omega2 * scaling_factor                                           # :66
    dlog_c_0 = -(K_inv_y * da) @ K_inv_y + diag_K_inv @ da                       # :67
    da = omega2 * scaling_factor * optical_depth * absorption                    # :70
    dlog_tau_0 = -(K_inv_y * da) @ K_inv_y + diag_K_inv @ da                     # :71
    da = omega2 * scaling_factor * absorption * beta * depth_log                 # :74, the line sum for tau log(lya)
    dlog_beta = -(K_inv_y * da) @ K_inv_y + diag_K_inv @ da                      # :75
    return nlog_p, dM, dlog_omega, dlog_c_0, dlog_tau_0, dlog_beta


def objective_forest(x, centered_rest_fluxes, lya_1pzs, rest_noise_variances, z_qsos, num_lines=31):
    num_quasars, num_pixels = centered_rest_fluxes.shape                         # :16
    k = (x.size - 3) // num_pixels - 1                                           # :18
    M = x[:num_pixels * k].reshape(num_pixels, k, order="F")                     # :20-21
    log_omega = x[num_pixels * k:num_pixels * (k + 1)]                           # :23-24
    log_c_0, log_tau_0, log_beta = x[-3], x[-2], x[-1]                           # :26-28
    omega2 = np.exp(2 * log_omega)                                               # :30
    c_0, tau_0, beta = np.exp(log_c_0), np.exp(log_tau_0), np.exp(log_beta)      # :31-33
    f = 0.0
    dM = np.zeros_like(M)
    dlog_omega = np.zeros_like(log_omega)
    dlog_c_0 = dlog_tau_0 = dlog_beta = 0.0
    for i in range(num_quasars):                                                 # :42
        ind = ~np.isnan(centered_rest_fluxes[i])                                 # :43
        tf, tdM, tdo, tc, tt, tb = spectrum_loss_forest(
            centered_rest_fluxes[i, ind], lya_1pzs[i, ind], rest_noise_variances[i, ind],
            M[ind], omega2[ind], c_0, tau_0, beta, float(z_qsos[i]), num_lines)  # :45-50
        f += tf
        dM[ind] += tdM
        dlog_omega[ind] += tdo
        dlog_c_0 += tc
        dlog_tau_0 += tt
        dlog_beta += tb
    dlog_tau_0 += tau_0 * (tau_0 - 0.0023) / 0.0007 ** 2                         # :60-64
    dlog_beta += beta * (beta - 3.65) / 0.21 ** 2                                # :67-71
    g = np.concatenate([dM.ravel(order="F"), dlog_omega, [dlog_c_0, dlog_tau_0, dlog_beta]])
    return f, g                                                                  # :73


def mean_flux(lya_1pzs, z_qsos, tau_0=SO.MEAN_FLUX_TAU_0, beta=SO.MEAN_FLUX_BETA, num_lines=31):
    """F = exp(-sum_i t_i) per entry of the Q x P matrix of 1 + z_Lya (NaN stays NaN)."""
    lya_1pzs = np.asarray(lya_1pzs, dtype=np.float64)
    out = np.full(lya_1pzs.shape, np.nan)
    for q, z in enumerate(z_qsos):
        ok = ~np.isnan(lya_1pzs[q])
        out[q, ok] = np.exp(-SO.forest_tau(lya_1pzs[q, ok] * LAMBDA_1, float(z), tau_0, beta, num_lines))
    return out


def mean_flux_preparation(rest_fluxes, rest_noise_variances, lya_1pzs, z_qsos, tau_0=SO.MEAN_FLUX_TAU_0,
                          beta=SO.MEAN_FLUX_BETA, num_lines=31):
    """The step between learn_qso_model.m:71 and :77 -> (mu, centred fluxes, noise variances): fluxes over F,
    noise variances over F^2, then the mean over the spectra and the centring as before."""
    F = mean_flux(lya_1pzs, z_qsos, tau_0, beta, num_lines)
    fl = rest_fluxes / F
    nv = rest_noise_variances / F ** 2
    mu = np.nanmean(fl, axis=0)                                                  # :77
    return mu, fl - mu, nv                                                       # :78

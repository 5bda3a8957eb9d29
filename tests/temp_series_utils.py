"""The least-squares line of ``cartnet_adp_temp_series`` (csrc/series_ops.hip) restated in fp64 numpy, and the bounds the
tests hold the kernel to.  No device, no cartnet_amd import."""
import numpy as np

EPS23 = 2.0 ** -23


def line_reference(u_cif, u_eq, temps):
    """fp64 closed form.  ``u_cif`` [T,M,6], ``u_eq`` [T,M], ``temps`` [T] (taken through fp32, as the kernel reads them).
    Returns ``(slope [M,7], intercept [M,7], resid [M], drops [M] int)``; column 6 is ``u_eq``'s."""
    t = np.asarray(temps, dtype=np.float32).astype(np.float64)
    u = np.concatenate([np.asarray(u_cif, dtype=np.float64), np.asarray(u_eq, dtype=np.float64)[..., None]], axis=2)
    tbar = t.mean()
    d = t - tbar
    centre = u.mean(axis=0)
    slope = np.einsum("t,tmc->mc", d, u) / (d * d).sum()
    intercept = centre - slope * tbar
    fit = centre[None] + slope[None] * d[:, None, None]
    resid = np.abs(u - fit).max(axis=(0, 2)) if u.shape[1] else np.zeros(0)
    drops = (np.asarray(u_eq)[1:] < np.asarray(u_eq)[:-1]).sum(axis=0)
    return slope, intercept, resid, drops


def line_bounds(u_cif, u_eq, temps, slope, intercept, resid):
    """``(slope, intercept, resid)`` bounds for one crystal's rows: one fp32 rounding of the largest reference value plus a
    floor for the fp64 noise of the sums, ``1e-12 max|u|`` (over the smallest temperature step for the slope)."""
    t = np.asarray(temps, dtype=np.float64)
    umax = max(np.abs(np.asarray(u_cif, dtype=np.float64)).max(), np.abs(np.asarray(u_eq, dtype=np.float64)).max())
    return (EPS23 * np.abs(slope).max() + 1e-12 * umax / np.diff(t).min(),
            EPS23 * np.abs(intercept).max() + 1e-12 * umax,
            EPS23 * resid.max() + 1e-12 * umax)

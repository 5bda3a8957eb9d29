"""The metrics oracle against the reference's train/metrics.py outputs (tests/golden/adp_metrics.npz)."""
import numpy as np
import torch

import golden_utils as gu
from oracle import metrics_ref as om


def _load():
    return {k: torch.from_numpy(v) for k, v in np.load(gu.GOLDEN + "/adp_metrics.npz").items()}


def test_oracle_matches_reference_metrics():
    z = _load()
    for name in ("close", "far"):
        pred, true = z[f"{name}_pred"], z[f"{name}_true"]
        # |v1 - v2| / v1 amplifies the rounding of the fp32 determinants, which differs between LAPACK builds and CPUs:
        # first-order bound of the fp32 evaluation's error, eps32 * (cond(pred) + cond(true)) * v2 / v1 (the reference's
        # own fp32 run stays within 0.56 of it).  The oracle's fp32 result must be that close to the fp64 one, and agree
        # with the reference's fp32 run to 1e-5 beyond it.
        v1, v2 = om.get_volume(pred.double()), om.get_volume(true.double())
        bound = float(np.finfo(np.float32).eps) * (torch.linalg.cond(pred.double()) + torch.linalg.cond(true.double())) * v2 / v1
        ev = om.get_error_volume(pred, true).double()
        assert torch.all((ev - z[f"{name}_volume_error64"]).abs() <= bound)
        ref = z[f"{name}_volume_error"].double()
        assert torch.all((ev - ref).abs() <= 1e-5 * ref.abs() + 1e-7 + bound)
        assert torch.allclose(om.get_similarity_index(pred, true), z[f"{name}_similarity_index"], rtol=1e-4, atol=1e-3)
        assert torch.allclose(om.compute_3d_iou(pred, true), z[f"{name}_iou"], rtol=0, atol=1e-4)
        # fp64 evaluation of the same formulas reproduces the reference's fp64 run
        assert torch.allclose(om.get_error_volume(pred.double(), true.double()), z[f"{name}_volume_error64"],
                              rtol=1e-12, atol=1e-14)
        assert torch.allclose(om.get_similarity_index(pred.double(), true.double()),
                              z[f"{name}_similarity_index64"], rtol=1e-9, atol=1e-10)


def test_metric_identities():
    z = _load()
    t = z["close_true"][:8]
    assert torch.all(om.compute_3d_iou(t, t) == 1.0)
    assert om.get_error_volume(t, t).abs().max() == 0
    assert om.get_similarity_index(t.double(), t.double()).abs().max() < 1e-10
    # a sphere of covariance I/sqrt(3) * s: radius^2 = s/sqrt(3) after normalisation by |.|_F = s
    eye = torch.eye(3).unsqueeze(0)
    m = om.ellipsoid_masks(eye / 3 ** 0.5, 64)
    frac = m.float().mean().item()
    # 64 lattice points span [-1, 1] inclusive: one point per (2/63)^3 of volume
    assert abs(frac - (4 / 3) * np.pi * (3 ** -0.25) ** 3 / 8 * (63 / 64) ** 3) < 2e-3

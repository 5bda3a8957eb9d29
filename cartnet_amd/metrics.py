"""ADP evaluation metrics on the GPU: the step right after the hot path at test time.

Same names and argument meaning as the reference's ``train/metrics.py`` (:30-180) so that
``compute_metrics_and_logging`` (:201-214) and the inference loops (main.py:47-49,101-102) can call them unchanged;
all three metrics of a batch come from one kernel launch (``adp_metrics``).  There is no CPU path.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import lib as _l

SMOOTH = 1e-8          # train/metrics.py:11


def _check_fp32(name: str, t: torch.Tensor, trailing: tuple = (3, 3), shape: str = "[M,3,3]") -> None:
    """``t`` must be a CUDA fp32 tensor of one leading dimension followed by ``trailing``; ``shape`` is how the message
    writes that."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 1 + len(trailing) and tuple(t.shape[1:]) == trailing):
        raise ValueError(f"{name} must be a CUDA fp32 tensor {shape}")


def _check_pair(pred: torch.Tensor, true: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, int]:
    _check_fp32("pred", pred)
    _check_fp32("true", true)
    if pred.shape[0] != true.shape[0]:
        raise ValueError("pred and true must hold the same number of atoms")
    return pred.detach().contiguous(), true.detach().contiguous(), int(pred.shape[0])


def adp_metrics(pred: torch.Tensor, true: torch.Tensor, volume: bool = True, similarity: bool = True,
                iou: bool = True, num_points: int = 64
                ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(volume_error [M], similarity_index [M], iou [M]) of the requested metrics, ``None`` for the others."""
    pred, true, M = _check_pair(pred, true)
    lib = _l.load()
    dev = pred.device
    outs = [torch.empty(M, dtype=torch.float32, device=dev) if want else None for want in (volume, similarity, iou)]
    if M == 0 or not any((volume, similarity, iou)):
        return tuple(outs)
    grid = torch.linspace(-1, 1, num_points, device=dev, dtype=torch.float32) if iou else None   # metrics.py:128
    _l.check(lib.cartnet_adp_metrics(pred.data_ptr(), true.data_ptr(), M, grid.data_ptr() if iou else None,
                                     int(num_points), *[o.data_ptr() if o is not None else None for o in outs],
                                     _l.stream_ptr()), "cartnet_adp_metrics")
    return tuple(outs)


def get_error_volume(pred: torch.Tensor, true: torch.Tensor) -> torch.Tensor:
    """train/metrics.py:42-58."""
    return adp_metrics(pred, true, True, False, False)[0]


def get_similarity_index(pred: torch.Tensor, true: torch.Tensor) -> torch.Tensor:
    """train/metrics.py:76-94."""
    return adp_metrics(pred, true, False, True, False)[1]


def compute_3D_IoU(pred: torch.Tensor, true: torch.Tensor, num_points: int = 64) -> torch.Tensor:
    """train/metrics.py:148-180 (with get_ellipsoids :114-146 and iou_pytorch3D :96-112 fused)."""
    return adp_metrics(pred, true, False, False, True, num_points)[2]


# ---------------------------------------------------------------------------------------------------------------------
# Evaluation at any batch size with the results of batch size 1 (csrc/eval_ops.hip): the reference's ADP test loader has
# batch size 1 (loader/loader.py:121), so its numbers are per-crystal means, its rotations per crystal.

class AdpEval(NamedTuple):
    """What ``adp_eval`` returns.  ``true``: the truth the metrics were taken against ([M,3,3]; the pseudo-truth with
    ``rot``); ``abs_err`` [M,3,3]; the three per-atom metrics [M] (``None`` if not requested); ``crystal_sums`` [B,4] fp64:
    per crystal the sums of abs_err (over 9 * rows elements), volume error, similarity index and IoU; ``rows`` [B] int64."""
    true: torch.Tensor
    abs_err: torch.Tensor
    volume_error: Optional[torch.Tensor]
    similarity_index: Optional[torch.Tensor]
    iou: Optional[torch.Tensor]
    crystal_sums: torch.Tensor
    rows: torch.Tensor


def target_row_ptr(batch) -> torch.Tensor:
    """[B+1] int64 on the batch's device: crystal g owns rows ``[ptr[g], ptr[g+1])`` of the model's per-atom output (its
    non-hydrogen atoms).  A shard-collated batch carries these offsets already (``Batch._meta``); otherwise they are counted
    with device ops on ``batch`` / ``non_H_mask`` / ``ptr``: no host synchronisation either way."""
    B = int(batch.num_graphs)
    meta = getattr(batch, "_meta", None)
    if meta is not None and meta.numel() == 4 * B + 3:              # [sel | atom offsets | edge offsets | target offsets]
        return meta[3 * B + 2:4 * B + 3].to(batch.x.device)
    mask = getattr(batch, "non_H_mask", None)
    if mask is None:
        return batch.ptr.to(torch.int64)
    counts = torch.zeros(B, dtype=torch.int64, device=mask.device).index_add_(0, batch.batch, mask.to(torch.int64))
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=mask.device), torch.cumsum(counts, 0)])


def edge_row_ptr(batch) -> torch.Tensor:
    """[B+1] int64: crystal g owns edges ``[ptr[g], ptr[g+1])``.  The edges of a batch are sorted by target atom, so the
    first edge of a crystal is the first whose target is not below the crystal's first atom."""
    return torch.searchsorted(batch.edge_index[1].contiguous(), batch.ptr.to(torch.int64).contiguous())


def _check_row_ptr(row_ptr: torch.Tensor, dev) -> Tuple[torch.Tensor, int]:
    if not (row_ptr.dtype == torch.int64 and row_ptr.dim() == 1 and row_ptr.numel() >= 2 and row_ptr.device == dev):
        raise ValueError("row_ptr must be an int64 tensor [B+1], B >= 1, on the data's device")
    return row_ptr.contiguous(), int(row_ptr.numel()) - 1


def _check_rot(rot: torch.Tensor, B: int, dev) -> torch.Tensor:
    if not (rot.dtype == torch.float32 and tuple(rot.shape) == (B, 3, 3) and rot.device == dev):
        raise ValueError("rot must be an fp32 tensor [B,3,3] on the data's device")
    return rot.contiguous()


def rotate_rows(v: torch.Tensor, row_ptr: torch.Tensor, rot: torch.Tensor, out: Optional[torch.Tensor] = None
                ) -> torch.Tensor:
    """``v[r] @ rot[g(r)]`` for the rows of ``v`` [n,3], ``g(r)`` the segment of row ``r`` in ``row_ptr``; one launch, the
    arithmetic of ``DeviceShard.collate(sel, rot)``.  ``out`` may be ``v`` itself (rotation in place)."""
    if not (v.is_cuda and v.dtype == torch.float32 and v.dim() == 2 and v.shape[1] == 3 and v.is_contiguous()):
        raise ValueError("v must be a contiguous CUDA fp32 tensor [n,3]")
    row_ptr, B = _check_row_ptr(row_ptr, v.device)
    rot = _check_rot(rot, B, v.device)
    if out is None:
        out = torch.empty_like(v)
    elif not (out.shape == v.shape and out.dtype == v.dtype and out.device == v.device and out.is_contiguous()):
        raise ValueError("out must have v's shape, dtype and device")
    _l.check(_l.load().cartnet_rotate_rows(v.data_ptr(), row_ptr.data_ptr(), B, int(v.shape[0]), rot.data_ptr(),
                                           out.data_ptr(), _l.stream_ptr()), "cartnet_rotate_rows")
    return out


def adp_eval(pred: torch.Tensor, true: torch.Tensor, row_ptr: torch.Tensor, rot: Optional[torch.Tensor] = None,
             volume: bool = True, similarity: bool = True, iou: bool = True, num_points: int = 64) -> AdpEval:
    """Everything the three evaluation paths take from a batch, with crystal boundaries kept: per atom the absolute error
    and the requested metrics (bit-identical to ``adp_metrics``), per crystal their fp64 sums.  With ``rot`` [B,3,3],
    ``true`` is the first prediction of a Monte-Carlo step and the metrics are taken against ``R_g^T true R_g``."""
    pred, true, M = _check_pair(pred, true)
    dev = pred.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    if rot is not None:
        rot = _check_rot(rot, B, dev)
    outs = [torch.empty(M, dtype=torch.float32, device=dev) if want else None for want in (volume, similarity, iou)]
    true_out = torch.empty_like(true) if rot is not None else None
    abs_err = torch.empty_like(pred)
    sums = torch.empty((B, 4), dtype=torch.float64, device=dev)
    grid = torch.linspace(-1, 1, num_points, device=dev, dtype=torch.float32) if iou else None   # metrics.py:128
    _l.check(_l.load().cartnet_adp_eval(pred.data_ptr(), true.data_ptr(), row_ptr.data_ptr(), B, M, _l.ptr(rot),
                                        _l.ptr(grid), int(num_points), _l.ptr(true_out), abs_err.data_ptr(),
                                        *[_l.ptr(o) for o in outs], sums.data_ptr(), _l.stream_ptr()),
             "cartnet_adp_eval")
    return AdpEval(true_out if rot is not None else true, abs_err, outs[0], outs[1], outs[2], sums,
                   row_ptr[1:] - row_ptr[:-1])


# ---------------------------------------------------------------------------------------------------------------------
# Export in CIF convention (csrc/export_ops.hip): the inverse of the transform that brought the dataset's targets into
# the Cartesian frame (the reference's dataset/extract_csd_data.py:115-123).

ADP_EXPORT_TILE = 1024      # rows per workgroup tile of the export kernel (csrc/shard_tiles.h: SO_TILE)


class AdpExport(NamedTuple):
    """What ``adp_export`` returns, all on the device.  ``u_cif`` [M,6] fp32: U11 U22 U33 U23 U13 U12 on the unit
    reciprocal axes; ``u_eq`` [M]; ``principal`` [M,3] ascending; ``axes`` [M,3,3], rows = unit principal axes, largest
    component positive (``None`` if not requested); ``crystal_stats`` [B,3] fp64: per crystal the sum of ``u_eq``, the
    smallest principal value (+inf without rows) and the number of rows whose smallest principal value is <= 0 (``None``
    if not requested); ``status`` [B] int32: bit 0 set for a singular cell, whose rows are NaN."""
    u_cif: torch.Tensor
    u_eq: torch.Tensor
    principal: torch.Tensor
    axes: Optional[torch.Tensor]
    crystal_stats: Optional[torch.Tensor]
    status: torch.Tensor


def check_export_status(status, names=None) -> None:
    """Raises ``ValueError`` naming the first crystal whose ``AdpExport.status`` is set.  ``status``: a host tensor or
    sequence (bring it over with the results: one transfer); ``names``: the crystals' names, if they have any."""
    for g, s in enumerate(status.tolist() if hasattr(status, "tolist") else status):
        if int(s) & 1:
            who = f"crystal {g}" + (f" ({names[g]})" if names is not None else "")
            raise ValueError(f"{who}: singular cell (its lattice vectors span no volume): no reciprocal axes to export "
                             "the ADPs on")


def adp_export(pred: torch.Tensor, row_ptr: torch.Tensor, cell: torch.Tensor, axes: bool = True, stats: bool = True,
               check: bool = True) -> AdpExport:
    """The predictions ``pred`` [M,3,3] (Cartesian frame of the dataset) in CIF convention, with their equivalent isotropic
    value and principal values / axes: one call of ``cartnet_adp_export``.  ``row_ptr`` [B+1]: crystal g owns rows
    ``[row_ptr[g], row_ptr[g+1])``; ``cell`` [B,3,3] fp32, rows = lattice vectors.  With ``check`` the status is read back
    (one small device-to-host copy) and a singular cell raises ``ValueError`` naming the crystal; with ``check=False`` the
    caller passes ``AdpExport.status`` to ``check_export_status`` once it has brought the results to the host."""
    _check_fp32("pred", pred)
    pred, M, dev = pred.detach().contiguous(), int(pred.shape[0]), pred.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    if not (cell.dtype == torch.float32 and tuple(cell.shape) == (B, 3, 3) and cell.device == dev):
        raise ValueError("cell must be an fp32 tensor [B,3,3] on the data's device")
    cell = cell.detach().contiguous()
    u_cif = torch.empty((M, 6), dtype=torch.float32, device=dev)
    u_eq = torch.empty(M, dtype=torch.float32, device=dev)
    principal = torch.empty((M, 3), dtype=torch.float32, device=dev)
    ax = torch.empty((M, 3, 3), dtype=torch.float32, device=dev) if axes else None
    if M == 0:                                   # the entry point launches nothing: no rows, nothing to flag
        st = torch.tensor([0.0, float("inf"), 0.0], dtype=torch.float64, device=dev).repeat(B, 1) if stats else None
        return AdpExport(u_cif, u_eq, principal, ax, st, torch.zeros(B, dtype=torch.int32, device=dev))
    st = torch.empty((B, 3), dtype=torch.float64, device=dev) if stats else None
    status = torch.empty(B, dtype=torch.int32, device=dev)
    _l.check(_l.load().cartnet_adp_export(pred.data_ptr(), row_ptr.data_ptr(), cell.data_ptr(), B, M, u_cif.data_ptr(),
                                          u_eq.data_ptr(), principal.data_ptr(), _l.ptr(ax), _l.ptr(st),
                                          status.data_ptr(), _l.stream_ptr()), "cartnet_adp_export")
    if check:
        check_export_status(status.cpu())
    return AdpExport(u_cif, u_eq, principal, ax, st, status)


# ---------------------------------------------------------------------------------------------------------------------
# Mean over rotated frames (csrc/frame_ops.hip): the predictions of K rotated copies of a batch, each brought back to the
# stored frame (the inverse of the Monte-Carlo pseudo-truth, main.py:95-97), and how far the members scatter about it.

class FrameMean(NamedTuple):
    """What ``frame_mean`` returns, all on the device.  ``mean`` [M,3,3] fp32: per row the mean over the K frames of
    ``R P_k R^T``; ``spread`` [M]: the largest deviation of a member from that mean over the nine components;
    ``crystal_spread`` [B,2] fp64: per crystal the sum of ``spread`` over its rows and its maximum, (0, 0) without rows
    (``None`` if not requested)."""
    mean: torch.Tensor
    spread: torch.Tensor
    crystal_spread: Optional[torch.Tensor]


def frame_mean(pred: torch.Tensor, rot: torch.Tensor, row_ptr: torch.Tensor, stats: bool = True) -> FrameMean:
    """The mean of a batch's predictions over K frames: one call of ``cartnet_adp_frame_mean``.  ``pred`` [K*M,3,3]
    replica-major (rows ``k*M ... (k+1)*M-1``: the batch's M rows as predicted from ``cart_dir @ rot[k, g]``); ``rot``
    [K,B,3,3] fp32; ``row_ptr`` [B+1] over ONE replica's rows.  Member k comes back as ``R P_k R^T`` (fp64 arithmetic, one
    rounding to fp32); K = 1 with the identity returns ``pred``'s values and a zero spread."""
    _check_fp32("pred", pred, shape="[K*M,3,3]")
    dev = pred.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    if not (rot.dtype == torch.float32 and rot.dim() == 4 and rot.shape[0] >= 1 and tuple(rot.shape[1:]) == (B, 3, 3)
            and rot.device == dev):
        raise ValueError("rot must be an fp32 tensor [K,B,3,3], K >= 1, on the data's device")
    K, rot = int(rot.shape[0]), rot.contiguous()
    if int(pred.shape[0]) % K:
        raise ValueError(f"pred holds {int(pred.shape[0])} rows: no multiple of the {K} frames of rot")
    pred, M = pred.detach().contiguous(), int(pred.shape[0]) // K
    mean = torch.empty((M, 3, 3), dtype=torch.float32, device=dev)
    spread = torch.empty(M, dtype=torch.float32, device=dev)
    if M == 0:                                   # the entry point launches nothing
        return FrameMean(mean, spread, torch.zeros((B, 2), dtype=torch.float64, device=dev) if stats else None)
    cs = torch.empty((B, 2), dtype=torch.float64, device=dev) if stats else None
    _l.check(_l.load().cartnet_adp_frame_mean(pred.data_ptr(), rot.data_ptr(), K, row_ptr.data_ptr(), B, M,
                                              mean.data_ptr(), spread.data_ptr(), _l.ptr(cs), _l.stream_ptr()),
             "cartnet_adp_frame_mean")
    return FrameMean(mean, spread, cs)


def stored_frame(pred: torch.Tensor, rotation: torch.Tensor, row_ptr: torch.Tensor, slices: int = 1) -> torch.Tensor:
    """Predictions made in ONE other frame per crystal, back in the stored frame: one call of
    ``cartnet_adp_stored_frame``.  ``pred`` [T*M,3,3] temperature-major, T = ``slices`` (1: one prediction of the batch's
    M rows), as the model gives it for ``cart_dir @ R`` (``DeviceShard.frame_view``: the reduced cell of the iComformer
    recipe); ``rotation`` [B,3,3] fp32, shared by the T slices; ``row_ptr`` [B+1] over ONE slice's rows.  Row i of crystal g comes
    back as ``R_g P R_g^T`` (fp64 arithmetic, one rounding to fp32): bit for bit ``frame_mean(slice, rotation[None]).mean``;
    with the identity it has ``pred``'s values."""
    _check_fp32("pred", pred, shape="[T*M,3,3]")
    dev = pred.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    rotation = _check_rot(rotation, B, dev)
    T = int(slices)
    if T < 1 or int(pred.shape[0]) % T:
        raise ValueError(f"pred holds {int(pred.shape[0])} rows: no multiple of the {T} slices")
    pred, M = pred.detach().contiguous(), int(pred.shape[0]) // T
    out = torch.empty((T * M, 3, 3), dtype=torch.float32, device=dev)
    if M == 0:                                   # the entry point launches nothing
        return out
    _l.check(_l.load().cartnet_adp_stored_frame(pred.data_ptr(), rotation.data_ptr(), row_ptr.data_ptr(), B, M, T,
                                                out.data_ptr(), _l.stream_ptr()), "cartnet_adp_stored_frame")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Rigid-bond test (csrc/bond_ops.hip): how well the displacement amplitudes of bonded atoms agree along their bond --
# what a crystallographer checks first on a set of ADPs, and it needs no truth.  The bond rule and the radii: bonds.py.

class BondTest(NamedTuple):
    """What ``bond_test`` returns, all on the device, per row (= non-hydrogen atom) over its bonds: ``bonds`` [M] int32;
    ``delta_sum`` [M] fp32, the sum of ``|D|`` with ``D = d^T U_i d - d^T U_j d``; ``delta_max`` [M] fp32, the largest
    ``|D|`` (0 without bonds); ``worst`` [M] int64, the batch's atom index of the partner with the largest ``|D|`` (-1
    without bonds); ``over`` [M] int32, the bonds with ``|D| > threshold``; ``ueq_ratio`` [M] fp32, ``tr(U_i)`` over the
    mean of ``tr(U_j)`` of the partners (NaN without bonds); ``crystal_stats`` [B,4] fp64: per crystal the sum of
    ``bonds``, the sum of ``delta_sum``, the maximum of ``delta_max`` and the sum of ``over``.  Every bond is seen from both
    of its ends, so the counts and sums are DIRECTED: a crystal with n bonds has ``crystal_stats[g, 0] == 2 n``."""
    bonds: torch.Tensor
    delta_sum: torch.Tensor
    delta_max: torch.Tensor
    worst: torch.Tensor
    over: torch.Tensor
    ueq_ratio: torch.Tensor
    crystal_stats: torch.Tensor


_radii_cache: dict = {}


def covalent_radii(device) -> torch.Tensor:
    """``bonds.COVALENT_RADII`` as an fp32 tensor on ``device``: uploaded once per device."""
    from .bonds import COVALENT_RADII
    key = torch.device(device)
    if key.type == "cuda" and key.index is None:
        key = torch.device("cuda", torch.cuda.current_device())
    if key not in _radii_cache:
        _radii_cache[key] = torch.tensor(COVALENT_RADII, dtype=torch.float32, device=key)
    return _radii_cache[key]


def _batch_field(batch, *names):
    for name in names:
        t = batch.get(name) if isinstance(batch, dict) else getattr(batch, name, None)
        if t is not None:
            return t
    return None


class BatchGraph(NamedTuple):
    """Everything the bond-graph analyses (``bond_test``, ``riding_h``, ``molecules``, ``molecule_test``, ``tls_fit``,
    ``aniso_h``, ``bond_index``, ``bond_table``, ``angle_index``, ``angle_table``) take from a batch, checked once by ``batch_graph`` and good for every prediction of that batch: ``z`` [N]
    int64; ``edge_index`` [2,E] sorted by target; ``cart_dist`` [E]; ``cart_dir`` [E,3] (``None`` if not asked for);
    ``mask`` = ``non_H_mask`` [N] (``None``: every atom has a row); ``M``, the rows; the two lookups of the kernels,
    ``atom_row`` [N] int64 (an atom's row, -1 outside the mask) and ``seg_ptr`` [N+1] int64 (atom i owns the edges
    ``[seg_ptr[i], seg_ptr[i+1])``); ``atom_ptr`` [B+1] int64 with ``B``, the crystals' atom offsets (both ``None`` for a
    batch without ``ptr``); ``radii``, ``covalent_radii`` on the batch's device."""
    z: torch.Tensor
    N: int
    edge_index: torch.Tensor
    E: int
    cart_dist: torch.Tensor
    cart_dir: Optional[torch.Tensor]
    mask: Optional[torch.Tensor]
    M: int
    atom_row: torch.Tensor
    seg_ptr: torch.Tensor
    atom_ptr: Optional[torch.Tensor]
    B: Optional[int]
    radii: torch.Tensor


def _atom_lookups(mask, ei: torch.Tensor, N: int, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(atom_row [N], seg_ptr [N+1])`` int64: an atom's row (-1 outside the mask; without a mask every atom has one) and
    its edge segment, with static-shape device ops."""
    if mask is None:
        atom_row = torch.arange(N, dtype=torch.int64, device=dev)
    else:
        mask = mask.to(torch.bool)
        atom_row = torch.where(mask, torch.cumsum(mask, 0, dtype=torch.int64) - 1, -1)
    # the edges are sorted by target: atom i owns the edges between the first target >= i and the first target >= i + 1
    seg_ptr = torch.searchsorted(ei[1].contiguous(), torch.arange(N + 1, dtype=torch.int64, device=dev))
    return atom_row, seg_ptr


def batch_graph(batch, rows: Optional[int] = None, who: str = "batch_graph", what: str = "rows", need_dir: bool = True,
                need_ptr: bool = True, dev=None) -> BatchGraph:
    """The ``BatchGraph`` of ``batch``: a batch of either loader, or a dict of its arrays -- ``x`` (or ``z``) [N] int64
    atomic numbers, ``edge_index`` [2,E] int64 sorted by target (every loader's order), ``cart_dist`` [E], ``cart_dir``
    [E,3], ``ptr`` [B+1] and, if some atoms have no row, ``non_H_mask`` [N] (without it every atom has a row, as
    ``target_row_ptr`` assumes).  ``rows``: the number M of rows, which the caller usually knows from the prediction's
    shape; without it M is the batch's ``y``'s, N if there is no mask, and else counted from the mask (the one host read
    this can cost).  The two lookups are built here, once, with static-shape device ops; nothing else is read back.  A
    ``BatchGraph`` comes back as it is, after the check that it has ``rows`` rows and what the caller needs.  ``who`` and
    ``what`` name the caller and its per-row argument in the messages; ``dev``: the device the arrays must be on (default:
    that of the atomic numbers)."""
    if isinstance(batch, BatchGraph):
        g = batch
        if rows is not None and int(rows) != g.M:
            raise ValueError(f"{what} holds {int(rows)} rows, the batch graph was built for {g.M}")
        if dev is not None and g.z.device != dev:
            raise ValueError(f"{what} and the batch graph are on different devices")
    else:
        z = _batch_field(batch, "x", "z")
        if dev is None and torch.is_tensor(z):
            dev = z.device
        if not (torch.is_tensor(z) and z.dtype == torch.int64 and z.dim() == 1 and z.device == dev):
            raise ValueError(f"{who} needs the atomic numbers in batch.x (a forward has overwritten them)")
        z, N = z.contiguous(), int(z.shape[0])
        ei, dist = (_batch_field(batch, k) for k in ("edge_index", "cart_dist"))
        dirs = _batch_field(batch, "cart_dir") if need_dir else None
        if not (torch.is_tensor(ei) and ei.dtype == torch.int64 and ei.dim() == 2 and ei.shape[0] == 2 and ei.device == dev):
            raise ValueError("edge_index must be an int64 tensor [2,E] on the data's device")
        ei, E = ei.contiguous(), int(ei.shape[1])
        if not (torch.is_tensor(dist) and dist.dtype == torch.float32 and tuple(dist.shape) == (E,) and dist.device == dev
                and (not need_dir or (torch.is_tensor(dirs) and dirs.dtype == torch.float32
                                      and tuple(dirs.shape) == (E, 3) and dirs.device == dev))):
            raise ValueError("cart_dist [E] and cart_dir [E,3] must be fp32 tensors on the data's device" if need_dir else
                             "cart_dist [E] must be an fp32 tensor on the data's device")
        dist, dirs = dist.detach().contiguous(), dirs.detach().contiguous() if need_dir else None
        mask = _batch_field(batch, "non_H_mask")
        if mask is not None and not (tuple(mask.shape) == (N,) and mask.device == dev):
            raise ValueError("non_H_mask must be a tensor [N] on the data's device")
        if rows is None:
            y = _batch_field(batch, "y")
            rows = N if mask is None else int(y.shape[0]) if torch.is_tensor(y) else int(mask.sum())
        M = int(rows)
        if mask is None and M != N:
            raise ValueError(f"{what} holds {M} rows for {N} atoms and the batch has no non_H_mask")
        ptr = _batch_field(batch, "ptr")
        atom_ptr, B = _check_row_ptr(ptr.to(torch.int64), dev) if torch.is_tensor(ptr) else (None, None)
        g = BatchGraph(z, N, ei, E, dist, dirs, mask, M, *_atom_lookups(mask, ei, N, dev), atom_ptr, B,
                       covalent_radii(dev))
    if need_dir and g.cart_dir is None:
        raise ValueError("cart_dist [E] and cart_dir [E,3] must be fp32 tensors on the data's device")
    if need_ptr and g.atom_ptr is None:
        raise ValueError(f"{who} needs the crystals' atom offsets in batch.ptr")
    return g


def bond_test(u: torch.Tensor, batch, row_ptr: torch.Tensor, tol: float = 0.4, threshold: float = 1e-3) -> BondTest:
    """Hirshfeld's rigid-bond test of the ADPs ``u`` [M,3,3] on the bonds of ``batch``: one call of
    ``cartnet_adp_bond_test``.  ``batch``: what ``batch_graph`` takes (``ptr`` is not needed) or its ``BatchGraph``, with
    ``u`` holding one row per atom of the mask, in atom order.  ``row_ptr`` [B+1]: ``target_row_ptr``.  An edge ``j -> i``
    is a bond by the rule of ``cartnet_amd.bonds`` (``r_i + r_j + tol``, both ends non-hydrogen, no self image); only edges
    the graph holds are seen.  Nothing is read back."""
    _check_fp32("u", u)
    u, M, dev = u.detach().contiguous(), int(u.shape[0]), u.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    g = batch_graph(batch, M, "bond_test", "u", need_ptr=False, dev=dev)
    z, N, ei, E, dist, dirs = g.z, g.N, g.edge_index, g.E, g.cart_dist, g.cart_dir
    bonds = torch.empty(M, dtype=torch.int32, device=dev)
    delta_sum = torch.empty(M, dtype=torch.float32, device=dev)
    delta_max = torch.empty(M, dtype=torch.float32, device=dev)
    worst = torch.empty(M, dtype=torch.int64, device=dev)
    over = torch.empty(M, dtype=torch.int32, device=dev)
    ratio = torch.empty(M, dtype=torch.float32, device=dev)
    if M == 0 or N == 0:                         # the entry point launches nothing
        return BondTest(bonds, delta_sum, delta_max, worst, over, ratio,
                        torch.zeros((B, 4), dtype=torch.float64, device=dev))
    stats = torch.empty((B, 4), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _l.check(_l.load().cartnet_adp_bond_test(
            u.data_ptr(), z.data_ptr(), ei.data_ptr(), dist.data_ptr(), dirs.data_ptr(), g.atom_row.data_ptr(),
            g.seg_ptr.data_ptr(), row_ptr.data_ptr(), g.radii.data_ptr(),
            int(g.radii.numel()), float(tol), float(threshold), B, N, M, E, bonds.data_ptr(), delta_sum.data_ptr(),
            delta_max.data_ptr(), worst.data_ptr(), over.data_ptr(), ratio.data_ptr(), stats.data_ptr(),
            _l.stream_ptr()), "cartnet_adp_bond_test")
    return BondTest(bonds, delta_sum, delta_max, worst, over, ratio, stats)


# ---------------------------------------------------------------------------------------------------------------------
# Riding hydrogens (csrc/riding_ops.hip): the model predicts no ADP for a hydrogen; the riding model gives it an isotropic
# U that is a fixed multiple of its parent's U_eq.  The rule: bonds.py.

class RidingH(NamedTuple):
    """What ``riding_h`` returns, all on the device, per atom of the batch: ``parent`` [N] int64, the batch's atom index of
    the atom a hydrogen rides on (-1 for an orphan and for every non-hydrogen atom); ``count`` [N] int32, the hydrogens
    that ride on a non-hydrogen atom (0 for a hydrogen); ``mult`` [N] fp32, a hydrogen's multiplier (0 for an orphan and for
    every non-hydrogen atom); ``u_iso`` [N] fp32, ``mult * u_eq[parent's row]`` for a hydrogen (NaN for an orphan) and the
    atom's own ``u_eq`` for a non-hydrogen atom (NaN without a row); ``crystal_stats`` [B,4] fp64: per crystal its
    hydrogens, its orphans, the sum of the finite ``u_iso`` of its hydrogens and the hydrogens whose parent's ``u_eq`` is
    not positive."""
    parent: torch.Tensor
    count: torch.Tensor
    mult: torch.Tensor
    u_iso: torch.Tensor
    crystal_stats: torch.Tensor


def riding_h(u_eq: torch.Tensor, batch, tol: float = 0.4, f: float = 1.2, f_rot: float = 1.5) -> RidingH:
    """An isotropic U for every hydrogen of ``batch`` from ``u_eq`` [M] (``AdpExport.u_eq``: one row per atom of the mask,
    in atom order): one call of ``cartnet_adp_riding_h``.  ``batch``: what ``batch_graph`` takes (``cart_dir`` is not
    needed) or its ``BatchGraph``.  A hydrogen's parent is the nearest non-hydrogen atom with a row within
    ``r_H + r_parent + tol`` among the edges the graph holds; the multiplier is ``f_rot`` on oxygen and on a carbon that
    carries three or more hydrogens, ``f`` otherwise (the rule: ``cartnet_amd.bonds``).  Nothing is read back."""
    _check_fp32("u_eq", u_eq, (), "[M]")
    u_eq, M, dev = u_eq.detach().contiguous(), int(u_eq.shape[0]), u_eq.device
    g = batch_graph(batch, M, "riding_h", "u_eq", need_dir=False, dev=dev)
    z, N, ei, E, dist, B = g.z, g.N, g.edge_index, g.E, g.cart_dist, g.B
    parent = torch.empty(N, dtype=torch.int64, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    mult = torch.empty(N, dtype=torch.float32, device=dev)
    u_iso = torch.empty(N, dtype=torch.float32, device=dev)
    if N == 0:                                   # the entry point launches nothing
        return RidingH(parent, count, mult, u_iso, torch.zeros((B, 4), dtype=torch.float64, device=dev))
    stats = torch.empty((B, 4), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _l.check(_l.load().cartnet_adp_riding_h(
            _l.ptr(u_eq) if M else None, z.data_ptr(), _l.ptr(ei) if E else None, _l.ptr(dist) if E else None,
            g.atom_row.data_ptr(), g.seg_ptr.data_ptr(), g.atom_ptr.data_ptr(), g.radii.data_ptr(),
            int(g.radii.numel()), float(tol),
            float(f), float(f_rot), B, N, M, E, parent.data_ptr(), count.data_ptr(), mult.data_ptr(), u_iso.data_ptr(),
            stats.data_ptr(), _l.stream_ptr()), "cartnet_adp_riding_h")
    return RidingH(parent, count, mult, u_iso, stats)


# ---------------------------------------------------------------------------------------------------------------------
# Molecules and the rigid-body test (csrc/molecule_ops.hip): the components of the bond graph with every atom's unwrapped
# position, and Hirshfeld's postulate for all pairs of atoms of a molecule (Rosenfield, Trueblood & Dunitz 1978).  Two
# calls, because molecules do not depend on U: found once per batch, tested as often as there are predictions of it.
# The rule: bonds.py.

class Molecules(NamedTuple):
    """What ``molecules`` returns, all on the device: ``label`` [N] int64, the batch's atom index of the root (the lowest
    atom) of an atom's molecule, -1 for an atom without a row; ``x`` [N,3] fp64, the atom's position relative to that
    root, unwrapped through the cell faces; per row ``mol`` [M] int32 (the molecule's number inside its crystal, in the
    order of the roots), ``size`` [M] int32 (its atoms) and ``status`` [M] int32 (bit 1 periodic, bit 2 open; 0 and two or
    more atoms: tested); ``crystal_counts`` [B,5] fp64: molecules, tested, periodic, open, largest size."""
    label: torch.Tensor
    x: torch.Tensor
    mol: torch.Tensor
    size: torch.Tensor
    status: torch.Tensor
    crystal_counts: torch.Tensor


class MoleculeTest(NamedTuple):
    """What ``molecule_test`` returns, all on the device, per row over the other atoms of its molecule: ``pairs`` [M]
    int32; ``delta_sum`` [M] fp32, the sum of ``|D|`` with ``D = r^T (U_i - U_j) r / r.r``; ``delta_max`` [M] fp32;
    ``worst`` [M] int64, the batch's atom index of the partner with the largest ``|D|``; ``over`` [M] int32, the pairs with
    ``|D| > threshold``.  Rows of untested molecules hold 0, 0, 0, -1, 0.  ``crystal_stats`` [B,4] fp64: per crystal the
    sum of ``pairs``, the sum of ``delta_sum``, the maximum of ``delta_max`` and the sum of ``over`` -- DIRECTED, as
    ``BondTest``'s: every pair is seen from both of its ends."""
    pairs: torch.Tensor
    delta_sum: torch.Tensor
    delta_max: torch.Tensor
    worst: torch.Tensor
    over: torch.Tensor
    crystal_stats: torch.Tensor


def _check_molecules(mo: "Molecules", g: BatchGraph, B: int, M: int, dev) -> tuple:
    """``(label, x, status, size)`` of ``mo``, contiguous, after the check that they are the molecules of the batch of
    ``g`` and of a prediction of ``M`` rows in ``B`` crystals on ``dev``."""
    N = g.N
    if not (g.B == B and tuple(mo.label.shape) == (N,) and tuple(mo.x.shape) == (N, 3) and mo.x.dtype == torch.float64
            and mo.label.dtype == torch.int64
            and all(t.dtype == torch.int32 and tuple(t.shape) == (M,) for t in (mo.status, mo.size))
            and all(t.device == dev for t in (mo.label, mo.x, mo.status, mo.size))):
        raise ValueError(f"molecules does not belong to this batch and u ({B} crystals, {M} rows)")
    return tuple(t.contiguous() for t in (mo.label, mo.x, mo.status, mo.size))


def molecules(batch, row_ptr: torch.Tensor, tol: float = 0.4, rows: Optional[int] = None) -> Molecules:
    """The molecules of ``batch``: one call of ``cartnet_molecules``, one workgroup per crystal, nothing read back.
    ``batch`` and ``rows``: what ``batch_graph`` takes, or its ``BatchGraph``.  ``row_ptr`` [B+1]: ``target_row_ptr``.
    A bond is the rigid-bond test's (``cartnet_amd.bonds``); a molecule is a component of the bond graph."""
    g = batch_graph(batch, rows, "molecules")
    z, N, ei, E, dist, dirs, M, dev = g.z, g.N, g.edge_index, g.E, g.cart_dist, g.cart_dir, g.M, g.z.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    if g.B != B:
        raise ValueError(f"row_ptr names {B} crystals, batch.ptr {g.B}")
    label = torch.empty(N, dtype=torch.int64, device=dev)
    x = torch.empty((N, 3), dtype=torch.float64, device=dev)
    mol, size, status = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(3))
    if M == 0 or N == 0:                         # the entry point launches nothing
        return Molecules(label.fill_(-1), x.zero_(), mol, size, status, torch.zeros((B, 5), dtype=torch.float64, device=dev))
    counts = torch.empty((B, 5), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _l.check(_l.load().cartnet_molecules(
            z.data_ptr(), _l.ptr(ei) if E else None, _l.ptr(dist) if E else None, _l.ptr(dirs) if E else None,
            g.atom_row.data_ptr(), g.seg_ptr.data_ptr(), g.atom_ptr.data_ptr(), row_ptr.data_ptr(), g.radii.data_ptr(),
            int(g.radii.numel()), float(tol), B, N, M, E, label.data_ptr(), x.data_ptr(), mol.data_ptr(), size.data_ptr(),
            status.data_ptr(), counts.data_ptr(), _l.stream_ptr()), "cartnet_molecules")
    return Molecules(label, x, mol, size, status, counts)


def molecule_test(u: torch.Tensor, batch, row_ptr: torch.Tensor, molecules: Molecules,
                  threshold: float = 1e-3) -> MoleculeTest:
    """The rigid-body test of the ADPs ``u`` [M,3,3] on the ``molecules`` of ``batch`` (``molecules(batch, row_ptr)``):
    one call of ``cartnet_adp_molecule_test``.  For every row of a tested molecule (status 0, two or more atoms) the other
    atoms of the molecule in atom order, ``D = r^T (U_i - U_j) r / r.r`` along ``r = x_i - x_j``.  ``batch``: the one the
    molecules were found in, or its ``BatchGraph``; nothing is read back."""
    _check_fp32("u", u)
    u, M, dev = u.detach().contiguous(), int(u.shape[0]), u.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    g = batch_graph(batch, M, "molecule_test", "u", need_dir=False, dev=dev)
    N = g.N
    label, x, status, size = _check_molecules(molecules, g, B, M, dev)
    pairs = torch.empty(M, dtype=torch.int32, device=dev)
    delta_sum = torch.empty(M, dtype=torch.float32, device=dev)
    delta_max = torch.empty(M, dtype=torch.float32, device=dev)
    worst = torch.empty(M, dtype=torch.int64, device=dev)
    over = torch.empty(M, dtype=torch.int32, device=dev)
    if M == 0 or N == 0:                         # the entry point launches nothing
        return MoleculeTest(pairs, delta_sum, delta_max, worst, over, torch.zeros((B, 4), dtype=torch.float64, device=dev))
    stats = torch.empty((B, 4), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _l.check(_l.load().cartnet_adp_molecule_test(
            u.data_ptr(), label.data_ptr(), x.data_ptr(), g.atom_row.data_ptr(), g.atom_ptr.data_ptr(), row_ptr.data_ptr(),
            status.data_ptr(), size.data_ptr(), float(threshold), B, N, M, pairs.data_ptr(), delta_sum.data_ptr(),
            delta_max.data_ptr(), worst.data_ptr(), over.data_ptr(), stats.data_ptr(), _l.stream_ptr()),
            "cartnet_adp_molecule_test")
    return MoleculeTest(pairs, delta_sum, delta_max, worst, over, stats)


class TlsFit(NamedTuple):
    """What ``tls_fit`` returns, all on the device, per row: ``u_tls`` [M,3,3] fp32, the ADP the fitted rigid body gives
    the row's atom; ``resid`` [M] fp32, ``|Sym U - u_tls|_F``; and the figures of the row's molecule, repeated on each of
    its rows: ``params`` [M,24] fp32 (T as 11 22 33 23 13 12, L the same, S row-major, the origin relative to the
    molecule's root atom), ``eig`` [M,6] fp32 (the principal values of T, then of L, ascending), ``rank`` [M] int32 (20: all
    parameters determined; less: the minimum-norm representative; -1: the iteration's sweeps ran out) and ``rfac`` [M]
    fp32.  Rows of unfitted molecules hold NaN, 0, NaN, NaN, 0, 0.  ``crystal_stats`` [B,6] fp64: fitted molecules, those
    with ``rank < 20``, those with a negative principal value of T or L, the sum of ``resid^2``, the sum of
    ``|Sym U|_F^2`` over the fitted rows and the largest ``resid``."""
    u_tls: torch.Tensor
    resid: torch.Tensor
    params: torch.Tensor
    eig: torch.Tensor
    rank: torch.Tensor
    rfac: torch.Tensor
    crystal_stats: torch.Tensor


def tls_fit(u: torch.Tensor, batch, row_ptr: torch.Tensor, molecules: Molecules) -> TlsFit:
    """The TLS fit of the ADPs ``u`` [M,3,3] on the ``molecules`` of ``batch`` (``molecules(batch, row_ptr)``): one call of
    ``cartnet_adp_tls_fit``.  Every molecule with status 0 and five or more atoms gets the rigid-body tensors T, L and S
    that explain its ADPs best (Schomaker & Trueblood 1968; the rule: ``cartnet_amd.bonds``).  ``batch``: the one the
    molecules were found in, or its ``BatchGraph``; nothing is read back."""
    _check_fp32("u", u)
    u, M, dev = u.detach().contiguous(), int(u.shape[0]), u.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    g = batch_graph(batch, M, "tls_fit", "u", need_dir=False, dev=dev)
    N = g.N
    label, x, status, size = _check_molecules(molecules, g, B, M, dev)
    u_tls = torch.empty((M, 3, 3), dtype=torch.float32, device=dev)
    resid = torch.empty(M, dtype=torch.float32, device=dev)
    params = torch.empty((M, 24), dtype=torch.float32, device=dev)
    eig = torch.empty((M, 6), dtype=torch.float32, device=dev)
    rank = torch.empty(M, dtype=torch.int32, device=dev)
    rfac = torch.empty(M, dtype=torch.float32, device=dev)
    if M == 0 or N == 0:                         # the entry point launches nothing
        return TlsFit(u_tls, resid, params, eig, rank, rfac, torch.zeros((B, 6), dtype=torch.float64, device=dev))
    stats = torch.empty((B, 6), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _l.check(_l.load().cartnet_adp_tls_fit(
            u.data_ptr(), label.data_ptr(), x.data_ptr(), g.atom_row.data_ptr(), g.atom_ptr.data_ptr(), row_ptr.data_ptr(),
            status.data_ptr(), size.data_ptr(), B, N, M, u_tls.data_ptr(), resid.data_ptr(), params.data_ptr(),
            eig.data_ptr(), rank.data_ptr(), rfac.data_ptr(), stats.data_ptr(), _l.stream_ptr()), "cartnet_adp_tls_fit")
    return TlsFit(u_tls, resid, params, eig, rank, rfac, stats)


# ---------------------------------------------------------------------------------------------------------------------
# Anisotropic hydrogens (csrc/aniso_h_ops.hip): where the riding model gives a hydrogen one number, this gives it a tensor
# -- its parent's, plus the change of the molecule's fitted rigid-body motion from the parent to the hydrogen, plus a
# nominal internal X-H motion in the bond frame (SHADE, ADPH).  The rule: bonds.py.

class AnisoH(NamedTuple):
    """What ``aniso_h`` returns, all on the device, per atom of the batch: ``u_h`` [N,3,3] fp32, a non-hydrogen atom's own
    row (bit for bit; NaN without a row) and a hydrogen's tensor (exactly symmetric; NaN for an orphan); ``source`` [N]
    int32: 0 no tensor, 1 the atom's own row, 2 the parent's tensor plus the internal motion, 3 that plus the libration
    of a fully determined TLS fit, 4 the same from a rank-deficient fit (its minimum-norm representative);
    ``crystal_stats`` [B,4] fp64: per crystal the hydrogens with a tensor, those with ``source >= 3``, the sum of their
    ``trace / 3`` and those whose tensor is not positive definite."""
    u_h: torch.Tensor
    source: torch.Tensor
    crystal_stats: torch.Tensor


def aniso_h(u: torch.Tensor, batch, row_ptr: torch.Tensor, riding: RidingH, molecules: Optional[Molecules] = None,
            tls: Optional[TlsFit] = None, stretch: float = 0.005, bend: float = 0.020) -> AnisoH:
    """A displacement tensor for every hydrogen of ``batch`` from the ADPs ``u`` [M,3,3] of the non-hydrogen atoms: one
    call of ``cartnet_adp_aniso_h``.  ``batch``: what ``batch_graph`` takes, or its ``BatchGraph``;
    ``row_ptr`` [B+1]: ``target_row_ptr``; ``riding``: ``riding_h`` of the same batch (its ``parent``
    is read).  ``molecules`` and ``tls`` (``molecules(batch, row_ptr)`` and ``tls_fit`` on them): both or neither; with
    them a hydrogen whose parent's molecule was fitted also gets the change of that rigid-body motion from the parent's
    position to its own, without them every hydrogen with a parent has ``source = 2``.  ``stretch`` / ``bend`` (A^2): the
    internal mean-square displacement along and across the X-H bond; the defaults are nominal figures
    (``cartnet_amd.bonds``).  Nothing is read back."""
    _check_fp32("u", u)
    u, M, dev = u.detach().contiguous(), int(u.shape[0]), u.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    g = batch_graph(batch, M, "aniso_h", "u", dev=dev)
    if g.B != B:
        raise ValueError(f"row_ptr names {B} crystals, batch.ptr {g.B}")
    z, N, ei, E, dist, dirs = g.z, g.N, g.edge_index, g.E, g.cart_dist, g.cart_dir
    parent = riding.parent
    if not (parent.dtype == torch.int64 and tuple(parent.shape) == (N,) and parent.device == dev):
        raise ValueError(f"riding does not belong to this batch ({N} atoms)")
    if (molecules is None) != (tls is None):
        raise ValueError("molecules and tls come together or not at all")
    x = params = rank = None
    if tls is not None:
        x, params, rank = _check_molecules(molecules, g, B, M, dev)[1], tls.params, tls.rank
        if not (tuple(params.shape) == (M, 24) and params.dtype == torch.float32 and tuple(rank.shape) == (M,)
                and rank.dtype == torch.int32 and params.device == dev and rank.device == dev):
            raise ValueError(f"molecules and tls do not belong to this batch and u ({N} atoms, {M} rows)")
        params, rank = params.contiguous(), rank.contiguous()
    u_h = torch.empty((N, 3, 3), dtype=torch.float32, device=dev)
    source = torch.empty(N, dtype=torch.int32, device=dev)
    if N == 0:                                   # the entry point launches nothing
        return AnisoH(u_h, source, torch.zeros((B, 4), dtype=torch.float64, device=dev))
    parent = parent.contiguous()
    stats = torch.empty((B, 4), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _l.check(_l.load().cartnet_adp_aniso_h(
            _l.ptr(u) if M else None, z.data_ptr(), _l.ptr(ei) if E else None, _l.ptr(dist) if E else None,
            _l.ptr(dirs) if E else None, g.atom_row.data_ptr(), g.seg_ptr.data_ptr(), g.atom_ptr.data_ptr(), parent.data_ptr(),
            _l.ptr(x) if M else None, _l.ptr(params) if M else None, _l.ptr(rank) if M else None, float(stretch),
            float(bend), B, N, M, E, u_h.data_ptr(), source.data_ptr(), stats.data_ptr(), _l.stream_ptr()),
            "cartnet_adp_aniso_h")
    return AnisoH(u_h, source, stats)


# ---------------------------------------------------------------------------------------------------------------------
# The bond table (csrc/bond_table_ops.hip): one entry per bond where the analyses above give figures per atom -- D with
# its sign, the Busing & Levy bounds on the bond length and the length corrected for the fitted libration.  Two calls,
# because the bonds do not depend on U: counted once per batch, filled as often as there are predictions of it.  The
# rule: bonds.py.

class BondIndex(NamedTuple):
    """What ``bond_index`` returns: ``counts`` [N] int32, per atom ``i`` the bonds ``j -> i`` with ``j < i``, which the
    table lists; ``offsets`` [N+1] int64, their exclusive scan (atom i's entries start at ``offsets[i]``); ``bond_ptr``
    [B+1] int64, the crystals' offsets into the table, on the device, and ``bond_ptr_host``, the same on the host (the one
    copy ``bond_index`` makes: the table's length is ``bond_ptr_host[-1]``); ``unlisted`` [N] int32, per atom ``i`` its
    bond edges with ``j > i``, which are counted and never listed; ``tol``, the tolerance the bonds were found with."""
    counts: torch.Tensor
    offsets: torch.Tensor
    bond_ptr: torch.Tensor
    bond_ptr_host: torch.Tensor
    unlisted: torch.Tensor
    tol: float


class BondTable(NamedTuple):
    """What ``bond_table`` returns, all on the device, per listed bond (``nb`` of them, in target order and within a target
    in edge order): ``a`` and ``b`` [nb] int64, the batch's atom indices of the edge's source and target, ``a < b``;
    ``dir`` [nb,3] and ``length`` [nb] fp32, the edge's ``cart_dir`` and ``cart_dist`` as stored; ``delta`` [nb] fp32,
    ``d^T (Sym U_b - Sym U_a) d``, signed; ``lower`` and ``upper`` [nb] fp32, the Busing & Levy bounds on the thermally
    averaged length (NaN where a tensor has a negative or NaN mean-square displacement across the bond); ``libration``
    [nb] fp32, the length corrected for the libration ``L`` of the TLS fit of ``b``'s molecule (NaN without a fit) and
    ``tls_rank`` [nb] int32, that fit's rank (0 without one); ``crystal_stats`` [B,9] fp64: listed bonds, unlisted ``j > i``
    bond edges, sum of ``length``, sum of ``|delta|``, largest ``|delta|`` (keeps a NaN), bonds with a finite
    ``libration``, sum and largest of ``libration - length`` over those, bonds with a NaN bound."""
    a: torch.Tensor
    b: torch.Tensor
    dir: torch.Tensor
    length: torch.Tensor
    delta: torch.Tensor
    lower: torch.Tensor
    upper: torch.Tensor
    libration: torch.Tensor
    tls_rank: torch.Tensor
    crystal_stats: torch.Tensor


def bond_index(batch, row_ptr: torch.Tensor, tol: float = 0.4, rows: Optional[int] = None) -> BondIndex:
    """Where the bonds of ``batch`` go in its bond table: one call of ``cartnet_bond_table_count``, a static-shape scan
    (``torch.cumsum``) and ONE small device-to-host copy, the ``B + 1`` offsets of the crystals.  ``batch`` and ``rows``:
    what ``batch_graph`` takes, or its ``BatchGraph``; ``row_ptr`` [B+1]: ``target_row_ptr``.  A bond is the rigid-bond
    test's (``cartnet_amd.bonds``); it does not depend on U, so one index serves every prediction of the batch."""
    g = batch_graph(batch, rows, "bond_index", need_dir=False)
    z, N, ei, E, dist, M, dev = g.z, g.N, g.edge_index, g.E, g.cart_dist, g.M, g.z.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    if g.B != B:
        raise ValueError(f"row_ptr names {B} crystals, batch.ptr {g.B}")
    counts = torch.zeros(N, dtype=torch.int32, device=dev)
    unlisted = torch.zeros(N, dtype=torch.int32, device=dev)
    if N and M:                                  # else nothing is launched: no atom has a bond
        with torch.cuda.device(dev):
            _l.check(_l.load().cartnet_bond_table_count(
                z.data_ptr(), _l.ptr(ei) if E else None, _l.ptr(dist) if E else None, g.atom_row.data_ptr(),
                g.seg_ptr.data_ptr(), g.radii.data_ptr(), int(g.radii.numel()), float(tol), N, M, E, counts.data_ptr(),
                unlisted.data_ptr(), _l.stream_ptr()), "cartnet_bond_table_count")
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0, dtype=torch.int64)])
    bond_ptr = offsets[g.atom_ptr.clamp(0, N)]
    return BondIndex(counts, offsets, bond_ptr, bond_ptr.cpu(), unlisted, float(tol))


def bond_table(u: torch.Tensor, batch, row_ptr: torch.Tensor, index: BondIndex, tls: Optional[TlsFit] = None) -> BondTable:
    """The bond table of the ADPs ``u`` [M,3,3] on the bonds of ``batch``: one call of ``cartnet_adp_bond_table``.
    ``batch``: what ``batch_graph`` takes, or its ``BatchGraph``; ``row_ptr`` [B+1]: ``target_row_ptr``; ``index``:
    ``bond_index`` of the same batch.  ``tls``: a ``tls_fit`` of the same ``u``; with it a bond of a fitted molecule gets
    its ``libration`` and ``tls_rank``, without it they are NaN and 0.  Nothing is read back."""
    _check_fp32("u", u)
    u, M, dev = u.detach().contiguous(), int(u.shape[0]), u.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    g = batch_graph(batch, M, "bond_table", "u", dev=dev)
    if g.B != B:
        raise ValueError(f"row_ptr names {B} crystals, batch.ptr {g.B}")
    z, N, ei, E, dist, dirs = g.z, g.N, g.edge_index, g.E, g.cart_dist, g.cart_dir
    offsets, unlisted, on_host = index.offsets, index.unlisted, index.bond_ptr_host
    if not (tuple(offsets.shape) == (N + 1,) and offsets.dtype == torch.int64 and tuple(unlisted.shape) == (N,)
            and unlisted.dtype == torch.int32 and offsets.device == dev and unlisted.device == dev
            and tuple(on_host.shape) == (B + 1,) and on_host.device.type == "cpu"):
        raise ValueError(f"index does not belong to this batch ({N} atoms, {B} crystals)")
    params = rank = None
    if tls is not None:
        params, rank = tls.params, tls.rank
        if not (tuple(params.shape) == (M, 24) and params.dtype == torch.float32 and tuple(rank.shape) == (M,)
                and rank.dtype == torch.int32 and params.device == dev and rank.device == dev):
            raise ValueError(f"tls does not belong to this u ({M} rows)")
        params, rank = params.contiguous(), rank.contiguous()
    nb = int(on_host[-1])
    a, b = (torch.empty(nb, dtype=torch.int64, device=dev) for _ in range(2))
    out_dir = torch.empty((nb, 3), dtype=torch.float32, device=dev)
    length, delta, lower, upper, libration = (torch.empty(nb, dtype=torch.float32, device=dev) for _ in range(5))
    tls_rank = torch.empty(nb, dtype=torch.int32, device=dev)
    if M == 0 or N == 0:                         # the entry point launches nothing
        return BondTable(a, b, out_dir, length, delta, lower, upper, libration, tls_rank,
                         torch.zeros((B, 9), dtype=torch.float64, device=dev))
    stats = torch.empty((B, 9), dtype=torch.float64, device=dev)
    offsets, unlisted = offsets.contiguous(), unlisted.contiguous()
    entries = (a, b, out_dir, length, delta, lower, upper, libration, tls_rank)
    with torch.cuda.device(dev):
        _l.check(_l.load().cartnet_adp_bond_table(
            u.data_ptr(), z.data_ptr(), _l.ptr(ei) if E else None, _l.ptr(dist) if E else None, _l.ptr(dirs) if E else None,
            g.atom_row.data_ptr(), g.seg_ptr.data_ptr(), g.atom_ptr.data_ptr(), g.radii.data_ptr(), int(g.radii.numel()),
            float(index.tol), offsets.data_ptr(), unlisted.data_ptr(), _l.ptr(params) if M else None,
            _l.ptr(rank) if M else None, B, N, M, E, nb, *(t.data_ptr() if nb else None for t in entries),
            stats.data_ptr(), _l.stream_ptr()), "cartnet_adp_bond_table")
    return BondTable(*entries, stats)


# ---------------------------------------------------------------------------------------------------------------------
# The angle and torsion tables (csrc/angle_table_ops.hip): the valence angles and the torsions of the bond graph from the
# edges alone, each with the value the fitted libration gives.  Two calls, as for the bond table: what is listed does not
# depend on U, only the libration columns do (through the TLS fit).  The rule: bonds.py.

class AngleIndex(NamedTuple):
    """What ``angle_index`` returns, all on the device but the last: ``bonds``, the ``BondIndex`` it builds on (a degree
    is its ``counts + unlisted``, a torsion's central bond a row of its table); ``nbr_ptr`` [N+1] int64, the exclusive scan
    of the degrees; ``adj`` [E] int64, atom i's bond edges in edge order from ``adj[nbr_ptr[i]]`` on (what lies past
    ``nbr_ptr[N]`` is not written); per listed bond ``bond_edge`` [nb] int64 (its edge), ``reverse`` [nb] int64 (the edge
    that holds it in the other direction, -1 if the graph has none) and ``torsion_counts`` [nb] int64 with their
    exclusive scan ``torsion_offsets`` [nb+1]; ``angle_counts`` [N] int64, ``d (d - 1) / 2`` per atom, with
    ``angle_offsets`` [N+1]; ``angle_ptr`` and ``torsion_ptr`` [B+1] int64, the crystals' offsets into the two tables, and
    ``table_ptr_host`` [2,B+1], both on the host (the one copy ``angle_index`` makes: the tables' lengths are
    ``table_ptr_host[:, -1]``)."""
    bonds: BondIndex
    nbr_ptr: torch.Tensor
    adj: torch.Tensor
    bond_edge: torch.Tensor
    reverse: torch.Tensor
    torsion_counts: torch.Tensor
    torsion_offsets: torch.Tensor
    angle_counts: torch.Tensor
    angle_offsets: torch.Tensor
    angle_ptr: torch.Tensor
    torsion_ptr: torch.Tensor
    table_ptr_host: torch.Tensor


class AngleTable(NamedTuple):
    """What ``angle_table`` returns, all on the device.  Per valence angle a-b-c (centres in atom order, the pairs of a
    centre's bond edges by the first, then the second): ``angle_a``, ``angle_b``, ``angle_c`` [na] int64, the batch's atom
    indices; ``angle_value`` [na] fp32, degrees; ``angle_libration`` [na] fp32, the angle after the libration ``L`` of the
    TLS fit of ``b``'s molecule (NaN without a fit) and ``angle_tls_rank`` [na] int32, that fit's rank (0 without one).
    Per torsion a-b-c-d (the bond table's bonds b-c in its order, then the neighbours of ``b``, then those of ``c``):
    ``torsion_a`` ... ``torsion_d`` [nt] int64; ``torsion_value`` [nt] fp32, degrees in (-180, 180] with the IUPAC sign,
    NaN for a collinear end; ``torsion_libration`` and ``torsion_tls_rank`` as above, read at ``c``.  ``angle_stats``
    [B,5] fp64: entries, sum of the values, entries with a finite libration, sum and largest of ``|libration - value|``
    over those; ``torsion_stats`` [B,5] fp64: entries, NaN values, entries with a finite libration, sum and largest of the
    circular ``|libration - value|`` over those."""
    angle_a: torch.Tensor
    angle_b: torch.Tensor
    angle_c: torch.Tensor
    angle_value: torch.Tensor
    angle_libration: torch.Tensor
    angle_tls_rank: torch.Tensor
    torsion_a: torch.Tensor
    torsion_b: torch.Tensor
    torsion_c: torch.Tensor
    torsion_d: torch.Tensor
    torsion_value: torch.Tensor
    torsion_libration: torch.Tensor
    torsion_tls_rank: torch.Tensor
    angle_stats: torch.Tensor
    torsion_stats: torch.Tensor


def _scan(counts: torch.Tensor) -> torch.Tensor:
    """The exclusive scan of ``counts`` [n] with its total, [n+1] int64: a static-shape device op."""
    return torch.cat([counts.new_zeros(1, dtype=torch.int64), torch.cumsum(counts, 0, dtype=torch.int64)])


def _check_bond_index(bonds: BondIndex, N: int, B: int, dev) -> int:
    """The length of the bond table of ``bonds`` after the check that it is the index of a batch of ``N`` atoms in ``B``
    crystals on ``dev``."""
    offsets, unlisted, counts, on_host = bonds.offsets, bonds.unlisted, bonds.counts, bonds.bond_ptr_host
    if not (tuple(offsets.shape) == (N + 1,) and offsets.dtype == torch.int64 and offsets.device == dev
            and all(tuple(t.shape) == (N,) and t.dtype == torch.int32 and t.device == dev for t in (unlisted, counts))
            and tuple(bonds.bond_ptr.shape) == (B + 1,) and bonds.bond_ptr.device == dev
            and tuple(on_host.shape) == (B + 1,) and on_host.device.type == "cpu"):
        raise ValueError(f"index does not belong to this batch ({N} atoms, {B} crystals)")
    return int(on_host[-1])


def angle_index(batch, row_ptr: torch.Tensor, tol: float = 0.4, rows: Optional[int] = None,
                bonds: Optional[BondIndex] = None) -> AngleIndex:
    """Where the angles and the torsions of ``batch`` go in their tables: ``cartnet_bond_adjacency`` and
    ``cartnet_angle_table_count``, static-shape scans around them and ONE small device-to-host copy, the two ``[B+1]``
    offsets of the crystals together.  ``batch`` and ``rows``: what ``batch_graph`` takes, or its ``BatchGraph``;
    ``row_ptr`` [B+1]: ``target_row_ptr``; ``bonds``: the ``bond_index`` of the same batch and tolerance if there is one
    already (else it is built here, with its own copy).  Nothing depends on U, so one index serves every prediction of the batch."""
    g = batch_graph(batch, rows, "angle_index")
    N, ei, E, dist, dirs, M, dev = g.N, g.edge_index, g.E, g.cart_dist, g.cart_dir, g.M, g.z.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    if g.B != B:
        raise ValueError(f"row_ptr names {B} crystals, batch.ptr {g.B}")
    if bonds is None:
        bonds = bond_index(g, row_ptr, tol)
    elif bonds.tol != float(tol):
        raise ValueError(f"bonds was built with the tolerance {bonds.tol}, not {float(tol)}")
    nb = _check_bond_index(bonds, N, B, dev)
    nbr_ptr = _scan(bonds.counts.to(torch.int64) + bonds.unlisted)
    adj = torch.empty(E, dtype=torch.int64, device=dev)
    bond_edge, reverse, torsion_counts = (torch.empty(nb, dtype=torch.int64, device=dev) for _ in range(3))
    angle_counts = torch.zeros(N, dtype=torch.int64, device=dev)
    if N and M and E:                            # else nothing is launched: no atom has a bond
        offsets = bonds.offsets.contiguous()
        with torch.cuda.device(dev):
            _l.check(_l.load().cartnet_bond_adjacency(
                g.z.data_ptr(), ei.data_ptr(), dist.data_ptr(), g.atom_row.data_ptr(), g.seg_ptr.data_ptr(),
                g.radii.data_ptr(), int(g.radii.numel()), float(tol), nbr_ptr.data_ptr(), offsets.data_ptr(), N, M, E, nb,
                adj.data_ptr(), _l.ptr(bond_edge) if nb else None, _l.stream_ptr()), "cartnet_bond_adjacency")
            _l.check(_l.load().cartnet_angle_table_count(
                ei.data_ptr(), dist.data_ptr(), dirs.data_ptr(), nbr_ptr.data_ptr(), offsets.data_ptr(), adj.data_ptr(),
                _l.ptr(bond_edge) if nb else None, N, E, nb, angle_counts.data_ptr(), _l.ptr(reverse) if nb else None,
                _l.ptr(torsion_counts) if nb else None, _l.stream_ptr()), "cartnet_angle_table_count")
    angle_offsets, torsion_offsets = _scan(angle_counts), _scan(torsion_counts)
    angle_ptr, torsion_ptr = angle_offsets[g.atom_ptr.clamp(0, N)], torsion_offsets[bonds.bond_ptr.clamp(0, nb)]
    return AngleIndex(bonds, nbr_ptr, adj, bond_edge, reverse, torsion_counts, torsion_offsets, angle_counts, angle_offsets,
                      angle_ptr, torsion_ptr, torch.stack([angle_ptr, torsion_ptr]).cpu())


def angle_table(batch, row_ptr: torch.Tensor, index: AngleIndex, tls: Optional[TlsFit] = None) -> AngleTable:
    """The angle and torsion tables of ``batch``: one call of ``cartnet_adp_angle_table``.  ``batch``: what
    ``batch_graph`` takes, or its ``BatchGraph``; ``row_ptr`` [B+1]: ``target_row_ptr``; ``index``: ``angle_index`` of the
    same batch.  ``tls``: a ``tls_fit`` of a prediction of the batch; with it an entry of a fitted molecule gets its
    ``libration`` and ``tls_rank``, without it they are NaN and 0.  Nothing is read back."""
    g = batch_graph(batch, None if tls is None else int(tls.rank.shape[0]), "angle_table", "tls")
    N, ei, E, dist, dirs, M, dev = g.N, g.edge_index, g.E, g.cart_dist, g.cart_dir, g.M, g.z.device
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    if g.B != B:
        raise ValueError(f"row_ptr names {B} crystals, batch.ptr {g.B}")
    nb = _check_bond_index(index.bonds, N, B, dev)
    on_host = index.table_ptr_host
    lists = {"nbr_ptr": N + 1, "adj": E, "bond_edge": nb, "reverse": nb, "torsion_offsets": nb + 1, "angle_offsets": N + 1}
    if not (all(tuple(getattr(index, k).shape) == (n,) and getattr(index, k).dtype == torch.int64
                and getattr(index, k).device == dev for k, n in lists.items())
            and tuple(on_host.shape) == (2, B + 1) and on_host.device.type == "cpu"):
        raise ValueError(f"index does not belong to this batch ({N} atoms, {B} crystals)")
    params = rank = None
    if tls is not None:
        params, rank = tls.params, tls.rank
        if not (tuple(params.shape) == (M, 24) and params.dtype == torch.float32 and tuple(rank.shape) == (M,)
                and rank.dtype == torch.int32 and params.device == dev and rank.device == dev):
            raise ValueError(f"tls does not belong to this batch ({M} rows)")
        params, rank = params.contiguous(), rank.contiguous()
    na, nt = int(on_host[0, -1]), int(on_host[1, -1])
    angles = tuple(torch.empty(na, dtype=d, device=dev) for d in (torch.int64,) * 3 + (torch.float32,) * 2 + (torch.int32,))
    torsions = tuple(torch.empty(nt, dtype=d, device=dev) for d in (torch.int64,) * 4 + (torch.float32,) * 2 + (torch.int32,))
    if M == 0 or N == 0:                         # the entry point launches nothing
        return AngleTable(*angles, *torsions, *(torch.zeros((B, 5), dtype=torch.float64, device=dev) for _ in range(2)))
    stats = tuple(torch.empty((B, 5), dtype=torch.float64, device=dev) for _ in range(2))
    nbr_ptr, offsets, adj, bond_edge, reverse, angle_offsets, torsion_offsets = (t.contiguous() for t in (
        index.nbr_ptr, index.bonds.offsets, index.adj, index.bond_edge, index.reverse, index.angle_offsets,
        index.torsion_offsets))
    with torch.cuda.device(dev):
        _l.check(_l.load().cartnet_adp_angle_table(
            _l.ptr(ei) if E else None, _l.ptr(dist) if E else None, _l.ptr(dirs) if E else None, g.atom_row.data_ptr(),
            g.atom_ptr.data_ptr(), nbr_ptr.data_ptr(), offsets.data_ptr(), _l.ptr(adj) if E else None,
            _l.ptr(bond_edge) if nb else None, _l.ptr(reverse) if nb else None, angle_offsets.data_ptr(),
            torsion_offsets.data_ptr(), _l.ptr(params), _l.ptr(rank), B, N, M, E, nb, na, nt,
            *(t.data_ptr() if na else None for t in angles), *(t.data_ptr() if nt else None for t in torsions),
            stats[0].data_ptr(), stats[1].data_ptr(), _l.stream_ptr()), "cartnet_adp_angle_table")
    return AngleTable(*angles, *torsions, *stats)


# ---------------------------------------------------------------------------------------------------------------------
# Temperature series (csrc/series_ops.hip): the exported ADPs of one batch predicted at T temperatures, as a least-squares
# line per row and component -- how fast the ellipsoids grow, and whether they grow at all.

class TempSeries(NamedTuple):
    """What ``temp_series`` returns, all on the device.  ``slope`` [M,6] fp32 (A^2/K) and ``intercept`` [M,6] (the line
    extrapolated to 0 K) of ``u_cif``'s six components; ``ueq_slope`` [M] and ``ueq_intercept`` [M], the same for ``u_eq``;
    ``resid`` [M], the largest distance of a member from its line over the temperatures and the seven columns (a NaN is
    kept); ``drops`` [M] int32, the steps on which ``u_eq`` falls; ``crystal_stats`` [B,4] fp64: per crystal the sum of
    ``ueq_slope``, the rows whose ``ueq_slope`` is not > 0 (a NaN counts), the rows with ``drops > 0`` and the maximum of
    ``resid``, (0, 0, 0, 0) without rows (``None`` if not requested)."""
    slope: torch.Tensor
    intercept: torch.Tensor
    ueq_slope: torch.Tensor
    ueq_intercept: torch.Tensor
    resid: torch.Tensor
    drops: torch.Tensor
    crystal_stats: Optional[torch.Tensor]


def check_temperatures(temps, least: int = 2, name: str = "temps") -> list:
    """``temps`` (a sequence or a tensor of Kelvin values) as a list of floats; raises ``ValueError`` unless it holds at
    least ``least`` values, all finite and > 0, strictly increasing."""
    import math
    values = [float(v) for v in (temps.tolist() if torch.is_tensor(temps) else temps)]
    if len(values) < least:
        raise ValueError(f"{name} must hold at least {least} temperature{'s' if least > 1 else ''}")
    if not all(math.isfinite(v) and v > 0 for v in values):
        raise ValueError(f"{name} must be finite and > 0 (Kelvin)")
    if any(b <= a for a, b in zip(values, values[1:])):
        raise ValueError(f"{name} must be strictly increasing")
    return values


def temp_series(u_cif: torch.Tensor, u_eq: torch.Tensor, temps, row_ptr: torch.Tensor, stats: bool = True) -> TempSeries:
    """The line through a batch's exported ADPs over T temperatures: one call of ``cartnet_adp_temp_series``.  ``u_cif``
    [T*M,6] and ``u_eq`` [T*M] temperature-major (rows ``t*M ... (t+1)*M-1``: ``AdpExport.u_cif`` / ``.u_eq`` of the batch
    at ``temps[t]``); ``temps``: T >= 2 Kelvin values, a sequence or a tensor, finite, > 0 and strictly increasing (checked
    on the host); ``row_ptr`` [B+1] over ONE temperature's rows.  fp64 arithmetic from the fp32 inputs, one rounding to
    fp32 per result."""
    _check_fp32("u_cif", u_cif, (6,), "[T*M,6]")
    _check_fp32("u_eq", u_eq, (), "[T*M]")
    dev = u_cif.device
    if u_eq.device != dev or u_eq.shape[0] != u_cif.shape[0]:
        raise ValueError("u_eq must hold one value per row of u_cif, on its device")
    row_ptr, B = _check_row_ptr(row_ptr, dev)
    values = check_temperatures(temps)
    T = len(values)
    if int(u_cif.shape[0]) % T:
        raise ValueError(f"u_cif holds {int(u_cif.shape[0])} rows: no multiple of the {T} temperatures of temps")
    if torch.is_tensor(temps) and temps.device == dev and temps.dtype == torch.float32:
        t_dev = temps.detach().reshape(-1).contiguous()
    else:
        t_dev = torch.tensor(values, dtype=torch.float32, device=dev)
    u_cif, u_eq, M = u_cif.detach().contiguous(), u_eq.detach().contiguous(), int(u_cif.shape[0]) // T
    slope = torch.empty((M, 7), dtype=torch.float32, device=dev)
    intercept = torch.empty((M, 7), dtype=torch.float32, device=dev)
    resid = torch.empty(M, dtype=torch.float32, device=dev)
    drops = torch.empty(M, dtype=torch.int32, device=dev)
    if M == 0:                                   # the entry point launches nothing
        cs = torch.zeros((B, 4), dtype=torch.float64, device=dev) if stats else None
    else:
        cs = torch.empty((B, 4), dtype=torch.float64, device=dev) if stats else None
        _l.check(_l.load().cartnet_adp_temp_series(u_cif.data_ptr(), u_eq.data_ptr(), t_dev.data_ptr(), T,
                                                   row_ptr.data_ptr(), B, M, slope.data_ptr(), intercept.data_ptr(),
                                                   resid.data_ptr(), drops.data_ptr(), _l.ptr(cs), _l.stream_ptr()),
                 "cartnet_adp_temp_series")
    return TempSeries(slope[:, :6], intercept[:, :6], slope[:, 6], intercept[:, 6], resid, drops, cs)


def split_rows(t: torch.Tensor, rows) -> list:
    """The per-crystal pieces of a host tensor whose dim 0 runs over the rows of a batch: one transfer per batch, then
    this split by the crystals' row counts (a sequence of ints) gives the reference's one-entry-per-crystal lists.  Every
    piece owns its memory: a pickled view would drag the whole batch's storage along."""
    return [piece.clone() for piece in torch.split(t, [int(r) for r in rows], dim=0)]


def to_host(tensors: dict) -> dict:
    """The device tensors of ``tensors`` on the host, through ONE device-to-host copy: their bytes are packed into one
    buffer on the device, and every tensor is cut back out of its host copy (each owning its memory)."""
    items = [(k, t.detach().contiguous()) for k, t in tensors.items()]
    flat = torch.cat([t.view(torch.uint8).reshape(-1) if t.numel() else t.new_empty(0, dtype=torch.uint8)
                      for _, t in items]).to("cpu")
    out, at = {}, 0
    for k, t in items:
        n = t.numel() * t.element_size()
        out[k] = flat[at:at + n].clone().view(t.dtype).reshape(t.shape)
        at += n
    return out

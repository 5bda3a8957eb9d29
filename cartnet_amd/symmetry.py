"""From the asymmetric unit of a CIF to the contents of the unit cell, and predictions back to one ADP per site.

The reference takes the packed cell from the CSD API and drops repeated atoms on the host
(dataset/extract_csd_data.py:84-88, ``delete_repeated`` :28-40), then brings the file's ``U_ij`` into the Cartesian frame
(:115-123).  ``expand`` does that for a list of ``cartnet_amd.cif.CifCrystal`` with the file's own symmetry operators, all
crystals in one pass on the GPU (csrc/symmetry_ops.hip): one count pass, ONE device-to-host copy of the sizes, one fill
pass.  ``site_average`` goes the other way for a batch of predictions.  ``expand_host`` states the same rule in torch fp64
on the CPU, with the kernels' operation order.

The rule.  Candidate ``c = s * n + a`` of a crystal with n atoms and m operators is atom a under operator s (operator 0 is
the identity): ``f' = ((W0 f0 + W1 f1) + W2 f2) + w`` in fp64, minus its floor, rounded to fp32, then the reference's
normalisation (< 0: + 1; > 1: - 1; within 1.1e-4 of 1: 0).  ``rep[i]`` is the lowest ``j < i`` whose fp32 Euclidean
distance to i is below 1e-4 (no periodic wrap), else i; candidate i is kept iff ``rep[i] == i``.  A crystal in which some
``rep[rep[i]] != rep[i]`` (atoms between one and two thresholds apart) is refused by name, and so is a singular cell.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _l
from .cif import CifCrystal

TILE = 256                       # candidates per workgroup (SO_THREADS of csrc/shard_tiles.h)
THRESHOLD = 1e-4                 # delete_repeated's distance threshold


@dataclass
class CifSymmetry:
    """What maps the rows of an expanded shard back to the asymmetric units.  On the host: ``names``, and per crystal
    ``labels``, ``frac`` [n,3] fp64, ``z`` [n], ``symops`` (strings, identity first) and ``sites`` (the indices of the
    non-hydrogen asymmetric atoms); ``site_count`` [G].  On the device: ``op_ptr``, ``op_rot`` [S,9] int8, ``op_trans``
    [S,3], ``cell`` [G,9] fp64, ``orb_ptr``, ``orbit_row`` (per non-hydrogen asymmetric atom and operator: the
    crystal-local row of the image's representative), and ``row_asym`` / ``row_op`` per non-hydrogen row -- all indexed by
    non-hydrogen rows, so they survive ``DeviceShard.without_hydrogens()``."""
    names: List[str]
    labels: List[List[str]]
    frac: List[np.ndarray]
    z: List[np.ndarray]
    symops: List[List[str]]
    sites: List[np.ndarray]
    site_count: np.ndarray
    op_ptr: torch.Tensor
    op_rot: torch.Tensor
    op_trans: torch.Tensor
    cell: torch.Tensor
    orb_ptr: torch.Tensor
    orbit_row: torch.Tensor
    row_asym: torch.Tensor
    row_op: torch.Tensor
    y_ptr: np.ndarray


def _check(crystals: Sequence[CifCrystal], labeled: bool, temperature: Optional[float]) -> None:
    if len(crystals) == 0:
        raise ValueError("no crystals to expand")
    for c in crystals:
        why = c.reject_reason(labeled, temperature)
        if why is not None:
            raise ValueError(f"crystal {c.name}: {why}")


def host_inputs(crystals: Sequence[CifCrystal], labeled: bool, temperature: Optional[float] = None) -> Dict[str, np.ndarray]:
    """The CSR arrays the kernels read, and the tile table: one entry per 256 consecutive candidates of one crystal."""
    _check(crystals, labeled, temperature)
    n = np.array([len(c.labels) for c in crystals], dtype=np.int64)
    m = np.array([len(c.symops) for c in crystals], dtype=np.int64)
    z = np.concatenate([np.asarray(c.z, dtype=np.int32) for c in crystals])
    heavy = [np.asarray(c.z) != 1 for c in crystals]
    sites = np.array([int(h.sum()) for h in heavy], dtype=np.int64)

    def csr(counts):
        return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cand = n * m
    tiles = (cand + TILE - 1) // TILE
    tile_g = np.repeat(np.arange(len(crystals), dtype=np.int32), tiles)
    cand_ptr = csr(cand)
    first_tile = csr(tiles)[:-1]
    tile_c0 = cand_ptr[tile_g] + (np.arange(tile_g.shape[0], dtype=np.int64) - first_tile[tile_g]) * TILE
    out = {
        "asym_ptr": csr(n), "op_ptr": csr(m), "cand_ptr": cand_ptr, "site_ptr": csr(sites), "orb_ptr": csr(sites * m),
        "asym_frac": np.concatenate([np.asarray(c.frac, dtype=np.float64).reshape(-1, 3) for c in crystals]),
        "asym_z": z,
        "asym_site": np.concatenate([np.where(h, np.cumsum(h) - 1, -1) for h in heavy]).astype(np.int32),
        "op_rot": np.concatenate([np.stack([W for W, _ in c.symops]).reshape(-1, 9) for c in crystals]).astype(np.int8),
        "op_trans": np.concatenate([np.stack([w for _, w in c.symops]).reshape(-1, 3) for c in crystals]).astype(np.float64),
        "cell": np.stack([c.cell().reshape(9) for c in crystals]).astype(np.float64),
        "tile_g": tile_g, "tile_c0": tile_c0.astype(np.int64),
        "temperature": np.array([c.temperature if c.temperature is not None else temperature for c in crystals],
                                dtype=np.float32),
    }
    if not np.isfinite(out["asym_frac"]).all():
        raise ValueError("a fractional coordinate is not finite")
    if labeled:
        out["asym_ucif"] = np.concatenate([c.u_cif() for c in crystals]).astype(np.float64)
    return out


def _refuse(crystals: Sequence[CifCrystal], g: int, bits: int) -> None:
    what = "its cell is singular or not finite" if bits & 1 else \
        f"atoms between {THRESHOLD:g} and {2 * THRESHOLD:g} apart in fractional coordinates: which of them repeat is ambiguous"
    raise ValueError(f"crystal {crystals[g].name}: {what}")


def _symmetry(crystals, h: Dict[str, np.ndarray], dev: Dict[str, torch.Tensor], y_ptr: np.ndarray) -> CifSymmetry:
    return CifSymmetry(
        names=[c.name for c in crystals], labels=[list(c.labels) for c in crystals],
        frac=[np.asarray(c.frac, dtype=np.float64).reshape(-1, 3) for c in crystals],
        z=[np.asarray(c.z, dtype=np.int32) for c in crystals], symops=[list(c.symop_strings) for c in crystals],
        sites=[np.nonzero(np.asarray(c.z) != 1)[0] for c in crystals], site_count=np.diff(h["site_ptr"]),
        op_ptr=dev["op_ptr"], op_rot=dev["op_rot"], op_trans=dev["op_trans"], cell=dev["cell"], orb_ptr=dev["orb_ptr"],
        orbit_row=dev["orbit_row"], row_asym=dev["row_asym"], row_op=dev["row_op"], y_ptr=np.asarray(y_ptr, dtype=np.int64))


def expand(crystals: Sequence[CifCrystal], device="cuda:0", labeled: bool = False,
           temperature: Optional[float] = None) -> Tuple[Dict[str, np.ndarray], CifSymmetry]:
    """The unit-cell contents of ``crystals`` (every one accepted by ``reject_reason``; ``temperature`` fills in a missing
    one).  Returns ``(arrays, CifSymmetry)``: ``arrays`` is a geometry-only dict as ``shard.pack`` gives -- ``atom_ptr``,
    ``y_ptr``, ``z``, ``pos``, ``non_h_mask``, ``cell``, ``temperature`` (Kelvin) and, labeled, ``y`` [Y,9] -- for
    ``DeviceShard(arrays, device, labeled=..., names=...)`` or ``shard.write_arrays``.  Raises ``ValueError`` naming the
    first crystal that is ambiguous or whose cell is singular."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("expand runs on the GPU (expand_host states the rule on the CPU)")
    h = host_inputs(crystals, labeled, temperature)
    lib = _l.load()
    G, A, S, C, nT = len(crystals), int(h["asym_ptr"][-1]), int(h["op_ptr"][-1]), int(h["cand_ptr"][-1]), len(h["tile_g"])
    O = int(h["orb_ptr"][-1])
    with torch.cuda.device(dev):
        d = {k: torch.from_numpy(v).to(dev) for k, v in h.items() if k != "temperature"}
        common = [d[k].data_ptr() for k in ("asym_ptr", "asym_frac", "asym_z", "op_ptr", "op_rot", "op_trans", "cell",
                                            "cand_ptr", "tile_g", "tile_c0")] + [G, A, S, C, nT]
        ws_bytes = int(lib.cartnet_symmetry_expand_workspace_bytes(G, C, nT))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        atom_ptr = torch.empty(G + 1, dtype=torch.int64, device=dev)
        y_ptr = torch.empty(G + 1, dtype=torch.int64, device=dev)
        totals = torch.empty(4, dtype=torch.int64, device=dev)
        _l.check(lib.cartnet_symmetry_expand_count(*common, ws.data_ptr(), ws_bytes, atom_ptr.data_ptr(), y_ptr.data_ptr(),
                                                   totals.data_ptr(), _l.stream_ptr()), "cartnet_symmetry_expand_count")
        n_out, y_out, bits, bad = totals.tolist()                # the one device-to-host copy: sizes and status
        if bits:
            _refuse(crystals, int(bad), int(bits))
        new = {"z": torch.empty(n_out, dtype=torch.int32, device=dev),
               "pos": torch.empty((n_out, 3), dtype=torch.float32, device=dev),
               "non_h_mask": torch.empty(n_out, dtype=torch.uint8, device=dev),
               "cell": torch.empty((G, 9), dtype=torch.float32, device=dev)}
        rows = {"row_asym": torch.empty(y_out, dtype=torch.int32, device=dev),
                "row_op": torch.empty(y_out, dtype=torch.int32, device=dev),
                "orbit_row": torch.full((O,), -1, dtype=torch.int32, device=dev)}
        _l.check(lib.cartnet_symmetry_expand_fill(
            *common, ws.data_ptr(), ws_bytes, y_ptr.data_ptr(), d["asym_site"].data_ptr(), d["orb_ptr"].data_ptr(), n_out,
            y_out, new["z"].data_ptr(), new["pos"].data_ptr(), new["non_h_mask"].data_ptr(), rows["row_asym"].data_ptr(),
            rows["row_op"].data_ptr(), rows["orbit_row"].data_ptr(), new["cell"].data_ptr(), _l.stream_ptr()),
            "cartnet_symmetry_expand_fill")
        if labeled:
            new["y"] = torch.empty((y_out, 9), dtype=torch.float32, device=dev)
            _l.check(lib.cartnet_symmetry_targets(
                d["asym_ptr"].data_ptr(), d["asym_ucif"].data_ptr(), d["op_ptr"].data_ptr(), d["op_rot"].data_ptr(),
                d["cell"].data_ptr(), y_ptr.data_ptr(), rows["row_asym"].data_ptr(), rows["row_op"].data_ptr(), G, y_out,
                new["y"].data_ptr(), _l.stream_ptr()), "cartnet_symmetry_targets")
        from .metrics import to_host
        host = to_host({"atom_ptr": atom_ptr, "y_ptr": y_ptr, **new})
    arrays = {k: host[k].numpy() for k in ("atom_ptr", "y_ptr", "z", "pos", "non_h_mask", "cell")}
    arrays["temperature"] = h["temperature"]
    if labeled:
        arrays["y"] = host["y"].numpy()
    return arrays, _symmetry(crystals, h, {**d, **rows}, arrays["y_ptr"])


def site_average(pred: torch.Tensor, row_ptr: torch.Tensor, sel: Sequence[int], sym: CifSymmetry):
    """One ADP per non-hydrogen asymmetric atom of the crystals ``sel`` (indices into the expansion) of a batch whose
    per-atom predictions are ``pred`` [M,3,3] with row offsets ``row_ptr`` [B+1] (device): ``(u_cif_asym [H,6],
    spread [H])`` on the device, the crystals' sites in batch order.  ``u_cif_asym`` is the mean over the operators of the
    orbit's predictions, each brought back to the site (``U11 U22 U33 U23 U13 U12`` in the file's own setting);
    ``spread`` the largest deviation of a member from that mean.  No device-to-host copy."""
    sel_np = np.asarray(sel.cpu() if torch.is_tensor(sel) else sel, dtype=np.int64).reshape(-1)
    B = int(sel_np.shape[0])
    G = int(sym.site_count.shape[0])
    if B and (int(sel_np.min()) < 0 or int(sel_np.max()) >= G):
        raise IndexError("crystal index out of range")
    dev = pred.device
    meta = np.zeros(2 * B + 1, dtype=np.int64)                  # [sel | site offsets]
    meta[:B] = sel_np
    np.cumsum(sym.site_count[sel_np], out=meta[B + 1:])
    H = int(meta[-1])
    u = torch.empty((H, 6), dtype=torch.float32, device=dev)
    spread = torch.empty(H, dtype=torch.float32, device=dev)
    if H == 0:
        return u, spread
    pred = pred.contiguous()
    if pred.dtype != torch.float32 or pred.numel() % 9:
        raise ValueError("pred must be fp32 [M,3,3]")
    M = pred.numel() // 9
    with torch.cuda.device(dev):
        meta_d = torch.from_numpy(meta).pin_memory().to(dev, non_blocking=True)
        row_ptr = row_ptr.to(torch.int64).contiguous()
        _l.check(_l.load().cartnet_symmetry_average(
            pred.data_ptr(), row_ptr.data_ptr(), meta_d.data_ptr(), meta_d.data_ptr() + 8 * B, B, M, H,
            sym.op_ptr.data_ptr(), sym.op_rot.data_ptr(), sym.orb_ptr.data_ptr(), sym.orbit_row.data_ptr(),
            sym.cell.data_ptr(), G, int(sym.op_rot.shape[0]), int(sym.orbit_row.shape[0]), u.data_ptr(), spread.data_ptr(),
            _l.stream_ptr()), "cartnet_symmetry_average")
    return u, spread


# ------------------------------------------------------------------------------------------------ the rule on the host
def _normalise(x: torch.Tensor) -> torch.Tensor:
    """The reference's normalisation of fp32 fractions (dataset/extract_csd_data.py:29-31)."""
    one = torch.ones((), dtype=torch.float32)
    x = torch.where(x < 0, x + one, x)
    x = torch.where(x > 1, x - one, x)
    near = (x - one).abs() <= torch.tensor(1e-4, dtype=torch.float32) + torch.tensor(1e-5, dtype=torch.float32)
    return torch.where(near, torch.zeros((), dtype=torch.float32), x)


def candidates_host(frac: torch.Tensor, W: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """[m * n, 3] fp32 normalised fractions of the candidates, operator-major; ``frac`` [n,3], ``W`` [m,3,3], ``w`` [m,3]
    fp64."""
    f = frac.to(torch.float64)
    W = W.to(torch.float64)
    v = ((W[:, None, :, 0] * f[None, :, None, 0] + W[:, None, :, 1] * f[None, :, None, 1])
         + W[:, None, :, 2] * f[None, :, None, 2]) + w.to(torch.float64)[:, None, :]
    v = v - torch.floor(v)
    return _normalise(v.to(torch.float32)).reshape(-1, 3)


def first_duplicate_host(x: torch.Tensor) -> torch.Tensor:
    """``rep`` [c] int64 of fp32 coordinates ``x`` [c,3]: the lowest j with distance(i, j) < 1e-4 in fp32 (j = i at the
    latest)."""
    d = x[:, None, :] - x[None, :, :]
    dist = torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    idx = torch.arange(x.shape[0])
    close = (dist < torch.tensor(THRESHOLD, dtype=torch.float32)) & (idx[None, :] <= idx[:, None])
    return torch.where(close, idx[None, :], x.shape[0]).min(dim=1).values


def targets_host(u_cif: torch.Tensor, W: torch.Tensor, cell: torch.Tensor) -> torch.Tensor:
    """[r,3,3] fp64: ``cell^T (W (N U N) W^T) cell`` for ``u_cif`` [r,6] (U11 U22 U33 U23 U13 U12), ``W`` [r,3,3]."""
    u = u_cif.to(torch.float64)
    full = torch.stack([u[:, 0], u[:, 5], u[:, 4], u[:, 5], u[:, 1], u[:, 3], u[:, 4], u[:, 3], u[:, 2]], 1).view(-1, 3, 3)
    M = cell.to(torch.float64).view(3, 3)
    n = torch.linalg.norm(torch.linalg.inv(M.T), dim=-1)
    W = W.to(torch.float64)
    beta = W @ (n[:, None] * full * n[None, :]) @ W.transpose(1, 2)
    return M.T @ beta @ M


def expand_host(crystals: Sequence[CifCrystal], labeled: bool = False, temperature: Optional[float] = None):
    """``expand`` in torch on the CPU, crystal by crystal: ``(arrays, rows)`` with ``arrays`` as ``expand`` returns them
    and ``rows`` = ``{"row_asym", "row_op", "orbit_row", "orb_ptr"}`` as numpy arrays.  Same operation order as the
    kernels; ``pos`` and ``y`` are the fp64 results rounded once."""
    h = host_inputs(crystals, labeled, temperature)
    out = {k: [] for k in ("z", "pos", "non_h_mask", "y", "row_asym", "row_op", "orbit_row")}
    atoms, heavy_rows = [0], [0]
    for g, c in enumerate(crystals):
        a0, a1, s0, s1 = (int(v) for v in (h["asym_ptr"][g], h["asym_ptr"][g + 1], h["op_ptr"][g], h["op_ptr"][g + 1]))
        n, m = a1 - a0, s1 - s0
        W = torch.from_numpy(h["op_rot"][s0:s1].astype(np.int64)).view(m, 3, 3)
        cell = torch.from_numpy(h["cell"][g]).view(3, 3)
        if not bool(torch.isfinite(cell).all()) or float(torch.linalg.det(cell)) == 0.0:
            _refuse(crystals, g, 1)
        x = candidates_host(torch.from_numpy(h["asym_frac"][a0:a1]), W, torch.from_numpy(h["op_trans"][s0:s1]))
        rep = first_duplicate_host(x)
        if bool((rep[rep] != rep).any()):
            _refuse(crystals, g, 2)
        idx = torch.arange(n * m)
        keep = rep == idx
        z = torch.from_numpy(h["asym_z"][a0:a1].astype(np.int64)).repeat(m)
        heavy = keep & (z != 1)
        xk = x[keep].to(torch.float64)
        pos = (xk[:, 0:1] * cell[0:1] + xk[:, 1:2] * cell[1:2]) + xk[:, 2:3] * cell[2:3]
        rank_h = torch.cumsum(heavy.to(torch.int64), 0) - 1
        a_of, s_of = idx % n, idx // n
        out["z"].append(z[keep].to(torch.int32))
        out["pos"].append(pos.to(torch.float32))
        out["non_h_mask"].append((z[keep] != 1).to(torch.uint8))
        out["row_asym"].append(a_of[heavy].to(torch.int32))
        out["row_op"].append(s_of[heavy].to(torch.int32))
        sites = torch.nonzero(z[:n] != 1).reshape(-1)
        cand = s_of.new_tensor(range(m))[None, :] * n + sites[:, None]          # [sites, m]
        out["orbit_row"].append(rank_h[rep[cand]].reshape(-1).to(torch.int32))
        if labeled:
            u = torch.from_numpy(h["asym_ucif"][a0:a1])
            out["y"].append(targets_host(u[a_of[heavy]], W[s_of[heavy]], cell).reshape(-1, 9).to(torch.float32))
        atoms.append(atoms[-1] + int(keep.sum()))
        heavy_rows.append(heavy_rows[-1] + int(heavy.sum()))
    arrays = {"atom_ptr": np.array(atoms, dtype=np.int64), "y_ptr": np.array(heavy_rows, dtype=np.int64),
              "z": torch.cat(out["z"]).numpy(), "pos": torch.cat(out["pos"]).numpy(),
              "non_h_mask": torch.cat(out["non_h_mask"]).numpy(), "cell": h["cell"].astype(np.float32),
              "temperature": h["temperature"]}
    if labeled:
        arrays["y"] = torch.cat(out["y"]).numpy()
    rows = {k: torch.cat(out[k]).numpy() for k in ("row_asym", "row_op", "orbit_row")}
    rows["orb_ptr"] = h["orb_ptr"]
    return arrays, rows

"""Packed crystal shards and device-side batching.

The reference keeps one pickled PyG ``Data`` per structure, ``torch.load``s it per sample in 5 worker processes
(dataset/datasetADP.py:41-42; loader/loader.py:114-124), augments / standardises on the CPU (:33-39,43-45,76-77) and
copies every batch over PCIe.  Here a dataset split is ONE flat file of CSR arrays that is uploaded to HBM once
(the whole ADP dataset -- ~2e5 crystals, ~6e8 edges, ~25 GB -- is a fraction of the 288 GB), and a batch is built by a
single kernel launch on the device (``cartnet_collate``), including the SO(3) augmentation.

File layout (little endian): 8-byte magic ``CNSHARD1``, a JSON header padded to a multiple of 64 bytes (its length
as uint64 right after the magic) listing ``{"name": [dtype, shape, offset]}``, then the arrays, each 64-byte aligned:

    atom_ptr, edge_ptr, y_ptr [G+1] int64 | z [N] int32 | pos [N,3] f32 | non_h_mask [N] u8 |
    edge_src, edge_tgt [E] int32 (atom index inside the crystal) | cart_dist [E] f32 | cart_dir [E,3] f32 |
    cell [G,9] f32 | temperature [G] f32 | y [Y, y_width] f32 (y_width 9: one ADP tensor per non-H atom)

``pos``, ``non_h_mask``, ``cell`` and ``temperature`` are optional (the Jarvis / MP graphs carry no mask or
temperature).  A geometry-only shard leaves out ``edge_ptr`` and the four edge arrays and must carry ``pos`` and
``cell``: ``DeviceShard.with_radius_graph`` builds its graph on the GPU.  The header may record the graph's provenance,
``"graph": {"radius": r, "max_neighbors": k or null}`` (``read_shard_meta``).

An unlabeled shard (crystals to predict ADPs for: the header says ``"targets": false``) has no ``y``; its ``y_ptr`` counts
the non-hydrogen atoms (``z != 1``), the rows the per-atom head produces, and it always stores ``non_h_mask``.  The header
may also carry ``"names"``, one string per crystal.
"""
from __future__ import annotations

import json
import struct
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import lib as _l
from .data import Batch, Data

MAGIC = b"CNSHARD1"
_ALIGN = 64
_OPTIONAL = ("pos", "non_h_mask", "cell", "temperature")
_EDGE_ARRAYS = ("edge_ptr", "edge_src", "edge_tgt", "cart_dist", "cart_dir")


def graph_record(radius: float, max_neighbors: Optional[int] = None) -> Dict[str, object]:
    """The provenance record of a radius graph: ``{"radius": r, "max_neighbors": k or None}`` (a cap <= 0 is no cap)."""
    k = int(max_neighbors) if max_neighbors is not None and int(max_neighbors) > 0 else None
    return {"radius": float(radius), "max_neighbors": k}


def pack(data_list: Sequence[Data]) -> Dict[str, np.ndarray]:
    """Flat CSR arrays of a list of crystals (the attribute set of cartnet_amd.data / SURVEY.md 8a).  Crystals without
    ``edge_index`` -- all of the list or none -- give a geometry-only shard (no ``edge_ptr``, no edge arrays), which needs
    ``pos`` and ``cell``.  Crystals without ``y`` -- again all or none -- give an unlabeled ADP shard: no ``y`` array,
    ``y_ptr`` over the non-hydrogen atoms, ``non_h_mask`` from ``z != 1`` where the crystals carry none."""
    if len(data_list) == 0:
        raise ValueError("cannot pack an empty list of crystals")
    with_edges = [hasattr(d, "edge_index") for d in data_list]
    if any(with_edges) and not all(with_edges):
        raise ValueError("crystals with and without edge_index in one list: a shard carries the graph of all its crystals "
                         "or of none")
    with_y = [hasattr(d, "y") for d in data_list]
    if any(with_y) and not all(with_y):
        raise ValueError("crystals with and without y in one list: a shard carries the targets of all its crystals or of "
                         "none")
    labeled = with_y[0]
    d0 = data_list[0]
    if not with_edges[0] and not all(hasattr(d, "pos") and hasattr(d, "cell") for d in data_list):
        raise ValueError("a crystal without edge_index needs pos and cell (DeviceShard.with_radius_graph builds the graph)")
    n = [int(d.x.shape[0]) for d in data_list]
    if labeled:
        per_atom = d0.y.dim() == 3
        ys = [d.y.reshape(-1, 9) if per_atom else d.y.reshape(1, -1) for d in data_list]
        rows = [y.shape[0] for y in ys]
    else:
        rows = [int((d.x != 1).sum()) for d in data_list]      # the rows the per-atom head will produce
    e = [int(d.edge_index.shape[1]) for d in data_list] if with_edges[0] else []

    def edge(make):                       # an edge array, in its place in the file's array order; None for geometry only
        return make() if with_edges[0] else None
    out = {
        "atom_ptr": np.concatenate([[0], np.cumsum(n)]).astype(np.int64),
        "edge_ptr": edge(lambda: np.concatenate([[0], np.cumsum(e)]).astype(np.int64)),
        "y_ptr": np.concatenate([[0], np.cumsum(rows)]).astype(np.int64),
        "z": torch.cat([d.x for d in data_list]).numpy().astype(np.int32),
        "edge_src": edge(lambda: torch.cat([d.edge_index[0] for d in data_list]).numpy().astype(np.int32)),
        "edge_tgt": edge(lambda: torch.cat([d.edge_index[1] for d in data_list]).numpy().astype(np.int32)),
        "cart_dist": edge(lambda: torch.cat([d.cart_dist for d in data_list]).numpy().astype(np.float32)),
        "cart_dir": edge(lambda: torch.cat([d.cart_dir for d in data_list]).numpy().astype(np.float32).reshape(-1, 3)),
        "y": torch.cat(ys).numpy().astype(np.float32) if labeled else None,
    }
    out = {k: v for k, v in out.items() if v is not None}
    if hasattr(d0, "pos"):
        out["pos"] = torch.cat([d.pos for d in data_list]).numpy().astype(np.float32).reshape(-1, 3)
    if hasattr(d0, "non_H_mask"):
        out["non_h_mask"] = torch.cat([d.non_H_mask for d in data_list]).numpy().astype(np.uint8)
    elif not labeled:
        out["non_h_mask"] = (out["z"] != 1).astype(np.uint8)
    if hasattr(d0, "cell"):
        out["cell"] = torch.cat([d.cell.reshape(1, 9) for d in data_list]).numpy().astype(np.float32)
    if hasattr(d0, "temperature"):
        out["temperature"] = torch.cat([d.temperature.reshape(1) for d in data_list]).numpy().astype(np.float32)
    for i, d in enumerate(data_list):
        if with_edges[0] and e[i] and bool((d.edge_index[1][1:] < d.edge_index[1][:-1]).any()):
            raise ValueError(f"crystal {i}: edge_index[1] must be sorted ascending")
    return out


def pack_with_gpu_graph(geometries: Sequence[Data], radius: float = 5.0, device="cuda:0",
                        max_neighbors: Optional[int] = None) -> Dict[str, np.ndarray]:
    """Flat CSR arrays (as ``pack``) of crystals given WITHOUT edges -- ``x`` (atomic numbers), ``pos``, ``cell`` and the
    targets -- whose periodic radius graphs are built on the GPU in one pass (``DeviceShard.with_radius_graph``: the
    reference's dataset/utils.py:57-237 edge order, integers bit-exact) and brought back to the host."""
    arrays = pack(geometries)
    out = DeviceShard(arrays, device, labeled="y" in arrays).with_radius_graph(radius, max_neighbors)
    return {k: v.cpu().numpy() for k, v in out.t.items()}


def write_shard(path: str, data_list: Sequence[Data], graph: Optional[Dict[str, object]] = None,
                names: Optional[Sequence[str]] = None) -> None:
    """``names``: one string per crystal, stored in the header.  ``graph``: how the crystals' edges were built,
    ``{"radius": r, "max_neighbors": k or None}``; recorded in the header, so that a loader can tell whether the graph it
    wants is the one stored (the reference's cached-directory test, dataset/utils.py:462-464)."""
    write_arrays(path, pack(data_list), graph=graph, names=names)


def write_arrays(path: str, arrays: Dict[str, np.ndarray], graph: Optional[Dict[str, object]] = None,
                 names: Optional[Sequence[str]] = None) -> None:
    """``write_shard`` for crystals that are flat CSR arrays already (``pack``'s result, or the host copy of a resident
    shard's tensors): arrays without ``y`` give an unlabeled shard."""
    order = ("atom_ptr", "edge_ptr", "y_ptr", "z", "edge_src", "edge_tgt", "cart_dist", "cart_dir", "y", "pos", "non_h_mask",
             "cell", "temperature")
    arrays = {k: np.asarray(arrays[k]) for k in order if k in arrays}
    n_graphs = int(arrays["atom_ptr"].shape[0]) - 1
    if graph is not None:
        if "edge_ptr" not in arrays:
            raise ValueError("a geometry-only shard has no graph to record")
        graph = graph_record(graph["radius"], graph.get("max_neighbors"))
    meta, off = {}, 0
    for k, a in arrays.items():
        meta[k] = [a.dtype.str, list(a.shape), off]
        off += (a.nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
    head = {"arrays": meta, "graphs": n_graphs}
    if graph is not None:
        head["graph"] = graph
    if "y" not in arrays:
        head["targets"] = False
    if names is not None:
        names = [str(n) for n in names]
        if len(names) != n_graphs:
            raise ValueError(f"{len(names)} names for {n_graphs} crystals")
        head["names"] = names
    header = json.dumps(head).encode()
    header += b" " * (-(len(MAGIC) + 8 + len(header)) % _ALIGN)
    with open(path, "wb") as f:
        f.write(MAGIC)
        f.write(struct.pack("<Q", len(header)))
        f.write(header)
        for k, a in arrays.items():
            f.write(np.ascontiguousarray(a).tobytes())
            f.write(b"\0" * (-a.nbytes % _ALIGN))


def _read_header(path: str):
    with open(path, "rb") as f:
        if f.read(8) != MAGIC:
            raise ValueError(f"{path}: not a CartNet shard")
        (hlen,) = struct.unpack("<Q", f.read(8))
        return json.loads(f.read(hlen).decode()), 16 + hlen


def read_shard_meta(path: str) -> Dict[str, object]:
    """The JSON header of a shard file: ``arrays``, ``graphs`` and, if they were recorded, ``graph``, ``names`` and
    ``"targets": false`` (an unlabeled shard)."""
    return _read_header(path)[0]


def read_shard(path: str) -> Dict[str, np.ndarray]:
    """Memory-maps the arrays of a shard file (no copy until they are uploaded)."""
    meta, base = _read_header(path)
    out = {}
    for k, (dt, shape, off) in meta["arrays"].items():
        out[k] = np.memmap(path, dtype=np.dtype(dt), mode="r", offset=base + off, shape=tuple(shape))
    return out


class DeviceShard:
    """A shard resident in HBM.  ``collate(sel)`` builds the batch of crystals ``sel`` with one kernel launch.
    ``graph``: the provenance of its edges, ``{"radius": r, "max_neighbors": k or None}``, or None when unknown.  A
    geometry-only shard (``has_graph`` False: ``pos`` and ``cell`` but no edge arrays) only serves ``with_radius_graph``.
    ``labeled=False``: an unlabeled ADP shard, arrays without ``y`` (None means labeled; ``from_file`` takes it from the
    header); its batches carry a zero ``y`` of the right size.  ``names``: one string per crystal, or None."""

    def __init__(self, arrays: Dict[str, np.ndarray], device="cuda:0", graph: Optional[Dict[str, object]] = None,
                 labeled: Optional[bool] = None, names: Optional[Sequence[str]] = None):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("DeviceShard lives on the GPU; there is no CPU path (use Batch.from_data_list on the host)")
        self._labeled = True if labeled is None else bool(labeled)
        if not self._labeled and "y" in arrays:
            raise ValueError("an unlabeled shard carries no y")
        # unlabeled: per-atom ADP prediction only, whose rows are the non-hydrogen atoms
        need = ("atom_ptr", "y_ptr", "z") + (("y",) if self._labeled else ("non_h_mask",))
        if any(k in arrays for k in _EDGE_ARRAYS):
            need += _EDGE_ARRAYS
        else:
            need += ("pos", "cell")                                 # geometry only: with_radius_graph() needs both
        missing = [k for k in need if k not in arrays]
        if missing:
            raise ValueError(f"shard lacks {missing}")
        self.device = dev
        self.graph = graph_record(graph["radius"], graph.get("max_neighbors")) if graph is not None else None
        # host copies of the offsets: batch sizes are known without a device round trip
        self.atom_ptr = np.asarray(arrays["atom_ptr"], dtype=np.int64)
        self.num_graphs = int(self.atom_ptr.shape[0] - 1)
        self.names = [str(n) for n in names] if names is not None else None
        if self.names is not None and len(self.names) != self.num_graphs:
            raise ValueError(f"{len(self.names)} names for {self.num_graphs} crystals")
        self.edge_ptr = (np.asarray(arrays["edge_ptr"], dtype=np.int64) if "edge_ptr" in arrays
                         else np.zeros(self.num_graphs + 1, dtype=np.int64))
        self.y_ptr = np.asarray(arrays["y_ptr"], dtype=np.int64)
        for name, p in (("atom_ptr", self.atom_ptr), ("edge_ptr", self.edge_ptr), ("y_ptr", self.y_ptr)):
            if p.shape[0] != self.num_graphs + 1 or p[0] != 0 or bool((np.diff(p) < 0).any()):
                raise ValueError(f"{name} is not a valid offset array")
        sizes = {"z": self.atom_ptr[-1], "pos": self.atom_ptr[-1], "non_h_mask": self.atom_ptr[-1],
                 "edge_src": self.edge_ptr[-1], "edge_tgt": self.edge_ptr[-1], "cart_dist": self.edge_ptr[-1],
                 "cart_dir": self.edge_ptr[-1], "cell": self.num_graphs, "temperature": self.num_graphs,
                 "y": self.y_ptr[-1]}
        self.t: Dict[str, torch.Tensor] = {}
        for k, a in arrays.items():
            if k in sizes and int(a.shape[0]) != int(sizes[k]):
                raise ValueError(f"{k}: {a.shape[0]} rows, expected {int(sizes[k])}")
            self.t[k] = torch.from_numpy(np.array(a)).to(dev)       # np.array: memmaps are read-only
        self._describe()

    def _describe(self) -> None:
        """The C descriptor of the device tensors in ``self.t``."""
        if self._labeled:
            self.y_width = int(self.t["y"].shape[1]) if self.t["y"].dim() == 2 else 1
        else:
            self.y_width = 9                    # the per-atom head's 3x3 rows; the descriptor's y stays NULL
        self.per_atom_target = self.y_width == 9
        d = _l.Shard()
        for k in ("atom_ptr", "edge_ptr", "y_ptr", "z", "pos", "non_h_mask", "edge_src", "edge_tgt", "cart_dist",
                  "cart_dir", "cell", "temperature", "y"):
            setattr(d, k, self.t[k].data_ptr() if k in self.t else None)
        d.y_width = self.y_width
        self._desc = d
        self._lib = _l.load()

    @classmethod
    def from_file(cls, path: str, device="cuda:0") -> "DeviceShard":
        meta = read_shard_meta(path)
        return cls(read_shard(path), device, graph=meta.get("graph"), labeled=bool(meta.get("targets", True)),
                   names=meta.get("names"))

    @classmethod
    def from_data_list(cls, data_list: Sequence[Data], device="cuda:0") -> "DeviceShard":
        arrays = pack(data_list)
        return cls(arrays, device, labeled="y" in arrays)

    @property
    def labeled(self) -> bool:
        """False for an unlabeled shard: no ``y``; ``collate`` gives its batches a zero ``y`` with one row per non-hydrogen
        atom."""
        return self._labeled

    def nbytes(self) -> int:
        return sum(v.numel() * v.element_size() for v in self.t.values())

    @property
    def has_graph(self) -> bool:
        return "edge_src" in self.t

    def _need_graph(self, what: str) -> None:
        if not self.has_graph:
            raise ValueError(f"{what}: this shard holds only geometry; build its graph first with with_radius_graph()")

    def _derived(self, new: Dict[str, torch.Tensor], atom_ptr: np.ndarray, edge_ptr: np.ndarray,
                 graph: Optional[Dict[str, object]]) -> "DeviceShard":
        """A resident shard that owns the tensors in ``new`` and shares every other one with this shard."""
        out = object.__new__(DeviceShard)
        out.device, out.num_graphs, out._lib, out.graph = self.device, self.num_graphs, self._lib, graph
        out._labeled, out.names = self._labeled, self.names
        out.atom_ptr, out.edge_ptr, out.y_ptr = atom_ptr, edge_ptr, self.y_ptr
        out.t = {**self.t, **new}
        out._describe()
        return out

    def with_radius_graph(self, radius: float = 5.0, max_neighbors: Optional[int] = None) -> "DeviceShard":
        """The same crystals with the periodic radius graph of ``radius`` (capped at ``max_neighbors`` per target atom,
        None or <= 0: uncapped) rebuilt from ``pos`` and ``cell``, as a new resident shard (this one is untouched): what the
        reference's ``compute_knn`` does per file on the CPU before an e/iComformer run on ADP (dataset/utils.py:456-486,
        loader/loader.py:24-26) and ``Figshare_Dataset.process`` for Jarvis / MegNet (dataset/figshare_dataset.py:50-76),
        done in one pass over the whole shard on the GPU (csrc/radius_graph.hip, driven by
        ``cartnet_amd.graph.radius_graph_csr``, which ``radius_graph_pbc`` runs over a batch).  The new shard owns
        ``edge_ptr``, ``edge_src``, ``edge_tgt``, ``cart_dist`` and ``cart_dir``; every other array is shared.  Apply it
        BEFORE ``without_hydrogens()`` / ``with_optimized_cell()``, as the reference caps the graph of the full crystal in
        the stored frame."""
        t = self.t
        if "pos" not in t or "cell" not in t:
            raise ValueError("with_radius_graph needs the shard's pos and cell")
        if not float(radius) > 0.0:
            raise ValueError("radius must be positive")
        from .graph import radius_graph_csr
        new = dict(zip(_EDGE_ARRAYS, radius_graph_csr(t["pos"], t["cell"], t["atom_ptr"], radius, max_neighbors)))
        edge_ptr = new["edge_ptr"].cpu().numpy()                # ShardLoader balances ranks by it
        return self._derived(new, self.atom_ptr, edge_ptr, graph_record(radius, max_neighbors))

    def without_hydrogens(self) -> "DeviceShard":
        """The same crystals without their hydrogen atoms, as a new resident shard (this one is untouched): what the
        reference's ``DatasetADP(hydrogens=False)`` does per crystal and per access on the host
        (dataset/datasetADP.py:49-72; ``cartnet_amd.data.remove_hydrogens`` states the rule in torch), done once for the
        whole shard by a stable compaction on the GPU (csrc/shard_ops.hip).  ``y``, ``y_ptr``, ``cell`` and
        ``temperature`` are shared with this shard.  Raises ``ValueError`` if a stored ``non_h_mask`` disagrees with
        ``z != 1``: the rows of a per-atom ``y`` would no longer line up with the kept atoms."""
        self._need_graph("without_hydrogens")
        dev, t, G = self.device, self.t, self.num_graphs
        N, E = int(self.atom_ptr[-1]), int(self.edge_ptr[-1])
        with torch.cuda.device(dev):
            ws_bytes = int(self._lib.cartnet_shard_drop_h_workspace_bytes(N, E))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            atom_ptr = torch.empty(G + 1, dtype=torch.int64, device=dev)
            edge_ptr = torch.empty(G + 1, dtype=torch.int64, device=dev)
            totals = torch.empty(3, dtype=torch.int64, device=dev)
            _l.check(self._lib.cartnet_shard_drop_h_count(_l.C.byref(self._desc), G, N, E, ws.data_ptr(), ws_bytes,
                                                          atom_ptr.data_ptr(), totals.data_ptr(), _l.stream_ptr()),
                     "cartnet_shard_drop_h_count")
            n_out, e_out, status = totals.tolist()              # the one device-to-host copy: sizes of the new arrays
            if status == 1:
                raise ValueError("the shard's non_h_mask disagrees with z != 1: its per-atom targets would not match the "
                                 "atoms that remain")
            if status != 0:
                raise ValueError("the shard has an edge whose end lies outside its crystal")
            new: Dict[str, torch.Tensor] = {"atom_ptr": atom_ptr, "edge_ptr": edge_ptr,
                                            "z": torch.empty(n_out, dtype=torch.int32, device=dev),
                                            "edge_src": torch.empty(e_out, dtype=torch.int32, device=dev),
                                            "edge_tgt": torch.empty(e_out, dtype=torch.int32, device=dev),
                                            "cart_dist": torch.empty(e_out, dtype=torch.float32, device=dev),
                                            "cart_dir": torch.empty((e_out, 3), dtype=torch.float32, device=dev)}
            if "pos" in t:
                new["pos"] = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
            if "non_h_mask" in t:
                new["non_h_mask"] = torch.empty(n_out, dtype=torch.uint8, device=dev)
            _l.check(self._lib.cartnet_shard_drop_h_fill(
                _l.C.byref(self._desc), G, N, E, ws.data_ptr(), ws_bytes, atom_ptr.data_ptr(), n_out, e_out,
                new["z"].data_ptr(), _l.ptr(new.get("pos")), _l.ptr(new.get("non_h_mask")), edge_ptr.data_ptr(),
                new["edge_src"].data_ptr(), new["edge_tgt"].data_ptr(), new["cart_dist"].data_ptr(),
                new["cart_dir"].data_ptr(), _l.stream_ptr()), "cartnet_shard_drop_h_fill")
            ptrs = torch.stack((atom_ptr, edge_ptr)).cpu().numpy()      # ShardLoader balances ranks by these
        return self._derived(new, ptrs[0].copy(), ptrs[1].copy(), self.graph)

    def with_optimized_cell(self) -> "DeviceShard":
        """The same crystals, each in the frame of its canonical reduced lattice, as a new resident shard (this one is
        untouched): what the reference's ``DatasetADP(optimize_cell=True)`` does per crystal and per access on the host
        for iComformer (dataset/datasetADP.py:75-80, dataset/utils.py:366-452; ``cartnet_amd.data.optimize_cell`` states
        the rule in torch), done once for the whole shard on the GPU (csrc/lattice_ops.hip).  The new shard owns ``cell``,
        ``cart_dir`` and, for per-atom 3x3 targets, ``y``; every other array is shared.  It also carries ``rotation``
        [G,9] fp32 (R per crystal) and ``basis`` [G,9] int8 (the signed integer coefficients of the three chosen vectors in
        the rows of the old cell).  Composes with ``without_hydrogens()`` in either order.  Raises ``ValueError`` naming
        the first crystal whose cell is degenerate (no three independent vectors among the candidates).  An unlabeled shard
        has no ``y`` to rotate and gets the other four arrays: predictions made in this frame go back to the stored one as
        ``R P R^T`` (``frame_view``, ``metrics.stored_frame``)."""
        self._need_graph("with_optimized_cell")
        dev, t, G = self.device, self.t, self.num_graphs
        if "cell" not in t:
            raise ValueError("the shard carries no cell")
        E, M = int(self.edge_ptr[-1]), int(self.y_ptr[-1]) if self._labeled else 0     # unlabeled: no targets to rotate
        with torch.cuda.device(dev):
            new: Dict[str, torch.Tensor] = {"cell": torch.empty((G, 9), dtype=torch.float32, device=dev),
                                            "rotation": torch.empty((G, 9), dtype=torch.float32, device=dev),
                                            "basis": torch.empty((G, 9), dtype=torch.int8, device=dev),
                                            "cart_dir": torch.empty((E, 3), dtype=torch.float32, device=dev)}
            if self.per_atom_target and self._labeled:
                new["y"] = torch.empty((M, 9), dtype=torch.float32, device=dev)
            status = torch.empty(G, dtype=torch.int32, device=dev)
            first_bad = torch.empty(1, dtype=torch.int64, device=dev)
            _l.check(self._lib.cartnet_shard_optimize_cell_select(
                t["cell"].data_ptr(), G, new["cell"].data_ptr(), new["rotation"].data_ptr(), new["basis"].data_ptr(),
                status.data_ptr(), first_bad.data_ptr(), _l.stream_ptr()), "cartnet_shard_optimize_cell_select")
            _l.check(self._lib.cartnet_shard_optimize_cell_rotate(
                _l.C.byref(self._desc), G, E, M, new["rotation"].data_ptr(), new["cart_dir"].data_ptr(),
                _l.ptr(new.get("y")), _l.stream_ptr()), "cartnet_shard_optimize_cell_rotate")
            bad = int(first_bad.item())                         # the one device-to-host copy
        if bad >= 0:
            raise ValueError(f"crystal {bad}: degenerate cell: no three linearly independent lattice vectors among the "
                             "candidates")
        return self._derived(new, self.atom_ptr, self.edge_ptr, self.graph)

    def collate(self, sel: Sequence[int], rot: Optional[torch.Tensor] = None, temp_mean: float = 0.0,
                temp_std: float = 1.0) -> Batch:
        """Batch of crystals ``sel`` (in that order) with PyG's collation rules (cartnet_amd/data.py), on the GPU.
        ``rot`` [B,3,3] fp32 (device): per-crystal augmentation rotation (dataset/datasetADP.py:33-39)."""
        self._need_graph("collate")
        sel_np = np.asarray(sel, dtype=np.int64).reshape(-1)
        B = int(sel_np.shape[0])
        if B == 0:
            raise ValueError("cannot collate an empty selection")
        if int(sel_np.min()) < 0 or int(sel_np.max()) >= self.num_graphs:
            raise IndexError("crystal index out of range")
        meta = np.empty(4 * B + 3, dtype=np.int64)                 # [sel | atom offsets | edge offsets | target offsets]
        meta[:B] = sel_np
        for j, p in enumerate((self.atom_ptr, self.edge_ptr, self.y_ptr)):
            seg = meta[B + j * (B + 1):B + (j + 1) * (B + 1)]
            seg[0] = 0
            np.cumsum(p[sel_np + 1] - p[sel_np], out=seg[1:])
        N, E, M = (int(meta[B + j * (B + 1) + B]) for j in range(3))
        M_copy = M if self._labeled else 0                         # unlabeled: the kernel copies no targets
        dev = self.device
        meta_d = torch.from_numpy(meta).pin_memory().to(dev, non_blocking=True)
        if rot is not None:
            if not (rot.is_cuda and rot.dtype == torch.float32 and tuple(rot.shape) == (B, 3, 3)):
                raise ValueError("rot must be a CUDA fp32 tensor [B,3,3]")
            rot = rot.contiguous()
        b = Batch()
        b.x = torch.empty(N, dtype=torch.int64, device=dev)
        b.batch = torch.empty(N, dtype=torch.int64, device=dev)
        b.ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
        b.edge_index = torch.empty((2, E), dtype=torch.int64, device=dev)
        b.cart_dist = torch.empty(E, dtype=torch.float32, device=dev)
        b.cart_dir = torch.empty((E, 3), dtype=torch.float32, device=dev)
        if self._labeled:
            b.y = torch.empty((M, 3, 3) if self.per_atom_target else ((M,) if self.y_width == 1 else (M, self.y_width)),
                              dtype=torch.float32, device=dev)
        else:                                 # the models size their output by y.shape[0]; nothing reads the values
            b.y = torch.zeros((M, 3, 3), dtype=torch.float32, device=dev)
        if "pos" in self.t:
            b.pos = torch.empty((N, 3), dtype=torch.float32, device=dev)
        if "non_h_mask" in self.t:
            b.non_H_mask = torch.empty(N, dtype=torch.bool, device=dev)
        if "cell" in self.t:
            b.cell = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
        if "temperature" in self.t:
            b.temperature = torch.empty(B, dtype=torch.float32, device=dev)
        o = _l.Collated()
        o.x, o.batch, o.ptr = b.x.data_ptr(), b.batch.data_ptr(), b.ptr.data_ptr()
        o.edge_index, o.cart_dist, o.cart_dir = b.edge_index.data_ptr(), b.cart_dist.data_ptr(), b.cart_dir.data_ptr()
        o.y = b.y.data_ptr()
        o.pos = b.pos.data_ptr() if "pos" in self.t else None
        o.non_h_mask = b.non_H_mask.data_ptr() if "non_h_mask" in self.t else None
        o.cell = b.cell.data_ptr() if "cell" in self.t else None
        o.temperature = b.temperature.data_ptr() if "temperature" in self.t else None
        base = meta_d.data_ptr()
        _l.check(self._lib.cartnet_collate(_l.C.byref(self._desc), base, base + 8 * B, base + 8 * (2 * B + 1),
                                           base + 8 * (3 * B + 2), B, N, E, M_copy,
                                           rot.data_ptr() if rot is not None else None, float(temp_mean),
                                           float(temp_std), _l.C.byref(o), _l.stream_ptr()), "cartnet_collate")
        b.num_graphs = B
        b._sel = sel_np                       # the crystals of the batch, on the host
        b._meta = meta_d                      # keeps the offsets alive until the kernel has run
        b._offsets = meta[B:]                 # the three offset arrays on the host: frame_view compares counts with them
        return b

    def frame_view(self, batch: Batch) -> Batch:
        """The model's view of ``batch``, which another shard of the same crystals has collated (the stored frame), in this
        shard's frame (``with_optimized_cell()`` of that shard: the reduced cell): a shallow copy of ``batch`` whose
        ``cart_dir`` and ``cell`` are gathered from this shard by one launch (``cartnet_collate_frame_view``: bit for bit
        those of ``self.collate(batch._sel)``) and which also carries ``rotation`` [B,3,3] (R per crystal: a prediction P
        made on the view is ``R P R^T`` in the stored frame, ``metrics.stored_frame``).  Every other tensor is shared and
        ``batch`` is not modified.  Raises ``ValueError`` unless this shard holds the batch's crystals, each with the atom
        and edge count it has in the batch."""
        self._need_graph("frame_view")
        if "rotation" not in self.t or "cell" not in self.t:
            raise ValueError("frame_view: this shard carries no rotation (it is no with_optimized_cell() shard)")
        sel_np, offsets = getattr(batch, "_sel", None), getattr(batch, "_offsets", None)
        if sel_np is None or offsets is None:
            raise ValueError("frame_view: the batch was not collated from a resident shard")
        B = int(sel_np.shape[0])
        if B == 0:
            raise ValueError("frame_view: the batch holds no crystal")
        if B != int(batch.num_graphs) or int(sel_np.min()) < 0 or int(sel_np.max()) >= self.num_graphs:
            raise ValueError("frame_view: the batch's crystals are not crystals of this shard")
        meta = np.empty(2 * B + 1, dtype=np.int64)                 # [sel | edge offsets in THIS shard]
        meta[:B] = sel_np
        meta[B] = 0
        np.cumsum(self.edge_ptr[sel_np + 1] - self.edge_ptr[sel_np], out=meta[B + 1:])
        E = int(meta[2 * B])
        atoms = self.atom_ptr[sel_np + 1] - self.atom_ptr[sel_np]
        if (offsets.shape[0] != 3 * (B + 1) or not np.array_equal(np.diff(offsets[:B + 1]), atoms)
                or not np.array_equal(offsets[B + 1:2 * B + 2], meta[B:])
                or E != int(batch.edge_index.shape[1]) or int(atoms.sum()) != int(batch.batch.shape[0])):
            raise ValueError("frame_view: a crystal of this shard has another atom or edge count than the batch's (the two "
                             "shards must hold the same graph)")
        dev = self.device
        meta_d = torch.from_numpy(meta).pin_memory().to(dev, non_blocking=True)
        view = batch.__class__()
        view.__dict__.update(batch.__dict__)
        view.cart_dir = torch.empty((E, 3), dtype=torch.float32, device=dev)
        view.cell = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
        base = meta_d.data_ptr()
        with torch.cuda.device(dev):
            _l.check(self._lib.cartnet_collate_frame_view(_l.C.byref(self._desc), base, base + 8 * B, B, E,
                                                          view.cart_dir.data_ptr(), view.cell.data_ptr(), _l.stream_ptr()),
                     "cartnet_collate_frame_view")
            view.rotation = self.t["rotation"][meta_d[:B]].view(B, 3, 3)
        view._view_meta = meta_d              # keeps the offsets alive until the kernel has run
        return view


def random_rotations(n: int, gen: torch.Generator, device) -> torch.Tensor:
    """[n,3,3] uniform rotations from unit quaternions, generated on the device (stands in for
    roma.utils.random_rotmat, dataset/datasetADP.py:34)."""
    q = torch.randn(n, 4, generator=gen, device=device, dtype=torch.float32)
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=1)
    return R.view(n, 3, 3).contiguous()


class ShardLoader:
    """Loader over a resident shard with the interface of cartnet_amd.data.DataLoader: seeded shuffling, ``rank`` /
    ``world_size`` crystal sharding (every rank walks the same permutation and takes a disjoint edge-balanced slice), optional
    SO(3) augmentation.  Batches are born on the GPU; the host only draws the permutation."""

    def __init__(self, shard: DeviceShard, batch_size: int, shuffle: bool = False, seed: int = 0, rank: int = 0,
                 world_size: int = 1, drop_last: bool = False, augment: bool = False, temp_mean: float = 0.0,
                 temp_std: float = 1.0, indices: Optional[Sequence[int]] = None):
        self.shard, self.batch_size, self.shuffle, self.seed = shard, int(batch_size), shuffle, seed
        self.rank, self.world_size, self.drop_last, self.augment = rank, world_size, drop_last, augment
        if augment and not shard.labeled:
            raise ValueError("augment=True on an unlabeled shard: there are no targets to rotate")
        self.temp_mean, self.temp_std = temp_mean, temp_std
        self.indices = list(range(shard.num_graphs)) if indices is None else list(indices)
        self.epoch = 0
        self._gen = torch.Generator(device=shard.device).manual_seed(seed + 7919 * rank)

    def _batches(self) -> List[List[int]]:
        """Crystal ids of this rank's batches for the current epoch (same rule as cartnet_amd.data.DataLoader: one
        rank -> consecutive chunks of the permutation; several -> edge-balanced contiguous slices, nothing dropped,
        equally many batches per rank; edge counts come from the shard's host copy of ``edge_ptr``)."""
        n = len(self.indices)
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            order = [self.indices[i] for i in torch.randperm(n, generator=g).tolist()]
        else:
            order = list(self.indices)
        if self.world_size > 1:
            from .distributed import rank_batches
            ep = self.shard.edge_ptr
            weights = [int(ep[j + 1] - ep[j]) for j in order]
            return [[order[i] for i in r] for r in rank_batches(weights, self.batch_size, self.rank, self.world_size)]
        chunks = [order[i:i + self.batch_size] for i in range(0, len(order), self.batch_size)]
        if self.drop_last and chunks and len(chunks[-1]) < self.batch_size:
            chunks.pop()
        return chunks

    def __len__(self) -> int:
        return len(self._batches())

    def __iter__(self) -> Iterable[Batch]:
        batches = self._batches()
        self.epoch += 1
        for chunk in batches:
            if not chunk:
                yield None
                continue
            rot = random_rotations(len(chunk), self._gen, self.shard.device) if self.augment else None
            yield self.shard.collate(chunk, rot, self.temp_mean, self.temp_std)

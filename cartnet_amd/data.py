"""Minimal ``Data`` / ``Batch`` containers with PyG's collation rules for the attributes CartNet reads.

The reference consumes ``torch_geometric.data.Batch`` objects produced by PyG's ``DataLoader``
(reference: train/train.py:167-171).  torch_geometric is not installed on the
target image, so this module restates the collation contract for exactly the attribute set on the hot path:

  * node-level tensors (``x``, ``non_H_mask``, ``pos``, ``y`` when per-atom) are concatenated on dim 0;
  * ``edge_index`` [2, E_g] is concatenated on dim 1 after adding the cumulative node offset of each graph;
  * edge-level tensors (``cart_dist``, ``cart_dir``) are concatenated on dim 0;
  * per-graph tensors (``temperature`` [1], ``cell`` [1,3,3], scalar ``y``) are concatenated on dim 0;
  * ``batch`` [N] (sorted graph id per node) and ``ptr`` [Bg+1] are added.
"""
from __future__ import annotations

import math
from typing import Iterable, List, Sequence

import torch

_NODE_KEYS = {"x", "non_H_mask", "pos"}
_EDGE_KEYS = {"cart_dist", "cart_dir"}
_GRAPH_KEYS = {"temperature", "cell", "natoms"}


class Data:
    """Attribute bag of tensors describing one crystal graph (or a collated batch of them)."""

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def keys(self) -> List[str]:
        return [k for k, v in self.__dict__.items() if not k.startswith("_")]

    def to(self, device, non_blocking: bool = False):
        """In-place move of every tensor attribute; returns self (PyG semantics, train/train.py:169)."""
        for k, v in list(self.__dict__.items()):
            if torch.is_tensor(v):
                setattr(self, k, v.to(device, non_blocking=non_blocking))
        return self

    def clone(self):
        out = self.__class__()
        for k, v in self.__dict__.items():
            setattr(out, k, v.clone() if torch.is_tensor(v) else v)
        return out

    @property
    def num_nodes(self) -> int:
        return int(self.x.shape[0])

    @property
    def num_edges(self) -> int:
        return int(self.edge_index.shape[1])

    def __repr__(self):
        parts = []
        for k in self.keys():
            v = getattr(self, k)
            parts.append(f"{k}={list(v.shape)}" if torch.is_tensor(v) else f"{k}={v!r}")
        return f"{self.__class__.__name__}({', '.join(parts)})"


def remove_hydrogens(data: Data) -> Data:
    """The crystal without its hydrogen atoms: the reference's ``DatasetADP.get`` with ``hydrogens=False``
    (dataset/datasetADP.py:49-72), as a new ``Data`` (the input is not modified).

      * ``x`` / ``pos`` (and ``natoms``) of the atoms with ``x != 1``;
      * an edge stays if its source and its target stay, in the original order, so ``edge_index[1]`` is still sorted;
        ``edge_index`` is renumbered to each atom's rank among the survivors; ``cart_dir`` / ``cart_dist`` follow;
      * ``y``, ``cell``, ``temperature`` as they are (per-atom targets exist for non-hydrogen atoms only);
      * ``non_H_mask`` (if the crystal carries one) all ones.

    A crystal that keeps no edge gets ``edge_index`` of shape [2, 0] int64; the reference builds it from an empty
    Python list there, ``torch.tensor([]).t()``: a float tensor of shape [0].  ``DeviceShard.without_hydrogens`` does
    the same to a whole resident shard on the GPU."""
    keep = data.x != 1
    if hasattr(data, "non_H_mask") and not torch.equal(data.non_H_mask.to(torch.bool), keep):
        raise ValueError("non_H_mask disagrees with x != 1: the per-atom targets would not match the atoms that remain")
    new_id = torch.cumsum(keep.to(torch.int64), 0) - 1                   # rank among the survivors
    src, tgt = data.edge_index[0], data.edge_index[1]
    keep_e = keep[src] & keep[tgt]
    out = data.__class__()
    for k, v in data.__dict__.items():
        setattr(out, k, v)
    out.x = data.x[keep]
    if hasattr(data, "pos"):
        out.pos = data.pos[keep]
    if hasattr(data, "natoms"):
        out.natoms = torch.tensor([int(out.x.shape[0])], dtype=data.natoms.dtype)
    out.edge_index = torch.stack((new_id[src[keep_e]], new_id[tgt[keep_e]])).to(torch.int64).reshape(2, -1)
    out.cart_dir = data.cart_dir[keep_e]
    out.cart_dist = data.cart_dist[keep_e]
    if hasattr(data, "non_H_mask"):
        out.non_H_mask = torch.ones(out.x.shape[0], dtype=torch.bool)
    return out


# enumeration of the reference's expand_lattice (dataset/utils.py:400-408): i, j, k in -2..2 with k fastest, (0,0,0) skipped
_LATTICE_COEFFS = torch.tensor([(i, j, k) for i in range(-2, 3) for j in range(-2, 3) for k in range(-2, 3)
                                if (i, j, k) != (0, 0, 0)], dtype=torch.int64)


def _lattice_candidates(cell: torch.Tensor) -> torch.Tensor:
    """The 124 vectors i c0 + j c1 + k c2, evaluated as the reference does: ((i c0) + (j c1)) + (k c2)."""
    c = _LATTICE_COEFFS.to(cell.dtype)
    return (c[:, 0:1] * cell[0] + c[:, 1:2] * cell[1]) + c[:, 2:3] * cell[2]


def _select_lattice(cand: torch.Tensor, half_pi: float):
    """Ranks (positions in the (norm, enumeration index) order) and signs of the three vectors the reference's
    ``optmize_lattice`` picks (dataset/utils.py:425-449, before the handedness step), or None for a degenerate cell."""
    order = torch.sort(torch.norm(cand, dim=1), stable=True).indices      # ties: the lower enumeration index first
    v = cand[order]
    v1 = v[0]

    def sign(w):                                                          # vector_angle(v1, w) > pi / 2
        cos = torch.dot(v1, w) / (torch.norm(v1) * torch.norm(w))
        return -1 if bool(torch.abs(torch.acos(cos)) > half_pi) else 1
    r2 = next((r for r in range(1, v.shape[0])
               if not bool(torch.norm(torch.linalg.cross(v1, v[r])) <= 1e-3)), None)
    if r2 is None:
        return None
    s2 = sign(v[r2])
    n12 = torch.linalg.cross(v1, s2 * v[r2])
    # the reference restarts one element early (closest_vectors[i:], i = r2 - 1): that element was rejected as collinear
    # with v1 or is v1 itself, and v2 lies in its own plane with v1, so both are rejected again and the search in effect
    # starts after v2
    r3 = next((r for r in range(r2 + 1, v.shape[0]) if not bool(torch.abs(torch.dot(n12, v[r])) <= 1e-3)), None)
    if r3 is None:
        return None
    return order, (0, r2, r3), (1, s2, sign(v[r3]))


def lattice_basis(cell: torch.Tensor) -> torch.Tensor:
    """[3,3] int64: row r holds the signed integer coefficients, in the rows of ``cell`` [3,3] fp32, of the r-th vector of
    the canonical reduced lattice (the reference's ``optmize_lattice``, dataset/utils.py:420-449, handedness included).

    Candidates are ordered by (Euclidean norm, enumeration index).  The reference's ``argsort`` is not stable, so its
    order inside a +v / -v pair is an accident of the sort; for a generic cell the final lattice is the same, because a
    flipped v1 flips v2 and v3 with it (their sign is taken against v1) and the handedness step undoes the overall sign.
    Raises ``ValueError`` for a cell with no admissible second or third vector."""
    cell = cell.to(torch.float32).reshape(3, 3)
    cand = _lattice_candidates(cell)
    # the reference compares an fp32 angle with the Python float pi / 2: the comparison runs in fp32, where acos(0) equals
    # fp32(pi / 2), so exactly orthogonal vectors are not negated
    sel = _select_lattice(cand, float(torch.tensor(math.pi / 2, dtype=torch.float32)))
    if sel is None:
        raise ValueError("degenerate cell: no three linearly independent lattice vectors among the candidates")
    order, ranks, signs = sel
    idx = order[list(ranks)]
    basis = _LATTICE_COEFFS[idx] * torch.tensor(signs).unsqueeze(1)
    v = cand[idx] * torch.tensor(signs, dtype=cand.dtype).unsqueeze(1)
    if bool(torch.dot(torch.linalg.cross(v[0], v[1]), v[2]) < 0):        # find_right_hand_system, dataset/utils.py:414-418
        basis = -basis
    return basis


def lattice_frame(vectors: torch.Tensor):
    """(new_cell, R) of three lattice vectors [3,3] (rows), the reference's ``rotate_crystal_to_lattice``
    (dataset/utils.py:366-398): the rows of R are x = v1 / |v1|, y = the normalised part of v2 orthogonal to x and
    z = x cross y; ``new_cell = vectors @ R^T`` is lower-triangular with a positive diagonal."""
    x = vectors[0] / torch.linalg.norm(vectors[0])
    p = vectors[1] - torch.dot(vectors[1], x) * x
    y = p / torch.linalg.norm(p)
    R = torch.stack([x, y, torch.linalg.cross(x, y)])
    return vectors @ R.T, R


def optimize_lattice(cell: torch.Tensor):
    """``(new_cell, R)`` of a cell [3,3] fp32 (rows are lattice vectors): the reference's ``optmize_lattice``
    (dataset/utils.py:420-452) on the CPU.  ``new_cell`` describes the same lattice by its three shortest independent
    vectors (see ``lattice_basis``), rotated by ``R`` into the frame of ``lattice_frame``."""
    cell = cell.to(torch.float32).reshape(3, 3)
    cand = _lattice_candidates(cell)
    b = lattice_basis(cell)
    idx = ((b[:, 0] + 2) * 25 + (b[:, 1] + 2) * 5 + (b[:, 2] + 2))
    idx = idx - (idx > 62).to(idx.dtype)                                  # (0,0,0) is not enumerated
    return lattice_frame(cand[idx])


def lattice_margins(cell: torch.Tensor):
    """How far the selection of ``lattice_basis`` is from a tie, in fp64: ``(gap, cos)``.  ``gap`` is the smallest
    relative difference between the norms of consecutive candidates, up to the one after the third chosen vector, that
    are not each other's negative; ``cos`` is the smaller |cos| of the angle between the first chosen vector and the
    other two.  Where both exceed fp32 rounding by a wide margin, every fp32 evaluation of the rule picks the same basis.
    (0, 0) for a degenerate cell."""
    cand = _lattice_candidates(cell.to(torch.float64).reshape(3, 3))
    sel = _select_lattice(cand, math.pi / 2)
    if sel is None:
        return 0.0, 0.0
    order, ranks, _ = sel
    norms = torch.norm(cand, dim=1)[order]
    coeff = _LATTICE_COEFFS[order]
    gap = float("inf")
    for r in range(min(ranks[2] + 1, norms.shape[0] - 1)):
        if bool((coeff[r] == -coeff[r + 1]).all()):
            continue
        gap = min(gap, float((norms[r + 1] - norms[r]) / norms[r + 1]))
    v = cand[order[list(ranks)]]
    cos = min(abs(float(torch.dot(v[0], v[j]) / (norms[0] * torch.norm(v[j])))) for j in (1, 2))
    return gap, cos


def optimize_cell(data: Data, name=None) -> Data:
    """The crystal in the frame of its canonical reduced lattice: the reference's ``DatasetADP.get`` with
    ``optimize_cell=True`` (dataset/datasetADP.py:75-80), as a new ``Data`` (the input is not modified).

      * ``cell`` <- the reduced lattice of ``optimize_lattice`` ([1,3,3]), ``cell_og`` <- the cell as it was;
      * ``cart_dir`` <- ``cart_dir @ R`` and, for per-atom 3x3 targets, ``y`` <- ``R^T y R``.

    The lattice is multiplied by ``R^T`` and the directions by ``R``: that is what the reference does, reproduced as it is
    (DESIGN.md section 3).  ``DeviceShard.with_optimized_cell`` does the same to a whole resident shard on the GPU.
    Raises ``ValueError`` naming the crystal (``name``, else its ``refcode`` if it has one) for a degenerate cell."""
    try:
        new_cell, R = optimize_lattice(data.cell.reshape(3, 3))
    except ValueError as e:
        who = name if name is not None else getattr(data, "refcode", "?")
        raise ValueError(f"crystal {who}: {e}") from None
    out = data.__class__()
    for k, v in data.__dict__.items():
        setattr(out, k, v)
    out.cell_og = data.cell
    out.cell = new_cell.unsqueeze(0)
    out.cart_dir = data.cart_dir @ R
    if data.y.dim() == 3 and tuple(data.y.shape[1:]) == (3, 3):
        out.y = R.transpose(-1, -2) @ data.y @ R
    return out


class Batch(Data):
    """A collated batch of graphs.  ``num_graphs`` is kept on the host so no device sync is needed."""

    @classmethod
    def from_data_list(cls, data_list: Sequence[Data]) -> "Batch":
        if len(data_list) == 0:
            raise ValueError("cannot collate an empty list of graphs")
        out = cls()
        keys = data_list[0].keys()
        n_nodes = [d.num_nodes for d in data_list]
        offsets = [0]
        for n in n_nodes:
            offsets.append(offsets[-1] + n)
        for k in keys:
            vals = [getattr(d, k) for d in data_list]
            if not torch.is_tensor(vals[0]):
                setattr(out, k, vals)
                continue
            if k == "edge_index":
                setattr(out, k, torch.cat([v + off for v, off in zip(vals, offsets[:-1])], dim=1))
            elif k == "y":
                # per-atom targets [M_g,3,3] or per-graph scalars ([] or [1]) -- both concatenate on dim 0
                vals = [v.reshape(1) if v.dim() == 0 else v for v in vals]
                setattr(out, k, torch.cat(vals, dim=0))
            else:
                vals = [v.reshape(1) if v.dim() == 0 else v for v in vals]
                setattr(out, k, torch.cat(vals, dim=0))
        out.batch = torch.repeat_interleave(
            torch.arange(len(data_list), dtype=torch.int64), torch.tensor(n_nodes, dtype=torch.int64)
        )
        out.ptr = torch.tensor(offsets, dtype=torch.int64)
        out.num_graphs = len(data_list)
        return out


class DataLoader:
    """Tiny single-process loader: shuffles graph indices with a seeded generator and collates ``batch_size``
    graphs at a time (stand-in for ``torch_geometric.loader.DataLoader``; reference: loader/loader.py:114-124).

    ``rank`` / ``world_size`` give the batched-graph sharding mode: every rank walks the same permutation and
    takes a contiguous, disjoint, edge-balanced slice of it (no crystal is dropped), so crystals are partitioned
    across GPUs with no data-path collective.
    """

    def __init__(self, dataset: Sequence[Data], batch_size: int, shuffle: bool = False, seed: int = 0,
                 rank: int = 0, world_size: int = 1, drop_last: bool = False, transform=None):
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self.seed = seed
        self.rank = rank
        self.world_size = world_size
        self.drop_last = drop_last
        self.transform = transform
        self.epoch = 0

    def _order(self) -> List[int]:
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            return torch.randperm(n, generator=g).tolist()
        return list(range(n))

    def _batches(self) -> List[List[int]]:
        """Crystal indices of this rank's batches for the current epoch.  One rank: consecutive chunks of
        ``batch_size`` (PyG's DataLoader).  Several ranks: cartnet_amd.distributed.rank_batches -- contiguous
        EDGE-balanced slices of the common permutation, nothing dropped, the same number of batches on every rank."""
        order = self._order()
        if self.world_size > 1:
            from .distributed import rank_batches
            weights = [int(self.dataset[j].edge_index.shape[1]) for j in order]
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
            if not chunk:                 # fewer crystals than steps on this rank: a step with a zero gradient
                yield None
                continue
            items = [self.dataset[j] for j in chunk]
            if self.transform is not None:
                items = [self.transform(d.clone()) for d in items]
            yield Batch.from_data_list(items)

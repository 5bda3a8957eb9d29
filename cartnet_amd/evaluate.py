"""The evaluation passes of ``main.py`` on a trained checkpoint: ``--inference`` (reference main.py:21-60) and
``--montecarlo`` (main.py:62-119), one loop each for every ``--eval_batch``.

``inference`` runs one forward and one ``adp_eval`` per batch, whatever its size, and cuts what comes back into one
pickle entry per crystal: at batch size 1 that is the reference's loop bit for bit (``adp_eval`` is the metrics kernel
and ``(pred - true).abs()``, and one packed copy holds the bits of the reference's separate ones;
tests/test_gpu_eval_batch.py::test_inference_at_batch_1_is_the_reference_loop).  ``montecarlo`` has two steps per
batch: ``montecarlo_reference``, the reference's statements, for a loader of batch size 1, and ``montecarlo_batch`` (one
rotation per crystal by ``rotate_rows`` and ``adp_eval(rot=)``) for any other.  Both passes keep the pickle layout of
batch size 1 (``batch_entries``) and the reference's result keys (``summary``)."""
from __future__ import annotations

import pickle

import torch

from .metrics import (adp_eval, batch_graph, bond_test, compute_3D_IoU, edge_row_ptr, get_similarity_index, molecule_test,
                      molecules, rotate_rows, split_rows, target_row_ptr, tls_fit as tls_fit_call, to_host)
from .predict import STATISTICS, TLS_KEYS, Analyses, frame_stage, tls_entries
from .shard import random_rotations

# the keys of the two pickles in the order the reference's loops create them (a Monte-Carlo round stores no temperature)
INFERENCE_KEYS = ("pred", "true", "temp", "cell", "refcode", "pos", "atoms", "iou", "mae", "similarity_index")
MONTECARLO_KEYS = ("pred", "true", "cell", "refcode", "pos", "atoms", "mae", "iou", "similarity_index")
# what --inference --rigid_molecule adds to its pickle: the molecules, then the test of the prediction and of the truth
MOLECULE_KEYS = ("mol", "mol_size", "mol_status", "mol_pairs", "mol_delta_max", "mol_over", "mol_pairs_true",
                 "mol_delta_max_true", "mol_over_true")
# what --inference --tls_fit adds on top of that: predict.TLS_KEYS but the per-crystal figures, for the prediction and,
# with the suffix _true, for the truth
TLS_ROW_KEYS = tuple(k for k in TLS_KEYS if k != "tls_stats")


def summary(iou: torch.Tensor, mae: torch.Tensor, sim: torch.Tensor) -> dict:
    """Mean and standard deviation over all atoms of a pass (main.py:52-60, 112-119)."""
    return {"iou_mean": float(iou.mean()), "iou_std": float(iou.std()), "mae_mean": float(mae.mean()),
            "mae_std": float(mae.std()), "similarity_index_mean": float(sim.mean()),
            "similarity_index_std": float(sim.std())}


def flush_graph_checks(model) -> None:
    """End of a pass: the models that defer their checks of the batches' graphs raise now what they found."""
    if hasattr(model, "flush_graph_checks"):
        model.flush_graph_checks()


def batch_entries(out: dict, batch, row_ptr, per_row: dict, with_pos: bool) -> None:
    """Appends one list entry per crystal to ``out``: the tensors of ``per_row`` (dim 0 runs over the batch's non-hydrogen
    atoms, in crystal order), ``cell``, ``atoms`` and, if asked for, ``pos``.  One transfer brings everything to the host,
    the crystals' row counts included; the split by those counts happens there -- the lists the reference's loop writes
    (main.py:38-49).  ``batch.x`` must hold the atomic numbers."""
    dev = dict(per_row)
    dev["atoms"] = batch.x[batch.non_H_mask]
    dev["cell"] = batch.cell
    if with_pos and hasattr(batch, "pos"):
        dev["pos"] = batch.pos[batch.non_H_mask]
    dev["_row_ptr"] = row_ptr
    host = to_host(dev)
    rp = host.pop("_row_ptr")
    rows = (rp[1:] - rp[:-1]).tolist()
    out["cell"] += [c.unsqueeze(0) for c in host.pop("cell").unbind(0)]
    for k, t in host.items():
        out[k] += split_rows(t, rows)


def inference(model, loader, device, output_path: str, rotations: int = 1, seed: int = 0, rigid_bond=None,
              rigid_molecule=None, tls_fit=None) -> dict:
    """main.py:21-60 at any batch size: eval mode, per test batch one forward and one ``adp_eval`` -- the prediction, the
    target and the per-atom IoU / MAE / similarity index -- and everything pickled to ``output_path`` with one list entry
    per crystal (the reference's test loader has batch size 1, loader/loader.py:121).  The crystals carry no refcode /
    original temperature: those two lists stay empty.  ``rotations`` = K > 1: the prediction that is evaluated against the
    truth is the mean over K frames (``predict.frame_stage``; one generator seeded with ``seed`` for the whole pass); the
    pickle then also has ``rot_spread`` per crystal, the result ``rotations`` and ``rot_spread_max``.  The analyses
    (``predict.Analyses``: a ``tls_fit`` without ``rigid_molecule`` is a ``ValueError``) run on the prediction and on the
    truth of every batch, the truth's figures -- suffix ``_true`` -- being the baseline the prediction's are to be
    compared with; the result's figures are those of ``predict.STATISTICS`` over the pass.  ``rigid_bond`` =
    ``(tol, threshold)``: ``metrics.bond_test``; the pickle then also has ``bond_delta_max`` / ``_true`` (one value per
    row), the result ``rigid_bond_mean`` / ``_true``.  ``rigid_molecule`` = ``(tol, threshold)``: the molecules of every
    batch (``metrics.molecules``, found once) and ``metrics.molecule_test``; the pickle then also has ``MOLECULE_KEYS``,
    the result ``molecules``, ``molecules_tested``, ``rigid_molecule_pairs`` and ``rigid_molecule_mean`` / ``_max`` /
    ``_over`` / those three ``_true``.  ``tls_fit`` = ``True``: ``metrics.tls_fit`` on the same molecules; the pickle then
    also has ``TLS_ROW_KEYS`` / ``_true``, the result ``tls_molecules`` and ``tls_rank_deficient``, ``tls_nonphysical``,
    ``tls_r``, ``tls_resid_max`` / those four ``_true``."""
    Analyses(rigid_bond=rigid_bond, rigid_molecule=rigid_molecule, tls_fit=tls_fit).checked()
    model.eval()
    out = {k: [] for k in INFERENCE_KEYS}
    gen = torch.Generator(device=device).manual_seed(seed) if rotations > 1 else None
    if rotations > 1:
        out["rot_spread"] = []
    bond_sums = None                                      # [2,4] fp64 on the device: crystal_stats summed, prediction / truth
    if rigid_bond is not None:
        out["bond_delta_max"], out["bond_delta_max_true"] = [], []
        bond_sums = torch.zeros((2, 4), dtype=torch.float64, device=device)
    mol_counts = mol_sums = mol_max = None                # on the device: crystal_counts summed; crystal_stats, as bond_sums
    if rigid_molecule is not None:
        out.update({k: [] for k in MOLECULE_KEYS})
        mol_counts = torch.zeros(5, dtype=torch.float64, device=device)
        mol_sums = torch.zeros((2, 4), dtype=torch.float64, device=device)
        mol_max = torch.zeros(2, dtype=torch.float64, device=device)
    tls_sums = tls_max = None                             # the same for the TLS fit's crystal_stats
    if tls_fit:
        out.update({k + suffix: [] for suffix in ("", "_true") for k in TLS_ROW_KEYS})
        tls_sums = torch.zeros((2, 5), dtype=torch.float64, device=device)
        tls_max = torch.zeros(2, dtype=torch.float64, device=device)
    with torch.no_grad():
        for batch in loader:
            if batch is None:
                continue
            batch.to(device)
            row_ptr = target_row_ptr(batch)
            true = batch.y
            pred, _, fm = frame_stage(model, batch, row_ptr, rotations, gen, stats=False)
            extra = {} if fm is None else {"rot_spread": fm.spread}
            if rigid_bond is not None or rigid_molecule is not None:          # batch.x holds the atomic numbers again
                graph = batch_graph(batch, int(pred.shape[0]), "inference")   # checked and looked up once per batch
            if rigid_bond is not None:
                for k, (name, u) in enumerate((("bond_delta_max", pred), ("bond_delta_max_true", true))):
                    bt = bond_test(u, graph, row_ptr, *rigid_bond)
                    extra[name] = bt.delta_max
                    bond_sums[k] += bt.crystal_stats.sum(0)
            if rigid_molecule is not None:                                    # found once, tested twice
                mo = molecules(graph, row_ptr, rigid_molecule[0])
                extra.update(mol=mo.mol, mol_size=mo.size, mol_status=mo.status)
                mol_counts += mo.crystal_counts.sum(0)
                for k, (suffix, u) in enumerate((("", pred), ("_true", true))):
                    mt = molecule_test(u, graph, row_ptr, mo, rigid_molecule[1])
                    extra.update({"mol_pairs" + suffix: mt.pairs, "mol_delta_max" + suffix: mt.delta_max,
                                  "mol_over" + suffix: mt.over})
                    mol_sums[k] += mt.crystal_stats.sum(0)
                    mol_max[k] = torch.maximum(mol_max[k], mt.crystal_stats[:, 2].max())
                    if tls_fit:
                        entries = tls_entries(tls_fit_call(u, graph, row_ptr, mo))
                        extra.update({key + suffix: entries[key] for key in TLS_ROW_KEYS})
                        tls_sums[k] += entries["tls_stats"][:, :5].sum(0)
                        tls_max[k] = torch.maximum(tls_max[k], entries["tls_stats"][:, 5].max())
            res = adp_eval(pred, true, row_ptr, None, volume=False)
            batch_entries(out, batch, row_ptr, {"pred": pred, "true": true, "mae": res.abs_err, "iou": res.iou,
                                                "similarity_index": res.similarity_index, **extra}, with_pos=True)
    flush_graph_checks(model)
    iou, mae, sim = (torch.cat(out[k]) for k in ("iou", "mae", "similarity_index"))
    with open(output_path, "wb") as f:
        pickle.dump(out, f)
    result = {**summary(iou, mae, sim), "output": output_path}
    if rotations > 1:
        spread = torch.cat(out["rot_spread"])
        result.update(rotations=rotations, rot_spread_max=float(spread.max()) if spread.numel() else 0.0)
    def figures(key: str, sums: list, highs: list, once: tuple, twice: tuple) -> None:
        """The figures of predict.STATISTICS[key] from the column sums and maxima of the prediction and of the truth
        (0 where none is kept): those of ``once`` for the prediction, those of ``twice`` for both, the truth's as *_true."""
        pred, true = (STATISTICS[key][1](s, hi) for s, hi in zip(sums, highs))
        result.update({k: pred[k] for k in once})
        result.update({k + suffix: f[k] for suffix, f in (("", pred), ("_true", true)) for k in twice})
    if rigid_bond is not None:
        figures("bond_stats", bond_sums.tolist(), [[0.0] * 4] * 2, (), ("rigid_bond_mean",))
    if rigid_molecule is not None:
        counts = mol_counts.tolist()
        figures("mol_stats", [counts + s for s in mol_sums.tolist()], [[0.0] * 7 + [hi, 0.0] for hi in mol_max.tolist()],
                ("molecules", "molecules_tested", "rigid_molecule_pairs"),
                ("rigid_molecule_mean", "rigid_molecule_max", "rigid_molecule_over"))
    if tls_fit:
        figures("tls_stats", [s + [0.0] for s in tls_sums.tolist()], [[0.0] * 5 + [hi] for hi in tls_max.tolist()],
                ("tls_molecules",), ("tls_rank_deficient", "tls_nonphysical", "tls_r", "tls_resid_max"))
    return result


def _clone(batch):
    """A second copy of ``batch`` for the rotated forward: a forward overwrites ``batch.x`` (main.py:87)."""
    copy = batch.clone()
    copy.num_graphs = batch.num_graphs
    return copy


def montecarlo_reference(model, batch, gen: torch.Generator):
    """One Monte-Carlo step as the reference writes it, for its test loader's batch of one crystal (main.py:85-103):
    clone, forward, one rotation R drawn from ``gen``, ``cart_dir @ R`` on the clone (``cell`` is not rotated), the
    pseudo-truth ``R^T pred_1 R``, forward again, and the three metric calls.  Returns ``(per_row, row_ptr)``: what
    ``batch_entries`` takes; ``batch`` comes back with its atomic numbers in ``x``."""
    row_ptr = target_row_ptr(batch)
    batch_copy = _clone(batch)
    atoms = batch.x                                                           # the forward replaces x, it writes into nothing
    pseudo_true, _ = model(batch)
    batch.x = atoms
    R = random_rotations(1, gen, gen.device)[0]
    batch_copy.cart_dir = batch_copy.cart_dir @ R
    pseudo_true = R.transpose(-1, -2) @ pseudo_true @ R
    pred, _ = model(batch_copy)
    return {"pred": pred, "true": pseudo_true, "iou": compute_3D_IoU(pred, pseudo_true),
            "similarity_index": get_similarity_index(pred, pseudo_true), "mae": (pred - pseudo_true).abs()}, row_ptr


def montecarlo_batch(model, batch, R: torch.Tensor):
    """One Monte-Carlo step (main.py:85-103) for a whole batch on the device, crystal g rotated by ``R[g]`` [B,3,3]:
    clone, forward, rotate the clone's ``cart_dir`` per crystal (``cell`` is not rotated, as in the reference), forward
    again, and one ``adp_eval`` that forms the pseudo-truth ``R_g^T pred_1 R_g`` and compares.  Returns
    ``(pred, AdpEval, row_ptr)``; ``batch`` comes back with its atomic numbers in ``x``."""
    row_ptr = target_row_ptr(batch)
    copy = _clone(batch)
    atoms = batch.x.clone()
    first, _ = model(batch)
    batch.x = atoms
    copy.cart_dir = rotate_rows(copy.cart_dir.contiguous(), edge_row_ptr(copy), R)
    pred, _ = model(copy)
    return pred, adp_eval(pred, first, row_ptr, rot=R, volume=False), row_ptr


def montecarlo(model, loader, device, output_path: str, rounds: int = 100, seed: int = 0) -> dict:
    """main.py:62-119 at any batch size: for ``rounds`` passes over the test loader, predict, rotate ``cart_dir`` by a
    uniform random rotation per crystal, predict again and compare with the rotated first prediction (IoU, MAE,
    similarity index): how equivariant the trained network has become.  A loader of batch size 1 takes
    ``montecarlo_reference`` (one draw of 1 rotation per crystal), any other ``montecarlo_batch`` (one draw of B per
    batch).  One pickle per round, as the reference writes them, with one list entry per crystal."""
    model.eval()
    gen = torch.Generator(device=device).manual_seed(seed)
    iou_all, mae_all, sim_all = [], [], []
    with torch.no_grad():
        for i in range(rounds):
            out = {k: [] for k in MONTECARLO_KEYS}
            for batch in loader:
                if batch is None:
                    continue
                batch.to(device)
                if loader.batch_size == 1:
                    per_row, row_ptr = montecarlo_reference(model, batch, gen)
                else:
                    pred, res, row_ptr = montecarlo_batch(model, batch, random_rotations(int(batch.num_graphs), gen, device))
                    per_row = {"pred": pred, "true": res.true, "mae": res.abs_err, "iou": res.iou,
                               "similarity_index": res.similarity_index}
                batch_entries(out, batch, row_ptr, per_row, with_pos=False)     # (main.py:62-119 stores no pos)
            with open(output_path.replace(".pkl", f"_montecarlo_{i}.pkl"), "wb") as f:
                pickle.dump(out, f)
            iou_all += out["iou"]
            mae_all += out["mae"]
            sim_all += out["similarity_index"]
    flush_graph_checks(model)
    iou, mae, sim = torch.cat(iou_all), torch.cat(mae_all), torch.cat(sim_all)
    return {"rounds": rounds, **summary(iou, mae, sim)}

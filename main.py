#!/usr/bin/env python3
"""Entry point with the reference's flag surface and call order (reference: main.py:121-227), on the MI355X path.

What is kept: the argparse flags and their defaults (main.py:123-154), the copy into the global ``cfg``
(:156-188), seed -> loaders -> ``create_model()`` -> Adam -> ``train`` (:196-227), OneCycleLR, gradient accumulation
with the last-iteration flush, best-validation checkpoint ``{"model_state", "optimizer_state"}`` under
``results/<name>/<seed>/ckpt/best.ckpt`` (train/train.py:91-102) and its reload for the test pass (:114-115),
``--inference`` / ``--montecarlo`` on a checkpoint (main.py:21-119, 212-225; the passes are in cartnet_amd/evaluate.py).
This file holds the parser, ``fill_cfg``, the dataset recipe and the loaders, the argument checks and the dispatch.
What differs: the datasets (CSD / Jarvis need licences or the network) are replaced by synthetic ADP-shaped crystals
(``--synthetic N`` graphs, ``--atoms lo hi``), wandb / GraphGym logging are dropped, ``--device`` replaces the hard-coded
"cuda:0", and under ``torch.distributed.run`` the crystals are sharded across ranks with one gradient all-reduce per
optimiser step.  ``--shard_dir DIR`` trains from packed shard files (cartnet_amd/shard.py) instead of synthetic crystals:
the reference's dataset recipe -- graph, hydrogen removal, canonical cell, temperature standardisation -- is applied to the
resident shards in the reference's order.  ``--eval_batch N`` runs the ADP test pass, ``--inference`` and
``--montecarlo`` with N crystals per forward and keeps the results of the reference's test batch size 1 (per-crystal means,
rotations and pickle entries).  ``--predict`` applies a checkpoint to the crystals of ONE shard file, labeled or not
(``--predict_input``), and writes their ADPs in CIF convention (cartnet_amd/predict.py); the input may also be a CIF
file or a directory of them, whose asymmetric units are expanded on the GPU (cartnet_amd/symmetry.py) and get one
site-averaged ADP per atom back.  ``--rotations K`` makes ``--predict`` and ``--inference`` predict every crystal in K
frames (the stored one and K - 1 random rotations), bring the predictions back and report their mean, with the largest
deviation of a frame from it per atom.  ``--rigid_bond`` adds Hirshfeld's rigid-bond test to ``--predict`` and
``--inference``: a plausibility figure per bonded pair of atoms that needs no truth (cartnet_amd/bonds.py,
``metrics.bond_test``).  ``--riding_h`` gives every hydrogen of a ``--predict`` pass an isotropic U by the riding model, a
multiple of its parent's predicted U_eq (``metrics.riding_h``).  ``--predict_temperatures SPEC`` predicts every crystal of a
``--predict`` pass at a series of temperatures in one forward per batch and fits a line per atom through them
(``metrics.temp_series``).  ``--rigid_molecule`` finds the molecules of every crystal of a ``--predict`` or ``--inference``
pass on the GPU and tests the ADPs for rigid-body motion over all pairs of atoms of a molecule (``metrics.molecules``,
``metrics.molecule_test``).  ``--tls_fit`` (with ``--rigid_molecule``) fits the rigid-body tensors T, L and S of
Schomaker & Trueblood to the ADPs of every such molecule (``metrics.tls_fit``).  ``--aniso_h`` (with ``--riding_h``) gives
every hydrogen a full tensor from its parent's, that rigid-body motion and a nominal internal X-H motion
(``metrics.aniso_h``).  ``--bond_table`` lists the bonds of every crystal of a ``--predict`` pass with Hirshfeld's D, the
Busing & Levy bounds on the bond length and, after a TLS fit, the libration-corrected length (``metrics.bond_table``).
``--angle_table`` lists the valence angles and the torsions of the same bond graph, with their values after that
libration (``metrics.angle_table``).
There is no CPU path: the model runs on an AMD GPU only.
"""
from __future__ import annotations

import argparse
import json
import os
import time
from typing import Optional, Tuple

import torch

from cartnet_amd import distributed as cdist
from cartnet_amd import evaluate
from cartnet_amd.bonds import ANISO_H_BEND, ANISO_H_STRETCH, BOND_TOLERANCE, RIDING_FACTOR, RIDING_FACTOR_ROTATING, RIGID_BOND_THRESHOLD
from cartnet_amd.config import cfg, set_cfg
from cartnet_amd.data import DataLoader, optimize_cell, remove_hydrogens
from cartnet_amd.master import create_model
from cartnet_amd.optim import FlatAdam, one_cycle_lr, one_cycle_momentum
from cartnet_amd.predict import parse_temperatures
from cartnet_amd.synthetic import augment_data, make_crystal
from cartnet_amd.train import eval_epoch, train_epoch


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    # --- the reference's flags (main.py:123-154), same names / defaults / store_false quirks
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--name", type=str, default="CartNet")
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--batch_accumulation", type=int, default=16)
    p.add_argument("--dataset", type=str, default="ADP")
    p.add_argument("--dataset_path", type=str, default="./dataset/ADP_DATASET/")
    p.add_argument("--inference", action="store_true")
    p.add_argument("--montecarlo", action="store_true")
    p.add_argument("--checkpoint_path", type=str, default=None)
    p.add_argument("--inference_output", type=str, default="./inference.pkl")
    p.add_argument("--figshare_target", type=str, default="formation_energy_peratom")
    p.add_argument("--wandb_project", type=str, default="ADP")
    p.add_argument("--wandb_entity", type=str, default="aiquaneuro")
    p.add_argument("--loss", type=str, default="MAE")
    p.add_argument("--epochs", type=int, default=50)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--warmup", type=float, default=0.01)
    p.add_argument("--model", type=str, default="CartNet")
    p.add_argument("--max_neighbours", type=int, default=25)
    p.add_argument("--radius", type=float, default=5.0)
    p.add_argument("--num_layers", type=int, default=4)
    p.add_argument("--dim_in", type=int, default=256)
    p.add_argument("--dim_rbf", type=int, default=64)
    p.add_argument("--augment", action="store_true")
    p.add_argument("--invariant", action="store_true")
    p.add_argument("--disable_temp", action="store_false")
    p.add_argument("--no_standarize_temp", action="store_false")
    p.add_argument("--disable_envelope", action="store_false")
    p.add_argument("--disable_H", action="store_false")
    p.add_argument("--disable_atom_types", action="store_false")
    p.add_argument("--threads", type=int, default=8)
    p.add_argument("--workers", type=int, default=5)
    # --- this build
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--synthetic", type=int, default=32, help="number of synthetic crystals (80/10/10 split)")
    p.add_argument("--atoms", type=int, nargs=2, default=(30, 70), help="atoms per synthetic crystal: lo hi")
    p.add_argument("--gemm_precision", type=int, default=0, choices=(0, 1, 2),
                   help="GEMM arithmetic: 0 exact fp32 products (fp32 MFMA), 1 bf16x3 split operands (fp32-level "
                        "accuracy on the bf16 MFMA), 2 plain bf16 operands")
    p.add_argument("--montecarlo_rounds", type=int, default=100, help="passes of --montecarlo (the reference hard-codes 100)")
    p.add_argument("--fused_accumulation", action="store_true",
                   help="run the batch x batch_accumulation micro-batches of an optimiser step as ONE pass with BatchNorm "
                        "statistics and loss per micro-batch (CartnetGroups): the reference recipe's numbers at the "
                        "large-batch rate; CartNet (also with --gemm_precision 2 --bf16_storage) and iComformer (ignored for "
                        "the other models)")
    p.add_argument("--bf16_storage", action="store_true",
                   help="with --gemm_precision 2: keep the layers' edge-sized intermediate tensors in HBM as bf16 (fp32 "
                        "accumulate, fp64-summed BatchNorm statistics); combines with --fused_accumulation (the per-micro-batch "
                        "gate statistics are then those of the bf16 values as stored)")
    p.add_argument("--sync_batchnorm", action="store_true",
                   help="data-parallel runs: BatchNorm statistics over the crystals of ALL ranks (one small all-reduce per "
                        "BatchNorm and direction) instead of per rank; CartNet only (iComformer has no sync-BatchNorm), not "
                        "with --fused_accumulation")
    p.add_argument("--resident_dataset", action="store_true",
                   help="keep the splits as packed shards in HBM and build every batch (and its augmentation) on the GPU")
    p.add_argument("--shard_dir", type=str, default=None,
                   help="train from DIR/train.cnshard, val.cnshard and test.cnshard (tools/make_shards.py writes such a "
                        "directory) instead of synthetic crystals: implies --resident_dataset, ignores --synthetic and "
                        "--atoms; the radius graph is rebuilt on the GPU where the reference would rebuild it")
    p.add_argument("--eval_batch", type=int, default=1,
                   help="ADP: crystals per batch of the test pass, --inference and --montecarlo.  The reference tests at "
                        "batch size 1 (the default); N > 1 runs N crystals per forward and still "
                        "reports batch size 1's results: per-crystal means, one rotation per crystal, one pickle entry "
                        "per crystal.  Other datasets ignore it (they test at --batch)")
    p.add_argument("--predict", action="store_true",
                   help="ADP, CartNet / eComformer: apply --checkpoint_path to the crystals of --predict_input (targets not "
                        "needed) and write their ADPs, Cartesian and in CIF convention, to --predict_output")
    p.add_argument("--predict_input", type=str, default=None,
                   help="what --predict reads: a shard file (FILE.cnshard), a CIF file (FILE.cif) or a directory of CIF files")
    p.add_argument("--predict_temperature", type=float, default=None,
                   help="--predict from CIF files: the temperature in Kelvin of a crystal whose file gives none")
    p.add_argument("--predict_temperatures", type=str, default=None, metavar="SPEC",
                   help="--predict: predict every crystal at these temperatures (Kelvin) instead of its stored one, in one "
                        "pass: a list 100,150,200 or a range A:B:STEP (100:300:50 is five values; B is included when STEP "
                        "reaches it).  One forward then holds --eval_batch * T (* --rotations) crystals, the output has one "
                        "entry and one CIF per crystal and temperature (NAME_150K), and with two or more temperatures a "
                        "least-squares line per atom through them (series).  Not with --disable_temp, and with --predict "
                        "only")
    p.add_argument("--model_frame", type=str, default="stored", choices=["stored", "reduced_cell"],
                   help="--predict: the frame the model reads every crystal in.  stored (default): the cell and cart_dir as "
                        "the input stores them, as CartNet and eComformer are trained.  reduced_cell: --model icomformer "
                        "only, and required for it -- the forward runs in the frame of each crystal's canonical reduced "
                        "cell, as iComformer is trained (graph capped at --max_neighbours), and the predictions are "
                        "brought back (U = R P R^T), so that every key of the pickle, the analyses and the CIFs stay in "
                        "the stored cell; the pickle gains cell_rotation and cell_reduced.  Not with --rotations K > 1")
    p.add_argument("--predict_output", type=str, default="./predictions.pkl")
    p.add_argument("--predict_cif_dir", type=str, default=None, help="--predict: also write one CIF per crystal here (a shard's crystals in P1, a CIF's in its own setting)")
    p.add_argument("--rotations", type=int, default=1,
                   help="--predict / --inference: predict every crystal in K frames (the stored one and K - 1 random "
                        "rotations drawn from --seed), bring the predictions back to the stored frame and report their "
                        "mean, with the largest deviation of a frame from it per atom (rot_spread).  One forward then "
                        "holds --eval_batch * K crystals.  1 (the default): the pass as it always was.  --montecarlo and "
                        "training ignore it")
    p.add_argument("--rigid_bond", action="store_true",
                   help="--predict / --inference: Hirshfeld's rigid-bond test on the ADPs (and, with --inference, on the "
                        "truth as the baseline): per bonded pair of non-hydrogen atoms the difference of the mean-square "
                        "displacement amplitudes along the bond, which well-refined structures keep below about 0.001 "
                        "A^2.  Bonds are the edges of the radius graph within r_i + r_j + --bond_tolerance.  --montecarlo "
                        "and training ignore it")
    p.add_argument("--bond_tolerance", type=float, default=BOND_TOLERANCE,
                   help="--rigid_bond: an edge is a bond up to the sum of the covalent radii plus this many Angstrom")
    p.add_argument("--rigid_bond_threshold", type=float, default=RIGID_BOND_THRESHOLD,
                   help="--rigid_bond: bonds whose amplitudes differ by more than this (A^2) are counted as over")
    p.add_argument("--rigid_molecule", action="store_true",
                   help="--predict / --inference: find the molecules of every crystal (the components of the bond graph, "
                        "bonds as for --rigid_bond with --bond_tolerance) and run the rigid-body test of Rosenfield, "
                        "Trueblood & Dunitz on the ADPs (and, with --inference, on the truth): Hirshfeld's test over ALL "
                        "pairs of atoms of a molecule, along the unwrapped interatomic vectors.  Molecules that reach their "
                        "own image (polymers, frameworks) or whose graph is capped are reported and not tested.  Not "
                        "without --predict or --inference; --montecarlo and training ignore it")
    p.add_argument("--rigid_molecule_threshold", type=float, default=RIGID_BOND_THRESHOLD,
                   help="--rigid_molecule: pairs whose amplitudes differ by more than this (A^2) are counted as over")
    p.add_argument("--tls_fit", action="store_true",
                   help="--rigid_molecule: also fit the TLS model of Schomaker & Trueblood to the ADPs of every molecule of "
                        "five or more atoms (and, with --inference, to the truth as the baseline): the translation, "
                        "libration and screw tensors of the rigid body that explains them best, the ADP that body gives "
                        "every atom (tls_u) and what is left over (tls_resid, and tls_r per molecule).  It uses "
                        "--rigid_molecule's molecules and --bond_tolerance, and is refused without that flag; --montecarlo "
                        "and training ignore it")
    p.add_argument("--riding_h", action="store_true",
                   help="--predict: give every hydrogen an isotropic U by the riding model, a multiple of the predicted U_eq "
                        "of the atom it is bonded to (the nearest non-hydrogen atom within r_H + r + --bond_tolerance among "
                        "the edges of the radius graph), and write _atom_site_U_iso_or_equiv for every atom of the CIFs.  "
                        "Not with --disable_H; --inference, --montecarlo and training ignore it (the truth has no hydrogen "
                        "values)")
    p.add_argument("--riding_h_factor", type=float, default=RIDING_FACTOR,
                   help="--riding_h: U_iso(H) / U_eq(parent)")
    p.add_argument("--riding_h_factor_rotating", type=float, default=RIDING_FACTOR_ROTATING,
                   help="--riding_h: the same for hydrogens on oxygen (hydroxyl, water) and on a carbon that carries three "
                        "or more (methyl)")
    p.add_argument("--aniso_h", action="store_true",
                   help="--predict --riding_h: also give every hydrogen with a parent a full displacement tensor (SHADE / "
                        "ADPH style): its parent's predicted tensor, plus -- with --rigid_molecule --tls_fit -- the change "
                        "of the molecule's fitted rigid-body motion from the parent to the hydrogen, plus an internal X-H "
                        "motion of --aniso_h_stretch along and --aniso_h_bend across the bond; the CIFs then list the "
                        "hydrogens as Uani.  Refused without --predict and without --riding_h; --tls_fit is optional")
    p.add_argument("--aniso_h_stretch", type=float, default=ANISO_H_STRETCH,
                   help="--aniso_h: internal mean-square displacement along X-H (A^2).  The default is a nominal figure, "
                        "not a checked literature value: put in your own")
    p.add_argument("--aniso_h_bend", type=float, default=ANISO_H_BEND,
                   help="--aniso_h: the same across X-H, in both directions alike (A^2); nominal as well")
    p.add_argument("--bond_table", action="store_true",
                   help="--predict: list the bonds of every crystal (the edges of the radius graph within r_i + r_j + "
                        "--bond_tolerance between non-hydrogen atoms, each once) with Hirshfeld's D per bond, signed, the "
                        "Busing & Levy lower and upper bounds on the thermally averaged bond length and -- with "
                        "--rigid_molecule --tls_fit -- the length corrected for the fitted libration (bonds_* in the "
                        "pickle).  It needs no other analysis flag; refused without --predict.  The CIFs do not change")
    p.add_argument("--angle_table", action="store_true",
                   help="--predict: list the valence angles a-b-c and the torsions a-b-c-d of every crystal's bond graph "
                        "(the bonds of --bond_table, found with --bond_tolerance), in degrees, from the edges of the "
                        "radius graph, so through cell faces as well, and -- with --rigid_molecule --tls_fit -- their "
                        "values after the fitted libration (angles_* and torsions_* in the pickle).  It needs no other "
                        "analysis flag; refused without --predict.  The CIFs do not change")
    return p


def fill_cfg(args) -> None:
    """main.py:156-188."""
    set_cfg()
    cfg.seed, cfg.name = args.seed, args.name
    cfg.run_dir = "results/" + cfg.name + "/" + str(cfg.seed)
    cfg.batch, cfg.batch_accumulation = args.batch, args.batch_accumulation
    cfg.dataset.name = args.dataset
    cfg.loss, cfg.lr, cfg.warmup = args.loss, args.lr, args.warmup
    cfg.optim.max_epoch = args.epochs
    cfg.model = args.model
    cfg.max_neighbours = -1 if cfg.model == "CartNet" else args.max_neighbours
    cfg.radius, cfg.num_layers, cfg.dim_in, cfg.dim_rbf = args.radius, args.num_layers, args.dim_in, args.dim_rbf
    cfg.augment = False if cfg.model in ("icomformer", "ecomformer") else args.augment
    cfg.invariant = args.invariant
    cfg.use_temp = False if cfg.dataset.name != "ADP" else args.disable_temp
    cfg.standarize_temp = args.no_standarize_temp
    cfg.envelope, cfg.use_H, cfg.use_atom_types = args.disable_envelope, args.disable_H, args.disable_atom_types
    cfg.workers = args.workers
    cfg.device = args.device
    cfg.shard_dir = args.shard_dir
    if args.eval_batch < 1:
        raise ValueError("--eval_batch must be at least 1")
    cfg.eval_batch = args.eval_batch
    if args.rotations < 1:
        raise ValueError("--rotations must be at least 1")
    cfg.rotations = args.rotations
    cfg.gemm_precision = args.gemm_precision
    cfg.bn_group_size = 0
    cfg.half_storage = bool(args.bf16_storage) and cfg.model == "CartNet" and args.gemm_precision == 2
    cfg.sync_batchnorm = bool(args.sync_batchnorm) and cfg.model == "CartNet" and not args.fused_accumulation
    if args.fused_accumulation and cfg.model in ("CartNet", "icomformer") and cfg.batch_accumulation > 1:
        # the loader hands out whole optimiser steps; the model normalises (and train_epoch averages the loss) per
        # micro-batch of the reference's size
        cfg.bn_group_size = cfg.batch
        cfg.batch, cfg.batch_accumulation = cfg.batch * cfg.batch_accumulation, 1


def graph_request(cfg, shard_graph: Optional[dict], has_graph: bool) -> Optional[Tuple[float, Optional[int]]]:
    """The radius graph a ``--shard_dir`` run must build on a shard, ``(radius, cap)``, or None to keep the stored one.
    ``shard_graph``: the shard's recorded provenance ``{"radius", "max_neighbors"}`` or None; ``has_graph``: whether it
    stores edges at all.
      ADP + CartNet: the reference reads the edges from its files whatever --radius says (loader/loader.py:29,
        dataset/datasetADP.py:42); only a geometry-only shard is graphed, at (radius, uncapped).
      ADP + e/iComformer: compute_knn(cfg.max_neighbours, cfg.radius) (loader/loader.py:24-26).
      any other dataset: Figshare_Dataset(radius, max_neigh) with -1 -> no cap (loader/loader.py:106-110,
        dataset/figshare_dataset.py:18,65).
    A request equal to the recorded graph is skipped, as compute_knn skips a directory it has already written
    (dataset/utils.py:462-464)."""
    cap = cfg.max_neighbours if cfg.max_neighbours is not None and cfg.max_neighbours > 0 else None
    if cfg.dataset.name == "ADP" and cfg.model == "CartNet":
        return None if has_graph else (float(cfg.radius), None)
    want = (float(cfg.radius), cap)
    if has_graph and shard_graph is not None:
        k = shard_graph.get("max_neighbors")
        if (float(shard_graph["radius"]), int(k) if k is not None and int(k) > 0 else None) == want:
            return None
    return want


def shard_recipe(shards: list, cell: bool = True):
    """The reference's dataset recipe on resident shards, in the reference's order -- graph (graph_request), hydrogen
    removal (dataset/datasetADP.py:49-72), canonical cell (:75-80; not with ``cell=False``: ``predict`` keeps the stored
    frame and derives the model's from it).  Returns the new shards and the (mean, std) of the temperature
    standardisation of :17-18,43-45, which the collation kernel applies (the files hold Kelvin)."""
    from cartnet_amd.synthetic import TEMP_MEAN, TEMP_STD
    adp = cfg.dataset.name == "ADP"
    shards = list(shards)
    for i, s in enumerate(shards):
        req = graph_request(cfg, s.graph, s.has_graph)
        if req is not None:
            shards[i] = s.with_radius_graph(*req)
    return hydrogen_and_cell_steps(shards, cell), ((TEMP_MEAN, TEMP_STD) if adp and cfg.standarize_temp else (0.0, 1.0))


def hydrogen_and_cell_steps(shards: list, cell: bool = True) -> list:
    """The steps of the recipe that follow the graph, on resident shards: hydrogen removal under ``--disable_H``
    (loader/loader.py:29-32: DatasetADP(hydrogens=cfg.use_H), whatever the model), then -- unless ``cell`` is False -- the
    canonical lattice frame of iComformer on ADP (loader/loader.py:24-32: DatasetADP(optimize_cell=True))."""
    adp = cfg.dataset.name == "ADP"
    if adp and not cfg.use_H:
        shards = [s.without_hydrogens() for s in shards]
    if cell and adp and cfg.model == "icomformer":
        shards = [s.with_optimized_cell() for s in shards]
    return shards


def shard_loaders(rank: int, world: int):
    """``--shard_dir``: the three splits from shard files with ``shard_recipe`` applied."""
    from cartnet_amd.shard import DeviceShard, ShardLoader
    adp = cfg.dataset.name == "ADP"
    shards, (mean, std) = shard_recipe([DeviceShard.from_file(os.path.join(cfg.shard_dir, f"{part}.cnshard"), cfg.device)
                                        for part in ("train", "val", "test")])
    return [ShardLoader(shards[0], cfg.batch, shuffle=True, seed=cfg.seed, rank=rank, world_size=world,
                        augment=cfg.augment, temp_mean=mean, temp_std=std),
            ShardLoader(shards[1], cfg.batch, temp_mean=mean, temp_std=std),
            ShardLoader(shards[2], cfg.eval_batch if adp else cfg.batch, temp_mean=mean, temp_std=std)]


def create_loaders(args, rank: int, world: int):
    """Synthetic stand-in for loader/loader.py:create_loader: seed-123 80/10/10 split (loader.py:130-141)."""
    if cfg.shard_dir:
        return shard_loaders(rank, world)
    adp = cfg.dataset.name == "ADP"
    # every model but CartNet trains on the capped graphs (main.py:176, loader/loader.py:26,108: compute_knn)
    cap = cfg.max_neighbours if cfg.max_neighbours > 0 else None
    graphs = [make_crystal(g, None, cfg.radius, tuple(args.atoms), adp=adp, max_neighbors=cap)
              for g in range(args.synthetic)]
    perm = torch.randperm(len(graphs), generator=torch.Generator().manual_seed(123)).tolist()
    n_tr, n_va = int(0.8 * len(graphs)), int(0.1 * len(graphs))
    tr = [graphs[i] for i in perm[:n_tr]]
    va = [graphs[i] for i in perm[n_tr:n_tr + n_va]] or tr[:1]
    te = [graphs[i] for i in perm[n_tr + n_va:]] or tr[:1]
    # as in DatasetADP.get the order is: cap on the full crystal, hydrogen removal, canonical lattice frame
    if args.resident_dataset:                                             # cartnet_amd/shard.py
        from cartnet_amd.shard import DeviceShard, ShardLoader
        shards = hydrogen_and_cell_steps([DeviceShard.from_data_list(part, cfg.device) for part in (tr, va, te)])
        return [ShardLoader(shards[0], cfg.batch, shuffle=True, seed=cfg.seed, rank=rank, world_size=world,
                            augment=cfg.augment),
                ShardLoader(shards[1], cfg.batch), ShardLoader(shards[2], cfg.eval_batch if adp else cfg.batch)]
    if adp and not cfg.use_H:                                             # the host form of hydrogen_and_cell_steps
        tr, va, te = ([remove_hydrogens(d) for d in part] for part in (tr, va, te))
    if adp and cfg.model == "icomformer":
        tr, va, te = ([optimize_cell(d) for d in part] for part in (tr, va, te))
    gen = torch.Generator().manual_seed(cfg.seed + 1000 * rank)
    aug = (lambda d: augment_data(d, gen)) if cfg.augment else None
    return [DataLoader(tr, cfg.batch, shuffle=True, seed=cfg.seed, rank=rank, world_size=world, transform=aug),
            DataLoader(va, cfg.batch), DataLoader(te, cfg.eval_batch if adp else cfg.batch)]


def check_predict_args(args) -> None:
    """``--predict``'s requirements, checked before anything touches the device."""
    if not args.predict:
        raise SystemExit("--predict_temperatures serves --predict only")
    if cfg.dataset.name != "ADP":
        raise SystemExit("--predict: ADPs are predicted for the ADP dataset only")
    if args.checkpoint_path is None:
        raise SystemExit("--predict: weights not provided (--checkpoint_path)")
    if args.predict_input is None:
        raise SystemExit("--predict: no input shard (--predict_input FILE.cnshard)")
    if cfg.model == "icomformer" and args.model_frame != "reduced_cell":
        raise SystemExit("--predict does not serve --model icomformer in the stored frame: its recipe reads crystals in the "
                         "frame of the reduced cell.  Give --model_frame reduced_cell: the forward then runs there and U is "
                         "mapped back to the stored cell")
    if cfg.model != "icomformer" and args.model_frame != "stored":
        raise SystemExit(f"--model_frame {args.model_frame} serves --model icomformer only: {cfg.model} is trained in the "
                         "stored frame")
    if cfg.model == "icomformer" and cfg.rotations > 1:
        raise SystemExit("--predict --model icomformer serves one frame only (--rotations 1): its features are invariant, "
                         "and the K frames rotate cart_dir but not the cell, so they would feed it inconsistent inputs and "
                         "nothing would be averaged")
    if args.riding_h and not cfg.use_H:
        raise SystemExit("--riding_h with --disable_H: the hydrogens are gone, so there is nothing to ride")
    if args.predict_temperatures is not None:
        if not cfg.use_temp:
            raise SystemExit("--predict_temperatures with --disable_temp: the model has no temperature input, so the "
                             "series would be flat by construction")
        parse_temperatures(args.predict_temperatures)


def analysis_options(args, inference: bool = False) -> dict:
    """The analysis flags as the keywords of ``predict_adps`` or, with ``inference``, of ``evaluate.inference`` (no
    hydrogens there).  ``rigid_bond`` and ``riding_h`` are always among them, ``None`` without their flag; a later flag
    that is not given contributes no keyword at all: the passes are called as they always were (``main`` has refused a
    ``--tls_fit`` without ``--rigid_molecule``)."""
    tol = args.bond_tolerance
    options = {"rigid_bond": (tol, args.rigid_bond_threshold) if args.rigid_bond else None}
    if not inference:
        options["riding_h"] = (tol, args.riding_h_factor, args.riding_h_factor_rotating) if args.riding_h else None
    if args.rigid_molecule:
        options["rigid_molecule"] = (tol, args.rigid_molecule_threshold)
        if args.tls_fit:
            options["tls_fit"] = True
    if args.aniso_h and not inference:
        options["aniso_h"] = (args.aniso_h_stretch, args.aniso_h_bend)
    if args.bond_table and not inference:
        options["bond_table"] = tol
    if args.angle_table and not inference:
        options["angle_table"] = tol
    return options


def predict(model, args) -> dict:
    """``--predict``: the one shard of ``--predict_input`` through ``shard_recipe`` as the test split goes through it, in
    batches of ``--eval_batch``; the pickle of ``cartnet_amd.predict.predict_adps`` and, if asked for, one CIF per
    crystal.  CIF input (a file or a directory): the crystals the reference's filters accept are expanded to their unit
    cells on the GPU and take the same path; the pickle and the CIFs then carry one site-averaged ADP per atom of the
    asymmetric unit, and the result counts the ``rejected`` crystals (names and reasons go to stderr).
    ``--model icomformer --model_frame reduced_cell``: the recipe stops before the canonical cell, so the loader's shard -- graphed with
    ``--max_neighbours``, as iComformer is trained -- stays in the stored frame for the export, the analyses and the
    writers; its ``with_optimized_cell()`` is the ``model_frame`` of the pass, the frame only the forward sees, and the
    result says ``"model_frame": "reduced_cell"``."""
    import pickle
    from cartnet_amd import predict as pr
    from cartnet_amd.shard import ShardLoader
    source, sym, rejected = pr.load_input(args.predict_input, cfg.device, args.predict_temperature)
    (shard,), (mean, std) = shard_recipe([source], cell=False)
    frame = {"model_frame": shard.with_optimized_cell()} if cfg.model == "icomformer" else {}
    temps = parse_temperatures(args.predict_temperatures) if args.predict_temperatures is not None else None
    out = pr.predict_adps(
        model, ShardLoader(shard, cfg.eval_batch, temp_mean=mean, temp_std=std), cfg.device, sym=sym,
        rotations=cfg.rotations, seed=cfg.seed, temperatures=temps, **analysis_options(args), **frame)
    with open(args.predict_output, "wb") as f:
        pickle.dump(out, f)
    if args.predict_cif_dir:
        os.makedirs(args.predict_cif_dir, exist_ok=True)
        for k, name in enumerate(out["name"]):            # entries: one per crystal, or per crystal and temperature
            (pr.write_cif if sym is None else pr.write_cif_symmetric)(
                os.path.join(args.predict_cif_dir, f"{name}.cif"), pr.entry(out, k))
    res = pr.pass_statistics(out, args.predict_output, args.predict_cif_dir, rejected, cfg.rotations, temps)
    if frame:
        res["model_frame"] = "reduced_cell"
    return res


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    fill_cfg(args)
    if args.aniso_h and not args.predict:
        raise SystemExit("--aniso_h serves --predict only")
    if args.aniso_h and not args.riding_h:
        raise SystemExit("--aniso_h builds on the parents of --riding_h: give that flag as well")
    if args.bond_table and not args.predict:
        raise SystemExit("--bond_table serves --predict only")
    if args.angle_table and not args.predict:
        raise SystemExit("--angle_table serves --predict only")
    if args.model_frame != "stored" and not args.predict:
        raise SystemExit("--model_frame serves --predict only")
    if args.predict or args.predict_temperatures is not None:
        check_predict_args(args)
    if args.rigid_molecule and not (args.predict or args.inference):
        raise SystemExit("--rigid_molecule serves --predict and --inference only")
    if args.tls_fit and not args.rigid_molecule:
        raise SystemExit("--tls_fit fits the molecules of --rigid_molecule: give that flag as well")
    torch.set_num_threads(args.threads)
    rank, world, local = cdist.init_from_env()
    if world > 1:
        if os.environ.get("CARTNET_SHARE_GPU"):      # rehearsal on a box with fewer GPUs than ranks (gloo backend)
            local %= max(1, torch.cuda.device_count())
        cfg.device = f"cuda:{local}"
    torch.manual_seed(cfg.seed)
    if args.predict:
        model = create_model()
        model.load_state_dict(torch.load(args.checkpoint_path, map_location=cfg.device)["model_state"])
        res = predict(model, args)
        if rank == 0:
            print(json.dumps(res), flush=True)
        return res
    loaders = create_loaders(args, rank, world)
    model = create_model()
    n_params = sum(p.numel() for p in model.parameters())
    if args.inference or args.montecarlo:                                  # main.py:212-225 (ADP only, trained checkpoint)
        assert cfg.dataset.name == "ADP", "ADPs inference only for ADP dataset."
        assert args.checkpoint_path is not None, "Weights not provided."
        ck = torch.load(args.checkpoint_path, map_location=cfg.device)
        model.load_state_dict(ck["model_state"])
        if args.inference:
            res = evaluate.inference(model, loaders[-1], cfg.device, args.inference_output, rotations=cfg.rotations,
                                     seed=cfg.seed, **analysis_options(args, inference=True))
        else:
            res = evaluate.montecarlo(model, loaders[-1], cfg.device, args.inference_output,
                                      rounds=args.montecarlo_rounds, seed=cfg.seed)
        if rank == 0:
            print(json.dumps(res), flush=True)
        return res
    opt = FlatAdam(model, lr=cfg.lr)
    steps_per_epoch = len(loaders[0])
    total_steps = cfg.optim.max_epoch * steps_per_epoch // cfg.batch_accumulation + cfg.optim.max_epoch   # train.py:59
    sched_step = [0]

    def scheduler():          # OneCycleLR.step() (train/train.py:188): the learning rate and, with Adam, beta1
        sched_step[0] += 1
        k = min(sched_step[0], total_steps - 1)
        opt.set_lr(one_cycle_lr(k, total_steps, cfg.lr, cfg.warmup))
        opt.set_beta1(one_cycle_momentum(k, total_steps, cfg.warmup))

    opt.set_lr(one_cycle_lr(0, total_steps, cfg.lr, cfg.warmup))
    opt.set_beta1(one_cycle_momentum(0, total_steps, cfg.warmup))
    ckpt_dir = os.path.join(cfg.run_dir, "ckpt")
    best, history = float("inf"), []
    for epoch in range(cfg.optim.max_epoch):
        t0 = time.perf_counter()
        tr = train_epoch(loaders[0], model, opt, cfg.batch_accumulation, scheduler, device=cfg.device)
        va = eval_epoch(loaders[1], model, device=cfg.device)
        history.append({"epoch": epoch, "train_mae": tr["mae"], "val_mae": va["mae"],
                        "graphs_per_s": tr["graphs"] * world / tr["seconds"], "time_epoch": time.perf_counter() - t0})
        if rank == 0:
            print(json.dumps(history[-1]), flush=True)
            if va["mae"] < best:                                          # train/train.py:91-102
                best = va["mae"]
                os.makedirs(ckpt_dir, exist_ok=True)
                torch.save({"model_state": model.state_dict(), "optimizer_state": opt.state_dict()},
                           os.path.join(ckpt_dir, "best.ckpt"))
    cdist.assert_replicas_in_sync(model)
    cdist.barrier()
    result = {"params": n_params, "history": history, "best_val_mae": best}
    if rank == 0 and os.path.exists(os.path.join(ckpt_dir, "best.ckpt")):  # train/train.py:114-117
        ck = torch.load(os.path.join(ckpt_dir, "best.ckpt"), map_location=cfg.device)
        model.load_state_dict(ck["model_state"])
        adp = cfg.dataset.name == "ADP"
        test = eval_epoch(loaders[2], model, device=cfg.device, adp_metrics=adp, test_metrics=adp,
                          per_crystal=adp and cfg.eval_batch > 1)
        result["test_mae"] = test["mae"]
        result["test_metrics"] = test                                      # train/metrics.py:201-214
        print(json.dumps({"params": n_params, "best_val_mae": best, "test": test}), flush=True)
    return result


if __name__ == "__main__":
    main()

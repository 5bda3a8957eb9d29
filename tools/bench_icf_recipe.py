"""iComformer on the reference's ADP recipe (scripts/train_icomformer_adp.sh:3: --batch 4 --batch_accumulation 16), three ways
on ONE seeded set of 64 x 194-atom crystals, C = 256, fp32: forward + MAE + backward + one FlatAdam step per optimiser step.

  A  ungrouped   one batch of 64, BatchNorm over the whole batch (not the recipe's numbers: the large-batch rate)
  B  literal     16 micro-batches of 4, gradients accumulated, one Adam step (what the reference runs)
  C  grouped     one batch of 64 with bn_group_size = 4: statistics, running-statistics updates and loss per micro-batch

The variants are taken alternately in one process (A B C A B C ...), each warmed up first; a timed window is a whole
number of optimiser steps of at least one second and ends in a device synchronise; the medians are reported.  Prints one
JSON object (and writes it to --out).

    python tools/bench_icf_recipe.py [--rounds 5] [--graphs 64] [--atoms 194] [--group 4] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch

from cartnet_amd import train as ctrain
from cartnet_amd.comformer import iComformer, make_icomformer_state_dict
from cartnet_amd.config import cfg
from cartnet_amd.data import Batch
from cartnet_amd.optim import FlatAdam
from cartnet_amd.synthetic import make_crystal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per variant")
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--atoms", type=int, default=194)
    ap.add_argument("--group", type=int, default=4, help="micro-batch size of the recipe")
    ap.add_argument("--window", type=float, default=1.0, help="seconds a timed window lasts at least")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    cfg.radius = 5.0
    dev = torch.device("cuda:0")
    items = [make_crystal(100_000 + g, args.atoms) for g in range(args.graphs)]
    full = Batch.from_data_list(items).to(dev)
    micro = [Batch.from_data_list(items[s:s + args.group]).to(dev) for s in range(0, args.graphs, args.group)]
    z0 = {id(b): b.x for b in [full] + micro}         # forward replaces batch.x with the final atom features: re-arm it

    model = iComformer(256)
    model.load_state_dict(make_icomformer_state_dict(256, seed=0))
    model = model.to(dev).train()
    opt = FlatAdam(model, lr=1e-3)
    opt.zero_grad()

    def fwd_bwd(b, group):
        b.x = z0[id(b)]
        pred, true = model(b)
        loss = ctrain.grouped_loss(pred, true, b, group)[0] if group else ctrain.compute_loss(pred, true)[0]
        ctrain.backward(loss)

    def step_a():
        model.bn_group_size = 0
        fwd_bwd(full, 0)
        opt.step()
        opt.zero_grad()

    def step_b():
        model.bn_group_size = 0
        for b in micro:
            fwd_bwd(b, 0)
        opt.step()
        opt.zero_grad()

    def step_c():
        model.bn_group_size = args.group
        fwd_bwd(full, args.group)
        opt.step()
        opt.zero_grad()

    variants = {"A_ungrouped": step_a, "B_literal_micro_batches": step_b, "C_grouped": step_c}

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    counts = {}
    for name, fn in variants.items():                  # warm-up, and how many steps fill a window
        window(fn, 3)
        per = window(fn, 3) / 3
        counts[name] = max(2, int(args.window * 1.1 / per) + 1)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            while True:
                dt = window(fn, counts[name])
                if dt >= args.window:
                    break
                counts[name] = int(counts[name] * 1.3) + 1      # (a window that came out short is not counted)
            times[name].append(1e3 * dt / counts[name])
    res = {"workload": f"iComformer C=256 fp32, {args.graphs} x {args.atoms}-atom crystals (N {int(full.batch.shape[0])}, "
                       f"E {int(full.edge_index.shape[1])}), forward + MAE + backward + FlatAdam step; recipe batch "
                       f"{args.group} x accumulation {len(micro)}",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_seconds": args.window, "variants": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        res["variants"][name] = {"ms_per_optimizer_step_median": round(med, 3), "ms_min": round(min(ts), 3),
                                 "ms_max": round(max(ts), 3), "graphs_per_s": round(1e3 * args.graphs / med, 1),
                                 "steps_per_window": counts[name]}
    a, b, c = (res["variants"][k]["ms_per_optimizer_step_median"] for k in variants)
    res["C_over_A"] = round(c / a, 4)
    res["B_over_C"] = round(b / c, 3)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Time a ``--predict`` pass with and without riding hydrogens: ``cartnet_amd.predict.predict_adps`` with ``riding_h`` off
and on at ``--eval_batch 16`` over one unlabeled shard -- CartNet D = 256, L = 4 (fresh weights, eval mode) on 512
synthetic crystals of 30-70 atoms, packed geometry-only without targets and graphed at radius 5 on the GPU, the shard of
tools/bench_predict.py.  Its atoms sit at uniform random positions, so a hydrogen has a parent where chance put a
non-hydrogen atom within the bond limit; the tool reports how many do (``riders``) and refuses a shard without any.

The two variants are taken alternately (off on off on ...) in one process after a warm-up round; a time is the host clock
between two device synchronisations around the whole pass (forwards, exports, riding calls, transfers, the host-side split),
and the figure kept is the median of ``--rounds`` (5).  The pass without the flag is the code path of every earlier version:
the baseline.  One more pass runs with a HIP event pair around every ``riding_h`` call (the two lookups built with torch and
``cartnet_adp_riding_h``'s three launches): the share of the pass spent there.  There is no threshold: the tool reports.

The measurement runs in a child process under a time limit; the parent never touches the GPU.  One JSON object goes to
stdout and, with ``--out``, to a file.

usage: python tools/bench_riding_h.py [--rounds 5] [--out profiles/exp_riding_h.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CRYSTALS, ATOMS = 512, (30, 70)
EVAL_BATCH = 16
RIDING = (0.4, 1.2, 1.5)     # --bond_tolerance, --riding_h_factor, --riding_h_factor_rotating: the defaults
CHILD_LIMIT_S = 300


def measure(rounds: int) -> dict:
    import torch

    import main as entry
    from cartnet_amd import predict as cp
    from cartnet_amd.config import cfg
    from cartnet_amd.master import create_model
    from cartnet_amd.shard import DeviceShard, ShardLoader
    from cartnet_amd.synthetic import make_geometry
    if not torch.cuda.is_available():
        raise SystemExit("bench_riding_h.py measures on the GPU; none found")
    entry.fill_cfg(entry.build_parser().parse_args(["--dim_in", "256", "--num_layers", "4", "--no_standarize_temp"]))
    torch.manual_seed(0)
    model = create_model()
    crystals = [make_geometry(50000 + g, None, ATOMS) for g in range(CRYSTALS)]
    for d in crystals:
        del d.y
    (shard,), _ = entry.shard_recipe([DeviceShard.from_data_list(crystals, cfg.device)])
    assert not shard.labeled and shard.has_graph

    def timed(riding):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = cp.predict_adps(model, ShardLoader(shard, EVAL_BATCH), cfg.device, riding_h=riding)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    variants = [("off", None), ("on", RIDING)]
    first = {name: timed(riding)[1] for name, riding in variants}            # warm-up; kept for the counts
    print("warm-up done", file=sys.stderr, flush=True)
    stats = torch.stack(first["on"]["h_stats"])
    hydrogens, orphans = int(stats[:, 0].sum()), int(stats[:, 1].sum())
    if hydrogens == orphans:
        raise SystemExit("the shard has no bonded hydrogen: nothing rides, nothing to time")
    ms = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, riding in variants:
            ms[name].append(round(timed(riding)[0], 2))
    print(f"passes {ms}", file=sys.stderr, flush=True)
    med = {name: statistics.median(v) for name, v in ms.items()}

    # the share of a pass inside riding_h: an event pair around every call
    pairs, plain = [], cp.riding_h_call

    def stamped(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = plain(*a, **kw)
        e1.record()
        pairs.append((e0, e1))
        return out
    cp.riding_h_call = stamped
    try:
        wall, _ = timed(RIDING)
    finally:
        cp.riding_h_call = plain
    inside = sum(a.elapsed_time(b) for a, b in pairs)
    return {"device": torch.cuda.get_device_name(0), "crystals": CRYSTALS, "atoms": int(shard.atom_ptr[-1]),
            "edges": int(shard.edge_ptr[-1]), "rows": int(shard.y_ptr[-1]), "rounds": rounds, "eval_batch": EVAL_BATCH,
            "bond_tolerance": RIDING[0], "riding_h_factor": RIDING[1], "riding_h_factor_rotating": RIDING[2],
            "ms": ms, "ms_median": {name: round(v, 2) for name, v in med.items()},
            "on_over_off": round(med["on"] / med["off"], 3),
            "riding_h": {"wall_ms": round(wall, 2), "calls": len(pairs), "ms": round(inside, 3),
                         "us_per_call": round(1e3 * inside / len(pairs), 2), "share": round(inside / wall, 4)},
            # what the synthetic crystals (uniform random positions) and an untrained network give: no statement about a
            # real structure or a trained model
            "hydrogens": hydrogens, "orphans": orphans, "riders": hydrogens - orphans,
            "h_non_positive_untrained": int(stats[:, 3].sum())}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", action="store_true", help="(child) measure and print the JSON")
    a = ap.parse_args(argv)
    if a.child:
        print("RESULT " + json.dumps(measure(a.rounds)), flush=True)
        return
    # a child under its own time limit; the parent never touches the GPU
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds)]
    p = subprocess.run(cmd, timeout=CHILD_LIMIT_S, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        raise SystemExit(f"measurement: exit status {p.returncode}")
    res = {"tool": "tools/bench_riding_h.py", "model": "CartNet D=256 L=4, eval mode, fresh weights",
           "shard": f"{CRYSTALS} synthetic crystals of {ATOMS[0]}-{ATOMS[1]} atoms, unlabeled, geometry only, radius-5 graph "
                    "built on the GPU; uniform random positions, so hydrogens are bonded by chance"}
    res.update(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):]))
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

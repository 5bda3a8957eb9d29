"""Time ``cartnet_amd.predict.predict_adps`` at --eval_batch 1 / 16 / 64 over one unlabeled shard: CartNet D = 256, L = 4
(fresh weights, eval mode) on 512 synthetic crystals of 30-70 atoms, packed geometry-only without targets and graphed at
radius 5 on the GPU -- the shard ``main.py --predict`` would hold.

The settings are taken alternately (1 16 64 1 16 64 ...) in one process after a warm-up round; a time is the host clock
between two device synchronisations around the whole pass (forwards, exports, transfers, the host-side split), and the
figure kept is the median of ``--rounds`` (3).  One more pass per setting runs with a HIP event pair around every
``adp_export`` call: the share of the pass spent in ``cartnet_adp_export``'s two launches.  There is no threshold: the tool
reports.

The measurement runs in a child process under a time limit; the parent never touches the GPU.  One JSON object goes to
stdout and, with ``--out``, to a file.

usage: python tools/bench_predict.py [--rounds 3] [--out profiles/exp_predict.json]"""
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
SETTINGS = (1, 16, 64)
CHILD_LIMIT_S = 540


def measure(rounds: int) -> dict:
    import torch

    import main as entry
    from cartnet_amd import predict as cp
    from cartnet_amd.config import cfg
    from cartnet_amd.master import create_model
    from cartnet_amd.shard import DeviceShard, ShardLoader
    from cartnet_amd.synthetic import make_geometry
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict.py measures on the GPU; none found")
    entry.fill_cfg(entry.build_parser().parse_args(["--dim_in", "256", "--num_layers", "4", "--no_standarize_temp"]))
    torch.manual_seed(0)
    model = create_model()
    crystals = [make_geometry(50000 + g, None, ATOMS) for g in range(CRYSTALS)]
    for d in crystals:
        del d.y
    (shard,), _ = entry.shard_recipe([DeviceShard.from_data_list(crystals, cfg.device)])
    assert not shard.labeled and shard.has_graph

    def timed(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = cp.predict_adps(model, ShardLoader(shard, n), cfg.device)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    first = {n: timed(n)[1] for n in SETTINGS}                                     # warm-up; kept to compare the numbers
    print("warm-up done", file=sys.stderr, flush=True)
    ms = {n: [] for n in SETTINGS}
    for _ in range(rounds):
        for n in SETTINGS:
            ms[n].append(round(timed(n)[0], 2))
    print(f"passes {ms}", file=sys.stderr, flush=True)
    med = {n: statistics.median(v) for n, v in ms.items()}

    # the share of a pass inside cartnet_adp_export: an event pair around every call
    export, plain = {}, cp.adp_export
    for n in SETTINGS:
        pairs = []

        def stamped(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = plain(*a, **k)
            e1.record()
            pairs.append((e0, e1))
            return out
        cp.adp_export = stamped
        try:
            wall, _ = timed(n)
        finally:
            cp.adp_export = plain
        in_export = sum(a.elapsed_time(b) for a, b in pairs)
        export[str(n)] = {"wall_ms": round(wall, 2), "adp_export_calls": len(pairs), "adp_export_ms": round(in_export, 3),
                          "adp_export_us_per_call": round(1e3 * in_export / len(pairs), 2),
                          "adp_export_share": round(in_export / wall, 4)}

    def worst(n):        # a crystal's prediction at eval_batch n against eval_batch 1, norm-wise
        return max(float((a.double() - b.double()).abs().max() / b.double().abs().max())
                   for a, b in zip(first[n]["u_cart"], first[1]["u_cart"]))
    return {"device": torch.cuda.get_device_name(0), "crystals": CRYSTALS, "atoms": int(shard.atom_ptr[-1]),
            "edges": int(shard.edge_ptr[-1]), "rows": int(shard.y_ptr[-1]), "rounds": rounds,
            "ms": {str(n): v for n, v in ms.items()}, "ms_median": {str(n): round(v, 2) for n, v in med.items()},
            "speedup_vs_eval_batch_1": {str(n): round(med[1] / med[n], 2) for n in SETTINGS[1:]},
            "export": export,
            "u_cart_relative_difference_to_eval_batch_1": {str(n): worst(n) for n in SETTINGS[1:]},
            "non_positive_rows": int(sum(float(s[2]) for s in first[64]["stats"]))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
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
    res = {"tool": "tools/bench_predict.py", "model": "CartNet D=256 L=4, eval mode, fresh weights",
           "shard": f"{CRYSTALS} synthetic crystals of {ATOMS[0]}-{ATOMS[1]} atoms, unlabeled, geometry only, radius-5 graph "
                    "built on the GPU",
           "settings": list(SETTINGS)}
    res.update(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):]))
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

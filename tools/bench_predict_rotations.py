"""Time a ``--predict`` pass in K frames: ``cartnet_amd.predict.predict_adps`` at ``rotations`` 1 / 4 / 8 with
``--eval_batch 16`` over one unlabeled shard -- CartNet D = 256, L = 4 (fresh weights, eval mode) on 512 synthetic crystals
of 30-70 atoms, packed geometry-only without targets and graphed at radius 5 on the GPU, the shard of
tools/bench_predict.py -- against K plain passes at ``--eval_batch 16``, which is what predicting in K frames costs without
the flag (one pass per frame; the rotation of the input and the mean would come on top).

The variants are taken alternately (r1 r4 r8 4x 8x r1 ...) in one process after a warm-up round; a time is the host clock
between two device synchronisations around the whole pass (forwards, frame means, exports, transfers, the host-side split),
and the figure kept is the median of ``--rounds`` (3).  One more pass per K > 1 runs with a HIP event pair around every
``frame_mean`` call: the share of the pass spent in ``cartnet_adp_frame_mean``'s two launches.  There is no threshold: the
tool reports.

The measurement runs in a child process under a time limit; the parent never touches the GPU.  One JSON object goes to
stdout and, with ``--out``, to a file.

usage: python tools/bench_predict_rotations.py [--rounds 3] [--out profiles/exp_predict_rotations.json]"""
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
ROTATIONS = (1, 4, 8)
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
        raise SystemExit("bench_predict_rotations.py measures on the GPU; none found")
    entry.fill_cfg(entry.build_parser().parse_args(["--dim_in", "256", "--num_layers", "4", "--no_standarize_temp"]))
    torch.manual_seed(0)
    model = create_model()
    crystals = [make_geometry(50000 + g, None, ATOMS) for g in range(CRYSTALS)]
    for d in crystals:
        del d.y
    (shard,), _ = entry.shard_recipe([DeviceShard.from_data_list(crystals, cfg.device)])
    assert not shard.labeled and shard.has_graph

    def timed(k, passes=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(passes):
            out = cp.predict_adps(model, ShardLoader(shard, EVAL_BATCH), cfg.device, rotations=k, seed=0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    variants = [(f"rotations_{k}", k, 1) for k in ROTATIONS] + [(f"{k}_plain_passes", 1, k) for k in ROTATIONS[1:]]
    first = {name: timed(k, passes)[1] for name, k, passes in variants}            # warm-up; kept to compare the numbers
    print("warm-up done", file=sys.stderr, flush=True)
    ms = {name: [] for name, _, _ in variants}
    for _ in range(rounds):
        for name, k, passes in variants:
            ms[name].append(round(timed(k, passes)[0], 2))
    print(f"passes {ms}", file=sys.stderr, flush=True)
    med = {name: statistics.median(v) for name, v in ms.items()}

    # the share of a pass inside cartnet_adp_frame_mean: an event pair around every call
    share, plain = {}, cp.frame_mean
    for k in ROTATIONS[1:]:
        pairs = []

        def stamped(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = plain(*a, **kw)
            e1.record()
            pairs.append((e0, e1))
            return out
        cp.frame_mean = stamped
        try:
            wall, _ = timed(k)
        finally:
            cp.frame_mean = plain
        inside = sum(a.elapsed_time(b) for a, b in pairs)
        share[str(k)] = {"wall_ms": round(wall, 2), "frame_mean_calls": len(pairs), "frame_mean_ms": round(inside, 3),
                         "frame_mean_us_per_call": round(1e3 * inside / len(pairs), 2),
                         "frame_mean_share": round(inside / wall, 4)}

    def spread(k):       # what the frames of an untrained network scatter by: no statement about a trained one
        rot = torch.stack(first[f"rotations_{k}"]["rot_stats"])
        return {"max": float(rot[:, 1].max()), "mean_per_row": float(rot[:, 0].sum()) / int(shard.y_ptr[-1])}
    return {"device": torch.cuda.get_device_name(0), "crystals": CRYSTALS, "atoms": int(shard.atom_ptr[-1]),
            "edges": int(shard.edge_ptr[-1]), "rows": int(shard.y_ptr[-1]), "rounds": rounds, "eval_batch": EVAL_BATCH,
            "ms": ms, "ms_median": {name: round(v, 2) for name, v in med.items()},
            "one_pass_in_k_frames_over_k_plain_passes": {str(k): round(med[f"rotations_{k}"] / med[f"{k}_plain_passes"], 3)
                                                         for k in ROTATIONS[1:]},
            "cost_over_one_frame": {str(k): round(med[f"rotations_{k}"] / med["rotations_1"], 2) for k in ROTATIONS[1:]},
            "frame_mean": share,
            "rot_spread_untrained": {str(k): spread(k) for k in ROTATIONS[1:]}}


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
    res = {"tool": "tools/bench_predict_rotations.py", "model": "CartNet D=256 L=4, eval mode, fresh weights",
           "shard": f"{CRYSTALS} synthetic crystals of {ATOMS[0]}-{ATOMS[1]} atoms, unlabeled, geometry only, radius-5 graph "
                    "built on the GPU",
           "rotations": list(ROTATIONS)}
    res.update(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):]))
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

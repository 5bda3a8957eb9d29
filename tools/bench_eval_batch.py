"""Time the three evaluation paths of main.py at --eval_batch 1 / 16 / 64: the test pass after training
(``eval_epoch(adp_metrics=True, test_metrics=True)``), ``--inference`` and two rounds of ``--montecarlo``, with CartNet
D = 256, L = 4 (fresh weights, eval mode) on two synthetic test splits held as resident shards:

    small   512 crystals of 30-70 atoms
    large   128 crystals of 194 atoms

``eval_batch`` 1 is the reference's batch size, the baseline: ``eval_epoch`` per batch, and ``evaluate.inference`` /
``evaluate.montecarlo`` on a loader of batch size 1 (the latter then takes the reference's step, ``montecarlo_reference``).
16 and 64 are the batched forms (``per_crystal=True``, and the same two passes on a larger loader; ``montecarlo_batch``
is then the step).  The settings are taken alternately (1 16 64 1 16 64 ...) in one process after a warm-up round;
a time is the host clock between two device synchronisations around the whole workload, pickles included, and the figure
kept is the median of ``--rounds`` (3).  One more batched Monte-Carlo round runs with a HIP event pair around every
``adp_eval`` call: the share of the round spent in ``cartnet_adp_eval``'s two launches.

Each split runs in a child process of its own under a time limit, and the tool stops at the first child that fails; the
parent never touches the GPU.  One JSON object goes to stdout and, with ``--out``, to a file.

usage: python tools/bench_eval_batch.py [--rounds 3] [--out profiles/exp_eval_batch.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SPLITS = {"small": dict(crystals=512, atoms=(30, 70)), "large": dict(crystals=128, atoms=(194, 194))}
SETTINGS = (1, 16, 64)
CHILD_LIMIT_S = 540


def run_split(name: str, rounds: int, mc_rounds: int) -> dict:
    import torch

    import main as entry
    from cartnet_amd import evaluate
    from cartnet_amd.config import cfg
    from cartnet_amd.master import create_model
    from cartnet_amd.shard import DeviceShard, ShardLoader
    from cartnet_amd.synthetic import make_crystal
    from cartnet_amd.train import eval_epoch
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_batch.py measures on the GPU; none found")
    spec = SPLITS[name]
    entry.fill_cfg(entry.build_parser().parse_args(["--dim_in", "256", "--num_layers", "4"]))
    torch.manual_seed(0)
    model = create_model()
    lo, hi = spec["atoms"]
    crystals = [make_crystal(50000 + g, lo if lo == hi else None, cfg.radius, (lo, hi)) for g in range(spec["crystals"])]
    shard = DeviceShard.from_data_list(crystals, cfg.device)
    tmp = tempfile.mkdtemp(prefix="bench_eval_batch_")
    pkl = os.path.join(tmp, "out.pkl")

    def workloads(n):
        loader = ShardLoader(shard, n)
        return {"test_pass": lambda: eval_epoch(loader, model, cfg.device, adp_metrics=True, test_metrics=True,
                                                per_crystal=n > 1),
                "inference": lambda: evaluate.inference(model, loader, cfg.device, pkl),
                "montecarlo": lambda: evaluate.montecarlo(model, loader, cfg.device, pkl, rounds=mc_rounds)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    runs = {n: workloads(n) for n in SETTINGS}
    results = {n: {w: fn() for w, fn in runs[n].items()} for n in SETTINGS}          # warm-up; kept to compare the numbers
    ms = {w: {n: [] for n in SETTINGS} for w in ("test_pass", "inference", "montecarlo")}
    print(f"{name}: warm-up done", file=sys.stderr, flush=True)
    for w in ms:
        for _ in range(rounds):
            for n in SETTINGS:
                ms[w][n].append(round(timed(runs[n][w])[0], 2))
        print(f"{name}: {w} {ms[w]}", file=sys.stderr, flush=True)       # progress, so that a watcher sees the child alive
    med = {w: {n: statistics.median(v) for n, v in per.items()} for w, per in ms.items()}

    # the share of a batched Monte-Carlo round inside cartnet_adp_eval: an event pair around every call
    pairs, plain = [], evaluate.adp_eval

    def stamped(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = plain(*a, **k)
        e1.record()
        pairs.append((e0, e1))
        return out
    evaluate.adp_eval = stamped
    try:
        wall, _ = timed(lambda: evaluate.montecarlo(model, ShardLoader(shard, 64), cfg.device, pkl, rounds=1))
    finally:
        evaluate.adp_eval = plain
    in_eval = sum(a.elapsed_time(b) for a, b in pairs)

    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    ref = results[1]
    return {"device": torch.cuda.get_device_name(0), "crystals": spec["crystals"], "atoms": int(shard.atom_ptr[-1]), "edges": int(shard.edge_ptr[-1]),
            "target_rows": int(shard.y_ptr[-1]), "montecarlo_rounds": mc_rounds, "rounds": rounds,
            "ms": {w: {str(n): v for n, v in per.items()} for w, per in ms.items()},
            "ms_median": {w: {str(n): round(v, 2) for n, v in per.items()} for w, per in med.items()},
            "speedup_vs_eval_batch_1": {w: {str(n): round(per[1] / per[n], 2) for n in SETTINGS[1:]}
                                        for w, per in med.items()},
            "test_pass_relative_difference_to_eval_batch_1": {
                str(n): max(abs(results[n]["test_pass"][k] - ref["test_pass"][k]) / abs(ref["test_pass"][k])
                            for k in ref["test_pass"]) for n in SETTINGS[1:]},
            "inference_mae_mean": {str(n): results[n]["inference"]["mae_mean"] for n in SETTINGS},
            "montecarlo_64_one_round": {"wall_ms": round(wall, 2), "adp_eval_calls": len(pairs),
                                        "adp_eval_ms": round(in_eval, 3), "adp_eval_share": round(in_eval / wall, 4)}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--montecarlo_rounds", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--split", choices=sorted(SPLITS), default=None, help="(child) measure one split, print its JSON")
    a = ap.parse_args(argv)
    if a.split:
        print("RESULT " + json.dumps(run_split(a.split, a.rounds, a.montecarlo_rounds)), flush=True)
        return
    res = {"tool": "tools/bench_eval_batch.py", "model": "CartNet D=256 L=4, eval mode, fresh weights",
           "settings": list(SETTINGS), "splits": {}}
    for name in ("small", "large"):
        # a child per split: it ends at its own time limit, and a failure ends the tool before the next one starts
        cmd = [sys.executable, os.path.abspath(__file__), "--split", name, "--rounds", str(a.rounds),
               "--montecarlo_rounds", str(a.montecarlo_rounds)]
        p = subprocess.run(cmd, timeout=CHILD_LIMIT_S, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.stdout.write(p.stdout)
            raise SystemExit(f"split {name}: exit status {p.returncode}")
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
        res["splits"][name] = json.loads(line[len("RESULT "):])
        res["device"] = res["splits"][name].pop("device")
    res["eval_batch_64_faster_everywhere"] = all(v["64"] > 1.0 for s in res["splits"].values()
                                                 for v in s["speedup_vs_eval_batch_1"].values())
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not res["eval_batch_64_faster_everywhere"]:
        raise SystemExit("eval_batch 64 is not faster than 1 everywhere")


if __name__ == "__main__":
    main()

"""What the ``predict_adps`` benchmarks share (bench_predict.py, bench_predict_rotations.py, bench_bond_test.py,
bench_riding_h.py, bench_rigid_molecule.py, bench_bond_table.py): the model and the shard, the timed pass, the alternating
rounds, the event-stamping wrapper and the time-limited child process.  A tool states its variants and builds its JSON; everything else is here.

The model is CartNet D = 256, L = 4 (fresh weights, eval mode); the shard 512 synthetic crystals of 30-70 atoms, packed
geometry-only without targets and graphed at radius 5 on the GPU -- the shard ``main.py --predict`` would hold.  A time is
the host clock between two device synchronisations around whole passes (forwards, kernels, transfers, the host-side
split)."""
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
MODEL = "CartNet D=256 L=4, eval mode, fresh weights"
SHARD = f"{CRYSTALS} synthetic crystals of {ATOMS[0]}-{ATOMS[1]} atoms, unlabeled, geometry only, radius-5 graph built on the GPU"


class Bench:
    """The model and the shard on the device; ``tool`` names the caller in the message of a machine without a GPU."""

    def __init__(self, tool: str, crystals=None):
        """``crystals``: geometry-only ``Data`` objects to pack instead of the synthetic ones (bench_rigid_molecule.py)."""
        import torch

        import main as entry
        from cartnet_amd import predict
        from cartnet_amd.config import cfg
        from cartnet_amd.master import create_model
        from cartnet_amd.shard import DeviceShard
        from cartnet_amd.synthetic import make_geometry
        if not torch.cuda.is_available():
            raise SystemExit(f"{tool} measures on the GPU; none found")
        entry.fill_cfg(entry.build_parser().parse_args(["--dim_in", "256", "--num_layers", "4", "--no_standarize_temp"]))
        torch.manual_seed(0)
        self.torch, self.predict, self.device = torch, predict, cfg.device
        self.model = create_model()
        if crystals is None:
            crystals = [make_geometry(50000 + g, None, ATOMS) for g in range(CRYSTALS)]
            for d in crystals:
                del d.y
        self.crystals = len(crystals)
        (self.shard,), _ = entry.shard_recipe([DeviceShard.from_data_list(crystals, cfg.device)])
        assert not self.shard.labeled and self.shard.has_graph

    def sizes(self, rounds: int) -> dict:
        """The keys every tool's JSON starts with."""
        s = self.shard
        return {"device": self.torch.cuda.get_device_name(0), "crystals": self.crystals, "atoms": int(s.atom_ptr[-1]),
                "edges": int(s.edge_ptr[-1]), "rows": int(s.y_ptr[-1]), "rounds": rounds}

    def timed(self, eval_batch: int, passes: int = 1, **kw):
        """``(ms, result of the last pass)`` of ``passes`` passes of ``predict_adps(**kw)`` at ``eval_batch``."""
        from cartnet_amd.shard import ShardLoader
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(passes):
            out = self.predict.predict_adps(self.model, ShardLoader(self.shard, eval_batch), self.device, **kw)
        self.torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def rounds(self, variants: dict, rounds: int):
        """``variants``: name -> the keyword arguments of ``timed``.  One warm-up pass each, then ``rounds`` rounds that take
        the variants alternately.  Returns ``(results of the warm-up, ms per variant, their medians)``."""
        first = {name: self.timed(**kw)[1] for name, kw in variants.items()}
        print("warm-up done", file=sys.stderr, flush=True)
        ms = {name: [] for name in variants}
        for _ in range(rounds):
            for name, kw in variants.items():
                ms[name].append(round(self.timed(**kw)[0], 2))
        print(f"passes {ms}", file=sys.stderr, flush=True)
        return first, ms, {name: statistics.median(v) for name, v in ms.items()}

    def stamped(self, attr: str, **kw):
        """One more timed pass with a HIP event pair around every call of ``cartnet_amd.predict.<attr>``:
        ``(wall ms, calls, ms inside the calls)``."""
        torch, pairs, plain = self.torch, [], getattr(self.predict, attr)

        def stamped(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = plain(*a, **k)
            e1.record()
            pairs.append((e0, e1))
            return out
        setattr(self.predict, attr, stamped)
        try:
            wall, _ = self.timed(**kw)
        finally:
            setattr(self.predict, attr, plain)
        return wall, len(pairs), sum(a.elapsed_time(b) for a, b in pairs)


def share(wall: float, calls: int, inside: float, prefix: str = "") -> dict:
    """The JSON of one ``Bench.stamped`` pass; ``prefix`` goes in front of every key but ``wall_ms``."""
    return {"wall_ms": round(wall, 2), f"{prefix}calls": calls, f"{prefix}ms": round(inside, 3),
            f"{prefix}us_per_call": round(1e3 * inside / calls, 2), f"{prefix}share": round(inside / wall, 4)}


def run(tool: str, measure, rounds: int, limit_s: int, head: dict, argv=None) -> None:
    """A tool's ``main``: ``--rounds`` (default ``rounds``), ``--out FILE``.  ``measure(rounds)`` runs in a child process
    (the tool itself with ``--child``) under ``limit_s`` seconds; the parent never touches the GPU.  One JSON object --
    ``head``, then what ``measure`` returned -- goes to stdout and, with ``--out``, to a file."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=rounds)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", action="store_true", help="(child) measure and print the JSON")
    a = ap.parse_args(argv)
    if a.child:
        print("RESULT " + json.dumps(measure(a.rounds)), flush=True)
        return
    cmd = [sys.executable, os.path.join(ROOT, "tools", tool), "--child", "--rounds", str(a.rounds)]
    p = subprocess.run(cmd, timeout=limit_s, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        raise SystemExit(f"measurement: exit status {p.returncode}")
    res = {"tool": f"tools/{tool}", "model": MODEL, **head}
    res.update(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):]))
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

"""Time the symmetry expansion of CIF crystals (cartnet_amd/symmetry.py) on the GPU against its host statement, and the
site average as a share of a ``--predict`` batch.

4096 crystals: the five test crystals of tests/cif_utils.py (P1, P2_1/c, R-3, Fm-3m with 192 operators, one atom) cycled,
every second one a synthetic P2_1/c cell of 30 to 70 atoms (a seeded asymmetric unit on a jittered grid, so that no two
atoms come near the duplicate threshold).  Measured:

  expand       ``symmetry.expand`` (unlabeled and labeled): host packing, upload, count pass, the one device-to-host copy,
               fill pass, the copy of the result to the host -- the host clock between two device synchronisations, median
               of ``--rounds``; and the GPU passes alone (a HIP event pair around count and fill)
  expand_host  the same rule in torch fp64 on the CPU, once, over the first ``--host_crystals`` (512) crystals
  predict      ``predict_adps`` at --eval_batch 64 over the expanded crystals (CartNet D = 256, L = 4, fresh weights) with
               an event pair around every ``site_average`` call: its share of the pass

There is no threshold: the tool reports.  The measurement runs in a child process under a time limit; the parent never
touches the GPU.  One JSON object goes to stdout and, with ``--out``, to a file.

usage: python tools/bench_cif_expand.py [--rounds 3] [--out profiles/exp_cif_expand.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CRYSTALS = 4096
CHILD_LIMIT_S = 540


def synthetic_p21c(k: int) -> str:
    """A P2_1/c cell of 30 to 70 atoms: 8 to 17 atoms in general positions, 40 % hydrogen, every atom anisotropic."""
    import numpy as np

    import cif_utils as cu
    rng = np.random.default_rng(9000 + k)
    n = int(rng.integers(8, 18))
    cell = (rng.uniform(6, 9), rng.uniform(8, 13), rng.uniform(7, 11), 90.0, rng.uniform(95, 115), 90.0)
    pts = rng.choice(17 ** 3, size=n, replace=False)
    frac = np.stack([pts // 289, (pts // 17) % 17, pts % 17], 1) / 17.0 + 0.013 + rng.uniform(0, 0.02, (n, 3))
    lines = [f"data_syn{k}"] + [f"_cell_{t} {v:.4f}" for t, v in zip(
        ("length_a", "length_b", "length_c", "angle_alpha", "angle_beta", "angle_gamma"), cell)]
    lines += [f"_diffrn_ambient_temperature {rng.uniform(90, 300):.0f}", "loop_", "_symmetry_equiv_pos_as_xyz"]
    lines += [f"'{cu.op_string(o)}'" for o in cu.P21C]
    lines += ["loop_", "_atom_site_label", "_atom_site_type_symbol", "_atom_site_fract_x", "_atom_site_fract_y",
              "_atom_site_fract_z"]
    sym = [("H" if rng.uniform() < 0.4 else ("C", "N", "O")[int(rng.integers(0, 3))]) for _ in range(n)]
    sym[0] = "C"
    lines += [f"{s}{i + 1} {s} {f[0]:.5f} {f[1]:.5f} {f[2]:.5f}" for i, (s, f) in enumerate(zip(sym, frac))]
    lines += ["loop_", "_atom_site_aniso_label"] + [f"_atom_site_aniso_U_{q}" for q in ("11", "22", "33", "23", "13", "12")]
    for i, s in enumerate(sym):
        if s != "H":
            d, o = rng.uniform(0.015, 0.05, 3), rng.uniform(-0.004, 0.004, 3)
            lines.append(f"{s}{i + 1} " + " ".join(f"{v:.4f}" for v in (*d, *o)))
    return "\n".join(lines) + "\n"


def crystals(count: int):
    import cif_utils as cu
    from cartnet_amd.cif import read_cif
    keys = sorted(cu.CRYSTALS)
    text = "".join(synthetic_p21c(k) if k % 2 else cu.cif_text(keys[(k // 2) % len(keys)], name=f"t{k}") for k in range(count))
    out = read_cif(text)
    assert len(out) == count and all(c.reject_reason(True) is None for c in out)
    return out


def measure(rounds: int, host_crystals: int) -> dict:
    import torch

    import main as entry
    from cartnet_amd import predict as cp
    from cartnet_amd import symmetry
    from cartnet_amd.config import cfg
    from cartnet_amd.master import create_model
    from cartnet_amd.shard import DeviceShard, ShardLoader
    if not torch.cuda.is_available():
        raise SystemExit("bench_cif_expand.py measures on the GPU; none found")
    t0 = time.perf_counter()
    cs = crystals(CRYSTALS)
    read_s = time.perf_counter() - t0
    lib = symmetry._l.load()
    passes = {"count": [], "fill": []}

    def stamped(name):
        plain = getattr(lib, name)

        def call(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = plain(*a)
            e1.record()
            passes[name.rsplit("_", 1)[1]].append((e0, e1))
            return rc
        return plain, call

    def timed(labeled):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = symmetry.expand(cs, cfg_device, labeled=labeled)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    cfg_device = "cuda:0"
    timed(True)                                                                    # warm-up
    ms = {"unlabeled": [], "labeled": []}
    for _ in range(rounds):
        for k in ms:
            ms[k].append(round(timed(k == "labeled")[0], 2))
    # the GPU passes alone: an event pair around the count and the fill entry point
    saved = {}
    for name in ("cartnet_symmetry_expand_count", "cartnet_symmetry_expand_fill"):
        saved[name], wrapped = stamped(name)
        setattr(lib, name, wrapped)
    try:
        _, (arrays, sym) = timed(False)
    finally:
        for name, plain in saved.items():
            setattr(lib, name, plain)
    gpu = {k: round(sum(a.elapsed_time(b) for a, b in v), 3) for k, v in passes.items()}
    calls = {k: len(v) for k, v in passes.items()}
    t0 = time.perf_counter()
    symmetry.expand_host(cs[:host_crystals], labeled=False)
    host_ms = (time.perf_counter() - t0) * 1e3
    print(f"expand {ms}, passes {gpu}, host {host_ms:.0f} ms / {host_crystals}", file=sys.stderr, flush=True)

    # the site average inside a --predict pass
    entry.fill_cfg(entry.build_parser().parse_args(["--dim_in", "256", "--num_layers", "4"]))
    torch.manual_seed(0)
    model = create_model()
    (shard,), (mean, std) = entry.shard_recipe([DeviceShard(arrays, cfg.device, labeled=False, names=sym.names)])

    def predict_pass():
        torch.cuda.synchronize()
        t = time.perf_counter()
        cp.predict_adps(model, ShardLoader(shard, 64, temp_mean=mean, temp_std=std), cfg.device, sym=sym)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    predict_pass()
    plain_ms = [round(predict_pass(), 2) for _ in range(rounds)]
    pairs, plain = [], symmetry.site_average

    def stamped_average(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = plain(*a, **k)
        e1.record()
        pairs.append((e0, e1))
        return out
    symmetry.site_average = stamped_average
    try:
        wall = predict_pass()
    finally:
        symmetry.site_average = plain
    in_avg = sum(a.elapsed_time(b) for a, b in pairs)
    med = {k: statistics.median(v) for k, v in ms.items()}
    host_per_crystal = host_ms / host_crystals
    return {"device": torch.cuda.get_device_name(0), "crystals": CRYSTALS, "read_cif_s": round(read_s, 2),
            "asymmetric_atoms": int(sum(len(c.labels) for c in cs)), "operators": int(sum(len(c.symops) for c in cs)),
            "candidates": int(sum(len(c.labels) * len(c.symops) for c in cs)), "atoms": int(arrays["atom_ptr"][-1]),
            "rows": int(arrays["y_ptr"][-1]), "rounds": rounds, "expand_ms": ms,
            "expand_ms_median": {k: round(v, 2) for k, v in med.items()},
            "gpu_passes_ms": gpu, "gpu_pass_calls": calls,
            "expand_host": {"crystals": host_crystals, "ms": round(host_ms, 1), "ms_per_crystal": round(host_per_crystal, 4)},
            "expand_us_per_crystal": round(1e3 * med["unlabeled"] / CRYSTALS, 2),
            "speedup_vs_expand_host": round(host_per_crystal / (med["unlabeled"] / CRYSTALS), 1),
            "predict": {"eval_batch": 64, "ms": plain_ms, "wall_ms": round(wall, 2), "site_average_calls": len(pairs),
                        "site_average_ms": round(in_avg, 3), "site_average_us_per_call": round(1e3 * in_avg / len(pairs), 2),
                        "site_average_share": round(in_avg / wall, 4)}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host_crystals", type=int, default=512)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--child", action="store_true", help="(child) measure and print the JSON")
    a = ap.parse_args(argv)
    if a.child:
        print("RESULT " + json.dumps(measure(a.rounds, a.host_crystals)), flush=True)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--host_crystals",
           str(a.host_crystals)]
    p = subprocess.run(cmd, timeout=CHILD_LIMIT_S, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stdout.write(p.stdout)
        raise SystemExit(f"measurement: exit status {p.returncode}")
    res = {"tool": "tools/bench_cif_expand.py",
           "crystals_from": "the five test crystals of tests/cif_utils.py cycled, every second crystal a synthetic P2_1/c "
                            "cell of 30-70 atoms",
           "model": "CartNet D=256 L=4, eval mode, fresh weights"}
    res.update(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):]))
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

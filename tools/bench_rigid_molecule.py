"""Time a ``--predict`` pass with and without the rigid-body test on molecules: ``cartnet_amd.predict.predict_adps`` with
``rigid_molecule`` off and on at ``--eval_batch 16`` -- CartNet D = 256, L = 4 (fresh weights, eval mode).

The synthetic shard of tools/bench_predict.py has uniformly random atoms and holds few real molecules, so the tool builds a
shard of its own in process: 512 crystals, each a cell of 82 x 12 x 12 A with four lanes along a, 6 A apart; two to four of
the lanes hold a zig-zag chain of 10-60 carbons that starts anywhere along a (so many cross the cell face) or a ring of
6-8; unlabeled, geometry only, graphed at radius 5 on the GPU.  The flag-off pass is also taken on the synthetic shard, the
figure ``profiles/exp_bond_test.json`` holds for the parent commit.

The variants are taken alternately (off on off on ...) in one process after a warm-up round; a time is the host clock
between two device synchronisations around the whole pass, and the figure kept is the median of ``--rounds`` (5).  Two more
passes run with a HIP event pair around every ``molecules`` call (``cartnet_molecules``' launch on the batch's graph) and
around every ``molecule_test`` call: the two entry points' own share.  The sweeps per crystal are those of
``bonds.molecules_host`` on the same batches.  There is no threshold: the tool reports.

The measurement runs in a child process under a time limit; the parent never touches the GPU.  One JSON object goes to
stdout and, with ``--out``, to a file.

usage: python tools/bench_rigid_molecule.py [--rounds 5] [--out profiles/exp_rigid_molecule.json]"""
import predict_bench as pb

EVAL_BATCH = 16
MOLECULE = (0.4, 1e-3)       # --bond_tolerance, --rigid_molecule_threshold: the defaults
CELL = (82.0, 12.0, 12.0)
LANES = ((3.0, 3.0), (3.0, 9.0), (9.0, 3.0), (9.0, 9.0))
STEP, ZIG = 1.25, 0.8        # a chain's bonds are 1.484 A long, its second neighbours 2.5 A apart
SHARD = (f"{pb.CRYSTALS} crystals of 2-4 molecules (zig-zag chains of 10-60 carbons, rings of 6-8) in a cell of "
         "82 x 12 x 12 A, unlabeled, geometry only, radius-5 graph built on the GPU")


def molecular_crystals() -> list:
    import numpy as np
    import torch
    from cartnet_amd.data import Data
    out = []
    for g in range(pb.CRYSTALS):
        rng = np.random.default_rng(70000 + g)
        parts = []
        for lane in rng.permutation(4)[:rng.integers(2, 5)]:
            y, z = LANES[lane]
            x0 = rng.random() * CELL[0]
            if rng.random() < 0.75:
                k = np.arange(rng.integers(10, 61), dtype=np.float64)
                parts.append(np.stack([x0 + STEP * k, y + ZIG * (k % 2), z + 0.0 * k], axis=1))
            else:
                n = int(rng.integers(6, 9))
                a = 2 * np.pi * np.arange(n) / n
                r = 1.45 / (2 * np.sin(np.pi / n))
                parts.append(np.stack([x0 + r * np.cos(a), y + r * np.sin(a), z + 0.0 * a], axis=1))
        pos = np.mod(np.concatenate(parts), CELL)
        pos = pos[rng.permutation(len(pos))]                                  # a molecule's atoms are not neighbours in order
        out.append(Data(x=torch.full((len(pos),), 6, dtype=torch.int64), pos=torch.tensor(pos, dtype=torch.float32),
                        cell=torch.diag(torch.tensor(CELL)).unsqueeze(0), natoms=torch.tensor([len(pos)]),
                        temperature=torch.tensor([0.25])))
    return out


def sweeps(b) -> list:
    """The sweeps ``bonds.molecules_host`` takes per crystal of the shard (the last one, which changes nothing, included)."""
    from cartnet_amd.bonds import molecules_host
    from cartnet_amd.shard import ShardLoader
    out = []
    for batch in ShardLoader(b.shard, EVAL_BATCH):
        z, mask = batch.x.cpu().numpy(), batch.non_H_mask.cpu().numpy()
        row = mask.cumsum() - 1
        row[~mask] = -1
        out += molecules_host(z, batch.edge_index.cpu().numpy(), batch.cart_dist.cpu().numpy(),
                              batch.cart_dir.cpu().numpy(), row, batch.ptr.cpu().numpy(), MOLECULE[0])["sweeps"].tolist()
    return out


def measure(rounds: int) -> dict:
    import statistics
    off, on = {"eval_batch": EVAL_BATCH}, {"eval_batch": EVAL_BATCH, "rigid_molecule": MOLECULE}
    synthetic = pb.Bench("bench_rigid_molecule.py")
    _, ms_s, med_s = synthetic.rounds({"off": off, "on": on}, rounds)
    sizes_s = synthetic.sizes(rounds)
    del synthetic
    b = pb.Bench("bench_rigid_molecule.py", molecular_crystals())
    first, ms, med = b.rounds({"off": off, "on": on}, rounds)
    stats = b.torch.stack(first["on"]["mol_stats"])                           # the warm-up is kept for the counts
    pairs = int(stats[:, 5].sum())
    n_sweeps = sweeps(b)
    return {**b.sizes(rounds), "eval_batch": EVAL_BATCH, "bond_tolerance": MOLECULE[0],
            "rigid_molecule_threshold": MOLECULE[1],
            "ms": ms, "ms_median": {name: round(v, 2) for name, v in med.items()},
            "on_over_off": round(med["on"] / med["off"], 3),
            "molecules_call": pb.share(*b.stamped("find_molecules", **on)),   # an event pair around every call
            "molecule_test_call": pb.share(*b.stamped("molecule_test", **on)),
            "sweeps_per_crystal": {"min": min(n_sweeps), "median": statistics.median(n_sweeps), "max": max(n_sweeps)},
            "molecules": int(stats[:, 0].sum()), "molecules_tested": int(stats[:, 1].sum()),
            "molecules_periodic": int(stats[:, 2].sum()), "molecules_open": int(stats[:, 3].sum()),
            "molecule_atoms_max": int(stats[:, 4].max()), "directed_pairs": pairs,
            # what an untrained network gives: no statement about a trained model
            "rigid_molecule_mean_untrained": float(stats[:, 6].sum()) / max(pairs, 1),
            "synthetic_shard": {"shard": pb.SHARD, **sizes_s, "ms": ms_s,
                                "ms_median": {name: round(v, 2) for name, v in med_s.items()},
                                "on_over_off": round(med_s["on"] / med_s["off"], 3),
                                "off_parent_ms": 43.47, "off_parent_source": "profiles/exp_bond_test.json"}}


if __name__ == "__main__":
    pb.run("bench_rigid_molecule.py", measure, rounds=5, limit_s=420, head={"shard": SHARD})

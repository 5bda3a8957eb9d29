"""Time a ``--predict`` pass with and without the rigid-bond test: ``cartnet_amd.predict.predict_adps`` with ``rigid_bond``
off and on at ``--eval_batch 16`` over one unlabeled shard -- CartNet D = 256, L = 4 (fresh weights, eval mode) on 512
synthetic crystals of 30-70 atoms, packed geometry-only without targets and graphed at radius 5 on the GPU, the shard of
tools/bench_predict.py.

The two variants are taken alternately (off on off on ...) in one process after a warm-up round; a time is the host clock
between two device synchronisations around the whole pass (forwards, exports, bond tests, transfers, the host-side split),
and the figure kept is the median of ``--rounds`` (5).  One more pass runs with a HIP event pair around every ``bond_test``
call (``cartnet_adp_bond_test``'s two launches; the lookups are built per batch, outside the call): the share of the pass
spent there.
There is no threshold: the tool reports.

The measurement runs in a child process under a time limit; the parent never touches the GPU.  One JSON object goes to
stdout and, with ``--out``, to a file.

usage: python tools/bench_bond_test.py [--rounds 5] [--out profiles/exp_bond_test.json]"""
import predict_bench as pb

EVAL_BATCH = 16
BOND = (0.4, 1e-3)           # --bond_tolerance, --rigid_bond_threshold: the defaults


def measure(rounds: int) -> dict:
    b = pb.Bench("bench_bond_test.py")
    on = {"eval_batch": EVAL_BATCH, "rigid_bond": BOND}
    first, ms, med = b.rounds({"off": {"eval_batch": EVAL_BATCH, "rigid_bond": None}, "on": on}, rounds)
    stats = b.torch.stack(first["on"]["bond_stats"])                          # the warm-up is kept for the counts
    bonds = int(stats[:, 0].sum())
    return {**b.sizes(rounds), "eval_batch": EVAL_BATCH, "bond_tolerance": BOND[0], "rigid_bond_threshold": BOND[1],
            "ms": ms, "ms_median": {name: round(v, 2) for name, v in med.items()},
            "on_over_off": round(med["on"] / med["off"], 3),
            "bond_test": pb.share(*b.stamped("bond_test", **on)),             # an event pair around every bond_test call
            # what the synthetic crystals (uniform random positions) and an untrained network give: no statement about a
            # real structure or a trained model
            "directed_bonds": bonds, "rigid_bond_mean_untrained": float(stats[:, 1].sum()) / max(bonds, 1),
            "rigid_bond_over_untrained": int(stats[:, 3].sum())}


if __name__ == "__main__":
    pb.run("bench_bond_test.py", measure, rounds=5, limit_s=300, head={"shard": pb.SHARD})

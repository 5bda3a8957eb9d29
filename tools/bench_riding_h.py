"""Time a ``--predict`` pass with and without riding hydrogens: ``cartnet_amd.predict.predict_adps`` with ``riding_h`` off
and on at ``--eval_batch 16`` over one unlabeled shard -- CartNet D = 256, L = 4 (fresh weights, eval mode) on 512
synthetic crystals of 30-70 atoms, packed geometry-only without targets and graphed at radius 5 on the GPU, the shard of
tools/bench_predict.py.  Its atoms sit at uniform random positions, so a hydrogen has a parent where chance put a
non-hydrogen atom within the bond limit; the tool reports how many do (``riders``) and refuses a shard without any.

The two variants are taken alternately (off on off on ...) in one process after a warm-up round; a time is the host clock
between two device synchronisations around the whole pass (forwards, exports, riding calls, transfers, the host-side split),
and the figure kept is the median of ``--rounds`` (5).  The pass without the flag is the code path of every earlier version:
the baseline.  One more pass runs with a HIP event pair around every ``riding_h`` call (``cartnet_adp_riding_h``'s three
launches; the lookups are built per batch, outside the call): the share of the pass spent there.  There is no threshold:
the tool reports.

The measurement runs in a child process under a time limit; the parent never touches the GPU.  One JSON object goes to
stdout and, with ``--out``, to a file.

usage: python tools/bench_riding_h.py [--rounds 5] [--out profiles/exp_riding_h.json]"""
import predict_bench as pb

EVAL_BATCH = 16
RIDING = (0.4, 1.2, 1.5)     # --bond_tolerance, --riding_h_factor, --riding_h_factor_rotating: the defaults


def measure(rounds: int) -> dict:
    b = pb.Bench("bench_riding_h.py")
    on = {"eval_batch": EVAL_BATCH, "riding_h": RIDING}
    first, ms, med = b.rounds({"off": {"eval_batch": EVAL_BATCH, "riding_h": None}, "on": on}, rounds)
    stats = b.torch.stack(first["on"]["h_stats"])                             # the warm-up is kept for the counts
    hydrogens, orphans = int(stats[:, 0].sum()), int(stats[:, 1].sum())
    if hydrogens == orphans:
        raise SystemExit("the shard has no bonded hydrogen: nothing rides, nothing to report")
    return {**b.sizes(rounds), "eval_batch": EVAL_BATCH,
            "bond_tolerance": RIDING[0], "riding_h_factor": RIDING[1], "riding_h_factor_rotating": RIDING[2],
            "ms": ms, "ms_median": {name: round(v, 2) for name, v in med.items()},
            "on_over_off": round(med["on"] / med["off"], 3),
            "riding_h": pb.share(*b.stamped("riding_h_call", **on)),          # an event pair around every riding_h call
            # what the synthetic crystals (uniform random positions) and an untrained network give: no statement about a
            # real structure or a trained model
            "hydrogens": hydrogens, "orphans": orphans, "riders": hydrogens - orphans,
            "h_non_positive_untrained": int(stats[:, 3].sum())}


if __name__ == "__main__":
    pb.run("bench_riding_h.py", measure, rounds=5, limit_s=300,
           head={"shard": pb.SHARD + "; uniform random positions, so hydrogens are bonded by chance"})

"""Time a ``--predict`` pass over a temperature series: ``cartnet_amd.predict.predict_adps`` with ``temperatures`` of T = 1 /
4 / 8 values (evenly spaced from 100 K to 300 K) at ``--eval_batch 16`` over one unlabeled shard -- CartNet D = 256, L = 4
(fresh weights, eval mode) on 512 synthetic crystals of 30-70 atoms, packed geometry-only without targets and graphed at
radius 5 on the GPU, the shard of tools/bench_predict.py -- against T plain passes at ``--eval_batch 16``, which is what a
series costs without the flag (one pass per temperature; rewriting the shard, loading the checkpoint and uploading again
would come on top).

The variants are taken alternately (t1 t4 t8 1x 4x 8x t1 ...) in one process after a warm-up round; a time is the host clock
between two device synchronisations around the whole pass (forwards, exports, the line fit, transfers, the host-side split),
and the figure kept is the median of ``--rounds`` (3).  One more pass per T > 1 runs with a HIP event pair around every
``temp_series`` call: the share of the pass spent in ``cartnet_adp_temp_series``'s two launches (and the small upload of the
temperatures in front of them).  There is no threshold: the tool reports.

The measurement runs in a child process under a time limit; the parent never touches the GPU.  One JSON object goes to
stdout and, with ``--out``, to a file.

usage: python tools/bench_predict_temperatures.py [--rounds 3] [--out profiles/exp_predict_temperatures.json]"""
import statistics
import sys

import predict_bench as pb

EVAL_BATCH = 16
SERIES = (1, 4, 8)
LOW, HIGH = 100.0, 300.0


def temperatures(T: int) -> list:
    """T values evenly spaced over [LOW, HIGH]; T = 1: the middle."""
    return [0.5 * (LOW + HIGH)] if T == 1 else [LOW + (HIGH - LOW) * t / (T - 1) for t in range(T)]


def measure(rounds: int) -> dict:
    b = pb.Bench("bench_predict_temperatures.py")
    variants = {f"temperatures_{T}": {"eval_batch": EVAL_BATCH, "temperatures": temperatures(T)} for T in SERIES}
    variants["plain_pass"] = {"eval_batch": EVAL_BATCH}
    variants.update({f"{T}_plain_passes": {"eval_batch": EVAL_BATCH, "passes": T} for T in SERIES[1:]})
    # One warm-up pass each, then the rounds.  No result is kept (Bench.rounds keeps the warm-up's): a T = 8 result is
    # 8 * 512 entries of a dozen tensors each, and with six of them alive the collector's passes show up in the times.
    rows = int(b.shard.y_ptr[-1])
    for name, kw in variants.items():
        out = b.timed(**kw)[1]
        T = len(kw.get("temperatures", (0,)))
        assert len(out["name"]) == pb.CRYSTALS * T and ("series" in out) == (T > 1)
        assert T == 1 or sum(int(t.shape[0]) for t in out["series"]["t_resid"]) == rows
        del out
    print("warm-up done", file=sys.stderr, flush=True)
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, kw in variants.items():
            ms[name].append(round(b.timed(**kw)[0], 2))
    print(f"passes {ms}", file=sys.stderr, flush=True)
    med = {name: statistics.median(v) for name, v in ms.items()}
    # the share of a pass inside cartnet_adp_temp_series: an event pair around every call
    share = {str(T): pb.share(*b.stamped("temp_series", **variants[f"temperatures_{T}"]), prefix="temp_series_")
             for T in SERIES[1:]}
    return {**b.sizes(rounds), "eval_batch": EVAL_BATCH,
            "temperatures": {str(T): [round(v, 2) for v in temperatures(T)] for T in SERIES},
            "ms": ms, "ms_median": {name: round(v, 2) for name, v in med.items()},
            "one_pass_at_t_temperatures_over_t_plain_passes": {
                str(T): round(med[f"temperatures_{T}"] / med[f"{T}_plain_passes"], 3) for T in SERIES[1:]},
            "cost_over_one_plain_pass": {str(T): round(med[f"temperatures_{T}"] / med["plain_pass"], 2) for T in SERIES},
            "temp_series": share}


if __name__ == "__main__":
    pb.run("bench_predict_temperatures.py", measure, rounds=3, limit_s=540,
           head={"shard": pb.SHARD, "series": list(SERIES)})

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
import predict_bench as pb

SETTINGS = (1, 16, 64)


def measure(rounds: int) -> dict:
    b = pb.Bench("bench_predict.py")
    first, ms, med = b.rounds({n: {"eval_batch": n} for n in SETTINGS}, rounds)  # the warm-up is kept to compare the numbers
    # the share of a pass inside cartnet_adp_export: an event pair around every call
    export = {str(n): pb.share(*b.stamped("adp_export", eval_batch=n), prefix="adp_export_") for n in SETTINGS}

    def worst(n):        # a crystal's prediction at eval_batch n against eval_batch 1, norm-wise
        return max(float((p.double() - q.double()).abs().max() / q.double().abs().max())
                   for p, q in zip(first[n]["u_cart"], first[1]["u_cart"]))
    return {**b.sizes(rounds),
            "ms": {str(n): v for n, v in ms.items()}, "ms_median": {str(n): round(v, 2) for n, v in med.items()},
            "speedup_vs_eval_batch_1": {str(n): round(med[1] / med[n], 2) for n in SETTINGS[1:]},
            "export": export,
            "u_cart_relative_difference_to_eval_batch_1": {str(n): worst(n) for n in SETTINGS[1:]},
            "non_positive_rows": int(sum(float(s[2]) for s in first[64]["stats"]))}


if __name__ == "__main__":
    pb.run("bench_predict.py", measure, rounds=3, limit_s=540, head={"shard": pb.SHARD, "settings": list(SETTINGS)})

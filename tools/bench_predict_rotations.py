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
import predict_bench as pb

EVAL_BATCH = 16
ROTATIONS = (1, 4, 8)


def measure(rounds: int) -> dict:
    b = pb.Bench("bench_predict_rotations.py")
    torch = b.torch
    variants = {f"rotations_{k}": {"eval_batch": EVAL_BATCH, "rotations": k, "seed": 0} for k in ROTATIONS}
    variants.update({f"{k}_plain_passes": {"eval_batch": EVAL_BATCH, "passes": k, "rotations": 1, "seed": 0}
                     for k in ROTATIONS[1:]})
    first, ms, med = b.rounds(variants, rounds)                               # the warm-up is kept to compare the numbers
    # the share of a pass inside cartnet_adp_frame_mean: an event pair around every call
    share = {str(k): pb.share(*b.stamped("frame_mean", **variants[f"rotations_{k}"]), prefix="frame_mean_")
             for k in ROTATIONS[1:]}
    rows = int(b.shard.y_ptr[-1])

    def spread(k):       # what the frames of an untrained network scatter by: no statement about a trained one
        rot = torch.stack(first[f"rotations_{k}"]["rot_stats"])
        return {"max": float(rot[:, 1].max()), "mean_per_row": float(rot[:, 0].sum()) / rows}
    return {**b.sizes(rounds), "eval_batch": EVAL_BATCH,
            "ms": ms, "ms_median": {name: round(v, 2) for name, v in med.items()},
            "one_pass_in_k_frames_over_k_plain_passes": {str(k): round(med[f"rotations_{k}"] / med[f"{k}_plain_passes"], 3)
                                                         for k in ROTATIONS[1:]},
            "cost_over_one_frame": {str(k): round(med[f"rotations_{k}"] / med["rotations_1"], 2) for k in ROTATIONS[1:]},
            "frame_mean": share,
            "rot_spread_untrained": {str(k): spread(k) for k in ROTATIONS[1:]}}


if __name__ == "__main__":
    pb.run("bench_predict_rotations.py", measure, rounds=3, limit_s=540,
           head={"shard": pb.SHARD, "rotations": list(ROTATIONS)})

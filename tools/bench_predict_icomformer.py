"""Time ``predict_adps(model_frame=...)``, the pass of ``main.py --predict --model icomformer``: iComformer D = 256 (fresh
weights, eval mode) on the shard of bench_predict.py -- 512 synthetic crystals of 30-70 atoms, unlabeled, geometry only --
graphed at radius 5 with the cap of ``--max_neighbours`` 25 on the GPU, at ``--eval_batch 16``.  The stored shard feeds the
export; its ``with_optimized_cell()`` is the frame the model reads.

Two variants, taken alternately in one process after a warm-up pass each, the median of ``--rounds`` (5) kept; a time is
the host clock between two device synchronisations around the whole pass:

  frame_view      the pass as it is: per batch one ``cartnet_collate_frame_view`` and one ``cartnet_adp_stored_frame``
  second_collate  the same pass with a second full ``collate`` of the reduced shard in place of ``frame_view``

One more ``frame_view`` pass runs with a HIP event pair around every ``frame_view`` and every ``stored_frame`` call: their
share of the pass.  There is no threshold: the tool reports.

The measurement runs in a child process under a time limit; the parent never touches the GPU.  One JSON object goes to
stdout and, with ``--out``, to a file.

usage: python tools/bench_predict_icomformer.py [--rounds 5] [--out profiles/exp_predict_icomformer.json]"""
import statistics
import sys
import time

import predict_bench as pb

EVAL_BATCH = 16
MODEL = "iComformer D=256, eval mode, fresh weights"


class _Frame:
    """A ``model_frame`` that answers ``frame_view`` through ``view(batch)``; everything else is the reduced shard's."""

    def __init__(self, reduced, view):
        self.t, self.num_graphs, self.frame_view = reduced.t, reduced.num_graphs, view
        self.atom_ptr, self.edge_ptr = reduced.atom_ptr, reduced.edge_ptr


def measure(rounds: int) -> dict:
    import torch

    import main as entry
    from cartnet_amd import predict
    from cartnet_amd.config import cfg
    from cartnet_amd.master import create_model
    from cartnet_amd.shard import DeviceShard, ShardLoader
    from cartnet_amd.synthetic import make_geometry
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict_icomformer.py measures on the GPU; none found")
    entry.fill_cfg(entry.build_parser().parse_args(["--model", "icomformer", "--dim_in", "256", "--no_standarize_temp"]))
    torch.manual_seed(0)
    model = create_model()
    crystals = [make_geometry(50000 + g, None, pb.ATOMS) for g in range(pb.CRYSTALS)]
    for d in crystals:
        del d.y
    (stored,), (mean, std) = entry.shard_recipe([DeviceShard.from_data_list(crystals, cfg.device)], cell=False)
    reduced = stored.with_optimized_cell()
    assert not stored.labeled and stored.has_graph and stored.graph["max_neighbors"] == cfg.max_neighbours

    def second_collate(batch):
        b = reduced.collate(batch._sel, None, mean, std)
        b.rotation = reduced.t["rotation"][b._meta[:int(b.num_graphs)]].view(-1, 3, 3)
        return b
    frames = {"frame_view": reduced, "second_collate": _Frame(reduced, second_collate)}

    def timed(frame):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = predict.predict_adps(model, ShardLoader(stored, EVAL_BATCH, temp_mean=mean, temp_std=std), cfg.device,
                                   model_frame=frame)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    first = {name: timed(f)[1] for name, f in frames.items()}
    print("warm-up done", file=sys.stderr, flush=True)
    ms = {name: [] for name in frames}
    for _ in range(rounds):
        for name, f in frames.items():
            ms[name].append(round(timed(f)[0], 2))
    print(f"passes {ms}", file=sys.stderr, flush=True)
    med = {name: statistics.median(v) for name, v in ms.items()}

    # the share of the two new calls: an event pair around each
    pairs = {"frame_view": [], "stored_frame": []}

    def stamp(name, fn):
        def stamped(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            pairs[name].append((e0, e1))
            return out
        return stamped
    plain = predict.stored_frame
    predict.stored_frame = stamp("stored_frame", plain)
    try:
        wall, _ = timed(_Frame(reduced, stamp("frame_view", reduced.frame_view)))
    finally:
        predict.stored_frame = plain
    inside = {name: sum(a.elapsed_time(b) for a, b in p) for name, p in pairs.items()}
    calls = {name: pb.share(wall, len(pairs[name]), inside[name], prefix=f"{name}_") for name in pairs}
    same = all(torch.equal(a, b) for a, b in zip(first["frame_view"]["u_cart"], first["second_collate"]["u_cart"]))
    return {"device": torch.cuda.get_device_name(0), "crystals": len(crystals), "atoms": int(stored.atom_ptr[-1]),
            "edges": int(stored.edge_ptr[-1]), "rows": int(stored.y_ptr[-1]), "rounds": rounds, "eval_batch": EVAL_BATCH,
            "ms": ms, "ms_median": {k: round(v, 2) for k, v in med.items()},
            "second_collate_over_frame_view": round(med["second_collate"] / med["frame_view"], 3),
            "stamped_pass": {"wall_ms": round(wall, 2), **{k: v for c in calls.values() for k, v in c.items() if k != "wall_ms"},
                             "both_share": round((inside["frame_view"] + inside["stored_frame"]) / wall, 4)},
            "u_cart_equal_in_both_variants": bool(same)}


if __name__ == "__main__":
    pb.run("bench_predict_icomformer.py", measure, rounds=5, limit_s=540,
           head={"model": MODEL, "shard": pb.SHARD + ", capped at 25 neighbours", "variants": ["frame_view", "second_collate"]})

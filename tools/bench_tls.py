"""Time a ``--predict --rigid_molecule`` pass with and without the TLS fit: ``cartnet_amd.predict.predict_adps`` with
``tls_fit`` off and on at ``--eval_batch 16`` -- CartNet D = 256, L = 4 (fresh weights, eval mode) -- on the molecular
crystals of tools/bench_rigid_molecule.py: 512 crystals of two to four molecules, zig-zag chains of 10-60 carbons and
rings of 6-8.  Those molecules are planar, so every fit is the rank-19 case; the kernel's work does not depend on the rank
(the Jacobi iteration runs on the full 20 x 20 matrix either way).

The variants are taken alternately (off on off on ...) in one process after a warm-up round; a time is the host clock
between two device synchronisations around the whole pass, and the figure kept is the median of ``--rounds`` (5).  One more
pass runs with a HIP event pair around every ``tls_fit`` call (``cartnet_adp_tls_fit``'s two launches; the lookups are
per batch): the entry point's own share.  The flag-off pass is the parent commit's flag-on pass of
``profiles/exp_rigid_molecule.json``; without ``--rigid_molecule`` nothing of this runs.  There is no threshold: the tool
reports.

The measurement runs in a child process under a time limit; the parent never touches the GPU.  One JSON object goes to
stdout and, with ``--out``, to a file.

usage: python tools/bench_tls.py [--rounds 5] [--out profiles/exp_tls.json]"""
import bench_rigid_molecule as rm
import predict_bench as pb


def measure(rounds: int) -> dict:
    off = {"eval_batch": rm.EVAL_BATCH, "rigid_molecule": rm.MOLECULE}
    on = {**off, "tls_fit": True}
    b = pb.Bench("bench_tls.py", rm.molecular_crystals())
    first, ms, med = b.rounds({"off": off, "on": on}, rounds)
    stats = b.torch.stack(first["on"]["tls_stats"])                           # the warm-up is kept for the counts
    sizes = b.torch.cat([t[r > 0] for t, r in zip(first["on"]["mol_size"], first["on"]["tls_rank"])])
    r2, s2 = float(stats[:, 3].sum()), float(stats[:, 4].sum())
    return {**b.sizes(rounds), "eval_batch": rm.EVAL_BATCH, "bond_tolerance": rm.MOLECULE[0],
            "ms": ms, "ms_median": {name: round(v, 2) for name, v in med.items()},
            "on_over_off": round(med["on"] / med["off"], 3),
            "tls_fit_call": pb.share(*b.stamped("tls_fit_call", **on)),       # an event pair around every call
            "tls_molecules": int(stats[:, 0].sum()), "tls_rank_deficient": int(stats[:, 1].sum()),
            "tls_nonphysical": int(stats[:, 2].sum()), "fitted_rows": int(sizes.numel()),
            "fitted_molecule_atoms_max": int(sizes.max()) if sizes.numel() else 0,
            # what an untrained network gives: no statement about a trained model
            "tls_r_untrained": (r2 / s2) ** 0.5 if s2 > 0 else 0.0,
            "off_parent_ms": 72.66, "off_parent_source": "profiles/exp_rigid_molecule.json (its flag-on pass)"}


if __name__ == "__main__":
    pb.run("bench_tls.py", measure, rounds=5, limit_s=420, head={"shard": rm.SHARD})

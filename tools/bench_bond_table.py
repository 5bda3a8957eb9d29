"""Time a ``--predict`` pass with and without the bond table: ``cartnet_amd.predict.predict_adps`` with ``bond_table`` off
and on at ``--eval_batch 16`` -- CartNet D = 256, L = 4 (fresh weights, eval mode) -- on the molecular crystals of
tools/bench_rigid_molecule.py (512 crystals of two to four molecules, chains of 10-60 carbons and rings of 6-8), once as
the plain pass and once beside ``rigid_molecule`` and ``tls_fit``, where the table gains its libration column.

The variants are taken alternately (off on off on ...) in one process after a warm-up round; a time is the host clock
between two device synchronisations around the whole pass, and the figure kept is the median of ``--rounds`` (5).  Two more
passes run with a HIP event pair around every ``bond_index`` call (``cartnet_bond_table_count``, the scan and the copy of
the crystals' offsets to the host, which ends the event pair only after the host has waited for it) and around every
``bond_table_call`` (``cartnet_adp_bond_table``'s two launches): the two calls' own share.  The flag-off pass runs no line
of the feature -- no index is built, no key is added -- so it is the parent commit's path; it was not timed on the
parent's tree.  There is no threshold: the tool reports.

The measurement runs in a child process under a time limit; the parent never touches the GPU.  One JSON object goes to
stdout and, with ``--out``, to a file; the commit a kept file was taken on is added to it by hand.

usage: python tools/bench_bond_table.py [--rounds 5] [--out profiles/exp_bond_table.json]"""
import bench_rigid_molecule as rm
import predict_bench as pb

TOL = rm.MOLECULE[0]             # --bond_tolerance: the default


def measure(rounds: int) -> dict:
    off = {"eval_batch": rm.EVAL_BATCH}
    tls_off = {**off, "rigid_molecule": rm.MOLECULE, "tls_fit": True}
    variants = {"off": off, "on": {**off, "bond_table": TOL}, "tls_off": tls_off, "tls_on": {**tls_off, "bond_table": TOL}}
    b = pb.Bench("bench_bond_table.py", rm.molecular_crystals())
    first, ms, med = b.rounds(variants, rounds)
    stats = b.torch.stack(first["tls_on"]["bonds_stats"])                     # the warm-up is kept for the counts
    listed, with_l = int(stats[:, 0].sum()), int(stats[:, 5].sum())
    return {**b.sizes(rounds), "eval_batch": rm.EVAL_BATCH, "bond_tolerance": TOL, "ms": ms,
            "ms_median": {name: round(v, 2) for name, v in med.items()},
            "on_over_off": round(med["on"] / med["off"], 3), "tls_on_over_tls_off": round(med["tls_on"] / med["tls_off"], 3),
            "bond_index_call": pb.share(*b.stamped("bond_index", **variants["on"])),      # an event pair around every call
            "bond_table_call": pb.share(*b.stamped("bond_table_call", **variants["on"])),
            "bond_table_call_with_tls": pb.share(*b.stamped("bond_table_call", **variants["tls_on"])),
            "bonds_listed": listed, "bonds_unlisted": int(stats[:, 1].sum()),
            "bond_length_mean": float(stats[:, 2].sum()) / max(listed, 1), "bond_libration_bonds": with_l,
            # what an untrained network gives: no statement about a trained model
            "bond_libration_mean_untrained": float(stats[:, 6].sum()) / max(with_l, 1),
            "bond_bounds_nan_untrained": int(stats[:, 8].sum()),
            "off_path": "the flag-off pass runs no line of the feature; it was not timed on the parent commit's tree"}


if __name__ == "__main__":
    pb.run("bench_bond_table.py", measure, rounds=5, limit_s=420, head={"shard": rm.SHARD})

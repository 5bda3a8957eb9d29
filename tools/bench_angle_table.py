"""Time a ``--predict`` pass with and without the angle and torsion tables: ``cartnet_amd.predict.predict_adps`` with
``angle_table`` off and on at ``--eval_batch 16`` -- CartNet D = 256, L = 4 (fresh weights, eval mode) -- on the molecular
crystals of tools/bench_rigid_molecule.py (512 crystals of two to four molecules, chains of 10-60 carbons and rings of
6-8), once as the plain pass and once beside ``rigid_molecule`` and ``tls_fit``, where the tables gain their libration
columns.

The variants are taken alternately (off on off on ...) in one process after a warm-up round; a time is the host clock
between two device synchronisations around the whole pass, and the figure kept is the median of ``--rounds`` (5).  Two more
passes run with a HIP event pair around every ``angle_index`` call (the bond index it builds on with its copy,
``cartnet_bond_adjacency``, ``cartnet_angle_table_count``, the scans and the copy of the crystals' offsets to the host) and
around every ``angle_table_call`` (``cartnet_adp_angle_table``'s three launches): the two calls' own share.  The flag-off
pass builds no index and adds no key; it is the ``off`` variant of tools/bench_bond_table.py, which exists on the parent
commit as well and is the tool to time it against that tree.  There is no threshold: the tool reports.

The measurement runs in a child process under a time limit; the parent never touches the GPU.  One JSON object goes to
stdout and, with ``--out``, to a file; the commit a kept file was taken on is added to it by hand.

usage: python tools/bench_angle_table.py [--rounds 5] [--out profiles/exp_angle_table.json]"""
import bench_rigid_molecule as rm
import predict_bench as pb

TOL = rm.MOLECULE[0]             # --bond_tolerance: the default


def measure(rounds: int) -> dict:
    off = {"eval_batch": rm.EVAL_BATCH}
    tls_off = {**off, "rigid_molecule": rm.MOLECULE, "tls_fit": True}
    variants = {"off": off, "on": {**off, "angle_table": TOL}, "tls_off": tls_off, "tls_on": {**tls_off, "angle_table": TOL}}
    b = pb.Bench("bench_angle_table.py", rm.molecular_crystals())
    first, ms, med = b.rounds(variants, rounds)
    sa = b.torch.stack(first["tls_on"]["angles_stats"])                       # the warm-up is kept for the counts
    st = b.torch.stack(first["tls_on"]["torsions_stats"])
    angles, torsions = int(sa[:, 0].sum()), int(st[:, 0].sum())
    return {**b.sizes(rounds), "eval_batch": rm.EVAL_BATCH, "bond_tolerance": TOL, "ms": ms,
            "ms_median": {name: round(v, 2) for name, v in med.items()},
            "on_over_off": round(med["on"] / med["off"], 3), "tls_on_over_tls_off": round(med["tls_on"] / med["tls_off"], 3),
            "angle_index_call": pb.share(*b.stamped("angle_index", **variants["on"])),    # an event pair around every call
            "angle_table_call": pb.share(*b.stamped("angle_table_call", **variants["on"])),
            "angle_table_call_with_tls": pb.share(*b.stamped("angle_table_call", **variants["tls_on"])),
            "angles_listed": angles, "angle_mean": float(sa[:, 1].sum()) / max(angles, 1),
            "torsions_listed": torsions, "torsions_undefined": int(st[:, 1].sum()),
            "angle_libration_angles": int(sa[:, 2].sum()), "torsion_libration_torsions": int(st[:, 2].sum()),
            # what an untrained network gives: no statement about a trained model
            "angle_libration_mean_untrained": float(sa[:, 3].sum()) / max(int(sa[:, 2].sum()), 1),
            "torsion_libration_mean_untrained": float(st[:, 3].sum()) / max(int(st[:, 2].sum()), 1),
            "off_path": "the flag-off passes are bench_bond_table.py's off variants: timed against the parent commit's tree with it"}


if __name__ == "__main__":
    pb.run("bench_angle_table.py", measure, rounds=5, limit_s=420, head={"shard": rm.SHARD})

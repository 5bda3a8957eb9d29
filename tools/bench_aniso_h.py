"""Time a ``--predict --riding_h --rigid_molecule --tls_fit`` pass with and without anisotropic hydrogens:
``cartnet_amd.predict.predict_adps`` with ``aniso_h`` off and on at ``--eval_batch 16`` -- CartNet D = 256, L = 4 (fresh
weights, eval mode) -- on the molecular crystals of tools/bench_rigid_molecule.py with a hydrogen added 1 A above every
carbon (the chains and rings lie in planes of constant z, the lanes are 6 A apart): 512 crystals of two to four molecules.
Those molecules are planar, so every fitted one is the rank-19 case and its hydrogens are source 4; the kernel's work does
not depend on the rank.

The variants are taken alternately (off on off on ...) in one process after a warm-up round; a time is the host clock
between two device synchronisations around the whole pass, and the figure kept is the median of ``--rounds`` (5).  Two more
passes run with a HIP event pair around every ``aniso_h`` call (``cartnet_adp_aniso_h``'s two launches; the lookups are per batch)
and around every ``aniso_entries`` call (the export over atoms as rows): the feature's own share.  The flag-off pass runs
no line of the feature; the parent commit's figure for it (``off_parent_ms``) was taken once with the parent's tree on the
same box and is a constant here, with its source.  There is no threshold: the tool reports.

The measurement runs in a child process under a time limit; the parent never touches the GPU.  One JSON object goes to
stdout and, with ``--out``, to a file.

usage: python tools/bench_aniso_h.py [--rounds 5] [--out profiles/exp_aniso_h.json]"""
import bench_rigid_molecule as rm
import predict_bench as pb

RIDING = (0.4, 1.2, 1.5)         # --bond_tolerance, --riding_h_factor, --riding_h_factor_rotating: the defaults
ANISO = (0.005, 0.020)           # --aniso_h_stretch, --aniso_h_bend: the (nominal) defaults
OFF_PARENT_MS = 145.57
OFF_PARENT_SOURCE = ("the same flag-off pass with the parent commit's tree, a process of its own in the call that wrote "
                     "profiles/exp_aniso_h.json: median of 5; see off_pass_same_box there")
SHARD = rm.SHARD.replace("carbons", "carbons, a hydrogen 1 A above each")


def crystals_with_hydrogens() -> list:
    import torch
    from cartnet_amd.data import Data
    out = []
    for d in rm.molecular_crystals():
        h = d.pos + torch.tensor([0.0, 0.0, 1.0])
        n = int(d.pos.shape[0])
        out.append(Data(x=torch.stack([d.x, torch.ones_like(d.x)], dim=1).reshape(-1),
                        pos=torch.stack([d.pos, h], dim=1).reshape(-1, 3), cell=d.cell, natoms=torch.tensor([2 * n]),
                        temperature=d.temperature))
    return out


def measure(rounds: int) -> dict:
    off = {"eval_batch": rm.EVAL_BATCH, "riding_h": RIDING, "rigid_molecule": rm.MOLECULE, "tls_fit": True}
    on = {**off, "aniso_h": ANISO}
    b = pb.Bench("bench_aniso_h.py", crystals_with_hydrogens())
    first, ms, med = b.rounds({"off": off, "on": on}, rounds)
    stats = b.torch.stack(first["on"]["h_aniso_stats"])                       # the warm-up is kept for the counts
    count = int(stats[:, 0].sum())
    return {**b.sizes(rounds), "eval_batch": rm.EVAL_BATCH, "bond_tolerance": RIDING[0], "aniso_h_stretch": ANISO[0],
            "aniso_h_bend": ANISO[1], "ms": ms, "ms_median": {name: round(v, 2) for name, v in med.items()},
            "on_over_off": round(med["on"] / med["off"], 3),
            "aniso_h_call": pb.share(*b.stamped("aniso_h_call", **on)),       # an event pair around every call
            "aniso_entries_call": pb.share(*b.stamped("aniso_entries", **on)),
            "h_aniso": count, "h_aniso_tls": int(stats[:, 1].sum()),
            # what an untrained network gives: no statement about a trained model
            "h_aniso_ueq_mean_untrained": float(stats[:, 2].sum()) / max(count, 1),
            "h_aniso_non_positive_untrained": int(stats[:, 3].sum()),
            "off_parent_ms": OFF_PARENT_MS, "off_parent_source": OFF_PARENT_SOURCE}


if __name__ == "__main__":
    pb.run("bench_aniso_h.py", measure, rounds=5, limit_s=420, head={"shard": SHARD})

"""The bytes of the bond-graph analyses: ``metrics.bond_test``, ``riding_h``, ``molecules``, ``molecule_test``,
``tls_fit`` and ``aniso_h`` (with and without the TLS results) on a fixed set of small batches, as the sha256 of every
output array.  These kernels promise "two runs give the same bytes", so the digests of one commit are an oracle for the
next: ``tests/golden/analysis_bytes.json`` holds those of the commit before the kernels moved onto csrc/bond_graph.h, and
tests/test_gpu_analysis_bytes.py holds every later one to them.

The batches are those of the GPU tests (tests/molecule_utils.py, tls_utils.py, aniso_utils.py and the dense-segment,
ragged and edgeless cases of test_gpu_bond_test.py); ``cases`` says what each one holds and checks that it does.

usage: python tools/analysis_bytes.py [--out tests/golden/analysis_bytes.json]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

STRETCH, BEND = 0.005, 0.020


def cases() -> dict:
    """name -> ``(batch, u, row_ptr)`` on the GPU:
      dense_segment  atom 0 has more than 64 incoming edges and its only bond lies beyond edge 64: the fold takes passes
      ragged         crystals of 0, 1, 65, 130 and 7 rows, hydrogens interleaved (an atom's index is not its row)
      no_edges       one atom, no edge
      pairs          molecules of 1, 2, 17, 65 and 130 atoms, a periodic polymer, and a chain cut open
      tls            every size class and rank of the TLS fit, a crystal without rows in the middle
      aniso          every source code: a methyl group, an orphan hydrogen, hydrogens through a cell face (radius 10)"""
    import numpy as np
    import torch

    import aniso_utils as au
    import molecule_utils as mu
    import tls_utils as tu
    from test_gpu_bond_test import ROWS, _cubic, _make, _random_crystal
    out = {}
    # test_the_only_bond_sits_beyond_edge_64_of_a_dense_segment
    rng = np.random.default_rng(7)
    centre = np.array([4.0, 4.0, 4.0])
    pts = rng.random((400, 3)) * 8.0
    pts = pts[np.linalg.norm(pts - centre, axis=1) > 2.5][:90]
    pos = np.concatenate([centre[None], pts, (centre + [0.9, 0.8, 0.9])[None]])
    z = np.array([6] + [6 if k % 3 else 1 for k in range(90)] + [6])
    out["dense_segment"] = _make([(pos, _cubic(8.0), z)], 3)
    src, tgt = out["dense_segment"][0]["edge_index"].cpu().numpy()
    partner = np.nonzero(src[tgt == 0] == len(z) - 1)[0]           # the only atom within bonding range of atom 0
    assert int((tgt == 0).sum()) > 64 and len(partner) == 1 and partner[0] >= 64
    out["ragged"] = _make([_random_crystal(n, h, 100 + k) for k, (n, h) in enumerate(zip(ROWS, (3, 2, 30, 60, 4)))], 2)
    assert ROWS[0] == 0
    out["no_edges"] = _make([(np.array([[1.0, 2.0, 3.0]]), _cubic(12.0), np.array([6]))], 4)
    assert out["no_edges"][0]["edge_index"].shape[1] == 0
    # the fixture of test_gpu_molecule_test.py: one direction of the last chain cut, so its two halves are open
    batch, u, row_ptr = _make(mu.pair_test_crystals(), 31)
    src, tgt = batch["edge_index"]
    first = int(batch["ptr"][3])
    keep = ~((src == first + 1) & (tgt == first + 2))
    assert int((~keep).sum()) == 1
    out["pairs"] = (dict(batch, edge_index=batch["edge_index"][:, keep].contiguous(), cart_dist=batch["cart_dist"][keep],
                         cart_dir=batch["cart_dir"][keep]), u, row_ptr)
    crystals, rows = tu.gpu_crystals()
    out["tls"] = _make(crystals, 0, u=torch.from_numpy(rows))
    crystals, rows = au.gpu_crystals()
    out["aniso"] = _make(crystals, 0, radius=10.0, u=torch.from_numpy(rows))
    return out


def digest(t) -> str:
    a = t.detach().cpu().contiguous().numpy()
    return hashlib.sha256(f"{a.dtype} {a.shape} ".encode() + a.tobytes()).hexdigest()


def run() -> dict:
    """name of the case -> "<entry point>.<field>" -> sha256 of the array (dtype, shape and bytes)."""
    import molecule_utils as mu
    from cartnet_amd import metrics as gm
    out = {}
    for name, (batch, u, row_ptr) in cases().items():
        u_eq = ((u[:, 0, 0] + u[:, 1, 1] + u[:, 2, 2]) / 3).contiguous()
        rh = gm.riding_h(u_eq, batch)
        mo = gm.molecules(batch, row_ptr, mu.TOL, rows=int(u.shape[0]))
        tf = gm.tls_fit(u, batch, row_ptr, mo)
        results = {"bond_test": gm.bond_test(u, batch, row_ptr, mu.TOL, mu.THRESHOLD), "riding_h": rh, "molecules": mo,
                   "molecule_test": gm.molecule_test(u, batch, row_ptr, mo, mu.THRESHOLD), "tls_fit": tf,
                   "aniso_h": gm.aniso_h(u, batch, row_ptr, rh, mo, tf, STRETCH, BEND),
                   "aniso_h_bare": gm.aniso_h(u, batch, row_ptr, rh, stretch=STRETCH, bend=BEND)}
        out[name] = {f"{entry}.{field}": digest(getattr(res, field)) for entry, res in results.items()
                     for field in res._fields}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    text = json.dumps(run(), indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")

"""Molecules and the rigid-body test on the host: the flags, the keys, the two entry points' declaration and binding and
their returns that need no launch, and ``bonds.molecules_host`` on hand-checked graphs (no GPU)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_defaults_and_old_defaults_stay():
    import main as entry
    p = entry.build_parser()
    d = p.parse_args([])
    assert (d.rigid_molecule, d.rigid_molecule_threshold, d.bond_tolerance) == (False, 1e-3, 0.4)
    assert (d.rigid_bond, d.rigid_bond_threshold, d.riding_h, d.predict_temperatures) == (False, 1e-3, False, None)
    assert (d.rotations, d.eval_batch, d.predict, d.inference, d.predict_output) == (1, 1, False, False, "./predictions.pkl")
    a = p.parse_args(["--rigid_molecule", "--bond_tolerance", "0.25", "--rigid_molecule_threshold", "5e-4"])
    assert (a.rigid_molecule, a.bond_tolerance, a.rigid_molecule_threshold, a.rigid_bond_threshold) == (True, 0.25, 5e-4, 1e-3)
    off = {"rigid_bond": None, "riding_h": None}                                         # always given; the later flags add a keyword or none
    assert entry.analysis_options(d) == off and entry.analysis_options(a) == {**off, "rigid_molecule": (0.25, 5e-4)}


def test_keys():
    from cartnet_amd import predict as p
    assert p.MOL_KEYS == ("mol", "mol_size", "mol_status", "mol_pos", "mol_pairs", "mol_delta_mean", "mol_delta_max",
                          "mol_worst", "mol_over", "mol_stats")
    assert not set(p.MOL_KEYS) & set(p.KEYS + p.SYM_KEYS + p.ROT_KEYS + p.BOND_KEYS + p.H_KEYS + p.H_SYM_KEYS + p.SERIES_KEYS)
    assert tuple(p.MOL_SPLIT) == p.MOL_KEYS and set(p.MOL_SPLIT.values()) == {"row", "crystal"}       # no "atom" key
    assert [k for k, v in p.MOL_SPLIT.items() if v == "crystal"] == ["mol_stats"]
    assert not set(p.MOL_SPLIT) & set(p.SPLIT)


@pytest.mark.parametrize("name, count", [("cartnet_molecules", 22), ("cartnet_adp_molecule_test", 19)])
def test_entry_points_are_declared_bound_and_built(name, count):
    from cartnet_amd import lib
    from cartnet_amd.build import SOURCES
    hdr = open(os.path.join(ROOT, "include", "cartnet_hip.h")).read()
    assert "Rosenfield, Trueblood & Dunitz" in hdr
    block = hdr[:hdr.index(f"int {name}(")].rsplit("/*", 1)[1]
    assert "main.py:47-49" in block                                           # the reference-site comment of its neighbours
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m and len(m.group(1).split(",")) == count == len(lib.PROTOTYPES[name][1])
    assert "struct" not in m.group(1)                                         # plain arguments
    assert "molecule_ops.hip" in SOURCES and os.path.exists(os.path.join(ROOT, "cartnet_amd", "csrc", "molecule_ops.hip"))
    assert lib.ABI_VERSION == 16 == lib.load().cartnet_abi_version()          # no struct changed


def test_no_launch_and_refusal_returns():
    from cartnet_amd import lib
    l = lib.load()
    f, nul, out = l.cartnet_molecules, [None] * 9, [None] * 7
    assert f(*nul, 97, 0.4, 4, 10, 0, 50, *out) == 0                          # no rows
    assert f(*nul, 97, 0.4, 0, 10, 5, 50, *out) == 0                          # no crystals
    assert f(*nul, 97, 0.4, 4, 0, 5, 50, *out) == 0                           # no atoms
    for bad in ((-1, 10, 5, 50), (4, -1, 5, 50), (4, 10, -1, 50), (4, 10, 5, -1)):
        assert f(*nul, 97, 0.4, *bad, *out) != 0
        assert b"cartnet_molecules: bad sizes" in l.cartnet_last_error()
    assert f(*nul, -1, 0.4, 4, 10, 5, 50, *out) != 0 and b"bad sizes" in l.cartnet_last_error()
    assert f(*nul, 97, float("nan"), 4, 10, 5, 50, *out) != 0
    assert b"must be a number" in l.cartnet_last_error()
    assert f(*nul, 97, 0.4, 4, 10, 5, 50, *out) != 0                          # before any launch
    assert b"cartnet_molecules: null pointer" in l.cartnet_last_error()
    f, nul, out = l.cartnet_adp_molecule_test, [None] * 8, [None] * 7
    assert f(*nul, 1e-3, 4, 10, 0, *out) == 0
    assert f(*nul, 1e-3, 0, 10, 5, *out) == 0
    assert f(*nul, 1e-3, 4, 0, 5, *out) == 0
    for bad in ((-1, 10, 5), (4, -1, 5), (4, 10, -1)):
        assert f(*nul, 1e-3, *bad, *out) != 0
        assert b"cartnet_adp_molecule_test: bad sizes" in l.cartnet_last_error()
    assert f(*nul, float("nan"), 4, 10, 5, *out) != 0
    assert b"must be a number" in l.cartnet_last_error()
    assert f(*nul, 1e-3, 4, 10, 5, *out) != 0                                 # before any launch
    assert b"cartnet_adp_molecule_test: null pointer" in l.cartnet_last_error()


def test_the_flag_is_refused_without_predict_or_inference(monkeypatch):
    import main as entry

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(entry.cdist, "init_from_env", touched)
    monkeypatch.setattr(entry, "create_model", touched)
    for extra in ([], ["--montecarlo"], ["--rigid_bond"]):
        with pytest.raises(SystemExit, match="--rigid_molecule serves --predict and --inference only"):
            entry.main(["--rigid_molecule"] + extra)
    with pytest.raises(SystemExit, match="does not serve --model icomformer"):      # --predict's own refusal stays
        entry.main(["--rigid_molecule", "--predict", "--model", "icomformer", "--checkpoint_path", "x", "--predict_input",
                    "y.cnshard"])
    from cartnet_amd.config import set_cfg
    set_cfg()


def test_metrics_surface():
    import torch
    from cartnet_amd import metrics
    assert metrics.Molecules._fields == ("label", "x", "mol", "size", "status", "crystal_counts")
    assert metrics.MoleculeTest._fields == ("pairs", "delta_sum", "delta_max", "worst", "over", "crystal_stats")
    with pytest.raises(ValueError, match="a forward has overwritten"):
        metrics.molecules({}, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="u must be"):
        metrics.molecule_test(torch.zeros(2, 3, 3, dtype=torch.float64), {}, torch.zeros(2, dtype=torch.int64), None)


# ---- molecules_host on graphs written down by hand: every directed edge is given with its distance and direction

def _graph(pos, cell, pairs):
    """Directed edges both ways for ``pairs`` = [(i, j, image of j as integer cell offsets)]: edge j -> i holds
    ``pos_i - (pos_j + image @ cell)``, as the radius graph stores it; sorted by target."""
    pos, cell = np.asarray(pos, dtype=np.float64), np.asarray(cell, dtype=np.float64)
    edges = []
    for i, j, image in pairs:
        shift = np.asarray(image, dtype=np.float64) @ cell
        edges.append((i, j, pos[i] - (pos[j] + shift)))                       # j -> i
        edges.append((j, i, pos[j] - (pos[i] - shift)))                       # i -> j
    edges.sort(key=lambda e: e[0])
    tgt, src = (np.array([e[k] for e in edges], dtype=np.int64) for k in (0, 1))
    vec = np.array([e[2] for e in edges])
    dist = np.linalg.norm(vec, axis=1)
    return np.stack([src, tgt]), dist.astype(np.float32), (vec / dist[:, None]).astype(np.float32)


def test_two_bonded_carbons_and_one_apart():
    from cartnet_amd.bonds import molecules_host
    pos = [[5.0, 5.0, 5.0], [6.54, 5.0, 5.0], [5.0, 7.4, 5.0]]                # 1.54 A: a bond; 2.4 A: none
    ei, dist, dirs = _graph(pos, np.eye(3) * 20, [(0, 1, (0, 0, 0)), (0, 2, (0, 0, 0))])
    got = molecules_host([6, 6, 6], ei, dist, dirs, [0, 1, 2])
    assert got["label"].tolist() == [0, 0, 2] and got["mol"].tolist() == [0, 0, 1]
    assert got["size"].tolist() == [2, 2, 1] and got["status"].tolist() == [0, 0, 0]
    assert got["crystal_counts"].tolist() == [[2.0, 1.0, 0.0, 0.0, 2.0]] and got["sweeps"].tolist() == [2]
    assert np.abs(got["x"] - [[0, 0, 0], [1.54, 0, 0], [0, 0, 0]]).max() < 1e-6
    assert got["label"].dtype == np.int64 and got["x"].dtype == np.float64 and got["mol"].dtype == np.int32
    # hydrogens interleaved have no row and no label; the rows are those of the carbons
    got = molecules_host([6, 1, 6, 6], *_graph([pos[0], [5, 5, 6.0], pos[1], pos[2]], np.eye(3) * 20,
                                               [(0, 2, (0, 0, 0)), (0, 1, (0, 0, 0))]), [0, -1, 1, 2])
    assert got["label"].tolist() == [0, -1, 0, 3] and got["mol"].tolist() == [0, 0, 1] and got["size"].tolist() == [2, 2, 1]


def test_a_chain_across_a_cell_face_is_unwrapped():
    """C0 - C1 - C2 along a in a 10 A cell with C1 - C2 through the face: C2 is stored at 0.3 A, its bonded image sits at
    10.3 A.  x is the unwrapped geometry relative to atom 0, which pins the sign of the stored direction."""
    from cartnet_amd.bonds import molecules_host
    pos = [[7.5, 2.0, 2.0], [8.9, 2.0, 2.0], [0.3, 2.0, 2.0]]
    ei, dist, dirs = _graph(pos, np.eye(3) * 10, [(0, 1, (0, 0, 0)), (1, 2, (1, 0, 0))])
    assert np.allclose(dist, 1.4, atol=1e-6)
    got = molecules_host([6, 6, 6], ei, dist, dirs, [0, 1, 2])
    assert got["label"].tolist() == [0, 0, 0] and got["status"].tolist() == [0, 0, 0] and got["sweeps"].tolist() == [3]
    assert np.abs(got["x"] - [[0, 0, 0], [1.4, 0, 0], [2.8, 0, 0]]).max() < 1e-6          # not 0.3 - 7.5 = -7.2
    assert got["crystal_counts"].tolist() == [[1.0, 1.0, 0.0, 0.0, 3.0]]


def test_a_chain_bonded_through_the_face_is_periodic():
    """Two atoms per cell along a, 1.5 A apart inside the cell and 1.5 A through the face of a 3 A cell: following the
    bonds leads to the atom's own image, one lattice translation away."""
    from cartnet_amd.bonds import MOLECULE_PERIODIC, molecules_host
    pos = [[0.5, 5.0, 5.0], [2.0, 5.0, 5.0]]
    cell = np.diag([3.0, 20.0, 20.0])
    ei, dist, dirs = _graph(pos, cell, [(0, 1, (0, 0, 0)), (0, 1, (-1, 0, 0))])
    got = molecules_host([6, 6], ei, dist, dirs, [0, 1])
    assert got["label"].tolist() == [0, 0] and got["status"].tolist() == [MOLECULE_PERIODIC] * 2
    assert got["crystal_counts"].tolist() == [[1.0, 0.0, 1.0, 0.0, 2.0]]
    # one atom per cell bonds only to its own image: no bond, a single atom
    ei = np.array([[0, 0], [0, 0]])
    got = molecules_host([6], ei, np.float32([1.5, 1.5]), np.float32([[1, 0, 0], [-1, 0, 0]]), [0])
    assert got["size"].tolist() == [1] and got["status"].tolist() == [0]


def test_a_missing_direction_opens_both_molecules_and_crystals_are_numbered_apart():
    from cartnet_amd.bonds import MOLECULE_OPEN, molecules_host
    pos = [[5.0, 5.0, 5.0], [6.5, 5.0, 5.0], [5.0, 9.0, 5.0], [6.5, 9.0, 5.0]]
    ei, dist, dirs = _graph(pos, np.eye(3) * 20, [(0, 1, (0, 0, 0)), (2, 3, (0, 0, 0))])
    keep = ~((ei[0] == 0) & (ei[1] == 1))                                     # drop 0 -> 1: atom 1 never hears of atom 0
    got = molecules_host([6] * 4, ei[:, keep], dist[keep], dirs[keep], [0, 1, 2, 3])
    assert got["label"].tolist() == [0, 1, 2, 2] and got["status"].tolist() == [MOLECULE_OPEN] * 2 + [0, 0]
    assert got["crystal_counts"].tolist() == [[3.0, 1.0, 0.0, 2.0, 2.0]]
    # the same four atoms as two crystals: the numbering starts again in each
    two = molecules_host([6] * 4, ei, dist, dirs, [0, 1, 2, 3], ptr=[0, 2, 4])
    assert two["mol"].tolist() == [0, 0, 0, 0] and two["label"].tolist() == [0, 0, 2, 2]
    assert two["crystal_counts"].tolist() == [[1.0, 1.0, 0.0, 0.0, 2.0]] * 2 and two["sweeps"].tolist() == [2, 2]

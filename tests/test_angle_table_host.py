"""The angle and torsion tables of ``cartnet_amd.bonds`` in numpy (``angle_table_host``) on graphs built on the host:
against a brute-force triple loop with the counts of every crystal, known geometry within the bound the fp32 inputs give,
the libration columns in closed form, a capped graph; then the surface around it: the three entry points' declarations and
bindings, the keys of a result, the flag and the two rows of ``STATISTICS``."""
import os
import re

import numpy as np
import pytest

import angle_table_utils as at
import molecule_utils as mu
import tls_utils as tu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CRYSTALS = at.counted_crystals()
# name -> (angles, torsions, torsions with a == d, undefined torsions): radius 5, tolerance 0.4
COUNTS = {"small": (15, 14, 0, 0), "long": (191, 189, 0, 0), "polymer": (8, 8, 0, 0), "five": (3, 2, 0, 0),
          "star": (666, 5082, 366, 0), "images": (2, 2, 0, 2), "helix": (5, 4, 0, 0), "planar": (6, 5, 0, 0),
          "3-ring": (3, 3, 3, 0)}


def _tables(pos, cell, z, radius=5.0, max_neighbors=None, **kw):
    from cartnet_amd.bonds import angle_table_host
    z = np.asarray(z, dtype=np.int64)
    ei, dist, dirs = at.graph(pos, cell, radius, max_neighbors)
    atom_row = mu.atom_rows(z != 1)
    return angle_table_host(z, ei, dist, dirs, atom_row, **kw), (ei, dist, dirs, atom_row)


def _against_the_loops(got, z, ei, dist, dirs, atom_row):
    angles, torsions, reverse, nearest, wrong = at.brute_force(z, ei, dist, dirs, atom_row)
    A, T = got["angles"], got["torsions"]
    assert [tuple(r) for r in zip(A["a"], A["b"], A["c"])] == [r[:3] for r in angles]
    assert [tuple(r) for r in zip(T["a"], T["b"], T["c"], T["d"])] == [r[:4] for r in torsions]
    assert got["bond_edge"].tolist() == list(reverse) and got["reverse"].tolist() == list(reverse.values())
    assert all(k.dtype == np.int64 for k in (A["a"], A["b"], A["c"], T["a"], T["b"], T["c"], T["d"]))
    assert A["value"].dtype == T["value"].dtype == A["libration"].dtype == np.float32 and A["tls_rank"].dtype == np.int32
    d = got["degree"]
    assert np.array_equal(got["angle_counts"], d * (d - 1) // 2) and got["angle_ptr"].tolist() == [0, len(angles)]
    assert got["torsion_counts"].sum() == len(torsions) and got["torsion_ptr"].tolist() == [0, len(torsions)]
    # the values against fp64 vector algebra on the same edges: acos, and the torsion as the signed angle of the two end
    # vectors' parts across the central bond
    u = dirs.astype(np.float64)
    u = u / np.linalg.norm(u, axis=1, keepdims=True)                          # the stored ones are unit to fp32 only
    if angles:
        e1, e2 = (np.array([r[k] for r in angles]) for k in (3, 4))
        cos = np.clip((u[e1] * u[e2]).sum(1), -1.0, 1.0)
        away = np.abs(cos) < 0.99                                                         # acos is fine away from 0 and 180
        plain = np.degrees(np.arccos(cos[away]))
        assert not away.any() or np.abs(A["value"][away] - plain).max() <= np.spacing(np.float32(180.0))
    if torsions:
        ea, e0, ed = (np.array([r[k] for r in torsions]) for k in (4, 5, 6))
        axis = u[e0]
        pa = -u[ea] - (-u[ea] * axis).sum(1, keepdims=True) * axis                        # b -> a across the bond b -> c
        pd = -u[ed] - (-u[ed] * axis).sum(1, keepdims=True) * axis                        # c -> d across it
        la, ld = np.linalg.norm(pa, axis=1), np.linalg.norm(pd, axis=1)
        well = (la > 0.1) & (ld > 0.1)                                                    # both ends well off the axis
        assert np.array_equal(np.isnan(T["value"]), (la == 0.0) | (ld == 0.0))
        plain = np.degrees(np.arctan2((np.cross(pa, pd) * axis).sum(1), (pa * pd).sum(1)))[well]
        assert not well.any() or at.circular(T["value"][well], plain).max() <= np.spacing(np.float32(180.0))
    return len(angles), len(torsions), nearest, wrong


@pytest.mark.parametrize("name", list(COUNTS))
def test_against_a_triple_loop_with_the_counts_of_every_crystal(name):
    pos, cell, z = CRYSTALS[name]
    got, (ei, dist, dirs, atom_row) = _tables(pos, cell, z)
    na, nt, nearest, wrong = _against_the_loops(got, np.asarray(z), ei, dist, dirs, atom_row)
    T = got["torsions"]
    print(f"{name}: {na} angles, {nt} torsions, {int((T['a'] == T['d']).sum())} with a == d, "
          f"{int(np.isnan(T['value']).sum())} undefined; reverse edges at {max(nearest.values()):.3g}, "
          f"nearest wrong candidate {wrong:.4g}")
    assert (na, nt, int((T["a"] == T["d"]).sum()), int(np.isnan(T["value"]).sum())) == COUNTS[name]
    # every listed bond found its reverse edge, at 0.0; no other candidate is anywhere near the 0.5 A of the rule
    assert (got["reverse"] >= 0).all() and max(nearest.values()) == 0.0 and (got["reverse_m"] == 0.0).all()
    assert wrong >= 2.75 and (wrong == 2.75) == (name == "images")
    if name == "star":
        assert got["degree"][-1] == 20
    if name == "images":
        assert got["angles"]["value"].tolist() == [180.0, 180.0]
    s, t = got["angle_stats"][0], got["torsion_stats"][0]
    assert s[0] == na and s[1] == pytest.approx(got["angles"]["value"].astype(np.float64).sum(), rel=1e-12)
    assert t[0] == nt and t[1] == COUNTS[name][3] and s[2:].tolist() == t[2:].tolist() == [0.0] * 3   # no TLS results
    assert np.isnan(got["angles"]["libration"]).all() and not got["torsions"]["tls_rank"].any()


def test_the_branched_centre():
    pos, cell, z = at.branched()
    got, (ei, dist, dirs, atom_row) = _tables(pos, cell, z)
    na, nt, nearest, wrong = _against_the_loops(got, z, ei, dist, dirs, atom_row)
    assert got["degree"].tolist() == [2, 1, 1, 1, 1, 4] and (na, nt) == (7, 3) and wrong == np.inf


def _direction_bound(pos, bond):
    """How far (radians) a stored unit direction can lie from the exact one: both ends rounded to fp32 (half a spacing of
    the largest coordinate each) and their difference rounded once more, over the bond length, in three components; then
    the fp32 norm, division and storage of the unit vector, three roundings of half a unit of 1.0 per component."""
    s = float(np.spacing(np.float32(np.abs(pos).max())))
    return np.sqrt(3.0) * (1.5 * s / bond + 1.5 * float(np.spacing(np.float32(1.0))))


def _angle_bound(pos, bond, value):
    """Degrees: two directions off by ``_direction_bound``, and the rounding of the stored fp32 value."""
    return np.degrees(2.0 * _direction_bound(pos, bond)) + 0.5 * float(np.spacing(np.float32(abs(value))))


def _torsion_bound(pos, bond, bond_angle_deg, value):
    """Degrees: a torsion is the angle of the normals ``b1 x b2`` and ``b2 x b3``; a normal turns by at most the sum of its
    two directions' errors over the sine of their angle."""
    return (np.degrees(4.0 * _direction_bound(pos, bond) / np.sin(np.radians(bond_angle_deg)))
            + 0.5 * float(np.spacing(np.float32(abs(value)))))


def _rotated(pos, cell, seed):
    """The crystal turned about the middle of its cell."""
    R, mid = tu.rotation(seed), 0.5 * np.asarray(cell).sum(0)
    return (pos - mid) @ R + mid @ R, np.asarray(cell) @ R


def test_known_angles_and_their_rotation():
    want = np.degrees(np.arccos(-1.0 / 3.0))
    for (pos, cell, z), n, exact in ((at.tetrahedral(), 6, want), (at.three_ring(), 3, 60.0)):
        got, _ = _tables(pos, cell, z)
        value = got["angles"]["value"].astype(np.float64)
        bound = _angle_bound(pos, 1.5, exact)
        print(f"{n} angles of {exact:.6f}: worst {np.abs(value - exact).max():.3e}, bound {bound:.3e}")
        assert len(value) == n and np.abs(value - exact).max() <= bound
        for seed in (1, 2):
            rpos, rcell = _rotated(pos, cell, seed)
            turned, _ = _tables(rpos, rcell, z)
            bound = _angle_bound(np.concatenate([pos, rpos]), 1.5, exact)
            assert np.array_equal(turned["angles"]["b"], got["angles"]["b"])
            assert np.abs(turned["angles"]["value"].astype(np.float64) - value).max() <= bound


@pytest.mark.parametrize("torsion,mirror,want", [(60.0, False, 60.0), (60.0, True, -60.0), (180.0, False, 180.0),
                                                 (-135.0, False, -135.0), (0.0, False, 0.0)])
def test_known_torsions_their_sign_and_their_rotation(torsion, mirror, want):
    pos, cell, z = at.chain4(torsion, mirror=mirror)
    got, _ = _tables(pos, cell, z)
    T = got["torsions"]
    assert list(zip(T["a"], T["b"], T["c"], T["d"])) == [(0, 1, 2, 3)] and len(got["angles"]["a"]) == 2
    value = float(T["value"][0])
    bound = _torsion_bound(pos, 1.5, 110.0, want)
    print(f"torsion {want}: got {value!r}, off by {at.circular(value, want):.3e}, bound {bound:.3e}")
    assert at.circular(value, want) <= bound and value > -180.0                       # a trans chain: 180, never -180
    if want == 180.0:
        assert value > 0.0
    assert np.abs(got["angles"]["value"].astype(np.float64) - 110.0).max() <= _angle_bound(pos, 1.5, 110.0)
    for seed in (3, 4):
        rpos, rcell = _rotated(pos, cell, seed)
        turned, _ = _tables(rpos, rcell, z)
        bound = _torsion_bound(np.concatenate([pos, rpos]), 1.5, 110.0, want)
        assert at.circular(turned["torsions"]["value"][0], value) <= bound and turned["torsions"]["value"][0] > -180.0


def test_an_isotropic_libration_changes_nothing():
    """``L = lambda I``: ``v' = (1 + lambda) v`` for every vector, up to the rounding of the products, and neither formula
    depends on the scale."""
    for pos, cell, z in (CRYSTALS["helix"], CRYSTALS["small"], at.branched()):
        n = len(z)
        params = np.full((n, 24), 7.0, dtype=np.float32)                                  # T, S and the origin do not enter
        params[:, 6:9], params[:, 9:12] = 0.01, 0.0
        got, _ = _tables(pos, cell, z, params=params, rank=np.full(n, 20, dtype=np.int32))
        for table in (got["angles"], got["torsions"]):
            assert len(table["a"]) and np.isfinite(table["libration"]).all() and set(table["tls_rank"]) == {20}
            assert at.bu.ulps(table["libration"], table["value"]).max() <= 1


def test_a_libration_about_z_against_the_closed_form():
    """Two hand-placed bonds at a centre: ``L = diag(0, 0, lambda)`` maps a vector by ``diag(1 + lambda/2, 1 + lambda/2,
    1)``.  The centre has the highest index, so both bonds are listed and its row decides."""
    lam = 0.02
    c = np.array([10.0, 10.0, 10.0])
    p, q = np.array([1.5, 0.0, 0.0]), np.array([-0.5, 0.0, 1.375])                        # in the xz plane: the map shears it
    pos = np.stack([c - p, c - q, c])
    params = np.zeros((3, 24), dtype=np.float32)
    params[:, 8] = lam
    got, (ei, dist, dirs, _) = _tables(pos, mu.cubic(20.0), np.full(3, 6), params=params,
                                      rank=np.array([0, 0, 19], dtype=np.int32))
    A = got["angles"]
    assert list(zip(A["a"], A["b"], A["c"])) == [(0, 2, 1)] and A["tls_rank"].tolist() == [19]
    scale = np.array([1.0 + np.float64(params[0, 8]) / 2.0] * 2 + [1.0])
    pl, ql = p * scale, q * scale
    want = np.degrees(np.arctan2(np.linalg.norm(np.cross(pl, ql)), pl @ ql))
    raw = np.degrees(np.arctan2(np.linalg.norm(np.cross(p, q)), p @ q))
    bound = _angle_bound(pos, 1.5, want)
    assert abs(float(A["value"][0]) - raw) <= bound and abs(raw - want) > 0.1 > 100 * bound    # the libration changes the angle
    assert abs(float(A["libration"][0]) - want) <= bound
    far = params.copy()
    far[:2, 6:12] = 0.5                                                                   # the rows of a and c are not read
    other, _ = _tables(pos, mu.cubic(20.0), np.full(3, 6), params=far, rank=np.array([20, 20, 19], dtype=np.int32))
    assert other["angles"]["libration"].tobytes() == A["libration"].tobytes()
    # a torsion: a chain a-b-c-d with b-c along x; rotating about z mixes x and y and leaves z
    pos, cell, z = at.chain4(60.0)
    params = np.zeros((4, 24), dtype=np.float32)
    params[:, 8] = lam
    rank = np.array([0, 0, 20, 0], dtype=np.int32)                                        # row c decides
    got, (ei, dist, dirs, _) = _tables(pos, cell, z, params=params, rank=rank)
    T = got["torsions"]
    b1, b2, b3 = ((pos[k + 1] - pos[k]) * scale for k in range(3))
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    want = np.degrees(np.arctan2(np.linalg.norm(b2) * (b1 @ n2), n1 @ n2))
    assert T["tls_rank"].tolist() == [20] and abs(want - 60.0) > 0.1
    assert abs(float(T["libration"][0]) - want) <= _torsion_bound(pos, 1.5, 110.0, want)
    assert np.isnan(got["angles"]["libration"][0]) and got["angles"]["tls_rank"].tolist() == [0, 20]   # centres b, then c
    pl, ql = (pos[1] - pos[2]) * scale, (pos[3] - pos[2]) * scale                         # the angle b-c-d at the fitted c
    want_c = np.degrees(np.arctan2(np.linalg.norm(np.cross(pl, ql)), pl @ ql))
    assert abs(want_c - 110.0) > 0.1 and abs(float(got["angles"]["libration"][1]) - want_c) <= _angle_bound(pos, 1.5, want_c)
    assert got["angle_stats"][0, 2] == 1 and got["torsion_stats"][0, 2] == 1
    assert got["torsion_stats"][0, 4] == abs(np.float64(T["libration"][0]) - np.float64(T["value"][0]))


def test_without_a_fit_the_libration_is_nan_and_the_rank_is_kept():
    pos, cell, z = CRYSTALS["five"]
    params = np.full((5, 24), np.nan, dtype=np.float32)
    got, _ = _tables(pos, cell, z, params=params, rank=np.array([0, -1, 0, -1, 0], dtype=np.int32))
    assert np.isnan(got["angles"]["libration"]).all() and np.isnan(got["torsions"]["libration"]).all()
    assert got["angles"]["tls_rank"].tolist() == [-1, 0, -1] and got["torsions"]["tls_rank"].tolist() == [0, -1]
    bare, _ = _tables(pos, cell, z)
    assert not bare["angles"]["tls_rank"].any() and bare["angles"]["value"].tobytes() == got["angles"]["value"].tobytes()
    with pytest.raises(ValueError, match="together"):
        _tables(pos, cell, z, params=params)
    undefined, _ = _tables(*CRYSTALS["images"], params=np.zeros((2, 24), np.float32), rank=np.full(2, 20, np.int32))
    assert np.isnan(undefined["torsions"]["libration"]).all() and undefined["angles"]["libration"].tolist() == [180.0] * 2


def test_a_capped_graph_and_a_bond_without_its_reverse_edge():
    """Under a cap of two neighbours the rule still agrees with the loops; and the chain of 5 with the edges INTO atom 1
    removed holds 1 - 2 only as 1 -> 2: that listed bond has no reverse edge, so nothing is excluded on its ``a`` side."""
    from cartnet_amd.bonds import angle_table_host
    c = np.array([6.0, 6.0, 6.0])
    pos = mu.on_grid(np.stack([c, c + [-1.3125, 0, 0], c + [1.4375, 0, 0], c + [0, 1.5, 0], c + [0, -1.5625, 0]]))
    for order in ((0, 1, 2, 3, 4), (4, 1, 2, 3, 0)):
        got, (ei, dist, dirs, atom_row) = _tables(pos[list(order)], mu.cubic(12.0), np.full(5, 6), max_neighbors=2)
        assert ei.shape[1] == 15                                                          # three of four kept per atom
        na, nt, nearest, wrong = _against_the_loops(got, np.full(5, 6), ei, dist, dirs, atom_row)
        assert na == 3 and (got["reverse"] < 0).sum() == (1 if order[0] == 0 else 0)     # B - F is held as B -> F only
    pos, cell, z = CRYSTALS["five"]
    full = at.graph(pos, cell)
    for keep, degree, counts, torsions in (
            (full[0][1] != 1, [1, 0, 2, 2, 1], [0, 1, 0], [(1, 2, 3, 4)]),                # no edge into 1: 0 - 1 is not listed
            (~((full[0][0] == 2) & (full[0][1] == 1)), [1, 1, 2, 2, 1], [0, 1, 1, 0], [(0, 1, 2, 3), (1, 2, 3, 4)])):
        ei, dist, dirs = full[0][:, keep], full[1][keep], full[2][keep]
        got = angle_table_host(z, ei, dist, dirs, np.arange(5))
        _against_the_loops(got, z, ei, dist, dirs, np.arange(5))
        T = got["torsions"]
        assert got["degree"].tolist() == degree and got["torsion_counts"].tolist() == counts
        k = len(counts) - 3                                                               # the bond 1 -> 2
        assert got["reverse"][k] == -1 and (np.delete(got["reverse"], k) >= 0).all()
        assert list(zip(T["a"], T["b"], T["c"], T["d"])) == torsions                      # 0 -> 1 stays on the a side of 1 - 2


def test_the_entry_points_are_declared_bound_and_built():
    from cartnet_amd import lib
    from cartnet_amd.build import EXTRA_FLAGS, SOURCES
    hdr = open(os.path.join(ROOT, "include", "cartnet_hip.h")).read()
    block = hdr[:hdr.index("int cartnet_bond_adjacency(")].rsplit("/*", 1)[1]
    assert all(w in block for w in ("angle_table_host", "cartnet_angle_table_count ", "cartnet_adp_angle_table ", "IUPAC",
                                    "libration"))
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, count in (("cartnet_bond_adjacency", 17), ("cartnet_angle_table_count", 14), ("cartnet_adp_angle_table", 37)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and len(m.group(1).split(",")) == count == len(lib.PROTOTYPES[name][1]), name
        assert "struct" not in m.group(1)                                                 # plain arguments
    assert "angle_table_ops.hip" in SOURCES and os.path.exists(os.path.join(ROOT, "cartnet_amd", "csrc", "angle_table_ops.hip"))
    assert "-ffp-contract=off" in EXTRA_FLAGS["angle_table_ops.hip"]
    assert "-ffp-contract=off" not in EXTRA_FLAGS.get("bond_table_ops.hip", []) + EXTRA_FLAGS.get("bond_ops.hip", [])
    source = open(os.path.join(ROOT, "cartnet_amd", "csrc", "angle_table_ops.hip")).read()
    assert "bg_form(" not in re.sub(r"//.*", "", source)                                  # nothing here may be contracted
    assert lib.ABI_VERSION == 16 == lib.load().cartnet_abi_version()                      # no struct changed
    so = lib.load()
    adjacency, count, fill = so.cartnet_bond_adjacency, so.cartnet_angle_table_count, so.cartnet_adp_angle_table
    assert adjacency(*[None] * 6, 97, 0.4, None, None, 0, 5, 50, 3, None, None, None) == 0      # no atoms
    assert adjacency(*[None] * 6, 97, 0.4, None, None, 10, 5, 50, 3, None, None, None) == 1     # null pointers: no fault
    assert adjacency(*[None] * 6, 97, float("nan"), None, None, 10, 5, 50, 3, None, None, None) == 1
    assert count(*[None] * 7, 0, 50, 3, None, None, None, None) == 0
    assert count(*[None] * 7, 10, 50, 3, None, None, None, None) == 1
    assert count(*[None] * 7, 10, 50, -1, None, None, None, None) == 1
    nul, out = [None] * 14, [None] * 15
    assert fill(*nul, 0, 10, 5, 50, 3, 7, 9, *out, None) == 0                             # no crystals
    assert fill(*nul, 2, 0, 5, 50, 3, 7, 9, *out, None) == 0                              # no atoms
    assert fill(*nul, 2, 10, 5, 50, 3, 7, 9, *out, None) == 1
    assert fill(*nul, 2, 10, 5, 50, 3, -1, 9, *out, None) == 1


def test_the_keys_of_a_result():
    from cartnet_amd import predict as p
    from cartnet_amd.predict import Analyses, result_keys
    angles = ("angles_a", "angles_b", "angles_c", "angles_value", "angles_libration", "angles_tls_rank", "angles_stats")
    torsions = ("torsions_a", "torsions_b", "torsions_c", "torsions_d", "torsions_value", "torsions_libration",
                "torsions_tls_rank", "torsions_stats")
    assert p.AT_KEYS == angles and p.TT_KEYS == torsions
    assert list(p.AT_SPLIT.items()) == [(k, "angle") for k in angles[:-1]] + [("angles_stats", "crystal")]
    assert list(p.TT_SPLIT.items()) == [(k, "torsion") for k in torsions[:-1]] + [("torsions_stats", "crystal")]
    assert all(p.CUT[k] == c for split in (p.AT_SPLIT, p.TT_SPLIT) for k, c in split.items())
    assert list(p.GROUPS)[-3:] == ["series", "angle_table", "torsion_table"]
    every = Analyses(rigid_bond=(0.4, 1e-3), riding_h=(0.4, 1.2, 1.5), rigid_molecule=(0.4, 1e-3), tls_fit=True,
                     aniso_h=(0.005, 0.020))
    for a, sym, K in ((Analyses(), False, 1), (every, True, 2), (every, False, 1)):
        off = result_keys(a, sym, K)
        assert result_keys(a, sym, K, None, None) == off and not [k for k in off if k.startswith(("angles_", "torsions_"))]
        assert result_keys(a, sym, K, angle_table=0.4) == off + angles + torsions         # last, in the stated order
        assert result_keys(a, sym, K, 0.4, 0.4) == result_keys(a, sym, K, 0.4) + angles + torsions     # after bonds_*
    assert Analyses() == (None,) * 5 and "angle_table" not in Analyses._fields


def test_the_statistics_rows():
    from cartnet_amd import predict as p
    assert list(p.STATISTICS)[-3:] == ["bonds_stats", "angles_stats", "torsions_stats"]
    width, figures = p.STATISTICS["angles_stats"]
    assert width == 5 and figures([12.0, 1320.0, 4.0, 0.5, 0.0], [0.0] * 4 + [0.25]) == {
        "angles_listed": 12, "angle_mean": 110.0, "angle_libration_angles": 4, "angle_libration_mean": 0.125,
        "angle_libration_max": 0.25}
    width, figures = p.STATISTICS["torsions_stats"]
    assert width == 5 and figures([10.0, 2.0, 4.0, 1.0, 0.0], [0.0] * 4 + [0.75]) == {
        "torsions_listed": 10, "torsions_undefined": 2, "torsion_libration_torsions": 4, "torsion_libration_mean": 0.25,
        "torsion_libration_max": 0.75}
    assert figures([0.0] * 5, [0.0] * 5)["torsion_libration_mean"] == 0.0
    out = {"name": ["a", "b"], "u_eq": [np.zeros(3), np.zeros(2)], "stats": [], "angles_stats": [], "torsions_stats": []}
    import torch
    out["u_eq"] = [torch.zeros(3), torch.zeros(2)]
    out["stats"] = [torch.zeros(3, dtype=torch.float64)] * 2
    out["angles_stats"] = [torch.tensor(r, dtype=torch.float64) for r in ([3.0, 330.0, 3.0, 0.3, 0.2], [1.0, 90.0, 0.0, 0.0, 0.0])]
    out["torsions_stats"] = [torch.tensor(r, dtype=torch.float64) for r in ([2.0, 0.0, 2.0, 0.5, 0.4], [0.0] * 5)]
    line = p.pass_statistics(out)
    assert list(line)[-10:] == ["angles_listed", "angle_mean", "angle_libration_angles", "angle_libration_mean",
                                "angle_libration_max", "torsions_listed", "torsions_undefined",
                                "torsion_libration_torsions", "torsion_libration_mean", "torsion_libration_max"]
    assert line["angles_listed"] == 4 and line["angle_mean"] == 105.0 and line["angle_libration_max"] == 0.2
    assert line["torsions_listed"] == 2 and line["torsion_libration_mean"] == 0.25 and line["torsion_libration_max"] == 0.4


def test_the_flag_is_refused_before_the_device_is_touched(monkeypatch):
    import main as entry

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(entry.cdist, "init_from_env", touched)
    monkeypatch.setattr(entry, "create_model", touched)
    with pytest.raises(SystemExit, match="--angle_table serves --predict only"):
        entry.main(["--angle_table"])
    with pytest.raises(SystemExit, match="--angle_table serves --predict only"):
        entry.main(["--angle_table", "--inference", "--rigid_molecule", "--tls_fit"])
    args = entry.build_parser().parse_args([])
    assert args.angle_table is False and entry.analysis_options(args) == {"rigid_bond": None, "riding_h": None}
    args = entry.build_parser().parse_args(["--angle_table", "--bond_tolerance", "0.3"])
    assert entry.analysis_options(args) == {"rigid_bond": None, "riding_h": None, "angle_table": 0.3}
    assert entry.analysis_options(args, inference=True) == {"rigid_bond": None}
    args = entry.build_parser().parse_args(["--angle_table", "--bond_table"])
    assert list(entry.analysis_options(args)) == ["rigid_bond", "riding_h", "bond_table", "angle_table"]

"""Shared by the angle-table tests: graphs of one crystal from ``synthetic.radius_graph_pbc_single``, the brute-force triple
loop the numpy rule is held to, the two crystals that only these tests need (a three-membered ring, a centre of degree 4),
the crystals of the counts table and the comparison of a kernel's tables with the rule's."""
import numpy as np

import bond_table_utils as bu
import molecule_utils as mu
import tls_utils as tu

ANGLE_COLUMNS = ("a", "b", "c", "value", "libration", "tls_rank")
TORSION_COLUMNS = ("a", "b", "c", "d", "value", "libration", "tls_rank")
VALUES = ("value", "libration")
CLOSURE = 0.5


def graph(pos, cell, radius=5.0, max_neighbors=None):
    """``(edge_index [2,E], cart_dist [E], cart_dir [E,3])`` as numpy arrays, sorted by target (stable: edge order kept)."""
    import torch
    from cartnet_amd.synthetic import radius_graph_pbc_single
    ei, dist, dirs = radius_graph_pbc_single(torch.tensor(np.asarray(pos), dtype=torch.float32),
                                             torch.tensor(np.asarray(cell), dtype=torch.float32), radius,
                                             max_neighbors=max_neighbors)
    ei, dist, dirs = ei.numpy(), dist.numpy(), dirs.numpy()
    order = np.argsort(ei[1], kind="stable")
    return ei[:, order], dist[order], dirs[order]


def three_ring(side=1.5):
    """Three carbons at the corners of an equilateral triangle, off the grid: every angle is 60 degrees."""
    h = side * np.sqrt(3.0) / 2.0
    return np.array([[10.0, 10.0, 10.0], [10.0 + side, 10.0, 10.0], [10.0 + side / 2.0, 10.0 + h, 10.0]]), mu.cubic(20.0), \
        np.full(3, 6)


def tetrahedral(bond=1.5, centre_first=False):
    """A carbon with four carbons at the corners of a tetrahedron around it, ``bond`` A away (the outer ones 2.45 A apart:
    not bonded): six angles of ``acos(-1/3)``.  The centre has the HIGHEST index unless ``centre_first``."""
    corners = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)
    outer, centre = 10.0 + bond * corners, [[10.0, 10.0, 10.0]]
    return np.concatenate([centre, outer] if centre_first else [outer, centre]), mu.cubic(20.0), np.full(5, 6)


def branched():
    """A centre of degree 4 inside a chain: the tetrahedral centre (last atom) with one more carbon on its first corner."""
    pos, cell, z = tetrahedral()
    out = pos[0] - 10.0
    extra = pos[0] + 1.5 * np.array([out[0], -out[1], out[2]]) / np.linalg.norm(out)
    return np.concatenate([pos[:4], [extra], pos[4:]]), cell, np.full(6, 6)


def chain4(torsion_deg, angle_deg=110.0, bond=1.5, mirror=False):
    """Four carbons a-b-c-d with both bond angles ``angle_deg`` and the torsion ``torsion_deg`` (IUPAC sign), built in fp64:
    b at the origin of a local frame, c along x.  ``mirror`` reflects the molecule in the xy plane."""
    th, ph = np.radians(angle_deg), np.radians(torsion_deg)
    b, c = np.zeros(3), np.array([bond, 0.0, 0.0])
    a = b + bond * np.array([np.cos(th), np.sin(th), 0.0])
    d = c + bond * np.array([-np.cos(th), np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph)])
    pos = np.stack([a, b, c, d])
    if mirror:
        pos[:, 2] = -pos[:, 2]
    return pos + 10.0, mu.cubic(24.0), np.full(4, 6)


def counted_crystals():
    """name -> (pos, cell, z): the crystals of the counts table."""
    small, long_, polymer, five = mu.pair_test_crystals()
    helix, planar = tu.helix(7, (3, 12, 12)), tu.planar_chain(8, (3, 3, 3))
    return {"small": small, "long": long_, "polymer": polymer, "five": five, "star": bu.star(), "images": bu.two_images(),
            "helix": (helix, mu.cubic(30.0), np.full(7, 6)), "planar": (planar, mu.cubic(30.0), np.full(8, 6)),
            "3-ring": three_ring()}


def brute_force(z, edge_index, cart_dist, cart_dir, atom_row, tol=mu.TOL):
    """The angles and torsions by loops over atoms and ALL edges, the reverse edge by the fp64 distance of the two bond
    vectors' sum from zero: ``(angles [(a, b, c, e1, e2)], torsions [(a, b, c, d, ea, e0, ed)], reverse {e0: edge or -1},
    nearest {e0: the distance of the accepted candidate}, wrong: the smallest distance of any other candidate)``."""
    from cartnet_amd.bonds import is_bond
    src, tgt = np.asarray(edge_index)
    E, N = len(src), len(z)
    v = cart_dist.astype(np.float64)[:, None] * cart_dir.astype(np.float64)
    bond = [atom_row[tgt[e]] >= 0 and atom_row[src[e]] >= 0
            and bool(is_bond(cart_dist[e], z[tgt[e]], z[src[e]], tol, same_atom=src[e] == tgt[e])) for e in range(E)]
    into = [[e for e in range(E) if tgt[e] == i and bond[e]] for i in range(N)]
    angles = [(src[e1], i, src[e2], e1, e2) for i in range(N) for x, e1 in enumerate(into[i]) for e2 in into[i][x + 1:]]
    torsions, reverse, nearest, wrong = [], {}, {}, np.inf
    for c in range(N):
        for e0 in into[c]:
            b = src[e0]
            if not b < c:
                continue
            gaps = {e: np.linalg.norm(v[e] + v[e0]) for e in into[b] if src[e] == c}
            rev = min(gaps, key=lambda e: (gaps[e], e)) if gaps else -1
            if rev >= 0 and not gaps[rev] < CLOSURE:
                rev = -1
            reverse[e0] = rev
            if rev >= 0:
                nearest[e0] = gaps[rev]
            wrong = min([wrong] + [g for e, g in gaps.items() if e != rev])
            for ea in into[b]:
                for ed in into[c]:
                    if ea != rev and ed != e0:
                        torsions.append((src[ea], b, c, src[ed], ea, e0, ed))
    return angles, torsions, reverse, nearest, wrong


def circular(got, want) -> np.ndarray:
    """``min(x, 360 - x)`` of ``x = |got - want|`` in fp64; NaN where either is."""
    x = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    return np.minimum(x, 360.0 - x)


def same_tables(got: dict, want: dict) -> dict:
    """Asserts what the tests ask of a kernel's two tables (``{"angles": {...}, "torsions": {...}}``) against the numpy
    rule's: indices and ``tls_rank`` bit for bit, NaNs in the same places, ``value`` and ``libration`` within one fp32 unit
    in the last place -- a torsion also when the two lie one unit apart across the cut at 180 (the circular distance is
    then at most one unit of 180).  Returns the largest distance per column in units in the last place."""
    worst = {}
    for table, columns in (("angles", ANGLE_COLUMNS), ("torsions", TORSION_COLUMNS)):
        for k in columns:
            g, w = np.asarray(got[table][k]), np.asarray(want[table][k])
            assert g.shape == w.shape and g.dtype == w.dtype, (table, k, g.shape, w.shape, g.dtype, w.dtype)
            if k not in VALUES:
                assert g.tobytes() == w.tobytes(), (table, k)
                continue
            assert np.array_equal(np.isnan(g), np.isnan(w)), (table, k)
            d = bu.ulps(g, w)
            if table == "torsions" and d.size:
                across = circular(g, w) <= np.spacing(np.float32(180.0))
                d = np.where(across & (d > 1), 1, d)
            worst[f"{table}_{k}"] = int(d.max()) if d.size else 0
            assert worst[f"{table}_{k}"] <= 1, (table, k, worst[f"{table}_{k}"])
    return worst

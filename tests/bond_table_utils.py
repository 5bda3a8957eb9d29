"""Shared by the bond-table tests: the brute-force double loop the numpy rule is held to, the crystals that only these
tests need (a star whose centre owns more than sixteen bonds, a cell so small that one pair is bonded through two
images) and the comparison of two fp32 columns to within one unit in the last place."""
import numpy as np

import molecule_utils as mu

COLUMNS = ("a", "b", "dir", "length", "delta", "lower", "upper", "libration", "tls_rank")
EXACT = ("a", "b", "dir", "length", "tls_rank")
# The columns whose fp64 expression holds products and sums that the device compiler may contract into fused
# multiply-adds (bond_table_ops.hip is compiled with bond_ops.hip's contraction setting, as the rule asks) and numpy
# may not: the two fp64 values can differ in their last bits, so the single rounding to fp32 can fall to either side.
ONE_ULP = ("delta", "lower", "upper", "libration")


def brute_force(z, edge_index, cart_dist, atom_row, tol=mu.TOL):
    """``(a, b, edge)`` of the listed bonds by a double loop: targets in order, each target's edges in edge order."""
    from cartnet_amd.bonds import is_bond
    src, tgt = np.asarray(edge_index)
    a, b, edges = [], [], []
    for i in range(len(z)):
        for e in range(len(src)):
            j = src[e]
            if tgt[e] != i or not j < i or atom_row[i] < 0 or atom_row[j] < 0:
                continue
            if bool(is_bond(cart_dist[e], z[i], z[j], tol, same_atom=i == j)):
                a.append(j)
                b.append(i)
                edges.append(e)
    return np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(edges, dtype=np.int64)


def star(n=20, bond=1.5):
    """``n`` carbons on a sphere of ``bond`` A around one more carbon, which has the HIGHEST atom index: the centre owns
    all ``n`` bonds, more than the sixteen lanes of a group take in one pass.  The points are a Fibonacci lattice: at n =
    20 neighbours on the sphere are more than 1 A apart, some of them bonded to each other as well."""
    k = np.arange(n) + 0.5
    phi, theta = np.arccos(1.0 - 2.0 * k / n), np.pi * (1.0 + 5.0 ** 0.5) * k
    shell = bond * np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)
    pos = mu.on_grid(np.concatenate([shell, [[0.0, 0.0, 0.0]]]) + 10.0)
    return pos, mu.cubic(20.0), np.full(n + 1, 6)


def two_images(a=2.75):
    """Two carbons 1.375 A apart along x in a cell of ``a`` = 2.75 A along x: each reaches the other directly and through
    the face, at the same distance."""
    pos = mu.on_grid([[0.625, 6.0, 6.0], [2.0, 6.0, 6.0]])
    return pos, np.diag([a, 12.0, 12.0]), np.full(2, 6)


def ulps(got, want) -> np.ndarray:
    """The distance of two fp32 arrays in units in the last place, 0 where both are NaN and a large number where one is."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)

    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    both = np.isnan(got) & np.isnan(want)
    one = np.isnan(got) != np.isnan(want)
    return np.where(both, 0, np.where(one, 1 << 40, np.abs(key(got) - key(want))))


def same_table(got: dict, want: dict) -> dict:
    """Asserts what the bond-table tests ask of a kernel's table against the numpy rule's -- the columns of ``EXACT`` bit
    for bit, those of ``ONE_ULP`` within one fp32 unit in the last place -- and returns the largest distance per column."""
    worst = {}
    for k in COLUMNS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        if k in EXACT:
            assert g.tobytes() == w.tobytes(), k
        else:
            d = ulps(g, w)
            worst[k] = int(d.max()) if d.size else 0
            assert worst[k] <= 1, (k, worst[k])
    return worst

"""``cartnet_adp_riding_h`` (csrc/riding_ops.hip) against ``bonds.riding_hydrogens_host`` on the same inputs: ``parent`` and
``count`` equal, ``mult`` and ``u_iso`` bit for bit (NaN positions included), the per-crystal figures from the values as
stored.  The graphs are edge lists written by hand (sorted by target, as every loader's), so every segment length and every
edge of the rule is placed where the test wants it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL, F, F_ROT = 0.4, 1.2, 1.5
FAR = 3.0                                        # no bond at any Z of the tests


def _batch(z, edges, ptr=None, mask="z", u_eq=None, seed=0):
    """The dict ``riding_h`` takes and ``u_eq``.  ``edges``: directed (source, target, dist), sorted here by target (stable:
    the order inside a segment is the order given); ``mask``: "z" (the non-hydrogen atoms), None (every atom has a row) or
    a list of bools."""
    z = np.asarray(z, dtype=np.int64).reshape(-1)
    edges = sorted(edges, key=lambda e: e[1])
    ei = np.array([[e[0] for e in edges], [e[1] for e in edges]], dtype=np.int64).reshape(2, -1)
    dist = np.array([e[2] for e in edges], dtype=np.float32)
    ptr = [0, len(z)] if ptr is None else ptr
    batch = {"x": torch.from_numpy(z).cuda(), "edge_index": torch.from_numpy(ei).cuda(),
             "cart_dist": torch.from_numpy(dist).cuda(), "ptr": torch.tensor(ptr, dtype=torch.int64).cuda()}
    if mask is not None:
        m = z != 1 if isinstance(mask, str) else np.asarray(mask, dtype=bool)
        batch["non_H_mask"] = torch.from_numpy(m).cuda()
    M = len(z) if mask is None else int(batch["non_H_mask"].sum())
    if u_eq is None:
        u_eq = 0.02 + 0.03 * np.random.default_rng(seed).random(M)
    return batch, torch.tensor(np.asarray(u_eq), dtype=torch.float32).reshape(-1).cuda()


def _host(batch, u_eq, tol=TOL, f=F, f_rot=F_ROT):
    from cartnet_amd.bonds import riding_hydrogens_host
    z = batch["x"].cpu().numpy()
    mask = batch["non_H_mask"].cpu().numpy().astype(bool) if "non_H_mask" in batch else np.ones(len(z), dtype=bool)
    row = np.where(mask, np.cumsum(mask) - 1, -1)
    return riding_hydrogens_host(z, batch["edge_index"].cpu().numpy(), batch["cart_dist"].cpu().numpy(), row,
                                 u_eq.cpu().numpy(), tol, f, f_rot) + (row,)


def _check(batch, u_eq, tol=TOL, f=F, f_rot=F_ROT):
    """Runs the kernel, compares everything with the host rule and a second run; returns the result as numpy arrays."""
    from cartnet_amd import metrics as gm
    res = gm.riding_h(u_eq, batch, tol, f, f_rot)
    parent, count, mult, u_iso, row = _host(batch, u_eq, tol, f, f_rot)
    N, B = len(parent), int(batch["ptr"].numel()) - 1
    got = {k: getattr(res, k).cpu().numpy() for k in res._fields}
    assert got["parent"].dtype == np.int64 and got["count"].dtype == np.int32
    assert got["mult"].dtype == got["u_iso"].dtype == np.float32 and got["crystal_stats"].dtype == np.float64
    assert got["parent"].shape == got["count"].shape == got["mult"].shape == got["u_iso"].shape == (N,)
    assert np.array_equal(got["parent"], parent) and np.array_equal(got["count"], count)
    assert got["mult"].tobytes() == mult.tobytes()
    assert got["u_iso"].tobytes() == u_iso.tobytes()                          # bit for bit, NaN positions included
    # per crystal, from the values as stored: the counts exactly, the fp64 sum of fp32 values up to its order
    z, ptr, u = batch["x"].cpu().numpy(), batch["ptr"].cpu().numpy(), u_eq.cpu().numpy()
    assert got["crystal_stats"].shape == (B, 4)
    for g in range(B):
        sl = slice(ptr[g], ptr[g + 1])
        h = z[sl] == 1
        rider = h & (parent[sl] >= 0)
        want_sum = u_iso[sl][rider & np.isfinite(u_iso[sl])].astype(np.float64).sum()
        pu = u[row[parent[sl][rider]]]
        assert got["crystal_stats"][g, 0] == h.sum() and got["crystal_stats"][g, 1] == (h & (parent[sl] < 0)).sum()
        assert got["crystal_stats"][g, 3] == (~(pu > 0)).sum()
        assert abs(got["crystal_stats"][g, 2] - want_sum) <= 1e-12 * abs(want_sum)
    again = gm.riding_h(u_eq, batch, tol, f, f_rot)
    for a, b in zip(res, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()         # two runs, equal bytes
    return got


def _random(counts, seed, max_edges=40):
    """Crystals of ``counts`` atoms (H, C, N, O, S interleaved at random), every atom with 0 ... ``max_edges`` incoming edges
    from atoms of its own crystal at distances drawn from a short list, so that ties, bonds at every kind of atom and
    hydrogens with several candidates all occur."""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    z = rng.choice([1, 1, 1, 6, 6, 7, 8, 16], size=int(ptr[-1]))
    edges = []
    for g, n in enumerate(counts):
        for i in range(ptr[g], ptr[g + 1]):
            for _ in range(int(rng.integers(0, max_edges // 2 + 1))):
                j, d = int(rng.integers(ptr[g], ptr[g + 1])), float(rng.choice([0.9, 1.0, 1.09, 1.3, 1.6, 2.5, 4.0]))
                edges.append((j, i, d))
                if rng.random() < 0.8:                                        # most pairs are held in both directions
                    edges.append((i, j, d))
    return z, edges, [int(v) for v in ptr]


@pytest.mark.parametrize("N", [1, 17, 257])
def test_atom_counts_around_a_workgroup(N):
    """16 atoms per workgroup: one atom, one past a workgroup, one past sixteen."""
    z, edges, ptr = _random([N], N)
    got = _check(*_batch(z, edges, ptr, seed=N))
    assert N == 1 or ((got["parent"] >= 0).sum() >= 2 and got["count"].sum() >= 2)         # not vacuous


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 33])
def test_hydrogen_segment_lengths_with_the_only_parent_at_the_last_edge(length):
    """H0's segment: ``length - 1`` carbons too far to bond, then C1 at 1.09 A."""
    z = [1, 6] + [6] * max(length - 1, 0)
    edges = [(2 + k, 0, FAR) for k in range(length - 1)] + ([(1, 0, 1.09), (0, 1, 1.09)] if length else [])
    got = _check(*_batch(z, edges))
    assert got["parent"][0] == (1 if length else -1) and got["mult"][0] == (np.float32(F) if length else 0.0)
    assert bool(np.isnan(got["u_iso"][0])) == (length == 0)


def test_parent_segment_of_33_edges_with_its_hydrogens_at_0_16_and_32():
    """C0's segment: H1 first, H2 at edge 16, H3 at edge 32, far carbons and a far hydrogen between them."""
    z = [6, 1, 1, 1, 1] + [6] * 30
    seg = [(1, 0, 1.09)] + [(5 + k, 0, FAR) for k in range(15)] + [(2, 0, 1.09)] + [(20 + k, 0, FAR) for k in range(14)]
    seg += [(4, 0, 2.4), (3, 0, 1.09)]
    assert len(seg) == 33 and [e[0] for e in (seg[0], seg[16], seg[32])] == [1, 2, 3]
    got = _check(*_batch(z, seg + [(0, 1, 1.09), (0, 2, 1.09), (0, 3, 1.09), (0, 4, 2.4)]))
    assert got["count"][0] == 3 and got["parent"][:5].tolist() == [-1, 0, 0, 0, -1]
    assert got["mult"][1:5].tolist() == [np.float32(F_ROT)] * 3 + [0.0]


def test_ragged_batch_with_an_empty_crystal_and_interleaved_hydrogens():
    z, edges, ptr = _random([5, 0, 70, 1, 23], 7)
    got = _check(*_batch(z, edges, ptr, seed=7))
    assert got["crystal_stats"][1].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert got["crystal_stats"][2, 0] > got["crystal_stats"][2, 1] > 0         # riders and orphans in one crystal


def test_no_edges_and_no_rows():
    z = [6, 1, 1, 8, 1]
    got = _check(*_batch(z, []))                                              # E == 0
    assert got["parent"].tolist() == [-1] * 5 and got["crystal_stats"][0].tolist() == [3.0, 3.0, 0.0, 0.0]
    assert np.isnan(got["u_iso"][[1, 2, 4]]).all() and not np.isnan(got["u_iso"][[0, 3]]).any()
    edges = [(0, 1, 1.09), (1, 0, 1.09), (3, 4, 0.96), (4, 3, 0.96)]
    got = _check(*_batch(z, edges, mask=[False] * 5))                         # M == 0: nobody has a row, so nobody is a parent
    assert got["parent"].tolist() == [-1] * 5 and np.isnan(got["u_iso"]).all() and got["count"].tolist() == [0] * 5
    got = _check(*_batch([1, 1, 1], [(0, 1, 0.74), (1, 0, 0.74)]))            # hydrogens only
    assert got["crystal_stats"][0].tolist() == [3.0, 3.0, 0.0, 0.0]


def test_the_limit_itself_is_a_bond_and_the_next_float_is_not():
    from cartnet_amd.bonds import COVALENT_RADII
    r = np.asarray(COVALENT_RADII, dtype=np.float32)
    limit = (r[1] + r[6]) + np.float32(TOL)
    above = np.nextafter(limit, np.float32(np.inf))
    assert above > limit
    z = [1, 6, 1, 6]
    got = _check(*_batch(z, [(1, 0, limit), (0, 1, limit), (3, 2, above), (2, 3, above)]))
    assert got["parent"].tolist() == [1, -1, -1, -1] and got["count"].tolist() == [0, 1, 0, 0]
    got = _check(*_batch([1, 6], [(1, 0, float("nan")), (0, 1, float("nan"))]))               # a NaN distance never qualifies
    assert got["parent"].tolist() == [-1, -1]


def test_which_neighbour_is_the_parent():
    # two carbons at the same fp32 distance: the lower edge wins, whichever atom index it names
    got = _check(*_batch([1, 6, 6], [(2, 0, 1.1), (1, 0, 1.1), (0, 1, 1.1), (0, 2, 1.1)]))
    assert got["parent"][0] == 2 and got["count"].tolist() == [0, 0, 1]
    # ... also across lanes and passes: edges 1 and 18 (lanes 1 and 2), then edges 2 and 17 (the later lane holds the lower)
    seg = [(3, 0, FAR)] + [(1, 0, 1.1)] + [(3, 0, FAR)] * 16 + [(2, 0, 1.1)]
    got = _check(*_batch([1, 6, 6, 6], seg))
    assert len(seg) == 19 and got["parent"][0] == 1
    seg = [(3, 0, FAR)] * 2 + [(2, 0, 1.1)] + [(3, 0, FAR)] * 14 + [(1, 0, 1.1)]
    got = _check(*_batch([1, 6, 6, 6], seg))
    assert len(seg) == 18 and got["parent"][0] == 2
    # the nearest neighbour is a hydrogen, the next a Z beyond the table, the next Z = 0, then the atom's own image: skipped
    z = [1, 1, 97, 0, 6, 120]
    got = _check(*_batch(z, [(1, 0, 0.7), (2, 0, 0.8), (3, 0, 0.85), (0, 0, 0.9), (5, 0, 0.95), (4, 0, 1.2)]))
    assert got["parent"][0] == 4 and got["mult"][0] == np.float32(F)
    # the same carbon through two images: the nearer edge names it, and its count sees the hydrogen twice
    got = _check(*_batch([1, 6], [(1, 0, 1.3), (1, 0, 1.0), (0, 1, 1.0), (0, 1, 1.3)]))
    assert got["parent"][0] == 1 and got["count"][1] == 2
    # a nearer carbon without a row is skipped
    got = _check(*_batch([1, 6, 6], [(1, 0, 1.0), (2, 0, 1.2), (0, 1, 1.0), (0, 2, 1.2)], mask=[False, False, True]))
    assert got["parent"][0] == 2 and got["count"].tolist() == [0, 0, 1]


def test_multipliers():
    def molecule(zp, n):
        return [zp] + [1] * n, [e for k in range(n) for e in ((0, 1 + k, 1.0), (1 + k, 0, 1.0))]
    for zp, n, want in ((6, 2, F), (6, 3, F_ROT), (6, 4, F_ROT), (8, 1, F_ROT), (8, 2, F_ROT), (7, 3, F), (6, 1, F)):
        z, edges = molecule(zp, n)
        got = _check(*_batch(z, edges, seed=zp * 10 + n))
        assert got["count"][0] == n and got["mult"].tolist() == [0.0] + [np.float32(want)] * n, (zp, n)
    # a capped, asymmetric graph that holds only p -> i: n falls back to 1, so three hydrogens on a carbon stay at f
    z, edges = molecule(6, 3)
    got = _check(*_batch(z, [e for e in edges if e[0] == 0]))
    assert got["count"][0] == 0 and got["parent"].tolist() == [-1, 0, 0, 0] and got["mult"][1:].tolist() == [np.float32(F)] * 3
    # other factors are the caller's
    got = _check(*_batch(*molecule(6, 3)), tol=0.3, f=1.25, f_rot=1.75)
    assert got["mult"][1:].tolist() == [1.75] * 3


def test_a_parent_that_is_not_positive_is_passed_through_and_counted():
    z = [6, 1, 1, 8, 1, 7, 1]
    edges = [(0, 1, 1.0), (1, 0, 1.0), (0, 2, 1.0), (2, 0, 1.0), (3, 4, 0.96), (4, 3, 0.96), (5, 6, 1.0), (6, 5, 1.0)]
    got = _check(*_batch(z, edges, u_eq=[-0.01, 0.0, float("nan")]))
    assert got["u_iso"][1] == got["u_iso"][2] == np.float32(np.float64(np.float32(F)) * np.float64(np.float32(-0.01)))
    assert got["u_iso"][4] == 0.0 and np.isnan(got["u_iso"][6]) and got["parent"][6] == 5
    assert got["crystal_stats"][0].tolist()[:2] == [4.0, 0.0] and got["crystal_stats"][0, 3] == 4.0
    assert got["crystal_stats"][0, 2] == np.float64(got["u_iso"][1]) * 2          # the finite ones: a NaN stays out of the sum


def test_without_a_mask_and_as_a_batch_object():
    from cartnet_amd import metrics as gm
    from cartnet_amd.data import Batch
    z, edges, ptr = _random([9, 30], 11)
    batch, u_eq = _batch(z, edges, ptr, mask=None, seed=11)                   # every atom has a row, the hydrogens too
    got = _check(batch, u_eq)
    assert (got["parent"] >= 0).any() and not np.isnan(got["u_iso"][z != 1]).any()
    batch, u_eq = _batch(z, edges, ptr, seed=12)
    ref = gm.riding_h(u_eq, batch)
    obj = Batch(**batch)
    obj.num_graphs = 2
    for a, b in zip(ref, gm.riding_h(u_eq, obj)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    named = {("z" if k == "x" else k): v for k, v in batch.items()}
    for a, b in zip(ref, gm.riding_h(u_eq, named, TOL, F, F_ROT)):            # the defaults are the flags' defaults
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_argument_checks():
    from cartnet_amd import metrics as gm
    batch, u_eq = _batch([6, 1], [(0, 1, 1.0), (1, 0, 1.0)])
    with pytest.raises(ValueError, match="u_eq must be"):
        gm.riding_h(u_eq.double(), batch)
    with pytest.raises(ValueError, match="u_eq must be"):
        gm.riding_h(u_eq.view(1, 1), batch)
    with pytest.raises(ValueError, match="batch.ptr"):
        gm.riding_h(u_eq, {k: v for k, v in batch.items() if k != "ptr"})
    with pytest.raises(ValueError, match="a forward has overwritten"):
        gm.riding_h(u_eq, dict(batch, x=torch.zeros(2, 8, device="cuda:0")))
    with pytest.raises(ValueError, match="edge_index must be"):
        gm.riding_h(u_eq, dict(batch, edge_index=batch["edge_index"].to(torch.int32)))
    with pytest.raises(ValueError, match="cart_dist"):
        gm.riding_h(u_eq, dict(batch, cart_dist=batch["cart_dist"][:1]))
    with pytest.raises(ValueError, match="non_H_mask must be"):
        gm.riding_h(u_eq, dict(batch, non_H_mask=batch["non_H_mask"][:1]))
    with pytest.raises(ValueError, match="no non_H_mask"):
        gm.riding_h(u_eq, {k: v for k, v in batch.items() if k != "non_H_mask"})
    from cartnet_amd.lib import CartnetHipError
    with pytest.raises(CartnetHipError, match="must be numbers"):             # the entry point's own check, before a launch
        gm.riding_h(u_eq, batch, f=float("nan"))
    empty = gm.riding_h(u_eq[:0], dict(batch, x=batch["x"][:0], non_H_mask=batch["non_H_mask"][:0],
                                       edge_index=batch["edge_index"][:, :0], cart_dist=batch["cart_dist"][:0],
                                       ptr=torch.zeros(2, dtype=torch.int64, device="cuda:0")))
    assert empty.parent.numel() == 0 and empty.crystal_stats.tolist() == [[0.0, 0.0, 0.0, 0.0]]

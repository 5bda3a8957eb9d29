"""``cartnet_adp_bond_test`` (csrc/bond_ops.hip) against an fp64 numpy restatement on the same fp32 inputs: the bond rule
(``cartnet_amd.bonds``), ``D = d^T U_i d - d^T U_j d`` per bond, the per-row figures in edge order and the per-crystal
sums; the edge cases of the rule, and the direction of the convention (a rigid body's amplitudes agree along every bond,
independent ones do not).  Graphs come from ``graph.radius_graph_pbc`` on explicit positions."""
import numpy as np
import pytest
import torch

import predict_utils as pu

pytestmark = pytest.mark.gpu

EPS23 = 2.0 ** -23
TOL, THRESHOLD = 0.4, 1e-3
ROWS = (0, 1, 65, 130, 7)       # an empty crystal, a single row, past one and two strides of a wave, a ragged tail


def _cubic(a):
    return np.eye(3) * a


def _random_crystal(n_heavy, n_h, seed, volume_per_atom=12.0):
    """``n_heavy`` non-hydrogen atoms (C, N, O, S, Cl) and ``n_h`` hydrogens at uniform random positions in a cubic cell,
    the hydrogens interleaved (an atom's index is not its row)."""
    rng = np.random.default_rng(seed)
    n = n_heavy + n_h
    z = np.ones(n, dtype=np.int64)
    heavy = np.sort(rng.permutation(n)[:n_heavy])
    z[heavy] = rng.choice([6, 6, 6, 7, 8, 16, 17], size=n_heavy)
    a = max((n * volume_per_atom) ** (1.0 / 3.0), 5.5)
    return rng.random((n, 3)) * a, _cubic(a), z


def _make(crystals, seed, radius=5.0, u=None):
    """One batch from ``[(pos [n,3], cell [3,3], z [n]), ...]``: the dict ``bond_test`` takes, ``u`` and ``row_ptr``."""
    from cartnet_amd.graph import radius_graph_pbc
    pos = torch.tensor(np.concatenate([c[0] for c in crystals]), dtype=torch.float32).cuda()
    cell = torch.tensor(np.stack([c[1] for c in crystals]), dtype=torch.float32).cuda()
    z = torch.tensor(np.concatenate([c[2] for c in crystals]), dtype=torch.int64).cuda()
    counts = [len(c[2]) for c in crystals]
    ptr = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0).cuda()
    ei, dist, dirs = radius_graph_pbc(pos, cell, ptr, radius)
    assert bool((ei[1][1:] >= ei[1][:-1]).all())                              # sorted by target
    mask = z != 1
    rows = [int((c[2] != 1).sum()) for c in crystals]
    row_ptr = torch.tensor([0] + rows, dtype=torch.int64).cumsum(0).cuda()
    if u is None:
        u = pu.spd_rows(sum(rows), seed)
    batch = {"x": z, "edge_index": ei, "cart_dist": dist, "cart_dir": dirs, "non_H_mask": mask, "ptr": ptr}
    return batch, u.to(torch.float32).cuda(), row_ptr


def _reference(batch, u, tol=TOL, threshold=THRESHOLD):
    """fp64 numpy on the same fp32 inputs: per-row arrays as the kernel defines them, the per-bond ``|D|`` with their rows,
    and the margins of the two decisions (distance against the limit, ``|D|`` against the threshold)."""
    from cartnet_amd.bonds import COVALENT_RADII, is_bond
    z, mask = batch["x"].cpu().numpy(), batch["non_H_mask"].cpu().numpy()
    src, tgt = batch["edge_index"].cpu().numpy()
    dist, d = batch["cart_dist"].cpu().numpy(), batch["cart_dir"].cpu().numpy().astype(np.float64)
    U = u.cpu().numpy().astype(np.float64)
    S = 0.5 * (U + U.transpose(0, 2, 1))
    M = len(U)
    row = np.where(mask, np.cumsum(mask) - 1, -1)
    bond = is_bond(dist, z[tgt], z[src], tol, same_atom=src == tgt) & (row[src] >= 0) & (row[tgt] >= 0)
    # the margin of the distance decision, over every edge whose ends could bond at some distance
    r = np.asarray(COVALENT_RADII, dtype=np.float32)
    can = (src != tgt) & (z[src] > 1) & (z[src] < len(r)) & (z[tgt] > 1) & (z[tgt] < len(r))
    limit = (r[np.where(can, z[tgt], 0)] + r[np.where(can, z[src], 0)]) + np.float32(tol)
    dist_margin = np.abs(dist.astype(np.float64) - limit.astype(np.float64))[can].min() if can.any() else np.inf
    out = {"bonds": np.zeros(M, np.int32), "delta_sum": np.zeros(M), "delta_max": np.zeros(M),
           "worst": np.full(M, -1, np.int64), "over": np.zeros(M, np.int32), "ueq_ratio": np.full(M, np.nan)}
    traces, deltas = np.zeros(M), []
    for e in np.nonzero(bond)[0]:                                             # edge order
        m, mj = row[tgt[e]], row[src[e]]
        a = abs(d[e] @ S[m] @ d[e] - d[e] @ S[mj] @ d[e])
        deltas.append((m, a))
        out["bonds"][m] += 1
        out["delta_sum"][m] += a
        out["over"][m] += a > threshold
        traces[m] += np.trace(U[mj])
        if out["worst"][m] < 0 or a > out["delta_max"][m]:                    # a tie keeps the lower edge
            out["delta_max"][m], out["worst"][m] = a, src[e]
    has = out["bonds"] > 0
    out["ueq_ratio"][has] = np.trace(U, axis1=1, axis2=2)[has] / (traces[has] / out["bonds"][has])
    thr_margin = min((abs(a - threshold) for _, a in deltas), default=np.inf)
    return out, deltas, dist_margin, thr_margin, bond


def _check(batch, u, row_ptr, trivial=False, tol=TOL, threshold=THRESHOLD):
    """Runs the kernel, compares everything with the reference, returns (result, reference, bond mask)."""
    from cartnet_amd import metrics as gm
    res = gm.bond_test(u, batch, row_ptr, tol, threshold)
    ref, deltas, dist_margin, thr_margin, bond = _reference(batch, u, tol, threshold)
    # conditions on the inputs: the case must not pass vacuously, and no decision may hang on a rounding
    assert trivial or len(deltas) >= 1
    assert thr_margin > 1e-9 and dist_margin > 1e-5
    M, B = int(u.shape[0]), int(row_ptr.numel()) - 1
    got = {k: getattr(res, k).cpu().numpy() for k in ref}
    assert got["bonds"].dtype == np.int32 and got["worst"].dtype == np.int64 and got["over"].dtype == np.int32
    for k in ("bonds", "worst", "over"):
        assert got[k].shape == (M,) and np.array_equal(got[k], ref[k]), k
    assert np.array_equal(np.isnan(got["ueq_ratio"]), ref["bonds"] == 0)      # NaN exactly where there is no bond
    rp = row_ptr.cpu().numpy()
    U = u.cpu().numpy().astype(np.float64)
    stats = res.crystal_stats.cpu().numpy()
    assert stats.dtype == np.float64 and stats.shape == (B, 4)
    for g in range(B):
        sl = slice(rp[g], rp[g + 1])
        if rp[g] == rp[g + 1]:
            assert stats[g].tolist() == [0.0, 0.0, 0.0, 0.0]
            continue
        umax = np.abs(U[sl]).max()
        for k in ("delta_sum", "delta_max", "ueq_ratio"):
            a, b = got[k][sl].astype(np.float64), ref[k][sl]
            ok = ~np.isnan(b)
            err, bound = np.abs(a - b)[ok], EPS23 * np.abs(b)[ok] + 1e-12 * umax
            if ok.any():
                print(f"crystal {g} {k}: max error {err.max():.3e}, bound there {bound[err.argmax()]:.3e}")
            assert (err <= bound).all(), (g, k)
        # per crystal: the fp64 sums of the per-row values AS STORED
        assert stats[g, 0] == got["bonds"][sl].sum() and stats[g, 3] == got["over"][sl].sum()
        assert stats[g, 2] == got["delta_max"][sl].astype(np.float64).max()
        want = got["delta_sum"][sl].astype(np.float64).sum()
        assert abs(stats[g, 1] - want) <= 1e-12 * want                        # only the order differs
    again = gm.bond_test(u, batch, row_ptr, tol, threshold)
    for a, b in zip(res, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()         # two runs, equal bytes
    return res, ref, bond


def _pair(offset):
    c = np.array([10.0, 10.0, 10.0])
    return np.stack([c, c + np.asarray(offset)]), _cubic(20.0), np.array([6, 6])


def test_two_atoms():
    res, ref, _ = _check(*_make([_pair([1.5, 0.0, 0.0])], 1))
    assert ref["bonds"].tolist() == [1, 1] and res.worst.tolist() == [1, 0]
    assert res.crystal_stats[0, 0].item() == 2.0                             # one bond, seen from both ends


def test_ragged_batch_with_an_empty_crystal_and_interleaved_hydrogens():
    crystals = [_random_crystal(n, h, 100 + k) for k, (n, h) in enumerate(zip(ROWS, (3, 2, 30, 60, 4)))]
    batch, u, row_ptr = _make(crystals, 2)
    assert (row_ptr[1:] - row_ptr[:-1]).tolist() == list(ROWS)
    mask = batch["non_H_mask"].cpu().numpy()
    assert not np.array_equal(np.nonzero(mask)[0], np.arange(mask.sum()))    # an atom's index is not its row
    res, ref, _ = _check(batch, u, row_ptr)
    rp = row_ptr.tolist()
    for g in (2, 3, 4):                                                       # every larger crystal has bonds of its own
        assert ref["bonds"][rp[g]:rp[g + 1]].sum() > 0
    assert (ref["over"] > 0).any() and (ref["over"] < ref["bonds"]).any()    # the threshold splits the bonds
    # worst is an atom index of the BATCH, inside the row's own crystal, and never a hydrogen
    worst, ptr = res.worst.cpu().numpy(), batch["ptr"].cpu().numpy()
    crystal = np.repeat(np.arange(len(ROWS)), ROWS)
    has = worst >= 0
    assert (worst[has] >= ptr[crystal[has]]).all() and (worst[has] < ptr[crystal[has] + 1]).all() and mask[worst[has]].all()


def test_the_only_bond_sits_beyond_edge_64_of_a_dense_segment():
    rng = np.random.default_rng(7)
    centre = np.array([4.0, 4.0, 4.0])
    pts = rng.random((400, 3)) * 8.0
    pts = pts[np.linalg.norm(pts - centre, axis=1) > 2.5][:90]                # nothing else within bonding range of atom 0
    pos = np.concatenate([centre[None], pts, (centre + [0.9, 0.8, 0.9])[None]])  # the partner is the LAST atom: 1.5 A
    z = np.array([6] + [6 if k % 3 else 1 for k in range(90)] + [6])
    batch, u, row_ptr = _make([(pos, _cubic(8.0), z)], 3)
    res, ref, bond = _check(batch, u, row_ptr)
    tgt = batch["edge_index"][1].cpu().numpy()
    seg = np.nonzero(tgt == 0)[0]
    assert len(seg) > 64 and bond[seg].sum() == 1 and np.nonzero(bond[seg])[0][0] >= 64
    assert res.bonds[0].item() == 1 and res.worst[0].item() == len(z) - 1


def test_an_atom_without_edges_and_a_batch_without_edges():
    batch, u, row_ptr = _make([(np.array([[1.0, 2.0, 3.0]]), _cubic(12.0), np.array([6]))], 4)
    assert batch["edge_index"].shape[1] == 0
    res, _, _ = _check(batch, u, row_ptr, trivial=True)
    assert res.bonds.tolist() == [0] and res.worst.tolist() == [-1] and res.delta_max.tolist() == [0.0]
    assert res.delta_sum.tolist() == [0.0] and res.over.tolist() == [0] and bool(torch.isnan(res.ueq_ratio).all())
    assert res.crystal_stats.tolist() == [[0.0, 0.0, 0.0, 0.0]]
    # the same atom beside a bonded pair: an empty segment between full ones
    batch, u, row_ptr = _make([(np.array([[1.0, 2.0, 3.0]]), _cubic(12.0), np.array([6])), _pair([0.0, 1.4, 0.0])], 4)
    res, ref, _ = _check(batch, u, row_ptr)
    assert res.bonds.tolist() == [0, 1, 1]


def test_an_atoms_own_image_is_no_bond():
    """One caesium atom in a 3 A cell: every edge joins the atom to an image of itself, at 3 A and more, well inside
    (2.44 + 2.44) + 0.4 A -- by distance alone each would be a bond."""
    batch, u, row_ptr = _make([(np.array([[0.5, 0.5, 0.5]]), _cubic(3.0), np.array([55]))], 5)
    src, tgt = batch["edge_index"].cpu().numpy()
    assert len(src) > 0 and (src == tgt).all() and float(batch["cart_dist"].min()) < 4.0
    res, _, _ = _check(batch, u, row_ptr, trivial=True)
    assert res.bonds.tolist() == [0] and res.worst.tolist() == [-1]


def test_an_atom_bonded_only_to_hydrogens_has_no_bond():
    c = np.array([10.0, 10.0, 10.0])
    pos = np.stack([c + [1.0, 0, 0], c, c + [0, 1.0, 0], c + [0, 0, -1.0]])
    batch, u, row_ptr = _make([(pos, _cubic(20.0), np.array([1, 6, 1, 1]))], 6)
    assert batch["edge_index"].shape[1] == 12
    res, _, _ = _check(batch, u, row_ptr, trivial=True)
    assert res.bonds.tolist() == [0] and bool(torch.isnan(res.ueq_ratio).all())


def test_z_of_zero_and_z_beyond_the_table_never_bond():
    c = np.array([10.0, 10.0, 10.0])
    pos = np.stack([c, c + [1.4, 0, 0], c + [0, 1.4, 0], c + [0, 0, 1.5]])
    batch, u, row_ptr = _make([(pos, _cubic(20.0), np.array([6, 0, 97, 6]))], 7)
    assert int(u.shape[0]) == 4                                               # Z = 0 and Z = 97 have rows: they are no hydrogens
    res, _, _ = _check(batch, u, row_ptr)
    assert res.bonds.tolist() == [1, 0, 0, 1] and res.worst.tolist() == [3, -1, -1, 0]


def test_a_tie_goes_to_the_lower_edge():
    """B and C sit at c + v and c - v with bit-identical U: the two directions are exact negatives, the quadratic form is
    even, so the two |D| of the centre atom are the same number."""
    c, v = np.array([10.0, 10.0, 10.0]), np.array([1.0, 0.75, 0.5])
    pos = np.stack([c + v, c, c - v])                                          # the centre is atom 1
    u = pu.spd_rows(3, 8)
    u[2] = u[0]
    batch, u, row_ptr = _make([(pos, _cubic(20.0), np.array([6, 8, 6]))], 8, u=u)
    src, tgt = batch["edge_index"].cpu().numpy()
    d = batch["cart_dir"].cpu().numpy()
    e0, e2 = (np.nonzero((tgt == 1) & (src == s))[0][0] for s in (0, 2))
    assert e0 < e2 and np.array_equal(d[e0], -d[e2])
    res, ref, _ = _check(batch, u, row_ptr)
    assert ref["bonds"].tolist() == [1, 2, 1] and ref["delta_max"][1] > 0
    assert res.worst.tolist() == [1, 0, 1]                                    # the centre keeps the earlier edge


@pytest.mark.parametrize("where", ["xx", "yy"])
def test_direction_on_diagonals(where):
    """A bond along x: only U_xx enters.  The difference in xx comes out as |a - a'|, the same difference in yy as 0."""
    from cartnet_amd import metrics as gm
    a, a2, b = np.float32(0.02), np.float32(0.03), np.float32(0.015)
    u = torch.zeros(2, 3, 3)
    u[0] = torch.diag(torch.tensor([a, b, b]))
    u[1] = torch.diag(torch.tensor([a2, b, b] if where == "xx" else [a, a2, b]))
    batch, u, row_ptr = _make([_pair([1.5, 0.0, 0.0])], 9, u=u)
    assert batch["cart_dir"].abs().cpu().tolist() == [[1.0, 0.0, 0.0]] * 2    # exact: the positions and 1.5 are
    res = gm.bond_test(u, batch, row_ptr)
    want = abs(float(a) - float(a2)) if where == "xx" else 0.0
    bound = EPS23 * want + 1e-12 * float(u.abs().max())
    got = res.delta_max.cpu().double().numpy()
    print(f"{where}: delta_max {got}, expected {want:.9e}, bound {bound:.3e}")
    assert res.bonds.tolist() == [1, 1] and (np.abs(got - want) <= bound).all()
    assert (np.abs(res.delta_sum.cpu().double().numpy() - want) <= bound).all()


def _cube():
    """Eight carbons on a cube of edge 1.5 A in a generic orientation at the centre of a 20 A cell: inside a ball of 6 A,
    so no edge crosses a cell face; three bonds each (the face diagonals, 2.12 A, are none)."""
    corners = np.array([[x, y, z] for x in (-0.75, 0.75) for y in (-0.75, 0.75) for z in (-0.75, 0.75)])
    pos = np.float32(corners @ pu.fixed_rotation().T + 10.0)
    return pos.astype(np.float64), _cubic(20.0), np.full(8, 6)


def test_direction_on_a_rigid_body():
    """U_i = the covariance of t + lambda x r_i over a fixed ensemble of translations t and rotation vectors lambda: along
    r_i - r_j the displacements of i and j are equal member by member, so D = 0 for every pair, up to the rounding of the
    inputs (six entries of each U to fp32 and the direction: 2^-20 max|U| leaves a margin of eight).  Independent random
    SPD rows on the same positions are not rigid: some bond is off by more than 1e-2 max|U|."""
    from cartnet_amd import metrics as gm
    pos, cell, z = _cube()
    rng = np.random.default_rng(11)
    t, lam = 0.1 * rng.standard_normal((64, 3)), 0.03 * rng.standard_normal((64, 3))
    r = pos - 10.0                                                            # about the centre of the ball
    disp = t[:, None, :] + np.cross(lam[:, None, :], r[None, :, :])           # [64, 8, 3]
    U = np.einsum("kia,kib->iab", disp, disp) / len(t)
    batch, u, row_ptr = _make([(pos, cell, z)], 12, u=torch.tensor(U, dtype=torch.float32))
    assert float(batch["cart_dist"].max()) < 6.0                              # no image: every edge is inside the ball
    res = gm.bond_test(u, batch, row_ptr)
    assert res.bonds.tolist() == [3] * 8
    umax = float(u.abs().max())
    print(f"rigid body: delta_max {float(res.delta_max.max()):.3e}, bound {2.0 ** -20 * umax:.3e}, max|U| {umax:.3e}")
    assert float(res.delta_max.max()) <= 2.0 ** -20 * umax
    assert res.over.tolist() == [0] * 8 and res.crystal_stats[0].tolist()[0] == 24.0
    loose, v, _ = _make([(pos, cell, z)], 13)
    free = gm.bond_test(v, loose, row_ptr)
    print(f"independent rows: delta_max {float(free.delta_max.max()):.3e}, max|U| {float(v.abs().max()):.3e}")
    assert float(free.delta_max.max()) > 1e-2 * float(v.abs().max())


def test_a_batch_of_the_host_loader_gives_what_its_arrays_give():
    """``bond_test`` reads a ``data.Batch`` (three synthetic crystals collated on the host, hydrogens among them) as it
    reads a dict of the same arrays."""
    from cartnet_amd import metrics as gm
    from cartnet_amd.synthetic import make_batch
    b = make_batch(3, 24)
    b.to("cuda:0")
    row_ptr = gm.target_row_ptr(b)
    view = {"x": b.x, "edge_index": b.edge_index, "cart_dist": b.cart_dist, "cart_dir": b.cart_dir,
            "non_H_mask": b.non_H_mask}
    assert bool((b.edge_index[1][1:] >= b.edge_index[1][:-1]).all()) and not bool(b.non_H_mask.all())
    res, _, _ = _check(view, b.y, row_ptr)
    direct = gm.bond_test(b.y, b, row_ptr, TOL, THRESHOLD)
    for x, y in zip(res, direct):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_argument_checks():
    from cartnet_amd import metrics as gm
    batch, u, row_ptr = _make([_pair([1.5, 0.0, 0.0])], 14)
    with pytest.raises(ValueError, match="u must be"):
        gm.bond_test(u.double(), batch, row_ptr)
    with pytest.raises(ValueError, match="row_ptr"):
        gm.bond_test(u, batch, row_ptr.to(torch.int32))
    with pytest.raises(ValueError, match="a forward has overwritten"):
        gm.bond_test(u, dict(batch, x=torch.zeros(2, 8, device="cuda:0")), row_ptr)
    with pytest.raises(ValueError, match="edge_index must be"):
        gm.bond_test(u, dict(batch, edge_index=batch["edge_index"].to(torch.int32)), row_ptr)
    with pytest.raises(ValueError, match="cart_dist"):
        gm.bond_test(u, dict(batch, cart_dir=batch["cart_dir"][:1]), row_ptr)
    with pytest.raises(ValueError, match="no non_H_mask"):
        gm.bond_test(u[:1], {k: v for k, v in batch.items() if k != "non_H_mask"}, row_ptr)
    empty = gm.bond_test(u[:0], dict(batch, non_H_mask=torch.zeros(2, dtype=torch.bool, device="cuda:0")),
                         torch.zeros(2, dtype=torch.int64, device="cuda:0"))
    assert tuple(empty.bonds.shape) == (0,) and empty.crystal_stats.tolist() == [[0.0, 0.0, 0.0, 0.0]]
    radii = gm.covalent_radii("cuda:0")
    assert radii is gm.covalent_radii(torch.device("cuda", 0)) and radii.numel() == 97 and radii.dtype == torch.float32

"""``cartnet_bond_adjacency``, ``cartnet_angle_table_count`` and ``cartnet_adp_angle_table`` (csrc/angle_table_ops.hip)
against ``bonds.angle_table_host`` on the arrays the kernels read: the eleven crystals of the bond-table test in one batch --
chains through cell faces and the polymer, a star whose centre owns twenty bonds, a pair bonded through two images, a
crystal without bonds, one of hydrogens only, a helix and a planar chain for the TLS fit -- plus a three-membered ring and a
centre of degree 4; a graph capped at two neighbours; the same crystals alone, twice and in another order; and the
cross-checks against the bond table and ``cartnet_adp_bond_test``.

Indices, order, counts, reverse edges and ``tls_rank`` are exact and NaNs fall in the same places.  ``value`` and
``libration`` are allowed one fp32 unit in the last place: the file is compiled without contraction, so both sides compute
the same fp64 cross and dot products in one order from the same fp32 inputs and round once; only ``atan2``'s last bits can
differ.  A torsion is compared on the circle."""
import numpy as np
import pytest
import torch

import angle_table_utils as at
import bond_table_utils as bu
import molecule_utils as mu
import tls_utils as tu

pytestmark = pytest.mark.gpu

TOL = mu.TOL
NAMES = ("small", "long", "polymer", "five", "star", "images", "apart", "hydrogens", "bad", "helix", "planar", "ring",
         "branched")
INDEX = ("nbr_ptr", "bond_edge", "reverse", "torsion_counts", "torsion_offsets", "angle_counts", "angle_offsets", "angle_ptr",
         "torsion_ptr")


def _host(t):
    return t.cpu().numpy()


def _spd(n, seed):
    a = np.random.default_rng(seed).standard_normal((n, 3, 3))
    return (0.01 * a @ a.transpose(0, 2, 1) + 0.02 * np.eye(3)).astype(np.float32)


def _crystals():
    """``[(pos, cell, z, rows)]`` in the order of ``NAMES``."""
    out = [(p, c, z, _spd(len(z), 40 + k)) for k, (p, c, z) in enumerate(mu.pair_test_crystals())]
    out.append(bu.star() + (_spd(21, 50),))
    out.append(bu.two_images() + (_spd(2, 51),))
    out.append((np.array([[1.0, 1.0, 1.0], [5.0, 5.0, 5.0], [9.0, 1.0, 5.0]]), mu.cubic(12.0), np.full(3, 6), _spd(3, 52)))
    out.append((np.array([[1.0, 1.0, 1.0], [1.5, 1.5, 1.5], [7.0, 7.0, 7.0]]), mu.cubic(10.0), np.ones(3, dtype=np.int64),
                np.zeros((0, 3, 3), dtype=np.float32)))
    bad = _spd(5, 53)
    bad[1] = np.nan
    bad[3] = -bad[3]
    out.append(mu.pair_test_crystals()[3] + (bad,))
    helix, planar = tu.helix(7, (3, 12, 12)), tu.planar_chain(8, (3, 3, 3))
    out.append((helix, mu.cubic(30.0), np.full(7, 6), tu.rigid_rows(helix, 500, tu.NOISE).astype(np.float32)))
    out.append((planar, mu.cubic(30.0), np.full(8, 6), tu.rigid_rows(planar, 507, tu.NOISE).astype(np.float32)))
    out.append(at.three_ring() + (_spd(3, 54),))
    branched = at.branched()
    out.append(branched + (tu.rigid_rows(branched[0], 514, tu.NOISE).astype(np.float32),))
    return out


def _batch(crystals, radius=5.0, max_neighbors=None):
    """The dict the analyses take, ``u`` and ``row_ptr`` of ``[(pos, cell, z, rows)]`` as one batch."""
    from cartnet_amd.graph import radius_graph_pbc
    pos = torch.tensor(np.concatenate([c[0] for c in crystals]), dtype=torch.float32).cuda()
    cell = torch.tensor(np.stack([c[1] for c in crystals]), dtype=torch.float32).cuda()
    z = torch.tensor(np.concatenate([c[2] for c in crystals]), dtype=torch.int64).cuda()
    ptr = torch.tensor([0] + [len(c[2]) for c in crystals], dtype=torch.int64).cumsum(0).cuda()
    ei, dist, dirs = radius_graph_pbc(pos, cell, ptr, radius, max_neighbors)
    assert bool((ei[1][1:] >= ei[1][:-1]).all())                              # sorted by target
    row_ptr = torch.tensor([0] + [int((c[2] != 1).sum()) for c in crystals], dtype=torch.int64).cumsum(0).cuda()
    u = torch.tensor(np.concatenate([c[3] for c in crystals]), dtype=torch.float32).cuda()
    return {"x": z, "edge_index": ei, "cart_dist": dist, "cart_dir": dirs, "non_H_mask": z != 1, "ptr": ptr}, u, row_ptr


def _rule(batch, tf=None, tol=TOL):
    from cartnet_amd.bonds import angle_table_host
    extra = dict(params=_host(tf.params), rank=_host(tf.rank)) if tf is not None else {}
    return angle_table_host(_host(batch["x"]), _host(batch["edge_index"]), _host(batch["cart_dist"]),
                            _host(batch["cart_dir"]), mu.atom_rows(_host(batch["non_H_mask"])), _host(batch["ptr"]), tol,
                            **extra)


def _tables(res) -> dict:
    return {"angles": {k: _host(getattr(res, f"angle_{k}")) for k in at.ANGLE_COLUMNS},
            "torsions": {k: _host(getattr(res, f"torsion_{k}")) for k in at.TORSION_COLUMNS}}


def _margin(batch, tol=TOL):
    """How far the nearest distance decision of the batch is from its limit."""
    from cartnet_amd.bonds import COVALENT_RADII
    z, (src, tgt), dist = _host(batch["x"]), _host(batch["edge_index"]), _host(batch["cart_dist"])
    r = np.asarray(COVALENT_RADII, dtype=np.float32)
    can = (src != tgt) & (z[src] > 1) & (z[tgt] > 1)
    limit = (r[np.where(can, z[tgt], 0)] + r[np.where(can, z[src], 0)]) + np.float32(tol)
    return np.abs(dist.astype(np.float64) - limit.astype(np.float64))[can].min()


def _closures(batch, ref):
    """Every value the reverse-edge rule compares with 0.5 A: per listed bond ``b -> c`` and per bond edge ``c -> b``."""
    (src, tgt), dist, dirs = _host(batch["edge_index"]), _host(batch["cart_dist"]), _host(batch["cart_dir"])
    v = dist[:, None] * dirs                                                  # fp32
    out = []
    for e0 in ref["bond_edge"]:
        into_b = ref["adj"][ref["nbr_ptr"][src[e0]]:ref["nbr_ptr"][src[e0] + 1]]
        out += [float(np.abs(v[e] + v[e0]).max()) for e in into_b if src[e] == tgt[e0]]
    return np.asarray(out)


def _check_index(index, ref, N):
    assert np.array_equal(_host(index.bonds.counts).astype(np.int64) + _host(index.bonds.unlisted), ref["degree"])
    for k in INDEX:
        t = getattr(index, k)
        assert t.dtype == torch.int64 and t.is_cuda, k
    assert np.array_equal(np.diff(_host(index.nbr_ptr)), ref["degree"]) and tuple(index.nbr_ptr.shape) == (N + 1,)
    d = ref["degree"]
    assert np.array_equal(_host(index.angle_counts), d * (d - 1) // 2)
    assert np.array_equal(_host(index.angle_counts), ref["angle_counts"])
    assert np.array_equal(_host(index.bond_edge), ref["bond_edge"]) and np.array_equal(_host(index.reverse), ref["reverse"])
    assert np.array_equal(_host(index.torsion_counts), ref["torsion_counts"])
    total = int(ref["nbr_ptr"][-1])
    assert np.array_equal(_host(index.adj)[:total], ref["adj"])
    assert _host(index.angle_ptr).tolist() == index.table_ptr_host[0].tolist() == ref["angle_ptr"].tolist()
    assert _host(index.torsion_ptr).tolist() == index.table_ptr_host[1].tolist() == ref["torsion_ptr"].tolist()
    assert not index.table_ptr_host.is_cuda and index.table_ptr_host.dtype == torch.int64


def _check_stats(res, tables, index):
    """Both ``crystal_stats`` from the values as stored; only the order of the fp64 sums differs."""
    ap, tp = index.table_ptr_host.numpy()
    for stats, table, cut, circular in ((_host(res.angle_stats), tables["angles"], ap, False),
                                        (_host(res.torsion_stats), tables["torsions"], tp, True)):
        assert stats.shape == (len(cut) - 1, 5) and stats.dtype == np.float64
        for g in range(len(cut) - 1):
            v, lib = (table[k][cut[g]:cut[g + 1]].astype(np.float64) for k in ("value", "libration"))
            fin = np.isfinite(lib)
            x = np.abs(lib - v)[fin]
            x = np.minimum(x, 360.0 - x) if circular else x
            assert stats[g, 0] == len(v) and stats[g, 2] == fin.sum() and stats[g, 4] == (x.max() if len(x) else 0.0)
            assert stats[g, 3] == pytest.approx(x.sum(), rel=1e-12, abs=1e-300)
            if circular:
                assert stats[g, 1] == np.isnan(v).sum()
            else:
                assert stats[g, 1] == pytest.approx(v.sum(), rel=1e-12, abs=1e-300)


@pytest.fixture(scope="module")
def fixture():
    """The batch, its index, the TLS fit the GPU gives for it, one pair of tables with and one without the fit, and the
    numpy rule on the same arrays; computed once."""
    from cartnet_amd import metrics as gm
    batch, u, row_ptr = _batch(_crystals())
    bonds = gm.bond_index(batch, row_ptr, TOL, rows=int(u.shape[0]))
    index = gm.angle_index(batch, row_ptr, TOL, rows=int(u.shape[0]), bonds=bonds)
    mo = gm.molecules(batch, row_ptr, TOL, rows=int(u.shape[0]))
    tf = gm.tls_fit(u, batch, row_ptr, mo)
    res = gm.angle_table(batch, row_ptr, index, tf)
    bare = gm.angle_table(batch, row_ptr, index)
    return batch, u, row_ptr, index, tf, res, bare, _rule(batch, tf), _rule(batch)


def test_the_fixture_holds_every_case(fixture):
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    assert _margin(batch) > 1e-5                                              # no bond decision hangs on a rounding
    m = _closures(batch, ref)
    print(f"{len(m)} reverse-edge candidates: {np.sort(np.unique(m))[:4]} ... {m.max()}")
    assert len(m) >= len(ref["bond_edge"]) and ((m < 0.25) | (m > 1.0)).all() and (m > 1.0).any()   # nor a reverse edge
    g = {name: k for k, name in enumerate(NAMES)}
    na, nt = np.diff(ref["angle_ptr"]).tolist(), np.diff(ref["torsion_ptr"]).tolist()
    names = ("small", "long", "polymer", "five", "star", "images", "apart", "hydrogens", "bad", "helix", "planar", "ring",
             "branched")
    assert [na[g[n]] for n in names] == [15, 191, 8, 3, 666, 2, 0, 0, 3, 5, 6, 3, 7]
    assert [nt[g[n]] for n in names] == [14, 189, 8, 2, 5082, 2, 0, 0, 2, 4, 5, 3, 3]
    ptr = _host(batch["ptr"])
    assert ref["degree"][ptr[g["star"] + 1] - 1] == 20 > 16                   # the centre: past one pass of sixteen lanes
    T = ref["torsions"]
    tp = ref["torsion_ptr"]
    assert np.isnan(T["value"][tp[g["images"]]:tp[g["images"] + 1]]).all() and np.isnan(T["value"]).sum() == 2
    same = T["a"] == T["d"]
    assert same[tp[g["ring"]]:tp[g["ring"] + 1]].all() and same[tp[g["star"]]:tp[g["star"] + 1]].sum() == 366
    ap = ref["angle_ptr"]
    assert ref["angles"]["value"][ap[g["images"]]:ap[g["images"] + 1]].tolist() == [180.0, 180.0]
    assert (ref["reverse"] >= 0).all()                                        # symmetric graphs
    rank, rp = _host(tf.rank), _host(row_ptr)
    assert set(rank[rp[g["helix"]]:rp[g["helix"] + 1]].tolist()) == {20}
    assert set(rank[rp[g["planar"]]:rp[g["planar"] + 1]].tolist()) == {19}


def test_the_index(fixture):
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    _check_index(index, ref, int(batch["x"].shape[0]))


@pytest.mark.parametrize("with_tls", [True, False], ids=["tls", "no_tls"])
def test_the_tables_against_the_numpy_rule(fixture, with_tls):
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    got, want = (res, ref) if with_tls else (bare, ref_bare)
    tables = _tables(got)
    na, nt = (int(n) for n in index.table_ptr_host[:, -1])
    assert na == len(want["angles"]["a"]) > 900 and nt == len(want["torsions"]["a"]) > 5000
    worst = at.same_tables(tables, want)
    print(f"{na} angles, {nt} torsions; largest distance from the numpy rule in fp32 units in the last place: {worst}")
    A, T = tables["angles"], tables["torsions"]
    assert (np.diff(A["b"]) >= 0).all() and (T["b"] < T["c"]).all() and (np.diff(T["c"]) >= 0).all()
    assert (T["value"][~np.isnan(T["value"])] > -180.0).all() and (T["value"][~np.isnan(T["value"])] <= 180.0).all()
    if with_tls:
        row = mu.atom_rows(_host(batch["non_H_mask"]))
        rank = _host(tf.rank)
        assert np.array_equal(A["tls_rank"], rank[row[A["b"]]]) and np.array_equal(T["tls_rank"], rank[row[T["c"]]])
        for table, cut in ((A, index.table_ptr_host[0].numpy()), (T, index.table_ptr_host[1].numpy())):
            for name, r in (("helix", 20), ("planar", 19), ("star", 20), ("polymer", 0), ("ring", 0), ("branched", 20)):
                sl = slice(cut[NAMES.index(name)], cut[NAMES.index(name) + 1])
                assert set(table["tls_rank"][sl].tolist()) == {r}, name
                assert np.isfinite(table["libration"][sl]).all() == (r > 0), name
            fitted = np.isfinite(table["libration"])
            assert fitted.sum() > 500 and (table["tls_rank"][fitted] > 0).all()
            bad = slice(cut[NAMES.index("bad")], cut[NAMES.index("bad") + 1])   # a NaN row: whatever its fit gives
            off = (table["tls_rank"] <= 0) | np.isnan(table["value"])
            assert not fitted[off].any() and np.array_equal(np.delete(~fitted, bad), np.delete(off, bad))
            assert (table["libration"][fitted] != table["value"][fitted]).any()
    else:
        for table, other in ((A, res), (T, res)):
            assert np.isnan(table["libration"]).all() and not table["tls_rank"].any()
        for k in ("a", "b", "c", "value"):                                    # the fit changes nothing else
            assert A[k].tobytes() == _host(getattr(res, f"angle_{k}")).tobytes(), k
            assert T[k].tobytes() == _host(getattr(res, f"torsion_{k}")).tobytes(), k
        assert T["d"].tobytes() == _host(res.torsion_d).tobytes()
    _check_stats(got, tables, index)
    assert np.array_equal(_host(got.angle_stats)[:, [0, 2]], want["angle_stats"][:, [0, 2]])
    assert np.array_equal(_host(got.torsion_stats)[:, [0, 1, 2]], want["torsion_stats"][:, [0, 1, 2]])


def test_two_runs_give_the_same_bytes(fixture):
    from cartnet_amd import metrics as gm
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    again_index = gm.angle_index(batch, row_ptr, TOL, rows=int(u.shape[0]))          # with a bond index of its own
    again = gm.angle_table(batch, row_ptr, again_index, tf)
    total = int(index.nbr_ptr[-1])
    assert _host(index.adj)[:total].tobytes() == _host(again_index.adj)[:total].tobytes()
    for k in INDEX:
        assert _host(getattr(index, k)).tobytes() == _host(getattr(again_index, k)).tobytes(), k
    for p, q in zip(res, again):
        assert _host(p).tobytes() == _host(q).tobytes()


def test_the_bond_table_and_the_rigid_bond_test_see_the_same_bonds(fixture):
    """Every torsion's central bond is a row of the bond table of the same index, in its order; and every angle's two
    sources are bond partners of ``b`` in ``bond_test``'s count."""
    from cartnet_amd import metrics as gm
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    bt = gm.bond_table(u, batch, row_ptr, index.bonds)
    rows = list(zip(_host(bt.a).tolist(), _host(bt.b).tolist()))
    b, c = _host(bare.torsion_b), _host(bare.torsion_c)
    counts, at_row = _host(index.torsion_counts), np.repeat(np.arange(len(rows)), _host(index.torsion_counts))
    assert len(at_row) == len(b) and counts.sum() == len(b)
    assert all(rows[k] == (b[s], c[s]) for s, k in enumerate(at_row))
    (src, _), edges = _host(batch["edge_index"]), _host(index.bond_edge)
    assert np.array_equal(src[edges], _host(bt.a)) and _host(batch["cart_dist"])[edges].tobytes() == _host(bt.length).tobytes()
    clean = torch.nan_to_num(u, nan=0.02)                                     # bond_test counts whatever the rows hold
    bonds = _host(gm.bond_test(clean, batch, row_ptr, TOL, mu.THRESHOLD).bonds)
    row = mu.atom_rows(_host(batch["non_H_mask"]))
    centre, per = np.unique(_host(bare.angle_b), return_counts=True)
    d = bonds[row[centre]].astype(np.int64)
    assert np.array_equal(per, d * (d - 1) // 2)                              # all pairs of the centre's bond partners
    partners = {(int(t), int(s)) for s, t in zip(*_host(batch["edge_index"])[:, ref["adj"]])}
    assert all((int(y), int(x)) in partners and (int(y), int(w)) in partners
               for x, y, w in zip(_host(bare.angle_a), _host(bare.angle_b), _host(bare.angle_c)))


def test_a_capped_graph_lists_what_it_holds():
    """B with four bonded neighbours under a cap of 2 (the bond table's case): B keeps A, C and D while F keeps B, so the
    bond B - F is held as B -> F only.  With B the lowest atom it is listed and has no reverse edge."""
    from cartnet_amd import metrics as gm
    c = np.array([6.0, 6.0, 6.0])
    pos = mu.on_grid(np.stack([c, c + [-1.3125, 0, 0], c + [1.4375, 0, 0], c + [0, 1.5, 0], c + [0, -1.5625, 0]]))
    for order, missing in (((0, 1, 2, 3, 4), 1), ((4, 1, 2, 3, 0), 0)):         # B first, then B last
        batch, u, row_ptr = _batch([(pos[list(order)], mu.cubic(12.0), np.full(5, 6), _spd(5, 60))], max_neighbors=2)
        assert int(batch["edge_index"].shape[1]) == 15 and _margin(batch) > 1e-5        # three of four kept per atom
        index = gm.angle_index(batch, row_ptr, TOL)
        ref = _rule(batch)
        _check_index(index, ref, 5)
        res = gm.angle_table(batch, row_ptr, index)
        at.same_tables(_tables(res), ref)
        assert int((index.reverse < 0).sum()) == missing and res.angle_stats[0, 0] == 3   # B's three kept neighbours
        assert res.torsion_stats[0, 0] == len(ref["torsions"]["a"]) == int(index.table_ptr_host[1, -1])


def test_selections_a_repeated_crystal_and_another_order(fixture):
    """Every crystal alone, the whole batch twice, and the whole batch backwards: a crystal's pieces of the tables are the same bytes
    wherever the crystal stands, its atom indices shifted with it."""
    from cartnet_amd import metrics as gm
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    crystals = _crystals()
    whole, cuts, ptr = _tables(bare), index.table_ptr_host.numpy(), _host(batch["ptr"])
    stats = (_host(bare.angle_stats), _host(bare.torsion_stats))
    kinds = (("angles", at.ANGLE_COLUMNS), ("torsions", at.TORSION_COLUMNS))

    def check(selection):
        b, v, rp = _batch([crystals[g] for g in selection])
        idx = gm.angle_index(b, rp, TOL, rows=int(v.shape[0]))
        got = gm.angle_table(b, rp, idx)
        t, p, q = _tables(got), idx.table_ptr_host.numpy(), _host(b["ptr"])
        at.same_tables(t, _rule(b))
        for k, g in enumerate(selection):
            for w, (kind, columns) in enumerate(kinds):
                for key in columns:
                    shift = key in ("a", "b", "c", "d")
                    mine = t[kind][key][p[w, k]:p[w, k + 1]] - (q[k] if shift else 0)
                    want = whole[kind][key][cuts[w, g]:cuts[w, g + 1]] - (ptr[g] if shift else 0)
                    assert mine.tobytes() == want.tobytes(), (selection, g, kind, key)
            assert _host(got.angle_stats)[k].tobytes() == stats[0][g].tobytes(), (selection, g)
            assert _host(got.torsion_stats)[k].tobytes() == stats[1][g].tobytes(), (selection, g)
    for g in range(len(crystals)):                                            # every crystal alone
        check([g])
    check(list(range(len(crystals))) * 2)                                     # the batch twice: every case behind an offset
    check(list(range(len(crystals)))[::-1])                                   # the whole batch, backwards


def test_argument_checks_and_empty_cases(fixture):
    from cartnet_amd import metrics as gm
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    with pytest.raises(ValueError, match="row_ptr"):
        gm.angle_table(batch, row_ptr.to(torch.int32), index)
    with pytest.raises(ValueError, match="index does not belong"):
        gm.angle_table(batch, row_ptr, index._replace(nbr_ptr=index.nbr_ptr[:-1]))
    with pytest.raises(ValueError, match="index does not belong"):
        gm.angle_table(batch, row_ptr, index._replace(bonds=index.bonds._replace(offsets=index.bonds.offsets[:-1])))
    with pytest.raises(ValueError, match="tls does not belong"):
        gm.angle_table(batch, row_ptr, index, tf._replace(params=tf.params[:, :20]))
    with pytest.raises(ValueError, match="tolerance"):
        gm.angle_index(batch, row_ptr, 0.3, bonds=index.bonds)
    with pytest.raises(ValueError, match="batch.ptr"):
        gm.angle_index({k: v for k, v in batch.items() if k != "ptr"}, row_ptr, TOL)
    with pytest.raises(ValueError, match="a forward has overwritten"):
        gm.angle_index(dict(batch, x=torch.zeros(2, 8, device="cuda:0")), row_ptr, TOL)
    dev = u.device
    zero = torch.zeros(2, dtype=torch.int64, device=dev)

    def empty(idx, got, B):
        assert idx.table_ptr_host.tolist() == [[0] * (B + 1)] * 2 and not bool(idx.angle_counts.any())
        assert tuple(got.angle_a.shape) == tuple(got.torsion_d.shape) == tuple(got.torsion_value.shape) == (0,)
        assert got.angle_value.dtype == torch.float32 and got.torsion_a.dtype == torch.int64
        assert got.angle_tls_rank.dtype == torch.int32
        assert got.angle_stats.tolist() == got.torsion_stats.tolist() == [[0.0] * 5] * B
    # M == 0: no atom has a row, nothing is launched
    none = dict(batch, non_H_mask=torch.zeros_like(batch["non_H_mask"]))
    rp0 = torch.zeros_like(row_ptr)
    idx = gm.angle_index(none, rp0, TOL, rows=0)
    empty(idx, gm.angle_table(gm.batch_graph(none, 0), rp0, idx), len(NAMES))
    # N == 0
    nothing = {"x": torch.zeros(0, dtype=torch.int64, device=dev), "edge_index": torch.zeros((2, 0), dtype=torch.int64, device=dev),
               "cart_dist": torch.zeros(0, device=dev), "cart_dir": torch.zeros((0, 3), device=dev), "ptr": zero}
    idx = gm.angle_index(nothing, zero, TOL)
    empty(idx, gm.angle_table(nothing, zero, idx), 1)
    # E == 0, no bonds at all (the crystal "apart") and hydrogens only: empty tables, the crystals' figures zero
    lone = dict(batch, edge_index=torch.zeros((2, 0), dtype=torch.int64, device=dev), cart_dist=torch.zeros(0, device=dev),
                cart_dir=torch.zeros((0, 3), device=dev))
    for b, v, rp in ((lone, u, row_ptr),) + tuple(_batch([_crystals()[g]]) for g in (6, 7)):
        idx = gm.angle_index(b, rp, TOL, rows=int(v.shape[0]))
        empty(idx, gm.angle_table(gm.batch_graph(b, int(v.shape[0])), rp, idx), int(rp.shape[0]) - 1)

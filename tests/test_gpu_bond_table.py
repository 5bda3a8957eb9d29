"""``cartnet_bond_table_count`` and ``cartnet_adp_bond_table`` (csrc/bond_table_ops.hip) against ``bonds.bond_table_host``
on the arrays the kernels read: eleven crystals in one batch -- chains and rings through cell faces and the polymer, a star
whose centre owns twenty bonds, a pair bonded through two images, a crystal without bonds, one of hydrogens only, one with
a NaN row and a negative definite row, a helix and a planar chain for the TLS fit --, a graph capped at two neighbours,
the same crystals alone, twice and in another order, and the cross-checks against ``cartnet_adp_bond_test``.

Indices, order, ``dir``, ``length`` and ``tls_rank`` are exact.  ``delta``, ``lower``, ``upper`` and ``libration`` are
allowed one fp32 unit in the last place (``bond_table_utils.ONE_ULP``): both sides compute in fp64 in the same order and
round once, but the device compiler may contract a product and a sum of these expressions into a fused multiply-add, which
numpy does not, so the fp64 values can differ in their last bits before the rounding."""
import numpy as np
import pytest
import torch

import bond_table_utils as bu
import molecule_utils as mu
import tls_utils as tu

pytestmark = pytest.mark.gpu

TOL = mu.TOL
NAMES = ("small", "long", "polymer", "five", "star", "images", "apart", "hydrogens", "bad", "helix", "planar")


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


def _rule(batch, u, tf=None, tol=TOL):
    from cartnet_amd.bonds import bond_table_host
    extra = dict(params=_host(tf.params), rank=_host(tf.rank)) if tf is not None else {}
    return bond_table_host(_host(u), _host(batch["x"]), _host(batch["edge_index"]), _host(batch["cart_dist"]),
                           _host(batch["cart_dir"]), mu.atom_rows(_host(batch["non_H_mask"])), _host(batch["ptr"]), tol,
                           **extra)


def _table(res) -> dict:
    return {k: _host(getattr(res, k)) for k in bu.COLUMNS}


def _margin(batch, tol=TOL):
    """How far the nearest distance decision of the batch is from its limit."""
    from cartnet_amd.bonds import COVALENT_RADII
    z, (src, tgt), dist = _host(batch["x"]), _host(batch["edge_index"]), _host(batch["cart_dist"])
    r = np.asarray(COVALENT_RADII, dtype=np.float32)
    can = (src != tgt) & (z[src] > 1) & (z[tgt] > 1)
    limit = (r[np.where(can, z[tgt], 0)] + r[np.where(can, z[src], 0)]) + np.float32(tol)
    return np.abs(dist.astype(np.float64) - limit.astype(np.float64))[can].min()


def _check_stats(stats, table, unlisted, ptr, bond_ptr):
    """``crystal_stats`` from the values as stored; only the order of the fp64 sums differs."""
    assert stats.shape == (len(ptr) - 1, 9) and stats.dtype == np.float64
    for g in range(len(ptr) - 1):
        sl = slice(bond_ptr[g], bond_ptr[g + 1])
        ln, d, lib = (table[k][sl].astype(np.float64) for k in ("length", "delta", "libration"))
        fin = np.isfinite(lib)
        grow = (lib - ln)[fin]
        assert stats[g, 0] == len(ln) and stats[g, 1] == unlisted[ptr[g]:ptr[g + 1]].sum() and stats[g, 5] == fin.sum()
        assert stats[g, 8] == (np.isnan(table["lower"][sl]) | np.isnan(table["upper"][sl])).sum()
        assert stats[g, 2] == pytest.approx(ln.sum(), rel=1e-12, abs=1e-300)
        assert stats[g, 6] == pytest.approx(grow.sum(), rel=1e-12, abs=1e-18)
        assert stats[g, 7] == (grow.max() if len(grow) else 0.0)
        if np.isnan(d).any():
            assert np.isnan(stats[g, 3]) and np.isnan(stats[g, 4])
        else:
            assert stats[g, 3] == pytest.approx(np.abs(d).sum(), rel=1e-12, abs=1e-300)
            assert stats[g, 4] == (np.abs(d).max() if len(d) else 0.0)


@pytest.fixture(scope="module")
def fixture():
    """The batch, its index, the molecules and the TLS fit the GPU gives for it, one table with and one without the fit,
    and the numpy rule on the same arrays; computed once."""
    from cartnet_amd import metrics as gm
    batch, u, row_ptr = _batch(_crystals())
    index = gm.bond_index(batch, row_ptr, TOL, rows=int(u.shape[0]))
    mo = gm.molecules(batch, row_ptr, TOL, rows=int(u.shape[0]))
    tf = gm.tls_fit(u, batch, row_ptr, mo)
    res = gm.bond_table(u, batch, row_ptr, index, tf)
    bare = gm.bond_table(u, batch, row_ptr, index)
    return batch, u, row_ptr, index, tf, res, bare, _rule(batch, u, tf), _rule(batch, u)


def test_the_fixture_holds_every_case(fixture):
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    assert _margin(batch) > 1e-5                                              # no decision hangs on a rounding
    ptr, counts = _host(batch["ptr"]), ref["counts"]
    per = np.diff(ref["bond_ptr"]).tolist()
    g = {name: k for k, name in enumerate(NAMES)}
    assert [per[g[n]] for n in ("small", "long", "polymer", "five", "images", "apart", "hydrogens", "bad", "helix", "planar")] \
        == [17, 193, 8, 4, 2, 0, 0, 4, 6, 7]
    assert counts[ptr[g["star"] + 1] - 1] == 20 > 16 and per[g["star"]] > 20  # the centre: past one pass of sixteen lanes
    seg = np.bincount(_host(batch["edge_index"])[1], minlength=len(counts))
    assert seg[ptr[g["star"] + 1] - 1] >= 20 and seg[ptr[g["long"]]:ptr[g["long"] + 1]].min() < 16   # one pass, and two
    at = ref["bond_ptr"][g["images"]]
    assert ref["a"][at:at + 2].tolist() == [ptr[g["images"]]] * 2 and ref["length"][at] == ref["length"][at + 1]
    assert np.array_equal(ref["unlisted"].reshape(-1), np.bincount(ref["a"], minlength=len(counts)))   # symmetric graphs
    rank = _host(tf.rank)
    rp = _host(row_ptr)
    assert set(rank[rp[g["helix"]]:rp[g["helix"] + 1]].tolist()) == {20}
    assert set(rank[rp[g["planar"]]:rp[g["planar"] + 1]].tolist()) == {19}
    assert ref["crystal_stats"][g["bad"], 8] == 4 and ref["crystal_stats"][:, 8].sum() == 4


def test_the_index(fixture):
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    N = int(batch["x"].shape[0])
    assert index.counts.dtype == index.unlisted.dtype == torch.int32 and tuple(index.counts.shape) == (N,)
    assert np.array_equal(_host(index.counts), ref["counts"]) and np.array_equal(_host(index.unlisted), ref["unlisted"])
    assert index.offsets.dtype == torch.int64 and tuple(index.offsets.shape) == (N + 1,)
    assert np.array_equal(_host(index.offsets)[1:], np.cumsum(ref["counts"])) and int(index.offsets[0]) == 0
    assert index.bond_ptr.is_cuda and not index.bond_ptr_host.is_cuda and index.tol == TOL
    assert _host(index.bond_ptr).tolist() == index.bond_ptr_host.tolist() == ref["bond_ptr"].tolist()


@pytest.mark.parametrize("with_tls", [True, False], ids=["tls", "no_tls"])
def test_the_table_against_the_numpy_rule(fixture, with_tls):
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    got, want = (res, ref) if with_tls else (bare, ref_bare)
    table = _table(got)
    nb = int(index.bond_ptr_host[-1])
    assert nb == len(want["a"]) > 250 and table["dir"].shape == (nb, 3)
    worst = bu.same_table(table, want)
    print(f"{nb} bonds; largest distance from the numpy rule in fp32 units in the last place: {worst}")
    assert (table["a"] < table["b"]).all() and (np.diff(table["b"]) >= 0).all()
    if with_tls:
        rank_of_b = _host(tf.rank)[mu.atom_rows(_host(batch["non_H_mask"]))[table["b"]]]
        assert np.array_equal(table["tls_rank"], rank_of_b)
        bp = index.bond_ptr_host.numpy()
        for name, rank in (("helix", 20), ("planar", 19), ("star", 20), ("polymer", 0)):
            sl = slice(bp[NAMES.index(name)], bp[NAMES.index(name) + 1])
            assert set(table["tls_rank"][sl].tolist()) == {rank}, name
            assert np.isfinite(table["libration"][sl]).all() == (rank > 0), name
        fitted = np.isfinite(table["libration"])
        assert fitted.sum() > 200 and (table["tls_rank"][fitted] > 0).all()
        assert np.isnan(table["libration"][table["tls_rank"] <= 0]).all()
        assert (table["libration"][fitted] != table["length"][fitted]).all()
        # the formula on the stored params, in fp64 matrix form
        p = _host(tf.params).astype(np.float64)[mu.atom_rows(_host(batch["non_H_mask"]))[table["b"][fitted]]]
        L = p[:, 6:12][:, [0, 5, 4, 5, 1, 3, 4, 3, 2]].reshape(-1, 3, 3)
        r = table["length"][fitted].astype(np.float64)[:, None] * table["dir"][fitted].astype(np.float64)
        v = r + 0.5 * (np.trace(L, axis1=1, axis2=2)[:, None] * r - np.einsum("npq,nq->np", L, r))
        assert np.abs(table["libration"][fitted] - np.linalg.norm(v, axis=1)).max() <= 2.0 ** -23 * 2.0
    else:
        assert np.isnan(table["libration"]).all() and not table["tls_rank"].any()
        for k in ("a", "b", "dir", "length", "delta", "lower", "upper"):      # the fit changes nothing else
            assert table[k].tobytes() == _host(getattr(res, k)).tobytes(), k
    _check_stats(_host(got.crystal_stats), table, _host(index.unlisted), _host(batch["ptr"]), index.bond_ptr_host.numpy())
    assert np.array_equal(_host(got.crystal_stats)[:, [0, 1, 5, 8]], want["crystal_stats"][:, [0, 1, 5, 8]])


def test_the_rigid_bond_test_sees_the_same_bonds_and_the_same_bits(fixture):
    """Symmetric graphs: every listed bond is two of ``bond_test``'s directed bonds, and the largest ``|delta|`` of a
    crystal has the bits of the largest ``|D|`` that kernel folds."""
    from cartnet_amd import metrics as gm
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    bt = gm.bond_test(u, batch, row_ptr, TOL, mu.THRESHOLD)
    theirs, mine = _host(bt.crystal_stats), _host(bare.crystal_stats)
    assert np.array_equal(2.0 * mine[:, 0], theirs[:, 0]) and np.array_equal(mine[:, 0], mine[:, 1])
    delta, bp = np.abs(_host(bare.delta)), index.bond_ptr_host.numpy()
    for g in range(len(NAMES)):
        d = delta[bp[g]:bp[g + 1]].astype(np.float64)
        if np.isnan(d).any():                                                  # both keep the NaN
            assert np.isnan(theirs[g, 2]) and np.isnan(mine[g, 4]), NAMES[g]
            continue
        top = d.max() if len(d) else 0.0
        assert np.float64(top).tobytes() == theirs[g, 2].tobytes() == mine[g, 4].tobytes(), NAMES[g]
    # per row: the largest |delta| over the bonds that end or start at the row's atom is delta_max
    row = mu.atom_rows(_host(batch["non_H_mask"]))
    a, b = _host(bare.a), _host(bare.b)
    ok = ~np.isnan(delta)
    per = np.zeros(int(u.shape[0]), dtype=np.float32)
    np.maximum.at(per, row[a[ok]], delta[ok])
    np.maximum.at(per, row[b[ok]], delta[ok])
    clean = ~np.isnan(_host(bt.delta_max))
    assert per[clean].tobytes() == _host(bt.delta_max)[clean].tobytes()


def test_two_runs_give_the_same_bytes(fixture):
    from cartnet_amd import metrics as gm
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    again_index = gm.bond_index(batch, row_ptr, TOL, rows=int(u.shape[0]))
    again = gm.bond_table(u, batch, row_ptr, again_index, tf)
    for p, q in zip(tuple(index)[:5] + tuple(res), tuple(again_index)[:5] + tuple(again)):
        assert _host(p).tobytes() == _host(q).tobytes()


def test_a_capped_graph_lists_what_it_holds_and_counts_the_rest():
    """B with four bonded neighbours A, C, D and F at 1.31, 1.44, 1.5 and 1.56 A, none of them bonded to another, under a
    cap of 2: a row longer than the cap keeps the edges up to its third smallest distance (the reference's rule), so B
    keeps A, C and D while F keeps B.  The bond B - F is held as B -> F only; with B the lowest atom it is listed and its
    reverse is missing from the count, with B the highest atom the other way round."""
    from cartnet_amd import metrics as gm
    c = np.array([6.0, 6.0, 6.0])
    pos = mu.on_grid(np.stack([c, c + [-1.3125, 0, 0], c + [1.4375, 0, 0], c + [0, 1.5, 0], c + [0, -1.5625, 0]]))
    for order, want in (((0, 1, 2, 3, 4), (4.0, 3.0)), ((4, 1, 2, 3, 0), (3.0, 4.0))):  # B first, then B last
        batch, u, row_ptr = _batch([(pos[list(order)], mu.cubic(12.0), np.full(5, 6), _spd(5, 60))], max_neighbors=2)
        assert int(batch["edge_index"].shape[1]) == 15 and _margin(batch) > 1e-5        # three of four kept per atom
        index = gm.bond_index(batch, row_ptr, TOL)
        res, ref = gm.bond_table(u, batch, row_ptr, index), _rule(batch, u)
        bu.same_table(_table(res), ref)
        assert res.crystal_stats[0, :2].tolist() == list(want) == ref["crystal_stats"][0, :2].tolist()
        assert np.array_equal(_host(index.unlisted), ref["unlisted"])


def test_selections_a_repeated_crystal_and_another_order(fixture):
    """Every crystal alone, one twice, and the whole batch backwards: a crystal's piece of the table is the same bytes
    wherever the crystal stands, its atom indices shifted with it."""
    from cartnet_amd import metrics as gm
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    crystals = _crystals()
    whole, bp, ptr = _table(bare), index.bond_ptr_host.numpy(), _host(batch["ptr"])
    stats = _host(bare.crystal_stats)

    def piece(g):
        sl = slice(bp[g], bp[g + 1])
        return {k: (whole[k][sl] - ptr[g] if k in ("a", "b") else whole[k][sl]) for k in bu.COLUMNS}

    def check(selection):
        b, v, rp = _batch([crystals[g] for g in selection])
        idx = gm.bond_index(b, rp, TOL, rows=int(v.shape[0]))
        got = gm.bond_table(v, b, rp, idx)
        t, p, q = _table(got), idx.bond_ptr_host.numpy(), _host(b["ptr"])
        bu.same_table(t, _rule(b, v))
        for k, g in enumerate(selection):
            want = piece(g)
            for key in bu.COLUMNS:
                mine = t[key][p[k]:p[k + 1]] - (q[k] if key in ("a", "b") else 0)
                assert mine.tobytes() == want[key].tobytes(), (selection, g, key)
            assert _host(got.crystal_stats)[k].tobytes() == stats[g].tobytes(), (selection, g)
    for g in (0, 4, 5, 7, 8):                                                 # [k]
        check([g])
    check([4, 4])                                                             # a repeated crystal
    check(list(range(len(crystals)))[::-1])                                   # the whole batch, backwards


def test_argument_checks_and_empty_cases(fixture):
    from cartnet_amd import metrics as gm
    batch, u, row_ptr, index, tf, res, bare, ref, ref_bare = fixture
    with pytest.raises(ValueError, match="u must be"):
        gm.bond_table(u.double(), batch, row_ptr, index)
    with pytest.raises(ValueError, match="row_ptr"):
        gm.bond_table(u, batch, row_ptr.to(torch.int32), index)
    with pytest.raises(ValueError, match="index does not belong"):
        gm.bond_table(u, batch, row_ptr, index._replace(offsets=index.offsets[:-1]))
    with pytest.raises(ValueError, match="tls does not belong"):
        gm.bond_table(u, batch, row_ptr, index, tf._replace(params=tf.params[:, :20]))
    with pytest.raises(ValueError, match="batch.ptr"):
        gm.bond_index({k: v for k, v in batch.items() if k != "ptr"}, row_ptr, TOL)
    with pytest.raises(ValueError, match="a forward has overwritten"):
        gm.bond_index(dict(batch, x=torch.zeros(2, 8, device="cuda:0")), row_ptr, TOL)
    dev = u.device
    zero = torch.zeros(2, dtype=torch.int64, device=dev)
    # M == 0: no atom has a row, nothing is launched
    none = dict(batch, non_H_mask=torch.zeros_like(batch["non_H_mask"]))
    rp0 = torch.zeros_like(row_ptr)
    idx = gm.bond_index(none, rp0, TOL, rows=0)
    got = gm.bond_table(u[:0], none, rp0, idx)
    assert int(idx.bond_ptr_host[-1]) == 0 and not bool(idx.counts.any()) and not bool(idx.unlisted.any())
    assert tuple(got.a.shape) == (0,) and tuple(got.dir.shape) == (0, 3) and float(got.crystal_stats.abs().sum()) == 0.0
    # N == 0
    empty = {"x": torch.zeros(0, dtype=torch.int64, device=dev), "edge_index": torch.zeros((2, 0), dtype=torch.int64, device=dev),
             "cart_dist": torch.zeros(0, device=dev), "cart_dir": torch.zeros((0, 3), device=dev), "ptr": zero}
    idx = gm.bond_index(empty, zero, TOL)
    assert idx.bond_ptr_host.tolist() == [0, 0]
    assert gm.bond_table(u[:0], empty, zero, idx).crystal_stats.tolist() == [[0.0] * 9]
    # E == 0, and edges but no bonds at all: an empty table, the crystals' figures zero
    lone = dict(batch, edge_index=torch.zeros((2, 0), dtype=torch.int64, device=dev), cart_dist=torch.zeros(0, device=dev),
                cart_dir=torch.zeros((0, 3), device=dev))
    for b, v, rp in ((lone, u, row_ptr),) + (_batch([_crystals()[6]]),):
        idx = gm.bond_index(b, rp, TOL, rows=int(v.shape[0]))
        got = gm.bond_table(v, b, rp, idx)
        assert int(idx.bond_ptr_host[-1]) == 0 and tuple(got.delta.shape) == (0,) and got.delta.dtype == torch.float32
        assert float(got.crystal_stats.abs().sum()) == 0.0 and got.a.dtype == torch.int64 and got.tls_rank.dtype == torch.int32

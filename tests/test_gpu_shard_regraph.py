"""``DeviceShard.with_radius_graph``: the radius graph of a whole resident shard rebuilt in one GPU pass
(csrc/radius_graph.hip, cn_sr_kernel) -- against the reference's own graphs (tests/golden/radius_graph*.npz), bitwise
against the same pass run one crystal at a time, and composed with the other whole-shard steps."""
import numpy as np
import pytest
import torch

import golden_utils as gu
from cartnet_amd import shard
from cartnet_amd.data import Batch, lattice_margins, optimize_cell, remove_hydrogens
from cartnet_amd.synthetic import make_geometry, radius_graph_pbc_single

pytestmark = pytest.mark.gpu

EDGE_KEYS = ("edge_ptr", "edge_src", "edge_tgt", "cart_dist", "cart_dir")


def _slice(s, g):
    """(edge_index [2,e] int64 inside the crystal, dist, dir) of crystal ``g`` of a resident shard."""
    ep = s.t["edge_ptr"].cpu()
    assert np.array_equal(ep.numpy(), s.edge_ptr)
    a, b = int(ep[g]), int(ep[g + 1])
    ei = torch.stack((s.t["edge_src"][a:b], s.t["edge_tgt"][a:b])).cpu().to(torch.int64)
    return ei, s.t["cart_dist"][a:b].cpu(), s.t["cart_dir"][a:b].cpu()


def test_reference_goldens_packed_as_one_geometry_only_shard():
    """Every crystal of the two reference fixtures in ONE geometry-only shard, regraphed once per (radius, cap) and sliced
    per crystal: integers bit-exact, dist rtol 1e-6, dir atol 1e-6 (the bounds of tests/test_gpu_radius_graph.py:11-14)."""
    z5, zr = np.load(gu.GOLDEN + "/radius_graph.npz"), np.load(gu.GOLDEN + "/radius_graph_radii.npz")
    t5, tr = (lambda k: torch.from_numpy(z5[k])), (lambda k: torch.from_numpy(zr[k]))
    names = ["c0", "c1", "c2", "cubic", "hexagonal", "triclinic", "pair0", "pair1"]
    geo = [(t5(f"pos{i}"), t5(f"cell{i}")) for i in range(3)] + [(t5("cubic_pos"), t5("cubic_cell"))]
    geo += [(tr(f"{n}_pos"), tr(f"{n}_cell")) for n in ("hexagonal", "triclinic", "pair0", "pair1")]
    base = shard.DeviceShard.from_data_list([gu.geometry(p, c) for p, c in geo])
    assert not base.has_graph and base.graph is None
    # (radius, cap) -> [(crystal, golden edge_index, dist, dir)]
    cases = {(5.0, None): [(f"c{i}", t5(f"edge_index{i}"), t5(f"dist{i}"), t5(f"dir{i}")) for i in range(3)],
             (5.0, 8): [(f"c{i}", t5(f"cap8_edge_index{i}"), t5(f"cap8_dist{i}"), t5(f"cap8_dir{i}")) for i in range(3)]}
    for k in (10, 25):
        cases[(5.0, k)] = [("cubic", t5(f"cubic_cap{k}_edge_index"), t5(f"cubic_cap{k}_dist"), t5(f"cubic_cap{k}_dir"))]
    for r in zr["radii"].tolist():
        for tag, cap in (("", None), ("cap8_", 8)):
            cases[(r, cap)] = [(n, tr(f"{n}_r{r}_{tag}edge_index"), tr(f"{n}_r{r}_{tag}dist"), tr(f"{n}_r{r}_{tag}dir"))
                               for n in ("hexagonal", "triclinic")]
    for i in range(2):
        cases.setdefault((float(zr[f"pair{i}_radius"]), None), []).append(
            (f"pair{i}", tr(f"pair{i}_edge_index"), torch.zeros(0), torch.zeros(0, 3)))
        cases.setdefault((float(zr[f"pair{i}_radius_up"]), None), []).append(
            (f"pair{i}", tr(f"pair{i}_up_edge_index"), tr(f"pair{i}_up_dist"), tr(f"pair{i}_up_dir")))
    # 4 at radius 5, 2 radii x {no cap, cap 8}, and the pairs' 4 radii of which pair0's 3.7 is already there; 20 graphs:
    # 3 + 3 + 1 + 1 at radius 5, 2 crystals x 4, and each pair below and above its threshold
    assert len(cases) == 11 and sum(len(v) for v in cases.values()) == 20
    worst_dist, worst_dir, checked = 0.0, 0.0, 0
    for (radius, cap), want in cases.items():
        out = base.with_radius_graph(radius, cap)
        assert out.has_graph and out.graph == {"radius": radius, "max_neighbors": cap}
        for name, ref_ei, ref_dist, ref_dir in want:
            ei, dist, dirs = _slice(out, names.index(name))
            assert torch.equal(ei, ref_ei.to(torch.int64)), (radius, cap, name)
            if name.startswith("pair"):
                assert ei.shape[1] == (0 if ref_dist.numel() == 0 else 2), (radius, name)
            if ref_dist.numel():
                worst_dist = max(worst_dist, float(((dist - ref_dist).abs() / ref_dist.abs()).max()))
                worst_dir = max(worst_dir, float((dirs - ref_dir).abs().max()))
                assert torch.allclose(dist, ref_dist, rtol=1e-6, atol=0), (radius, cap, name)
                assert torch.allclose(dirs, ref_dir, rtol=0, atol=1e-6), (radius, cap, name)
            checked += 1
    assert checked == 20
    print(f"\nshard regraph vs reference goldens: {checked} crystal graphs, worst dist rel {worst_dist:.3e}, "
          f"worst dir abs {worst_dir:.3e}")
    # the cubic cap-10 row keeps its tied shell: 18 edges per atom, not 10
    ei, _, _ = _slice(base.with_radius_graph(5.0, 10), names.index("cubic"))
    assert int(torch.bincount(ei[1]).max()) == 18


@pytest.fixture(scope="module")
def ragged():
    items = gu.ragged()
    return items, shard.DeviceShard.from_data_list(items)


@pytest.mark.parametrize("radius", [4.0, 5.0, 6.0])
def test_many_crystals_in_one_pass_bitwise_equal_to_one_crystal_per_pass(ragged, radius):
    """The shard-wide pass over ten ragged crystals against ``radius_graph_pbc`` called once per crystal -- the same pass
    over a single crystal, which tests/test_gpu_radius_graph.py pins to the reference."""
    from cartnet_amd.graph import radius_graph_pbc
    items, base = ragged
    uncapped, bites = base.with_radius_graph(radius), 0
    for cap in (None, 12, 25, 10_000):
        one = [radius_graph_pbc(d.pos.cuda(), d.cell.cuda(), torch.tensor([0, d.pos.shape[0]]).cuda(), radius, cap)
               for d in items]
        e = [int(ei.shape[1]) for ei, _, _ in one]
        want = {"edge_ptr": torch.tensor([0] + e, dtype=torch.int64).cumsum(0),
                "edge_src": torch.cat([ei[0] for ei, _, _ in one]).cpu().to(torch.int32),
                "edge_tgt": torch.cat([ei[1] for ei, _, _ in one]).cpu().to(torch.int32),
                "cart_dist": torch.cat([d for _, d, _ in one]).cpu(), "cart_dir": torch.cat([v for _, _, v in one]).cpu()}
        assert all(ei.dtype == torch.int64 for ei, _, _ in one) and want["cart_dir"].shape == (sum(e), 3)
        got = base.with_radius_graph(radius, cap)
        for k in EDGE_KEYS:
            ref = want[k]
            assert got.t[k].dtype == ref.dtype and torch.equal(got.t[k].cpu(), ref), (radius, cap, k)
        assert np.array_equal(got.edge_ptr, want["edge_ptr"].numpy())
        ep = got.edge_ptr
        assert ep[1] == 0 and ep[6] == ep[5] and ep[10] == ep[9]            # the far pairs have no edges
        bites += int(ep[-1]) < int(uncapped.edge_ptr[-1])
        if cap == 10_000:                                                   # a cap nobody reaches is no cap
            assert all(torch.equal(got.t[k], uncapped.t[k]) for k in EDGE_KEYS)
    assert bites >= 1                                                       # the d^2 / cutoff pass really ran


def test_two_calls_give_identical_bytes_and_leave_the_source_alone(ragged):
    _, base = ragged
    src = base.with_radius_graph(5.0)
    before = {k: (v.data_ptr(), v.clone()) for k, v in src.t.items()}
    a, b = src.with_radius_graph(6.0, 12), src.with_radius_graph(6.0, 12)
    for k in EDGE_KEYS:
        assert a.t[k].data_ptr() != b.t[k].data_ptr() and torch.equal(a.t[k], b.t[k]), k
        assert a.t[k].data_ptr() != src.t[k].data_ptr()
    assert np.array_equal(a.edge_ptr, b.edge_ptr)
    for k, (ptr, val) in before.items():
        assert src.t[k].data_ptr() == ptr and torch.equal(src.t[k], val), k
    for k in src.t:
        if k not in EDGE_KEYS:
            assert a.t[k].data_ptr() == src.t[k].data_ptr(), k               # shared, not copied
    assert a.atom_ptr is src.atom_ptr and a.y_ptr is src.y_ptr
    assert src.graph == {"radius": 5.0, "max_neighbors": None} and a.graph == {"radius": 6.0, "max_neighbors": 12}


def _dense(first, sizes):
    """ADP-shaped synthetic geometries, shrunk to ~2.4 x the density so that the cap of 25 bites at radius 5."""
    out = []
    for g, n in enumerate(sizes):
        d = make_geometry(first + g, n)
        d.pos, d.cell = 0.75 * d.pos, 0.75 * d.cell
        gap, cos = lattice_margins(d.cell[0])
        assert gap >= 1e-4 and cos >= 1e-4                                  # host and device pick the same lattice basis
        out.append(d)
    return out


def test_composes_with_hydrogen_removal_canonical_cell_and_collate():
    geo = _dense(780, (30, 45, 12, 64, 38, 7))
    host, full_edges = [], 0
    for d in geo:
        ei, dist, dirs = radius_graph_pbc_single(d.pos, d.cell[0], 5.0, max_neighbors=25)
        full_edges += radius_graph_pbc_single(d.pos, d.cell[0], 5.0)[0].shape[1]
        h = d.clone()
        h.edge_index, h.cart_dist, h.cart_dir = ei, dist, dirs
        host.append(optimize_cell(remove_hydrogens(h)))
    assert sum(int(h.edge_index.shape[1]) for h in host) < full_edges
    out = shard.DeviceShard.from_data_list(geo).with_radius_graph(5.0, 25)
    assert int(out.edge_ptr[-1]) < full_edges                               # the cap bites
    out = out.without_hydrogens().with_optimized_cell()
    sel = [3, 0, 5, 1, 4, 2]
    b, ref = out.collate(sel), Batch.from_data_list([host[i] for i in sel])
    for k in ("x", "non_H_mask", "batch", "ptr", "edge_index"):
        got, want = getattr(b, k).cpu(), getattr(ref, k)
        assert got.dtype == want.dtype and torch.equal(got, want), k
    assert torch.allclose(b.cart_dist.cpu(), ref.cart_dist, rtol=1e-6, atol=0)
    assert torch.allclose(b.cart_dir.cpu(), ref.cart_dir, rtol=0, atol=1e-6)
    assert torch.equal(b.pos.cpu(), ref.pos) and torch.equal(b.temperature.cpu(), ref.temperature)   # only copied
    for k in ("cell", "y"):              # the canonical-cell step's own budget (tests/test_gpu_optimize_cell.py: BUDGET)
        got, want = getattr(b, k).cpu(), getattr(ref, k)
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), k
    from cartnet_amd.comformer import iComformer, make_icomformer_state_dict
    m = iComformer(32)
    m.load_state_dict(make_icomformer_state_dict(32, seed=5))
    m = m.to("cuda:0").train()
    pred, true = m(b)
    loss = (pred - true).abs().mean()
    loss.backward()
    assert torch.isfinite(pred).all() and torch.isfinite(loss)
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)


def test_errors_and_degenerate_cells():
    items = gu.ragged()[1:5]
    geo = shard.DeviceShard.from_data_list(items)
    for what in (lambda: geo.collate([0]), geo.without_hydrogens, geo.with_optimized_cell):
        with pytest.raises(ValueError, match="with_radius_graph"):
            what()
    full = shard.pack_with_gpu_graph(items, 5.0)
    for drop in ("pos", "cell"):
        arrays = {k: v for k, v in full.items() if k != drop}
        with pytest.raises(ValueError, match="pos and cell"):
            shard.DeviceShard(arrays).with_radius_graph(5.0)
    with pytest.raises(ValueError):
        shard.DeviceShard({k: v for k, v in shard.pack(items).items() if k != "cell"})     # geometry-only needs both
    # zero-volume cells: the repetition cap of cn_rg_reps_kernel bounds the image walk, the call returns, and the healthy
    # crystal behind them still gets its exact graph
    good = items[3]
    flat = torch.tensor([[4.0, 0, 0], [0, 4.0, 0], [4.0, 4.0, 0]])
    pts = torch.rand(5, 3, generator=torch.Generator().manual_seed(3)) * 3
    bad = shard.DeviceShard.from_data_list([gu.geometry(pts, flat), gu.geometry(pts, torch.zeros(3, 3)), good])
    for cap in (None, 8):
        out = bad.with_radius_graph(5.0, cap)
        torch.cuda.synchronize()
        assert out.t["edge_src"].shape[0] == int(out.edge_ptr[-1]) == out.t["cart_dist"].shape[0]
        ei, dist, _ = _slice(out, 2)
        ref_ei, ref_dist, _ = radius_graph_pbc_single(good.pos, good.cell[0], 5.0, max_neighbors=cap)
        assert torch.equal(ei, ref_ei) and torch.allclose(dist, ref_dist, rtol=1e-6, atol=0)

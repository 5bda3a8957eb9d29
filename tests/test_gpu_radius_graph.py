"""GPU periodic radius graph against the reference's radius_graph_pbc (golden fixture) and the CPU restatement."""
import numpy as np
import pytest
import torch

import golden_utils as gu

pytestmark = pytest.mark.gpu


def _check(ei, dist, dirs, ref_ei, ref_dist, ref_dir):
    assert torch.equal(ei.cpu(), ref_ei)                                   # integers: bit-exact, same order
    assert torch.allclose(dist.cpu(), ref_dist, rtol=1e-6, atol=0)         # a few fp32 ulps (image offsets round differently)
    assert torch.allclose(dirs.cpu(), ref_dir, rtol=0, atol=1e-6)


def test_matches_reference_golden_fixture():
    from cartnet_amd.graph import radius_graph_pbc
    z = np.load(gu.GOLDEN + "/radius_graph.npz")
    for i in range(3):
        pos, cell = torch.from_numpy(z[f"pos{i}"]), torch.from_numpy(z[f"cell{i}"])
        ptr = torch.tensor([0, pos.shape[0]])
        ei, dist, dirs = radius_graph_pbc(pos.cuda(), cell.view(1, 3, 3).cuda(), ptr.cuda(), 5.0)
        _check(ei, dist, dirs, torch.from_numpy(z[f"edge_index{i}"]), torch.from_numpy(z[f"dist{i}"]),
               torch.from_numpy(z[f"dir{i}"]))


def test_neighbour_cap_matches_reference_golden_fixture():
    from cartnet_amd.graph import radius_graph_pbc
    z = np.load(gu.GOLDEN + "/radius_graph.npz")
    cases = [(f"pos{i}", f"cell{i}", 8, f"cap8_edge_index{i}", f"cap8_dist{i}", f"cap8_dir{i}") for i in range(3)]
    cases += [("cubic_pos", "cubic_cell", k, f"cubic_cap{k}_edge_index", f"cubic_cap{k}_dist", f"cubic_cap{k}_dir")
              for k in (10, 25)]
    for pk, ck, k, ek, dk, vk in cases:
        pos, cell = torch.from_numpy(z[pk]), torch.from_numpy(z[ck])
        ptr = torch.tensor([0, pos.shape[0]])
        ei, dist, dirs = radius_graph_pbc(pos.cuda(), cell.view(1, 3, 3).cuda(), ptr.cuda(), 5.0, max_neighbors=k)
        _check(ei, dist, dirs, torch.from_numpy(z[ek]), torch.from_numpy(z[dk]), torch.from_numpy(z[vk]))


def test_neighbour_cap_on_a_batch_matches_cpu_builder():
    """Dense crystals (up to ~60 neighbours), the iComformer cap of 25, several crystals per call; a cap nobody
    reaches returns the uncapped graph."""
    from cartnet_amd.graph import radius_graph_pbc
    from cartnet_amd.synthetic import radius_graph_pbc_single
    gen = torch.Generator().manual_seed(5)
    pos_l, cell_l, ref = [], [], []
    for n, a in ((40, 7.0), (150, 11.0), (3, 3.1), (64, 8.0)):
        cell = a * torch.eye(3) + 0.3 * torch.randn(3, 3, generator=gen)
        pos = torch.rand(n, 3, generator=gen) @ cell
        pos_l.append(pos); cell_l.append(cell)
        ref.append(radius_graph_pbc_single(pos, cell, 5.0, max_neighbors=25))
    off = 0
    ref_ei, ref_d, ref_v = [], [], []
    for (ei, d, v), p in zip(ref, pos_l):
        ref_ei.append(ei + off); ref_d.append(d); ref_v.append(v); off += p.shape[0]
    ptr = torch.tensor([0] + list(np.cumsum([p.shape[0] for p in pos_l])))
    pos, cell = torch.cat(pos_l).cuda(), torch.stack(cell_l).cuda()
    ei, dist, dirs = radius_graph_pbc(pos, cell, ptr.cuda(), 5.0, max_neighbors=25)
    _check(ei, dist, dirs, torch.cat(ref_ei, 1), torch.cat(ref_d), torch.cat(ref_v))
    deg = torch.bincount(ei[1].cpu(), minlength=pos.shape[0])
    assert int(deg.max()) >= 25 and int(deg.max()) < 40
    full = radius_graph_pbc(pos, cell, ptr.cuda(), 5.0)
    big = radius_graph_pbc(pos, cell, ptr.cuda(), 5.0, max_neighbors=10_000)
    assert all(torch.equal(a, b) for a, b in zip(full, big)) and full[0].shape[1] > ei.shape[1]


def test_batch_of_crystals_matches_cpu_builder_and_feeds_the_model():
    from cartnet_amd.data import Batch
    from cartnet_amd.graph import radius_graph_pbc
    from cartnet_amd.synthetic import make_crystal
    items = [make_crystal(600 + g, n) for g, n in enumerate((1, 2, 37, 194, 90))]
    b = Batch.from_data_list(items)
    ei, dist, dirs = radius_graph_pbc(b.pos.cuda(), b.cell.cuda(), b.ptr.cuda(), 5.0)
    _check(ei, dist, dirs, b.edge_index, b.cart_dist, b.cart_dir)
    assert bool((ei[1][1:] >= ei[1][:-1]).all())
    # end to end: the GPU-built graph drives the network to the same prediction as the CPU-built one
    from cartnet_amd.model import CartNet, make_state_dict
    m = CartNet(64, 32, 2)
    m.load_state_dict(make_state_dict(64, 32, 2, seed=9))
    m = m.cuda().eval()
    b1 = b.clone(); b1.num_graphs = b.num_graphs; b1.to("cuda:0")
    b2 = b.clone(); b2.num_graphs = b.num_graphs; b2.to("cuda:0")
    b2.edge_index, b2.cart_dist, b2.cart_dir = ei, dist, dirs
    with torch.no_grad():
        p1, _ = m(b1)
        p2, _ = m(b2)
    assert (p1 - p2).abs().max().item() <= 1e-5 * p1.abs().max().item()


def test_count_and_fill_passes_agree_on_pairs_at_the_cutoff():
    """Regression (round 2): 256 ragged crystals in one launch, among them one (chunk index 180) with a pair whose d^2
    lies within an ulp of radius^2.  The count and the fill pass used to round d^2 differently (compiler-chosen FMA
    contraction), leaving two edge slots unwritten and shifting every later crystal; the translation unit is now built
    with -ffp-contract=off.  Checks: targets sorted, every slot written, that crystal identical to the host builder
    (which restates the reference's dataset/utils.py bit for bit, tests/test_oracle_golden.py)."""
    from cartnet_amd.graph import radius_graph_pbc
    from cartnet_amd.synthetic import make_geometry, radius_graph_pbc_single
    part = [make_geometry(30000 + i, None) for i in range(2560, 2816)]
    pos = torch.cat([d.pos for d in part]).cuda()
    cell = torch.cat([d.cell for d in part]).cuda()
    sizes = torch.tensor([int(d.x.shape[0]) for d in part], dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)]).cuda()
    ei, dist, dirs = radius_graph_pbc(pos, cell, ptr, 5.0)
    assert bool((ei[1][1:] >= ei[1][:-1]).all())
    assert bool((dist > 0.01).all()) and bool((dist <= 5.0).all())
    gid = torch.repeat_interleave(torch.arange(len(part), device="cuda"), ptr[1:] - ptr[:-1])
    assert bool((gid[ei[0]] == gid[ei[1]]).all())
    for k in (90, 180, 255):
        sel = gid[ei[1]] == k
        mine = (ei[:, sel] - ptr[k]).cpu()
        ref_ei, ref_dist, ref_dir = radius_graph_pbc_single(part[k].pos, part[k].cell[0], 5.0)
        assert torch.equal(mine, ref_ei), k
        assert torch.allclose(dist[sel].cpu(), ref_dist, rtol=1e-6, atol=0)          # fp32 rounding of sqrt / division
        assert torch.allclose(dirs[sel].cpu(), ref_dir, rtol=0, atol=1e-6), k


def test_degenerate_cells_do_not_hang_or_fault():
    """A zero-volume cell (coplanar lattice vectors), an all-zero cell and a needle-thin one: the reference divides by
    the volume and produces inf / NaN repetition counts; here the counts are capped and the image box tolerates
    non-finite bounds, so the call returns (whatever edges it returns) instead of looping or faulting, and a healthy
    crystal in the same batch still gets its exact graph."""
    from cartnet_amd.graph import radius_graph_pbc
    from cartnet_amd.synthetic import make_geometry, radius_graph_pbc_single
    good = make_geometry(777, 40)
    cells = [torch.tensor([[4.0, 0, 0], [0, 4.0, 0], [4.0, 4.0, 0]]),          # coplanar: volume 0
             torch.zeros(3, 3),
             torch.tensor([[6.0, 0, 0], [0, 6.0, 0], [0, 0, 1e-4]]),            # needle: thousands of images wanted
             good.cell[0]]
    pos = [torch.rand(5, 3, generator=torch.Generator().manual_seed(i)) * 3 for i in range(3)] + [good.pos]
    ptr = torch.tensor([0, 5, 10, 15, 15 + good.pos.shape[0]])
    ei, dist, dirs = radius_graph_pbc(torch.cat(pos).cuda(), torch.stack(cells).cuda(), ptr.cuda(), 5.0)
    torch.cuda.synchronize()
    assert ei.shape[0] == 2 and dist.shape[0] == ei.shape[1]
    sel = ei[1] >= 15
    ref_ei, ref_dist, _ = radius_graph_pbc_single(good.pos, good.cell[0], 5.0)
    assert torch.equal((ei[:, sel] - 15).cpu(), ref_ei)
    assert torch.allclose(dist[sel].cpu(), ref_dist, rtol=1e-6, atol=0)


def test_batch_indices_are_the_one_crystal_indices_plus_ptr():
    """The library writes atom indices inside the crystal; ``radius_graph_pbc`` adds ``ptr[g]`` per edge on the device.
    Ten ragged crystals (tests/golden_utils.py: ragged -- 251 atoms; crystals without an edge first, in the middle and
    last; 64, 65 and 70 atoms) in one call against ten one-crystal calls with the offsets added: identical bytes."""
    from cartnet_amd.graph import radius_graph_pbc
    from cartnet_amd.synthetic import radius_graph_pbc_single
    items = gu.ragged()
    sizes = [int(d.pos.shape[0]) for d in items]
    ptr = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)
    pos, cell = torch.cat([d.pos for d in items]).cuda(), torch.cat([d.cell for d in items]).cuda()
    edges = {}
    for cap in (None, 12):
        ei, dist, dirs = radius_graph_pbc(pos, cell, ptr.cuda(), 5.0, max_neighbors=cap)
        one = [radius_graph_pbc(d.pos.cuda(), d.cell.cuda(), torch.tensor([0, n]).cuda(), 5.0, max_neighbors=cap)
               for d, n in zip(items, sizes)]
        assert [int(one[g][0].shape[1]) for g in (0, 5, 9)] == [0, 0, 0]          # the far pairs have no edges
        assert ei.dtype == torch.int64 and ei.shape[0] == 2
        assert torch.equal(ei, torch.cat([o[0] + int(ptr[g]) for g, o in enumerate(one)], 1)), cap
        assert torch.equal(dist, torch.cat([o[1] for o in one])), cap
        assert torch.equal(dirs, torch.cat([o[2] for o in one])), cap
        assert bool((ei[1][1:] >= ei[1][:-1]).all())
        host = [radius_graph_pbc_single(d.pos, d.cell[0], 5.0, max_neighbors=cap)[0] + int(ptr[g])
                for g, d in enumerate(items)]
        assert torch.equal(ei.cpu(), torch.cat(host, 1)), cap
        edges[cap] = int(ei.shape[1])
    assert 0 < edges[12] < edges[None]                                            # the cap bites on this batch


# ---------------------------------------------------------------------------------------------------------------
# Away from radius 5 and nearly cubic cells.  The reference is the host builder called per crystal (bit-identical to the
# reference's dataset/utils.py on these cells, atom counts and radii: tests/golden/make_golden.py asserts it for the
# radius_graph_radii fixture); the GPU is called on batches, so repetition counts differ per crystal within a launch.
_OBLIQUE = [("hexagonal", False), ("rhombohedral", False), ("triclinic", False), ("triclinic", True), ("small", False)]
_HOST_GRAPHS = {}


def _crystal(name, n, rotate=False):
    return gu.crystal(name, n, seed=1000 + 10 * n + sorted(gu.CELLS).index(name) + (5 if rotate else 0), rotate=rotate)


def _host_graph(pos, cell, radius, cap=None):
    """Host-builder graph of one crystal, computed once per (crystal, radius, cap) and shared between tests."""
    from cartnet_amd.synthetic import radius_graph_pbc_single
    key = (pos.numpy().tobytes(), cell.numpy().tobytes(), radius, cap)
    if key not in _HOST_GRAPHS:
        _HOST_GRAPHS[key] = radius_graph_pbc_single(pos, cell, radius, max_neighbors=cap)
    return _HOST_GRAPHS[key]


def _gpu_batch_against_host(crystals, radius, cap=None):
    """One GPU call on the whole batch against the per-crystal host graphs; returns the GPU edge_index."""
    from cartnet_amd.graph import radius_graph_pbc
    ref_ei, ref_d, ref_v, off = [], [], [], 0
    for pos, cell in crystals:
        ei, d, v = _host_graph(pos, cell, radius, cap)
        ref_ei.append(ei + off); ref_d.append(d); ref_v.append(v); off += pos.shape[0]
    ptr = torch.tensor([0] + list(np.cumsum([p.shape[0] for p, _ in crystals])))
    pos, cell = torch.cat([p for p, _ in crystals]).cuda(), torch.stack([c for _, c in crystals]).cuda()
    ei, dist, dirs = radius_graph_pbc(pos, cell, ptr.cuda(), radius, max_neighbors=cap)
    _check(ei, dist, dirs, torch.cat(ref_ei, 1), torch.cat(ref_d), torch.cat(ref_v))
    return ei


@pytest.mark.parametrize("radius", [2.0, 3.5, 6.0, 8.0])
def test_oblique_cells_and_other_radii_match_cpu_builder(radius):
    """Hexagonal, rhombohedral (50 degrees), triclinic, rotated triclinic and a cell smaller than the radius (repetition
    counts of 3 and more), 1 / 3 / 70 atoms (70: more than one 64-lane source round), all crystals of a radius in one
    batch.  The 2.6 x 2.9 x 3.3 cell keeps its 70 atoms up to radius 3.5 (~36k edges there)."""
    crystals = [_crystal(name, n, rot) for name, rot in _OBLIQUE for n in (1, 3, 70)
                if not (name == "small" and n == 70 and radius > 3.5)]
    assert len(crystals) == (15 if radius <= 3.5 else 14)
    ei = _gpu_batch_against_host(crystals, radius)
    assert ei.shape[1] > 0 and bool((ei[1][1:] >= ei[1][:-1]).all())
    if radius >= 6.0:         # the condition this case is for: some crystal needs three or more images along an axis
        cell = gu.lattice(*gu.CELLS["small"])
        height = torch.det(cell).abs() / torch.linalg.cross(cell[1], cell[2]).norm()
        assert radius / float(height) > 2.0


def test_atoms_stored_outside_the_unit_cell_match_cpu_builder():
    """A third of the atoms moved by integer lattice translations in [-2, 2]^3.  The reference only tests the images in
    [-R_d, R_d]; the kernel's per-pair image box is clamped to the same range and must emit exactly those edges.
    Image offsets reach 20 A here, so this is also the case that sees the rounding ORDER of the offset sum: with
    (a1 u1 + a3 u3) + a2 u2 in the kernel against (a1 u1 + a2 u2) + a3 u3 in this host's torch.bmm, two of 21,570
    directions were off by 1.27e-6 (a pair 0.74 A apart, offset one ulp apart); with the same order the maximum is 1.2e-7."""
    pos, cell = _crystal("triclinic", 70)
    gen = torch.Generator().manual_seed(77)
    shift = torch.randint(-2, 3, (70, 3), generator=gen).to(torch.float32)
    shift[torch.randperm(70, generator=gen)[70 // 3:]] = 0.0
    assert int((shift.abs().sum(1) > 0).sum()) >= 15
    moved = pos + shift @ cell
    ei = _gpu_batch_against_host([(moved, cell)], 6.0)
    inside = _host_graph(pos, cell, 6.0)[0]
    assert ei.shape[1] != inside.shape[1]        # the clamped range really drops (or adds) images for the moved atoms


@pytest.mark.parametrize("radius", [3.5, 6.0])
def test_neighbour_cap_on_oblique_cells_matches_cpu_builder(radius):
    crystals = [_crystal("hexagonal", 70), _crystal("triclinic", 70)]
    ei = _gpu_batch_against_host(crystals, radius, cap=12)
    full = sum(_host_graph(p, c, radius)[0].shape[1] for p, c in crystals)
    assert 12 * 140 <= ei.shape[1] < full


@pytest.mark.parametrize("radius,y", gu.THRESHOLD_PAIRS)
def test_cutoff_is_the_fp32_rounding_of_the_double_product(radius, y):
    """The reference keeps d^2 <= radius * radius with the product taken in double (dataset/utils.py:202) and rounded to
    fp32 for the comparison.  These pairs have an fp32 d^2 equal to fp32(radius) * fp32(radius), one ulp above that
    threshold: no edge at the radius, both edges one fp32 step above it -- on the host builder and on the GPU."""
    from cartnet_amd.graph import radius_graph_pbc
    from cartnet_amd.synthetic import radius_graph_pbc_single
    pos, cell = gu.threshold_pair(y)
    d2 = (pos[1] ** 2).sum().numpy()
    assert d2 == np.float32(radius) * np.float32(radius) and d2 > np.float32(radius * radius)   # between the thresholds
    ptr = torch.tensor([0, 2]).cuda()
    assert radius_graph_pbc_single(pos, cell, radius)[0].shape[1] == 0
    ei, dist, dirs = radius_graph_pbc(pos.cuda(), cell.view(1, 3, 3).cuda(), ptr, radius)
    print(f"radius {radius}: GPU edges {ei.shape[1]} (reference 0)")
    assert ei.shape[1] == 0
    up = float(np.nextafter(np.float32(radius), np.float32(10)))
    ref = radius_graph_pbc_single(pos, cell, up)
    assert ref[0].shape[1] == 2
    _check(*radius_graph_pbc(pos.cuda(), cell.view(1, 3, 3).cuda(), ptr, up), *ref)


def test_other_radii_match_reference_golden_fixture():
    """tests/golden/radius_graph_radii.npz: the reference's own output (not the restatement) at radius 3.7 and 6.0 on a
    hexagonal and a triclinic cell, uncapped and capped at 8, and on the two threshold pairs."""
    from cartnet_amd.graph import radius_graph_pbc
    z = np.load(gu.GOLDEN + "/radius_graph_radii.npz")
    t = lambda k: torch.from_numpy(z[k])
    for name in ("hexagonal", "triclinic"):
        pos, cell = t(f"{name}_pos").cuda(), t(f"{name}_cell").view(1, 3, 3).cuda()
        ptr = torch.tensor([0, pos.shape[0]]).cuda()
        for r in z["radii"].tolist():
            for tag, cap in (("", None), ("cap8_", 8)):
                key = f"{name}_r{r}_{tag}"
                _check(*radius_graph_pbc(pos, cell, ptr, r, max_neighbors=cap), t(key + "edge_index"), t(key + "dist"),
                       t(key + "dir"))
    for i in range(2):
        pos, cell = t(f"pair{i}_pos").cuda(), t(f"pair{i}_cell").view(1, 3, 3).cuda()
        ptr = torch.tensor([0, 2]).cuda()
        assert z[f"pair{i}_edge_index"].shape[1] == 0
        assert radius_graph_pbc(pos, cell, ptr, float(z[f"pair{i}_radius"]))[0].shape[1] == 0
        _check(*radius_graph_pbc(pos, cell, ptr, float(z[f"pair{i}_radius_up"])), t(f"pair{i}_up_edge_index"),
               t(f"pair{i}_up_dist"), t(f"pair{i}_up_dir"))

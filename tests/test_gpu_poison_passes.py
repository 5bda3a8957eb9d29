"""Passes under poison: every pass outside the training step that allocates with `torch.empty`, once per fill byte.

The Python layers hold some 150 `torch.empty` calls (metrics.py 58, shard.py 29, ops.py 21, symmetry.py 13, graph.py 8):
outputs the kernels must cover cell by cell, partial sums a finalize kernel folds, workspaces.  Each pass below is called
on the fixture its own test file builds (built before the poison is switched on), once with every such buffer filled with
0x00 and once with 0xFF (tests/poison_utils.py); every field of the two results is compared as bytes -- several results
hold NaN by contract (a crystal without rows, a molecule too small for a fit, a NaN input row), and the same NaN has the
same bytes.  A difference is an output cell nobody wrote, or a read of unwritten memory.  Each case asserts that fills
were counted.  No tolerance appears here.

The integer buffers of these passes were checked by reading the code first: the count kernels' `totals` and the status
words are cleared by a memset in the entry point that fills them (cartnet_shard_regraph_count, cartnet_shard_drop_h_count,
cartnet_symmetry_expand_count, cartnet_sort_by_key, cartnet_csr_build), offsets and index outputs are written entry by entry.
"""
import os
import sys

import pytest
import torch

import poison_utils as pu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
TOTALS = {"fills": 0, "bytes": 0}


@pytest.fixture(scope="module", autouse=True)
def _totals():
    """(after the last test of the file: what the helper counted, for the record)"""
    yield
    print(f"\npoison totals, passes: {TOTALS['fills']} fills, {TOTALS['bytes']} bytes")


def _both(run, what):
    (a, ra), (b, rb) = pu.under_both(run)
    print(f"poison [{what}]: {len(pu.flatten(a))} fields; fills {ra.count} / {rb.count}, bytes {ra.nbytes} / {rb.nbytes}")
    TOTALS["fills"] += ra.count + rb.count
    TOTALS["bytes"] += ra.nbytes + rb.nbytes
    for rec in (ra, rb):
        pu.assert_live(rec, [], f"{what}, fill 0x{rec.byte:02X}", workspace=False)
    assert ra.sizes == rb.sizes, f"{what}: the two runs allocated differently"
    pu.assert_same_bytes(a, b, what)
    return a


# ------------------------------------------------------------------------------------------------------------- metrics.py
def test_adp_metrics_and_adp_eval():
    from cartnet_amd import metrics as gm
    from cartnet_amd.shard import random_rotations
    from test_gpu_eval_batch import ROWS, _row_ptr, _spd_pair
    pred, true = _spd_pair(sum(ROWS))
    rp = _row_ptr(ROWS)
    rot = random_rotations(len(ROWS), torch.Generator(device=DEV).manual_seed(2), DEV)
    _both(lambda: {"metrics": gm.adp_metrics(pred, true, num_points=16),
                   "metrics7": gm.adp_metrics(pred, true, num_points=7),
                   "eval": gm.adp_eval(pred, true, rp, num_points=16),
                   "eval_part": gm.adp_eval(pred, true, rp, volume=False, iou=False, num_points=16),
                   "eval_rot": gm.adp_eval(pred, true, rp, rot=rot, volume=False, num_points=16),
                   "eval_empty": gm.adp_eval(pred[:0], true[:0], _row_ptr([0, 0]), num_points=16)},
          "adp_metrics, adp_eval and its crystal statistics")


@pytest.mark.parametrize("K", [1, 2, 7])
def test_frame_mean(K):
    from cartnet_amd import metrics as gm
    from cartnet_amd.shard import random_rotations
    from test_gpu_frame_mean import B, M, _ptr, _tensors
    pred = _tensors(K * M, 20 + K).cuda()
    rot = random_rotations(K * B, torch.Generator(device=DEV).manual_seed(5), DEV).view(K, B, 3, 3)
    _both(lambda: {"stats": gm.frame_mean(pred, rot, _ptr()), "bare": gm.frame_mean(pred, rot, _ptr(), stats=False)},
          f"frame_mean over {K} frames")


@pytest.mark.parametrize("rows", ["ragged", "tiled"])
def test_temp_series(rows):
    from cartnet_amd import metrics as gm
    from test_gpu_temp_series import ROWS, TEMPS, TILED, _members, _ptr
    rows = ROWS if rows == "ragged" else TILED

    def run():
        out = {}
        for T, temps in TEMPS.items():
            u_cif, u_eq = _members(T, sum(rows), 30 + T)
            out[T] = gm.temp_series(u_cif.cuda(), u_eq.cuda(), temps, _ptr(rows))
        return out
    _both(run, f"temp_series, rows {rows}")


def test_adp_export():
    from cartnet_amd import metrics as gm
    from test_gpu_adp_export import _cells, _ptr, _rows, _tensors
    rows = _rows()
    u, cells = _tensors(sum(rows), 3).cuda(), torch.from_numpy(_cells(len(rows), 1)).cuda()
    bad = u.clone()
    bad[4] = float("nan")                                     # a NaN row: reported in the status, NaN by contract
    _both(lambda: {"all": gm.adp_export(u, _ptr(rows), cells), "part": gm.adp_export(u, _ptr(rows), cells, axes=None, stats=None),
                   "nan_row": gm.adp_export(bad, _ptr(rows), cells, check=False),
                   "empty": gm.adp_export(u[:0], _ptr([0, 0, 0]), cells[:3])}, "adp_export")


@pytest.fixture(scope="module")
def analysis_cases():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import analysis_bytes
    finally:
        sys.path.pop(0)
    return analysis_bytes, analysis_bytes.cases()


@pytest.mark.parametrize("case", ["aniso", "dense_segment", "no_edges", "pairs", "ragged", "tls"])
def test_bond_graph_analyses(analysis_cases, case):
    """bond_test, riding_h, molecules, molecule_test, tls_fit and aniso_h (with and without the TLS results) on the batches of
    tools/analysis_bytes.py, and the bond table with and without the fit."""
    import molecule_utils as mu
    from cartnet_amd import metrics as gm
    ab, cases = analysis_cases
    batch, u, row_ptr = cases[case]
    u_eq = ((u[:, 0, 0] + u[:, 1, 1] + u[:, 2, 2]) / 3).contiguous()

    def run():
        rh = gm.riding_h(u_eq, batch)
        mo = gm.molecules(batch, row_ptr, mu.TOL, rows=int(u.shape[0]))
        tf = gm.tls_fit(u, batch, row_ptr, mo)
        index = gm.bond_index(batch, row_ptr, mu.TOL, rows=int(u.shape[0]))
        return {"bond_test": gm.bond_test(u, batch, row_ptr, mu.TOL, mu.THRESHOLD), "riding_h": rh, "molecules": mo,
                "molecule_test": gm.molecule_test(u, batch, row_ptr, mo, mu.THRESHOLD), "tls_fit": tf,
                "aniso_h": gm.aniso_h(u, batch, row_ptr, rh, mo, tf, ab.STRETCH, ab.BEND),
                "aniso_h_bare": gm.aniso_h(u, batch, row_ptr, rh, stretch=ab.STRETCH, bend=ab.BEND),
                "bond_index": index, "bond_table": gm.bond_table(u, batch, row_ptr, index, tf),
                "bond_table_bare": gm.bond_table(u, batch, row_ptr, index)}
    _both(run, f"bond-graph analyses, batch {case}")


def test_bond_table_on_its_own_fixture():
    """The crystals of tests/test_gpu_bond_table.py: a star, two images, atoms apart, hydrogens only, NaN and negative rows."""
    import molecule_utils as mu
    from cartnet_amd import metrics as gm
    from test_gpu_bond_table import _batch, _crystals
    batch, u, row_ptr = _batch(_crystals())

    def run():
        index = gm.bond_index(batch, row_ptr, mu.TOL, rows=int(u.shape[0]))
        tf = gm.tls_fit(u, batch, row_ptr, gm.molecules(batch, row_ptr, mu.TOL, rows=int(u.shape[0])))
        return {"index": index, "table": gm.bond_table(u, batch, row_ptr, index, tf),
                "bare": gm.bond_table(u, batch, row_ptr, index)}
    _both(run, "bond_index and bond_table")


# ------------------------------------------------------------------------------------------------------------ symmetry.py
def test_symmetry_expansion_targets_and_site_average():
    import cif_utils as cu
    from cartnet_amd import cif, symmetry
    crystals = cif.read_cif(cu.batch_text())
    arrays0, sym0 = symmetry.expand(crystals, DEV, labeled=True)              # (sizes, outside the poison)
    rows = int(arrays0["y_ptr"][-1])
    pred = (torch.randn(rows, 3, 3, generator=torch.Generator().manual_seed(11)) * 0.02).to(DEV)
    row_ptr = torch.from_numpy(arrays0["y_ptr"]).to(DEV)

    def run():
        arrays, sym = symmetry.expand(crystals, DEV, labeled=True)
        plain, _ = symmetry.expand(crystals, DEV, labeled=False)
        u, spread = symmetry.site_average(pred, row_ptr, list(range(len(crystals))), sym)
        some = symmetry.site_average(pred, row_ptr, list(range(len(crystals))), sym0)
        return {"arrays": arrays, "sym": sym, "unlabeled": plain, "u": u, "spread": spread, "again": some}
    _both(run, "symmetry.expand (labeled: targets; unlabeled) and site_average")


# ------------------------------------------------------------------------------------------------------- graph.py, shard.py
def _shard_fields(ds):
    return dict(ds.t, host_atom_ptr=ds.atom_ptr, host_edge_ptr=ds.edge_ptr, host_y_ptr=ds.y_ptr)


@pytest.mark.parametrize("radius,cap", [(5.0, None), (6.0, 12), (4.0, 25)])
def test_radius_graph(radius, cap):
    """graph.radius_graph_csr on the ten ragged crystals of tests/golden_utils.py as one pass, and the shard's rebuild on it
    (DeviceShard.with_radius_graph); cap 12 at radius 6 bites, so the d^2 pass runs."""
    import golden_utils as gu
    from cartnet_amd import shard
    from cartnet_amd.graph import radius_graph_csr
    base = shard.DeviceShard.from_data_list(gu.ragged())
    pos, cell, atom_ptr = base.t["pos"].contiguous(), base.t["cell"].contiguous(), torch.from_numpy(base.atom_ptr).to(DEV)
    if cap == 12:
        assert int(base.with_radius_graph(radius, cap).edge_ptr[-1]) < int(base.with_radius_graph(radius).edge_ptr[-1])
    _both(lambda: {"csr": radius_graph_csr(pos, cell, atom_ptr, radius, cap),
                   "shard": _shard_fields(base.with_radius_graph(radius, cap))}, f"radius graph, radius {radius}, cap {cap}")


@pytest.fixture(scope="module")
def resident():
    from cartnet_amd import shard
    from test_gpu_no_hydrogens import _edge_cases
    from test_gpu_shard import _items
    items = _items()
    return shard.DeviceShard.from_data_list(items), shard.DeviceShard.from_data_list(list(_edge_cases()))


def test_shard_collate(resident):
    from cartnet_amd.shard import random_rotations
    ds, _ = resident
    rot = random_rotations(3, torch.Generator(device=DEV).manual_seed(9), DEV)
    _both(lambda: {"plain": ds.collate([3, 1, 6]), "all": ds.collate(list(range(ds.num_graphs))),
                   "rotated": ds.collate([0, 4, 5], rot=rot, temp_mean=192.1785, temp_std=81.2135)}, "DeviceShard.collate")


def test_shard_without_hydrogens(resident):
    ds, edge = resident
    _both(lambda: {"items": _shard_fields(ds.without_hydrogens()), "edge_cases": _shard_fields(edge.without_hydrogens()),
                   "batch": edge.without_hydrogens().collate(list(range(edge.num_graphs)))}, "DeviceShard.without_hydrogens")


def test_shard_with_optimized_cell(resident):
    from cartnet_amd import shard
    from cartnet_amd.synthetic import make_crystal
    ds, _ = resident
    small = shard.DeviceShard.from_data_list([make_crystal(760 + g, n) for g, n in enumerate((9, 33, 2, 120))])
    _both(lambda: {"items": _shard_fields(ds.with_optimized_cell()), "small": _shard_fields(small.with_optimized_cell()),
                   "no_h": _shard_fields(ds.without_hydrogens().with_optimized_cell())}, "DeviceShard.with_optimized_cell")


# ----------------------------------------------------------------------------------------------------------------- ops.py
@pytest.fixture(scope="module")
def ops():
    from cartnet_amd import lib, ops as _ops
    lib.load()
    return _ops


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


@pytest.mark.parametrize("N,nkeys", [(1, 1), (63, 3), (65, 119), (1023, 7)])
def test_sort_by_key(ops, N, nkeys):
    g = torch.Generator().manual_seed(N + nkeys)
    z = torch.randint(0, nkeys, (N,), generator=g)
    bad = z.clone()
    if N > 10:
        z[::7] = z[0]
        bad[3], bad[N - 2] = -1, nkeys + 4
    z, bad = z.to(DEV), bad.to(DEV)

    def run():
        perm, ptr, status = ops.sort_by_key(z, nkeys)
        perm2, ptr2, status2 = ops.sort_by_key(bad, nkeys)
        return {"perm": perm[:N], "ptr": ptr, "status": status, "perm_bad": perm2[:N], "ptr_bad": ptr2, "status_bad": status2}
    out = _both(run, f"sort_by_key N={N} nkeys={nkeys}")
    assert torch.equal(out["perm"].cpu().long(), torch.argsort(z.cpu(), stable=True))


@pytest.mark.parametrize("total,nseg,W,ld", [(31, 3, 252, 256), (1000, 7, 516, 520), (97, 40, 24, 24)])
def test_segment_sums(ops, total, nseg, W, ld):
    """The three forms (long, chunked, chunked with the three-way fold): total is no multiple of the chunk of 32 rows, segments
    are empty or start inside a chunk, rows are strided; with and without a permutation."""
    from test_gpu_kernels import rnd
    g = torch.Generator().manual_seed(total + nseg)
    rows = rnd(total, ld, seed=total)[:, :W]
    dense = rows.contiguous()
    cuts = torch.sort(torch.randint(0, total + 1, (nseg - 1,), generator=g)).values
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([total])]).int().to(DEV)
    perm = torch.randperm(total, generator=g).int().to(DEV)
    assert total % 32 and W % 12 == 0

    def run():
        out = {k: _nan(nseg, W) for k in ("long", "long_perm", "chunked", "chunked_perm", "fold3_sums")}
        out["fold3"] = _nan(total, W // 3)
        ops.segment_sum_long(dense, ptr, None, total, out["long"])
        ops.segment_sum_long(dense, ptr, perm, total, out["long_perm"])
        ops.segment_sum_chunked(rows, ptr, None, total, out["chunked"])
        ops.segment_sum_chunked(rows, ptr, perm, total, out["chunked_perm"])
        ops.segment_sum_chunked_fold3(dense, ptr, total, out["fold3_sums"], out["fold3"])
        return out
    out = _both(run, f"segment sums, {total} rows in {nseg} segments of width {W}")
    assert torch.equal(out["long"], out["chunked"]) and torch.equal(out["chunked"], out["fold3_sums"])
    assert not bool(torch.isnan(out["long_perm"]).any())


@pytest.mark.parametrize("degs", ["long", "empty"])
def test_gate_gemm_eval(ops, degs):
    from test_gpu_kernels import _graph_with_degrees, rnd
    D = 256
    dl = [3, 300, 0, 0, 129, 1, 127, 128, 2, 500, 7] if degs == "long" else [0, 0, 5, 0, 0]
    ei, ptr = _graph_with_degrees(dl, seed=4)
    N, E = len(dl), ei.shape[1]
    ei, ptr = ei.to(DEV), ptr.to(DEV)
    g = torch.Generator().manual_seed(D + len(degs))
    pre, e_in = rnd(E, 2 * D, seed=1), rnd(E, D, seed=2)
    W2g, W2a = rnd(D, D, seed=3, scale=0.08), rnd(D, D, seed=4, scale=0.08)
    bg, ba = rnd(D, seed=5), rnd(D, seed=6)
    mr = torch.cat([rnd(D, seed=7, scale=0.3), (1.0 / torch.sqrt(0.5 + torch.rand(D, generator=g))).to(DEV)]).contiguous()
    gamma, beta = rnd(D, seed=8) * 0.3 + 1.0, rnd(D, seed=9) * 0.2
    env = torch.rand(E, generator=g).to(DEV)
    assert E % 128

    def run():
        lay = ops.GraphLayout(ei, N, ptr, need_csc=False)                    # (its int32 copies are `torch.empty` too)
        imgs = ops.pack_b([W2g.t(), W2a.t()])
        out = {}
        for name, v in (("env", env), ("plain", None)):
            out["e_out." + name], out["aggr." + name] = _nan(E, D), _nan(N, D)
            ops.gate_gemm_eval(pre, imgs[0], imgs[1], bg, ba, mr, gamma, beta, v, e_in, lay, out["e_out." + name],
                               out["aggr." + name])
        return out
    out = _both(run, f"gate_gemm_eval, degrees {degs}")
    assert not any(bool(torch.isnan(v).any()) for v in out.values())


def _ptr_of_degrees(S, maxdeg, seed):
    deg = torch.randint(0, maxdeg + 1, (S,), generator=torch.Generator().manual_seed(seed))
    return torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).int().to(DEV), int(deg.sum())


def test_column_sum_helpers(ops):
    """colsum, coldot_bc, softplus_bwd_sums, softplus_update_bwd_apply with sum_do, rowmul_bwd with its sums and
    att_gate_bwd_apply: fp64 partials in a `torch.empty`, folded by cartnet_colsum_finalize.  Rows / segments: 777, 999, 500
    and 700, the smallest parametrisations of tests/test_gpu_kernels.py whose last part is ragged (4097 rows for colsum,
    tests/test_gpu_comformer_kernels.py)."""
    from test_gpu_kernels import rnd
    Cc = 256
    x = rnd(4097, 260, seed=1)
    d, bc = rnd(777, Cc, seed=777), rnd(777, 2 * Cc, seed=778)
    sa, sb = rnd(777, Cc, seed=777), rnd(777, Cc, seed=778, scale=8.0)
    o, xx, dy = rnd(999, Cc, seed=1), rnd(999, Cc, seed=2), rnd(999, Cc, seed=3)
    mr = torch.cat([rnd(Cc, seed=4, scale=0.1), rnd(Cc, seed=5).abs() + 0.5])
    gam, bet, sums = rnd(Cc, seed=6), rnd(Cc, seed=7), rnd(2 * Cc, seed=8)
    ptr5, R5 = _ptr_of_degrees(500, 30, 500 + Cc)
    buf5, key5, q5 = rnd(R5, 2 * Cc, seed=1), rnd(R5, 2 * Cc, seed=2)[:, :Cc], rnd(500, 3 * Cc, seed=3)[:, :Cc]
    ptr7, R7 = _ptr_of_degrees(700, 30, 700 + Cc)
    gs7, key7, q7, da7 = rnd(R7, 2 * Cc, seed=1), rnd(R7, 2 * Cc, seed=2)[:, :Cc], rnd(700, 3 * Cc, seed=3)[:, :Cc], rnd(700, Cc, seed=4)

    def run():
        out = {"colsum": _nan(260)}
        ops.colsum(x, out["colsum"])
        out["coldot_a"], out["coldot_b"] = _nan(Cc), _nan(Cc)
        ops.coldot_bc(d, bc, out["coldot_a"], out["coldot_b"])
        out["softplus_out"], out["softplus_sum"] = _nan(777, Cc), _nan(Cc)
        ops.softplus_bwd_sums(sa, sb, out["softplus_out"], out["softplus_sum"])
        for training in (True, False):
            k = f"update.{training}."
            out[k + "d_o"], out[k + "dx"], out[k + "sum_do"] = _nan(999, Cc), _nan(999, Cc), _nan(Cc)
            ops.softplus_update_bwd_apply(o, xx, dy, mr, gam, bet, sums, training, out[k + "d_o"], None, out[k + "dx"],
                                          sum_do=out[k + "sum_do"])
        out["rowmul_dkey"], out["rowmul_dq"] = buf5.clone(), _nan(500, 3 * Cc)[:, :Cc]
        out["rowmul_sum_dkey"], out["rowmul_sum_dq"] = _nan(Cc), _nan(Cc)
        ops.rowmul_bwd(out["rowmul_dkey"][:, :Cc], key5, q5, ptr5, 0.0625, out["rowmul_dq"], sum_dkey=out["rowmul_sum_dkey"],
                       sum_dq=out["rowmul_sum_dq"])
        for name, key in (("stored_alpha", key7), ("recomputed_alpha", None)):
            k = f"att.{name}."
            out[k + "gs"], out[k + "dq"] = gs7.clone(), _nan(700, 3 * Cc)[:, :Cc]
            out[k + "sk"], out[k + "sm"], out[k + "sq"] = _nan(Cc), _nan(Cc), _nan(Cc)
            ops.att_gate_bwd_apply(out[k + "gs"], key, q7, da7, ptr7, mr, gam, bet, sums, R7, True, 1.0 / Cc ** 0.5,
                                   out[k + "dq"], out[k + "sk"], out[k + "sm"], out[k + "sq"])
        return out
    out = _both(run, "column-sum helpers")
    nan = [k for k, v in out.items() if bool(torch.isnan(v).any())]
    assert not nan, nan

"""BatchNorm groups under bf16 storage (model.bn_group_size with model.half_storage at gemm_precision 2): the reference's
ADP recipe -- batch 4 x accumulation 16, scripts/train_cartnet_adp.sh:4, train/train.py:183-189 -- as one pass with
pre / gs / dpre kept in HBM as bf16.  The per-group gate statistics then come from cartnet_colstats_grouped_h (the bf16
values as stored) and the three gate kernels run their *_h forms with a CartnetGroups descriptor.

Budgets are the ones the project gives bf16 everywhere (tests/test_gpu_model.py): predictions 3e-2 * max|ref|, gradients
8e-2 * max|g_all|; the running statistics get the prediction budget; HIP-against-HIP comparisons the same two; kernels
that only differ in how gs is loaded / stored get the fp32 kernels' own tolerances (tests/test_gpu_kernels.py)."""
import ctypes as C

import pytest
import torch

from conftest import rel_err
from test_gpu_groups import _oracle_micro_batches
from test_gpu_model import BF16_GRAD_TOL, BF16_PRED_TOL, _model

pytestmark = pytest.mark.gpu

KERNEL_TOL = 1e-5            # test_gpu_kernels.TOL: e_out, aggr, forward partial sums
APPLY_TOL = 2e-5             # test_gate_scatter_fwd_bwd: dg | ds
APPLY_SUM_TOL = 1e-4         # ... and their column sums


def dev():
    return torch.device("cuda:0")


# --------------------------------------------------------------------------------------------------- 1. kernels
def test_half_storage_gate_kernels_with_groups_equal_the_fp32_forms():
    """cartnet_gate_scatter_fwd_h / _bwd_stats_h / _bwd_apply_h with three groups -- atoms [0, 10), none, [10, 23); atom 4
    has no edge -- against the fp32 forms on the same bf16 values held as fp32.  Same arithmetic, only the loads and the
    apply pass's stores differ: every fp32 / fp64 output within the fp32 kernels' own test tolerances, dg | ds equal to
    the fp32 result rounded to bf16."""
    from cartnet_amd import lib
    l = lib.load()
    N, D, G, PARTS = 23, 256, 3, 2
    gen = torch.Generator().manual_seed(11)
    deg = torch.randint(1, 13, (N,), generator=gen)
    deg[4] = 0
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)]).int()
    E = int(rowptr[-1])
    node_gptr = torch.tensor([0, 10, 10, 23], dtype=torch.int32)
    edge_gptr = rowptr[node_gptr.long()].contiguous()
    rnd = lambda *s: torch.randn(*s, generator=gen)
    gs16 = rnd(E, 2 * D).bfloat16()
    e_in, de_out, daggr, env = rnd(E, D), rnd(E, D), rnd(N, D), torch.rand(E, generator=gen)
    mean_rstd = rnd(G, 2 * D) * 0.3
    mean_rstd[:, D:] = mean_rstd[:, D:].abs() + 0.5
    gamma, beta = rnd(D), rnd(D)
    d = lambda t: t.to(dev()).contiguous()
    rowptr_d, ng_d, eg_d = d(rowptr), d(node_gptr), d(edge_gptr)
    e_in, de_out, daggr, env, mean_rstd, gamma, beta = map(d, (e_in, de_out, daggr, env, mean_rstd, gamma, beta))
    grp = lib.Groups()
    grp.node_gptr, grp.edge_gptr, grp.G, grp.edge_parts, grp.node_parts = ng_d.data_ptr(), eg_d.data_ptr(), G, PARTS, PARTS
    gp = C.addressof(grp)
    st = lib.stream_ptr()
    parts = lambda: torch.full((G, PARTS, D), float("nan"), dtype=torch.float64, device=dev())

    def run(suffix, gs):
        out = {"e_out": torch.full((E, D), float("nan"), device=dev()), "aggr": torch.full((N, D), float("nan"), device=dev())}
        for k in ("ps", "pq", "pa", "pb", "pdg", "pds"):
            out[k] = parts()
        lib.check(getattr(l, "cartnet_gate_scatter_fwd" + suffix)(
            gs.data_ptr(), e_in.data_ptr(), env.data_ptr(), rowptr_d.data_ptr(), mean_rstd.data_ptr(), gamma.data_ptr(),
            beta.data_ptr(), N, D, out["e_out"].data_ptr(), out["aggr"].data_ptr(), out["ps"].data_ptr(),
            out["pq"].data_ptr(), gp, st), "fwd" + suffix)
        lib.check(getattr(l, "cartnet_gate_scatter_bwd_stats" + suffix)(
            gs.data_ptr(), de_out.data_ptr(), daggr.data_ptr(), env.data_ptr(), rowptr_d.data_ptr(), mean_rstd.data_ptr(),
            gamma.data_ptr(), beta.data_ptr(), N, D, out["pa"].data_ptr(), out["pb"].data_ptr(), gp, st), "stats" + suffix)
        torch.cuda.synchronize()
        return out

    gs_f, gs_h = d(gs16.float()), d(gs16)
    f, h = run("", gs_f), run("_h", gs_h)
    # the apply pass of both forms gets the SAME per-group sums (the fp32 form's statistics)
    sums = torch.cat([f["pa"].sum(1), f["pb"].sum(1)], dim=1).float().contiguous()
    for suffix, gs, out in (("", gs_f, f), ("_h", gs_h, h)):
        lib.check(getattr(l, "cartnet_gate_scatter_bwd_apply" + suffix)(
            gs.data_ptr(), de_out.data_ptr(), daggr.data_ptr(), env.data_ptr(), rowptr_d.data_ptr(), mean_rstd.data_ptr(),
            gamma.data_ptr(), beta.data_ptr(), sums.data_ptr(), E, 1, N, D, out["pdg"].data_ptr(), out["pds"].data_ptr(),
            gp, st), "apply" + suffix)
    torch.cuda.synchronize()
    assert gs_h.dtype == torch.bfloat16 and torch.isfinite(gs_h.float()).all() and gs_f.abs().max().item() > 0
    for k, tol in (("e_out", KERNEL_TOL), ("aggr", KERNEL_TOL), ("ps", KERNEL_TOL), ("pq", KERNEL_TOL), ("pa", KERNEL_TOL),
                   ("pb", KERNEL_TOL), ("pdg", APPLY_SUM_TOL), ("pds", APPLY_SUM_TOL)):
        assert torch.isfinite(f[k]).all() and torch.isfinite(h[k]).all(), k
        err = rel_err(h[k], f[k])
        print(f"{k}: {err:.3g} (bound {tol:g})")
        assert err < tol, (k, err)
    err = rel_err(gs_h.float(), gs_f.bfloat16().float())
    print(f"dg | ds as bf16: {err:.3g} (bound {APPLY_TOL:g})")
    assert err < APPLY_TOL
    # the atom without edges aggregates nothing; the empty group's partial rows are zeros
    assert not h["aggr"][4].any()
    for k in ("ps", "pq", "pa", "pb", "pdg", "pds"):
        assert not h[k][1].any(), k


# --------------------------------------------------------------------------------------------------- 2. oracle
CASES = {"d256_groups_of_4": (2, 4, (20, 31, 12, 25, 18, 40, 9, 22), True),
         "d256_ragged_last_group": (3, 2, (6, 11, 8, 14, 10), True),
         "scalar_head": (2, 3, (4, 9, 6, 12, 5, 7), False)}


def _case(name):
    from cartnet_amd.model import make_state_dict
    from cartnet_amd.synthetic import make_crystal
    L, gsz, sizes, chol = CASES[name]
    hp = dict(dim_in=256, dim_rbf=16, num_layers=L, radius=5.0, invariant=False, temperature=chol, use_envelope=True,
              atom_types=True, cholesky=chol)
    items = [make_crystal(9000 + i, n, adp=chol) for i, n in enumerate(sizes)]
    sd = make_state_dict(256, 16, L, seed=31, cholesky=chol, temperature=chol)
    return hp, items, sd, gsz


def _grouped_half_model(hp, sd, gsz, half=True):
    m = _model(hp, sd, 2).train()
    m.half_storage = half
    m.bn_group_size = gsz
    return m


def _grouped_step(m, items, gsz):
    from cartnet_amd.data import Batch
    from cartnet_amd.train import grouped_loss
    b = Batch.from_data_list(items).to("cuda:0")
    pred, true = m(b)
    mae, _, G = grouped_loss(pred, true, b, gsz)
    mae.backward()
    return pred.detach().clone(), G


@pytest.mark.parametrize("case", list(CASES))
def test_grouped_half_storage_pass_against_the_oracle_micro_batch_by_micro_batch(case):
    """Measured on an MI355X (prediction error, gradient error, worst running-statistic error):
    see DESIGN.md 4c, "BatchNorm groups under bf16 storage"."""
    hp, items, sd, gsz = _case(case)
    m = _grouped_half_model(hp, sd, gsz)
    pred, G = _grouped_step(m, items, gsz)
    assert G == -(-len(items) // gsz) and G > 1
    ref_pred, gref, ref_state = _oracle_micro_batches(sd, items, gsz, hp)
    names = list(gref)
    got = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}
    assert set(names) == set(got)
    gmax = max(v.abs().max().item() for v in gref.values())
    gerr = max((got[k].reshape(gref[k].shape) - gref[k]).abs().max().item() for k in names) / gmax
    perr = rel_err(pred, ref_pred)
    state = m.state_dict()
    serr = max(rel_err(state[k], v) for k, v in ref_state.items() if v.is_floating_point())
    print(f"{case}: pred {perr:.3g} (bound {BF16_PRED_TOL:g})  grad {gerr:.3g} (bound {BF16_GRAD_TOL:g})  "
          f"running statistics {serr:.3g} (bound {BF16_PRED_TOL:g})")
    assert all(torch.isfinite(v).all() for v in got.values())
    assert perr < BF16_PRED_TOL and gerr < BF16_GRAD_TOL, (perr, gerr)
    assert perr > 1e-6, "the bf16 kernels must actually run"
    for k, v in ref_state.items():
        if v.is_floating_point():
            assert rel_err(state[k], v) < BF16_PRED_TOL, k
        else:
            assert int(state[k]) == int(sd[k]) + G, k           # num_batches_tracked advanced once per micro-batch


# --------------------------------------------------------------------------------------------------- 3. HIP vs HIP
def test_grouped_pass_equals_separate_half_storage_passes():
    """One grouped pass over 8 crystals against two passes over 4, both through the HIP path, at precision 2 with bf16
    storage and -- the pair that exists without this feature -- with fp32 storage.  Under bf16 storage the grouped pass
    takes the gate statistics after rounding to bf16, the separate passes before (GEMM epilogue): the two differences
    are printed for DESIGN.md 4c."""
    from cartnet_amd.data import Batch
    from cartnet_amd.model import make_state_dict
    from cartnet_amd.synthetic import make_crystal
    hp = dict(dim_in=256, dim_rbf=64, num_layers=4, radius=5.0, invariant=False, temperature=True, use_envelope=True,
              atom_types=True, cholesky=True)
    items = [make_crystal(9100 + i, n) for i, n in enumerate((64, 90, 75, 120, 66, 81, 70, 101))]
    sd = make_state_dict(256, 64, 4, seed=32)
    for half in (False, True):
        ma = _grouped_half_model(hp, sd, 4, half)
        mb = _grouped_half_model(hp, sd, 0, half)
        pa, G = _grouped_step(ma, items, 4)
        assert G == 2
        preds = []
        for s in (0, 4):
            bb = Batch.from_data_list(items[s:s + 4]).to("cuda:0")
            p, t = mb(bb)
            (p - t).abs().mean().backward()                       # autograd accumulates into .grad
            preds.append(p.detach())
        ga = torch.cat([p.grad.flatten() for p in ma.parameters()])
        gb = torch.cat([p.grad.flatten() for p in mb.parameters()])
        perr, gerr = rel_err(pa, torch.cat(preds)), rel_err(ga, gb)
        print(f"{'bf16' if half else 'fp32'} storage: grouped vs separate passes  pred {perr:.3g}  grad {gerr:.3g}")
        assert torch.isfinite(ga).all() and ga.abs().max().item() > 0
        assert perr < BF16_PRED_TOL and gerr < BF16_GRAD_TOL, (half, perr, gerr)
        for (k, va), vb in zip(ma.state_dict().items(), mb.state_dict().values()):
            if "num_batches" in k:
                assert int(va) == int(vb) == int(sd[k]) + 2


# --------------------------------------------------------------------------------------------------- 4. repeatability, eval
def test_grouped_half_storage_is_bitwise_repeatable_and_eval_ignores_groups():
    from cartnet_amd.data import Batch
    hp, items, sd, gsz = _case("d256_groups_of_4")
    runs = []
    for _ in range(2):
        m = _grouped_half_model(hp, sd, gsz)
        pred, _ = _grouped_step(m, items, gsz)
        runs.append((pred, [p.grad.detach().clone() for p in m.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert all(torch.isfinite(g).all() for g in runs[0][1]) and any(g.abs().max().item() > 0 for g in runs[0][1])
    m.eval()
    outs = []
    with torch.no_grad():
        for g in (4, 0):
            m.bn_group_size = g
            outs.append(m(Batch.from_data_list(items).to("cuda:0"))[0].clone())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


# --------------------------------------------------------------------------------------------------- 5. workspace
def test_grouped_workspace_shrinks_by_the_bf16_tensors():
    """pre, gs of every layer, the two dpre buffers and the encoder's pre-activation -- (2L + 2) tensors [E, 2D] -- at
    two bytes per element less, with groups as without (the bound of test_bf16_storage_on_jarvis_shapes_and_adp_fixture)."""
    from cartnet_amd import lib
    from cartnet_amd.data import Batch
    hp, items, sd, gsz = _case("d256_groups_of_4")
    b = Batch.from_data_list(items)
    N, E, Bg, L, D = int(b.x.shape[0]), int(b.edge_index.shape[1]), int(b.num_graphs), hp["num_layers"], 256
    m = _grouped_half_model(hp, sd, gsz, False)
    sizes = []
    for half in (False, True):
        m.half_storage = half
        md = m._model_desc(dict(m.named_parameters()))
        assert md.bn_group_size == gsz and md.half_storage == int(half)
        sizes.append(int(lib.load().cartnet_workspace_bytes(C.byref(md), N, E, Bg, 0, 1)))
    assert sizes[0] - sizes[1] >= (2 * L + 2) * E * 2 * D * 2 - 65536, (sizes, E)


# --------------------------------------------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("precision,dim_in", [(0, 256), (1, 256), (2, 64)])
def test_half_storage_is_still_refused_without_its_kernels(precision, dim_in):
    from cartnet_amd.data import Batch
    from cartnet_amd.model import make_state_dict
    from cartnet_amd.synthetic import make_crystal
    hp = dict(dim_in=dim_in, dim_rbf=16, num_layers=2, radius=5.0, invariant=False, temperature=True, use_envelope=True,
              atom_types=True, cholesky=True)
    m = _model(hp, make_state_dict(dim_in, 16, 2, seed=31), precision).train()
    m.half_storage, m.bn_group_size = True, 2
    b = Batch.from_data_list([make_crystal(9000 + i, n) for i, n in enumerate((5, 7, 6, 4))]).to("cuda:0")
    with pytest.raises(ValueError, match="half_storage"):
        m(b)


def test_sync_batchnorm_with_groups_is_still_refused():
    from cartnet_amd.data import Batch
    hp, items, sd, gsz = _case("scalar_head")
    m = _grouped_half_model(hp, sd, gsz)
    m.sync_batchnorm = True
    with pytest.raises(ValueError, match="sync_batchnorm"):
        m(Batch.from_data_list(items).to("cuda:0"))


# --------------------------------------------------------------------------------------------------- 7. train_epoch
def test_train_epoch_with_groups_and_half_storage_follows_the_micro_batch_recipe():
    """train_epoch(batch 8, accumulation 1, groups of 2) against train_epoch(batch 2, accumulation 4), both at precision 2
    with bf16 storage, on the same crystals in the same order: the same number of optimiser steps, the epoch's MAE within
    the 5e-2 that test_main_jarvis_style_run_with_bf16_storage gives bf16 storage, finite parameters."""
    from cartnet_amd.data import DataLoader
    from cartnet_amd.model import make_state_dict
    from cartnet_amd.optim import FlatAdam
    from cartnet_amd.synthetic import make_crystal
    from cartnet_amd.train import train_epoch
    hp = dict(dim_in=256, dim_rbf=16, num_layers=2, radius=5.0, invariant=False, temperature=True, use_envelope=True,
              atom_types=True, cholesky=True)
    items = [make_crystal(9200 + i, 10 + (3 * i) % 17) for i in range(16)]
    sd = make_state_dict(256, 16, 2, seed=33)
    ma, mb = _grouped_half_model(hp, sd, 2), _grouped_half_model(hp, sd, 0)
    ma.validate_graph = mb.validate_graph = False
    oa, ob = FlatAdam(ma, lr=1e-3), FlatAdam(mb, lr=1e-3)
    ra = train_epoch(DataLoader(items, 8), ma, oa, 1)
    rb = train_epoch(DataLoader(items, 2), mb, ob, 4)
    print(f"train_epoch mae: grouped {ra['mae']:.6g}  micro-batches {rb['mae']:.6g}")
    assert ra["graphs"] == rb["graphs"] == 16
    assert oa.step_count == ob.step_count == 2
    assert ra["mae"] == ra["mae"] and abs(ra["mae"] - rb["mae"]) < 5e-2 * abs(rb["mae"])
    assert torch.isfinite(oa.flat_param).all() and torch.isfinite(ob.flat_param).all()

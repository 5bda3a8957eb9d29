"""BatchNorm groups in iComformer (CartnetIcfModel.bn_group_size; model.bn_group_size): the reference recipe's
micro-batches (--batch 4 --batch_accumulation 16, scripts/train_icomformer_adp.sh:3) carried through the network as ONE
batch.  The ten BatchNorm1d (bn_att / bn of the four ComformerConv and of ComformerConv_edge) are the only coupling
between the crystals of a batch, so the grouped pass must equal, within the usual parity budget, one forward / backward
per micro-batch with the statistics over that micro-batch only, running statistics updated after every micro-batch and
the gradients of the per-micro-batch mean losses accumulated unscaled -- replayed here by the fp64 oracle."""
import pytest
import torch

import icomformer_utils as iu
from conftest import rel_err
from test_gpu_model import PRED_TOL, _check_grads

pytestmark = pytest.mark.gpu


def _icf(C, sd, precision=0):
    from cartnet_amd.comformer import iComformer
    m = iComformer(C)
    m.load_state_dict(sd, strict=True)
    m.validate_graph = True
    m.gemm_precision = precision
    return m.to("cuda:0")


def _gpu_batch(items):
    from cartnet_amd.data import Batch
    return Batch.from_data_list(items).to("cuda:0")


def _oracle_micro_batches(sd, items, group_size, names):
    """Sequential micro-batches through the oracle, buffers carried from one to the next: returns (pred rows in batch
    order, grads of the summed losses, final BatchNorm buffers)."""
    from cartnet_amd.data import Batch
    from oracle import icomformer_ref as orc
    sd64 = {k: (v.double().requires_grad_(k in names) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    preds, total = [], 0.0
    for s in range(0, len(items), group_size):
        mb = iu.batch64(Batch.from_data_list(items[s:s + group_size]))
        new_stats = {}
        pred = orc.icomformer_forward(sd64, mb, training=True, new_stats=new_stats)
        total = total + (pred - mb.y).abs().mean()
        preds.append(pred.detach())
        for k, v in new_stats.items():                      # the next micro-batch starts from the updated buffers
            sd64[k] = v.detach()
    total.backward()
    return torch.cat(preds), {k: sd64[k].grad for k in names}, {k: v for k, v in sd64.items() if "running" in k or
                                                                "num_batches" in k}


CASES = {"c32_groups_of_2": (32, 2, (7, 12, 5, 9, 16, 3)),
         "c64_ragged_last_group": (64, 2, (6, 11, 8, 14, 10)),
         # weight images on, alpha-free kernels, group boundaries inside 128-row GEMM tiles, groups of ~1.2k edges / 3.6k
         # rows that span several workgroups
         "c256_groups_of_4": (256, 4, (20, 31, 12, 25, 18, 40, 9, 22)),
         # C > 256: the multi-chunk kernels and the stored-alpha path (cartnet_gate_scatter_* with groups)
         "c264_groups_of_3": (264, 3, (4, 9, 6, 12, 5, 7))}


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_grouped_pass_equals_sequential_micro_batches_of_the_oracle(case, precision):
    from cartnet_amd.comformer import make_icomformer_state_dict
    from cartnet_amd.synthetic import make_crystal
    from cartnet_amd.train import grouped_loss
    C, gsz, sizes = CASES[case]
    items = [make_crystal(9300 + i, n) for i, n in enumerate(sizes)]
    sd = make_icomformer_state_dict(C, seed=41)
    m = _icf(C, sd, precision).train()
    m.bn_group_size = gsz
    b = _gpu_batch(items)
    pred, true = m(b)
    mae, _, G = grouped_loss(pred, true, b, gsz)
    assert G == -(-len(items) // gsz)
    mae.backward()
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert len(got) >= 40
    ref_pred, ref_grads, ref_state = _oracle_micro_batches(sd, items, gsz, list(got))
    print(f"{case} precision {precision}: pred {rel_err(pred, ref_pred):.3g}")
    assert rel_err(pred, ref_pred) < PRED_TOL
    _check_grads(got, ref_grads, case)
    new = m.state_dict()
    for k, v in ref_state.items():
        if v.is_floating_point():
            assert rel_err(new[k], v) < 1e-5, k
        else:
            assert int(new[k]) == int(sd[k]) + G, k           # num_batches_tracked advanced once per micro-batch


def test_grouped_pass_equals_separate_hip_passes_eval_ignores_groups_and_runs_repeat():
    """The same micro-batches as separate forward / backward calls of the HIP path (autograd accumulates): predictions,
    gradients and BatchNorm buffers inside the project's parity budget (both sides are held to it against fp64
    independently; they differ in summation order -- the statistics' partial rows, the bias gradients over G x parts rows
    and lin_concate's statistics from a pass instead of the GEMM epilogue).  In eval mode BatchNorm uses the running
    statistics, so groups change nothing at all; two grouped training passes give identical bytes (no atomics).
    Measured on an MI355X: predictions and running statistics identical (distance 0), gradients 8.7e-8 of max|g|."""
    from cartnet_amd.comformer import make_icomformer_state_dict
    from cartnet_amd.synthetic import make_crystal
    from cartnet_amd.train import grouped_loss
    items = [make_crystal(9100 + i, n) for i, n in enumerate((64, 90, 75, 120, 66, 81, 70, 101))]
    sd = make_icomformer_state_dict(256, seed=42)
    ma, mb = _icf(256, sd).train(), _icf(256, sd).train()
    ma.bn_group_size = 4
    runs = []
    for _ in range(2):
        ma.load_state_dict(sd)
        ma.zero_grad(set_to_none=True)
        b = _gpu_batch(items)
        pa, ta = ma(b)
        la, _, _ = grouped_loss(pa, ta, b, 4)
        la.backward()
        runs.append((pa.detach().clone(), {k: p.grad.detach().clone() for k, p in ma.named_parameters() if p.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k, g in runs[0][1].items():
        assert torch.equal(g, runs[1][1][k]), k
    preds = []
    for s in (0, 4):
        p, t = mb(_gpu_batch(items[s:s + 4]))
        (p - t).abs().mean().backward()                       # autograd accumulates into .grad
        preds.append(p.detach())
    ga = runs[0][1]
    gb = {k: p.grad for k, p in mb.named_parameters() if p.grad is not None}
    gmax = max(float(g.abs().max()) for g in gb.values())
    worst_g = max(float((ga[k] - gb[k]).abs().max()) for k in gb) / gmax
    worst_s = max(rel_err(va, vb) for (k, va), vb in zip(ma.state_dict().items(), mb.state_dict().values()) if "running" in k)
    print(f"grouped vs separate: pred {rel_err(pa, torch.cat(preds)):.3g} grads {worst_g:.3g} of max|g| buffers {worst_s:.3g}")
    assert rel_err(pa, torch.cat(preds)) < PRED_TOL
    assert ga.keys() == gb.keys()
    _check_grads(ga, gb, "grouped vs separate")
    for (k, va), vb in zip(ma.state_dict().items(), mb.state_dict().values()):
        if "running" in k:
            assert rel_err(va, vb) < 1e-5, k
        elif "num_batches" in k:
            assert int(va) == int(vb) == int(sd[k]) + 2
    ma.eval(); mb.eval()
    mb.load_state_dict(ma.state_dict())
    with torch.no_grad():
        ea, _ = ma(_gpu_batch(items))
        eb, _ = mb(_gpu_batch(items))
    assert torch.equal(ea, eb)


def test_groups_of_one_crystal_equal_single_crystal_passes():
    """bn_group_size = 1: every crystal is its own group, so its prediction is that of a training-mode pass over that
    crystal alone."""
    from cartnet_amd.comformer import make_icomformer_state_dict
    from cartnet_amd.synthetic import make_crystal
    items = [make_crystal(9400 + i, n) for i, n in enumerate((5, 11, 3, 8, 14))]
    sd = make_icomformer_state_dict(32, seed=43)
    ma, mb = _icf(32, sd).train(), _icf(32, sd).train()
    ma.bn_group_size = 1
    with torch.no_grad():
        pa, _ = ma(_gpu_batch(items))
        per = torch.split(pa, [int(it.non_H_mask.sum()) for it in items])
        for i, it in enumerate(items):
            pb, _ = mb(_gpu_batch([it]))
            assert rel_err(per[i], pb) < PRED_TOL, i
    for k, v in ma.state_dict().items():
        if "num_batches" in k:
            assert int(v) == int(sd[k]) + len(items), k


def test_groups_need_the_native_sequence():
    from cartnet_amd.comformer import make_icomformer_state_dict
    from cartnet_amd.synthetic import make_crystal
    m = _icf(32, make_icomformer_state_dict(32, seed=44)).train()
    m.bn_group_size = 2
    m.native_sequence = False
    with pytest.raises(ValueError, match="native_sequence"):
        m(_gpu_batch([make_crystal(9500 + i, 6 + i) for i in range(4)]))


def test_train_epoch_with_groups_matches_the_micro_batch_recipe():
    """train_epoch(batch 8, accumulation 1, bn_group_size 2) == train_epoch(batch 2, accumulation 4) on the same
    crystals in the same order: Adam is fed the same summed gradient."""
    from cartnet_amd.comformer import make_icomformer_state_dict
    from cartnet_amd.data import DataLoader
    from cartnet_amd.optim import FlatAdam
    from cartnet_amd.synthetic import make_crystal
    from cartnet_amd.train import train_epoch
    items = [make_crystal(9200 + i, 10 + (3 * i) % 17) for i in range(16)]
    sd = make_icomformer_state_dict(64, seed=45)
    ma, mb = _icf(64, sd).train(), _icf(64, sd).train()
    ma.validate_graph = mb.validate_graph = False
    ma.bn_group_size = 2
    oa, ob = FlatAdam(ma, lr=1e-3), FlatAdam(mb, lr=1e-3)
    ra = train_epoch(DataLoader(items, 8), ma, oa, 1)
    rb = train_epoch(DataLoader(items, 2), mb, ob, 4)
    assert ra["graphs"] == rb["graphs"] == 16 and abs(ra["mae"] - rb["mae"]) < 1e-5 * abs(rb["mae"])
    assert oa.step_count == ob.step_count == 2
    assert rel_err(oa.exp_avg, ob.exp_avg) < 1e-4 and rel_err(oa.exp_avg_sq, ob.exp_avg_sq) < 1e-4

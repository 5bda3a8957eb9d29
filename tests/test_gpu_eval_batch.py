"""Evaluation at any batch size with the results of batch size 1 (--eval_batch): the two kernels of csrc/eval_ops.hip
against the existing metrics kernel, the collation kernel and fp64; eval_epoch(per_crystal=True), montecarlo_batch and
main.py's batched --inference / --montecarlo against their batch-size-1 forms; cartnet_amd.evaluate's two passes at batch
size 1 against the reference's loops (main.py:21-119), written out here statement by statement."""
import os
import pickle

import pytest
import torch

import golden_utils as gu
from conftest import rel_err
from test_gpu_model import PRED_TOL, _model

pytestmark = pytest.mark.gpu

ROWS = [1, 0, 65, 3, 300, 64]                       # six crystals, M = 433: an empty one, one row, more than one wave
ROT_TOL = 4e-6   # R^T p R in fp32: nine products of three factors, |R| <= 1, six roundings each: 6 * 2^-24 * 9 = 3.2e-6 (x max|p|)
ICF_EVAL_TOL = 2e-6                                 # tests/test_gpu_icomformer.py: a crystal's eval prediction across batches


def _spd_pair(M, seed=3):
    """SPD matrices drawn as in tests/test_gpu_metrics.py::test_identities_at_a_full_test_batch."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, 3, 3, generator=g)
    true = a @ a.transpose(1, 2) * 0.01 + 0.005 * torch.eye(3)
    b = torch.randn(M, 3, 3, generator=g) * 0.03
    return (true + b @ b.transpose(1, 2)).cuda(), true.cuda()


def _row_ptr(rows):
    return torch.tensor([0] + rows, dtype=torch.int64).cumsum(0).cuda()


def _segment_sums64(res_abs, vol, sim, iou, rows):
    """[B,4] fp64 torch sums of the per-atom results, per crystal."""
    cols = [res_abs.double().reshape(-1, 9).sum(1)] + [t.double() if t is not None else torch.zeros(sum(rows)).double().cuda()
                                                      for t in (vol, sim, iou)]
    per_atom = torch.stack(cols, 1).cpu()
    return torch.stack([p.sum(0) for p in torch.split(per_atom, rows)])


@pytest.mark.parametrize("P", [64, 7])
def test_kernel_without_rotation(P):
    from cartnet_amd import metrics as gm
    pred, true = _spd_pair(sum(ROWS))
    rp = _row_ptr(ROWS)
    res = gm.adp_eval(pred, true, rp, num_points=P)
    vol, sim, iou = gm.adp_metrics(pred, true, num_points=P)
    assert torch.equal(res.volume_error, vol) and torch.equal(res.similarity_index, sim) and torch.equal(res.iou, iou)
    assert torch.equal(res.abs_err, (pred - true).abs())
    assert res.true.data_ptr() == true.data_ptr() and res.rows.tolist() == ROWS
    ref = _segment_sums64(res.abs_err, vol, sim, iou, ROWS)
    got = res.crystal_sums.cpu()
    assert got.dtype == torch.float64 and tuple(got.shape) == (6, 4)
    assert torch.allclose(got, ref, rtol=1e-12, atol=0.0)                     # only the summation order differs
    assert torch.equal(got[1], torch.zeros(4, dtype=torch.float64))            # the crystal without rows: exactly 0
    again = gm.adp_eval(pred, true, rp, num_points=P)
    for a, b in zip(res, again):
        if a is not None:
            assert torch.equal(a, b)                                           # no atomics, fixed order
    assert res.crystal_sums.cpu().numpy().tobytes() == again.crystal_sums.cpu().numpy().tobytes()
    # a metric that is not requested: no tensor, column 0
    part = gm.adp_eval(pred, true, rp, volume=False, iou=False, num_points=P)
    assert part.volume_error is None and part.iou is None and torch.equal(part.similarity_index, sim)
    ps = part.crystal_sums.cpu()
    assert torch.equal(ps[:, 1], torch.zeros(6).double()) and torch.equal(ps[:, 3], torch.zeros(6).double())
    assert torch.equal(ps[:, 0], got[:, 0]) and torch.equal(ps[:, 2], got[:, 2])
    none = gm.adp_eval(pred, true, rp, volume=False, similarity=False, iou=False)
    assert torch.equal(none.crystal_sums.cpu()[:, 0], got[:, 0]) and torch.equal(none.abs_err, res.abs_err)
    # B = 1 is the batch-size-1 case: the same per-atom values, the six crystals' totals
    one = gm.adp_eval(pred, true, _row_ptr([sum(ROWS)]), num_points=P)
    assert torch.equal(one.iou, iou) and torch.equal(one.abs_err, res.abs_err)
    assert torch.allclose(one.crystal_sums.cpu()[0], got.sum(0), rtol=1e-12, atol=0.0)
    # no rows at all
    empty = gm.adp_eval(pred[:0], true[:0], _row_ptr([0, 0]), num_points=P)
    assert torch.equal(empty.crystal_sums.cpu(), torch.zeros(2, 4).double()) and empty.iou.numel() == 0


def test_kernel_with_rotation():
    from cartnet_amd import lib as _l
    from cartnet_amd import metrics as gm
    from cartnet_amd.shard import random_rotations
    M = sum(ROWS)
    pred, first = _spd_pair(M, seed=5)
    rp = _row_ptr(ROWS)
    R = random_rotations(6, torch.Generator(device="cuda").manual_seed(1), "cuda")
    res = gm.adp_eval(pred, first, rp, rot=R, volume=False, num_points=16)
    Ra = torch.repeat_interleave(R.double().cpu(), torch.tensor(ROWS), dim=0)
    ref = Ra.transpose(1, 2) @ first.double().cpu() @ Ra
    bound = ROT_TOL * first.abs().max().item()
    err = (res.true.double().cpu() - ref).abs().max().item()
    print(f"pseudo-truth: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert res.true.data_ptr() != first.data_ptr()
    # every metric is evaluated from the fp32 pseudo-truth as written
    vol, sim, iou = gm.adp_metrics(pred, res.true, False, True, True, num_points=16)
    assert torch.equal(res.similarity_index, sim) and torch.equal(res.iou, iou) and res.volume_error is None
    assert torch.equal(res.abs_err, (pred - res.true).abs())
    assert torch.allclose(res.crystal_sums.cpu(), _segment_sums64(res.abs_err, None, sim, iou, ROWS), rtol=1e-12, atol=0.0)
    # identity rotations return truth bit for bit
    eye = torch.eye(3, device="cuda").repeat(6, 1, 1)
    ident = gm.adp_eval(pred, first, rp, rot=eye, volume=False, num_points=16)
    assert torch.equal(ident.true, first)
    plain = gm.adp_eval(pred, first, rp, volume=False, num_points=16)
    assert torch.equal(ident.iou, plain.iou) and torch.equal(ident.crystal_sums, plain.crystal_sums)
    # with rot the pseudo-truth needs somewhere to go: refused on the host, before any launch
    sums = torch.empty(6, 4, dtype=torch.float64, device="cuda")
    rc = _l.load().cartnet_adp_eval(pred.data_ptr(), first.data_ptr(), rp.data_ptr(), 6, M, R.data_ptr(), None, 64, None,
                                    None, None, None, None, sums.data_ptr(), _l.stream_ptr())
    assert rc != 0
    with pytest.raises(_l.CartnetHipError, match="true_out"):
        _l.check(rc, "cartnet_adp_eval")
    with pytest.raises(ValueError):
        gm.adp_eval(pred, first, rp, rot=R[:5])


def test_rotate_rows():
    from cartnet_amd import metrics as gm
    from cartnet_amd.shard import DeviceShard, random_rotations
    from cartnet_amd.synthetic import make_crystal
    gen = torch.Generator(device="cuda").manual_seed(2)
    shard = DeviceShard.from_data_list([make_crystal(300 + i, n) for i, n in enumerate([3, 40, 17, 8, 29])], "cuda:0")
    sel = [3, 0, 4, 1, 2]
    rot = random_rotations(5, gen, "cuda")
    plain, turned = shard.collate(sel), shard.collate(sel, rot)
    ep = gm.edge_row_ptr(plain)
    assert torch.equal(ep, plain._meta[2 * 5 + 1:3 * 5 + 2])                   # the edge offsets the collation was given
    assert torch.equal(gm.target_row_ptr(plain), plain._meta[3 * 5 + 2:])
    out = gm.rotate_rows(plain.cart_dir, ep, rot)
    assert out.data_ptr() != plain.cart_dir.data_ptr()
    assert torch.equal(out, turned.cart_dir)                                    # cartnet_collate's arithmetic, bit for bit
    # hand-made offsets: an empty first, middle and last segment, three tiles, a ragged last thread
    n, rp = 2051, torch.tensor([0, 0, 700, 700, 700, 2051, 2051], dtype=torch.int64).cuda()
    v = torch.randn(n, 3, generator=torch.Generator().manual_seed(4)).cuda() * 3.0
    R = random_rotations(6, gen, "cuda")
    got = gm.rotate_rows(v, rp, R)
    seg = torch.repeat_interleave(torch.arange(6), (rp[1:] - rp[:-1]).cpu())
    ref = (v.double().cpu().unsqueeze(1) @ R.double().cpu()[seg]).squeeze(1)
    assert (got.double().cpu() - ref).abs().max().item() <= 1e-6 * v.abs().max().item()
    alias = v.clone()
    assert gm.rotate_rows(alias, rp, R, out=alias).data_ptr() == alias.data_ptr()
    assert torch.equal(alias, got)                                              # rotation in place
    assert gm.rotate_rows(v[:0], _row_ptr([0, 0]), R[:2]).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ the model paths

SIZES = [1, 2, 23, 40, 11, 64, 17]                   # seven crystals: batches of 4 and 3


class _Recorder:
    """The model, keeping what it returned for every batch."""

    def __init__(self, m):
        self.m, self.out = m, []

    def eval(self):
        self.m.eval()

    def flush_graph_checks(self):
        self.m.flush_graph_checks()

    def __call__(self, batch):
        pred, true = self.m(batch)
        self.out.append((pred.detach().clone(), true.detach().clone()))
        return pred, true


@pytest.fixture(scope="module")
def crystals():
    from cartnet_amd.synthetic import make_crystal
    return [make_crystal(4100 + i, n) for i, n in enumerate(SIZES)]


def _cartnet(dim, rbf, layers, seed):
    from cartnet_amd.model import make_state_dict
    hp = dict(dim_in=dim, dim_rbf=rbf, num_layers=layers, radius=5.0, invariant=False, temperature=True,
              use_envelope=True, atom_types=True, cholesky=True)
    sd = make_state_dict(dim, rbf, layers, seed=seed)
    return _model(hp, sd).eval(), hp, sd


@pytest.mark.parametrize("dim,rbf,layers", [(64, 16, 2), (256, 64, 1)])
def test_eval_epoch_per_crystal_at_batch_4(crystals, dim, rbf, layers):
    from cartnet_amd.data import Batch, DataLoader
    from cartnet_amd.metrics import adp_metrics
    from cartnet_amd.train import compute_loss, eval_epoch
    from oracle import cartnet_ref as orc
    m, hp, sd = _cartnet(dim, rbf, layers, seed=11)
    rec = _Recorder(m)
    got = eval_epoch(DataLoader(crystals, 4), rec, adp_metrics=True, test_metrics=True, per_crystal=True)
    assert set(got) == {"mae", "volume_percentage_error", "similarity_index", "iou"}
    assert [int(p.shape[0]) for p, _ in rec.out] == [sum(int(c.non_H_mask.sum()) for c in crystals[:4]),
                                                      sum(int(c.non_H_mask.sum()) for c in crystals[4:])]
    # expected: the batched path's own predictions, crystal by crystal through the existing loss / metrics
    rows = [int(c.non_H_mask.sum()) for c in crystals]
    preds = list(torch.split(torch.cat([p for p, _ in rec.out]), rows))
    trues = list(torch.split(torch.cat([t for _, t in rec.out]), rows))
    want = {k: 0.0 for k in got}
    for p, t in zip(preds, trues):
        vol, sim, iou = adp_metrics(p, t)
        want["mae"] += float(compute_loss(p, t)[0].item())
        want["volume_percentage_error"] += float(vol.double().mean().item())
        want["similarity_index"] += float(sim.double().mean().item())
        want["iou"] += float(iou.double().mean().item())
    for k in got:
        print(k, got[k], want[k] / len(crystals))
        assert abs(got[k] - want[k] / len(crystals)) <= 1e-6 * abs(want[k] / len(crystals)), k
    # a crystal inside the batch against the same crystal alone, both against the fp64 oracle
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        for g, c in enumerate(crystals):
            alone, _ = m(Batch.from_data_list([c]).to("cuda:0"))
            b64 = Batch.from_data_list([c])
            for k, v in list(b64.__dict__.items()):
                if torch.is_tensor(v) and v.is_floating_point():
                    setattr(b64, k, v.double())
            ref = orc.cartnet_forward(sd64, b64, training=False, **gu.oracle_kwargs(hp))
            assert rel_err(preds[g], alone) < 2 * PRED_TOL, g
            assert rel_err(preds[g], ref) < PRED_TOL and rel_err(alone, ref) < PRED_TOL, g
    # with a loader of batch size 1 the per-crystal path gives the existing path's numbers
    old = eval_epoch(DataLoader(crystals, 1), m, adp_metrics=True, test_metrics=True)
    new = eval_epoch(DataLoader(crystals, 1), m, adp_metrics=True, test_metrics=True, per_crystal=True)
    for k in old:
        assert abs(new[k] - old[k]) <= 1e-6 * abs(old[k]), (k, new[k], old[k])
    only_mae = eval_epoch(DataLoader(crystals, 4), m, per_crystal=True)
    assert set(only_mae) == {"mae"} and abs(only_mae["mae"] - got["mae"]) <= 1e-12 * got["mae"]


def test_montecarlo_batch_against_the_batch_1_steps(crystals):
    from cartnet_amd import evaluate as entry
    from cartnet_amd.data import Batch
    from cartnet_amd.shard import random_rotations
    m, _, _ = _cartnet(64, 16, 2, seed=12)
    items = crystals[1:6]
    R = random_rotations(len(items), torch.Generator(device="cuda").manual_seed(8), "cuda")
    with torch.no_grad():
        batch = Batch.from_data_list(items).to("cuda:0")
        atoms = batch.x.clone()
        pred, res, rp = entry.montecarlo_batch(m, batch, R)
        assert torch.equal(batch.x, atoms)                                     # the caller still reads the atomic numbers
        rows = [int(c.non_H_mask.sum()) for c in items]
        assert (rp[1:] - rp[:-1]).tolist() == rows and res.volume_error is None
        for g, (p, t) in enumerate(zip(torch.split(pred, rows), torch.split(res.true, rows))):
            one = Batch.from_data_list([items[g]]).to("cuda:0")               # main.py:85-103 at batch size 1
            copy = gu.clone_batch(one)
            first, _ = m(one)
            copy.cart_dir = copy.cart_dir @ R[g]
            pseudo = R[g].transpose(-1, -2) @ first @ R[g]
            second, _ = m(copy)
            assert rel_err(p, second) < 2 * PRED_TOL, g
            bound = 2 * PRED_TOL * pseudo.abs().max().item() + ROT_TOL * first.abs().max().item()
            assert (t - pseudo).abs().max().item() <= bound, g


# ------------------------------------------------------------------------- batch size 1 is the reference's loop

def _loader_of_one(crystals, kind):
    """The three smallest crystals (1, 2 and 23 atoms), one per batch, from the host loader or from a resident shard."""
    from cartnet_amd.data import DataLoader
    from cartnet_amd.shard import DeviceShard, ShardLoader
    three = crystals[:3]
    return DataLoader(three, 1) if kind == "host" else ShardLoader(DeviceShard.from_data_list(three, "cuda:0"), 1)


@pytest.mark.parametrize("kind", ["host", "shard"])
def test_inference_at_batch_1_is_the_reference_loop(crystals, tmp_path, kind):
    from cartnet_amd import evaluate
    from cartnet_amd.metrics import compute_3D_IoU, get_similarity_index
    m, _, _ = _cartnet(64, 16, 2, seed=13)
    path = str(tmp_path / "inf.pkl")
    res = evaluate.inference(m, _loader_of_one(crystals, kind), "cuda:0", path)
    out = pickle.load(open(path, "rb"))
    assert tuple(out) == ("pred", "true", "temp", "cell", "refcode", "pos", "atoms", "iou", "mae", "similarity_index")
    assert out["temp"] == [] and out["refcode"] == []
    assert all(len(out[k]) == 3 for k in out if k not in ("temp", "refcode"))
    ious, maes, sims = [], [], []
    with torch.no_grad():
        for g, batch in enumerate(_loader_of_one(crystals, kind)):            # main.py:33-49, statement by statement
            batch.to("cuda:0")
            cell = batch.cell.detach().to("cpu")
            atoms = batch.x[batch.non_H_mask].detach().to("cpu")
            pos = batch.pos[batch.non_H_mask].detach().to("cpu")
            pred, true = m(batch)
            ious.append(compute_3D_IoU(pred, true).detach().to("cpu"))
            maes.append((pred - true).abs().detach().to("cpu"))
            sims.append(get_similarity_index(pred, true).detach().to("cpu"))
            assert torch.equal(out["pred"][g], pred.detach().to("cpu")), g
            assert torch.equal(out["true"][g], true.detach().to("cpu")), g
            assert torch.equal(out["iou"][g], ious[g]) and torch.equal(out["mae"][g], maes[g]), g
            assert torch.equal(out["similarity_index"][g], sims[g]), g
            assert torch.equal(out["atoms"][g], atoms) and torch.equal(out["pos"][g], pos), g
            assert tuple(out["cell"][g].shape) == (1, 3, 3) and torch.equal(out["cell"][g], cell), g
    assert g == 2
    assert res == {**evaluate.summary(torch.cat(ious), torch.cat(maes), torch.cat(sims)), "output": path}


@pytest.mark.parametrize("kind", ["host", "shard"])
def test_montecarlo_at_batch_1_is_the_reference_loop(crystals, tmp_path, kind):
    from cartnet_amd import evaluate
    from cartnet_amd.metrics import compute_3D_IoU, get_similarity_index
    from cartnet_amd.shard import random_rotations
    m, _, _ = _cartnet(64, 16, 2, seed=14)
    res = evaluate.montecarlo(m, _loader_of_one(crystals, kind), "cuda:0", str(tmp_path / "mc.pkl"), rounds=2, seed=5)
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    ious, maes, sims = [], [], []
    with torch.no_grad():
        for i in range(2):
            out = pickle.load(open(tmp_path / f"mc_montecarlo_{i}.pkl", "rb"))
            assert tuple(out) == ("pred", "true", "cell", "refcode", "pos", "atoms", "mae", "iou", "similarity_index")
            assert out["refcode"] == [] and out["pos"] == []
            assert all(len(out[k]) == 3 for k in out if k not in ("refcode", "pos"))
            for g, batch in enumerate(_loader_of_one(crystals, kind)):        # main.py:85-103, statement by statement
                batch_copy = gu.clone_batch(batch)
                batch.to("cuda:0")
                cell = batch.cell.detach().to("cpu")
                atoms = batch.x[batch.non_H_mask].detach().to("cpu")
                pseudo_true, _ = m(batch)
                R = random_rotations(1, gen, "cuda:0")[0]
                batch_copy.to("cuda:0")
                batch_copy.cart_dir = batch_copy.cart_dir @ R
                pseudo_true = R.transpose(-1, -2) @ pseudo_true @ R
                pred, _ = m(batch_copy)
                ious.append(compute_3D_IoU(pred, pseudo_true).detach().to("cpu"))
                sims.append(get_similarity_index(pred, pseudo_true).detach().to("cpu"))
                maes.append((pred - pseudo_true).abs().detach().to("cpu"))
                assert torch.equal(out["pred"][g], pred.detach().to("cpu")), (i, g)
                assert torch.equal(out["true"][g], pseudo_true.detach().to("cpu")), (i, g)
                assert torch.equal(out["iou"][g], ious[-1]) and torch.equal(out["mae"][g], maes[-1]), (i, g)
                assert torch.equal(out["similarity_index"][g], sims[-1]), (i, g)
                assert torch.equal(out["atoms"][g], atoms) and torch.equal(out["cell"][g], cell), (i, g)
    assert len(ious) == 6
    assert res == {"rounds": 2, **evaluate.summary(torch.cat(ious), torch.cat(maes), torch.cat(sims))}


# ------------------------------------------------------------------------------------------------ through main.py

COMMON = ["--synthetic", "60", "--atoms", "10", "30", "--dim_in", "64", "--num_layers", "2"]      # six test crystals


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """One training epoch with --eval_batch 4: (directory, checkpoint, result)."""
    import main as entry
    d = tmp_path_factory.mktemp("eval_batch")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        res = entry.main(COMMON + ["--epochs", "1", "--batch", "4", "--batch_accumulation", "1", "--name", "ck",
                                   "--eval_batch", "4"])
    finally:
        os.chdir(cwd)
    return d, str(d / "results" / "ck" / "0" / "ckpt" / "best.ckpt"), res


def test_training_run_with_eval_batch_reports_the_test_metrics(trained):
    tm = trained[2]["test_metrics"]
    assert set(tm) == {"mae", "volume_percentage_error", "similarity_index", "iou"}
    assert 0.0 < tm["iou"] <= 1.0 and tm["mae"] > 0 and trained[2]["test_mae"] == tm["mae"]


def _compare_inference(d, ck, extra, tol):
    import main as entry
    a = entry.main(extra + ["--inference", "--checkpoint_path", ck, "--inference_output", str(d / "one.pkl")])
    b = entry.main(extra + ["--inference", "--checkpoint_path", ck, "--inference_output", str(d / "four.pkl"),
                            "--eval_batch", "4"])
    assert set(a) == set(b)
    one, four = pickle.load(open(d / "one.pkl", "rb")), pickle.load(open(d / "four.pkl", "rb"))
    assert set(one) == set(four)
    for k in one:
        assert len(one[k]) == len(four[k]), k
        assert len(one[k]) in (0, 6), k
        for x, y in zip(one[k], four[k]):
            assert x.shape == y.shape and x.dtype == y.dtype, k
    for g in range(6):
        assert torch.equal(one["atoms"][g], four["atoms"][g]) and torch.equal(one["true"][g], four["true"][g])
        assert torch.equal(one["cell"][g], four["cell"][g])
        assert rel_err(four["pred"][g], one["pred"][g]) < tol, g


@pytest.mark.parametrize("resident", [False, True])
def test_inference_with_eval_batch_matches_batch_1(trained, resident):
    d, ck, _ = trained
    _compare_inference(d, ck, COMMON + (["--resident_dataset"] if resident else []), 2 * PRED_TOL)


def test_montecarlo_with_eval_batch(trained):
    import main as entry
    d, ck, _ = trained
    mc = entry.main(COMMON + ["--montecarlo", "--montecarlo_rounds", "2", "--checkpoint_path", ck, "--eval_batch", "4",
                              "--inference_output", str(d / "mc.pkl")])
    assert mc["rounds"] == 2 and 0.0 <= mc["iou_mean"] <= 1.0 and mc["mae_mean"] >= 0
    assert set(mc) == {"rounds", "iou_mean", "iou_std", "mae_mean", "mae_std", "similarity_index_mean",
                       "similarity_index_std"}
    for i in range(2):
        out = pickle.load(open(d / f"mc_montecarlo_{i}.pkl", "rb"))
        assert all(len(out[k]) == 6 for k in ("pred", "true", "cell", "atoms", "mae", "iou", "similarity_index"))
        for g in range(6):
            t = out["true"][g].double()
            assert t.shape == out["pred"][g].shape and t.shape[0] == out["atoms"][g].shape[0] == out["iou"][g].shape[0]
            # R^T p R of a symmetric p, rounded in fp32: two mirrored entries are each within ROT_TOL max|p| of one exact
            # value, and max|p| <= |p|_F = |R^T p R|_F <= 3 max|t| up to that rounding
            assert (t - t.transpose(1, 2)).abs().max().item() <= 2 * ROT_TOL * 3.01 * t.abs().max().item()
            assert bool((torch.linalg.eigvalsh(0.5 * (t + t.transpose(1, 2))) > 0).all())


def test_icomformer_inference_with_eval_batch(tmp_path, monkeypatch):
    import main as entry
    monkeypatch.chdir(tmp_path)
    common = ["--synthetic", "60", "--atoms", "10", "20", "--dim_in", "32", "--model", "icomformer"]
    entry.main(common + ["--epochs", "1", "--batch", "4", "--batch_accumulation", "1", "--name", "icf"])
    ck = str(tmp_path / "results" / "icf" / "0" / "ckpt" / "best.ckpt")
    _compare_inference(tmp_path, ck, common, 2 * ICF_EVAL_TOL)

"""Steps under poison: no result of a pass may depend on the bytes of a buffer that came from `torch.empty`.

cartnet_model_forward / _backward work in one workspace of 86 carved regions (`carve`, csrc/model.hip; csrc/icomformer.hip has
50 more), several of them sized by a maximum and shared between uses of different extents, and the workspace, the outputs
and the gradient staging buffers are all `torch.empty`.  A fresh process sees zeroed pages there, a second run the first
run's values: a stray row in a column sum, or a partial that a finalize kernel sums but nobody wrote, is invisible to the
other tests.  Here every case runs the same pass twice -- a fresh model of the same state_dict, a clone of the same batch --
once with every such buffer filled with 0x00 and once with 0xFF (NaN as fp32 / fp64 / bf16, -1 as an integer;
tests/poison_utils.py).  The two result sets (`pred`, `x_out`, `e_out`, `grad.*`, `buf.*`: stream_utils.collect) must be
equal bit for bit and hold no NaN, and the poison must have been live: fills were counted, and an allocation of exactly
the size cartnet_workspace_bytes / cartnet_icomformer_workspace_bytes returned is among them.

The integer regions were checked by reading the code before the first run (each is written in full before it is read:
cartnet_csr_build zeroes status / rowptr / colptr / perm and writes src32 / tgt32 for every edge, cn_group_ptrs_kernel,
cn_mask_index_kernel, cn_sort_by_key_kernel and cn_icf_index_kernel write every entry they own); under 0xFF a stray integer
would be -1.  Every comparison is of bytes; there is no tolerance in this file.
"""
import functools

import pytest
import torch

import poison_utils as pu
import stream_utils as su
from test_gpu_model import _model
from test_gpu_stream_order import DEV, _crystals, _hp, _icomformer, _small

pytestmark = pytest.mark.gpu

CARTNET_WS = "cartnet_workspace_bytes"
ICF_WS = "cartnet_icomformer_workspace_bytes"
MODES = ("train", "flat_adam", "second_backward", "eval", "train_nograd")


def _both(make, run, what, ws=None):
    """`run(make())` under each fill: liveness, no NaN, the same bytes.  Returns the two Fills records."""
    res, recs = [], []
    for byte in pu.FILLS:
        ctx = make()                   # fresh per fill: no gradient cache, image plan or running statistic of the other run
        torch.cuda.synchronize()
        with pu.size_queries(*([ws] if ws else [])) as sizes, pu.poisoned(byte) as rec:
            out = run(ctx)
            torch.cuda.synchronize()
        pu.assert_live(rec, sizes, f"{what}, fill 0x{byte:02X}", workspace=ws is not None)
        res.append(out)
        recs.append(rec)
    print(f"poison [{what}]: {len(res[0])} tensors; fills {recs[0].count} / {recs[1].count}, "
          f"bytes {recs[0].nbytes} / {recs[1].nbytes}")
    POISON_TOTALS["fills"] += recs[0].count + recs[1].count
    POISON_TOTALS["bytes"] += recs[0].nbytes + recs[1].nbytes
    for byte, out in zip(pu.FILLS, res):
        nan = [k for k, v in out.items() if v.is_floating_point() and bool(torch.isnan(v).any())]
        assert not nan, f"{what}: NaN under the fill 0x{byte:02X} in {nan[:12]}"
    su.assert_same(res[0], res[1], what, than="the fill 0x00 to the fill 0xFF")
    assert recs[0].sizes == recs[1].sizes, f"{what}: the two runs allocated differently"
    return recs


POISON_TOTALS = {"fills": 0, "bytes": 0}


@pytest.fixture(scope="module", autouse=True)
def _totals():
    """(after the last test of the file: what the helper counted, for the record)"""
    yield
    print(f"\npoison totals, steps: {POISON_TOTALS['fills']} fills, {POISON_TOTALS['bytes']} bytes")


# ------------------------------------------------------------------------------------------------------------------ CartNet
@functools.lru_cache(maxsize=None)
def _sd(hp_items, seed=21):
    from cartnet_amd.model import make_state_dict
    hp = dict(hp_items)
    return make_state_dict(hp["dim_in"], hp["dim_rbf"], hp["num_layers"], seed=seed, cholesky=hp["cholesky"],
                           temperature=hp["temperature"], atom_types=hp["atom_types"], invariant=hp["invariant"])


def _wide(**kw):
    return _hp(**dict(dict(dim_in=256, dim_rbf=64, num_layers=2), **kw))


def _make_cartnet(hp, precision, mode, half=False, groups=0):
    from cartnet_amd.optim import FlatAdam

    def make():
        m = _model(hp, _sd(tuple(sorted(hp.items()))), precision)
        m.half_storage, m.bn_group_size = half, groups
        opt = None
        if mode in ("flat_adam", "second_backward", "fused_loss"):
            m.train()
            opt = FlatAdam(m, lr=1e-3)
            opt.direct_grads = True
        return m, opt
    return make


def _loss(pred, true, batch=None):
    return (pred - true).abs().mean()


def _cartnet_run(batch, mode, loss=_loss):
    def run(ctx):
        m, opt = ctx
        passes = 3 if mode == "second_backward" else 1       # direct into the flat buffer, staging buffer new, staging buffer reused
        if mode in ("eval", "train_nograd"):
            m.train(mode == "train_nograd")
            b = su.clone_batch(batch)
            with torch.no_grad():
                pred, _ = m(b)
            return su.collect(m, pred, b, grads=False)
        m.train()
        if opt is not None:
            opt.zero_grad()
        else:
            m.zero_grad(set_to_none=True)
        for _ in range(passes):
            b = su.clone_batch(batch)
            pred, true = m(b)
            loss(pred, true, b).backward()
        if mode == "second_backward":
            assert m.__dict__.get("_grad_cache") is not None and m.__dict__.get("_grad_direct") is not None
        return su.collect(m, pred, b)
    return run


def _cartnet_case(hp, precision, mode, batch, what, **kw):
    return _both(_make_cartnet(hp, precision, mode, **kw), _cartnet_run(batch, mode), what, ws=CARTNET_WS)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_cartnet_width_256(precision, mode):
    """train: the staging buffer of a model without an optimiser; flat_adam: the gradients go straight into FlatAdam's flat
    buffer; second_backward: two more backward passes before zero_grad (`_grad_cache` made, then reused); eval /
    train_nograd: need_backward = 0 -- the ping-pong buffers, and in eval mode at precision 0 `gate_bnd`."""
    hp = _wide()
    _cartnet_case(hp, precision, mode, _small(hp), f"CartNet D=256 L=2 precision {precision} {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_cartnet_half_storage(mode):
    hp = _wide()
    _cartnet_case(hp, 2, mode, _small(hp), f"CartNet D=256 precision 2, bf16 storage, {mode}", half=True)


@pytest.mark.parametrize("precision,half", [(0, False), (2, True)])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_cartnet_bn_groups(mode, precision, half):
    """bn_group_size = 2 on 4 crystals: gparts / nrows_n are G x parts per group, pa..pd are sized by their maximum."""
    hp = _wide()
    _cartnet_case(hp, precision, mode, _small(hp), f"CartNet D=256 precision {precision} half {half} groups of 2, {mode}",
                  half=half, groups=2)


@pytest.mark.parametrize("mode", MODES)
def test_cartnet_width_64_three_layers(mode):
    """No weight images at D = 64: the general kernels run every product."""
    hp = _hp(num_layers=3)
    _cartnet_case(hp, 0, mode, _small(hp), f"CartNet D=64 L=3 {mode}")


VARIANTS = {
    "invariant_kf50": dict(invariant=True, dim_rbf=50),       # kf = 50: ldf = 64, 14 zero-padded columns of feat / rows of edge0T
    "invariant_kf64": dict(invariant=True, dim_rbf=64),       # kf % 16 == 0: no padding
    "scalar_head": dict(cholesky=False, temperature=False),
    "no_atom_types": dict(atom_types=False),
    "no_temperature": dict(temperature=False),
    "plain": dict(atom_types=False, temperature=False),       # one learned row for every atom, no atom MLP
    "no_envelope": dict(use_envelope=False),
}


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_cartnet_variants(variant, mode):
    hp = _wide(**VARIANTS[variant])
    kf = hp["dim_rbf"] + (0 if hp["invariant"] else 3)
    assert (kf % 16 == 0) == (variant == "invariant_kf64")
    _cartnet_case(hp, 0, mode, _small(hp), f"CartNet D=256 {variant} {mode}")


# ------------------------------------------------------------------------------------------------------- degenerate batches
def _strip(d):
    d.edge_index = torch.zeros(2, 0, dtype=torch.int64)
    d.cart_dist, d.cart_dir = torch.zeros(0), torch.zeros(0, 3)
    return d


@functools.lru_cache(maxsize=None)
def _degenerate(kind):
    from cartnet_amd.data import Batch
    from cartnet_amd.synthetic import make_crystal
    if kind == "no_edges":                                   # E = 0 for the whole batch
        items = [_strip(make_crystal(40 + i, n)) for i, n in enumerate((3, 1, 5))]
    elif kind == "lonely_and_isolated":                      # a crystal without edges between two with edges; isolated atoms
        items = [make_crystal(2, 9), _strip(make_crystal(1, 3)), make_crystal(72, 17)]
        d = items[2]                                         # drop every edge into atom 5, and one more: E = 334
        keep = d.edge_index[1] != 5
        keep[int(torch.nonzero(keep)[0])] = False
        d.edge_index, d.cart_dist, d.cart_dir = d.edge_index[:, keep], d.cart_dist[keep], d.cart_dir[keep]
    elif kind == "one_atom":                                 # N = 1, M = 1: one non-H atom and its periodic images
        items = [make_crystal(43, 1)]
    else:                                                    # N = 271, E = 4,004: no multiple of 128, 256, 1024 / of 128
        items = [make_crystal(820 + i, n) for i, n in enumerate((37, 51, 66, 45, 72))]
    return Batch.from_data_list(items)


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("kind", ["no_edges", "lonely_and_isolated", "one_atom", "ragged"])
def test_cartnet_degenerate_batches(kind, precision, mode):
    hp = _wide()
    b = su.clone_batch(_degenerate(kind)).to(DEV)
    N, E = int(b.x.shape[0]), int(b.edge_index.shape[1])
    if kind == "no_edges":
        assert E == 0
    elif kind == "one_atom":
        assert N == 1 and E > 0 and int(b.y.shape[0]) == 1
    elif kind == "ragged":
        assert N % 128 and N % 256 and N % 1024 and E % 128 and N > 256
    else:
        deg = torch.bincount(b.edge_index[1], minlength=N)
        assert E % 16 and int((deg == 0).sum()) == 4 and bool((deg[9:12] == 0).all()) and int(deg[17]) == 0
    _cartnet_case(hp, precision, mode, b, f"CartNet D=256 precision {precision} {kind} {mode}")


# --------------------------------------------------------------------------------------------------------------- Comformer
def _comformer_run(batch, mode):
    def run(m):
        b = su.clone_batch(batch)
        if mode == "eval":
            m.eval()
            with torch.no_grad():
                pred, _ = m(b)
            return su.collect(m, pred, b, grads=False)
        m.train()
        m.zero_grad(set_to_none=True)
        pred, true = m(b)
        _loss(pred, true).backward()
        return su.collect(m, pred, b)
    return run


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("groups", [0, 2])
def test_icomformer_native_sequence(groups, precision, mode):
    b = su.clone_batch(_crystals(960, (10, 17, 24, 13))).to(DEV)
    _both(lambda: _icomformer(16, True, precision, groups)[0], _comformer_run(b, mode),
          f"iComformer C++ sequence, precision {precision}, groups {groups}, {mode}", ws=ICF_WS)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_icomformer_python_sequence(mode):
    """Every buffer of the sequence is a `torch.empty` of its own (`_e`, `_parts`); no workspace."""
    b = su.clone_batch(_crystals(960, (10, 17, 24, 13))).to(DEV)
    recs = _both(lambda: _icomformer(16, False, 0)[0], _comformer_run(b, mode), f"iComformer Python sequence, {mode}")
    assert recs[0].count > 50


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("width", [32, 256])
def test_ecomformer(width, mode):
    from cartnet_amd.comformer import eComformer, make_ecomformer_state_dict
    sd = make_ecomformer_state_dict(width, seed=4)

    def make():
        m = eComformer(width)
        m.load_state_dict(sd)
        m.validate_graph = True
        return m.to(DEV)
    b = su.clone_batch(_crystals(1000, (1, 2, 23, 11))).to(DEV)
    recs = _both(make, _comformer_run(b, mode), f"eComformer width {width}, {mode}")
    assert recs[0].count > 50


# ------------------------------------------------------------------------------------------------- fused loss and optimiser
def test_grouped_loss_step():
    """bn_group_size = 2 with train.grouped_loss, the recipe's pairing: the sum of the per-group MAEs is descended."""
    from cartnet_amd.train import grouped_loss
    hp = _wide()
    run = _cartnet_run(_small(hp), "train", loss=lambda pred, true, b: grouped_loss(pred, true, b, 2)[0])
    _both(_make_cartnet(hp, 0, "train", groups=2), run, "CartNet D=256 groups of 2, grouped_loss", ws=CARTNET_WS)


@pytest.mark.parametrize("which", [0, 1])
def test_fused_loss_step(which):
    """compute_loss + train.backward with a FlatAdam attached: the two-node shortcut, whose gradient is the one
    cartnet_loss_fwd_unit left in `ctx.unit` (a `torch.empty` of 2 n floats)."""
    from cartnet_amd import train
    hp = _wide()
    batch = _small(hp)

    def run(ctx):
        m, opt = ctx
        m.train()
        opt.zero_grad()
        b = su.clone_batch(batch)
        pred, true = m(b)
        assert pred.numel() <= 4096
        losses = train.compute_loss(pred, true)
        train.backward(losses[which])
        out = su.collect(m, pred, b)
        out["mae"], out["mse"] = losses[0].detach().clone(), losses[1].detach().clone()
        return out
    _both(_make_cartnet(hp, 0, "fused_loss"), run, f"CartNet D=256 fused loss, output {which}", ws=CARTNET_WS)


@pytest.mark.parametrize("n_rows", [3, 455, 456, 700])
def test_fused_loss_kernels(n_rows):
    """The loss alone, on both sides of its 4,096-element threshold (455 / 456 rows of 9): cartnet_loss_fwd_unit or
    cartnet_loss_fwd with its fp64 partials, and cartnet_loss_bwd into an `empty_like` for a seed that is not the cached one."""
    from cartnet_amd import train
    g = torch.Generator().manual_seed(n_rows)
    p0, t0 = torch.randn(n_rows, 3, 3, generator=g).to(DEV), torch.randn(n_rows, 3, 3, generator=g).to(DEV)

    def run(_):
        out = {}
        for name, seed in (("unit", None), ("scaled", 1.5)):
            for which in (0, 1):
                p = p0.clone().requires_grad_(True)
                losses = train.compute_loss(p, t0)
                if seed is None:
                    train.backward(losses[which])
                else:
                    (losses[which] * seed).backward()
                out[f"{name}.{which}.mae"], out[f"{name}.{which}.mse"] = losses[0].detach().clone(), losses[1].detach().clone()
                out[f"{name}.{which}.grad"] = p.grad.detach().clone()
        return out
    _both(lambda: None, run, f"fused loss, {n_rows} rows")


def test_flat_adam_step():
    """FlatAdam built under poison (its flat parameter buffer is a `torch.empty` that the copies must cover), one training
    step into it, one cartnet_adam_step."""
    from cartnet_amd.optim import FlatAdam
    hp = _wide()
    batch = _small(hp)

    def run(ctx):
        m, _ = ctx
        m.train()
        opt = FlatAdam(m, lr=1e-3)
        opt.direct_grads = True
        opt.zero_grad()
        b = su.clone_batch(batch)
        pred, true = m(b)
        _loss(pred, true).backward()
        opt.step()
        out = su.collect(m, pred, b)
        out.update(flat_param=opt.flat_param.clone(), exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone())
        for n, p in m.named_parameters():
            out["param." + n] = p.detach().clone()
        return out
    _both(_make_cartnet(hp, 0, "train"), run, "CartNet D=256, FlatAdam built, one step", ws=CARTNET_WS)

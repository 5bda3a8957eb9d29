"""Whole-network parity on the GPU: cartnet_amd.CartNet (HIP kernels through the C ABI) against
  (a) the golden vectors generated from the reference itself (tests/golden/*.npz), and
  (b) the oracle (oracle/cartnet_ref.py, fp64 on the CPU) on other seeded inputs,
plus size-independent properties at the benchmark's full graph size.

Tolerances (fp32 path): predictions max|delta| <= 1e-5 * max|ref| (north_star).  Gradients use the same norm-wise
metric over the whole gradient vector, max|delta| <= 3e-5 * max|ref_all| (the reference's OWN fp32 run is off by
up to 4.4e-5 on this metric against its fp64 run on these fixtures -- tests/golden/config1.npz, the bias in front of
a training-mode BatchNorm whose true gradient is 0; the HIP path measures 2e-6..1.3e-5), plus a per-parameter guard
||delta_k||_2 <= 1e-3 * max(||ref_k||_2, 1e-2 * ||ref_all||_2) that catches a wrong tensor.  Integers bit-exact.
"""
import numpy as np
import pytest
import torch

import golden_utils as gu
from conftest import rel_err

pytestmark = pytest.mark.gpu

PRED_TOL = 1e-5
GRAD_TOL = 3e-5
GRAD_TOL_PARAM = 1e-3


PRECISIONS = [0, 1]      # 0: fp32 MFMA, 1: bf16x3 split-operand MFMA -- both must meet the same parity budget


def _model(hp, sd, precision=0):
    """hp["radius"] is the encoder's RBF cutoff (a constructor argument); the layers' envelope radius is the global
    cfg.radius at construction time (models/cartnet.py:201), hp["env_radius"] where a fixture sets the two apart.  The
    global is put back: other tests build CartNet without setting it."""
    from cartnet_amd.config import cfg
    from cartnet_amd.model import CartNet
    old = cfg.radius, cfg.invariant
    cfg.radius = hp.get("env_radius", hp["radius"])
    cfg.invariant = hp["invariant"]
    try:
        m = CartNet(hp["dim_in"], hp["dim_rbf"], hp["num_layers"], radius=hp["radius"], invariant=hp["invariant"],
                    temperature=hp["temperature"], use_envelope=hp["use_envelope"], atom_types=hp["atom_types"],
                    cholesky=hp["cholesky"])
    finally:
        cfg.radius, cfg.invariant = old
    assert m.encoder.rbf.cutoff_upper == hp["radius"]
    assert all(l.envelope_radius == hp.get("env_radius", hp["radius"]) for l in m.layers)
    m.load_state_dict(sd, strict=True)
    m.validate_graph = True
    m.gemm_precision = precision
    return m.to("cuda:0")


def _check_grads(got, ref, what=""):
    """got / ref: dict name -> tensor.  Norm-wise check over the whole vector + per-parameter guard."""
    ref = {k: v.double().cpu() for k, v in ref.items()}
    got = {k: v.detach().double().cpu() for k, v in got.items()}
    gmax = max(v.abs().max().item() for v in ref.values())
    l2_all = sum((v ** 2).sum().item() for v in ref.values()) ** 0.5
    for k, r in ref.items():
        assert k in got and got[k] is not None, f"{what}: no gradient for {k}"
        d = got[k].reshape(r.shape) - r
        assert torch.isfinite(d).all(), f"{what}: non-finite gradient for {k}"
        assert d.abs().max().item() <= GRAD_TOL * gmax, (what, k, d.abs().max().item() / gmax)
        assert d.norm().item() <= GRAD_TOL_PARAM * max(r.norm().item(), 1e-2 * l2_all), \
            (what, k, d.norm().item(), r.norm().item())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", gu.MODEL_FIXTURES)
def test_forward_against_reference_golden(name, precision):
    z, hp, b, sd = gu.load(name)
    m = _model(hp, sd, precision)
    for mode in ("eval", "train"):
        m.train(mode == "train")
        bb = gu.clone_batch(b).to("cuda:0")
        with torch.no_grad():
            pred, true = m(bb)
        assert true is bb.y
        assert pred.shape == tuple(z[f"{mode}_pred_f64"].shape)
        assert rel_err(pred, torch.from_numpy(z[f"{mode}_pred_f64"])) < PRED_TOL, (name, mode)
        assert rel_err(pred, torch.from_numpy(z[f"{mode}_pred"])) < PRED_TOL, (name, mode)
        # forward replaces batch.x / batch.edge_attr with the final features, as the reference does
        assert bb.x.shape == (b.x.shape[0], hp["dim_in"]) and bb.x.dtype == torch.float32
        assert bb.edge_attr.shape == (b.edge_index.shape[1], hp["dim_in"])


def test_per_layer_features_against_reference_golden():
    z, hp, b, sd = gu.load("tiny_adp")
    L = hp["num_layers"]
    m = _model(hp, sd).train()
    bb = gu.clone_batch(b).to("cuda:0")
    with torch.no_grad():
        m(bb)
    assert rel_err(bb.x, torch.from_numpy(z[f"trace_x{L}"])) < PRED_TOL
    assert rel_err(bb.edge_attr, torch.from_numpy(z[f"trace_e{L}"])) < PRED_TOL


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["tiny_radius6", "tiny_radius4"])
def test_per_layer_features_with_two_radii_against_reference_golden(name, precision):
    """--radius 6 / 4 as the reference runs it (RBF cutoff 5.0, envelope radius = the flag): the last layer's node and
    edge features against the reference's trace."""
    z, hp, b, sd = gu.load(name)
    L = hp["num_layers"]
    m = _model(hp, sd, precision).train()
    bb = gu.clone_batch(b).to("cuda:0")
    with torch.no_grad():
        m(bb)
    assert rel_err(bb.x, torch.from_numpy(z[f"trace_x{L}"])) < PRED_TOL
    assert rel_err(bb.edge_attr, torch.from_numpy(z[f"trace_e{L}"])) < PRED_TOL


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_radii_at_width_256_against_oracle(precision):
    """--radius 6 at the width that takes the DMA-fed kernels: crystals built with radius 6 (edges with 5 <= d < 6: RBF
    block exactly 0, envelope positive), cfg.radius = 6 for the envelopes, RBF cutoff 5.0.  Train and eval against the fp64
    oracle; the same oracle with the envelope at 5.0 is far outside the budget, so crossed plumbing cannot pass."""
    from cartnet_amd.data import Batch
    from cartnet_amd.model import make_state_dict
    from cartnet_amd.synthetic import make_crystal
    from oracle import cartnet_ref as orc
    hp = dict(dim_in=256, dim_rbf=64, num_layers=2, radius=5.0, env_radius=6.0, invariant=False, temperature=True,
              use_envelope=True, atom_types=True, cholesky=True)
    b = Batch.from_data_list([make_crystal(340 + i, n, radius=6.0) for i, n in enumerate((12, 20))])
    assert int((b.cart_dist >= 5.0).sum()) >= 0.2 * b.cart_dist.numel() and bool((b.cart_dist < 6.0).all())
    sd = make_state_dict(256, 64, 2, seed=13)
    m = _model(hp, sd, precision)
    assert m.encoder.rbf.cutoff_upper == 5.0 and m.layers[0].envelope_radius == 6.0
    names = set(k for k, _ in m.named_parameters())
    m.train()
    pred, true = m(gu.clone_batch(b).to("cuda:0"))
    (pred - true).abs().mean().backward()
    ref, gref = _oracle_run(b, hp, sd, names)
    assert rel_err(pred, ref) < PRED_TOL
    _check_grads({k: p.grad for k, p in m.named_parameters()}, gref, "two radii")
    b64 = gu.clone_batch(b)
    for k, v in list(b64.__dict__.items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(b64, k, v.double())
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    crossed = orc.cartnet_forward(sd64, b64, training=True, **{**gu.oracle_kwargs(hp), "envelope_radius": 5.0})
    assert rel_err(pred, crossed) > 1e-3
    m.eval()
    m.load_state_dict(sd)                                  # the training pass moved the running statistics
    with torch.no_grad():
        pred_eval, _ = m(gu.clone_batch(b).to("cuda:0"))
    ref_eval = orc.cartnet_forward(sd64, b64, training=False, **gu.oracle_kwargs(hp))
    assert rel_err(pred_eval, ref_eval) < PRED_TOL
    crossed = orc.cartnet_forward(sd64, b64, training=False, **{**gu.oracle_kwargs(hp), "envelope_radius": 5.0})
    assert rel_err(pred_eval, crossed) > 1e-3


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", gu.MODEL_FIXTURES)
def test_train_step_gradients_and_bn_state_against_reference_golden(name, precision):
    z, hp, b, sd = gu.load(name)
    m = _model(hp, sd, precision).train()
    bb = gu.clone_batch(b).to("cuda:0")
    pred, true = m(bb)
    loss = (pred - true).abs().mean()                 # MAE, train/metrics.py:26 -- the reference's default loss
    assert abs(loss.item() - float(z["train_mae"])) < 1e-5 * abs(float(z["train_mae"]))
    loss.backward()
    params = dict(m.named_parameters())
    for k, p in params.items():
        assert p.grad is not None, f"no gradient for {k}"
    if ("grad64_" + next(iter(params))) in z.files:
        _check_grads({k: p.grad for k, p in params.items()},
                     {k: torch.from_numpy(z["grad64_" + k]) for k in params}, name)
    else:   # config2: the fixture keeps the first 64 entries, the norm and a random projection of every gradient
        _check_grads({k: p.grad.flatten()[:64] for k, p in params.items()},
                     {k: torch.from_numpy(z["gradhead_" + k]) for k in params}, name)
        rng = np.random.default_rng(12345)
        l2_all = sum(float(z["gradnorm_" + k]) ** 2 for k in params) ** 0.5
        for k, p in params.items():
            g = p.grad.detach().double().cpu().flatten().numpy()
            probe = rng.standard_normal(g.size)
            nrm = float(z["gradnorm_" + k])
            bound = GRAD_TOL_PARAM * max(nrm, 1e-2 * l2_all)
            assert abs(np.linalg.norm(g) - nrm) <= bound, k
            # <delta, probe> ~ N(0, ||delta||^2) for a unit-variance probe: 5 sigma
            assert abs(np.dot(g, probe) - float(z["gradprobe_" + k])) <= 5 * bound, k
    sd_new = m.state_dict()
    for k in z.files:
        if not k.startswith("state_"):
            continue
        ref = torch.from_numpy(z[k])
        got = sd_new[k[6:]]
        if ref.is_floating_point():
            assert rel_err(got, ref) < 1e-5, k
        else:
            assert int(got) == int(ref), k


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["tiny_adp", "config1"])
def test_mse_loss_train_step_against_the_oracle(name, precision):
    """cfg.loss = "MSE" (reference train/train.py:173-178 picks the loss by name, train/metrics.py:27 is MSELoss with mean
    reduction): one iteration of cartnet_amd.train.train_epoch on the fixture's batch -- forward, compute_loss, the
    configured loss, backward, optimiser boundary -- against the fp64 oracle's autograd of the same loss."""
    from cartnet_amd.config import cfg
    from cartnet_amd.train import train_epoch
    from oracle import cartnet_ref as orc
    z, hp, b, sd = gu.load(name)
    m = _model(hp, sd, precision).train()

    class Capture:                      # stands where the optimiser stands: keeps what the step would consume
        def __init__(self):
            self.grads, self.steps = None, 0

        def zero_grad(self):
            m.zero_grad(set_to_none=True)

        def step(self):
            self.grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
            self.steps += 1
    opt = Capture()
    old = cfg.loss
    cfg.loss = "MSE"
    try:
        stats = train_epoch([gu.clone_batch(b)], m, opt, batch_accumulation=1)
    finally:
        cfg.loss = old
    assert opt.steps == 1 and stats["graphs"] == b.num_graphs

    sd64 = {k: (v.double().requires_grad_(k in opt.grads) if v.is_floating_point() else v) for k, v in sd.items()}
    b64 = gu.clone_batch(b)
    for k, v in list(b64.__dict__.items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(b64, k, v.double())
    ref = orc.cartnet_forward(sd64, b64, training=True, **gu.oracle_kwargs(hp))
    mse = ((ref - b64.y) ** 2).mean()
    mse.backward()
    assert abs(stats["mae"] - (ref - b64.y).abs().mean().item()) < 1e-5 * (ref - b64.y).abs().mean().item()
    _check_grads(opt.grads, {k: sd64[k].grad for k in opt.grads}, f"MSE {name}")
    # and it is NOT the MAE gradient (the loss switch is live): the two differ by far more than the tolerance
    gmae = torch.from_numpy(z["grad64_" + next(iter(opt.grads))])
    g0 = opt.grads[next(iter(opt.grads))].double().cpu()
    assert (g0 - gmae).abs().max().item() > 1e-3 * gmae.abs().max().item()


@pytest.mark.parametrize("seed,n_graphs,dim,layers,cholesky", [(0, 5, 32, 3, True), (1, 3, 128, 1, True),
                                                               (2, 6, 32, 2, False)])
def test_against_oracle_on_ragged_batches(seed, n_graphs, dim, layers, cholesky):
    """Variable-size crystals (incl. a 1-atom and a 2-atom cell), fresh weights: HIP path vs fp64 oracle."""
    from cartnet_amd.data import Batch
    from cartnet_amd.model import make_state_dict
    from cartnet_amd.synthetic import make_crystal
    from oracle import cartnet_ref as orc
    sizes = [1, 2, 23, 40, 11, 64][:n_graphs]
    b = Batch.from_data_list([make_crystal(900 + seed * 10 + i, n, adp=cholesky) for i, n in enumerate(sizes)])
    hp = dict(dim_in=dim, dim_rbf=16, num_layers=layers, radius=5.0, invariant=False, temperature=cholesky,
              use_envelope=True, atom_types=True, cholesky=cholesky)
    sd = make_state_dict(dim, 16, layers, seed=seed, cholesky=cholesky, temperature=cholesky)
    m = _model(hp, sd).train()
    bb = gu.clone_batch(b).to("cuda:0")
    pred, true = m(bb)
    (pred - true).abs().mean().backward()

    sd64 = {k: (v.double().requires_grad_(k in dict(m.named_parameters())) if v.is_floating_point() else v)
            for k, v in sd.items()}
    b64 = gu.clone_batch(b)
    for k, v in list(b64.__dict__.items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(b64, k, v.double())
    ref = orc.cartnet_forward(sd64, b64, training=True, **gu.oracle_kwargs(hp))
    assert rel_err(pred, ref) < PRED_TOL
    (ref - b64.y).abs().mean().backward()
    _check_grads({k: p.grad for k, p in m.named_parameters()},
                 {k: sd64[k].grad for k, _ in m.named_parameters()}, "ragged")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_bitwise_reproducible_and_graph_order_invariant_at_full_size(precision):
    """BASELINE.json configs[1] shapes (D=256, L=4, 194-atom crystals): two runs are bit-identical (no atomics),
    and permuting the crystals inside the batch permutes the per-crystal outputs (CSR/CSC built per batch)."""
    from cartnet_amd.data import Batch
    from cartnet_amd.model import make_state_dict
    from cartnet_amd.synthetic import make_crystal
    items = [make_crystal(700 + g, 194) for g in range(4)]
    hp = dict(dim_in=256, dim_rbf=64, num_layers=4, radius=5.0, invariant=False, temperature=True,
              use_envelope=True, atom_types=True, cholesky=True)
    sd = make_state_dict(256, 64, 4, seed=5)
    m = _model(hp, sd, precision).train()

    def run(order):
        b = Batch.from_data_list([items[i] for i in order]).to("cuda:0")
        m.zero_grad(set_to_none=True)
        m.load_state_dict(sd)
        pred, true = m(b)
        (pred - true).abs().mean().backward()
        g = torch.cat([p.grad.flatten() for p in m.parameters()])
        sizes = [int(items[i].non_H_mask.sum()) for i in order]
        return pred.detach(), g.detach(), sizes

    p1, g1, s1 = run([0, 1, 2, 3])
    p2, g2, _ = run([0, 1, 2, 3])
    assert torch.equal(p1, p2) and torch.equal(g1, g2)
    assert torch.isfinite(p1).all() and torch.isfinite(g1).all()
    # symmetric positive definite outputs (Cholesky head)
    assert torch.equal(p1, p1.transpose(1, 2))
    assert bool((torch.linalg.eigvalsh(p1.double().cpu()) > 0).all())
    p3, g3, s3 = run([2, 0, 3, 1])
    chunks1 = dict(zip([0, 1, 2, 3], torch.split(p1, s1)))
    chunks3 = dict(zip([2, 0, 3, 1], torch.split(p3, s3)))
    for gi in range(4):
        assert rel_err(chunks3[gi], chunks1[gi]) < PRED_TOL
    assert rel_err(g3, g1) < 1e-4


@pytest.mark.parametrize("half", [False, True])
def test_bf16_step_is_bitwise_repeatable_on_the_benchmark_batch(half):
    """Precision 2 (and bf16 storage) on the whole benchmark batch -- 64 crystals x 194 atoms, ~177k edges, every GEMM a
    few thousand workgroups: forward + backward twice, bit-identical predictions and gradients.  The small fixtures cannot
    see a missing barrier in a K-loop (waves of a workgroup only drift apart when the chip is oversubscribed)."""
    from cartnet_amd.data import Batch
    from cartnet_amd.model import make_state_dict
    from cartnet_amd.synthetic import make_crystal
    items = [make_crystal(900 + g, 194) for g in range(64)]
    hp = dict(dim_in=256, dim_rbf=64, num_layers=4, radius=5.0, invariant=False, temperature=True,
              use_envelope=True, atom_types=True, cholesky=True)
    sd = make_state_dict(256, 64, 4, seed=6)
    m = _model(hp, sd, 2).train()
    m.half_storage = half

    def run():
        b = Batch.from_data_list(items).to("cuda:0")
        m.zero_grad(set_to_none=True)
        m.load_state_dict(sd)
        pred, true = m(b)
        (pred - true).abs().mean().backward()
        return pred.detach().clone(), torch.cat([p.grad.flatten() for p in m.parameters()]).clone()

    p1, g1 = run()
    assert torch.isfinite(p1).all() and torch.isfinite(g1).all() and g1.abs().max().item() > 0
    for _ in range(3):
        p2, g2 = run()
        assert torch.equal(p1, p2) and torch.equal(g1, g2)


def test_product_path_refuses_cpu_tensors():
    z, hp, b, sd = gu.load("tiny_adp")
    from cartnet_amd.model import CartNet
    m = CartNet(hp["dim_in"], hp["dim_rbf"], hp["num_layers"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(gu.clone_batch(b))


# ---------------------------------------------------------------------------------------------------------------
# BASELINE configs[2]: Jarvis formation-energy shapes (scripts/train_cartnet_jarvis.sh: batch 64, Scalar_head, no
# temperature -- main.py:183) in the reduced-precision GEMM mode (gemm_precision = 2: bf16 operands, one MFMA product,
# fp32 accumulate and fp32 storage).  The reference states no crystal sizes for Jarvis; SURVEY.md §8(d) assumes 2..20
# atoms per cell.  Tolerances are bf16's (8-bit significand, K = 256..512 products per output), written here:
# predictions 3e-2 * max|ref|, gradients 8e-2 * max|g_all| -- and the same model at precisions 0 and 1 must still meet
# the fp32 budget on these shapes.
BF16_PRED_TOL = 3e-2
BF16_GRAD_TOL = 8e-2


def _jarvis_case(seed=7, n_graphs=64):
    from cartnet_amd.data import Batch
    from cartnet_amd.model import make_state_dict
    from cartnet_amd.synthetic import make_crystal
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(2, 21, (n_graphs,), generator=gen).tolist()
    b = Batch.from_data_list([make_crystal(5000 + i, n, adp=False) for i, n in enumerate(sizes)])
    hp = dict(dim_in=256, dim_rbf=64, num_layers=4, radius=5.0, invariant=False, temperature=False,
              use_envelope=True, atom_types=True, cholesky=False)
    sd = make_state_dict(256, 64, 4, seed=seed, cholesky=False, temperature=False)
    return b, hp, sd


def _oracle_run(b, hp, sd, names):
    from oracle import cartnet_ref as orc
    sd64 = {k: (v.double().requires_grad_(k in names) if v.is_floating_point() else v) for k, v in sd.items()}
    b64 = gu.clone_batch(b)
    for k, v in list(b64.__dict__.items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(b64, k, v.double())
    ref = orc.cartnet_forward(sd64, b64, training=True, **gu.oracle_kwargs(hp))
    (ref - b64.y).abs().mean().backward()
    return ref.detach(), {k: sd64[k].grad for k in names}


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_jarvis_shapes_scalar_head_all_precisions(precision):
    b, hp, sd = _jarvis_case()
    m = _model(hp, sd, precision).train()
    bb = gu.clone_batch(b).to("cuda:0")
    pred, true = m(bb)
    assert pred.shape == (b.num_graphs,)
    (pred - true).abs().mean().backward()
    names = [k for k, _ in m.named_parameters()]
    ref, gref = _oracle_run(b, hp, sd, set(names))
    got = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}
    gmax = max(v.abs().max().item() for v in gref.values())
    gerr = max((got[k].reshape(gref[k].shape) - gref[k]).abs().max().item() for k in names) / gmax
    perr = rel_err(pred, ref)
    if precision == 2:
        assert perr < BF16_PRED_TOL and gerr < BF16_GRAD_TOL, (perr, gerr)
        assert perr > 1e-6, "precision 2 must actually run the bf16 kernels on D = 256"
    else:
        assert perr < PRED_TOL and gerr < GRAD_TOL, (perr, gerr)


def test_gradients_written_straight_into_a_fresh_flat_buffer():
    """FlatAdam.direct_grads: after zero_grad() the native backward writes the optimiser's flat gradient buffer itself
    (no staging buffer, no accumulation launch) -- bitwise the staged gradients; a second backward before the next
    zero_grad() accumulates (the staging path), and the flag is off unless a training loop switches it on."""
    from cartnet_amd.optim import FlatAdam
    from cartnet_amd.train import backward, compute_loss
    b, hp, sd = _jarvis_case(n_graphs=16)

    def grads(direct, twice):
        m = _model(hp, sd, 0).train()
        opt = FlatAdam(m, lr=1e-3)
        assert opt.direct_grads is False
        opt.direct_grads = direct
        opt.zero_grad()
        assert opt.fresh is direct
        for _ in range(2 if twice else 1):
            pred, true = m(gu.clone_batch(b).to("cuda:0"))
            backward(compute_loss(pred, true)[0])
            assert opt.fresh is False
        assert all(p.grad.data_ptr() >= opt.flat_grad.data_ptr() for p in m.parameters())
        return opt.flat_grad.clone()

    staged, direct = grads(False, False), grads(True, False)
    assert staged.abs().max().item() > 0 and torch.equal(staged, direct)
    assert torch.equal(grads(False, True), grads(True, True))      # second backward: accumulated in both modes


def test_training_helper_backward_without_the_autograd_engine():
    """cartnet_amd.train.backward runs the two backward functions of the step's two-node graph itself (no engine hand-off)
    when the graph is exactly compute_loss(CartNet(batch)) with a FlatAdam attached, and falls back to the engine for
    anything else; both deliver bitwise the same gradients, for either loss."""
    from cartnet_amd import train as ctrain
    from cartnet_amd.optim import FlatAdam
    b, hp, sd = _jarvis_case(n_graphs=16)

    def grads(which, how):
        m = _model(hp, sd, 0).train()
        opt = FlatAdam(m, lr=1e-3)
        opt.zero_grad()
        pred, true = m(gu.clone_batch(b).to("cuda:0"))
        loss = ctrain.compute_loss(pred, true)[which]
        if how == "engine":
            loss.backward()
        elif how == "helper":
            assert ctrain._two_node_backward(loss, torch.ones((), device="cuda:0"))
            with pytest.raises(RuntimeError):
                loss.backward()                  # the activations were consumed: a second backward says so
        else:                                    # one more term in the loss: not the two-node graph
            loss = loss + 0.0 * pred.sum()
            assert not ctrain._two_node_backward(loss, torch.ones((), device="cuda:0"))
            ctrain.backward(loss)
        return opt.flat_grad.clone()

    for which in (0, 1):
        ref = grads(which, "engine")
        assert ref.abs().max().item() > 0
        assert torch.equal(grads(which, "helper"), ref)
        assert torch.equal(grads(which, "other"), ref)
    m = _model(hp, sd, 0).train()                # no FlatAdam: the parameters' .grad come from the engine
    pred, true = m(gu.clone_batch(b).to("cuda:0"))
    loss = ctrain.compute_loss(pred, true)[0]
    assert not ctrain._two_node_backward(loss, torch.ones((), device="cuda:0"))
    ctrain.backward(loss)
    assert all(p.grad is not None for p in m.parameters())


def test_bf16_mode_on_adp_config2_fixture():
    """gemm_precision = 2 on the configs[1]-shaped golden fixture: bf16-level agreement, finite, SPD outputs."""
    z, hp, b, sd = gu.load("config2")
    m = _model(hp, sd, 2).train()
    bb = gu.clone_batch(b).to("cuda:0")
    pred, true = m(bb)
    assert rel_err(pred, torch.from_numpy(z["train_pred_f64"])) < BF16_PRED_TOL
    assert torch.linalg.eigvalsh(pred.detach().double().cpu()).min().item() > 0
    (pred - true).abs().mean().backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


def test_bf16_storage_on_jarvis_shapes_and_adp_fixture():
    """BASELINE configs[2] as SURVEY.md 8d defines it -- bf16 STORAGE, fp32 accumulate (CartNet.half_storage at
    gemm_precision 2: pre / gs / dpre of every layer live in HBM as bf16): same bf16 tolerances against the fp64 oracle
    as the fp32-storage bf16 mode, bitwise reproducible, a smaller workspace; the configs[1]-shaped golden fixture stays
    finite and SPD; refused at the other precisions."""
    from cartnet_amd import lib as _lib
    import ctypes
    b, hp, sd = _jarvis_case()
    names = None
    outs = []
    for half in (False, True):
        m = _model(hp, sd, 2).train()
        m.half_storage = half
        bb = gu.clone_batch(b).to("cuda:0")
        pred, true = m(bb)
        (pred - true).abs().mean().backward()
        names = [k for k, _ in m.named_parameters()]
        outs.append((pred.detach().clone(), {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}))
        if half:                       # bitwise reproducible
            m.zero_grad()
            bb2 = gu.clone_batch(b).to("cuda:0")
            pred2, true2 = m(bb2)
            (pred2 - true2).abs().mean().backward()
            assert torch.equal(pred2, pred)
            assert all(torch.equal(p.grad.double().cpu(), outs[-1][1][k]) for k, p in m.named_parameters())
    ref, gref = _oracle_run(b, hp, sd, set(names))
    gmax = max(v.abs().max().item() for v in gref.values())
    for pred, got in outs:
        gerr = max((got[k].reshape(gref[k].shape) - gref[k]).abs().max().item() for k in names) / gmax
        assert rel_err(pred, ref) < BF16_PRED_TOL and gerr < BF16_GRAD_TOL, (rel_err(pred, ref), gerr)
    assert not torch.equal(outs[0][0], outs[1][0]), "half storage must change the rounding somewhere"
    # workspace: three [E, 2D] tensors per layer at half size
    m = _model(hp, sd, 2)
    sizes = []
    for half in (False, True):
        m.half_storage = half
        md = m._model_desc(dict(m.named_parameters()))
        sizes.append(int(_lib.load().cartnet_workspace_bytes(ctypes.byref(md), int(b.x.shape[0]), int(b.edge_index.shape[1]),
                                                             int(b.num_graphs), 0, 1)))
    E, D, L = int(b.edge_index.shape[1]), 256, 4
    assert sizes[0] - sizes[1] >= (2 * L + 2) * E * 2 * D * 2 - 4096 * 16
    # ADP fixture
    z, hp2, b2, sd2 = gu.load("config2")
    m2 = _model(hp2, sd2, 2).train()
    m2.half_storage = True
    bb = gu.clone_batch(b2).to("cuda:0")
    pred, true = m2(bb)
    assert rel_err(pred, torch.from_numpy(z["train_pred_f64"])) < BF16_PRED_TOL
    assert torch.linalg.eigvalsh(pred.detach().double().cpu()).min().item() > 0
    (pred - true).abs().mean().backward()
    assert all(torch.isfinite(p.grad).all() for p in m2.parameters())
    m2.gemm_precision = 1
    with pytest.raises(ValueError, match="half_storage"):
        m2(gu.clone_batch(b2).to("cuda:0"))


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("variant", ["invariant", "no_temperature", "no_envelope"])
def test_model_variants_at_width_256_against_oracle(variant, precision):
    """The ablation switches of the reference (cartnet.py:41-46) at the width that takes the DMA-fed kernels: the
    invariant encoder has K = 64 for the first edge Linear (no padding), the others K = 67 -> 80."""
    from cartnet_amd.data import Batch
    from cartnet_amd.model import make_state_dict
    from cartnet_amd.synthetic import make_crystal
    hp = dict(dim_in=256, dim_rbf=64, num_layers=2, radius=5.0, invariant=variant == "invariant",
              temperature=variant != "no_temperature", use_envelope=variant != "no_envelope", atom_types=True,
              cholesky=True)
    b = Batch.from_data_list([make_crystal(300 + i, n) for i, n in enumerate((17, 40, 9))])
    sd = make_state_dict(256, 64, 2, seed=11, invariant=hp["invariant"], temperature=hp["temperature"])
    m = _model(hp, sd, precision).train()
    bb = gu.clone_batch(b).to("cuda:0")
    pred, true = m(bb)
    (pred - true).abs().mean().backward()
    names = set(k for k, _ in m.named_parameters())
    ref, gref = _oracle_run(b, hp, sd, names)
    assert rel_err(pred, ref) < PRED_TOL
    _check_grads({k: p.grad for k, p in m.named_parameters()}, gref, variant)


@pytest.mark.parametrize("precision", [0, 1])
def test_width_512_against_oracle(precision):
    """dim_in = 512: two 256-column tiles per layer GEMM, K = 512 / 1024 pipelines, the folded K-segment form does not
    apply (N != 256) and the segment form must take over."""
    from cartnet_amd.data import Batch
    from cartnet_amd.model import make_state_dict
    from cartnet_amd.synthetic import make_crystal
    hp = dict(dim_in=512, dim_rbf=64, num_layers=1, radius=5.0, invariant=False, temperature=True, use_envelope=True,
              atom_types=True, cholesky=True)
    b = Batch.from_data_list([make_crystal(330 + i, n) for i, n in enumerate((21, 33))])
    sd = make_state_dict(512, 64, 1, seed=12)
    m = _model(hp, sd, precision).train()
    bb = gu.clone_batch(b).to("cuda:0")
    pred, true = m(bb)
    (pred - true).abs().mean().backward()
    names = set(k for k, _ in m.named_parameters())
    ref, gref = _oracle_run(b, hp, sd, names)
    assert rel_err(pred, ref) < PRED_TOL
    _check_grads({k: p.grad for k, p in m.named_parameters()}, gref, "width512")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 3), (517, 3, 3), (12416, 3, 3), (64,)])
def test_fused_loss_matches_torch(shape):
    """compute_loss on device tensors = one launch for (MAE, MSE) and one for the gradient (cartnet_loss_fwd / _bwd):
    values against torch in fp64, gradients of either loss and of a mix of both, sign(0) = 0, bitwise repeatable."""
    from cartnet_amd.train import compute_loss
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(*shape, generator=g)
    t0 = torch.randn(*shape, generator=g)
    p0.view(-1)[0] = t0.view(-1)[0]                      # one exact zero difference
    for wa, ws in ((1.0, 0.0), (0.0, 1.0), (0.3, 1.7)):
        p = p0.cuda().requires_grad_(True)
        t = t0.cuda()
        mae, mse = compute_loss(p, t)
        (wa * mae + ws * mse).backward()
        pr = p0.double().requires_grad_(True)
        d = pr - t0.double()
        mae_r, mse_r = d.abs().mean(), (d * d).mean()
        (wa * mae_r + ws * mse_r).backward()
        assert abs(mae.item() - mae_r.item()) <= 2e-7 * abs(mae_r.item())
        assert abs(mse.item() - mse_r.item()) <= 2e-7 * abs(mse_r.item())
        gr = pr.grad
        assert (p.grad.double().cpu() - gr).abs().max().item() <= 1e-6 * gr.abs().max().item()
        assert p.grad.view(-1)[0].item() == (0.0 if ws == 0.0 else p.grad.view(-1)[0].item())
    a = compute_loss(p0.cuda(), t0.cuda())
    b = compute_loss(p0.cuda(), t0.cuda())
    assert a[0].item() == b[0].item() and a[1].item() == b[1].item()

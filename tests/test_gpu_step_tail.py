"""The kernels after the last GEMM of a training step, each against fp64 at the sizes where it changes code path:
cartnet_mask_index, the Cholesky and scalar heads, the fused loss and cartnet_adam_step (through cartnet_amd.ops,
cartnet_amd.lib and cartnet_amd.train).

Every figure is printed next to its bound and all of them are asserted at the end of a test (``_Figures``).  Heads:
max|delta| <= TOL * max|ref| per matrix entry / per weight row / per bias entry, not once over the tensor, so that a
large entry cannot hide a small one.  Adam: element by element with B = 2e-6 on the scale of the element's own update
(about ten fp32 roundings are 6e-7; an eps on the wrong side of the bias correction gives about 0.8).
"""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
ADAM_B = 2e-6
LOSS_VAL = 2e-7      # relative bound on MAE / MSE (the one of test_fused_loss_matches_torch)
LOSS_GRAD = 1e-6     # element-wise bound on the loss gradient, relative to its maximum


@pytest.fixture(scope="module")
def ops():
    from cartnet_amd import ops as _ops
    from cartnet_amd import lib
    lib.load()
    return _ops


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev())


def f32(x):
    """A Python float as the C entry point receives it."""
    return float(np.float32(x))


class _Figures:
    """Every figure of a test is printed; check() then asserts all of them, so one run shows every miss."""

    def __init__(self):
        self.bad = []

    def add(self, what, err, bound):
        print(f"{what}: {err:.3g} (bound {bound:g})")
        if not err < bound:
            self.bad.append((what, err, bound))

    def exact(self, what, ok):
        print(f"{what}: {'ok' if ok else 'MISS'} (exact)")
        if not ok:
            self.bad.append((what, "not exact"))

    def check(self):
        assert not self.bad, self.bad


# --------------------------------------------------------------------------------------------------- Adam
ADAM_SCHEDULE = [(1, 1e-3, 0.95, 1.0), (2, 7e-4, 0.9, 0.25), (3, 1e-3, 0.85, 1.0), (1000, 1e-3, 0.9, 0.5),
                 (100000, 4e-9, 0.95, 1.0)]      # (step, lr, beta1, grad_scale): OneCycle moves lr and beta1 every step
ADAM_BETA2, ADAM_EPS = 0.999, 1e-8
ADAM_GRID = 4096 * 256                           # threads of the largest launch: one trip of the grid-stride loop


def _wide_gradient(n, seed):
    """sign * 10**U(-10, 2), every 97th element exactly 0 (the same elements at every step, so their state stays 0)."""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 12.0 - 10.0)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    grad = (sign * mag).float()
    grad[96::97] = 0.0
    return grad


def _adam_case(ops, n, p_start, figs, tag):
    from oracle import train_ref
    gen = torch.Generator().manual_seed(n)
    p0 = torch.zeros(n) if p_start == "zero" else torch.randn(n, generator=gen)
    p, m, v = p0.to(dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    b2, eps = f32(ADAM_BETA2), f32(ADAM_EPS)
    for k, (step, lr, b1, gs) in enumerate(ADAM_SCHEDULE):
        lr, b1, gs = f32(lr), f32(b1), f32(gs)
        grad = _wide_gradient(n, seed=1000 * k + n % 997)
        # the reference starts every step from the GPU's own fp32 state: each step is judged on its own
        p_old, m_old, v_old = p.double().cpu(), m.double().cpu(), v.double().cpu()
        g64 = grad.double() * gs
        p_ref, m_ref, v_ref = p_old.clone(), m_old.clone(), v_old.clone()
        train_ref.adam_step(p_ref, g64, m_ref, v_ref, step, lr, (b1, b2), eps)
        ops.adam_step(p, grad.to(dev()), m, v, lr, b1, b2, eps, step, gs)
        pg, mg, vg = p.double().cpu(), m.double().cpu(), v.double().cpu()
        t = f"{tag} step {step}"
        figs.exact(f"{t}: p, m, v finite", bool(torch.isfinite(pg).all() and torch.isfinite(mg).all()
                                                and torch.isfinite(vg).all()))
        s_m = m_old.abs() + g64.abs()
        live = s_m > 0
        still = (g64 == 0) & (m_old == 0) & (v_old == 0)
        assert int(still.sum()) == n // 97 and bool((live | still).all())
        figs.exact(f"{t}: zero gradient on zero state leaves p, m, v alone",
                   bool(torch.equal(pg[still], p_old[still]) and (mg[still] == 0).all() and (vg[still] == 0).all()))
        if not bool(live.any()):
            continue
        figs.add(f"{t}: max |m - ref| / (|m_prev| + |g|)", ((mg - m_ref).abs()[live] / s_m[live]).max().item(), ADAM_B)
        big = v_ref > 1e-30
        assert bool((big | ((g64 == 0) & (v_old == 0))).all())
        figs.add(f"{t}: max |v - ref| / v_ref", ((vg - v_ref).abs()[big] / v_ref[big]).max().item(), ADAM_B)
        figs.exact(f"{t}: v == 0 where g and v_prev are 0", bool((vg[(g64 == 0) & (v_old == 0)] == 0).all()))
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        den_ref = v_ref.sqrt() / math.sqrt(bc2) + eps
        scale = (lr / bc1) * s_m / den_ref
        excess = ((pg - p_old) - (p_ref - p_old)).abs() - 2.0 ** -24 * pg.abs()     # less the rounding of the store
        figs.add(f"{t}: max (|dp - dp_ref| - 2^-24 |p|) / (lr/bc1 (|m_prev| + |g|) / den)",
                 (excess[live] / scale[live]).max().item(), ADAM_B)
        if n > ADAM_GRID:                         # the elements of the loop's second trip, on their own
            tail = torch.zeros(n, dtype=torch.bool)
            tail[ADAM_GRID:] = True
            tail &= live
            figs.add(f"{t}: the same over the {n - ADAM_GRID} elements of the second trip",
                     (excess[tail] / scale[tail]).max().item(), ADAM_B)
            figs.add(f"{t}: m over the second trip", ((mg - m_ref).abs()[tail] / s_m[tail]).max().item(), ADAM_B)
            figs.add(f"{t}: v over the second trip",
                     ((vg - v_ref).abs()[tail & big] / v_ref[tail & big]).max().item(), ADAM_B)


@pytest.mark.parametrize("p_start", ["zero", "randn"])
@pytest.mark.parametrize("n", [1, 255, 257, 20011])
def test_adam_step_element_by_element(ops, n, p_start):
    """cartnet_adam_step against oracle.train_ref.adam_step in fp64 with the hyper-parameters rounded to fp32 as the C
    entry point receives them; gradients over twelve decades (eps is invisible at |g| ~ 1), lr, beta1 and grad_scale
    changing from step to step, and step numbers up to 1e5."""
    figs = _Figures()
    _adam_case(ops, n, p_start, figs, f"n={n} p0={p_start}")
    figs.check()


def test_adam_step_second_trip_of_the_grid_stride_loop(ops):
    """n = 4096 * 256 + 257: the smallest size at which the capped grid goes round its loop twice."""
    figs = _Figures()
    _adam_case(ops, ADAM_GRID + 257, "randn", figs, f"n={ADAM_GRID + 257}")
    figs.check()


def test_flat_adam_grad_scale_is_the_scaled_gradient_bitwise():
    """FlatAdam.step(grad_scale=0.25) on g and step() on 0.25 * g: scaling by a power of two is exact, so parameters
    and both moments agree bit for bit, also after lr and beta1 have moved."""
    from cartnet_amd.optim import FlatAdam
    torch.manual_seed(3)
    nets = [torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Linear(53, 5)).to(dev()) for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    opts = [FlatAdam(net, lr=1e-3, betas=(0.95, 0.999)) for net in nets]
    n = opts[0].flat_param.numel()
    assert n == 37 * 53 + 53 + 53 * 5 + 5 and torch.equal(opts[0].flat_param, opts[1].flat_param)
    start = opts[0].flat_param.clone()
    for k, (lr, b1) in enumerate([(1e-3, 0.95), (7e-4, 0.9), (4e-5, 0.85)]):
        grad = _wide_gradient(n, seed=50 + k).to(dev())
        for o in opts:
            o.zero_grad()
            o.set_lr(lr)
            o.set_beta1(b1)
        opts[0].flat_grad.copy_(grad)
        opts[1].flat_grad.copy_(grad * 0.25)
        opts[0].step(grad_scale=0.25)
        opts[1].step()
        for name in ("flat_param", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(opts[0], name), getattr(opts[1], name)), (k, name)
        assert torch.equal(nets[0][0].weight, nets[1][0].weight)       # the parameters are views of the flat buffer
    assert not torch.equal(opts[0].flat_param, start)                  # (and they did move)


# --------------------------------------------------------------------------------------------------- mask_index
def _mask(kind, N, seed):
    if kind == "all":
        return torch.ones(N, dtype=torch.bool)
    if kind == "none":
        return torch.zeros(N, dtype=torch.bool)
    if kind == "one":
        m = torch.zeros(N, dtype=torch.bool)
        m[(2 * N) // 3] = True
        return m
    return torch.rand(N, generator=torch.Generator().manual_seed(seed)) < 0.55


def _mask_index(ops, mask):
    N = mask.numel()
    idx = torch.full((N,), -7, dtype=torch.int32, device=dev())
    cnt = torch.full((1,), -7, dtype=torch.int32, device=dev())
    ops.mask_index(mask.to(dev()), idx, cnt)
    return idx, cnt


@pytest.mark.parametrize("kind", ["all", "none", "random"])
@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 5000])
def test_mask_index_across_its_passes(ops, N, kind):
    """One workgroup ranks 1024 atoms per pass and carries the count over: exact ranks and count on both sides of a
    pass boundary and over several passes."""
    mask = _mask(kind, N, seed=N)
    idx, cnt = _mask_index(ops, mask)
    M = int(mask.sum())
    exp = torch.full((N,), -1, dtype=torch.int64)
    exp[mask] = torch.arange(M)
    assert int(cnt.item()) == M
    assert torch.equal(idx.cpu().long(), exp)


# --------------------------------------------------------------------------------------------------- Cholesky head
def _head_sd(H, w64, b64):
    # oracle head = Linear(D->H) [identity here] -> SiLU -> Linear(H->out)
    return {"head.MLP.0.weight": torch.eye(H, dtype=torch.float64), "head.MLP.0.bias": torch.zeros(H, dtype=torch.float64),
            "head.MLP.2.weight": w64, "head.MLP.2.bias": b64}


def _cholesky_case(ops, figs, tag, hid, W2, b2, mask, saturated=False):
    from oracle import cartnet_ref as orc
    import torch.nn.functional as F
    N, H = hid.shape
    idx, cnt = _mask_index(ops, mask)
    M = int(mask.sum())
    assert int(cnt.item()) == M and M >= 1
    p6 = torch.full((M, 6), float("nan"), device=dev())
    pred = torch.full((M, 3, 3), float("nan"), device=dev())
    ops.cholesky_head_fwd(hid, idx, W2, b2, p6, pred)
    h64 = hid.double().cpu().requires_grad_(True)
    w64, b64 = W2.double().cpu().requires_grad_(True), b2.double().cpu().requires_grad_(True)
    ref = orc.cholesky_head(_head_sd(H, w64, b64), h64, mask)
    with torch.no_grad():
        p_ref = F.linear(F.silu(h64[mask]), w64, b64)              # the reference's pre-activations
    if saturated:                                                  # both branches of softplus_f / dsoftplus_f, every atom
        assert float(p_ref[:, 0].min()) > 20.0 and float(p_ref[:, 1].max()) < -20.0
    for r in range(6):
        figs.add(f"{tag}: p6[:, {r}]", rel_err(p6[:, r], p_ref[:, r]), TOL)
    for i in range(3):
        for j in range(3):
            figs.add(f"{tag}: pred[:, {i}, {j}]", rel_err(pred[:, i, j], ref[:, i, j]), TOL)
    # (a seed with a mean: the six sums over the atoms that make db2 then do not cancel, and each is judged by itself)
    dpred = rnd(M, 3, 3, seed=4) + 1.0
    (ref * dpred.double().cpu()).sum().backward()
    dhid = torch.full((N, H), float("nan"), device=dev())
    nparts = ops.node_nparts(N)
    parts = torch.full((nparts * (7 * H + 8),), float("nan"), device=dev())
    ops.cholesky_head_bwd(hid, idx, W2, p6, dpred.contiguous(), dhid, parts)
    figs.add(f"{tag}: dhid", rel_err(dhid, h64.grad), TOL)
    figs.exact(f"{tag}: dhid rows of unmasked atoms are zero", bool((dhid.cpu()[~mask] == 0).all()))
    tot = parts.view(nparts, 7 * H + 8).double().sum(0).cpu()
    for r in range(6):
        figs.add(f"{tag}: dW2[{r}] (max |ref| {w64.grad[r].abs().max().item():.3g})",
                 rel_err(tot[r * H:(r + 1) * H], w64.grad[r]), TOL)
        figs.add(f"{tag}: db2[{r}] (ref {b64.grad[r].item():.3g})", rel_err(tot[6 * H + r:6 * H + r + 1], b64.grad[r:r + 1]),
                 TOL)
    figs.add(f"{tag}: column sums of dhid", rel_err(tot[6 * H + 8:], h64.grad.sum(0)), TOL)


# (N, H): one atom; H no multiple of 64... 64 itself with several atoms per backward wave (N > 1024); four and eight
# columns per lane (HEAD_MAX_H = 512); the forward's stride (N > 8192)
@pytest.mark.parametrize("kind", ["random", "all", "one"])
@pytest.mark.parametrize("N,H", [(1, 8), (1025, 64), (1300, 256), (4100, 512), (8200, 128)])
def test_cholesky_head_per_entry_at_full_width_and_depth(ops, N, H, kind):
    figs = _Figures()
    hid, W2, b2 = rnd(N, H, seed=1), rnd(6, H, seed=2, scale=0.3), rnd(6, seed=3)
    mask = _mask(kind, N, seed=H)
    if N == 1:
        mask[0] = True                        # (the only atom is kept under every mask)
    elif kind == "one":
        # With one atom kept every column of p6 is judged against that atom's own value, a sum of H products that can
        # cancel to any fraction of its terms (fp32 can only promise TOL of the terms).  So keep the atom whose six
        # pre-activations, in the fp64 reference, are farthest from zero: each is then a scale for itself.
        p_all = torch.nn.functional.linear(torch.nn.functional.silu(hid.double().cpu()), W2.double().cpu(), b2.double().cpu())
        mask = torch.zeros(N, dtype=torch.bool)
        mask[int(p_all.abs().min(dim=1).values.argmax())] = True
    _cholesky_case(ops, figs, f"N={N} H={H} mask={kind}", hid, W2, b2, mask)
    figs.check()


def test_cholesky_head_saturated_softplus(ops):
    """p0 > 20 and p1 < -20 for every atom: softplus_f / dsoftplus_f on their ``x > 20`` branch and far on the negative
    side, where d1 = softplus(p1) and the gradient of row 1 of W2 are about 1e-13 -- judged against their own size."""
    N, H = 1300, 256
    figs = _Figures()
    b2 = torch.tensor([25.0, -30.0, 0.3, -0.7, 0.4, 1.1], device=dev())
    _cholesky_case(ops, figs, f"N={N} H={H} saturated", rnd(N, H, seed=1), rnd(6, H, seed=2, scale=0.01), b2,
                   _mask("random", N, seed=H), saturated=True)
    figs.check()


# --------------------------------------------------------------------------------------------------- scalar head
def test_scalar_head_refuses_a_width_that_is_no_multiple_of_four(ops):
    """The forward reads four columns at a time: H = 6 would read past w2 and into the next atom's row.  The entry point
    refuses it before any launch (``out`` keeps its fill)."""
    from cartnet_amd.lib import CartnetHipError
    H, Bg = 6, 2
    ptr = torch.tensor([0, 2, 5], dtype=torch.int64, device=dev())
    out = torch.full((Bg,), 3.0, device=dev())
    with pytest.raises(CartnetHipError, match="multiple of 4"):
        ops.scalar_head_fwd(rnd(5, H, seed=1), rnd(1, H, seed=2), rnd(1, seed=3), ptr, out)
    assert bool((out == 3.0).all())


@pytest.mark.parametrize("H", [4, 32, 128, 132, 256, 512])
def test_scalar_head_at_every_lane_pattern(ops, H):
    """H = 4: one lane of each half-wave loads; 128: all of them, one trip; 132: a single lane takes the second trip;
    256 / 512: two and four trips (the backward's j >= 1).  Crystals of 1 atom (half the wave adds nothing), 2, 3, 64
    and 301 atoms, then random 1..40 up to N >= 1100, so that the backward's waves take more than one atom."""
    from oracle import cartnet_ref as orc
    figs = _Figures()
    g = torch.Generator().manual_seed(H)
    sizes = [1, 2, 3, 64, 301]
    while sum(sizes) < 1100:
        sizes.append(int(torch.randint(1, 41, (1,), generator=g)))
    sizes = torch.tensor(sizes)
    Bg = sizes.numel()
    ptr = torch.zeros(Bg + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(sizes, 0)
    N = int(ptr[-1])
    assert N > 1024
    batch = torch.repeat_interleave(torch.arange(Bg), sizes)
    hid, w2, b2 = rnd(N, H, seed=2), rnd(1, H, seed=3), rnd(1, seed=4)
    out = torch.full((Bg,), float("nan"), device=dev())
    ops.scalar_head_fwd(hid, w2, b2, ptr.to(dev()), out)
    h64 = hid.double().cpu().requires_grad_(True)
    w64, b64 = w2.double().cpu().requires_grad_(True), b2.double().cpu().requires_grad_(True)
    ref = orc.scalar_head(_head_sd(H, w64, b64), h64, batch, Bg)
    tag = f"H={H} N={N} Bg={Bg}"
    figs.add(f"{tag}: out", rel_err(out, ref), TOL)
    dout = rnd(Bg, seed=5) + 1.0
    (ref * dout.double().cpu()).sum().backward()
    dhid = torch.full((N, H), float("nan"), device=dev())
    nparts = ops.node_nparts(N)
    parts = torch.full((nparts * (2 * H + 8),), float("nan"), device=dev())
    ops.scalar_head_bwd(hid, w2, ptr.to(dev()), batch.to(dev()), dout, dhid, parts)
    figs.add(f"{tag}: dhid", rel_err(dhid, h64.grad), TOL)
    tot = parts.view(nparts, 2 * H + 8).double().sum(0).cpu()
    figs.add(f"{tag}: dw2", rel_err(tot[:H], w64.grad.view(-1)), TOL)
    figs.add(f"{tag}: db2", rel_err(tot[H:H + 1], b64.grad), TOL)
    figs.add(f"{tag}: column sums of dhid", rel_err(tot[H + 8:], h64.grad.sum(0)), TOL)
    figs.check()


# --------------------------------------------------------------------------------------------------- fused loss
def _loss_inputs(n, scale, seed):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g) * scale
    t0 = torch.randn(n, generator=g) * scale
    ties = sorted({0, n // 2, n - 1}) if n >= 8 else []
    for i in ties:
        p0[i] = t0[i]
    return p0, t0, ties


def _loss_bwd(p, t, ga, gs):
    """cartnet_loss_bwd with the upstream gradients as device scalars (None = absent)."""
    from cartnet_amd import lib as _l
    dpred = torch.full_like(p, float("nan"))
    _l.check(_l.load().cartnet_loss_bwd(p.data_ptr(), t.data_ptr(), p.numel(), _l.ptr(ga), _l.ptr(gs), dpred.data_ptr(),
                                        _l.stream_ptr()), "cartnet_loss_bwd")
    return dpred


@pytest.mark.parametrize("scale", [0.02, 1.0])
@pytest.mark.parametrize("n", [1, 4096, 4097, 262144, 262145, 1000003])
def test_fused_loss_at_the_slice_boundaries(n, scale):
    """One slice up to 4096 elements, two from 4097, the cap of 64 slices at 262144 and slices longer than 4096 elements
    beyond it: MAE and MSE against fp64, the gradient kernel element by element, ties exactly 0, all bitwise repeatable."""
    from cartnet_amd.train import compute_loss
    from cartnet_amd import lib as _l
    figs = _Figures()
    assert _l.load().cartnet_loss_nparts(n) == min(64, (n + 4095) // 4096)
    p0, t0, ties = _loss_inputs(n, scale, seed=n % 1000 + 7)
    p, t = p0.to(dev()), t0.to(dev())
    d = p0.double() - t0.double()
    mae_r, mse_r = d.abs().mean().item(), (d * d).mean().item()
    mae, mse = compute_loss(p, t)
    tag = f"n={n} scale={scale}"
    figs.add(f"{tag}: MAE", abs(mae.item() - mae_r) / mae_r, LOSS_VAL)
    figs.add(f"{tag}: MSE", abs(mse.item() - mse_r) / mse_r, LOSS_VAL)
    again = compute_loss(p, t)
    figs.exact(f"{tag}: values repeat bitwise", mae.item() == again[0].item() and mse.item() == again[1].item())
    for wa, ws in ((0.7, None), (None, 1.3), (0.3, 1.7)):
        ga = torch.tensor([wa], device=dev()) if wa is not None else None
        gs = torch.tensor([ws], device=dev()) if ws is not None else None
        got = _loss_bwd(p, t, ga, gs)
        ref = (f32(wa) if wa is not None else 0.0) * torch.sign(d) / n + (f32(ws) if ws is not None else 0.0) * 2.0 * d / n
        figs.add(f"{tag}: gradient for (g_mae, g_mse) = ({wa}, {ws})",
                 (got.double().cpu() - ref).abs().max().item() / ref.abs().max().item(), LOSS_GRAD)
        if ws is None and ties:
            figs.exact(f"{tag}: ties have MAE gradient 0", bool((got.cpu()[ties] == 0).all()))
        figs.exact(f"{tag}: gradient repeats bitwise", bool(torch.equal(got, _loss_bwd(p, t, ga, gs))))
    figs.check()


@pytest.mark.parametrize("n", [1, 64, 4096, 4097])
def test_fused_loss_unit_gradients_are_the_backward_kernel_bitwise(n):
    """With ``requires_grad`` and n <= 4096 the forward launch (cartnet_loss_fwd_unit) also writes both gradients for a
    seed of 1, and cartnet_amd.train.backward hands them out in place of a cartnet_loss_bwd launch: bitwise the same
    gradient, bitwise the same two losses as the route without ``requires_grad``.  n = 4097 takes the two-launch route."""
    from cartnet_amd import train
    figs = _Figures()
    p0, t0, ties = _loss_inputs(n, 0.02, seed=n + 11)
    t = t0.to(dev())
    one = torch.ones(1, device=dev())
    plain = train.compute_loss(p0.to(dev()), t)
    d = p0.double() - t0.double()
    for k, name in ((0, "MAE"), (1, "MSE")):
        p = p0.to(dev()).requires_grad_(True)
        losses = train.compute_loss(p, t)
        fn = losses[k].grad_fn
        tag = f"n={n} {name}"
        figs.exact(f"{tag}: the one-launch route is taken up to 4096 elements only", (fn.unit is not None) == (n <= 4096))
        figs.exact(f"{tag}: both losses equal the route without requires_grad bitwise",
                   losses[0].item() == plain[0].item() and losses[1].item() == plain[1].item())
        want = _loss_bwd(p.detach(), t, one if k == 0 else None, one if k == 1 else None)
        if fn.unit is not None:
            figs.exact(f"{tag}: unit gradients as written by the forward launch",
                       bool(torch.equal(fn.unit[k * n:(k + 1) * n], want)))
        train.backward(losses[k])
        figs.exact(f"{tag}: gradient from train.backward equals cartnet_loss_bwd for a seed of 1 bitwise",
                   bool(torch.equal(p.grad, want)))
        ref = torch.sign(d) / n if k == 0 else 2.0 * d / n
        figs.add(f"{tag}: gradient against fp64", (p.grad.double().cpu() - ref).abs().max().item() / ref.abs().max().item(),
                 LOSS_GRAD)
        if k == 0 and ties:
            figs.exact(f"{tag}: ties have gradient 0", bool((p.grad.cpu()[ties] == 0).all()))
        if fn.unit is not None:
            # that train.backward really hands out the forward launch's buffer: mark it in a second forward
            p2 = p0.to(dev()).requires_grad_(True)
            l2 = train.compute_loss(p2, t)
            l2[k].grad_fn.unit.fill_(7.0)
            train.backward(l2[k])
            figs.exact(f"{tag}: train.backward returns the unit buffer", bool((p2.grad == 7.0).all()))
    figs.check()

"""Kernel-level fp64 parity for the entry points that only the iComformer / eComformer path uses (BASELINE configs[4]).

Whole-model parity measures max|delta| / max|ref| and cannot see a large relative error in a small element.  Here each
kernel is compared with an fp64 evaluation of the same arithmetic (the oracle's functions where they exist), per element
where the arithmetic admits a per-element bound, at the shapes where the kernels change form: the vector and scalar
paths, grid-stride loops that run more than one trip, block caps, a second 256-column chunk with one active lane, empty
inputs, padded and misaligned views.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import ecomformer_ref as ecr
from oracle import icomformer_ref as icr

pytestmark = pytest.mark.gpu

TOL = 1e-5
U = 2.0 ** -24


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
    return torch.randn(*shape, generator=g) * scale


def within(got, want, bound):
    """|got - want| <= bound element-wise (fp64 on the CPU); returns (ok, worst ratio)."""
    err = (got.detach().double().cpu() - want).abs()
    ok = bool((err <= bound).all())
    return ok, float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0


# ------------------------------------------------------------------------------------------------ rbf_expand
def rbf_vector_form(bins):
    q = bins // 4
    return bins % 4 == 0 and 1 <= q <= 256 and 256 % q == 0


def rbf_big_n(bins):
    """Rows enough for the grid-stride loop to run more than one trip: the vector form caps its grid at 16,384 blocks of
    256 / (bins / 4) rows, the scalar form at 8,192 blocks of 256 elements."""
    if rbf_vector_form(bins):
        return 16384 * (256 // (bins // 4)) + 777
    return 8192 * 256 // bins + 777


def run_rbf(ops, n, bins, layout, seed):
    """out[r, k] = exp(-gamma (v[r] - c[k])^2) through cartnet_rbf_expand; returns (out view, its buffer, v, c, gamma,
    the buffer's columns that must stay untouched)."""
    v = (torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 10.0 - 1.0)
    c = torch.linspace(0.0, 8.0, bins)
    gamma = float(torch.tensor(max(bins - 1, 1) / 8.0, dtype=torch.float32))
    cbuf = torch.zeros(bins + 4)
    if layout == "misaligned_centers":      # 4 bytes past a 16-byte boundary: the scalar form
        cbuf[1:1 + bins] = c
        cd = cbuf.to(dev())[1:1 + bins]
    else:
        cd = c.to(dev())
    if layout == "padded":                  # ldo > bins, still 16-byte rows: the vector form where bins allows it
        buf = torch.full((n, bins + 8), 7.0, device=dev())
        out, keep = buf[:, :bins], (slice(None), slice(bins, None))
    elif layout == "misaligned_out":        # a column view offset by one: the scalar form
        buf = torch.full((n, bins + 4), 7.0, device=dev())
        out, keep = buf[:, 1:1 + bins], (slice(None), [0] + list(range(1 + bins, bins + 4)))
    else:
        buf = torch.full((n, bins), 7.0, device=dev())
        out, keep = buf, None
    ops.rbf_expand(v.to(dev()), cd, gamma, out)
    return out, buf, v, c, gamma, keep


def rbf_check(out, v, c, gamma):
    """Per element |out - ref| <= (2e-6 + 5 u a) ref + 1e-30, a = gamma (v - c)^2 in fp64 on the fp32 inputs: the fp32
    argument takes three roundings (v - c, its square, the product with gamma: 4 u a with the square's doubling) and
    __expf a fourth (a log2(e) rounded to fp32: u a), each a relative error of a that exp turns into one of the result;
    2e-6 covers the exp instruction and small a."""
    d = v.double().unsqueeze(1) - c.double()
    arg = gamma * d * d
    ref = torch.exp(-arg)
    bound = (2e-6 + 5 * U * arg) * ref + 1e-30
    return within(out, ref, bound)


@pytest.mark.parametrize("bins", [1, 3, 4, 12, 64, 256, 1024, 1028])
@pytest.mark.parametrize("size", ["one", "some", "grid_stride"])
def test_rbf_expand_against_fp64(ops, bins, size):
    """Both kernels (vector form: bins % 4 == 0 and 256 % (bins / 4) == 0; scalar otherwise) per element against fp64."""
    n = {"one": 1, "some": 1001, "grid_stride": rbf_big_n(bins)}[size]
    out, _, v, c, gamma, _ = run_rbf(ops, n, bins, "contiguous", seed=bins)
    ok, worst = rbf_check(out, v, c, gamma)
    print(f"RBF bins={bins} n={n} vector={rbf_vector_form(bins)} worst err / bound {worst:.3f}")
    assert ok, worst


@pytest.mark.parametrize("bins", [4, 12, 64, 256, 1024])
@pytest.mark.parametrize("layout", ["padded", "misaligned_out", "misaligned_centers"])
def test_rbf_expand_views(ops, bins, layout):
    """ldo > bins (columns past bins untouched), a misaligned output view and misaligned centers (both force the scalar
    form) stay within the same per-element bound; where the same kernel runs, the numbers are the contiguous launch's."""
    n = 3001
    out, buf, v, c, gamma, keep = run_rbf(ops, n, bins, layout, seed=7)
    ok, worst = rbf_check(out, v, c, gamma)
    assert ok, (layout, worst)
    if keep is not None:
        assert bool((buf[keep] == 7.0).all()), f"{layout}: rbf_expand wrote outside its columns"
    ref_out, *_ = run_rbf(ops, n, bins, "contiguous", seed=7)
    if layout == "padded" or not rbf_vector_form(bins):
        assert torch.equal(out, ref_out)


# ------------------------------------------------------------------------------------------------ lattice_features
def lattice_inputs(E, Bg, seed):
    g = torch.Generator().manual_seed(seed)
    cell = (torch.eye(3) * (3.0 + torch.rand(Bg, 1, 1, generator=g) * 5.0) + torch.randn(Bg, 3, 3, generator=g)).contiguous()
    nodes = torch.randint(2, 9, (Bg,), generator=g)
    batch = torch.repeat_interleave(torch.arange(Bg), nodes)
    src = torch.randint(0, int(batch.numel()), (E,), generator=g)
    vec = torch.randn(E, 3, generator=g) * 3.0
    if E >= 12:      # edges parallel and antiparallel to a cell vector of their crystal: the cosine clamps at +-1
        k = torch.arange(12)
        vec[k] = cell[batch[src[k]], k % 3] * torch.where(k % 2 == 0, 2.5, -0.75).unsqueeze(1)
    dist = vec.norm(dim=1)
    return cell, batch, src.int(), dist, vec.contiguous()


@pytest.mark.parametrize("E", [0, 1000, 4096 * 256 + 4099])
def test_lattice_features_against_fp64(ops, E):
    """edge_feat = -0.75 / dist, nei_len = -0.75 / |cell_a| (relative 2e-6), nei_cos = clamp(cos(cell_a, dir), -1, 1)
    (absolute 1e-6); several crystals with distinct cells; E = 0 writes nei_len only; E past 4,096 x 256 runs the grid
    stride twice."""
    Bg = 5
    cell, batch, src, dist, vec = lattice_inputs(E, Bg, seed=3)
    ef = torch.full((E,), 7.0, device=dev())
    nl = torch.full((3 * Bg,), 7.0, device=dev())
    nc = torch.full((E, 3), 7.0, device=dev())
    ops.lattice_features(cell.to(dev()), batch.to(dev()), src.to(dev()), dist.to(dev()), vec.to(dev()), ef, nl, nc)
    c64 = cell.double()
    ref_nl = -0.75 / c64.norm(dim=2).reshape(-1)
    ok, worst = within(nl, ref_nl, 2e-6 * ref_nl.abs())
    assert ok, ("nei_len", worst)
    if E == 0:
        return
    ref_ef = -0.75 / dist.double()
    ok, worst = within(ef, ref_ef, 2e-6 * ref_ef.abs())
    assert ok, ("edge_feat", worst)
    gcell = c64[batch[src.long()]]                                           # [E, 3, 3]
    ref_cos = torch.stack([icr.bond_cosine(gcell[:, a], vec.double()) for a in range(3)], dim=1)
    ok, worst = within(nc, ref_cos, torch.full_like(ref_cos, 1e-6))
    assert ok, ("nei_cos", worst)
    k = torch.arange(12)
    par = nc[k, k % 3].cpu()
    assert bool((par.abs() <= 1.0).all()), par
    assert torch.equal(par.sign(), torch.where(k % 2 == 0, 1.0, -1.0))


# ------------------------------------------------------------------------------------------------ softplus update
def update_inputs(N, D, seed):
    o, x, dy = rnd(N, D, seed=seed), rnd(N, D, seed=seed + 1, scale=2.0), rnd(N, D, seed=seed + 2)
    mr = torch.cat([rnd(D, seed=seed + 3, scale=0.1), rnd(D, seed=seed + 4).abs() + 0.5])
    gam, bet = rnd(D, seed=seed + 5), rnd(D, seed=seed + 6)
    return o, x, dy, mr, gam, bet


def update_ref(o, x, mr, gam, bet):
    """fp64: ohat, u = x + bn(o), and the fp32 argument's error scale 4 u (|x| + |ohat gamma| + |beta|)."""
    D = o.shape[1]
    mean, rstd = mr[:D].double(), mr[D:].double()
    ohat = (o.double() - mean) * rstd
    u = x.double() + ohat * gam.double() + bet.double()
    arg_err = 4 * U * (x.double().abs() + (ohat * gam.double()).abs() + bet.double().abs())
    return ohat, u, arg_err


@pytest.mark.parametrize("D", [4, 256, 260, 320])
@pytest.mark.parametrize("big", [False, True])
def test_softplus_update_fwd_against_fp64(ops, D, big):
    """y = softplus(x + bn(o)) per element: the softplus bound 2e-6 + 1e-7 |u| (tests/test_gpu_accuracy.py) plus
    sigmoid(u) times the error of the fp32 argument; N D / 4 below and above the 4,096 x 256 threads of the grid."""
    N = 4096 * 256 * 4 // D + 1001 if big else 777
    o, x, _, mr, gam, bet = update_inputs(N, D, seed=D)
    y = torch.full((N, D), float("nan"), device=dev())
    ops.softplus_update_fwd(o.to(dev()), x.to(dev()), mr.to(dev()), gam.to(dev()), bet.to(dev()), y)
    _, u, arg_err = update_ref(o, x, mr, gam, bet)
    ref = F.softplus(u)
    bound = (2e-6 + 1e-7 * u.abs()) * ref + torch.sigmoid(u) * arg_err + 1e-30
    ok, worst = within(y, ref, bound)
    assert ok, worst


def dsp_ref(u, dy):
    return dy.double() * torch.where(u > 20, torch.ones_like(u), torch.sigmoid(u))


@pytest.mark.parametrize("N", [0, 1, 4097, 20000])
@pytest.mark.parametrize("D", [8, 256, 260])
def test_softplus_update_bwd_stats_against_fp64(ops, N, D):
    """Column partials of du = dy * softplus'(u) and du * ohat (1,024-block cap at N = 4097 and 20000; at D = 260 the
    second 256-chunk has one active lane); their sums within 1e-6 of sum |terms| per column, exact zeros for N = 0."""
    o, x, dy, mr, gam, bet = update_inputs(max(N, 1), D, seed=N + D)
    o, x, dy = o[:N], x[:N], dy[:N]
    npart = ops.segment_nparts(N)
    pa = torch.full((npart * D,), float("nan"), dtype=torch.float64, device=dev())
    pb = torch.full_like(pa, float("nan"))
    d = lambda t: t.contiguous().to(dev())
    ops.softplus_update_bwd_stats(d(o), d(x), d(dy), d(mr), d(gam), d(bet), pa, pb)
    sa, sb = pa.view(npart, D).sum(0).cpu(), pb.view(npart, D).sum(0).cpu()
    if N == 0:
        assert torch.equal(sa, torch.zeros(D, dtype=torch.float64)) and torch.equal(sb, torch.zeros(D, dtype=torch.float64))
        return
    ohat, u, _ = update_ref(o, x, mr, gam, bet)
    du = dsp_ref(u, dy)
    for got, terms in ((sa, du), (sb, du * ohat)):
        assert bool(((got - terms.sum(0)).abs() <= 1e-6 * terms.abs().sum(0)).all())


@pytest.mark.parametrize("N", [0, 1, 4097, 20000])
@pytest.mark.parametrize("D", [8, 256, 260])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("with_add", [False, True])
def test_softplus_update_bwd_apply_against_fp64(ops, N, D, training, with_add):
    """d_o = gamma rstd (du - sums_a / N - ohat sums_b / N) (eval: gamma rstd du) and dx = du (+ dx_add) per element
    against fp64.  du = dy sigmoid(u) carries the softplus' bound 2e-6 + 1e-7 |u| and the fp32 argument's error (through
    sigmoid' / sigmoid = 1 - sigmoid <= 1); each term of the difference 4 u more.  The _sums form is bitwise the same and
    its column sums of d_o are within 1e-6 of sum |d_o|."""
    o, x, dy, mr, gam, bet = update_inputs(max(N, 1), D, seed=3 * N + D)
    o, x, dy = o[:N], x[:N], dy[:N]
    sums = rnd(2 * D, seed=N + 11, scale=max(N, 1) * 0.05)
    add = rnd(max(N, 1), D, seed=N + 12)[:N] if with_add else None
    d = lambda t: t.contiguous().to(dev()) if t is not None else None
    d_o, dx = torch.full((N, D), float("nan"), device=dev()), torch.full((N, D), float("nan"), device=dev())
    ops.softplus_update_bwd_apply(d(o), d(x), d(dy), d(mr), d(gam), d(bet), d(sums), training, d_o, d(add), dx)
    d_o2, dx2 = torch.full_like(d_o, float("nan")), torch.full_like(dx, float("nan"))
    sd = torch.full((D,), 9.0, device=dev())
    ops.softplus_update_bwd_apply(d(o), d(x), d(dy), d(mr), d(gam), d(bet), d(sums), training, d_o2, d(add), dx2, sum_do=sd)
    assert torch.equal(d_o, d_o2) and torch.equal(dx, dx2)
    if N == 0:
        assert torch.equal(sd.cpu(), torch.zeros(D))
        return
    ohat, u, arg_err = update_ref(o, x, mr, gam, bet)
    du = dsp_ref(u, dy)
    e_du = (2e-6 + 1e-7 * u.abs() + arg_err) * du.abs()
    g_r = gam.double() * mr[D:].double()
    inv = 1.0 / N if training else 0.0
    ma, mb = sums[:D].double() * inv, sums[D:].double() * inv
    ref_do = g_r * (du - ma - ohat * mb)
    b_do = g_r.abs() * (e_du + 4 * U * (du.abs() + ma.abs() + (ohat * mb).abs())) + 2 * U * ref_do.abs() + 1e-30
    ok, worst = within(d_o, ref_do, b_do)
    assert ok, ("d_o", worst)
    ref_dx = du + (add.double() if with_add else 0.0)
    ok, worst = within(dx, ref_dx, e_du + U * ref_dx.abs() + 1e-30)
    assert ok, ("dx", worst)
    ref_sum = d_o.double().cpu().sum(0)
    assert bool(((sd.double().cpu() - ref_sum).abs() <= 1e-6 * d_o.double().cpu().abs().sum(0) + U * ref_sum.abs()).all())


# ------------------------------------------------------------------------------------------------ eltwise ops 2 and 3
@pytest.mark.parametrize("rows,cols,pad", [(1, 4, 4), (1001, 260, 8), (33001, 256, 4)])
@pytest.mark.parametrize("op", [2, 3])
def test_eltwise_add_and_scale_are_the_fp32_expression(ops, rows, cols, pad, op):
    """op 2: out = a + b, op 3: out = a * scale on ld > cols views, rows that do not fill the last block (and, at 33,001
    rows of 256, more float4 units than the 8,192-block grid has threads): bitwise the fp32 expression, padding untouched."""
    a, b = rnd(rows, cols + pad, seed=1), rnd(rows, cols + pad + 4, seed=2)
    scale = 0.3183098861837907
    ad, bd = a.to(dev())[:, :cols], b.to(dev())[:, :cols]
    obuf = torch.full((rows, cols + pad), 7.0, device=dev())
    ops.eltwise(op, ad, bd if op == 2 else None, obuf[:, :cols], scale=scale)
    want = a[:, :cols] + b[:, :cols] if op == 2 else a[:, :cols] * torch.tensor(scale, dtype=torch.float32)
    assert torch.equal(obuf[:, :cols].cpu(), want)
    assert bool((obuf[:, cols:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("R", [0, 1, 5, 4097, 200000])
@pytest.mark.parametrize("C", [4, 256, 260])
def test_colsum_and_colstats_against_fp64(ops, R, C):
    """colsum (cartnet_colsum_partial + finaliser) and colstats_partial on ld > C views: fp64 partials, so the sums are
    within (R + 1) 2^-53 sum |x| of fp64 (plus the final fp32 rounding of colsum, and the fp32 square of colstats);
    R = 0 gives exact zeros."""
    buf = rnd(max(R, 1), C + 4, seed=R + C)[:R]
    xd = buf.to(dev())[:, :C]
    x = buf[:, :C].double()
    out = torch.full((C,), 9.0, device=dev())
    ops.colsum(xd, out)
    npart = ops.colstats_nparts(R)
    ps = torch.full((npart * C,), float("nan"), dtype=torch.float64, device=dev())
    pq = torch.full_like(ps, float("nan"))
    ops.colstats_partial(xd, ps, pq)
    s, q = ps.view(npart, C).sum(0).cpu(), pq.view(npart, C).sum(0).cpu()
    if R == 0:
        for t in (out.cpu().double(), s, q):
            assert torch.equal(t, torch.zeros(C, dtype=torch.float64))
        return
    acc = (R + 1) * 2.0 ** -53
    ref, ref_q = x.sum(0), (x * x).sum(0)
    assert bool(((out.cpu().double() - ref).abs() <= U * ref.abs() + acc * x.abs().sum(0)).all())
    assert bool(((s - ref).abs() <= acc * x.abs().sum(0)).all())
    assert bool(((q - ref_q).abs() <= (U + acc) * ref_q).all())


# ------------------------------------------------------------------------------------------------ eComformer equi
NS, NV, H1, NW = 64, 8, 128, 5120


def equi_graph(N=500, E=20000, seed=0):
    """edge_index sorted by target (the layout's order) and not by source, so the by-source permutation is not the
    identity; atoms 3, 77 and N-1 have no outgoing edge; atom 11 has more than 300."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, N, (E,), generator=g)
    iso = torch.tensor([3, 77, N - 1])
    src[torch.isin(src, iso)] = 5
    src[:320] = 11
    dst = torch.randint(0, N, (E,), generator=g)
    order = torch.argsort(dst, stable=True)
    return torch.stack([src[order], dst[order]]), iso


def tp1_ref(x0, w, vec, ei):
    """oracle/ecomformer_ref.py tp_layer_1 on a given per-edge weight tensor w; xi = x0[dst] is an input of its own so
    that its gradient is the kernel's dxe."""
    src, dst = ei
    y1, y2 = ecr.spherical_harmonics_12(vec)
    xi = x0[dst].detach().requires_grad_(True)
    W0 = w[:, :NS * NS].reshape(-1, NS, NS)
    W1 = w[:, NS * NS:NS * NS + NS * NV].reshape(-1, NS, NV)
    W2 = w[:, NS * NS + NS * NV:].reshape(-1, NS, NV)
    t0 = torch.einsum("eu,euw->ew", xi, W0) / 8.0
    t1 = torch.einsum("eu,euw->ew", xi, W1) / 8.0
    t2 = torch.einsum("eu,euw->ew", xi, W2) / 8.0
    out = torch.cat((t0, (t1.unsqueeze(-1) * y1.unsqueeze(1)).reshape(-1, 3 * NV),
                     (t2.unsqueeze(-1) * y2.unsqueeze(1)).reshape(-1, 5 * NV)), dim=-1)
    out = ecr._scatter_mean(out, src, x0.shape[0])
    return out + F.pad(x0, (0, out.shape[1] - x0.shape[1])), xi


def tp2_ref(h1, w, vec, ei):
    """oracle/ecomformer_ref.py tp_layer_2 on a given w; hi = h1[dst] is an input of its own (the kernel's dhe)."""
    src, dst = ei
    y1, y2 = ecr.spherical_harmonics_12(vec)
    hi = h1[dst].detach().requires_grad_(True)
    s = hi[:, :NS]
    v1 = hi[:, NS:NS + 3 * NV].reshape(-1, NV, 3)
    v2 = hi[:, NS + 3 * NV:].reshape(-1, NV, 5)
    inp = torch.cat((s, (v1 * y1.unsqueeze(1)).sum(-1) / math.sqrt(3.0), (v2 * y2.unsqueeze(1)).sum(-1) / math.sqrt(5.0)),
                    dim=-1)
    out = torch.einsum("eu,euw->ew", inp, w.reshape(-1, NS + 2 * NV, NS)) / math.sqrt(float(NS + 2 * NV))
    return ecr._scatter_mean(out, src, h1.shape[0]), hi


@pytest.fixture(scope="module")
def equi_case(ops):
    ei, iso = equi_graph()
    N, E = 500, int(ei.shape[1])
    lay = ops.GraphLayout(ei.to(dev()), N, torch.tensor([0, N], dtype=torch.int64, device=dev()))
    lay.validate()
    assert not torch.equal(lay.perm[:E].cpu().long(), torch.arange(E))
    w = rnd(E, NW, seed=21, scale=0.2)
    vec = rnd(E, 3, seed=22, scale=2.0)
    return dict(ei=ei, iso=iso, N=N, E=E, lay=lay, w=w, vec=vec, wd=w.to(dev()), vecd=vec.to(dev()))


def test_equi_tp1_against_fp64(ops, equi_case):
    """Layer 1 forward (h1) and backward (dw, dxe w.r.t. the gathered x0[dst]) against fp64 autograd through the restated
    layer, 1e-5 norm-wise per tensor; atoms without an outgoing edge give h1 = pad(x0) exactly; two runs bitwise equal."""
    c = equi_case
    N, E, lay = c["N"], c["E"], c["lay"]
    x0, dh1 = rnd(N, NS, seed=23), rnd(N, H1, seed=24)
    runs = []
    for _ in range(2):
        h1 = torch.full((N, H1), float("nan"), device=dev())
        ops.equi_tp1_fwd(x0.to(dev()), c["wd"], c["vecd"], lay, h1)
        dw = torch.full((E, NW), float("nan"), device=dev())
        dxe = torch.full((E, NS), float("nan"), device=dev())
        ops.equi_tp1_bwd(x0.to(dev()), c["wd"], c["vecd"], lay, dh1.to(dev()), dw, dxe)
        runs.append((h1, dw, dxe))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    h1, dw, dxe = runs[0]
    w64 = c["w"].double().requires_grad_(True)
    ref, xi = tp1_ref(x0.double(), w64, c["vec"].double(), c["ei"])
    (ref * dh1.double()).sum().backward()
    assert rel_err(h1, ref) < TOL
    assert rel_err(dw, w64.grad) < TOL
    assert rel_err(dxe, xi.grad) < TOL
    iso = c["iso"]
    assert torch.equal(h1[iso].cpu(), F.pad(x0[iso], (0, H1 - NS)))


def test_equi_tp2_against_fp64(ops, equi_case):
    """Layer 2 forward (o2) and backward (dw, dhe w.r.t. the gathered h1[dst]) against fp64 autograd, 1e-5 norm-wise per
    tensor; atoms without an outgoing edge give o2 = 0 exactly; two runs bitwise equal."""
    c = equi_case
    N, E, lay = c["N"], c["E"], c["lay"]
    h1, do2 = rnd(N, H1, seed=25), rnd(N, NS, seed=26)
    runs = []
    for _ in range(2):
        o2 = torch.full((N, NS), float("nan"), device=dev())
        ops.equi_tp2_fwd(h1.to(dev()), c["wd"], c["vecd"], lay, o2)
        dw = torch.full((E, NW), float("nan"), device=dev())
        dhe = torch.full((E, H1), float("nan"), device=dev())
        ops.equi_tp2_bwd(h1.to(dev()), c["wd"], c["vecd"], lay, do2.to(dev()), dw, dhe)
        runs.append((o2, dw, dhe))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    o2, dw, dhe = runs[0]
    w64 = c["w"].double().requires_grad_(True)
    ref, hi = tp2_ref(h1.double(), w64, c["vec"].double(), c["ei"])
    (ref * do2.double()).sum().backward()
    assert rel_err(o2, ref) < TOL
    assert rel_err(dw, w64.grad) < TOL
    assert rel_err(dhe, hi.grad) < TOL
    assert torch.equal(o2[c["iso"]].cpu(), torch.zeros(len(c["iso"]), NS))

"""The grouped forms of the iComformer kernels (include/cartnet_hip.h "iComformer: BatchNorm groups") through the C ABI,
each against torch fp64 evaluated group by group.  Seven segments of (0, 3, 1, 9, 2, 0, 5) rows -- empty ones included --
are cut into G = 3 groups of (2, 3, 2) segments; two workgroups per group, so a group's partial rows are more than one
and some workgroups have nothing to do; C = 8 (one lane pair), 256 (one full chunk), 264 (a second chunk with two active
lanes).  With groups = NULL every grouped entry point must return the bytes of the entry point without the suffix."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = (0, 3, 1, 9, 2, 0, 5)
SEGS_PER_GROUP = (2, 3, 2)
PARTS = 2
TOL = 1e-5
WIDTHS = (8, 256, 264)


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def layout():
    ptr = torch.tensor([0] + list(COUNTS)).cumsum(0).int()
    seg_gptr = torch.tensor([0] + list(SEGS_PER_GROUP)).cumsum(0).int()
    row_gptr = ptr[seg_gptr.long()].contiguous()
    return ptr, seg_gptr, row_gptr


class Ctx:
    """Library handle, stream and the two group descriptors: over the segments (rows counted through ptr) and over the rows
    themselves (the softplus update and the column statistics see plain rows)."""

    def __init__(self):
        from cartnet_amd import lib
        self.lib, self.l = lib, lib.load()
        self.ptr, self.seg_gptr, self.row_gptr = (t.to(dev()) for t in layout())
        self.S, self.R, self.G = len(COUNTS), int(sum(COUNTS)), len(SEGS_PER_GROUP)
        self.seg_groups = self._groups(self.seg_gptr, self.row_gptr)
        self.row_groups = self._groups(self.row_gptr, self.row_gptr)
        self.nparts = lambda n: int(self.l.cartnet_segment_nparts(n))

    def _groups(self, node_gptr, edge_gptr):
        g = self.lib.Groups()
        g.node_gptr, g.edge_gptr, g.G, g.edge_parts, g.node_parts = node_gptr.data_ptr(), edge_gptr.data_ptr(), self.G, PARTS, PARTS
        return g

    def call(self, name, *args):
        out = []
        for a in args:
            if torch.is_tensor(a):
                out.append(a.data_ptr())
            elif isinstance(a, self.lib.Groups):
                out.append(C.addressof(a))
            else:
                out.append(a)
        self.lib.check(getattr(self.l, name)(*out, self.lib.stream_ptr()), name)
        torch.cuda.synchronize()

    def parts(self, rows, cols):
        return torch.full((rows, cols), float("nan"), dtype=torch.float64, device=dev())


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


def close(got, ref, what):
    ref = ref.double().cpu()
    err = float((got.detach().double().cpu().reshape(ref.shape) - ref).abs().max()) if ref.numel() else 0.0
    bound = TOL * max(float(ref.abs().max()) if ref.numel() else 0.0, 1e-30)
    print(f"{what}: {err:.3g} (bound {bound:.3g})")
    assert err <= bound, (what, err, bound)


def group_of_segment():
    return torch.repeat_interleave(torch.arange(len(SEGS_PER_GROUP)), torch.tensor(SEGS_PER_GROUP))


def seg_of_row():
    return torch.repeat_interleave(torch.arange(len(COUNTS)), torch.tensor(COUNTS))


def group_sums(x, gid, G):
    """[G, cols] sums of the rows of x by group id (fp64)."""
    return torch.zeros(G, x.shape[1], dtype=torch.float64).index_add_(0, gid, x.double())


def stats_rows(width, seed):
    """mean | rstd rows [G, 2C] with rstd > 0"""
    mr = rnd(len(SEGS_PER_GROUP), 2 * width, seed=seed) * 0.3
    mr[:, width:] = mr[:, width:].abs() + 0.5
    return mr


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("write_alpha", [True, False])
def test_rowmul_fwd_grouped(ctx, width, write_alpha):
    S, R, G = ctx.S, ctx.R, ctx.G
    key, q, scale = rnd(R, width, seed=1), rnd(S, width, seed=2), 1.0 / width ** 0.5
    kd, qd = key.to(dev()), q.to(dev())
    alpha = torch.zeros(R, width, device=dev())
    ps, pq = ctx.parts(G * PARTS, width), ctx.parts(G * PARTS, width)
    ctx.call("cartnet_rowmul_fwd_grouped", kd, width, qd, width, ctx.ptr, S, width, scale, alpha if write_alpha else None,
             width, ps, pq, ctx.seg_groups)
    ref = key.double() * q.double()[seg_of_row()] * scale
    gid = group_of_segment()[seg_of_row()]
    if write_alpha:
        close(alpha, ref, "alpha")
    close(ps.view(G, PARTS, width).sum(1), group_sums(ref, gid, G), "sum alpha per group")
    close(pq.view(G, PARTS, width).sum(1), group_sums(ref * ref, gid, G), "sum alpha^2 per group")
    # groups = NULL: the single-group entry point's bytes
    n = ctx.nparts(S)
    a0, a1 = torch.zeros(R, width, device=dev()), torch.zeros(R, width, device=dev())
    p0, q0, p1, q1 = (ctx.parts(n, width) for _ in range(4))
    ctx.call("cartnet_rowmul_fwd", kd, width, qd, width, ctx.ptr, S, width, scale, a0, width, p0, q0)
    ctx.call("cartnet_rowmul_fwd_grouped", kd, width, qd, width, ctx.ptr, S, width, scale, a1, width, p1, q1, None)
    assert torch.equal(a0, a1) and torch.equal(p0, p1) and torch.equal(q0, q1)


def gate_reference(key, msg, q, mr, gamma, beta, scale, width):
    """fp64: alpha, ahat, z per row with the row's group statistics"""
    srow = seg_of_row()
    g = group_of_segment()[srow]
    alpha = key.double() * q.double()[srow] * scale
    ahat = (alpha - mr.double()[g, :width]) * mr.double()[g, width:]
    z = torch.sigmoid(ahat * gamma.double() + beta.double())
    return srow, g, alpha, ahat, z


@pytest.mark.parametrize("width", WIDTHS)
def test_att_gate_fwd_grouped(ctx, width):
    S, R, G = ctx.S, ctx.R, ctx.G
    key, msg, q = rnd(R, width, seed=3), rnd(R, width, seed=4), rnd(S, width, seed=5)
    mr, gamma, beta, scale = stats_rows(width, 6), rnd(width, seed=7), rnd(width, seed=8), 1.0 / width ** 0.5
    gs = torch.cat([key, msg], 1).contiguous().to(dev())
    qd, mrd, gd, bd = q.to(dev()), mr.to(dev()), gamma.to(dev()), beta.to(dev())
    aggr, bc = torch.full((S, width), 7.0, device=dev()), torch.full((S, 2 * width), 7.0, device=dev())
    ctx.call("cartnet_att_gate_fwd_grouped", gs, qd, width, ctx.ptr, mrd, gd, bd, scale, S, width, aggr, bc, ctx.seg_groups)
    srow, g, alpha, ahat, z = gate_reference(key, msg, q, mr, gamma, beta, scale, width)
    w = msg.double() * z * (1 - z)
    seg = lambda x: torch.zeros(S, width, dtype=torch.float64).index_add_(0, srow, x)
    close(aggr, seg(z * msg.double()), "aggr")
    close(bc[:, :width], seg(w), "bc B")
    close(bc[:, width:], seg(w * ahat), "bc C")
    a2 = torch.full((S, width), 7.0, device=dev())
    ctx.call("cartnet_att_gate_fwd_grouped", gs, qd, width, ctx.ptr, mrd, gd, bd, scale, S, width, a2, None, ctx.seg_groups)
    assert torch.equal(a2, aggr)                       # the form without the per-segment sums
    # groups = NULL (row 0 of the statistics): the single-group entry point's bytes
    o0, o1 = (torch.zeros(S, width, device=dev()) for _ in range(2))
    c0, c1 = (torch.zeros(S, 2 * width, device=dev()) for _ in range(2))
    ctx.call("cartnet_att_gate_fwd", gs, qd, width, ctx.ptr, mrd, gd, bd, scale, S, width, o0, c0)
    ctx.call("cartnet_att_gate_fwd_grouped", gs, qd, width, ctx.ptr, mrd, gd, bd, scale, S, width, o1, c1, None)
    assert torch.equal(o0, o1) and torch.equal(c0, c1)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("key_in_gs", [True, False])
def test_att_gate_bwd_apply_grouped(ctx, width, key_in_gs):
    """key_in_gs: gs = [key | msg] (the alpha-free forward); else gs = [alpha | msg] with the key rows beside it (C > 256)."""
    S, R, G = ctx.S, ctx.R, ctx.G
    key, msg, q, daggr = rnd(R, width, seed=9), rnd(R, width, seed=10), rnd(S, width, seed=11), rnd(S, width, seed=12)
    mr, gamma, beta, scale = stats_rows(width, 13), rnd(width, seed=14), rnd(width, seed=15), 1.0 / width ** 0.5
    sums = rnd(G, 2 * width, seed=16)
    srow, g, alpha, ahat, z = gate_reference(key, msg, q, mr, gamma, beta, scale, width)
    rows_g = torch.tensor([int((g == i).sum()) for i in range(G)], dtype=torch.float64)
    inv = torch.where(rows_g > 0, 1.0 / rows_g.clamp(min=1), torch.zeros_like(rows_g))[g].unsqueeze(1)
    dbn = daggr.double()[srow] * msg.double() * z * (1 - z)
    da = gamma.double() * mr.double()[g, width:] * (dbn - sums.double()[g, :width] * inv - ahat * sums.double()[g, width:] * inv)
    dkey, dmsg = da * q.double()[srow] * scale, daggr.double()[srow] * z
    dq = torch.zeros(S, width, dtype=torch.float64).index_add_(0, srow, da * key.double()) * scale

    def run(name, groups, nrows):
        first = key if key_in_gs else (key * q[srow] * scale)
        gs = torch.cat([first, msg], 1).contiguous().to(dev())
        dqd = torch.full((S, width), 7.0, device=dev())
        pk, pm, pq = (ctx.parts(nrows, width) for _ in range(3))
        args = [gs, None if key_in_gs else key.to(dev()), width, q.to(dev()), width, daggr.to(dev()), ctx.ptr, mr.to(dev()),
                gamma.to(dev()), beta.to(dev()), sums.to(dev()), R, 1, scale, S, width, dqd, width, pk, pm, pq]
        ctx.call(name, *(args + ([groups] if name.endswith("_grouped") else [])))
        return gs, dqd, pk, pm, pq

    gs, dqd, pk, pm, pq = run("cartnet_att_gate_bwd_apply_grouped", ctx.seg_groups, G * PARTS)
    close(gs[:, :width], dkey, "dkey")
    close(gs[:, width:], dmsg, "dmsg")
    close(dqd, dq, "dq")
    close(pk.sum(0), dkey.sum(0), "column sums of dkey over all G x parts rows")
    close(pm.sum(0), dmsg.sum(0), "column sums of dmsg")
    close(pq.sum(0), dq.sum(0), "column sums of dq")
    a = run("cartnet_att_gate_bwd_apply", None, ctx.nparts(S))
    b = run("cartnet_att_gate_bwd_apply_grouped", None, ctx.nparts(S))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("width", WIDTHS)
def test_coldot_bc_partial_grouped(ctx, width):
    S, G = ctx.S, ctx.G
    d, bc = rnd(S, width, seed=17), rnd(S, 2 * width, seed=18)
    dd, bcd = d.to(dev()), bc.to(dev())
    pa, pb = ctx.parts(G * PARTS, width), ctx.parts(G * PARTS, width)
    ctx.call("cartnet_coldot_bc_partial_grouped", dd, width, bcd, S, width, pa, pb, ctx.seg_groups)
    gid = group_of_segment()
    close(pa.view(G, PARTS, width).sum(1), group_sums(d.double() * bc.double()[:, :width], gid, G), "sum d B per group")
    close(pb.view(G, PARTS, width).sum(1), group_sums(d.double() * bc.double()[:, width:], gid, G), "sum d C per group")
    n = ctx.nparts(S)
    a0, b0, a1, b1 = (ctx.parts(n, width) for _ in range(4))
    ctx.call("cartnet_coldot_bc_partial", dd, width, bcd, S, width, a0, b0)
    ctx.call("cartnet_coldot_bc_partial_grouped", dd, width, bcd, S, width, a1, b1, None)
    assert torch.equal(a0, a1) and torch.equal(b0, b1)


@pytest.mark.parametrize("width", WIDTHS)
def test_softplus_update_grouped(ctx, width):
    """y = softplus(x + bn(o)) and its two-pass backward over N = 20 rows in groups of (3, 12, 5)."""
    N, G = ctx.R, ctx.G
    o, x, dy = rnd(N, width, seed=19), rnd(N, width, seed=20), rnd(N, width, seed=21)
    mr, gamma, beta, sums = stats_rows(width, 22), rnd(width, seed=23), rnd(width, seed=24), rnd(G, 2 * width, seed=25)
    dx_add = rnd(N, width, seed=26)
    g = torch.repeat_interleave(torch.arange(G), (ctx.row_gptr[1:] - ctx.row_gptr[:-1]).cpu().long())
    ohat = (o.double() - mr.double()[g, :width]) * mr.double()[g, width:]
    u = x.double() + ohat * gamma.double() + beta.double()
    du = dy.double() * torch.sigmoid(u)
    inv = (1.0 / torch.bincount(g, minlength=G).double())[g].unsqueeze(1)
    d_o = gamma.double() * mr.double()[g, width:] * (du - sums.double()[g, :width] * inv - ohat * sums.double()[g, width:] * inv)
    od, xd, dyd, mrd, gd, bd, sd, addd = (t.to(dev()) for t in (o, x, dy, mr, gamma, beta, sums, dx_add))

    y = torch.zeros(N, width, device=dev())
    ctx.call("cartnet_softplus_update_fwd_grouped", od, xd, mrd, gd, bd, N, width, y, ctx.row_groups)
    close(y, torch.nn.functional.softplus(u), "y")
    pa, pb = ctx.parts(G * PARTS, width), ctx.parts(G * PARTS, width)
    ctx.call("cartnet_softplus_update_bwd_stats_grouped", od, xd, dyd, mrd, gd, bd, N, width, pa, pb, ctx.row_groups)
    close(pa.view(G, PARTS, width).sum(1), group_sums(du, g, G), "sum du per group")
    close(pb.view(G, PARTS, width).sum(1), group_sums(du * ohat, g, G), "sum du ohat per group")
    do_, dx = torch.zeros(N, width, device=dev()), torch.zeros(N, width, device=dev())
    pd = ctx.parts(G * PARTS, width)
    ctx.call("cartnet_softplus_update_bwd_apply_grouped", od, xd, dyd, mrd, gd, bd, sd, 1, N, width, do_, addd, dx, pd,
             ctx.row_groups)
    close(do_, d_o, "d_o")
    close(dx, du + dx_add.double(), "dx")
    close(pd.sum(0), d_o.sum(0), "column sums of d_o over all G x parts rows")
    do2, dx2 = torch.zeros(N, width, device=dev()), torch.zeros(N, width, device=dev())
    ctx.call("cartnet_softplus_update_bwd_apply_grouped", od, xd, dyd, mrd, gd, bd, sd, 1, N, width, do2, None, dx2, None,
             ctx.row_groups)
    assert torch.equal(do2, do_)
    close(dx2, du, "dx without dx_add")

    # groups = NULL: the single-group entry points' bytes
    n = ctx.nparts(N)
    y0, y1 = torch.zeros(N, width, device=dev()), torch.zeros(N, width, device=dev())
    ctx.call("cartnet_softplus_update_fwd", od, xd, mrd, gd, bd, N, width, y0)
    ctx.call("cartnet_softplus_update_fwd_grouped", od, xd, mrd, gd, bd, N, width, y1, None)
    assert torch.equal(y0, y1)
    a0, b0, a1, b1 = (ctx.parts(n, width) for _ in range(4))
    ctx.call("cartnet_softplus_update_bwd_stats", od, xd, dyd, mrd, gd, bd, N, width, a0, b0)
    ctx.call("cartnet_softplus_update_bwd_stats_grouped", od, xd, dyd, mrd, gd, bd, N, width, a1, b1, None)
    assert torch.equal(a0, a1) and torch.equal(b0, b1)
    res = []
    for name, tail in (("cartnet_softplus_update_bwd_apply_sums", []), ("cartnet_softplus_update_bwd_apply_grouped", [None])):
        do_n, dx_n, p_n = torch.zeros(N, width, device=dev()), torch.zeros(N, width, device=dev()), ctx.parts(n, width)
        ctx.call(name, od, xd, dyd, mrd, gd, bd, sd, 1, N, width, do_n, addd, dx_n, p_n, *tail)
        res.append((do_n, dx_n, p_n))
    assert all(torch.equal(p, r) for p, r in zip(*res))
    do_n, dx_n = torch.zeros(N, width, device=dev()), torch.zeros(N, width, device=dev())
    ctx.call("cartnet_softplus_update_bwd_apply", od, xd, dyd, mrd, gd, bd, sd, 1, N, width, do_n, addd, dx_n)
    assert torch.equal(do_n, res[0][0]) and torch.equal(dx_n, res[0][1])


@pytest.mark.parametrize("width", WIDTHS)
def test_colstats_grouped_nodes(ctx, width):
    """per-group column sums / sums of squares over the groups' NODE ranges (a padded view: ld > C)"""
    N, G = ctx.R, ctx.G
    buf = rnd(N, width + 8, seed=27)
    x = buf[:, :width]
    xd = buf.to(dev())
    ps, pq = ctx.parts(G * PARTS, width), ctx.parts(G * PARTS, width)
    ctx.call("cartnet_colstats_grouped_nodes", xd, width + 8, width, ctx.row_groups, ps, pq)
    g = torch.repeat_interleave(torch.arange(G), (ctx.row_gptr[1:] - ctx.row_gptr[:-1]).cpu().long())
    close(ps.view(G, PARTS, width).sum(1), group_sums(x, g, G), "sum per group")
    close(pq.view(G, PARTS, width).sum(1), group_sums(x.double() ** 2, g, G), "sum of squares per group")

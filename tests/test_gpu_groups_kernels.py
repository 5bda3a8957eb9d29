"""CartNet's BatchNorm-group kernels (include/cartnet_hip.h "BatchNorm groups") and the three sync-BatchNorm steps, one by
one through the C ABI, each against torch fp64 on the CPU evaluated group by group from exactly the values the kernel
reads.  The grouped fp32 forms had only HIP-against-HIP tests (test_gpu_groups_half.py, test_gpu_colstats_grouped_h.py)
and whole train steps (test_gpu_groups.py) before; an error both storage forms share, or one in a finaliser, passed them.

One tiny layout serves parts 1, 2 and the finalisers: 60 target-sorted atoms in G = 6 groups --
  0  the 24 atoms of test_gpu_half_storage_kernels.DEGS (every remainder of the 8-edge rounds, zeros included),
  1  no atoms,
  2  one atom with one edge,
  3  five atoms without edges,
  4  27 atoms of in-degree (3 i + 1) % 5: more than 4 * edge_parts * 3, so a gate workgroup makes four sweeps and the
     last one is partial (a node workgroup three, the last partial),
  5  three atoms (2, 0, 3 edges): fewer than 4 * edge_parts, so one gate workgroup (two node workgroups) is idle and
     must still write its zero partial rows --
with edge_parts = 2 and node_parts = 3 (different on purpose: a kernel or finaliser that reads the wrong one shows),
D = 4 (one lane), 256 (one full pass), 260 (a second pass with one lane), 320 (a second pass with 16 of 64 lanes), and
per-group mean | rstd rows that differ by tenths from group to group.  Partial-sum buffers are allocated one
max(edge_parts, node_parts) x G block long and handed over as their first [G][parts][D]; like every output they start as
NaN, so a row that is not written, and one written past the view, shows.  Every check prints its figure and its bound
before it asserts.

Bounds are the ones the project uses for the same kernels without groups, named where they are defined below.

Measured on an MI355X (worst over all cases).  Gate forward: e_out 6.5e-8, aggr 2.3e-7, per-group sums of aggr 1.5e-7 and
of aggr^2 2.0e-7; backward statistics 2.3e-7 (sum dbn) and 3.7e-7 (sum dbn ghat); apply: dg | ds 2.9e-7, per-group sums of
ds 1.2e-7, of dg 5.1e-7 (eval) and 1.1e-5 of sum |dg| (training, bound 1e-4: the total of the one-edge group and of the
five-edge group in a column where the sigmoid is saturated, z = 0.999, so that 1 - z carries 1e-5 in fp32; a plain fp32
evaluation of the formula in torch gives the same 1.1e-5 there and 1.6e-7 or less for the two large groups); G = 1 against groups == NULL: the same bytes, column totals 0.  Node update: x_out 1.3e-7,
per-group sums 3.3e-7 and 7.8e-7, daggr 6.2e-7.  cartnet_colstats_grouped 3.9e-15 of sum |x|; cartnet_bn_finalize: mean
4.9e-8, rstd 4.4e-8, running statistics 3.8e-8 (the hand-written formula against nn.BatchNorm1d on the CPU: 5.6e-14);
cartnet_group_sums_finalize 5.0e-8; cartnet_colsum_finalize2 3.3e-8.  The chained layer: x_out 1.8e-7, e_out 4.8e-8,
dg | ds 3.2e-7, affine gradients 3.2e-7 or less, running buffers 1.0e-7 or less.  Sync-BatchNorm: gather 1.5e-16 of
sum |term|, statistics of the union 4.9e-8 or less, scaled sums 4.8e-8, daggr 2.3e-7, affine gradients 1.6e-7.
"""
import ctypes as C
import functools

import pytest
import torch

from conftest import rel_err
from test_gpu_half_storage_kernels import DEGS

pytestmark = pytest.mark.gpu

TOL = 1e-5                   # test_gpu_kernels.TOL (test_gate_scatter_fwd_bwd, test_gpu_half_storage_kernels._check_forward /
#                              _check_stats): e_out, aggr, forward column sums, backward statistics; x_out of the node update
APPLY_TOL = 2e-5             # test_gate_scatter_fwd_bwd / _check_apply: dg | ds
APPLY_SUM_TOL = 1e-4         # ... and their column sums
NODE_BWD_TOL = 2e-5          # test_bn_finalize_and_node_update: daggr and the two backward sums of the node update
BN_TOL = 1e-6                # test_bn_finalize_and_node_update (its eval-mode rstd): mean, rstd, running statistics
SUMS_TOL = 1e-6              # test_colsum_finalize: fp64 partial rows -> fp32 column sums
RUNNING_TOL = 1e-5           # test_bn_finalize_and_node_update: running buffers against nn.BatchNorm1d (chained test)
F64_SUM = 1e-12              # fp64 accumulation of at most 1030 terms: (n - 1) 2^-53 < 1.2e-13 of sum |term|, twice (the
#                              kernel's order and torch's), with a factor of four to spare
EPS, MOMENTUM = 1e-5, 0.1

EDGE_PARTS, NODE_PARTS = 2, 3
MAX_PARTS = max(EDGE_PARTS, NODE_PARTS)
WIDTHS = (4, 256, 260, 320)
BIG, SMALL = [(3 * i + 1) % 5 for i in range(27)], [2, 0, 3]
GROUP_DEGS = (DEGS, [], [1], [0] * 5, BIG, SMALL)
ONE_EDGE, NO_EDGES, EMPTY = 2, 3, 1


def dev():
    return torch.device("cuda:0")


def f32(x):
    """the value of x as the fp32 the C ABI receives, as a Python float"""
    return float(torch.tensor(x, dtype=torch.float32))


def _report(what, err, bound):
    print(f"{what}: {err:.3g} (bound {bound:g})")
    assert err < bound, (what, err, bound)


# --------------------------------------------------------------------------------------------------- layout and calls
class Layout:
    """Target-sorted atoms with the given in-degrees per group; only rowptr and the two group pointer arrays reach the
    kernels (the sources of the edges play no part in them)."""

    def __init__(self, group_degs):
        self.G = len(group_degs)
        self.deg = torch.tensor([d for g in group_degs for d in g], dtype=torch.int64)
        self.N, self.E = int(self.deg.numel()), int(self.deg.sum())
        self.rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), self.deg.cumsum(0)]).int()
        self.node_gptr = torch.tensor([0] + [len(g) for g in group_degs]).cumsum(0).int()
        self.edge_gptr = self.rowptr[self.node_gptr.long()].contiguous()
        self.nodes = (self.node_gptr[1:] - self.node_gptr[:-1]).long()          # rows per group
        self.edges = (self.edge_gptr[1:] - self.edge_gptr[:-1]).long()
        self.tgt = torch.repeat_interleave(torch.arange(self.N), self.deg)
        self.gid_node = torch.repeat_interleave(torch.arange(self.G), self.nodes)
        self.gid_edge = torch.repeat_interleave(torch.arange(self.G), self.edges)
        self.rowptr_d, self.node_gptr_d, self.edge_gptr_d = (t.to(dev()) for t in (self.rowptr, self.node_gptr, self.edge_gptr))


@functools.lru_cache(maxsize=None)
def shared():
    lay = Layout(GROUP_DEGS)
    assert lay.N == 60 and lay.nodes.tolist() == [24, 0, 1, 5, 27, 3] and lay.edges.tolist() == [242, 0, 1, 0, 55, 5]
    assert set((lay.deg[:24] % 8).tolist()) == set(range(8)) and int((lay.deg == 0).sum()) >= 8
    assert 27 > 4 * EDGE_PARTS * 3 and 27 % (4 * EDGE_PARTS) and 27 % (4 * NODE_PARTS) and 3 < 4 * EDGE_PARTS
    return lay


class Ctx:
    def __init__(self):
        from cartnet_amd import lib
        self.lib, self.l = lib, lib.load()

    def groups(self, lay, edge_parts=EDGE_PARTS, node_parts=NODE_PARTS):
        g = self.lib.Groups()
        g.node_gptr, g.edge_gptr, g.G = lay.node_gptr_d.data_ptr(), lay.edge_gptr_d.data_ptr(), lay.G
        g.edge_parts, g.node_parts = edge_parts, node_parts
        return g

    def rc(self, name, *args):
        out = []
        for a in args:
            if torch.is_tensor(a):
                out.append(a.data_ptr())
            elif isinstance(a, self.lib.Groups):
                out.append(C.addressof(a))
            else:
                out.append(a)
        rc = getattr(self.l, name)(*out, self.lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def call(self, name, *args):
        self.lib.check(self.rc(name, *args), name)


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev())


class Parts:
    """fp64 partial rows [G][parts][D]: the head of a NaN-filled buffer of G * MAX_PARTS + 1 rows."""

    def __init__(self, G, parts, D, fill=None):
        self.full = nan((G * max(parts, MAX_PARTS) + 1) * D, dtype=torch.float64)
        self.t = self.full[:G * parts * D].view(G, parts, D)
        if fill is not None:
            self.t.copy_(fill.to(dev()))

    def data_ptr(self):
        return self.full.data_ptr()

    def written(self, what):
        """every row of the view written, nothing behind it; returns the rows on the CPU"""
        assert bool(torch.isfinite(self.t).all()), what + ": a partial row was not written"
        assert bool(self.full[self.t.numel():].isnan().all()), what + ": written past [G][parts][D]"
        return self.t.cpu()


def call_with_parts(ctx, name, *args):
    """ctx.call with Parts objects passed as their buffers"""
    ctx.call(name, *[a.full if isinstance(a, Parts) else a for a in args])


def by_group(x, gid, G):
    """[G, cols] fp64 sums of the rows of x by group id"""
    return torch.zeros(G, x.shape[1], dtype=torch.float64).index_add_(0, gid, x.double())


def group_rows_err(got, ref):
    """got, ref [G, D]: per group max |got - ref| / max |ref| over the group's row, worst group; a group whose reference
    row is all zeros (no rows to sum) must be exact zeros"""
    worst = 0.0
    for g in range(ref.shape[0]):
        scale = float(ref[g].abs().max())
        if scale == 0.0:
            assert not bool(got[g].any()), f"group {g}: zeros expected"
        else:
            worst = max(worst, float((got[g].double() - ref[g]).abs().max()) / scale)
    return worst


def zero_rows(lay, parts, per_edge):
    """(group, workgroup) pairs whose partial row must be exact zeros: workgroup b of a group owns its atoms 4 b + w + 4 parts j
    (wave w, sweep j); it is idle when the group has no more than 4 b atoms, and sums nothing in a per-edge kernel when
    none of its atoms has an edge"""
    out = []
    for g in range(lay.G):
        n0, n = int(lay.node_gptr[g]), int(lay.nodes[g])
        for b in range(parts):
            mine = [t for t in range(n) if (t // 4) % parts == b]
            if not mine or (per_edge and not any(int(lay.deg[n0 + t]) for t in mine)):
                out.append((g, b))
    return out


def check_zero_rows(lay, rows, parts, per_edge, what):
    zr = zero_rows(lay, parts, per_edge)
    for g, b in zr:
        assert not bool(rows[g, b].any()), (what, "partial row must be zeros", g, b)
    return zr


def stats_rows(G, D, seed):
    """mean | rstd rows [G, 2D] that differ by tenths from group to group"""
    gen = torch.Generator().manual_seed(seed)
    k = torch.arange(G, dtype=torch.float32)[:, None]
    mean = 0.3 * torch.randn(G, D, generator=gen) + 0.4 * (k - 2.5)
    rstd = 0.6 + 0.5 * torch.rand(G, D, generator=gen) + 0.2 * k
    return torch.cat([mean, rstd], 1).contiguous()


# --------------------------------------------------------------------------------------------------- 1. gate kernels
class Gate:
    """Inputs of the three gate kernels on a layout (fp32 masters on the CPU) and the fp64 formulas, every row normalised
    with its own group's mean | rstd row."""

    def __init__(self, lay, D, seed):
        self.lay, self.D = lay, D
        gen = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=gen)
        E, N, G = lay.E, lay.N, lay.G
        self.gs, self.e_in, self.de_out, self.daggr = r(E, 2 * D), r(E, D), r(E, D), r(N, D)
        self.env = torch.rand(E, generator=gen)
        self.gamma, self.beta = r(D), r(D)
        self.mean_rstd = stats_rows(G, D, seed + 1)
        if G > ONE_EDGE and int(lay.edges[ONE_EDGE]) == 1:
            # the only edge of its group: at least one standard deviation off the group's mean, so that its training-mode dg
            # = -gamma rstd dbn ghat^2 is no difference of two nearly equal numbers
            e = int(lay.edge_gptr[ONE_EDGE])
            mr = self.mean_rstd[ONE_EDGE]
            sign = torch.where(r(D) < 0, -1.0, 1.0)
            self.gs[e, :D] = mr[:D] + sign * (1.0 + r(D).abs()) / mr[D:]
        ge = lay.gid_edge
        mr = self.mean_rstd.double()
        self.g, self.s = self.gs[:, :D].double(), self.gs[:, D:].double()
        self.rstd = mr[ge, D:]
        self.ghat = (self.g - mr[ge, :D]) * self.rstd
        self.z = torch.sigmoid(self.ghat * self.gamma.double() + self.beta.double())
        self._dev = {}

    def d(self, name):
        if name not in self._dev:
            self._dev[name] = getattr(self, name).to(dev()).contiguous()
        return self._dev[name]

    def ev(self, env):
        return self.env.double()[:, None] if env else 1.0

    def fwd(self, env=True):
        sig = self.ev(env) * self.z
        aggr = torch.zeros(self.lay.N, self.D, dtype=torch.float64).index_add_(0, self.lay.tgt, sig * self.s)
        return self.e_in.double() + sig, aggr

    def dbn(self, de=True):
        dsig = self.daggr.double()[self.lay.tgt] * self.s + (self.de_out.double() if de else 0.0)
        return dsig * self.ev(True) * self.z * (1.0 - self.z)

    def sums(self):
        """[G, 2D]: every group's [sum dbn | sum dbn ghat], as the fp32 rows the apply pass is given"""
        dbn = self.dbn()
        G, ge = self.lay.G, self.lay.gid_edge
        return torch.cat([by_group(dbn, ge, G), by_group(dbn * self.ghat, ge, G)], 1).float().contiguous()

    def apply(self, training):
        D, ge = self.D, self.lay.gid_edge
        cnt = self.lay.edges.double()
        inv = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1), torch.zeros_like(cnt))[ge][:, None] * (1.0 if training else 0.0)
        sums = self.sums().double()
        dg = self.gamma.double() * self.rstd * (self.dbn() - sums[ge, :D] * inv - self.ghat * sums[ge, D:] * inv)
        ds = self.daggr.double()[self.lay.tgt] * self.ev(True) * self.z
        return dg, ds


@functools.lru_cache(maxsize=None)
def gate_case(D):
    return Gate(shared(), D, seed=300 + D)


def gate_fwd(ctx, c, groups, ps, pq, env=True, with_e=True):
    lay = c.lay
    e_out = nan(lay.E, c.D) if with_e else None
    aggr = nan(lay.N, c.D)
    call_with_parts(ctx, "cartnet_gate_scatter_fwd", c.d("gs"), c.d("e_in") if with_e else None, c.d("env") if env else None,
                    lay.rowptr_d, c.d("mean_rstd"), c.d("gamma"), c.d("beta"), lay.N, c.D, e_out, aggr, ps, pq, groups)
    return e_out, aggr


@pytest.mark.parametrize("D", WIDTHS)
def test_gate_forward_with_groups_against_fp64(ctx, D):
    """cartnet_gate_scatter_fwd with the six groups: e_out, aggr, and every group's column totals of aggr and aggr^2 taken
    as parts.view(G, edge_parts, D).sum(1); also with env = NULL and with e_in = e_out = NULL; atoms without edges
    aggregate exact zeros; the partial rows of the empty group, of the group without edges and of the idle workgroups are
    exact zeros and no NaN is left."""
    c, lay = gate_case(D), shared()
    grp = ctx.groups(lay)
    for env, with_e in ((True, True), (False, True), (True, False)):
        ps, pq = Parts(lay.G, EDGE_PARTS, D), Parts(lay.G, EDGE_PARTS, D)
        e_out, aggr = gate_fwd(ctx, c, grp, ps, pq, env, with_e)
        eo_ref, ag_ref = c.fwd(env)
        t = f"D={D} fwd env={env} e_out={with_e}"
        if with_e:
            assert bool(torch.isfinite(e_out).all())
            _report(t + " e_out", rel_err(e_out, eo_ref), TOL)
        assert bool(torch.isfinite(aggr).all())
        _report(t + " aggr", rel_err(aggr, ag_ref), TOL)
        rs, rq = ps.written(t), pq.written(t)
        _report(t + " per-group sum aggr", group_rows_err(rs.sum(1), by_group(ag_ref, lay.gid_node, lay.G)), TOL)
        _report(t + " per-group sum aggr^2", group_rows_err(rq.sum(1), by_group(ag_ref ** 2, lay.gid_node, lay.G)), TOL)
        assert not bool(aggr[(lay.deg == 0).to(dev())].any())                    # exact zeros
        zr = check_zero_rows(lay, rs, EDGE_PARTS, True, t)
        check_zero_rows(lay, rq, EDGE_PARTS, True, t)
        assert {(EMPTY, 0), (EMPTY, 1), (NO_EDGES, 0), (NO_EDGES, 1), (ONE_EDGE, 1), (5, 1)} <= set(zr)


@pytest.mark.parametrize("D", WIDTHS)
def test_gate_backward_statistics_with_groups_against_fp64(ctx, D):
    """cartnet_gate_scatter_bwd_stats: every group's sum dbn and sum dbn ghat; also with de_out = NULL."""
    c, lay = gate_case(D), shared()
    grp = ctx.groups(lay)
    for de in (True, False):
        pa, pb = Parts(lay.G, EDGE_PARTS, D), Parts(lay.G, EDGE_PARTS, D)
        call_with_parts(ctx, "cartnet_gate_scatter_bwd_stats", c.d("gs"), c.d("de_out") if de else None, c.d("daggr"),
                        c.d("env"), lay.rowptr_d, c.d("mean_rstd"), c.d("gamma"), c.d("beta"), lay.N, D, pa, pb, grp)
        dbn = c.dbn(de)
        t = f"D={D} stats de_out={de}"
        ra, rb = pa.written(t), pb.written(t)
        _report(t + " per-group sum dbn", group_rows_err(ra.sum(1), by_group(dbn, lay.gid_edge, lay.G)), TOL)
        _report(t + " per-group sum dbn ghat", group_rows_err(rb.sum(1), by_group(dbn * c.ghat, lay.gid_edge, lay.G)), TOL)
        check_zero_rows(lay, ra, EDGE_PARTS, True, t)
        check_zero_rows(lay, rb, EDGE_PARTS, True, t)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("D", WIDTHS)
def test_gate_backward_apply_with_groups_against_fp64(ctx, D, training):
    """cartnet_gate_scatter_bwd_apply alone (its per-group ``sums`` are the fp64 reference's, cast to fp32): dg | ds in
    place; the training-mode means divide by the group's own edge count -- the call is given the whole batch's E and,
    a second time, a number that is nobody's count, and must return the same bytes; per-group column totals of ds and dg
    (training: sum dg per column against sum |dg|, as test_gpu_half_storage_kernels._check_apply does)."""
    c, lay = gate_case(D), shared()
    grp = ctx.groups(lay)
    dg, ds = c.apply(training)
    ref = torch.cat([dg, ds], 1)
    outs = []
    for E_arg in (lay.E, 7 * lay.E + 3):
        gs = c.d("gs").clone()
        pdg, pds = Parts(lay.G, EDGE_PARTS, D), Parts(lay.G, EDGE_PARTS, D)
        call_with_parts(ctx, "cartnet_gate_scatter_bwd_apply", gs, c.d("de_out"), c.d("daggr"), c.d("env"), lay.rowptr_d,
                        c.d("mean_rstd"), c.d("gamma"), c.d("beta"), c.sums().to(dev()), E_arg, int(training), lay.N, D,
                        pdg, pds, grp)
        outs.append((gs, pdg, pds))
    (gs, pdg, pds), (gs2, pdg2, pds2) = outs
    t = f"D={D} apply training={training}"
    assert torch.equal(gs, gs2) and torch.equal(pdg.t, pdg2.t) and torch.equal(pds.t, pds2.t), t + ": depends on the call's E"
    assert bool(torch.isfinite(gs).all())
    _report(t + " dg | ds", rel_err(gs, ref), APPLY_TOL)
    rg, rs = pdg.written(t), pds.written(t)
    ge, G = lay.gid_edge, lay.G
    _report(t + " per-group sum ds", group_rows_err(rs.sum(1), by_group(ds, ge, G)), APPLY_SUM_TOL)
    if training:
        tot, mass = by_group(dg, ge, G), by_group(dg.abs(), ge, G)
        live = lay.edges > 0
        assert not bool(rg.sum(1)[~live].any())
        worst = ((rg.sum(1)[live] - tot[live]).abs() / mass[live]).max().item()
        _report(t + " |sum dg - ref| / sum |dg|, worst group and column", worst, APPLY_SUM_TOL)
    else:
        _report(t + " per-group sum dg", group_rows_err(rg.sum(1), by_group(dg, ge, G)), APPLY_SUM_TOL)
    check_zero_rows(lay, rg, EDGE_PARTS, True, t)
    check_zero_rows(lay, rs, EDGE_PARTS, True, t)


@pytest.mark.parametrize("D", [4, 320])
def test_one_group_over_the_whole_batch_is_the_call_without_groups(ctx, D):
    """A G = 1 descriptor over all 60 atoms with edge_parts = cartnet_gate_scatter_nparts(N): e_out and aggr are the bytes of
    the call with groups == NULL (whose statistics row is row 0); the column totals agree within TOL -- the descriptor
    deals its workgroups in descending order, so the same partial rows may sit in another order."""
    c, lay = gate_case(D), shared()
    P = int(ctx.l.cartnet_gate_scatter_nparts(lay.N))
    one = Layout([[int(d) for d in lay.deg]])
    assert P == 15 and one.E == lay.E
    g1 = ctx.groups(one, P, P)
    res = []
    for grp in (None, g1):
        ps, pq = Parts(1, P, D), Parts(1, P, D)
        e_out, aggr = gate_fwd(ctx, c, grp, ps, pq)
        res.append((e_out, aggr, ps.written("ps"), pq.written("pq")))
    (e0, a0, s0, q0), (e1, a1, s1, q1) = res
    assert bool(torch.isfinite(e0).all()) and torch.equal(e0, e1) and torch.equal(a0, a1)
    _report(f"D={D} G=1 vs NULL sum aggr", rel_err(s1.sum(1), s0.sum(1)), TOL)
    _report(f"D={D} G=1 vs NULL sum aggr^2", rel_err(q1.sum(1), q0.sum(1)), TOL)


# --------------------------------------------------------------------------------------------------- 2. node update
class Node:
    def __init__(self, lay, D, seed):
        self.lay, self.D = lay, D
        gen = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=gen)
        self.aggr, self.x_in, self.dx = r(lay.N, D) * 2.0 + 0.5, r(lay.N, D), r(lay.N, D)
        self.gamma, self.beta = r(D), r(D)
        self.mean_rstd = stats_rows(lay.G, D, seed + 1)
        gn, mr = lay.gid_node, self.mean_rstd.double()
        self.rstd = mr[gn, D:]
        self.ahat = (self.aggr.double() - mr[gn, :D]) * self.rstd
        self.u = self.ahat * self.gamma.double() + self.beta.double()
        sg = torch.sigmoid(self.u)
        self.dxn = self.dx.double() * sg * (1.0 + self.u * (1.0 - sg))             # dx silu'(u)

    def d(self, name):
        return getattr(self, name).to(dev()).contiguous()

    def sums(self):
        G, gn = self.lay.G, self.lay.gid_node
        return torch.cat([by_group(self.dxn, gn, G), by_group(self.dxn * self.ahat, gn, G)], 1).float().contiguous()

    def apply(self, training):
        D, gn = self.D, self.lay.gid_node
        cnt = self.lay.nodes.double()
        inv = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1), torch.zeros_like(cnt))[gn][:, None] * (1.0 if training else 0.0)
        sums = self.sums().double()
        return self.gamma.double() * self.rstd * (self.dxn - sums[gn, :D] * inv - self.ahat * sums[gn, D:] * inv)


def check_node(ctx, c, t):
    lay, D = c.lay, c.D
    grp = ctx.groups(lay)
    aggr, dx, mr, gamma, beta = (c.d(k) for k in ("aggr", "dx", "mean_rstd", "gamma", "beta"))
    x_out = nan(lay.N, D)
    ctx.call("cartnet_node_update_fwd", aggr, c.d("x_in"), mr, gamma, beta, lay.N, D, x_out, grp)
    assert bool(torch.isfinite(x_out).all())
    _report(t + " x_out", rel_err(x_out, torch.nn.functional.silu(c.u) + c.x_in.double()), TOL)
    pa, pb = Parts(lay.G, NODE_PARTS, D), Parts(lay.G, NODE_PARTS, D)
    call_with_parts(ctx, "cartnet_node_update_bwd_stats", aggr, dx, mr, gamma, beta, lay.N, D, pa, pb, grp)
    ra, rb = pa.written(t), pb.written(t)
    gn, G = lay.gid_node, lay.G
    _report(t + " per-group sum dxn", group_rows_err(ra.sum(1), by_group(c.dxn, gn, G)), NODE_BWD_TOL)
    _report(t + " per-group sum dxn ahat", group_rows_err(rb.sum(1), by_group(c.dxn * c.ahat, gn, G)), NODE_BWD_TOL)
    check_zero_rows(lay, ra, NODE_PARTS, False, t)
    check_zero_rows(lay, rb, NODE_PARTS, False, t)
    for training in (1, 0):
        daggr = nan(lay.N, D)
        ctx.call("cartnet_node_update_bwd_apply", aggr, dx, mr, gamma, beta, c.sums().to(dev()), training, lay.N, D, daggr, grp)
        assert bool(torch.isfinite(daggr).all())
        _report(t + f" daggr training={training}", rel_err(daggr, c.apply(training)), NODE_BWD_TOL)


@pytest.mark.parametrize("D", WIDTHS)
def test_node_update_with_groups_against_fp64(ctx, D):
    """cartnet_node_update_fwd / _bwd_stats / _bwd_apply on the six groups: the backward kernels run node_parts workgroups
    per group, and the training-mode means divide by the group's own node count (the call's N is the whole batch's 60)."""
    c = Node(shared(), D, seed=500 + D)
    zr = zero_rows(c.lay, NODE_PARTS, False)
    assert {(EMPTY, 0), (ONE_EDGE, 1), (ONE_EDGE, 2), (NO_EDGES, 2), (5, 1), (5, 2)} <= set(zr)
    check_node(ctx, c, f"D={D} node")


def test_node_update_forward_takes_several_trips_through_a_group(ctx):
    """D = 4, 1103 atoms in groups of (37, 1040, 0, 26): the forward launches N D / 4 / G / 256 = 2 workgroups per group,
    512 threads for the 1040 float4 of the second group -- three trips of the grid-stride loop, the last over 16."""
    lay = Layout([[0] * 37, [0] * 1040, [], [0] * 26])
    assert (lay.N * 4 // 4 // lay.G + 255) // 256 == 2
    check_node(ctx, Node(lay, 4, seed=77), "1103 atoms D=4 node")


# --------------------------------------------------------------------------------------------------- 3. statistics, finalisers
ROWS = (0, 1, 3, 17, 1030)          # test_gpu_colstats_grouped_h.ROWS: empty, one row, fewer than four, more than one trip


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("width", [8, 256, 520])
def test_colstats_grouped_fp32_against_fp64(ctx, width, parts):
    """cartnet_colstats_grouped on the row layout of test_gpu_colstats_grouped_h.py, ld = 2 C + 8 with NaN in the padding:
    every group's totals within 1e-12 of sum |x| (of sum x^2) -- the kernel accumulates in fp64, and the square of an
    fp32 value is exact in fp64; the empty group's rows are zeros."""
    lay = Layout([[1] * n for n in ROWS])                      # one edge per "atom": the edge ranges are the row ranges
    G, R, ld = lay.G, sum(ROWS), 2 * width + 8
    x = torch.randn(R, width, generator=torch.Generator().manual_seed(width))
    buf = torch.full((R, ld), float("nan"))
    buf[:, :width] = x
    ps, pq = Parts(G, parts, width), Parts(G, parts, width)
    call_with_parts(ctx, "cartnet_colstats_grouped", buf.to(dev()), ld, width, ctx.groups(lay, parts, 7), ps, pq)
    rs, rq = ps.written("sums").sum(1), pq.written("squares").sum(1)
    x64 = x.double()
    for what, got, ref, mass in (("sums", rs, by_group(x64, lay.gid_edge, G), by_group(x64.abs(), lay.gid_edge, G)),
                                 ("squares", rq, by_group(x64 * x64, lay.gid_edge, G), by_group(x64 * x64, lay.gid_edge, G))):
        live = torch.tensor(ROWS) > 0
        worst = ((got[live] - ref[live]).abs() / mass[live]).max().item()
        _report(f"C={width} parts={parts} {what}: |got - ref| / sum |term|", worst, F64_SUM)
    assert not bool(ps.t[0].any()) and not bool(pq.t[0].any())


def bn_reference(s, q, n, rm, rv, eps, momentum, round32):
    """nn.BatchNorm1d's training-mode statistics by hand, from per-group column sums s, sums of squares q [G, C] and row
    counts n [G]: mean, biased variance clamped at 0, rstd = 1 / sqrt(var + eps); the running buffers take one momentum
    update per group, in group order, with the unbiased variance for counts > 1 (rounded to fp32 after each one with
    round32, as the running buffers of fp32 modules are).  A group of 0 rows counts as mean 0, variance 0."""
    mean, rstd = torch.zeros_like(s), torch.zeros_like(s)
    rm, rv = rm.double().clone(), rv.double().clone()
    for g in range(s.shape[0]):
        k = float(n[g])
        if k > 0:
            mean[g] = s[g] / k
            var = (q[g] / k - mean[g] * mean[g]).clamp(min=0.0)
        else:
            var = torch.zeros_like(s[g])
        rstd[g] = 1.0 / torch.sqrt(var + eps)
        unb = var * (k / (k - 1.0)) if k > 1 else var
        rm = (1.0 - momentum) * rm + momentum * mean[g]
        rv = (1.0 - momentum) * rv + momentum * unb
        if round32:
            rm, rv = rm.float().double(), rv.float().double()
    return mean, rstd, rm, rv


@pytest.mark.parametrize("pair", [(1, 1), (1, 0), (0, 0)], ids=["edge_rows_edge_counts", "edge_rows_node_counts", "node_rows_node_counts"])
@pytest.mark.parametrize("width", [4, 20, 256])
def test_bn_finalize_with_groups_training(ctx, width, pair):
    """cartnet_bn_finalize (cn_bn_group_stats_kernel + cn_bn_running_kernel) on the six groups, for the three
    (parts_over_edges, count_over_edges) pairs the model uses; C = 20 gives a second 16-column block with 4 live columns.
    The reference is the hand-written fp64 formula on the partial rows the kernel reads; the same formula is checked
    here, on the CPU, against nn.BatchNorm1d(C).double() fed the groups of two rows or more one after the other.  Groups
    of 0 rows and of 1 row: mean 0 (the row itself), variance 0, rstd = 1 / sqrt(eps), and the running buffers take
    that update too -- pinned exactly."""
    poe, coe = pair
    lay = shared()
    G, P = lay.G, EDGE_PARTS if poe else NODE_PARTS
    cnt = lay.edges if coe else lay.nodes
    gid = lay.gid_edge if coe else lay.gid_node
    gen = torch.Generator().manual_seed(900 + width + 10 * poe + coe)
    k = torch.arange(G, dtype=torch.float32)[gid][:, None]
    x = (torch.randn(int(cnt.sum()), width, generator=gen) * (0.5 + 0.3 * k) + 0.4 * k - 1.0).double()     # fp32 values
    first = torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)])
    rs, rq = torch.zeros(G, P, width, dtype=torch.float64), torch.zeros(G, P, width, dtype=torch.float64)
    for g in range(G):
        for r in range(int(cnt[g])):                       # row r of a group went to its workgroup r % P
            rs[g, r % P] += x[first[g] + r]
            rq[g, r % P] += x[first[g] + r] ** 2
    rm0 = torch.randn(width, generator=gen)
    rv0 = torch.rand(width, generator=gen) + 0.5
    eps, mom = f32(EPS), f32(MOMENTUM)
    mean, rstd, rm_ref, rv_ref = bn_reference(rs.sum(1), rq.sum(1), cnt, rm0, rv0, eps, mom, True)

    # the reference is the reference's BatchNorm: groups of at least two rows through nn.BatchNorm1d in fp64
    ok = [g for g in range(G) if int(cnt[g]) >= 2]
    bn = torch.nn.BatchNorm1d(width, eps=EPS, momentum=MOMENTUM).double().train()
    with torch.no_grad():
        bn.running_mean.copy_(rm0.double())
        bn.running_var.copy_(rv0.double())
    m2, r2, rm2, rv2 = bn_reference(rs.sum(1)[ok], rq.sum(1)[ok], cnt[ok], rm0, rv0, EPS, MOMENTUM, False)
    worst = 0.0
    for i, g in enumerate(ok):
        xg = x[first[g]:first[g + 1]]
        worst = max(worst, rel_err((xg - m2[i]) * r2[i], bn(xg)))
    worst = max(worst, rel_err(rm2, bn.running_mean), rel_err(rv2, bn.running_var))
    _report(f"C={width} {pair} hand-written formula against nn.BatchNorm1d (CPU, fp64)", worst, 1e-9)
    assert int(bn.num_batches_tracked) == len(ok) >= 3

    ps, pq = Parts(G, P, width, rs), Parts(G, P, width, rq)
    rm, rv = rm0.to(dev()), rv0.to(dev())
    nbt = torch.tensor([5], dtype=torch.int64, device=dev())
    mr = nan(G, 2 * width)
    # nparts and count are ignored with groups: handed values that fit no group
    call_with_parts(ctx, "cartnet_bn_finalize", ps, pq, 99, 12345, width, EPS, MOMENTUM, 1, rm, rv, nbt, mr, ctx.groups(lay),
                    poe, coe)
    t = f"C={width} (parts_over_edges, count_over_edges)={pair}"
    assert bool(torch.isfinite(mr).all())
    _report(t + " mean", rel_err(mr[:, :width], mean), BN_TOL)
    _report(t + " rstd", rel_err(mr[:, width:], rstd), BN_TOL)
    _report(t + " running_mean", rel_err(rm, rm_ref), BN_TOL)
    _report(t + " running_var", rel_err(rv, rv_ref), BN_TOL)
    assert int(nbt) == 5 + G
    flat = torch.tensor(1.0 / f32(EPS) ** 0.5, dtype=torch.float64).float()
    small = [g for g in range(G) if int(cnt[g]) <= 1]
    assert EMPTY in small and ONE_EDGE in small and (not coe or NO_EDGES in small)
    for g in small:
        want = x[first[g]].float() if int(cnt[g]) == 1 else torch.zeros(width)
        assert torch.equal(mr[g, :width].cpu(), want), (t, "mean of a group of 0 / 1 rows", g)
        assert bool((mr[g, width:].cpu() == flat).all()), (t, "rstd of a group of 0 / 1 rows", g)


@pytest.mark.parametrize("width", [4, 20, 256])
def test_bn_finalize_with_groups_eval(ctx, width):
    """training = 0 with groups: every group's row is the running-statistics row, bitwise the same for all groups; the
    running buffers and num_batches_tracked stay as they are."""
    lay = shared()
    gen = torch.Generator().manual_seed(width)
    rm0, rv0 = torch.randn(width, generator=gen), torch.rand(width, generator=gen) + 0.5
    rm, rv = rm0.to(dev()), rv0.to(dev())
    nbt = torch.tensor([5], dtype=torch.int64, device=dev())
    mr = nan(lay.G, 2 * width)
    ctx.call("cartnet_bn_finalize", None, None, 0, 0, width, EPS, MOMENTUM, 0, rm, rv, nbt, mr, ctx.groups(lay), 1, 0)
    assert all(torch.equal(mr[g], mr[0]) for g in range(lay.G))
    assert torch.equal(mr[0, :width].cpu(), rm0)
    _report(f"C={width} eval rstd", rel_err(mr[0, width:], 1.0 / torch.sqrt(rv0.double() + f32(EPS))), BN_TOL)
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and int(nbt) == 5


@pytest.mark.parametrize("over_edges", [1, 0])
@pytest.mark.parametrize("D", WIDTHS)
def test_group_sums_finalize(ctx, D, over_edges):
    """sums[g] = [column sums of group g's rows of parts_a | of parts_b], grad_a / grad_b = the sums over all groups; the
    rows per group are edge_parts = 2 with over_edges, node_parts = 3 without; also with grad_a = grad_b = NULL."""
    lay = shared()
    G, P = lay.G, EDGE_PARTS if over_edges else NODE_PARTS
    gen = torch.Generator().manual_seed(40 + D + over_edges)
    a, b = (torch.randn(G, P, D, generator=gen, dtype=torch.float64) for _ in range(2))
    ref = torch.cat([a.sum(1), b.sum(1)], 1)
    t = f"D={D} over_edges={over_edges}"
    res = []
    for grads in (True, False):
        pa, pb = Parts(G, P, D, a), Parts(G, P, D, b)
        sums, ga, gb = nan(G, 2 * D), nan(D), nan(D)
        call_with_parts(ctx, "cartnet_group_sums_finalize", pa, pb, D, ctx.groups(lay), over_edges, sums,
                        ga if grads else None, gb if grads else None)
        pa.written(t), pb.written(t)
        assert bool(torch.isfinite(sums).all())
        res.append(sums)
        if grads:
            _report(t + " sums", rel_err(sums, ref), SUMS_TOL)
            _report(t + " grad_a", rel_err(ga, a.sum((0, 1))), SUMS_TOL)
            _report(t + " grad_b", rel_err(gb, b.sum((0, 1))), SUMS_TOL)
        else:
            assert bool(ga.isnan().all()) and bool(gb.isnan().all())
    assert torch.equal(res[0], res[1])


@pytest.mark.parametrize("group_size", [1, 2, 3, 7, 9])
def test_group_ptrs(ctx, group_size):
    """node_gptr[g] = graph_ptr[min(g group_size, Bg)], edge_gptr[g] = rowptr[node_gptr[g]] for seven crystals of
    (3, 1, 7, 2, 5, 4, 6) atoms: exact integers; group size 3 leaves a ragged last group, 7 and 9 give G = 1; a G that does
    not match is refused with a message naming it, before any launch."""
    sizes, Bg = (3, 1, 7, 2, 5, 4, 6), 7
    graph_ptr = torch.tensor([0] + list(sizes)).cumsum(0).to(torch.int64)
    N = int(graph_ptr[-1])
    deg = torch.randint(0, 6, (N,), generator=torch.Generator().manual_seed(1))
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).int()
    G = -(-Bg // group_size)
    assert G == {1: 7, 2: 4, 3: 3, 7: 1, 9: 1}[group_size]
    want_n = graph_ptr[[min(g * group_size, Bg) for g in range(G + 1)]].int()
    want_e = rowptr[want_n.long()]
    gp, rp = graph_ptr.to(dev()), rowptr.to(dev())
    ng, eg = (torch.full((G + 2,), -1, dtype=torch.int32, device=dev()) for _ in range(2))
    ctx.call("cartnet_group_ptrs", gp, Bg, group_size, rp, G, ng, eg)
    assert torch.equal(ng[:G + 1].cpu(), want_n) and torch.equal(eg[:G + 1].cpu(), want_e)
    assert int(ng[G + 1]) == -1 and int(eg[G + 1]) == -1
    ng2, eg2 = (torch.full((G + 3,), -1, dtype=torch.int32, device=dev()) for _ in range(2))
    assert ctx.rc("cartnet_group_ptrs", gp, Bg, group_size, rp, G + 1, ng2, eg2) != 0
    assert f"G={G + 1}".encode() in ctx.l.cartnet_last_error()
    assert bool((ng2 == -1).all()) and bool((eg2 == -1).all())


def test_colsum_finalize2_second_destination(ctx):
    """outs2[j] receives the bytes of outs[j]; a NULL entry of outs2, and a NULL outs2, are skipped."""
    nparts, N, jobs = 37, 100, 3
    gen = torch.Generator().manual_seed(2)
    src = [torch.randn(nparts, N, generator=gen, dtype=torch.float64) for _ in range(jobs)]
    arr = lambda ts: (C.c_void_p * jobs)(*[None if t is None else t.data_ptr() for t in ts])
    for second in ("some", "none"):
        parts = [s.to(dev()) for s in src]                               # consumed by the call
        outs = [nan(N) for _ in range(jobs)]
        outs2 = [nan(N), None, nan(N)]
        ctx.call("cartnet_colsum_finalize2", arr(parts), arr(outs), arr(outs2) if second == "some" else None, jobs, nparts, N)
        for j in range(jobs):
            _report(f"colsum_finalize2 outs2={second} job {j}", rel_err(outs[j], src[j].sum(0)), SUMS_TOL)
            if outs2[j] is not None:
                assert torch.equal(outs2[j], outs[j]) if second == "some" else bool(outs2[j].isnan().all())


# --------------------------------------------------------------------------------------------------- 4. a layer, chained
def test_grouped_layer_chain_against_fp64_autograd_micro_batch_by_micro_batch(ctx):
    """The grouped kernel sequence of one layer at D = 256 on the three groups of the shared layout that have at least two
    atoms and two edges (24, 27 and 3 atoms): colstats -> finalize (1, 1) -> gate forward -> finalize (1, 0) -> node update
    forward; node statistics -> group sums (0) -> node apply -> gate statistics -> group sums (1) -> gate apply.  The
    reference is fp64 autograd of the same layer, one micro-batch at a time, through two nn.BatchNorm1d: "results equal G
    separate calls" where a wrong hand-over between two kernels shows.  Bounds: the single kernels' (TOL for x_out and
    e_out, APPLY_TOL for dg | ds, NODE_BWD_TOL for the affine gradients, RUNNING_TOL for the running buffers)."""
    D = 256
    lay = Layout([DEGS, BIG, SMALL])
    G, N, E = lay.G, lay.N, lay.E
    assert int(lay.nodes.min()) >= 2 and int(lay.edges.min()) >= 2
    gen = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=gen)
    k = torch.arange(G, dtype=torch.float32)[lay.gid_edge][:, None]
    gs = r(E, 2 * D)
    gs[:, :D] = gs[:, :D] * (0.6 + 0.4 * k) + 0.5 * k - 0.4            # statistics that differ from group to group
    e_in, de_out, x_in, dx_out, env = r(E, D), r(E, D), r(N, D), r(N, D), torch.rand(E, generator=gen)
    aff = {n: r(D) * 0.5 + (1.0 if n.startswith("w") else 0.0) for n in ("w1", "b1", "w2", "b2")}
    run0 = {"rm1": r(D), "rv1": torch.rand(D, generator=gen) + 0.5, "rm2": r(D), "rv2": torch.rand(D, generator=gen) + 0.5}

    # fp64 autograd, micro-batch by micro-batch
    bn1, bn2 = (torch.nn.BatchNorm1d(D, eps=EPS, momentum=MOMENTUM).double().train() for _ in range(2))
    with torch.no_grad():
        for bn, w, b, rm, rv in ((bn1, "w1", "b1", "rm1", "rv1"), (bn2, "w2", "b2", "rm2", "rv2")):
            bn.weight.copy_(aff[w].double()), bn.bias.copy_(aff[b].double())
            bn.running_mean.copy_(run0[rm].double()), bn.running_var.copy_(run0[rv].double())
    gs64 = gs.double().requires_grad_(True)
    x_ref, e_ref = [], []
    for g in range(G):
        e0, e1, n0, n1 = int(lay.edge_gptr[g]), int(lay.edge_gptr[g + 1]), int(lay.node_gptr[g]), int(lay.node_gptr[g + 1])
        sig = env[e0:e1].double()[:, None] * torch.sigmoid(bn1(gs64[e0:e1, :D]))
        eo = e_in[e0:e1].double() + sig
        aggr = torch.zeros(n1 - n0, D, dtype=torch.float64).index_add(0, lay.tgt[e0:e1] - n0, sig * gs64[e0:e1, D:])
        xo = torch.nn.functional.silu(bn2(aggr)) + x_in[n0:n1].double()
        ((xo * dx_out[n0:n1].double()).sum() + (eo * de_out[e0:e1].double()).sum()).backward()
        x_ref.append(xo.detach()), e_ref.append(eo.detach())

    # the kernels
    grp = ctx.groups(lay)
    d = lambda t: t.to(dev()).contiguous()
    gs_d, e_in_d, de_d, x_in_d, dx_d, env_d = map(d, (gs, e_in, de_out, x_in, dx_out, env))
    w1, b1, w2, b2 = (d(aff[n]) for n in ("w1", "b1", "w2", "b2"))
    rm1, rv1, rm2, rv2 = (d(run0[n]) for n in ("rm1", "rv1", "rm2", "rv2"))
    nbt1, nbt2 = (torch.zeros(1, dtype=torch.int64, device=dev()) for _ in range(2))
    mr1, mr2, sums1, sums2 = (nan(G, 2 * D) for _ in range(4))
    e_out, aggr, x_out, daggr = nan(E, D), nan(N, D), nan(N, D), nan(N, D)
    gw1, gb1, gw2, gb2 = (nan(D) for _ in range(4))
    edge_parts = lambda: (Parts(G, EDGE_PARTS, D), Parts(G, EDGE_PARTS, D))
    node_parts = lambda: (Parts(G, NODE_PARTS, D), Parts(G, NODE_PARTS, D))
    run = lambda name, *a: call_with_parts(ctx, name, *a)
    ps, pq = edge_parts()
    run("cartnet_colstats_grouped", gs_d, 2 * D, D, grp, ps, pq)
    run("cartnet_bn_finalize", ps, pq, 0, 0, D, EPS, MOMENTUM, 1, rm1, rv1, nbt1, mr1, grp, 1, 1)
    ps, pq = edge_parts()
    run("cartnet_gate_scatter_fwd", gs_d, e_in_d, env_d, lay.rowptr_d, mr1, w1, b1, N, D, e_out, aggr, ps, pq, grp)
    run("cartnet_bn_finalize", ps, pq, 0, 0, D, EPS, MOMENTUM, 1, rm2, rv2, nbt2, mr2, grp, 1, 0)
    run("cartnet_node_update_fwd", aggr, x_in_d, mr2, w2, b2, N, D, x_out, grp)
    pa, pb = node_parts()
    run("cartnet_node_update_bwd_stats", aggr, dx_d, mr2, w2, b2, N, D, pa, pb, grp)
    run("cartnet_group_sums_finalize", pa, pb, D, grp, 0, sums2, gb2, gw2)
    run("cartnet_node_update_bwd_apply", aggr, dx_d, mr2, w2, b2, sums2, 1, N, D, daggr, grp)
    pa, pb = edge_parts()
    run("cartnet_gate_scatter_bwd_stats", gs_d, de_d, daggr, env_d, lay.rowptr_d, mr1, w1, b1, N, D, pa, pb, grp)
    run("cartnet_group_sums_finalize", pa, pb, D, grp, 1, sums1, gb1, gw1)
    pdg, pds = edge_parts()
    run("cartnet_gate_scatter_bwd_apply", gs_d, de_d, daggr, env_d, lay.rowptr_d, mr1, w1, b1, sums1, E, 1, N, D, pdg, pds, grp)

    for t in (e_out, x_out, gs_d, gw1, gb1, gw2, gb2, rm1, rv1, rm2, rv2):
        assert bool(torch.isfinite(t).all())
    _report("chain x_out", rel_err(x_out, torch.cat(x_ref)), TOL)
    _report("chain e_out", rel_err(e_out, torch.cat(e_ref)), TOL)
    _report("chain dg | ds", rel_err(gs_d, gs64.grad), APPLY_TOL)
    _report("chain gate BatchNorm weight gradient", rel_err(gw1, bn1.weight.grad), NODE_BWD_TOL)
    _report("chain gate BatchNorm bias gradient", rel_err(gb1, bn1.bias.grad), NODE_BWD_TOL)
    _report("chain node BatchNorm weight gradient", rel_err(gw2, bn2.weight.grad), NODE_BWD_TOL)
    _report("chain node BatchNorm bias gradient", rel_err(gb2, bn2.bias.grad), NODE_BWD_TOL)
    for what, got, ref in (("gate running_mean", rm1, bn1.running_mean), ("gate running_var", rv1, bn1.running_var),
                           ("node running_mean", rm2, bn2.running_mean), ("node running_var", rv2, bn2.running_var)):
        _report("chain " + what, rel_err(got, ref), RUNNING_TOL)
    assert int(nbt1) == int(nbt2) == G == int(bn1.num_batches_tracked)


# --------------------------------------------------------------------------------------------------- 5. sync-BatchNorm steps
@pytest.mark.parametrize("nparts", [0, 1, 300])
@pytest.mark.parametrize("width", [4, 20, 256])
def test_bn_sync_gather(ctx, width, nparts):
    """row[0:C] | row[C:2C] = fp64 column sums of the two partial matrices, row[2C] = the local count exactly, out_a / out_b
    their fp32 roundings; also with both NULL.  C = 20: a second 16-column block with 4 live columns; 300 rows: more
    than the 64 row groups of a block; 0 rows: zeros."""
    gen = torch.Generator().manual_seed(width + nparts)
    a, b = (torch.randn(max(nparts, 1), width, generator=gen, dtype=torch.float64) for _ in range(2))
    ad, bd = a.to(dev()), b.to(dev())
    if nparts == 0:
        ad.fill_(float("nan")), bd.fill_(float("nan"))                  # no row may be read
    ra, rb = (a.sum(0), b.sum(0)) if nparts else (torch.zeros(width, dtype=torch.float64),) * 2
    rows = []
    for outs in (True, False):
        row, oa, ob = nan(2 * width + 2, dtype=torch.float64), nan(width), nan(width)
        ctx.call("cartnet_bn_sync_gather", ad, bd, nparts, width, 123456789, row, oa if outs else None, ob if outs else None)
        assert float(row[2 * width]) == 123456789.0 and bool(row[2 * width + 1].isnan())
        rows.append(row)
        t = f"C={width} nparts={nparts}"
        if not nparts:
            assert not bool(row[:2 * width].any())
        else:
            mass = torch.cat([a.abs().sum(0), b.abs().sum(0)])
            worst = ((row[:2 * width].cpu() - torch.cat([ra, rb])).abs() / mass).max().item()
            _report(t + " |row - ref| / sum |term|", worst, F64_SUM)
        if outs:
            assert torch.equal(oa, row[:width].float()) and torch.equal(ob, row[width:2 * width].float())
        else:
            assert bool(oa.isnan().all()) and bool(ob.isnan().all())
    assert torch.equal(rows[0][:2 * width + 1], rows[1][:2 * width + 1])


def test_bn_sync_scale_with_nothing_anywhere(ctx):
    """a total count of 0 gives zeros, whatever the sums hold"""
    width = 20
    row = torch.randn(2 * width + 1, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    row[2 * width] = 0.0
    sums = nan(2 * width)
    ctx.call("cartnet_bn_sync_scale", row.to(dev()), width, 0, sums)
    assert not bool(sums.any())


@pytest.mark.parametrize("counts", [(13, 7), (20, 0)], ids=["13_and_7_rows", "20_and_0_rows"])
@pytest.mark.parametrize("width", [4, 20, 256])
def test_sync_batchnorm_steps_of_two_ranks_on_one_card(ctx, width, counts):
    """Two "ranks" are two row slices of one [20, C] matrix; the all-reduce is a torch addition of their gathered rows.
    Forward: cartnet_bn_sync_gather per rank, cartnet_bn_finalize_row on the summed row -> mean, rstd and running buffers of
    the union's BatchNorm (1e-6), num_batches_tracked += 1.  Backward: cartnet_node_update_bwd_stats and gather per rank,
    the sum, cartnet_bn_sync_scale (sums = row local / total against fp64, 1e-6), then cartnet_node_update_bwd_apply with
    groups == NULL and training = 1 on each slice: the fp64 BatchNorm backward of the union restricted to the slice
    (2e-5, test_bn_finalize_and_node_update)."""
    N, D = sum(counts), width
    gen = torch.Generator().manual_seed(width + counts[1])
    r = lambda *s: torch.randn(*s, generator=gen)
    aggr, dx, gamma, beta = r(N, D) * 2.0 + 0.5, r(N, D), r(D), r(D)
    rm0, rv0 = r(D), torch.rand(D, generator=gen) + 0.5
    first = [0, counts[0], N]
    aggr_d, dx_d, gamma_d, beta_d = (t.to(dev()) for t in (aggr, dx, gamma, beta))
    at = lambda t, n: t.data_ptr() + n * D * t.element_size()           # row n of a [N, D] tensor (an empty slice included)

    # forward statistics: each rank's rows in three partial rows
    rows = []
    for k in range(2):
        x = aggr[first[k]:first[k + 1]].double()
        ps = torch.stack([x[j::3].sum(0) for j in range(3)]).to(dev())
        pq = torch.stack([(x[j::3] ** 2).sum(0) for j in range(3)]).to(dev())
        row = nan(2 * D + 1, dtype=torch.float64)
        ctx.call("cartnet_bn_sync_gather", ps, pq, 3, D, counts[k], row, None, None)
        rows.append(row)
    total = rows[0] + rows[1]                                          # the all-reduce
    rm, rv = rm0.to(dev()), rv0.to(dev())
    nbt = torch.tensor([5], dtype=torch.int64, device=dev())
    mr = nan(2 * D)
    ctx.call("cartnet_bn_finalize_row", total, D, EPS, MOMENTUM, rm, rv, nbt, mr)
    a64 = aggr.double().requires_grad_(True)
    bn = torch.nn.BatchNorm1d(D, eps=EPS, momentum=MOMENTUM).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma.double()), bn.bias.copy_(beta.double())
        bn.running_mean.copy_(rm0.double()), bn.running_var.copy_(rv0.double())
    xn = bn(a64)
    t = f"C={width} rows={counts}"
    _report(t + " mean", rel_err(mr[:D], a64.mean(0)), BN_TOL)
    _report(t + " rstd", rel_err(mr[D:], torch.rsqrt(a64.var(0, unbiased=False) + EPS)), BN_TOL)
    _report(t + " running_mean", rel_err(rm, bn.running_mean), BN_TOL)
    _report(t + " running_var", rel_err(rv, bn.running_var), BN_TOL)
    assert int(nbt) == 6

    # backward
    (torch.nn.functional.silu(xn) * dx.double()).sum().backward()
    rows, local = [], []
    for k in range(2):
        n = counts[k]
        P = int(ctx.l.cartnet_node_nparts(n))
        pa, pb = nan(P, D, dtype=torch.float64), nan(P, D, dtype=torch.float64)
        ctx.call("cartnet_node_update_bwd_stats", at(aggr_d, first[k]), at(dx_d, first[k]), mr, gamma_d, beta_d, n, D, pa, pb, None)
        assert bool(torch.isfinite(pa).all()) and bool(torch.isfinite(pb).all())
        row, oa, ob = nan(2 * D + 1, dtype=torch.float64), nan(D), nan(D)
        ctx.call("cartnet_bn_sync_gather", pa, pb, P, D, n, row, oa, ob)
        rows.append(row), local.append((oa, ob))
    total = rows[0] + rows[1]
    assert float(total[2 * D]) == N
    # the affine gradients stay local; their sum over the ranks is the union's
    _report(t + " bias gradient, summed over the ranks", rel_err(local[0][0] + local[1][0], bn.bias.grad), NODE_BWD_TOL)
    _report(t + " weight gradient, summed over the ranks", rel_err(local[0][1] + local[1][1], bn.weight.grad), NODE_BWD_TOL)
    for k in range(2):
        n = counts[k]
        sums = nan(2 * D)
        ctx.call("cartnet_bn_sync_scale", total, D, n, sums)
        _report(t + f" rank {k} scaled sums", rel_err(sums, total[:2 * D].cpu() * (n / N)), SUMS_TOL)
        if n == 0:
            assert not bool(sums.any())
        daggr = nan(N, D)
        ctx.call("cartnet_node_update_bwd_apply", at(aggr_d, first[k]), at(dx_d, first[k]), mr, gamma_d, beta_d, sums, 1, n, D,
                 at(daggr, first[k]), None)
        mine = torch.zeros(N, dtype=torch.bool)
        mine[first[k]:first[k + 1]] = True
        assert bool(daggr[~mine.to(dev())].isnan().all())                     # nothing outside the rank's slice
        if n:
            _report(t + f" rank {k} daggr", rel_err(daggr[mine.to(dev())], a64.grad[mine]), NODE_BWD_TOL)

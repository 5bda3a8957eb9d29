"""The bf16-storage ("half storage") kernels of csrc/edge_ops.hip against fp64, at fp32-level bounds, and the launch paths of
the gate kernels and the segment sums that no model-sized test reaches.

cartnet_gate_scatter_fwd_h / _bwd_stats_h / _bwd_apply_h and cartnet_segment_sum_pair_h read (and the apply pass writes)
bf16 rows; their arithmetic is the fp32 kernels'.  So every reference here is fp64 on the CPU, built from exactly the
values the kernel reads -- the bf16 tensors widened to fp64, the fp32 statistics as passed -- and the bounds are the fp32
kernels' own (tests/test_gpu_kernels.py), plus half a bf16 ulp where a result is stored as bf16.  Output buffers start as
NaN (7.0 where they are views of a wider buffer), so an element that is not written, or one written outside the view,
shows.  Every check prints its figure before it asserts.

Measured on an MI355X (worst over all cases): forward e_out 7.2e-8, aggr 2.3e-7, column sums 2.2e-7; backward statistics
2.1e-7; the stored bf16 dg | ds never more than half a bf16 ulp from fp64 (excess <= 1.4e-11 of max|r|) and different
from bf16(fp64) in at most 4.8e-5 of the elements; column sums of ds 1.1e-7, of dg 1.8e-7 (eval) and 9.7e-8 of sum |dg|
(training); the multi-sweep launches 2.2e-7 or less throughout; every segment sum bitwise.
"""
import functools

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5                   # test_gpu_kernels.TOL: fp32 arithmetic against fp64
APPLY_TOL = 2e-5             # test_gate_scatter_fwd_bwd: dg | ds
APPLY_SUM_TOL = 1e-4         # ... and their column sums
HALF_ULP = 2.0 ** -8         # bf16 keeps 8 significant bits: round-to-nearest is off by at most 2^-8 |r| (half an ulp)
MISMATCH_CAP = 0.01          # share of stored bf16 values that may differ from the rounded fp64 reference: an fp32
#                              evaluation of the same formula differs in 5e-5 ... 7e-5 of them (a value within fp32 error of
#                              a rounding boundary), truncation instead of round-to-nearest-even in half of them

DEGS = list(range(18)) + [24, 40, 0, 8, 16, 1]      # 24 atoms, 242 edges: every remainder of the 8-edge rounds, twice


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


def _graph(degs, crystal=512, seed=0):
    """Crystals of ``crystal`` consecutive atoms (the last one smaller); atom t has degs[t] incoming edges whose sources are
    drawn from its own crystal; target-sorted.  Returns edge_index [2, E] and graph_ptr (int64, CPU)."""
    g = torch.Generator().manual_seed(seed)
    degs = torch.as_tensor(degs, dtype=torch.int64)
    n = int(degs.numel())
    tgt = torch.repeat_interleave(torch.arange(n), degs)
    base = tgt // crystal * crystal
    size = torch.clamp(n - base, max=crystal)
    src = base + torch.randint(0, 2 ** 31 - 1, (int(tgt.numel()),), generator=g) % size
    ptr = torch.cat([torch.arange(0, n, crystal), torch.tensor([n])]).to(torch.int64)
    return torch.stack([src, tgt]).to(torch.int64), ptr


class _Gate:
    """Inputs of the three gate kernels on one graph (CPU masters: gs as bf16, the rest fp32; mean_rstd = the batch
    statistics of the gate half in fp64, cast to fp32) and the fp64 formulas on the values the kernels read."""

    def __init__(self, degs, D, seed):
        self.ei, self.ptr = _graph(degs, seed=seed)
        self.N, self.E, self.D = len(degs), int(self.ei.shape[1]), D
        self.deg = torch.as_tensor(degs)
        g = torch.Generator().manual_seed(seed + 1)
        r = lambda *s: torch.randn(*s, generator=g)
        self.gs16 = r(self.E, 2 * D).bfloat16()
        self.e_in, self.de_out, self.daggr = r(self.E, D), r(self.E, D), r(self.N, D)
        self.env = torch.rand(self.E, generator=g)
        self.gamma, self.beta = r(D), r(D)
        g64 = self.gs16[:, :D].double()
        self.mean_rstd = torch.cat([g64.mean(0), torch.rsqrt(g64.var(0, unbiased=False) + 1e-5)]).float().contiguous()
        # fp64 views of what the kernels read
        self.tgt = self.ei[1]
        self.g, self.s = g64, self.gs16[:, D:].double()
        mean, self.rstd = self.mean_rstd[:D].double(), self.mean_rstd[D:].double()
        self.ghat = (self.g - mean) * self.rstd
        self.z = torch.sigmoid(self.ghat * self.gamma.double() + self.beta.double())
        self._dev = {}

    def d(self, name):
        if name not in self._dev:
            self._dev[name] = getattr(self, name).to(dev()).contiguous()
        return self._dev[name]

    def layout(self, ops):
        if "lay" not in self._dev:
            self._dev["lay"] = ops.GraphLayout(self.ei.to(dev()), self.N, self.ptr.to(dev()))
            self._dev["lay"].validate()
        return self._dev["lay"]

    def gs(self, dtype):
        return self.gs16.to(dtype).to(dev()).clone()               # a fresh copy: the apply pass overwrites it

    def ev(self, env):
        return self.env.double()[:, None] if env else 1.0

    def fwd(self, env=True):
        sig = self.ev(env) * self.z
        aggr = torch.zeros(self.N, self.D, dtype=torch.float64).index_add_(0, self.tgt, sig * self.s)
        return self.e_in.double() + sig, aggr

    def dbn(self, env=True, de=True):
        dsig = self.daggr.double()[self.tgt] * self.s + (self.de_out.double() if de else 0.0)
        return dsig * self.ev(env) * self.z * (1.0 - self.z)

    def sums(self):
        """[sum dbn | sum dbn ghat] as the fp32 vector the apply pass is given."""
        dbn = self.dbn()
        return torch.cat([dbn.sum(0), (dbn * self.ghat).sum(0)]).float().contiguous()

    def apply(self, training):
        inv = 1.0 / self.E if training else 0.0
        sums = self.sums().double()
        m_a, m_b = sums[:self.D] * inv, sums[self.D:] * inv
        dg = self.gamma.double() * self.rstd * (self.dbn() - m_a - self.ghat * m_b)
        ds = self.daggr.double()[self.tgt] * self.ev(True) * self.z
        return dg, ds


@functools.lru_cache(maxsize=None)
def _small(D):
    return _Gate(DEGS, D, seed=100 + D)


@functools.lru_cache(maxsize=None)
def _multi_sweep():
    # 8197 atoms: cartnet_gate_scatter_nparts caps the grid at 1024 workgroups of 4 atoms, so a workgroup makes
    # ceil(8197 / 4096) = 3 sweeps, the last one over 5 atoms only
    return _Gate([(7 * i) % 4 for i in range(2 * 4096 + 5)], 64, seed=7)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev())


def _parts(ops, c):
    return _nan(ops.gate_nparts(c.N) * c.D, dtype=torch.float64)


def _colsum(p, c):
    return p.view(-1, c.D).sum(0)


def _report(what, err, bound):
    print(f"{what}: {err:.3g} (bound {bound:g})")
    assert err < bound, (what, err)


def _check_forward(ops, c, dtype, tag):
    lay = c.layout(ops)
    for env, with_e in ((True, True), (False, True), (True, False)):
        e_out = _nan(c.E, c.D) if with_e else None
        aggr, ps, pq = _nan(c.N, c.D), _parts(ops, c), _parts(ops, c)
        ops.gate_scatter_fwd(c.gs(dtype), c.d("e_in") if with_e else None, c.d("env") if env else None, lay,
                             c.d("mean_rstd"), c.d("gamma"), c.d("beta"), e_out, aggr, ps, pq)
        eo_ref, ag_ref = c.fwd(env)
        t = f"{tag} fwd env={env} e_out={with_e}"
        if with_e:
            _report(t + " e_out", rel_err(e_out, eo_ref), TOL)
        _report(t + " aggr", rel_err(aggr, ag_ref), TOL)
        _report(t + " parts_sum", rel_err(_colsum(ps, c), ag_ref.sum(0)), TOL)
        _report(t + " parts_sq", rel_err(_colsum(pq, c), (ag_ref ** 2).sum(0)), TOL)
        empty = (c.deg == 0).to(dev())
        assert int(empty.sum()) > 0 and not aggr[empty].any()          # exact zeros


def _check_stats(ops, c, dtype, tag):
    lay = c.layout(ops)
    for env, de in ((True, True), (True, False), (False, True)):
        pa, pb = _parts(ops, c), _parts(ops, c)
        ops.gate_scatter_bwd_stats(c.gs(dtype), c.d("de_out") if de else None, c.d("daggr"), c.d("env") if env else None,
                                   lay, c.d("mean_rstd"), c.d("gamma"), c.d("beta"), pa, pb)
        dbn = c.dbn(env, de)
        t = f"{tag} stats env={env} de_out={de}"
        _report(t + " sum dbn", rel_err(_colsum(pa, c), dbn.sum(0)), TOL)
        _report(t + " sum dbn ghat", rel_err(_colsum(pb, c), (dbn * c.ghat).sum(0)), TOL)


def _check_apply(ops, c, dtype, training, tag):
    lay = c.layout(ops)
    gs = c.gs(dtype)
    pdg, pds = _parts(ops, c), _parts(ops, c)
    ops.gate_scatter_bwd_apply(gs, c.d("de_out"), c.d("daggr"), c.d("env"), lay, c.d("mean_rstd"), c.d("gamma"),
                               c.d("beta"), c.sums().to(dev()), training, pdg, pds)
    dg, ds = c.apply(training)
    r = torch.cat([dg, ds], 1)
    out = gs.double().cpu()
    t = f"{tag} apply training={training}"
    assert gs.dtype == dtype and torch.isfinite(out).all()
    if dtype == torch.bfloat16:
        # the stored dg | ds is the round-to-nearest-even of the fp32 result
        excess = ((out - r).abs() - HALF_ULP * r.abs()).max().item() / r.abs().max().item()
        _report(t + " (|out - r| - 2^-8 |r|) / max|r|", excess, APPLY_TOL)
        assert ((out - r).abs() <= HALF_ULP * r.abs() + APPLY_TOL * r.abs().max()).all()
        share = (gs.cpu() != r.bfloat16()).double().mean().item()
        _report(t + " share of out != bf16(r)", share, MISMATCH_CAP)
    else:
        _report(t + " dg | ds", rel_err(out, r), APPLY_TOL)
    _report(t + " parts_ds", rel_err(_colsum(pds, c), ds.sum(0)), APPLY_SUM_TOL)
    if training:
        # sum dg is 0 up to the rounding of the statistics: bounded per column against sum |dg|
        worst = ((_colsum(pdg, c).cpu() - dg.sum(0)).abs() / dg.abs().sum(0)).max().item()
        _report(t + " |sum dg - ref| / sum |dg|, worst column", worst, APPLY_SUM_TOL)
    else:
        _report(t + " parts_dg", rel_err(_colsum(pdg, c), dg.sum(0)), APPLY_SUM_TOL)


# --------------------------------------------------------------------------------------------------- 1. gate kernels, bf16
# D = 64: a quarter of the lanes; 256: one full pass; 320: a second 256-column pass with 48 of 64 lanes idle; 512: two full
# passes.  No groups (groups == NULL), the launch of the plain half-storage model.
@pytest.mark.parametrize("D", [64, 256, 320, 512])
def test_gate_forward_bf16_gs_against_fp64(ops, D):
    """cartnet_gate_scatter_fwd_h, in-degrees 0..17, 24, 40, 0, 8, 16, 1: e_out, aggr and the column sums of aggr and
    aggr^2 within 1e-5 of fp64 on the widened bf16 values; also without the envelope and without e_in / e_out; the atoms
    without edges aggregate exact zeros."""
    _check_forward(ops, _small(D), torch.bfloat16, f"D={D} bf16")


@pytest.mark.parametrize("D", [64, 256, 320, 512])
def test_gate_backward_statistics_bf16_gs_against_fp64(ops, D):
    """cartnet_gate_scatter_bwd_stats_h: sum dbn and sum dbn ghat within 1e-5 of fp64; also with de_out = NULL and with
    env = NULL."""
    _check_stats(ops, _small(D), torch.bfloat16, f"D={D} bf16")


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("D", [64, 256, 320, 512])
def test_gate_backward_apply_bf16_gs_is_the_rounded_fp32_result(ops, D, training):
    """cartnet_gate_scatter_bwd_apply_h alone (its ``sums`` are the fp64 reference's, cast to fp32): the stored bf16 dg | ds
    is within half a bf16 ulp plus the fp32 apply tolerance of fp64, element by element, and differs from the fp64 result
    rounded to bf16 in at most 1 % of the elements (truncating stores differ in half).  parts_dg / parts_ds are the column
    sums of the fp32 values BEFORE they are rounded for the store, so they keep the fp32 kernel's 1e-4; in training mode
    sum dg is 0 in exact arithmetic and is bounded against sum |dg| per column instead."""
    _check_apply(ops, _small(D), torch.bfloat16, training, f"D={D} bf16")


# --------------------------------------------------------------------------------------------------- 2. multi-sweep launches
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_gate_kernels_over_more_than_one_sweep(ops, dtype):
    """8197 atoms (in-degrees (7 i) % 4, D = 64): the grid is capped at 1024 workgroups of 4 atoms, so each makes three
    sweeps -- descending in the forward and the apply pass -- and the last covers 5 atoms.  Forward, statistics and apply
    (training and eval) at the bounds of part 1; the fp32 form, whose gs holds the same bf16-representable values, gets
    the fp32 apply tolerance on dg | ds itself."""
    c = _multi_sweep()
    assert ops.gate_nparts(c.N) * 4 * 2 < c.N
    tag = "multi-sweep " + ("bf16" if dtype == torch.bfloat16 else "fp32")
    _check_forward(ops, c, dtype, tag)
    _check_stats(ops, c, dtype, tag)
    for training in (True, False):
        _check_apply(ops, c, dtype, training, tag)


# --------------------------------------------------------------------------------------------------- 3. segment_sum_pair, bf16
def _int_rows(E, W, seed, dtype):
    return torch.randint(-8, 9, (E, W), generator=torch.Generator().manual_seed(seed)).to(dtype)


@pytest.mark.parametrize("W", [256, 320, 512, 1024])
def test_segment_sum_pair_bf16_rows_every_batch_remainder_is_exact(ops, W):
    """cartnet_segment_sum_pair_h with segment lengths 0..17, 24, 40, 0, 8, 16, 1 (8 rows per round, a clamped remainder
    round) and integer-valued bf16 rows: exact sums, compared bitwise, by target and by source, into the two halves of one
    [N, 2W] matrix.  With 24 atoms W = 256 takes the plain grid (12 workgroups < 8 runs of 2) and W = 320, 512, 1024 the
    grid dealt by XCD (24, 24, 48 workgroups = 8 runs of 3, 3, 6).  W = 512 and 1024 also with ochunk = 512 (iComformer's
    interleaved layout; the model's 2D = 1024 at D = 512)."""
    ei, ptr = _graph(DEGS, seed=W)
    N, E = len(DEGS), ei.shape[1]
    lay = ops.GraphLayout(ei.to(dev()), N, ptr.to(dev()))
    rows = _int_rows(E, W, 1, torch.bfloat16)
    ref_t = torch.zeros(N, W).index_add_(0, ei[1], rows.float())
    ref_s = torch.zeros(N, W).index_add_(0, ei[0], rows.float())
    both = torch.full((N, 2 * W), 7.0, device=dev())
    ops.segment_sum_pair(rows.to(dev()), lay, both[:, :W], both[:, W:])
    assert torch.equal(both[:, :W].cpu(), ref_t) and torch.equal(both[:, W:].cpu(), ref_s)
    if W in (512, 1024):     # chunk j of 256 columns at column j * 512 -> [t0 | s0 | t1 | s1 | ...]
        inter = torch.full((N, 2 * W), 7.0, device=dev())
        ops.segment_sum_pair(rows.to(dev()), lay, inter[:, :2 * W - 256], inter[:, 256:], ochunk=512)
        want = torch.cat([r[:, j:j + 256] for j in range(0, W, 256) for r in (ref_t, ref_s)], 1)
        assert torch.equal(inter.cpu(), want)


def test_segment_sum_pair_bf16_rows_as_a_column_view(ops):
    """ld > W: the rows are columns [64, 384) of a [E, 512] bf16 matrix (W = 320: a partial second chunk)."""
    W = 320
    ei, ptr = _graph(DEGS, seed=5)
    N, E = len(DEGS), ei.shape[1]
    lay = ops.GraphLayout(ei.to(dev()), N, ptr.to(dev()))
    wide = _int_rows(E, 512, 2, torch.bfloat16)
    rows = wide[:, 64:64 + W]
    ref_t = torch.zeros(N, W).index_add_(0, ei[1], rows.float())
    ref_s = torch.zeros(N, W).index_add_(0, ei[0], rows.float())
    both = torch.full((N, 2 * W), 7.0, device=dev())
    ops.segment_sum_pair(wide.to(dev())[:, 64:64 + W], lay, both[:, :W], both[:, W:])
    assert torch.equal(both[:, :W].cpu(), ref_t) and torch.equal(both[:, W:].cpu(), ref_s)


# --------------------------------------------------------------------------------------------------- 4. grid-capped sums
@functools.lru_cache(maxsize=None)
def _capped(N):
    return _graph([(5 * i) % 3 for i in range(N)], seed=N)


def test_segment_sum_beyond_the_grid_cap(ops):
    """262181 segments of 4 columns: 65546 workgroups' worth of items on a grid capped at 65536, so the first ten
    workgroups take a second item -- by target in ascending order, through the permutation in descending order.  Integer
    rows (columns [0, 4) of a [E, 8] matrix), bitwise against index_add_; the other half of the output rows stays as it was."""
    N, W = 262144 + 37, 4
    ei, ptr = _capped(N)
    E = ei.shape[1]
    lay = ops.GraphLayout(ei.to(dev()), N, ptr.to(dev()))
    lay.validate()
    wide = _int_rows(E, 2 * W, 3, torch.float32)
    rows = wide.to(dev())[:, :W]
    for perm, idx in ((None, ei[1]), (lay.perm, ei[0])):
        out = torch.full((N, 2 * W), 7.0, device=dev())
        ops.segment_sum(rows, lay.rowptr if perm is None else lay.colptr, perm, out[:, :W])
        ref = torch.zeros(N, W).index_add_(0, idx, wide[:, :W])
        assert torch.equal(out[:, :W].cpu(), ref), "by target" if perm is None else "by source"
        assert bool((out[:, W:] == 7.0).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_segment_sum_pair_beyond_the_grid_cap(ops, dtype):
    """131109 atoms, 4 columns: 262218 items > 4 * 65536, and the XCD-dealt grid would need 65560 > 65536 workgroups, so the
    plain grid-stride path runs on 65536 workgroups.  Both sums bitwise, fp32 and bf16 rows."""
    N, W = 131072 + 37, 4
    ei, ptr = _capped(N)
    E = ei.shape[1]
    lay = ops.GraphLayout(ei.to(dev()), N, ptr.to(dev()))
    lay.validate()
    rows = _int_rows(E, W, 4, dtype)
    both = torch.full((N, 2 * W), 7.0, device=dev())
    ops.segment_sum_pair(rows.to(dev()), lay, both[:, :W], both[:, W:])
    ref_t = torch.zeros(N, W).index_add_(0, ei[1], rows.float())
    ref_s = torch.zeros(N, W).index_add_(0, ei[0], rows.float())
    assert torch.equal(both[:, :W].cpu(), ref_t) and torch.equal(both[:, W:].cpu(), ref_s)


def test_gate_wrappers_refuse_bc_with_bf16_gs(ops):
    c = _small(64)
    with pytest.raises(ValueError, match="bc"):
        ops.gate_scatter_fwd(c.gs(torch.bfloat16), None, None, c.layout(ops), c.d("mean_rstd"), c.d("gamma"), c.d("beta"),
                             None, _nan(c.N, c.D), _parts(ops, c), _parts(ops, c), bc=_nan(c.N, 2 * c.D))

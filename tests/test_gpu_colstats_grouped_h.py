"""cartnet_colstats_grouped_h through the C ABI: per-group column sums / sums of squares over rows kept as bf16 (the gate
half of gs when BatchNorm groups meet half storage), against fp64 sums of the same bf16 values in torch.

Five groups of (0, 1, 3, 17, 1030) rows: an empty group, one row, fewer rows than the four waves of a workgroup, and more
rows than one unrolled sweep of the grid (edge_parts x 4 waves x 8 rows = 96 at three parts).  C = 8 (two active lanes),
256 (exactly one column pass), 520 (a second, partly filled pass); ld = 2C + 8, and the base is 8 bytes past a 16-byte
boundary -- all the alignment the entry point asks for.

Tolerance.  The kernel accumulates in fp64.  A bf16 value is an 8-bit integer times a power of two; the non-zero values
here lie between 2^-24 and 2^13 (asserted below), so every partial sum of at most 1030 of them is an integer multiple
of 2^-31 below 2^23: 54 bits at the very worst, and the random columns stay below 2^13 -- exactly representable, whatever
the order.  The squares carry 16 bits each and may round in the last place after a few hundred terms: n * 2^-53 <
1.2e-13 relative for positive terms.  So every per-group total must match torch's fp64 total to 1e-12 of its own value,
element by element (an empty group: exactly zero)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = (0, 1, 3, 17, 1030)
WIDTHS = (8, 256, 520)
BIG = 4096.0                     # column 1 of every row: var = E[v^2] - mean^2 cancels to zero exactly, or not at all
REL = 1e-12


def dev():
    return torch.device("cuda:0")


class Ctx:
    def __init__(self):
        from cartnet_amd import lib
        self.lib, self.l = lib, lib.load()
        self.G, self.R = len(ROWS), int(sum(ROWS))
        self.gptr = torch.tensor([0] + list(ROWS)).cumsum(0).int().to(dev())
        self.gid = torch.repeat_interleave(torch.arange(self.G), torch.tensor(ROWS))

    def groups(self, parts):
        g = self.lib.Groups()
        g.node_gptr, g.edge_gptr, g.G, g.edge_parts, g.node_parts = self.gptr.data_ptr(), self.gptr.data_ptr(), self.G, parts, parts
        return g

    def rc(self, name, x_ptr, ld, width, groups, ps, pq):
        rc = getattr(self.l, name)(x_ptr, ld, width, C.addressof(groups) if groups is not None else None, ps.data_ptr(),
                                   pq.data_ptr(), self.lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def call(self, name, *args):
        self.lib.check(self.rc(name, *args), name)

    def parts(self, parts, width):
        return (torch.full((self.G * parts, width), float("nan"), dtype=torch.float64, device=dev()) for _ in range(2))


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


@pytest.fixture(scope="module")
def rows(ctx):
    """width -> (bf16 buffer on the device, pointer to its first element, ld, the values as fp64 [R, C], fp64 group sums of
    the values and of their squares) -- computed once, never written again."""
    out = {}
    for width in WIDTHS:
        ld = 2 * width + 8
        x = torch.randn(ctx.R, width, generator=torch.Generator().manual_seed(width)).bfloat16()
        x[:, 1] = BIG
        buf = torch.zeros(ctx.R * ld + 4, dtype=torch.bfloat16)
        buf[4:].view(ctx.R, ld)[:, :width] = x                  # the rows start 4 elements = 8 bytes into the buffer
        buf[4:].view(ctx.R, ld)[:, width:] = float("nan")        # the padding must never be read
        bd = buf.to(dev())
        assert bd.data_ptr() % 16 == 0
        x64 = x.double()
        assert float(x64.abs()[x64 != 0].min()) >= 2.0 ** -24       # what the exactness argument above assumes
        sums = torch.zeros(ctx.G, width, dtype=torch.float64).index_add_(0, ctx.gid, x64)
        sqs = torch.zeros(ctx.G, width, dtype=torch.float64).index_add_(0, ctx.gid, x64 * x64)
        out[width] = (bd, bd.data_ptr() + 8, ld, x64, sums, sqs)
    return out


def same(got, ref, what):
    got = got.cpu()
    err = (got - ref).abs()
    worst = float((err / ref.abs().clamp_min(1e-300)).max())
    print(f"{what}: max relative difference {worst:.3g} (bound {REL:g})")
    assert bool((err <= REL * ref.abs()).all()), (what, worst)


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("width", WIDTHS)
def test_group_totals_match_fp64_sums_of_the_stored_values(ctx, rows, width, parts):
    bd, ptr, ld, x64, sums, sqs = rows[width]
    g = ctx.groups(parts)
    ps, pq = ctx.parts(parts, width)
    ctx.call("cartnet_colstats_grouped_h", ptr, ld, width, g, ps, pq)
    assert torch.isfinite(ps).all() and torch.isfinite(pq).all(), "every partial row is written (and no padding read)"
    ps3, pq3 = ps.view(ctx.G, parts, width), pq.view(ctx.G, parts, width)
    same(ps3.sum(1), sums, "sums")
    same(pq3.sum(1), sqs, "sums of squares")
    # the empty group's rows are zeros, not leftovers
    empty = ROWS.index(0)
    assert not ps3[empty].any() and not pq3[empty].any()
    # the cancellation column: n * BIG and n * BIG^2 exactly, so that var = q / n - (s / n)^2 is exactly 0
    n = torch.tensor(ROWS, dtype=torch.float64)
    assert torch.equal(ps3.sum(1)[:, 1].cpu(), n * BIG) and torch.equal(pq3.sum(1)[:, 1].cpu(), n * BIG * BIG)
    # fixed order, no atomics: the same bytes again
    ps2, pq2 = ctx.parts(parts, width)
    ctx.call("cartnet_colstats_grouped_h", ptr, ld, width, g, ps2, pq2)
    assert torch.equal(ps, ps2) and torch.equal(pq, pq2)


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("width", WIDTHS)
def test_same_totals_as_the_fp32_form_on_the_same_values(ctx, rows, width, parts):
    bd, ptr, ld, x64, sums, sqs = rows[width]
    g = ctx.groups(parts)
    ps, pq = ctx.parts(parts, width)
    ctx.call("cartnet_colstats_grouped_h", ptr, ld, width, g, ps, pq)
    xf = torch.full((ctx.R, ld), float("nan"))
    xf[:, :width] = x64.float()                                   # bf16 -> fp32 is exact
    xf = xf.to(dev())
    fs, fq = ctx.parts(parts, width)
    ctx.call("cartnet_colstats_grouped", xf.data_ptr(), ld, width, g, fs, fq)
    same(ps.view(ctx.G, parts, width).sum(1), fs.view(ctx.G, parts, width).sum(1).cpu(), "sums, bf16 rows vs fp32 rows")
    same(pq.view(ctx.G, parts, width).sum(1), fq.view(ctx.G, parts, width).sum(1).cpu(), "squares, bf16 rows vs fp32 rows")


def test_bad_arguments_are_refused_before_any_launch(ctx, rows):
    bd, ptr, ld, *_ = rows[8]
    g = ctx.groups(1)
    ps, pq = ctx.parts(1, 8)
    assert ctx.rc("cartnet_colstats_grouped_h", ptr, ld, 8, None, ps, pq) != 0                # groups are required
    assert b"groups" in ctx.l.cartnet_last_error()
    assert ctx.rc("cartnet_colstats_grouped_h", ptr, ld, 6, g, ps, pq) != 0                   # C % 4
    assert b"multiples of 4" in ctx.l.cartnet_last_error()
    assert ctx.rc("cartnet_colstats_grouped_h", ptr, 6, 8, g, ps, pq) != 0                    # ld < C
    assert ctx.rc("cartnet_colstats_grouped_h", ptr + 2, ld, 8, g, ps, pq) != 0               # not 8-byte aligned
    with pytest.raises(ctx.lib.CartnetHipError, match="cartnet_colstats_grouped_h"):
        ctx.call("cartnet_colstats_grouped_h", ptr, ld, 6, g, ps, pq)
    # nothing was launched: the NaN-filled outputs are untouched
    assert bool(ps.isnan().all()) and bool(pq.isnan().all())

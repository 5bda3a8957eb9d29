"""Every case of tests/gemm_cases.py on the GPU: first the kernel family the plan gives (ops.gemm_plan, the code
cartnet_gemm plans with), then the launch against ``gemm_ref64``, the fp64 statement of the CartnetGemmArgs contract.

Bounds are the ones the suite already applies to each kind of result (no new tolerance):

* outputs at precision 0 / 1: TOL = 1e-5 of max|ref|;
* precision 2 on a bf16 kernel, against fp64 products of the bf16-rounded operands: 1e-6, and 1e-3 with SiLU on an
  operand (the kernel's own SiLU may round a few operands the other way); 1e-5 where the epilogue multiplies by an fp32
  silu' / sigmoid factor (H_DACT of tests/test_gpu_kernels.py);
* a_act_out: 1e-6; the fp64 column-sum partials: 1e-6 of the sums of the values the launch stored, row tile by row tile;
  the gate-statistics sums: 2e-6 (tests/test_gpu_kernels.py::test_gate_backward_sums_without_the_statistics_pass);
* every padding column of an output view (ld > N) still holds its sentinel;
* every row-indexed buffer has 160 rows behind its last (gemm_cases.TAIL): NaN behind the inputs (A, the tn layout's B,
  resid, dact, the gate-statistics operands), index 0 behind tgt / src, the sentinel behind the outputs.  A ragged last
  tile, a column-sum or gate-statistics epilogue or a split-K slab that takes in a row past M (or K) turns its figure
  into NaN, which fails every bound; the output tails must still hold the sentinel.

Per output tile (128 rows by the family's tile width) the worst error normalised by that tile's own max|ref| is printed
and asserted too: with the whole-matrix constant where the worst figure recorded for the family is at most a quarter of
it, else with four times the recorded figure (fixed inputs leave only summation-order freedom).  PER_TILE_RECORDED holds
those figures: the worst per family and whole-matrix bound over all cases, measured once on an MI355X against fp64 with
the kernels of the parent commit (this file adds no kernel change).
"""
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

TOL = 1e-5           # precision 0 / 1 (tests/test_gpu_kernels.py)
H_PLAIN = 1e-6       # precision 2, no SiLU on an operand: only the fp32 accumulation differs
H_ACT = 1e-3         # precision 2, SiLU on an operand
H_DACT = 1e-5        # precision 2, an fp32 silu' / sigmoid factor in the epilogue
ACT_OUT = 1e-6       # a_act_out against fp64 SiLU
SUMS = 1e-6          # fp64 column-sum partials against the sums of the stored values
GATE_SUMS = 2e-6     # gate-statistics sums

# worst per-tile error / that tile's max|ref| per "family@whole-matrix bound", MI355X, parent commit's kernels
PER_TILE_RECORDED = {
    "general64@1e-05": 4.04e-07, "general128@1e-05": 4.92e-07, "general256@1e-05": 3.36e-07, "general_x3@1e-05": 2.84e-07,
    "f32p@1e-05": 1.53e-06, "f32nn@1e-05": 9.45e-07, "f32nn_actout@1e-05": 9.87e-07, "f32nn128@1e-05": 1.71e-06,
    "f32tn@1e-05": 8.80e-07, "x3nn16@1e-05": 1.00e-06, "x3nn_actout@1e-05": 9.85e-07, "x3tn@1e-05": 7.35e-07,
    # precision 2, against the bf16-rounded operands
    "x3nn@1e-06": 2.39e-07, "x3nn@1e-05": 1.98e-07, "x3nn@0.001": 1.63e-07, "x3nn_actout@0.001": 6.50e-08,
    "x3tn@1e-06": 1.77e-07, "x3tn@0.001": 7.78e-08,
}
# (every figure is at most a quarter of its whole-matrix bound, so each per-tile bound is that constant; the worst whole-matrix
#  figures of the same run: 1.33e-6 at TOL (f32p, K = 768), 2.39e-7 at 1e-6 (x3nn, K = 528); a_act_out 1.26e-7; column-sum
#  partials 1.99e-7; gate-statistics sums and partials 1.84e-7.  hnn / htn: tests/test_gpu_kernels.py, unchanged bounds.)


def per_tile_bound(family, whole):
    rec = PER_TILE_RECORDED.get(f"{family}@{whole:g}")
    if rec is None or rec <= whole / 4:
        return whole
    return 4 * rec


def whole_bound(c):
    if not gc.bf16_products(c):
        return TOL
    if c.a_act or c.b_act:
        return H_ACT
    return H_DACT if ("dact" in c.epi or c.out_act) else H_PLAIN


def tile_errors(got, ref, width):
    """max|got - ref| per (128 x width) tile / that tile's max|ref| -> the worst of them."""
    M, N = ref.shape
    tm, tn = -(-M // gc.BM), -(-N // width)

    def tiles(x):
        p = torch.zeros(tm * gc.BM, tn * width, dtype=torch.float64)
        p[:M, :N] = x
        return p.view(tm, gc.BM, tn, width).abs().amax(dim=(1, 3))
    err, scale = tiles(got - ref), tiles(ref)
    assert bool((scale > 0).all())
    return float((err / scale).max())


def rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.fixture(scope="module")
def ops():
    from cartnet_amd import lib, ops as _ops
    lib.load()
    return _ops


@pytest.mark.parametrize("c", gc.CASES, ids=lambda c: c.name)
def test_case_reaches_its_family_and_matches_fp64(ops, c):
    dev = torch.device("cuda:0")
    t = gc.make_tensors(c, dev)
    A, B, C, kw = gc.gemm_kwargs(c, t, ops)
    plan = ops.gemm_plan(A, B, C, **kw)
    assert plan.family == c.family, plan                     # the family first: a rerouted case proves nothing below
    assert plan.width == gc.width_of(c.family)
    ops.gemm(A, B, C, **kw)
    torch.cuda.synchronize()
    ref = gc.gemm_ref64(c, t)
    cpu = lambda x: x.detach().double().cpu()
    whole, bad = whole_bound(c), []
    tile = per_tile_bound(c.family, whole)

    def fig(what, err, bound):
        print(f"GEMMFIG case={c.name} family={c.family} what={what} err={err:.3g} bound={bound:g}")
        if not err < bound:
            bad.append((what, err, bound))
    outputs = [("C", C, ref["C"])]
    if "cpre" in c.epi:
        outputs.append(("cpre", gc.views(c, t, "cpre"), ref["cpre"]))
    stored = {}
    for name, got, want in outputs:
        for g in range(c.groups):
            x = cpu(got[g])
            if c.splitk > 1:                                  # raw partial slabs: their sum is the product
                assert bool(torch.isfinite(x).all()), "a slab was not written"
                x = x.view(c.splitk, c.M, c.N).sum(0)
            stored[name, g] = x
            fig(f"{name}[{g}]", rel(x, want[g]), whole)
            fig(f"{name}[{g}] worst tile", tile_errors(x, want[g], plan.width), tile)
    if "a_act_out" in c.epi:
        for i, h in enumerate(gc.views(c, t, "a_act_out")):
            fig(f"a_act_out[{i}]", rel(cpu(h), ref["a_act_out"][i]), ACT_OUT)
    if "colsum" in c.epi:
        assert "cpre" in c.epi or not c.out_act, "the summed values are not among the outputs"
        for g in range(c.groups):
            v = stored["cpre" if "cpre" in c.epi else "C", g]
            got = cpu(gc.views(c, t, "colsum")[g]).view(-1, c.N)
            if "gate_stats" in c.epi:
                w, ghat = ref["gst_w"], ref["gst_ghat"]
                want, want2 = gc.tile_sums(v * w, c.M, c.N), gc.tile_sums(v * w * ghat, c.M, c.N)
                got2 = cpu(gc.views(c, t, "colsq")[g]).view(-1, c.N)
                fig("gate sums v w", rel(got.sum(0), want.sum(0)), GATE_SUMS)
                fig("gate sums v w ghat", rel(got2.sum(0), want2.sum(0)), GATE_SUMS)
                fig("gate partials v w", rel(got, want), GATE_SUMS)
                fig("gate partials v w ghat", rel(got2, want2), GATE_SUMS)
                continue
            fig(f"colsum[{g}]", rel(got, gc.tile_sums(v, c.M, c.N)), SUMS)
            if "colsq" in c.epi:
                got2 = cpu(gc.views(c, t, "colsq")[g]).view(-1, c.N)
                fig(f"colsq[{g}]", rel(got2, gc.tile_sums(v * v, c.M, c.N)), SUMS)
    # views with ld > N: the padding still holds its sentinel
    for name, field in (("C", "C"), ("P", "cpre"), ("H", "a_act_out")):
        if name in t and c.splitk == 1:
            mask = torch.ones(t[name].shape[1], dtype=torch.bool)
            for v_ in gc.views(c, t, field):
                off = v_.storage_offset() % t[name].stride(0)
                mask[off:off + v_.shape[1]] = False
            pad = t[name][:, mask.to(dev)]
            assert pad.numel() > 0 and bool((pad == gc.SENTINEL).all()), f"{name}: padding overwritten"
    # the rows behind the last: outputs still hold the sentinel (the NaN behind the inputs is in no figure above)
    gc.assert_tails(c, t)
    assert not bad, bad

"""Accuracy evidence beyond well-scaled N(0,1) operands, through the C ABI.

(a) The GEMM kernels at precision 0 (fp32 MFMA) and 1 (bf16x3: every fp32 product rebuilt from six bf16 MFMA products)
    on operands that stress a split-operand scheme: rows / columns whose scales span 2^-40 .. 2^+20, K-sums that cancel
    (O(1) terms, sum ~ 0) and operands whose LOW bf16 pieces sit next to the denormal range.  The error measure is the
    componentwise one every fp32 dot product obeys,

        err_ij = |C_ij - ref_ij| / (sum_k |a_ik| |b_kj|)        in units of u = 2^-24,

    (ref in fp64), which does not care about scaling or cancellation; a correct fp32 GEMM gives O(sqrt(K)) .. O(K) u.
    Asserted: both precisions stay under BOUND_U and bf16x3 is never worse than 2x the fp32 MFMA on the same operands.
(b) fast_sigmoid / fast_silu / fast_dsilu (v_exp_f32 + bare v_rcp_f32, csrc/gemm_kernel.h:39) and the gate kernels'
    cn_sigmoid at edge values -- +-88 (exp overflow threshold), +-1e4, +-inf, NaN -- against torch's own SiLU / sigmoid.
    cn_softplus (csrc/common.h) element by element through every site that runs it -- cartnet_eltwise op 0,
    cartnet_softplus_update_fwd and the GEMM out_act epilogue of the general, DMA-fed and persistent kernels -- on the edge
    values, ulp neighbourhoods and a dense sweep; softplus' (a * sigmoid(b), threshold 20) at the edge values.
The MSE-loss training step against the oracle's autograd (reference train/train.py:173-178) is in test_gpu_model.py.
"""
import math

import pytest
import torch

from gemm_cases import gemm_on

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BOUND_U = 48.0          # componentwise error bound asserted for K <= 512, in units of u (measured: 2 .. 12)


@pytest.fixture(scope="module")
def ops():
    from cartnet_amd import ops as _ops
    from cartnet_amd import lib
    lib.load()
    return _ops


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def comp_err_u(C, A64, B64, ref64):
    """max_ij |C - ref| / (|A| |B|)_ij in units of u; A64 [M,K], B64 [K,N] on the CPU in fp64."""
    bound = A64.abs() @ B64.abs()
    err = (C.detach().double().cpu() - ref64).abs()
    ok = bound > 0
    return (err[ok] / bound[ok]).max().item() / U


def pow2(exps):
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), exps.double()).float()


def operands(case, M, K, N, seed):
    """A [M,K], B [K,N] fp32 on the CPU for one stress case."""
    A, B = rnd(M, K, seed=seed), rnd(K, N, seed=seed + 1) * 0.1
    g = torch.Generator().manual_seed(seed + 2)
    if case == "row_col_scales":          # every row of A and every column of B at its own power of two, 2^-40 .. 2^+20
        A = A * pow2(torch.randint(-40, 21, (M, 1), generator=g))
        B = B * pow2(torch.randint(-40, 21, (1, N), generator=g))
    elif case == "k_scales":              # scales vary ALONG the reduction: terms of a dot product span 2^-30 .. 2^+10
        s = torch.randint(-30, 11, (1, K), generator=g)
        A = A * pow2(s)
        B = B * pow2(-s.t() + torch.randint(-3, 4, (K, 1), generator=g))
    elif case == "cancellation":          # second half of K repeats the first with the sign flipped (+ a 2^-20 residue)
        h = K // 2
        A = torch.cat([A[:, :h], -A[:, :h] + rnd(M, h, seed=seed + 3) * 2.0 ** -20], dim=1)
        B = torch.cat([B[:h], B[:h]], dim=0)
    elif case == "low_pieces_near_denormal":   # |a| ~ 2^-100: the third bf16 piece (2^-16 a) ~ 2^-116 .. 2^-122, normal but close
        A = A * 2.0 ** -100
        B = B * 2.0 ** 60                 # products ~ 2^-40: comfortably normal in the fp32 accumulator
    elif case == "mixed_magnitude_rows":  # a few huge entries per row next to tiny ones (outlier channels)
        mask = torch.rand(M, K, generator=g) < 0.02
        A = torch.where(mask, A * 2.0 ** 18, A * 2.0 ** -12)
    else:
        raise ValueError(case)
    return A.contiguous(), B.contiguous()


CASES = ["row_col_scales", "k_scales", "cancellation", "low_pieces_near_denormal", "mixed_magnitude_rows"]


def run_nn_image(ops, A, B, precision, family):
    """C = A @ B with the weights as a pre-arranged image: through the DMA-fed activation x weight kernels where the launch
    has the tiles for them (``family``: what the plan must name)."""
    Ad, Bd = A.to(dev()), B.to(dev())
    img = (ops.pack_b if precision == 0 else ops.split_b)([Bd])
    C = torch.full((A.shape[0], B.shape[1]), float("nan"), device=dev())
    gemm_on(ops, family, Ad, Bd, C, b_kstrided=True, precision=precision, b_split=img)
    return C


def run_nt_general(ops, A, B, precision, family):
    """C = A @ B through the general kernel (B handed over as [N, K] rows, no image)."""
    Ad, Bt = A.to(dev()), B.t().contiguous().to(dev())
    C = torch.full((A.shape[0], B.shape[1]), float("nan"), device=dev())
    gemm_on(ops, family, Ad, Bt, C, precision=precision)
    return C


def run_tn(ops, A, B, precision, family):
    """C = A @ B as a weight gradient: the reduction runs over the ROWS of two k-strided operands (A^T [K,M], B [K,N])."""
    At, Bd = A.t().contiguous().to(dev()), B.to(dev())
    C = torch.full((A.shape[0], B.shape[1]), float("nan"), device=dev())
    gemm_on(ops, family, At, Bd, C, a_kstrided=True, b_kstrided=True, precision=precision)
    return C


# (form, M, K) -> the kernel family at precision 0 and at precision 1.  The NT form has no bf16x3 kernel (general_x3 takes
# k-strided B only) and a weight gradient over a K that is no multiple of 16 runs un-split on the general kernel: those two
# shapes compare fp32 with fp32; the bf16x3 weight gradient with a K tail is a split-K case of tests/test_gpu_gemm_families.py
STRESS_FAMILY = {("nn_image", 33000, 256): ("f32nn128", "x3nn16"), ("nn_image", 13000, 512): ("f32nn128", "x3nn16"),
                 ("nt_general", 13000, 208): ("general128", "general256"), ("tn", 256, 6000): ("f32tn", "x3tn"),
                 ("tn", 256, 20001): ("general256", "general256"), ("nn_image", 1000, 512): ("general64", "general64"),
                 ("tn", 128, 777): ("general64", "general64")}


@pytest.mark.parametrize("case", CASES)
# Shapes: at precision 1 a launch with fewer than 96 tiles of 128 x 256 runs on the narrow-tile fp32 kernels by design
# (csrc/gemm.hip choose_bn), so the bf16x3 kernels only see M >= 12,288 rows (activation x weight products) or the
# 256-wide weight-gradient form; the small shapes at the end pin that fallback (both precisions then agree bit for bit).
@pytest.mark.parametrize("form,M,K,N", [("nn_image", 33000, 256, 256), ("nn_image", 13000, 512, 256),
                                        ("nt_general", 13000, 208, 256), ("tn", 256, 6000, 256), ("tn", 256, 20001, 256),
                                        ("nn_image", 1000, 512, 256), ("tn", 128, 777, 64)])
def test_gemm_stress_operands_both_precisions(ops, case, form, M, K, N):
    run = {"nn_image": run_nn_image, "nt_general": run_nt_general, "tn": run_tn}[form]
    A, B = operands(case, M, K, N, seed=100)
    A64, B64 = A.double(), B.double()
    ref = A64 @ B64
    family = STRESS_FAMILY[form, M, K]
    if (form, K, case) == ("tn", 20001, "cancellation"):      # this case pairs its columns: K = 20,000, whole K-steps
        family = ("f32tn", "x3tn")
    e = {p: comp_err_u(run(ops, A, B, p, family[p]), A64, B64, ref) for p in (0, 1)}
    # the error of a K-term fp32 dot product grows at most like K u (typically sqrt(K) u); both precisions are far below
    bound = BOUND_U * max(1.0, math.sqrt(K / 512.0))
    print(f"ACCURACY {case:26s} {form:10s} M={M:6d} K={K:5d} N={N:4d}  fp32 MFMA {e[0]:7.2f} u   bf16x3 {e[1]:7.2f} u")
    assert e[0] < bound, (case, form, e)
    assert e[1] < bound, (case, form, e)
    assert e[1] <= 2.0 * e[0] + 1.0, (case, form, e)      # bf16x3 never worse than 2x the fp32 MFMA (+1 u of slack)


def test_gemm_denormal_low_pieces_are_a_documented_limit(ops):
    """|a| ~ 2^-112: the third bf16 piece of an operand falls into the denormal range.  fp32 MFMA keeps its accuracy;
    bf16x3 may lose the piece (2^-16 relative to the product instead of 2^-24) -- asserted only against that bound, and
    DESIGN.md names it: activations of this model are O(1), 30 binary orders away."""
    M, K, N = 33000, 256, 256            # enough row tiles for the bf16x3 kernel to take the launch
    A, B = rnd(M, K, seed=5) * 2.0 ** -112, rnd(K, N, seed=6) * 2.0 ** 70
    A64, B64 = A.double(), B.double()
    ref = A64 @ B64
    e0 = comp_err_u(run_nn_image(ops, A, B, 0, "f32nn128"), A64, B64, ref)
    e1 = comp_err_u(run_nn_image(ops, A, B, 1, "x3nn16"), A64, B64, ref)
    print(f"ACCURACY denormal low pieces: fp32 MFMA {e0:.2f} u, bf16x3 {e1:.2f} u")
    assert e0 < BOUND_U
    assert e1 < 2.0 ** 10, (e0, e1)      # <= 2^-14 relative to sum |a||b|: two pieces always survive


# ------------------------------------------------------------------------------------------------ activations
EDGE = [0.0, -0.0, 1.0, -1.0, 20.0, -20.0, 87.0, -87.0, 88.0, -88.0, 88.7, -88.7, 89.0, -89.0, 103.0, -103.0, 1e4, -1e4,
        3e38, -3e38, float("inf"), float("-inf"), float("nan"), 1e-30, -1e-30, 1e-40, -1e-40]


def same_special(got, want, atol, rtol=2e-6):
    got, want = got.double().cpu(), want.double().cpu()
    nan_ok = torch.isnan(got) == torch.isnan(want)
    inf_ok = torch.where(torch.isinf(want), got == want, torch.ones_like(nan_ok))
    fin = torch.isfinite(want)
    close = torch.where(fin, (got - want).abs() <= atol + rtol * want.abs(), torch.ones_like(nan_ok))
    return bool(nan_ok.all() and inf_ok.all() and close.all()), (got, want)


@pytest.mark.parametrize("precision", [0, 1])
def test_silu_epilogue_edge_values(ops, precision):
    """out_act: C = silu(A B^T + bias) with A B^T = 0 exactly and the edge values in the bias, one per column; cpre
    receives the pre-activation.  NaN / +-inf propagate like torch.nn.functional.silu (silu(-inf) = NaN in both)."""
    v = torch.tensor(EDGE + [0.0] * (64 - len(EDGE)))
    M, K, N = 130, 32, 64
    A, B = torch.zeros(M, K, device=dev()), rnd(N, K, seed=1).to(dev())
    C, Cpre = torch.empty(M, N, device=dev()), torch.empty(M, N, device=dev())
    ops.gemm(A, B, C, out_act=True, bias=v.to(dev()), cpre=Cpre, precision=precision)
    want = torch.nn.functional.silu(v.double()).float().expand(M, N)
    ok, pair = same_special(C, want, atol=1e-30)
    assert ok, pair
    assert torch.equal(torch.nan_to_num(Cpre.cpu(), nan=7.0), torch.nan_to_num(v.expand(M, N), nan=7.0))


@pytest.mark.parametrize("precision", [0, 1])
def test_dsilu_epilogue_edge_values(ops, precision):
    """dact: C = (A B^T) * silu'(pre) with A B^T = 1 exactly and the edge values in `pre`."""
    v = torch.tensor(EDGE + [0.5] * (64 - len(EDGE)))
    M, K, N = 70, 16, 64
    A = torch.zeros(M, K, device=dev())
    A[:, 0] = 1.0
    B = torch.zeros(N, K, device=dev())
    B[:, 0] = 1.0
    pre = v.expand(M, N).contiguous().to(dev())
    C = torch.empty(M, N, device=dev())
    ops.gemm(A, B, C, dact=pre, precision=precision)
    x = v.double()
    s = torch.sigmoid(x)
    want = (s * (1 + x * (1 - s))).float().expand(M, N)        # torch's silu backward formula
    ok, pair = same_special(C, want, atol=1e-30)
    assert ok, pair


@pytest.mark.parametrize("precision", [0, 1])
def test_silu_prologue_finite_edge_values(ops, precision):
    """a_act: C = silu(A) @ I.  Finite edge values only: an infinite or NaN activation times the identity's zeros is
    NaN in every column of its row -- in torch too -- so +-inf / NaN are covered by the epilogue tests above."""
    fin = [x for x in EDGE if math.isfinite(x) and abs(x) < 1e30]
    K = 64
    v = torch.tensor(fin + [0.25] * (K - len(fin)))
    M = 200
    A = v.expand(M, K).contiguous().to(dev())
    eye = torch.eye(K, device=dev())
    C = torch.empty(M, K, device=dev())
    ops.gemm(A, eye, C, a_act=True, precision=precision)
    want = torch.nn.functional.silu(v.double()).float().expand(M, K)
    ok, pair = same_special(C, want, atol=1e-30, rtol=(2e-6 if precision == 0 else 4e-6))
    assert ok, pair


def test_gate_sigmoid_edge_values(ops):
    """cn_sigmoid in the forward gate: sigma = env * sigmoid(bn(g)) with mean 0, rstd 1, gamma 1, beta 0, so that the gate
    sees the edge values themselves; sender = 1 makes the aggregated row the sum of the sigmas."""
    D = 64
    v = torch.tensor(EDGE + [0.0] * (D - len(EDGE)))
    N, deg = 5, 3
    E = N * deg
    tgt = torch.arange(N).repeat_interleave(deg)
    ei = torch.stack([(tgt + 1) % N, tgt]).to(dev())                     # sorted by target, `deg` edges each
    lay = ops.GraphLayout(ei, N, torch.tensor([0, N], dtype=torch.int64, device=dev()))
    gs = torch.cat([v.expand(E, D), torch.ones(E, D)], dim=1).contiguous().to(dev())
    e_in = torch.zeros(E, D, device=dev())
    mr = torch.cat([torch.zeros(D), torch.ones(D)]).to(dev())
    ga, be = torch.ones(D, device=dev()), torch.zeros(D, device=dev())
    e_out, aggr = torch.empty(E, D, device=dev()), torch.empty(N, D, device=dev())
    nparts = ops.gate_nparts(N)
    ps, pq = (torch.zeros(nparts * D, dtype=torch.float64, device=dev()) for _ in range(2))
    ops.gate_scatter_fwd(gs, e_in, None, lay, mr, ga, be, e_out, aggr, ps, pq)
    want = torch.sigmoid(v.double()).float()
    ok, pair = same_special(e_out, want.expand(E, D), atol=1e-30)
    assert ok, pair
    ok, pair = same_special(aggr, (want.double() * deg).float().expand(N, D), atol=1e-30, rtol=4e-6)
    assert ok, pair


# ------------------------------------------------------------------------------------------------ softplus
SP_COLS = 256
SP_ROWS = 12416          # 97 row tiles of 128: enough for the bf16x3 kernels to take a precision-1 launch (96)
SERIES_T = -math.log(2.0 ** 11)      # where an earlier form switched from log(1 + t) to the series t - t^2/2


def ulp_neighbours(c, n=64):
    """Every fp32 value within +-n ulp of c (c != 0)."""
    bits = torch.tensor([c], dtype=torch.float32).view(torch.int32)
    return (bits + torch.arange(-n, n + 1, dtype=torch.int32)).view(torch.float32)


def softplus_sweep():
    """[SP_ROWS, SP_COLS] fp32: the finite EDGE values, every fp32 value within 64 ulp of +-20 (the threshold) and of the
    old series threshold, the underflow tail [-104, -30] and a dense sweep of [-30, 30] (over 2^20 values) filling the rest."""
    fin = torch.tensor([x for x in EDGE if math.isfinite(x)])
    near = torch.cat([ulp_neighbours(c) for c in (20.0, -20.0, SERIES_T)])
    tail = torch.linspace(-104.0, -30.0, 1 << 16, dtype=torch.float64).float()
    head = torch.cat([fin, near, tail])
    dense = torch.linspace(-30.0, 30.0, SP_ROWS * SP_COLS - head.numel(), dtype=torch.float64).float()
    assert dense.numel() >= 1 << 20
    return torch.cat([head, dense]).view(SP_ROWS, SP_COLS)


def softplus_rtol(x):
    """Per-element relative bound of the fast softplus, rtol(x) = 2e-6 + 1e-7 |x|.

    t = exp(-|x|) is v_exp_f32(fl(-|x| log2 e)): the rounded argument is off by up to |x| log2(e) 2^-24 in the exponent,
    i.e. exp by a relative |x| 2^-24 = 6e-8 |x|, on top of the instruction's own ~1 ulp.  log1p(t) passes a relative
    error of t on with a factor t / ((1 + t) log1p(t)) <= 1, and for x > 0 the sum x + log1p(t) only shrinks it.  What
    remains is a few roundings of the log1p evaluation and of the final sum (each 2^-24 = 6e-8), which 2e-6 covers with
    room; 1e-7 |x| covers the argument with a factor 1.7.  Past x = 20 the result is x itself (torch's threshold); below
    x = -69 the result is under 1e-30 and only the absolute term of the comparison applies."""
    return 2e-6 + 1e-7 * x.double().abs().nan_to_num(nan=0.0, posinf=0.0)      # (+-inf, NaN: compared exactly)


def softplus_check(site, got, x):
    """got = softplus(x) per element within softplus_rtol, NaN / +-inf as torch.nn.functional.softplus (fp64)."""
    want = torch.nn.functional.softplus(x.double().cpu())
    g = got.double().cpu()
    fin = torch.isfinite(want) & (want.abs() > 1e-30)       # (below 1e-30 only the absolute term applies)
    rel = ((g - want).abs() / want.abs())[fin]
    i = int(rel.argmax())
    print(f"SOFTPLUS {site:28s} max rel err {float(rel[i]):.3e} at x = {float(x.cpu().double()[fin][i]):.7g}")
    ok, pair = same_special(got, want, atol=1e-30, rtol=softplus_rtol(x.cpu()))
    assert ok, (site, pair)


def softplus_nonfinite():
    """Every EDGE value in one row (the columns past them 0): a bias vector for the GEMM epilogue, whose pre-activation is
    then A B + bias = the value itself with A = 0 -- +-inf and NaN cannot pass through an identity product."""
    return torch.tensor(EDGE + [0.0] * (SP_COLS - len(EDGE)))


GEMM_SP_FORMS = [("general", 0), ("general", 1), ("dma", 0), ("dma", 1), ("persistent", 0)]


def gemm_softplus(ops, A, bias, form, precision):
    """out = softplus(A I + bias) with the pre-activation kept (cpre), through the kernel family `form` takes:
    general -- no weight image (the general tile kernel, 64-wide at these 97 tiles; at precision 1 its 256-wide bf16x3
    form); dma -- weight image with
    tile_policy 256 (the DMA-fed 256-wide kernels: f32nn / x3nn16); persistent -- weight image with tile_policy 3, K = 256
    (gemm_f32p.h, precision 0 only: the bf16x3 path has no persistent kernel)."""
    eye = torch.eye(SP_COLS, device=dev())
    out = torch.full(tuple(A.shape), float("nan"), device=dev())
    pre = torch.full(tuple(A.shape), float("nan"), device=dev())
    kw = dict(b_kstrided=True, bias=bias.to(dev()), cpre=pre, out_act=True, dact_kind=1, precision=precision)
    if form != "general":
        kw["b_split"] = (ops.pack_b if precision == 0 else ops.split_b)([eye])[0]
        kw["tile_policy"] = 256 if form == "dma" else 3
    family = {("general", 0): "general64", ("general", 1): "general_x3", ("dma", 0): "f32nn", ("dma", 1): "x3nn16",
              ("persistent", 0): "f32p"}[form, precision]
    assert A.shape[0] == SP_ROWS
    gemm_on(ops, family, A.to(dev()), eye, out, **kw)
    return out, pre


def test_softplus_eltwise_and_update_sweep(ops):
    """cartnet_eltwise op 0 and cartnet_softplus_update_fwd (o = 0, mean 0, rstd 1, gamma 1, beta 0: u = x exactly) on the
    sweep and on the non-finite EDGE values: element-wise against fp64, and the two sites bit for bit."""
    X = softplus_sweep()
    for V in (X, softplus_nonfinite().expand(8, SP_COLS).contiguous()):
        Vd = V.to(dev())
        y0 = torch.full_like(Vd, float("nan"))
        ops.eltwise(0, Vd, None, y0)
        softplus_check("eltwise op 0", y0, V)
        D = SP_COLS
        mr = torch.cat([torch.zeros(D), torch.ones(D)]).to(dev())
        y1 = torch.full_like(Vd, float("nan"))
        ops.softplus_update_fwd(torch.zeros_like(Vd), Vd, mr, torch.ones(D, device=dev()), torch.zeros(D, device=dev()), y1)
        softplus_check("softplus_update_fwd", y1, V)
        assert torch.equal(y0.isnan(), y1.isnan()) and torch.equal(y0.nan_to_num(7.0), y1.nan_to_num(7.0))


@pytest.mark.parametrize("form,precision", GEMM_SP_FORMS)
def test_softplus_gemm_epilogue_sweep(ops, form, precision):
    """CartnetGemmArgs.out_act with dact_kind = 1 on the sweep: C = softplus(A I + 0) with cpre = A I + 0 (an identity
    operand: at precision 0 the pre-activation is the sweep value itself), and on the non-finite EDGE values through the
    bias.  Element-wise against fp64 of the kept pre-activation, and bit for bit what cartnet_eltwise op 0 makes of it."""
    X = softplus_sweep()
    out, pre = gemm_softplus(ops, X, torch.zeros(SP_COLS), form, precision)
    dev_rel = ((pre.cpu().double() - X.double()).abs() / X.double().abs().clamp(min=1e-30)).max()
    print(f"SOFTPLUS gemm {form} p{precision}: pre-activation vs the sweep value, max rel {float(dev_rel):.3e}")
    if precision == 0:
        assert torch.equal(pre.cpu(), X), form
    else:        # bf16x3: the module's bound for a split product that keeps two of its three pieces (2^-14 relative)
        assert float(dev_rel) <= 2.0 ** -14, form
    softplus_check(f"gemm {form} p{precision}", out, pre)
    chk = torch.empty_like(out)
    ops.eltwise(0, pre, None, chk)
    assert torch.equal(out, chk), f"{form} p{precision}: epilogue differs from cartnet_eltwise op 0"
    v = softplus_nonfinite()
    out, pre = gemm_softplus(ops, torch.zeros(SP_ROWS, SP_COLS), v, form, precision)
    assert torch.equal(pre.cpu().nan_to_num(7.0), v.expand(SP_ROWS, SP_COLS).nan_to_num(7.0))
    softplus_check(f"gemm {form} p{precision} edge", out, pre)
    ops.eltwise(0, pre, None, chk)
    assert torch.equal(out.isnan(), chk.isnan()) and torch.equal(out.nan_to_num(7.0), chk.nan_to_num(7.0))


# softplus' = a * sigmoid(b) with torch's threshold 20 (b > 20: a): EDGE and the +-20 neighbourhoods in b, a = 1 and a = -3
def dsoftplus_operands():
    b = torch.cat([torch.tensor(EDGE), ulp_neighbours(20.0, 50), ulp_neighbours(-20.0, 50)])
    b = torch.cat([b, torch.full((SP_COLS - b.numel(),), 0.5)])
    B = b.expand(64, SP_COLS).contiguous()
    A = torch.ones(64, SP_COLS)
    A[32:] = -3.0
    return A, B


def dsoftplus_check(site, got, A, B):
    b = B.double()
    want = A.double() * torch.where(b > 20, torch.ones_like(b), torch.sigmoid(b))
    # sigmoid(b) = rcp(1 + exp(-b)): the same argument rounding of the hardware exp as in softplus_rtol, relative
    # |b| 2^-24 of exp(-b) and at most that of the sigmoid; the rest is a few ulp
    ok, pair = same_special(got, want, atol=1e-30, rtol=softplus_rtol(B))
    assert ok, (site, pair)


def test_dsoftplus_eltwise_and_bwd_sums_edge_values(ops):
    """cartnet_eltwise op 1 and cartnet_softplus_bwd_sums (out = a * sigmoid(b), threshold 20) at the edge values."""
    A, B = dsoftplus_operands()
    Ad, Bd = A.to(dev()), B.to(dev())
    y0, y1 = torch.full_like(Ad, float("nan")), torch.full_like(Ad, float("nan"))
    ops.eltwise(1, Ad, Bd, y0)
    dsoftplus_check("eltwise op 1", y0, A, B)
    s = torch.empty(SP_COLS, device=dev())
    ops.softplus_bwd_sums(Ad, Bd, y1, s)
    dsoftplus_check("softplus_bwd_sums", y1, A, B)
    assert torch.equal(y0.nan_to_num(7.0), y1.nan_to_num(7.0))


@pytest.mark.parametrize("form,precision", [("general", 0), ("general", 1), ("dma", 0), ("dma", 1)])
def test_dsoftplus_gemm_epilogue_edge_values(ops, form, precision):
    """dact with dact_kind = 1: C = (A I) * sigmoid(pre), A I = a exactly, the edge values in `pre`.  general: the 64-wide
    general kernel (precision 0, two tiles) and its bf16x3 form; dma: f32nn and x3nn16 (tile_policy 256) -- which need 64 and
    96 tiles: with 256 rows the precision-0 "dma" case ran on the general kernel too."""
    A, B = dsoftplus_operands()
    M = SP_ROWS if precision == 1 or form == "dma" else 256          # enough row tiles for the DMA-fed / bf16x3 kernels
    A, B = A.repeat(M // 64, 1), B.repeat(M // 64, 1)
    eye = torch.eye(SP_COLS, device=dev())
    C = torch.full((M, SP_COLS), float("nan"), device=dev())
    kw = dict(b_kstrided=True, dact=B.to(dev()), dact_kind=1, precision=precision)
    if form == "dma":
        kw["b_split"] = (ops.pack_b if precision == 0 else ops.split_b)([eye])[0]
        kw["tile_policy"] = 256
    family = {("general", 0): "general64", ("general", 1): "general_x3", ("dma", 0): "f32nn", ("dma", 1): "x3nn16"}[form, precision]
    gemm_on(ops, family, A.to(dev()), eye, C, **kw)
    dsoftplus_check(f"gemm dact {form} p{precision}", C, A, B)


@pytest.mark.parametrize("training", [True, False])
def test_dsoftplus_update_bwd_apply_edge_values(ops, training):
    """cartnet_softplus_update_bwd_apply with o = 0, mean 0, rstd 1, gamma 1, beta 0 (u = x, ohat = 0) and the edge values
    in x: dx = dy * softplus'(u) (+ dx_add), d_o = gamma rstd (du - sums_a / N) -- here sums = 0, so d_o = du."""
    A, B = dsoftplus_operands()
    N, D = A.shape
    Ad, Bd = A.to(dev()), B.to(dev())
    mr = torch.cat([torch.zeros(D), torch.ones(D)]).to(dev())
    one, zero = torch.ones(D, device=dev()), torch.zeros(D, device=dev())
    d_o, dx = torch.full_like(Ad, float("nan")), torch.full_like(Ad, float("nan"))
    ops.softplus_update_bwd_apply(torch.zeros_like(Ad), Bd, Ad, mr, one, zero, torch.zeros(2 * D, device=dev()), training,
                                  d_o, None, dx)
    dsoftplus_check("softplus_update_bwd_apply dx", dx, A, B)
    dsoftplus_check("softplus_update_bwd_apply d_o", d_o, A, B)

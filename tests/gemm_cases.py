"""The CartnetGemmArgs contract in fp64, and the table of GEMM cases with the kernel family each must reach.

Two things live here (a helper module, not a conftest):

* ``gemm_ref64``: what include/cartnet_hip.h says cartnet_gemm computes, in fp64 torch on the CPU -- written from the
  header, not from a kernel.
* ``CASES``: launches as data (shapes, leading dimensions, views inside wider buffers, flags, precision, tile_policy)
  with the ``family`` the host-side plan (cartnet_gemm_plan) must give.  ``fake_args`` turns a case into a
  ``lib.GemmArgs`` of pointers that are never dereferenced (tests/test_gemm_plan_host.py, no GPU); ``make_tensors`` /
  ``gemm_kwargs`` allocate the operands for a real launch (tests/test_gpu_gemm_families.py); every buffer a launch
  indexes by its rows is allocated ``TAIL`` rows longer than the launch is told, with NaN behind the inputs and the
  sentinel behind the outputs (``tail_kind``), so that a read or a write past the last row shows.

Row counts are computed from tile counts: ``rows(t)`` is the smallest M with t row tiles of 128, so a case "at the
threshold" has a last tile of one row and the case one row tile below it (``rows(t) - 1`` rows) a full last tile.
"""
import ctypes
from types import SimpleNamespace

import torch

BM = 128                      # rows of an output tile (every kernel family)
SENTINEL = -7.0               # fills every padding column a launch must not touch
KS = (16, 32, 48, 64, 80, 96, 112, 128, 144, 256, 528)      # K-loop lengths: pipeline head alone ... steady state

EPILOGUES = ("bias", "gather", "resid", "dact", "colsum", "colsq", "cpre", "out_act", "a_act_out", "gate_stats")


def rows(tiles, extra=0):
    """The smallest M with ``tiles`` row tiles (a last tile of one row), plus ``extra`` rows (126: a last tile of 127
    rows, 127: a full one)."""
    return (tiles - 1) * BM + 1 + extra


def case(name, family, M, N, K, **kw):
    c = dict(name=name, family=family, M=M, N=N, K=K, groups=1, segs=1, precision=0, tile_policy=0, layout="nn",
             a_act=False, b_act=False, out_act=False, image=True, folded=False, splitk=1, epi=(), dact_kind=0,
             off_a=0, pad_a=16, pad_b=4, pad_c=8, pad_r=4, pad_d=12, pad_g=4, gather_rows=37, env=True)
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    assert all(e in EPILOGUES for e in c["epi"]), c["epi"]
    assert c["groups"] == 1 or c["segs"] == 1
    if c["layout"] != "nn":
        c["image"] = False
    return SimpleNamespace(**c)


# ------------------------------------------------------------------------------------------------ buffers and views
def _buffers(c):
    """Every buffer of a case and the views a launch is given: {name: (rows, cols, dtype)} and {field: [(buffer,
    first column, columns)]}.  Operands of the groups / K-segments are column blocks of one matrix, as in the model
    (pre = [gate | aggr]); outputs are column blocks of one matrix with ``pad_c`` columns of padding, every other
    epilogue operand has its own padded matrix."""
    n = c.groups * c.segs
    G = c.groups
    f32, f64, i32, u8 = torch.float32, torch.float64, torch.int32, torch.uint8
    buf, view = {}, {}
    if c.layout == "tn":                                   # A [K, M] (dY), B [K, N] (X): both reduce over rows
        buf["A"] = (c.K, c.off_a + n * c.M + c.pad_a, f32)
        view["A"] = [("A", c.off_a + i * c.M, c.M) for i in range(n)]
        buf["B"] = (c.K, n * c.N + c.pad_b, f32)
        view["B"] = [("B", i * c.N, c.N) for i in range(n)]
    else:
        buf["A"] = (c.M, c.off_a + n * c.K + c.pad_a, f32)
        view["A"] = [("A", c.off_a + i * c.K, c.K) for i in range(n)]
        for i in range(n):                                 # weights: [K, N] ("nn": dX = dY W) or [N, K] ("nt": Y = X W^T)
            buf[f"B{i}"] = (c.K, c.N, f32) if c.layout == "nn" else (c.N, c.K, f32)
        view["B"] = [(f"B{i}", 0, c.N if c.layout == "nn" else c.K) for i in range(n)]
    if c.splitk > 1:
        for g in range(G):
            buf[f"C{g}"] = (c.splitk * c.M, c.N, f32)
        view["C"] = [(f"C{g}", 0, c.N) for g in range(G)]
    else:
        buf["C"] = (c.M, G * c.N + c.pad_c, f32)
        view["C"] = [("C", g * c.N, c.N) for g in range(G)]
    tiles = (c.M + BM - 1) // BM
    for e in c.epi:
        if e == "bias":
            for g in range(G):
                buf[f"bias{g}"] = (1, c.N, f32)
            view["bias"] = [(f"bias{g}", 0, c.N) for g in range(G)]
        elif e == "gather":
            for g in range(G):
                buf[f"Gi{g}"] = buf[f"Gj{g}"] = (c.gather_rows, c.N + c.pad_g, f32)
            view["gather_i"] = [(f"Gi{g}", 0, c.N) for g in range(G)]
            view["gather_j"] = [(f"Gj{g}", 0, c.N) for g in range(G)]
            buf["tgt"] = buf["src"] = (1, c.M, i32)
        elif e in ("resid", "dact"):
            k, pad = ("R", c.pad_r) if e == "resid" else ("D", c.pad_d)
            for g in range(G):
                buf[f"{k}{g}"] = (c.M, c.N + pad, f32)
            view[e] = [(f"{k}{g}", 0, c.N) for g in range(G)]
        elif e in ("colsum", "colsq"):
            for g in range(G):
                buf[f"{e}{g}"] = (1, tiles * c.N, f64)
            view[e] = [(f"{e}{g}", 0, tiles * c.N) for g in range(G)]
        elif e == "cpre":
            buf["P"] = buf["C"]
            view["cpre"] = [("P", g * c.N, c.N) for g in range(G)]
        elif e == "a_act_out":
            buf["H"] = buf["A"]
            view["a_act_out"] = [("H", o, w) for _, o, w in view["A"]]
        elif e == "gate_stats":
            buf["gst_g"] = (c.M, 2 * c.N, f32)             # the gate half of a [gate | sender] matrix
            buf["gst_mean_rstd"] = (1, 2 * c.N, f32)
            buf["gst_gamma"] = buf["gst_beta"] = (1, c.N, f32)
            if c.env:
                buf["gst_env"] = (1, c.M, f32)
    if c.image:
        bytes_per = 4 if c.precision == 0 else 6
        for i in range(n):
            buf[f"img{i}"] = (1, bytes_per * c.K * c.N, u8)
        if c.folded:
            buf["imgf"] = (1, bytes_per * c.K * c.N * n, u8)
    return buf, view


def fake_args(c, lib):
    """The case as a lib.GemmArgs whose pointers are 256-byte aligned bases plus the view offsets: for the host-side
    plan query only, never dereferenced."""
    buf, view = _buffers(c)
    base, addr = {}, 1 << 20
    for name, (r, w, dt) in buf.items():
        base[name] = addr
        addr += (r * w * torch.empty(0, dtype=dt).element_size() + 255) // 256 * 256 + 256

    def ptrs(field):
        return [base[b] + 4 * off for b, off, _ in view[field]]
    a = lib.GemmArgs()
    a.M, a.N, a.K = c.M, c.N, c.K
    a.lda, a.ldc = buf["A"][1], (c.N if c.splitk > 1 else buf["C"][1])
    a.ldb = buf["B"][1] if c.layout == "tn" else buf["B0"][1]
    a.ngroups, a.nsegs, a.splitk = c.groups, c.segs, c.splitk
    a.a_kstrided, a.b_kstrided = int(c.layout == "tn"), int(c.layout != "nt")
    a.a_act, a.b_act, a.out_act = int(c.a_act), int(c.b_act), int(c.out_act)
    a.precision, a.tile_policy, a.dact_kind = c.precision, c.tile_policy, c.dact_kind
    for field in ("A", "B", "C", "bias", "gather_i", "gather_j", "resid", "dact", "colsum", "colsq", "cpre", "a_act_out"):
        if field in view:
            for i, p in enumerate(ptrs(field)):
                getattr(a, field)[i] = p
    if "gather" in c.epi:
        a.tgt, a.src, a.ldg, a.gather_rows = base["tgt"], base["src"], buf["Gi0"][1], c.gather_rows
    if "resid" in c.epi:
        a.ldr = buf["R0"][1]
    if "dact" in c.epi:
        a.ldd = buf["D0"][1]
    if c.image:
        for i in range(c.groups * c.segs):
            a.b_split[i] = base[f"img{i}"]
        if c.folded:
            a.b_split_folded = base["imgf"]
    if "gate_stats" in c.epi:
        a.gst_g, a.gst_ld = base["gst_g"], buf["gst_g"][1]
        a.gst_mean_rstd, a.gst_gamma, a.gst_beta = base["gst_mean_rstd"], base["gst_gamma"], base["gst_beta"]
        a.gst_env = base["gst_env"] if c.env else None
    return a


def plan_of(c, lib):
    """(return code, lib.GemmPlanInfo) of the case's fake launch."""
    info = lib.GemmPlanInfo()
    rc = lib.load().cartnet_gemm_plan(ctypes.byref(fake_args(c, lib)), ctypes.byref(info))
    return rc, info


def family_name(info, lib):
    if info.family < 0:
        return "none"
    name = lib.GEMM_FAMILIES[info.family]
    return name + str(info.width) if name == "general" else name


def gemm_on(ops, family, A, B, C, **kw):
    """ops.gemm, after asserting that the plan of the same arguments names ``family``: the existing GEMM tests say
    which kernel each of their launches is about."""
    plan = ops.gemm_plan(A, B, C, **kw)
    assert plan.family == family, (family, plan)
    ops.gemm(A, B, C, **kw)
    return plan


def width_of(family):
    """Column-tile width of a family name: 64 / 128 / 256 for the general kernel, 128 for f32nn128, else 256."""
    if family.startswith("general") and family[7:].isdigit():
        return int(family[7:])
    return 128 if family == "f32nn128" else 256


TAIL = 160                    # rows allocated behind the last row of every row-indexed buffer: more than one row tile


def tail_kind(c, name):
    """How a buffer of a case is indexed by the launch's rows (M, or K in the "tn" layout), and what lies behind its last
    row: (axis, fill) or None.  Inputs get NaN -- a ragged last tile that reads past its rows, or a split-K slab past K,
    shows in the product or in a column sum; tgt / src get 0, a valid row of the gathered matrices; outputs get SENTINEL,
    which must still be there after the launch."""
    if name in ("C", "P", "H") or (name[0] == "C" and name[1:].isdigit()):
        return 0, SENTINEL
    if name == "A" or (name == "B" and c.layout == "tn") or name == "gst_g" or (name[0] in "RD" and name[1:].isdigit()):
        return 0, float("nan")
    if name == "gst_env":
        return 1, float("nan")
    if name in ("tgt", "src"):
        return 1, 0
    return None


class Tensors(dict):
    """{buffer name: tensor of the case's shape}; ``full[name]`` is the allocation behind a row-indexed buffer, TAIL rows
    longer, of which the entry is the view of the first rows (same leading dimension)."""

    def __init__(self):
        super().__init__()
        self.full = {}


def assert_tails(c, t):
    """After a launch: every row behind the last still holds what make_tensors put there."""
    assert t.full, "no buffer of the case has a tail"
    for name, full in t.full.items():
        axis, fill = tail_kind(c, name)
        tail = full[t[name].shape[0]:] if axis == 0 else full[:, t[name].shape[1]:]
        assert tail.numel() == TAIL * full.shape[1 - axis], name
        ok = torch.isnan(tail) if fill != fill else tail == fill
        assert bool(ok.all()), f"{name}: {int((~ok).sum())} cells behind the last row were overwritten"


def make_tensors(c, device):
    """Real operands of a case on ``device``: different weights and biases per group (a kernel that reads the wrong
    group's shows), NaN in every cell a launch must write, SENTINEL in every padding column it must not, sorted tgt and
    random src.  Every buffer the launch indexes by its rows is allocated TAIL rows longer (``tail_kind``) and handed out
    as the view of its first rows.  Returns a ``Tensors`` {buffer name: tensor} (2-D; 1-row buffers are the vectors) --
    leave it unchanged after the launch except through the launch."""
    buf, view = _buffers(c)
    gen = torch.Generator().manual_seed(1000 + sum(map(ord, c.name)))
    t = Tensors()
    for name, (r, w, dt) in buf.items():
        if name in ("C", "P", "H") or name.startswith(("C", "colsum", "colsq")):
            x = torch.full((r, w), SENTINEL if name in ("C", "P", "H") else float("nan"), dtype=dt)
        elif name == "tgt":
            x = torch.sort(torch.randint(0, c.gather_rows, (r, w), generator=gen)).values.to(dt)
        elif name == "src":
            x = torch.randint(0, c.gather_rows, (r, w), generator=gen).to(dt)
        elif dt == torch.uint8:
            x = torch.zeros(r, w, dtype=dt)
        elif name == "gst_env":
            x = torch.rand(r, w, generator=gen)
        elif name == "gst_mean_rstd":
            x = torch.cat([torch.randn(1, c.N, generator=gen) * 0.1, 0.5 + torch.rand(1, c.N, generator=gen)], dim=1)
        else:
            scale = 0.1 if name.startswith("B") and c.layout != "tn" else 1.0
            x = torch.randn(r, w, generator=gen) * scale
        kind = tail_kind(c, name)
        if kind is None:
            t[name] = x.to(device)
            continue
        axis, fill = kind
        tail = torch.full((TAIL, w) if axis == 0 else (r, TAIL), fill, dtype=dt)
        t.full[name] = torch.cat([x, tail], dim=axis).to(device)
        t[name] = t.full[name][:r] if axis == 0 else t.full[name][:, :w]
    for field in ("C", "cpre", "a_act_out"):               # the cells the launch must write
        if field in view:
            for b, off, w in view[field]:
                t[b][:, off:off + w] = float("nan")
    return t


def views(c, t, field):
    _, view = _buffers(c)
    return [t[b][:, off:off + w] for b, off, w in view[field]] if field in view else None


def gemm_kwargs(c, t, ops):
    """(A, B, C, keywords) for ops.gemm / ops.gemm_plan from the tensors of make_tensors; builds the weight images."""
    v = lambda f: views(c, t, f)
    vec = lambda f: [x[0] for x in v(f)] if v(f) is not None else None
    kw = dict(a_kstrided=c.layout == "tn", b_kstrided=c.layout != "nt", a_act=c.a_act, b_act=c.b_act, out_act=c.out_act,
              segments=c.segs > 1, splitk=c.splitk, precision=c.precision, tile_policy=c.tile_policy,
              dact_kind=c.dact_kind, bias=vec("bias"), gather_i=v("gather_i"), gather_j=v("gather_j"), resid=v("resid"),
              dact=v("dact"), cpre=v("cpre"), colsum=vec("colsum"), colsq=vec("colsq"), a_act_out=v("a_act_out"))
    if "gather" in c.epi:
        kw["tgt"], kw["src"] = t["tgt"][0], t["src"][0]
    if c.image:
        make = ops.pack_b if c.precision == 0 else ops.split_b
        n = c.groups * c.segs
        imgs = make(v("B"), outs=[t[f"img{i}"][0] for i in range(n)])
        kw["b_split"] = imgs
        if c.folded:
            t["imgf"][0].copy_(torch.cat(imgs))
            kw["b_split_folded"] = t["imgf"][0]
    if "gate_stats" in c.epi:
        kw["gate_stats"] = (t["gst_g"][:, :c.N], t["gst_env"][0] if c.env else None, t["gst_mean_rstd"][0],
                            t["gst_gamma"][0], t["gst_beta"][0])
    return v("A"), v("B"), v("C"), kw


# ------------------------------------------------------------------------------------------------ the contract in fp64
def _silu(x):
    return x * torch.sigmoid(x)


def _dsilu(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def bf16_products(c):
    """Precision 2 multiplies bf16-rounded operands where a bf16 kernel takes the launch; every other launch of that
    precision runs at precision 0 (include/cartnet_hip.h, CartnetGemmArgs.precision)."""
    return c.precision == 2 and not c.family.startswith("general")


def gemm_ref64(c, t):
    """cartnet_gemm as include/cartnet_hip.h documents it, in fp64 on the CPU, from the (input) tensors of make_tensors:

        C[g] = epilogue(sum_s opA(A[s]) @ opB(B[s]))

    with the operand layouts and SiLU prologues of the case, groups or K-segments, and the epilogue in the header's order:
    bias, gathered node terms, resid, the dact factor (silu', or sigmoid with dact_kind 1), the column-sum partials per
    row tile of 128, cpre, out_act (SiLU, or softplus with threshold 20 at dact_kind 1).  Returns a dict: ``C`` (per
    group; split-K: the sum of the slabs, what cartnet_splitk_reduce makes of them), ``cpre``, ``v`` (the values the
    column sums are taken of), ``a_act_out`` and, with gate statistics, ``gst_w`` / ``gst_ghat`` [M, N] so that the sums
    are sum(v w) and sum(v w ghat) per row tile.  Precision 2: bf16_products -- except the last K % 16 rows of a split-K
    weight gradient, which the header says are multiplied in fp32 as stored."""
    rnd = bf16_products(c)

    # (the last K % 16 rows of a split-K weight gradient are multiplied in fp32 as stored, at any precision)
    exact_from = (c.K // 16) * 16 if c.layout == "tn" and c.splitk > 1 else c.K

    def operand(x, act):
        x = x.detach().cpu().double()
        if act:
            x = _silu(x)
        if rnd:
            r = x.float().bfloat16().double()
            if c.layout == "tn":
                r[exact_from:] = x[exact_from:]
            x = r
        return x
    A, B = views(c, t, "A"), views(c, t, "B")

    def given(field):
        x = views(c, t, field)
        return [y.detach().cpu().double() for y in x] if x is not None else None
    bias, gi, gj, resid, dact = given("bias"), given("gather_i"), given("gather_j"), given("resid"), given("dact")
    out = dict(C=[], cpre=[], v=[], a_act_out=None)
    for g in range(c.groups):
        acc = 0.0
        for s in range(c.segs):
            i = g if c.groups > 1 else s
            a, b = operand(A[i], c.a_act), operand(B[i], c.b_act)
            if c.layout == "tn":
                a = a.t()
            elif c.layout == "nt":
                b = b.t()
            acc = acc + a @ b
        v = acc
        if bias:
            v = v + bias[g][0]
        if gi:
            v = v + gi[g][t["tgt"][0].cpu().long()] + gj[g][t["src"][0].cpu().long()]
        if resid:
            v = v + resid[g]
        if dact:
            v = v * (torch.sigmoid(dact[g]) if c.dact_kind == 1 else _dsilu(dact[g]))
        out["v"].append(v)
        out["cpre"].append(v)
        if c.out_act:
            v = torch.nn.functional.softplus(v, threshold=20.0) if c.dact_kind == 1 else _silu(v)
        out["C"].append(v)
    if "a_act_out" in c.epi:
        out["a_act_out"] = [_silu(x.detach().cpu().double()) for x in A]
    if "gate_stats" in c.epi:
        gg = t["gst_g"][:, :c.N].cpu().double()
        mr = t["gst_mean_rstd"][0].cpu().double()
        ghat = (gg - mr[:c.N]) * mr[c.N:]
        s = torch.sigmoid(ghat * t["gst_gamma"][0].cpu().double() + t["gst_beta"][0].cpu().double())
        env = t["gst_env"][0].cpu().double()[:, None] if c.env else 1.0
        out["gst_w"], out["gst_ghat"] = env * s * (1 - s), ghat
    return out


def tile_sums(x, M, N):
    """Per-row-tile column sums of x [M, N] -> [tiles, N] (the layout of colsum / colsq)."""
    tiles = (M + BM - 1) // BM
    pad = torch.zeros(tiles * BM - M, N, dtype=x.dtype)
    return torch.cat([x, pad]).view(tiles, BM, N).sum(1)


# ------------------------------------------------------------------------------------------------ the table
# Smallest launches that still reach the DMA-fed kernels (choose_bn in csrc/gemm.hip): precision 0 with weight images needs
# 64 tiles, precision 1 needs 96.  N = 512 with two groups has four tiles per row tile.
T0, T1 = 64, 96                      # tiles at which a launch with images keeps its 256-wide plan (precision 0 / 1)
M0 = rows(T0 // 4)                   # 1,921: precision 0, N = 512, two groups
M1 = rows(T1 // 4)                   # 2,945: precision 1, N = 512, two groups
M0_256 = rows(T0)                    # 8,065: precision 0, N = 256, one group
M1_256 = rows(T1)                    # 12,161: precision 1, N = 256, one group
EDGE = (0, 126, 127)                 # a last row tile of 1, 127, 128 rows


def _nn_forms(fam, i):
    """Shapes that reach the NN family ``fam`` with the fewest rows; the i-th variant rotates row edges, column tiles
    and groups (1, 2, 4 groups; one and two column tiles)."""
    e = EDGE[i % 3]
    two = dict(N=512, groups=2)
    if fam == "f32nn":                       # 256-wide tiles: forced below 200 tiles (the automatic case is at the threshold)
        return [dict(M=M0 + e, tile_policy=256, **two), dict(M=rows(16) + e, N=256, groups=4, tile_policy=256),
                dict(M=M0_256 + e, N=256, tile_policy=256)][i % 3]
    if fam == "f32nn128":
        return [dict(M=M0 + e, **two), dict(M=M0_256 + e, N=256), dict(M=rows(16) + e, N=256, groups=4, tile_policy=128)][i % 3]
    if fam == "f32nn_actout":
        return [dict(M=M0 + e, **two), dict(M=M0_256 + e, N=256), dict(M=rows(16) + e, N=256, groups=4)][i % 3]
    if fam in ("x3nn16", "x3nn_actout"):
        return [dict(M=M1 + e, precision=1, **two), dict(M=M1_256 + e, N=256, precision=1),
                dict(M=rows(24) + e, N=256, groups=4, precision=1)][i % 3]
    raise KeyError(fam)


def _build_cases():
    cs = []
    add = lambda *a, **k: cs.append(case(*a, **k))
    # ---- K-loop lengths of the DMA-fed activation x weight kernels
    for fam in ("f32nn", "f32nn128", "x3nn16", "f32nn_actout", "x3nn_actout"):
        for i, K in enumerate(KS):
            f = _nn_forms(fam, i)
            ao = fam.endswith("actout")
            add(f"{fam}-K{K}", fam, K=K, a_act=ao or i % 2 == 1, epi=("bias", "a_act_out") if ao else ("bias",), **f)
    # precision 2 reaches its kernels from M = 1: single row, a first tile that is the only full one
    for i, K in enumerate(KS):
        add(f"x3nn-K{K}", "x3nn", M=(1, 127, 128, 129, 300)[i % 5], N=(256, 512)[i % 2], K=K, precision=2,
            groups=(1, 2, 4)[i % 3], a_act=i % 4 == 3, epi=("bias",))
    add("x3nn_actout-p2", "x3nn_actout", M=129, N=256, K=48, precision=2, groups=2, a_act=True, epi=("bias", "a_act_out"))
    # ---- weight gradients: whole K, and split-K with a K tail of 1..15 rows (one more slab)
    for fam, p in (("f32tn", 0), ("x3tn", 1)):
        for i, K in enumerate(KS):
            M, N, G = (4, 124, 128, 132)[i % 4], (256, 512)[i % 2], (1, 2, 4)[i % 3]
            add(f"{fam}-K{K}", fam, M=M, N=N, K=K, layout="tn", precision=p, groups=G, b_act=i % 3 == 2)
            if K >= 32:
                tail = 1 + (5 * i) % 15
                S = 2 if K < 64 else (3 if K < 128 else 5)
                add(f"{fam}-split{S}-K{K}+{tail}", fam, M=M, N=N, K=K + tail, layout="tn", precision=p, groups=G,
                    splitk=S, b_act=i % 3 == 1)
        add(f"{fam}-split4-K512", fam, M=132, N=256, K=512, layout="tn", precision=p, groups=2, splitk=4)
    add("x3tn-p2-K144", "x3tn", M=132, N=256, K=144, layout="tn", precision=2, groups=2)
    add("x3tn-p2-split3-K100", "x3tn", M=124, N=512, K=100, layout="tn", precision=2, splitk=3, b_act=True)
    # ---- every epilogue a family accepts, one case each, and the combined forms of the model
    single = (("bias",), ("gather",), ("resid",), ("dact",), ("colsum",), ("colsum", "colsq"), ("cpre",), ("out_act",))
    combined = ((("bias", "gather"), {}), (("resid", "dact", "colsum"), {}), (("bias", "cpre", "out_act"), dict(dact_kind=1)),
                (("resid", "dact", "colsum"), dict(dact_kind=1)))
    for fam in ("f32nn", "f32nn128", "x3nn16", "f32nn_actout", "x3nn_actout"):
        ao = fam.endswith("actout")
        forms = [(e, {}) for e in single] + list(combined)
        for i, (e, extra) in enumerate(forms):
            f = _nn_forms(fam, i)
            epi = tuple(x for x in e if x != "out_act") + (("a_act_out",) if ao else ())
            add(f"{fam}-{'+'.join(e)}{'-k1' if extra else ''}", fam, K=(64, 80, 256)[i % 3], a_act=ao, out_act="out_act" in e,
                epi=epi, **f, **extra)
    for i, e in enumerate(single + tuple(e for e, _ in combined[:2])):
        add(f"x3nn-{'+'.join(e)}", "x3nn", M=(129, 300)[i % 2], N=256, K=64, precision=2, groups=(1, 2)[i % 2],
            out_act="out_act" in e, epi=tuple(x for x in e if x != "out_act"))
    for fam, p in (("f32tn", 0), ("x3tn", 1)):             # whole-K weight gradients run the tile kernels' epilogue
        for i, e in enumerate(single):
            add(f"{fam}-{'+'.join(e)}", fam, M=(124, 132)[i % 2], N=256, K=64, layout="tn", precision=p,
                groups=(1, 2)[i % 2], out_act="out_act" in e, epi=tuple(x for x in e if x != "out_act"))
    # folded K-segments (+ resid): adjacent column blocks of one matrix run as one product over K * nsegs
    add("f32nn128-folded2+resid", "f32nn128", M=M0_256, N=256, K=256, segs=2, folded=True, epi=("resid",))
    add("f32nn128-folded4+resid+dact+colsum", "f32nn128", M=rows(97), N=256, K=256, segs=4, folded=True,
        epi=("resid", "dact", "colsum"))
    add("f32nn-folded2+resid", "f32nn", M=M0_256 + 126, N=256, K=64, segs=2, folded=True, tile_policy=256, epi=("resid",))
    add("x3nn16-folded2+resid", "x3nn16", M=M1_256, N=256, K=256, segs=2, folded=True, precision=1, epi=("resid",))
    add("x3nn-folded4+resid", "x3nn", M=300, N=256, K=64, segs=4, folded=True, precision=2, epi=("resid",))
    # gate statistics: the three families that carry the epilogue
    gst = ("resid", "colsum", "colsq", "gate_stats")
    add("f32p-gate_stats", "f32p", M=M0_256, N=256, K=256, segs=2, folded=True, tile_policy=3, epi=gst)
    add("f32nn128-gate_stats", "f32nn128", M=M0_256 + 126, N=256, K=256, segs=2, folded=True, epi=gst)
    add("f32nn128-gate_stats-noresid-noenv", "f32nn128", M=M0_256, N=256, K=64, epi=gst[1:], env=False)
    add("x3nn16-gate_stats", "x3nn16", M=M1_256, N=256, K=256, segs=2, folded=True, precision=1, epi=gst)
    add("x3nn16-gate_stats-noresid", "x3nn16", M=M1_256 + 127, N=256, K=48, precision=1, epi=gst[1:])
    # ---- the persistent kernel: K = 256 / 512 / 768 only, through tile_policy = 3
    add("f32p-K256-bias", "f32p", M=M0 + 126, N=512, K=256, groups=2, tile_policy=3, epi=("bias",))
    add("f32p-K256-silu-bias-stats-actout", "f32p", M=M0_256, N=256, K=256, tile_policy=3, a_act=True,
        epi=("bias", "colsum", "colsq", "a_act_out"))
    add("f32p-K512-cpre-silu-out", "f32p", M=rows(16, 127), N=256, K=512, groups=4, tile_policy=3, a_act=True, out_act=True,
        epi=("bias", "cpre", "a_act_out"))
    add("f32p-K256-gather", "f32p", M=M0, N=512, K=256, groups=2, tile_policy=3, epi=("bias", "gather"))
    add("f32p-K512-resid-dact-colsum", "f32p", M=M0_256, N=256, K=256, segs=2, folded=True, tile_policy=3,
        epi=("resid", "dact", "colsum"))
    add("f32p-K768-resid", "f32p", M=M0_256 + 126, N=256, K=256, segs=3, folded=True, tile_policy=3, epi=("resid",))
    add("f32p-K256-softplus-forward", "f32p", M=M0_256, N=256, K=256, tile_policy=3, out_act=True, dact_kind=1,
        epi=("bias", "cpre"))
    add("f32p-K512-softplus-backward", "f32p", M=M0_256, N=256, K=256, segs=2, folded=True, tile_policy=3, dact_kind=1,
        epi=("resid", "dact", "colsum"))
    # ---- thresholds: the case at the threshold and the case one row tile below it (see THRESHOLDS)
    add("at-64-tiles", "f32nn128", M=rows(64), N=256, K=64, epi=("bias",))
    add("below-64-tiles", "general64", M=rows(64) - 1, N=256, K=64, epi=("bias",))
    add("at-200-tiles-images", "f32nn", M=rows(50), N=512, K=32, groups=2, epi=("bias",))
    add("below-200-tiles-images", "f32nn128", M=rows(50) - 1, N=512, K=32, groups=2, epi=("bias",))
    add("actout-at-64-tiles", "f32nn_actout", M=rows(16), N=512, K=32, groups=2, a_act=True, epi=("bias", "a_act_out"))
    add("actout-below-64-tiles", "general64", M=rows(16) - 1, N=512, K=32, groups=2, a_act=True, epi=("bias", "a_act_out"))
    add("at-200-tiles-no-image", "general256", M=rows(25), N=512, K=40, groups=4, layout="nt", epi=("bias",))
    add("below-200-tiles-no-image", "general128", M=rows(25) - 1, N=512, K=40, groups=4, layout="nt", epi=("bias",))
    add("at-100-tiles", "general128", M=rows(25), N=256, K=40, groups=4, layout="nt", epi=("bias",))
    add("below-100-tiles", "general64", M=rows(25) - 1, N=256, K=40, groups=4, layout="nt", epi=("bias",))
    add("p1-at-96-tiles", "x3nn16", M=rows(24), N=512, K=32, groups=2, precision=1, epi=("bias",))
    add("p1-below-96-tiles", "general128", M=rows(24) - 1, N=512, K=32, groups=2, precision=1, epi=("bias",))
    add("p1-actout-at-96-tiles", "x3nn_actout", M=rows(24), N=256, K=32, groups=4, precision=1, a_act=True,
        epi=("bias", "a_act_out"))
    add("p1-actout-below-96-tiles", "general128", M=rows(24) - 1, N=256, K=32, groups=4, precision=1, a_act=True,
        epi=("bias", "a_act_out"))
    add("p1-no-image-at-96-tiles", "general_x3", M=rows(24), N=512, K=48, groups=2, precision=1, image=False, epi=("bias",))
    add("p1-no-image-below-96-tiles", "general128", M=rows(24) - 1, N=512, K=48, groups=2, precision=1, image=False,
        epi=("bias",))
    add("f32p-at-1024-tiles", "f32p", M=rows(256), N=256, K=256, groups=4, epi=("bias",))
    add("f32p-below-1024-tiles", "f32nn", M=rows(256) - 1, N=256, K=256, groups=4, epi=("bias",))
    add("tn-at-one-K-step", "f32tn", M=128, N=256, K=16, layout="tn")
    add("tn-below-one-K-step", "general256", M=128, N=256, K=15, layout="tn")
    # ---- fallbacks: a mis-aligned operand (base + 4 bytes) and an ldc that is no multiple of 4 plan to the general kernel
    add("misaligned-A", "general256", M=rows(200), N=256, K=64, off_a=1, pad_a=15, epi=("bias",))
    add("misaligned-A-few-tiles", "general64", M=M0_256, N=256, K=64, off_a=1, pad_a=15, epi=("bias", "resid"))
    add("odd-ldc", "general256", M=rows(200), N=256, K=64, pad_c=3, epi=("bias",))
    add("odd-ldc-few-tiles", "general64", M=M0_256, N=256, K=64, pad_c=3, epi=("bias", "cpre"))
    add("p1-misaligned-A", "general_x3", M=M1_256, N=256, K=64, precision=1, off_a=1, pad_a=15, epi=("bias",))
    add("p2-odd-ldc", "general256", M=300, N=256, K=64, precision=2, pad_c=3, epi=("bias",))
    add("tn-misaligned-A", "general256", M=128, N=256, K=64, layout="tn", off_a=1, pad_a=15)
    # ---- the general kernel's own forms: NT (weights as stored), ragged N and K
    add("general64-nt", "general64", M=129, N=64, K=67, layout="nt", epi=("bias",))
    add("general128-nt", "general128", M=333, N=128, K=256, layout="nt", a_act=True, out_act=True, epi=("bias", "cpre"))
    add("general256-nt-ragged", "general256", M=5, N=200, K=40, layout="nt")
    add("general-segments", "general64", M=450, N=64, K=64, segs=2, image=False, epi=("resid", "dact"))
    return cs


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "duplicate case names"

# (family with a shape threshold, the case at the threshold, the case one row tile (or K-step) below: the other family)
THRESHOLDS = (
    ("f32nn128", "at-64-tiles", "below-64-tiles"),
    ("f32nn", "at-200-tiles-images", "below-200-tiles-images"),
    ("f32nn_actout", "actout-at-64-tiles", "actout-below-64-tiles"),
    ("general256", "at-200-tiles-no-image", "below-200-tiles-no-image"),
    ("general128", "at-100-tiles", "below-100-tiles"),
    ("x3nn16", "p1-at-96-tiles", "p1-below-96-tiles"),
    ("x3nn_actout", "p1-actout-at-96-tiles", "p1-actout-below-96-tiles"),
    ("general_x3", "p1-no-image-at-96-tiles", "p1-no-image-below-96-tiles"),
    ("f32p", "f32p-at-1024-tiles", "f32p-below-1024-tiles"),
    ("f32tn", "tn-at-one-K-step", "tn-below-one-K-step"),
)

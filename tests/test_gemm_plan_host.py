"""The kernel family of every GEMM case, asserted on the host (no GPU): cartnet_gemm_plan is the code cartnet_gemm plans
its launch with, so a routing threshold that moves shows here, by case name, before any GPU run.

* every case of tests/gemm_cases.py plans to the family and tile width it names;
* all 13 families, and all three widths of the general kernel, are the expected family of at least one case;
* every family with a shape threshold has the case at the threshold and the case one row tile below it, which plans to
  another family;
* the launches of one CartNet training step at the benchmark batch (N = 12,416 atoms, E = 177,140 edges, D = 256), and the
  iComformer products with tile_policy = 1, plan to the families the comments in csrc/model.hip, csrc/icomformer.hip and
  csrc/gemm.hip and the variant names of the committed benchmark records (profiles/r06_bench_n1.json) name;
* what cartnet_gemm refuses, the query refuses with the same message.
"""
import ctypes

import pytest

import gemm_cases as gc


@pytest.fixture(scope="module")
def lib():
    from cartnet_amd import build, lib as _lib
    build.build(verbose=False)
    _lib.load()
    return _lib


ALL_FAMILIES = ("general64", "general128", "general256", "general_x3", "f32p", "f32nn", "f32nn_actout", "f32nn128", "f32tn",
                "x3nn16", "x3nn", "x3nn_actout", "x3tn", "hnn", "htn")


def test_family_enumerators_are_published_and_stable(lib):
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "cartnet_hip.h")).read()
    enum = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"CARTNET_GEMM_([A-Z0-9_]+) = (-?\d+)", hdr)}
    assert enum.pop("none") == -1 and enum.pop("families") == 13 == len(lib.GEMM_FAMILIES)
    assert enum == {name: i for i, name in enumerate(lib.GEMM_FAMILIES)}
    assert {f[:7] if f.startswith("general") and f[7:].isdigit() else f for f in ALL_FAMILIES} == set(lib.GEMM_FAMILIES)


@pytest.mark.parametrize("c", gc.CASES, ids=lambda c: c.name)
def test_every_case_plans_to_its_family(lib, c):
    rc, info = gc.plan_of(c, lib)
    assert rc == 0, lib.load().cartnet_last_error()
    assert gc.family_name(info, lib) == c.family, (c.name, info.width, info.prepass, info.k_folded)
    assert info.width == gc.width_of(c.family)
    assert info.reject == 0
    # the launch as it runs: adjacent K-segments with the folded image become one product over K * nsegs
    folds = c.folded and c.family not in ("general64", "general128")
    assert (info.k_folded, info.nsegs_run) == ((c.K * c.segs, 1) if folds else (c.K, c.segs))
    # silu(A) is written by the kernel itself only in the families that have the form
    if "a_act_out" in c.epi:
        assert info.prepass == (0 if c.family in ("f32nn_actout", "x3nn_actout", "f32p") else 1)
    assert info.gate_stats == (1 if c.family in ("f32p", "f32nn128", "x3nn16") else 0)


SMALL_CASES = [c for c in gc.CASES if c.M <= 300 and c.K <= 300]


def test_tails_cover_every_row_indexed_buffer_of_every_case():
    """gemm_cases.tail_kind names, for every case, exactly the buffers whose first dimension is the launch's M (K for the
    tn layout's operands; splitk * M for the slabs) or, for the row vectors tgt / src / gst_env, whose length is."""
    for c in gc.CASES:
        buf, _ = gc._buffers(c)
        rows_ = c.K if c.layout == "tn" else c.M
        for name, (r, w, dt) in buf.items():
            kind = gc.tail_kind(c, name)
            if name in ("tgt", "src", "gst_env"):
                assert kind is not None and kind[0] == 1 and (r, w) == (1, c.M), (c.name, name)
            elif name.startswith(("bias", "Gi", "Gj", "colsum", "colsq", "img", "gst_mean", "gst_gamma", "gst_beta")) or \
                    (name[0] == "B" and name != "B"):
                assert kind is None, (c.name, name)
            else:
                want = c.splitk * c.M if name[0] == "C" and name != "C" else (rows_ if name in ("A", "B", "H") else c.M)
                assert kind is not None and kind[0] == 0 and r == want, (c.name, name, r, want)
                assert (kind[1] == gc.SENTINEL) == (name[0] in "CPH"), (c.name, name)


@pytest.mark.parametrize("c", SMALL_CASES, ids=lambda c: c.name)
def test_operands_are_views_of_longer_buffers_with_the_same_leading_dimension(c):
    """make_tensors on the CPU: each row-indexed buffer is the first rows of an allocation TAIL rows longer, fake_args and
    gemm_ref64 see the case's own M and K, and the fp64 statement is finite (no tail reaches it)."""
    import torch
    t = gc.make_tensors(c, "cpu")
    buf, _ = gc._buffers(c)
    assert len(SMALL_CASES) >= 40 and t.full
    for name, full in t.full.items():
        r, w, _ = buf[name]
        axis, _ = gc.tail_kind(c, name)
        assert tuple(t[name].shape) == (r, w) and t[name].data_ptr() == full.data_ptr()
        assert tuple(full.shape) == ((r + gc.TAIL, w) if axis == 0 else (r, w + gc.TAIL))
        assert t[name].stride(0) == full.stride(0)
    gc.assert_tails(c, t)
    for f in ("A", "B", "C"):
        for v in gc.views(c, t, f):
            assert v.shape[0] == buf[f if f in buf else f + "0"][0]
    ref = gc.gemm_ref64(c, t)
    assert all(bool(torch.isfinite(x).all()) for x in ref["C"])
    t.full["C" if "C" in t.full else "C0"][-1, 0] = 0.0              # an overwritten tail cell is reported
    with pytest.raises(AssertionError, match="behind the last row"):
        gc.assert_tails(c, t)


# the half-storage families: planned here from fake pointers, computed in tests/test_gpu_half_storage_kernels.py and the
# half-storage block of tests/test_gpu_kernels.py (which assert the family of every launch)
def _half(lib, layout, **flags):
    c = gc.case("half", "hnn" if layout == "nn" else "htn", M=300 if layout == "nn" else 256, N=256, K=256, layout=layout,
                precision=2, groups=2)
    a = gc.fake_args(c, lib)
    for k, v in flags.items():
        setattr(a, k, v)
    info = lib.GemmPlanInfo()
    rc = lib.load().cartnet_gemm_plan(ctypes.byref(a), ctypes.byref(info))
    return rc, info


def test_every_family_and_every_general_width_is_expected_by_a_case(lib):
    expected = {c.family for c in gc.CASES}
    rc, info = _half(lib, "nn", a_half=1)
    assert rc == 0 and gc.family_name(info, lib) == "hnn"
    rc, info = _half(lib, "tn", a_half=1, b_half=1)
    assert rc == 0 and gc.family_name(info, lib) == "htn"
    assert expected | {"hnn", "htn"} == set(ALL_FAMILIES)
    # ... and no case expects a family it could not name
    assert expected <= set(ALL_FAMILIES)


@pytest.mark.parametrize("family,at,below", gc.THRESHOLDS, ids=[t[0] for t in gc.THRESHOLDS])
def test_thresholded_families_have_a_case_on_each_side(lib, family, at, below):
    a, b = gc.BY_NAME[at], gc.BY_NAME[below]
    assert a.family == family != b.family
    same = lambda x: {k: v for k, v in vars(x).items() if k not in ("name", "family", "M", "K")}
    assert same(a) == same(b)
    if a.layout == "tn":                    # the weight gradients' threshold is one K-step of 16 rows
        assert (a.K, b.K, a.M) == (16, 15, b.M)
    else:                                   # one row tile less: the last tile of one row is gone
        assert a.K == b.K and a.M == b.M + 1 and b.M % gc.BM == 0
    for c in (a, b):
        rc, info = gc.plan_of(c, lib)
        assert rc == 0 and gc.family_name(info, lib) == c.family, c.name


def test_thresholds_cover_every_family_that_has_one():
    # no shape threshold: x3nn and x3nn_actout at precision 2 (from M = 1), x3tn (as f32tn: one K-step), hnn / htn (precision 2)
    assert {t[0] for t in gc.THRESHOLDS} == set(ALL_FAMILIES) - {"general64", "x3nn", "x3tn", "hnn", "htn"}


# ---- one CartNet training step at the benchmark batch, and iComformer's tile_policy = 1 products
N_ATOMS, E_EDGES, D = 12416, 177140, 256
_C = gc.case
STEP = (
    # forward (csrc/model.hip)
    _C("edge encoder, first Linear: feat [E, 80] -> 2D", "f32nn", M=E_EDGES, N=2 * D, K=80, epi=("bias",)),
    _C("edge encoder, second Linear: K = 512, pre kept, silu out, silu(A) written", "f32p", M=E_EDGES, N=D, K=2 * D, a_act=True,
       out_act=True, epi=("bias", "cpre", "a_act_out")),
    _C("atom encoder Linear (side stream)", "f32nn128", M=N_ATOMS, N=D, K=2 * D, a_act=True, out_act=True, epi=("bias", "cpre")),
    _C("node terms: four groups into Pn", "f32nn", M=N_ATOMS, N=D, K=D, groups=4, epi=("bias",)),
    _C("layer product 1: two groups, node terms gathered", "f32p", M=E_EDGES, N=D, K=D, groups=2, epi=("gather",),
       gather_rows=N_ATOMS),
    _C("layer product 2: silu(pre), bias, BatchNorm sums, silu(pre) written", "f32p", M=E_EDGES, N=D, K=D, groups=2, a_act=True,
       epi=("bias", "colsum", "colsq", "a_act_out")),
    # backward
    _C("dpre: two groups, * silu'(pre)", "f32p", M=E_EDGES, N=D, K=D, groups=2, epi=("dact",)),
    _C("dE: two folded K-segments + residual + gate statistics", "f32p", M=E_EDGES, N=D, K=D, segs=2, folded=True,
       epi=("resid", "colsum", "colsq", "gate_stats")),
    _C("dE of layer 0: + silu'(e0_pre) and the bias gradient", "f32p", M=E_EDGES, N=D, K=D, segs=2, folded=True,
       epi=("resid", "dact", "colsum")),
    _C("dX: four folded K-segments at 12,416 rows (97 row tiles)", "f32nn128", M=N_ATOMS, N=D, K=D, segs=4, folded=True,
       epi=("resid",)),
    _C("dX of layer 0: + silu'(xa_pre) and the bias gradient", "f32nn128", M=N_ATOMS, N=D, K=D, segs=4, folded=True,
       epi=("resid", "dact", "colsum")),
    _C("dhe = d(he_pre): N = 512, * silu'(he_pre) and the bias gradient", "f32p", M=E_EDGES, N=2 * D, K=D, epi=("dact", "colsum")),
    _C("weight gradients of the second Linears from the kept silu(pre): split-K over E", "f32tn", M=D, N=D, K=E_EDGES,
       layout="tn", groups=2, splitk=64),
    _C("weight gradients of the first Linears, node blocks: split-K over N", "f32tn", M=D, N=D, K=N_ATOMS, layout="tn",
       groups=4, splitk=32),
    _C("weight gradient recomputing silu(X)", "f32tn", M=D, N=D, K=N_ATOMS, layout="tn", b_act=True, splitk=48),
    # bf16x3 (gemm_precision 1): the same products
    _C("precision 1, layer product 1", "x3nn16", M=E_EDGES, N=D, K=D, groups=2, precision=1, epi=("gather",)),
    _C("precision 1, layer product 2", "x3nn_actout", M=E_EDGES, N=D, K=D, groups=2, precision=1, a_act=True,
       epi=("bias", "colsum", "colsq", "a_act_out")),
    _C("precision 1, dX at 97 row tiles stays on the DMA-fed kernel (few = 96)", "x3nn16", M=N_ATOMS, N=D, K=D, segs=4,
       folded=True, precision=1, epi=("resid",)),
    _C("precision 1, weight gradients", "x3tn", M=D, N=D, K=E_EDGES, layout="tn", groups=2, precision=1, splitk=64),
    # iComformer (csrc/icomformer.hip: every product carries tile_policy = 1 unless it resets it)
    _C("iComformer Q K V of the atoms: three groups", "f32nn128", M=N_ATOMS, N=D, K=D, groups=3, tile_policy=1, epi=("bias",)),
    _C("iComformer Q K V of the edges: three groups (no persistent form)", "f32nn128", M=E_EDGES, N=D, K=D, groups=3,
       tile_policy=1, epi=("bias",)),
    _C("iComformer key / message first Linears of the edges: two groups", "f32p", M=E_EDGES, N=D, K=D, groups=2, tile_policy=1,
       epi=("bias",)),
    _C("iComformer concatenation Linear of the edges + BatchNorm sums", "f32p", M=E_EDGES, N=D, K=D, tile_policy=1,
       epi=("bias", "colsum", "colsq")),
    _C("iComformer RBF branch: pre kept, softplus out", "f32p", M=E_EDGES, N=D, K=D, tile_policy=1, out_act=True, dact_kind=1,
       epi=("bias", "cpre")),
    _C("iComformer d(rows): two folded segments, * sigmoid(pre), bias gradient", "f32p", M=E_EDGES, N=D, K=D, segs=2,
       folded=True, tile_policy=1, dact_kind=1, epi=("resid", "dact", "colsum")),
    _C("the same grouped product without tile_policy = 1 (CartNet's node terms)", "f32nn", M=N_ATOMS, N=D, K=D, groups=3,
       epi=("bias",)),
)


@pytest.mark.parametrize("c", STEP, ids=lambda c: c.name)
def test_training_step_launches_plan_to_the_documented_families(lib, c):
    rc, info = gc.plan_of(c, lib)
    assert rc == 0, lib.load().cartnet_last_error()
    assert gc.family_name(info, lib) == c.family
    assert info.prepass == 0                          # at the benchmark batch no launch needs the elementwise pre-pass
    # bits 4..7 of the launch timer's key: the tile width / 64; bit 18: the persistent kernel (ops.profile_gemm_read names
    # them nn128 / nn256 / nn256p / tn256 in the benchmark records)
    assert (info.variant >> 4) & 15 == (2 if c.family == "f32nn128" else 4)
    assert bool(info.variant & (1 << 18)) == (c.family == "f32p")


# ---- refusals: the query answers as cartnet_gemm does
def _both(lib, a):
    l = lib.load()
    info = lib.GemmPlanInfo()
    rc_plan = l.cartnet_gemm_plan(ctypes.byref(a), ctypes.byref(info))
    msg_plan = l.cartnet_last_error()
    rc_run = l.cartnet_gemm(ctypes.byref(a), None)      # refused before any launch: no GPU needed
    msg_run = l.cartnet_last_error()
    assert rc_plan != 0 and rc_run != 0 and msg_plan == msg_run
    assert info.family == -1
    return msg_plan, info


def test_refusals_are_the_same_through_the_query(lib):
    base = lambda **kw: gc.fake_args(gc.case("refused", "none", M=300, N=256, K=64, **kw), lib)
    # the layout / activation combination: SiLU on B of an activation x weight product
    a = base(b_act=True)
    msg, info = _both(lib, a)
    assert b"unsupported layout/activation combination" in msg and info.reject == 1
    a = base(layout="nt", b_act=True)
    assert b"unsupported layout" in _both(lib, a)[0]
    # half storage without a compiled combination: precision 0; no weight image; a bf16 weight operand
    a = base()
    a.a_half = 1
    assert b"need precision 2" in _both(lib, a)[0]
    a = base(precision=2, image=False)
    a.a_half = 1
    msg, info = _both(lib, a)
    assert b"no half-storage kernel" in msg and info.reject == 2
    a = base(precision=2)
    a.b_half = 1
    assert b"half storage" in _both(lib, a)[0]
    # gst_* where no kernel carries it: too few row tiles, precision 2, an epilogue the form does not have
    gst = ("resid", "colsum", "colsq", "gate_stats")
    a = gc.fake_args(gc.case("refused", "none", M=gc.rows(64) - 1, N=256, K=64, epi=gst), lib)
    assert b"gst_g is set" in _both(lib, a)[0]
    a = gc.fake_args(gc.case("refused", "none", M=gc.rows(96), N=256, K=64, precision=2, epi=gst), lib)
    assert b"gst_g is set" in _both(lib, a)[0]
    a = gc.fake_args(gc.case("refused", "none", M=gc.rows(64), N=256, K=64, epi=gst + ("bias",)), lib)
    assert b"gst_g is set" in _both(lib, a)[0]
    # split-K with an epilogue, with K-segments, with too short a K
    a = base(layout="tn", splitk=2, epi=("bias",))
    assert b"no epilogue allowed" in _both(lib, a)[0]
    a = gc.fake_args(gc.case("refused", "none", M=128, N=256, K=31, layout="tn", splitk=2), lib)
    assert b"split-K needs K >= 32" in _both(lib, a)[0]
    # the plain argument checks
    a = base()
    a.tile_policy = 2
    assert b"tile_policy=2" in _both(lib, a)[0]
    a = base(epi=("a_act_out",))                        # a_act_out without a_act
    assert b"a_act_out needs a_act" in _both(lib, a)[0]
    a = base()
    a.C[0] = None
    assert b"null output" in _both(lib, a)[0]
    l = lib.load()
    assert l.cartnet_gemm_plan(None, ctypes.byref(lib.GemmPlanInfo())) != 0 and b"null args" in l.cartnet_last_error()
    assert l.cartnet_gemm_plan(ctypes.byref(base()), None) != 0 and b"null out" in l.cartnet_last_error()


def test_an_empty_launch_plans_to_nothing(lib):
    a = gc.fake_args(gc.case("empty", "none", M=300, N=256, K=64), lib)
    a.M = 0
    info = lib.GemmPlanInfo()
    assert lib.load().cartnet_gemm_plan(ctypes.byref(a), ctypes.byref(info)) == 0 and info.family == -1

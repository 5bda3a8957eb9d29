"""CPU-only: the workspace sizes of the two step drivers (csrc/model.hip, csrc/icomformer.hip) are pure host arithmetic --
what carve / icarve take from the workspace, in which order.  tests/golden/workspace_bytes.json holds the numbers of the
commit before the drivers moved onto the shared kit of csrc/model_common.h; they must not move."""
import ctypes
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")

SHAPES = [(1, 0, 1, 1), (5, 12, 1, 3), (777, 20011, 7, 500), (12416, 620800, 64, 9000)]            # (N, E, Bg, M)
# (D, L, precision, bn_group_size, half_storage, invariant, cholesky)
CARTNET = [(256, 4, 0, 0, 0, 0, 1), (256, 4, 1, 0, 0, 0, 1), (256, 4, 2, 0, 1, 0, 1), (256, 4, 0, 4, 0, 0, 1),
           (64, 2, 0, 0, 0, 0, 1), (256, 4, 0, 0, 0, 1, 0)]
ICOMFORMER = [(256, 0, 0), (256, 1, 0), (256, 0, 4), (64, 0, 0), (512, 0, 0)]                       # (C, precision, bn_group_size)


def measure():
    """{key: bytes} for every variant x shape; only the scalar fields of the model structs are set, every pointer is null."""
    from cartnet_amd import lib
    l = lib.load()
    out = {}
    for D, L, prec, group, half, invariant, cholesky in CARTNET:
        m = lib.Model()
        m.D, m.L, m.R, m.n_types = D, L, 64, 119
        m.use_temperature = m.atom_types = 1
        m.invariant, m.cholesky = invariant, cholesky
        m.gemm_precision, m.bn_group_size, m.half_storage = prec, group, half
        for N, E, Bg, M in SHAPES:
            for bwd in (0, 1):
                key = f"cartnet D={D} L={L} prec={prec} group={group} half={half} inv={invariant} chol={cholesky} " \
                      f"N={N} E={E} Bg={Bg} M={M} bwd={bwd}"
                out[key] = int(l.cartnet_workspace_bytes(ctypes.byref(m), N, E, Bg, M, bwd))
    for Cdim, prec, group in ICOMFORMER:
        m = lib.IcfModel()
        m.C, m.n_types, m.gemm_precision, m.bn_group_size = Cdim, 119, prec, group
        for N, E, Bg, M in SHAPES:
            key = f"icomformer C={Cdim} prec={prec} group={group} N={N} E={E} Bg={Bg} M={M}"
            out[key] = int(l.cartnet_icomformer_workspace_bytes(ctypes.byref(m), N, E, Bg, M))
    return out


def test_workspace_bytes_are_those_of_the_drivers_before_the_shared_kit():
    golden = json.load(open(GOLDEN))
    got = measure()
    assert len(golden) == len(CARTNET) * len(SHAPES) * 2 + len(ICOMFORMER) * len(SHAPES) == 68
    assert sorted(got) == sorted(golden)
    assert all(v > 0 for v in golden.values())
    wrong = {k: (got[k], golden[k]) for k in golden if got[k] != golden[k]}
    assert not wrong, f"workspace sizes moved (got, expected): {wrong}"
    # the figures the issue quotes for the parent commit
    at = "N=777 E=20011 Bg=7 M=500"
    assert golden[f"cartnet D=256 L=4 prec=1 group=0 half=0 inv=0 chol=1 {at} bwd=0"] == 246886912
    assert golden[f"cartnet D=256 L=4 prec=1 group=0 half=0 inv=0 chol=1 {at} bwd=1"] == 769131776
    assert golden[f"icomformer C=256 prec=0 group=0 {at}"] == 2197169920
    assert golden[f"icomformer C=256 prec=0 group=4 {at}"] == 2197210880

"""``--predict --model icomformer --model_frame reduced_cell`` on the host: the two entry points' declarations and bindings
and their returns that need no launch, the flag and its refusals (``--rotations K > 1`` among them), the new row of
``predict.GROUPS``, the fixture crystals,
and ``cartnet_adp_stored_frame`` restated on the host (tests/model_frame_utils.py), which states the bits the GPU tests
expect (no GPU)."""
import os
import re
import types

import numpy as np
import pytest
import torch

import model_frame_utils as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSAL = "--predict --model icomformer serves one frame only"


def test_entry_points_are_declared_and_bound_and_the_abi_is_16():
    from cartnet_amd import lib
    hdr = open(os.path.join(ROOT, "include", "cartnet_hip.h")).read()
    assert "dataset/datasetADP.py:75-80" in hdr and "main.py:95-97" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n in (("cartnet_collate_frame_view", 8), ("cartnet_adp_stored_frame", 8)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and len(m.group(1).split(",")) == n == len(lib.PROTOTYPES[name][1]), name
    assert lib.ABI_VERSION == 16 == lib.load().cartnet_abi_version()          # no struct changed
    for name, n in (("cartnet_collate", 14), ("cartnet_adp_frame_mean", 10), ("cartnet_shard_optimize_cell_rotate", 8)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and len(m.group(1).split(",")) == n == len(lib.PROTOTYPES[name][1]), name     # where they were


def test_no_launch_and_refusal_returns():
    from cartnet_amd import lib
    l = lib.load()
    f = l.cartnet_adp_stored_frame
    assert f(None, None, None, 4, 0, 3, None, None) == 0                      # no rows
    assert f(None, None, None, 0, 0, 1, None, None) == 0                      # no crystals
    for bad in ((4, 5, 0), (4, 0, 0), (4, -1, 1), (-1, 5, 1), (4, 5, 65536)):  # T is checked before the early return
        assert f(None, None, None, bad[0], bad[1], bad[2], None, None) != 0
        assert b"cartnet_adp_stored_frame: bad sizes" in l.cartnet_last_error()
    assert f(None, None, None, 2, 5, 1, None, None) != 0                      # before any launch
    assert b"cartnet_adp_stored_frame: null pointer" in l.cartnet_last_error()
    v = l.cartnet_collate_frame_view
    assert v(None, None, None, 1, 0, None, None, None) != 0
    assert b"cartnet_collate_frame_view: null descriptor" in l.cartnet_last_error()
    s = lib.Shard()
    for bad in ((0, 0), (2, -1)):
        assert v(lib.C.byref(s), None, None, bad[0], bad[1], None, None, None) != 0
        assert b"cartnet_collate_frame_view: bad sizes" in l.cartnet_last_error()
    assert v(lib.C.byref(s), None, None, 2, 7, None, None, None) != 0         # before any launch
    assert b"cartnet_collate_frame_view: null selection" in l.cartnet_last_error()


def test_rotations_with_icomformer_exits_with_the_reason_before_the_device_is_touched(monkeypatch):
    import main as entry
    from cartnet_amd.config import cfg, set_cfg

    def touched(*a, **k):
        raise AssertionError("--predict --model icomformer --rotations 2 went on past its argument check")
    monkeypatch.setattr(entry.cdist, "init_from_env", touched)
    monkeypatch.setattr(entry, "create_model", touched)
    plain = ["--predict", "--model", "icomformer", "--predict_input", "x.cnshard", "--checkpoint_path", "x.ckpt"]
    argv = plain + ["--model_frame", "reduced_cell"]
    try:
        with pytest.raises(SystemExit) as e:
            entry.main(argv + ["--rotations", "2"])
        text = str(e.value)
        assert REFUSAL in text and "invariant" in text and "cart_dir but not the cell" in text and "averaged" in text
        # the frame is asked for by name: without the flag the old refusal stands and now says what to give
        assert entry.build_parser().parse_args([]).model_frame == "stored"
        with pytest.raises(SystemExit, match="--predict does not serve --model icomformer in the stored frame.*"
                                             "--model_frame reduced_cell"):
            entry.main(plain)
        for model in ("CartNet", "ecomformer"):
            with pytest.raises(SystemExit, match="--model_frame reduced_cell serves --model icomformer only"):
                entry.main(["--predict", "--model", model] + argv[3:])
        with pytest.raises(SystemExit, match="--model_frame serves --predict only"):
            entry.main(["--model", "icomformer", "--model_frame", "reduced_cell", "--inference"])
        # one frame is served: the argument check passes, also with every analysis flag and a temperature series
        for extra in ([], ["--rotations", "1"], ["--rigid_bond", "--riding_h", "--rigid_molecule", "--tls_fit", "--aniso_h",
                                                 "--bond_table", "--angle_table", "--predict_temperatures", "100,200,300",
                                                 "--predict_cif_dir", "c", "--eval_batch", "4"]):
            args = entry.build_parser().parse_args(argv + extra)
            entry.fill_cfg(args)
            entry.check_predict_args(args)
            assert cfg.model == "icomformer" and cfg.max_neighbours == args.max_neighbours
        with pytest.raises(SystemExit, match="--riding_h with --disable_H"):     # the other refusals are where they were
            args = entry.build_parser().parse_args(argv + ["--riding_h", "--disable_H"])
            entry.fill_cfg(args)
            entry.check_predict_args(args)
    finally:
        set_cfg()


def test_the_group_is_present_only_with_the_keyword():
    from cartnet_amd import predict as p
    from cartnet_amd.predict import Analyses, result_keys
    assert p.MF_KEYS == ("cell_rotation", "cell_reduced") == tuple(p.GROUPS["model_frame"].cuts)
    assert list(p.GROUPS["model_frame"].cuts.values()) == ["crystal", "crystal"]
    assert p.CUT["cell_rotation"] == p.CUT["cell_reduced"] == "crystal" and "cell_rotation" not in p.SPLIT
    names = list(p.GROUPS)
    assert names.index("model_frame") == names.index("base") + 1
    every = Analyses(rigid_bond=(0.4, 1e-3), riding_h=(0.4, 1.2, 1.5), rigid_molecule=(0.4, 1e-3), tls_fit=True,
                     aniso_h=(0.005, 0.020))
    for a, sym, bt, at in ((Analyses(), False, None, None), (every, True, 0.4, 0.4), (every, False, None, 0.4)):
        off = result_keys(a, sym, 1, bt, at)
        assert result_keys(a, sym, 1, bt, at, False) == off and not set(p.MF_KEYS) & set(off)
        on = result_keys(a, sym, 1, bt, at, True)
        assert on == p.KEYS + p.MF_KEYS + off[len(p.KEYS):]                   # after the base keys, nothing else moves
    for name, g in p.GROUPS.items():                                          # no other row looks at the switch
        args = (every, True, 2, [100.0, 200.0], 0.4, 0.4)
        assert bool(g.present(*args, True)) == (True if name == "model_frame" else bool(g.present(*args))), name
    assert not p.GROUPS["model_frame"].present(*args) and not p.GROUPS["model_frame"].present(*args, False)


def test_predict_adps_refuses_frames_with_a_model_frame():
    from cartnet_amd.predict import predict_adps
    shard = types.SimpleNamespace(per_atom_target=True, t={"pos": 0, "cell": 0, "non_h_mask": 0}, num_graphs=1)
    with pytest.raises(ValueError, match="model_frame serves one frame only"):
        predict_adps(None, types.SimpleNamespace(shard=shard), "cpu", rotations=2, model_frame=object())


def test_the_fixture_crystals_are_what_the_issue_asks_for():
    for restored in (False, True):
        items = mf.crystals(True, restored)
        assert len(items) == 4 and all(3 <= int(d.x.shape[0]) <= 12 for d in items)
        assert sum(bool((d.x == 1).any()) for d in items) == 1
        assert all(int(d.edge_index.shape[1]) > 0 and int(d.y.shape[0]) == int((d.x != 1).sum()) for d in items)
        if not restored:
            mf.check_crystals(items)
    from cartnet_amd.data import lattice_margins, optimize_lattice
    Q = mf.restore_rotations()
    for g, (a, b) in enumerate(zip(mf.crystals(False), mf.crystals(False, True))):
        gap, cos = lattice_margins(b.cell[0])
        assert gap >= 1e-3 and cos >= 1e-3, (g, gap, cos)
        assert abs(np.linalg.det(Q[g]) - 1.0) < 1e-6 and np.abs(Q[g] @ Q[g].T - np.eye(3)).max() < 1e-6
        assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.cart_dist, b.cart_dist)
        ca, cb = optimize_lattice(a.cell[0])[0], optimize_lattice(b.cell[0])[0]     # the same lattice: the same reduced cell
        assert float((ca - cb).abs().max()) <= 1e-5 * float(ca.abs().max()), g
        assert not torch.equal(a.cell, b.cell) and not hasattr(a, "y")


def _rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, 3, generator=g).numpy()


def _rotations(n, seed):
    from cartnet_amd.synthetic import random_rotation
    g = torch.Generator().manual_seed(seed)
    return torch.stack([random_rotation(g) for _ in range(n)]).numpy()


def test_the_host_form_states_the_expected_bits():
    ptr = [0, 5, 5, 12]                                                       # an empty crystal between two full ones
    R = _rotations(3, 11)
    for T in (1, 3):
        P = _rows(12 * T, 20 + T)
        out = mf.stored_frame_host(P, R, ptr, T)
        assert out.dtype == np.float32 and out.shape == (12 * T, 3, 3)
        # the identity gives pred's bits
        eye = np.tile(np.eye(3, dtype=np.float32), (3, 1, 1))
        assert mf.stored_frame_host(P, eye, ptr, T).tobytes() == P.tobytes()
        # against plain fp64 numpy: R P R^T of the row's crystal, the T slices sharing the rotations; the chains differ
        # from numpy's products in the last bits of the fp64 value, so after the one rounding by at most one fp32 unit
        crystal = np.repeat(np.arange(3), np.diff(ptr))
        for t in range(T):
            sl = slice(12 * t, 12 * (t + 1))
            Rg = R[crystal].astype(np.float64)
            want = Rg @ P[sl].astype(np.float64) @ Rg.transpose(0, 2, 1)
            assert np.abs(out[sl].astype(np.float64) - want).max() <= 2.0 ** -23 * np.abs(want).max()
            assert (out[sl] == want.astype(np.float32)).mean() > 0.99
    # the direction: members R^T V R (what a model trained on R^T y R returns) come back to V, members R V R^T do not
    V = _rows(12, 31).astype(np.float64)
    Rg = R[np.repeat(np.arange(3), np.diff(ptr))].astype(np.float64)
    there = (Rg.transpose(0, 2, 1) @ V @ Rg).astype(np.float32)
    back = mf.stored_frame_host(there, R, ptr).astype(np.float64)
    delta = np.abs(Rg @ Rg.transpose(0, 2, 1) - np.eye(3)).max()
    assert np.abs(back - V).max() <= (4 * 2.0 ** -24 + 6 * delta + 9 * delta ** 2) * 3 * np.abs(V).max()
    wrong = mf.stored_frame_host((Rg @ V @ Rg.transpose(0, 2, 1)).astype(np.float32), R, ptr).astype(np.float64)
    assert np.abs(wrong - V).max() > 0.1 * np.abs(V).max()
    # a NaN row stays NaN and spoils no neighbour
    P = _rows(12, 41)
    clean = mf.stored_frame_host(P, R, ptr)
    P[6, 1, 2] = np.nan
    out = mf.stored_frame_host(P, R, ptr)
    assert np.isnan(out[6]).all()
    keep = np.arange(12) != 6
    assert out[keep].tobytes() == clean[keep].tobytes()


def test_the_exact_fma_of_the_host_form():
    # a * b + c where the two-step form rounds twice and the fused form once
    a, b, c = 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, -1.0
    assert mf._fma(a, b, c) == 2.0 ** -29 + 2.0 ** -60 and a * b + c == 2.0 ** -29
    assert mf._fma(3.0, 0.0, -0.0) == 0.0 and np.isnan(mf._fma(np.nan, 1.0, 1.0)) and mf._fma(np.inf, 1.0, 1.0) == np.inf
    assert mf.member_host(np.arange(9, dtype=np.float32), np.eye(3, dtype=np.float32).reshape(-1)) == list(range(9))

"""The frame mean on the host: the entry point's declaration and binding, its returns that need no launch, the
``--rotations`` flag and ``predict.frames`` without random members (no GPU)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_and_bound_with_ten_parameters():
    from cartnet_amd import lib
    hdr = open(os.path.join(ROOT, "include", "cartnet_hip.h")).read()
    assert "main.py:95-97" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+cartnet_adp_frame_mean\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 10 == len(lib.PROTOTYPES["cartnet_adp_frame_mean"][1])
    assert lib.ABI_VERSION == 16 == lib.load().cartnet_abi_version()          # no struct changed
    m = re.search(r"\bint\s+cartnet_adp_export\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 12                             # the export's signature is where it was


def test_no_launch_and_refusal_returns():
    from cartnet_amd import lib
    l = lib.load()
    f = l.cartnet_adp_frame_mean
    assert f(None, None, 3, None, 4, 0, None, None, None, None) == 0          # no rows
    assert f(None, None, 3, None, 0, 0, None, None, None, None) == 0          # no crystals
    assert f(None, None, 0, None, 4, 5, None, None, None, None) != 0
    assert b"bad sizes" in l.cartnet_last_error()
    assert f(None, None, 0, None, 4, 0, None, None, None, None) != 0          # K is checked before the early return
    assert b"bad sizes" in l.cartnet_last_error()
    assert f(None, None, 2, None, 1, -1, None, None, None, None) != 0
    assert b"bad sizes" in l.cartnet_last_error()
    assert f(None, None, 2, None, -1, 3, None, None, None, None) != 0
    assert b"bad sizes" in l.cartnet_last_error()
    assert f(None, None, 2, None, 2, 5, None, None, None, None) != 0          # before any launch
    assert b"null pointer" in l.cartnet_last_error()


def test_rotations_flag_parses_and_old_defaults_stay():
    import main as entry
    from cartnet_amd.config import cfg, set_cfg
    p = entry.build_parser()
    d = p.parse_args([])
    assert d.rotations == 1
    assert (d.predict, d.predict_input, d.predict_output, d.predict_cif_dir, d.predict_temperature) == \
        (False, None, "./predictions.pkl", None, None)
    assert (d.inference, d.montecarlo, d.inference_output, d.eval_batch, d.model, d.radius, d.disable_H, d.seed,
            d.montecarlo_rounds, d.batch, d.batch_accumulation, d.dim_in, d.num_layers, d.augment, d.invariant) == \
        (False, False, "./inference.pkl", 1, "CartNet", 5.0, True, 0, 100, 4, 16, 256, 4, False, False)
    try:
        entry.fill_cfg(d)
        assert cfg.rotations == 1 and cfg.eval_batch == 1
        entry.fill_cfg(p.parse_args(["--rotations", "5", "--seed", "3"]))
        assert cfg.rotations == 5 and cfg.seed == 3
        for bad in ("0", "-2"):
            with pytest.raises(ValueError, match="--rotations must be at least 1"):
                entry.fill_cfg(p.parse_args(["--rotations", bad]))
    finally:
        set_cfg()
    assert cfg.rotations == 1
    assert "--eval_batch * K" in " ".join(p.format_help().split())            # the size of a forward is in the help


def test_frames_of_one_frame_are_identities():
    from cartnet_amd.predict import KEYS, ROT_KEYS, SYM_KEYS, frames
    f = frames(3, 1, None, "cpu")                                             # no member is drawn: no generator needed
    assert tuple(f.shape) == (1, 3, 3, 3) and f.dtype == torch.float32
    assert torch.equal(f, torch.eye(3).expand(1, 3, 3, 3))
    with pytest.raises(ValueError):
        frames(3, 0, None, "cpu")
    assert KEYS == ("name", "atoms", "frac", "z", "cell", "temp", "u_cart", "u_cif", "u_eq", "principal", "axes", "stats")
    assert SYM_KEYS == ("asym_labels", "asym_frac", "asym_z", "u_cif_asym", "spread", "symops")
    assert ROT_KEYS == ("rot_spread", "frames", "rot_stats")

"""--eval_batch on the host: the flag, the two new entry points' declarations, the crystal offsets of a batch and the
per-crystal split of what a batched evaluation brings back (no GPU)."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_batch_flag_parses_defaults_to_one_and_reaches_cfg():
    import main as entry
    from cartnet_amd.config import cfg, set_cfg
    p = entry.build_parser()
    assert p.parse_args([]).eval_batch == 1
    assert p.parse_args(["--eval_batch", "16"]).eval_batch == 16
    try:
        entry.fill_cfg(p.parse_args([]))
        assert cfg.eval_batch == 1
        entry.fill_cfg(p.parse_args(["--eval_batch", "64"]))
        assert cfg.eval_batch == 64
        try:
            entry.fill_cfg(p.parse_args(["--eval_batch", "0"]))
        except ValueError:
            pass
        else:
            raise AssertionError("--eval_batch 0 was accepted")
    finally:
        set_cfg()
    assert cfg.eval_batch == 1


def test_entry_points_are_declared_and_bound_and_the_abi_version_stays():
    from cartnet_amd import lib
    hdr = open(os.path.join(ROOT, "include", "cartnet_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n_args in (("cartnet_rotate_rows", 7), ("cartnet_adp_eval", 15)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/cartnet_hip.h"
        assert len(m.group(1).split(",")) == n_args
        assert name in lib.PROTOTYPES and len(lib.PROTOTYPES[name][1]) == n_args
    assert lib.ABI_VERSION == 16 == lib.load().cartnet_abi_version()     # its entry points changed no struct (16: the GEMM plan query)


def _crystal(z, tgt, src):
    from cartnet_amd.data import Data
    z = torch.tensor(z, dtype=torch.int64)
    n, e = len(z), len(tgt)
    return Data(x=z, non_H_mask=z != 1, pos=torch.arange(n * 3, dtype=torch.float32).reshape(n, 3),
                edge_index=torch.tensor([src, tgt], dtype=torch.int64).reshape(2, e),
                cart_dist=torch.ones(e), cart_dir=torch.zeros(e, 3), cell=torch.eye(3).unsqueeze(0) * (n + 1.0),
                y=torch.zeros(int((z != 1).sum()), 3, 3))


def _hand_made_batch():
    from cartnet_amd.data import Batch
    return Batch.from_data_list([_crystal([6, 1, 8], [0, 0, 1, 2, 2], [1, 2, 0, 0, 1]),      # 2 of 3 atoms kept, 5 edges
                                 _crystal([1, 1], [0, 1], [1, 0]),                            # hydrogen only: no target rows
                                 _crystal([7], [], []),                                       # one atom, no edge
                                 _crystal([8, 8, 1, 6], [0, 1, 1, 3], [1, 0, 3, 1])])


def test_row_offsets_of_a_hand_made_batch():
    from cartnet_amd.data import Batch
    from cartnet_amd.metrics import edge_row_ptr, target_row_ptr
    b = _hand_made_batch()
    rp = target_row_ptr(b)
    assert rp.dtype == torch.int64 and rp.tolist() == [0, 2, 2, 3, 6]                         # the second segment is empty
    ep = edge_row_ptr(b)
    assert ep.dtype == torch.int64 and ep.tolist() == [0, 5, 7, 7, 11]
    one = Batch.from_data_list([_crystal([6, 1, 8], [0, 0, 1, 2, 2], [1, 2, 0, 0, 1])])
    assert target_row_ptr(one).tolist() == [0, 2] and edge_row_ptr(one).tolist() == [0, 5]
    allh = Batch.from_data_list([_crystal([1, 1], [0, 1], [1, 0])])
    assert target_row_ptr(allh).tolist() == [0, 0] and edge_row_ptr(allh).tolist() == [0, 2]
    # without a mask every atom is a target row
    del b.non_H_mask
    assert target_row_ptr(b).tolist() == b.ptr.tolist()
    # a shard-collated batch carries [sel | atom offsets | edge offsets | target offsets] (DeviceShard.collate): taken as is
    b = _hand_made_batch()
    b._meta = torch.tensor([3, 1, 4, 1] + [0, 3, 5, 6, 10] + [0, 5, 7, 7, 11] + [0, 2, 2, 3, 6], dtype=torch.int64)
    got = target_row_ptr(b)
    assert got.tolist() == [0, 2, 2, 3, 6] and got.data_ptr() == b._meta[14:].data_ptr()


def test_per_crystal_split_of_a_batch_on_the_host():
    from cartnet_amd import evaluate
    from cartnet_amd.metrics import split_rows, target_row_ptr
    pieces = split_rows(torch.arange(12.).reshape(6, 2), [2, 0, 1, 3])
    assert [tuple(p.shape) for p in pieces] == [(2, 2), (0, 2), (1, 2), (3, 2)]
    assert pieces[3].tolist() == [[6., 7.], [8., 9.], [10., 11.]]
    assert all(p.untyped_storage().nbytes() == p.numel() * 4 for p in pieces)                 # each owns its memory
    b = _hand_made_batch()
    rp = target_row_ptr(b)
    pred = torch.arange(6 * 9, dtype=torch.float32).reshape(6, 3, 3)
    iou = torch.arange(6, dtype=torch.float32)
    out = {"pred": [], "iou": [], "cell": [], "atoms": [], "pos": []}
    evaluate.batch_entries(out, b, rp, {"pred": pred, "iou": iou}, with_pos=True)
    assert all(len(out[k]) == 4 for k in out)                                                 # one entry per crystal
    assert [tuple(p.shape) for p in out["pred"]] == [(2, 3, 3), (0, 3, 3), (1, 3, 3), (3, 3, 3)]
    assert torch.equal(torch.cat(out["pred"]), pred) and torch.equal(torch.cat(out["iou"]), iou)
    assert [a.tolist() for a in out["atoms"]] == [[6, 8], [], [7], [8, 8, 6]] and out["atoms"][0].dtype == torch.int64
    assert [tuple(c.shape) for c in out["cell"]] == [(1, 3, 3)] * 4 and out["cell"][3][0, 0, 0].item() == 5.0
    assert out["pos"][3].tolist() == [[0., 1., 2.], [3., 4., 5.], [9., 10., 11.]]
    out = {"pred": [], "cell": [], "atoms": [], "pos": []}
    evaluate.batch_entries(out, b, rp, {"pred": pred}, with_pos=False)                          # the Monte-Carlo pickles: no pos
    assert out["pos"] == [] and len(out["pred"]) == 4

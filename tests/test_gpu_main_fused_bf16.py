"""main.py --fused_accumulation --gemm_precision 2 --bf16_storage: the reference's micro-batch recipe (batch 4 x accumulation 4
here; scripts/train_cartnet_adp.sh:4 runs 4 x 16) as one pass per optimiser step with the layers' edge-sized tensors kept
as bf16, against the same command line run micro-batch by micro-batch."""
import pytest

pytestmark = pytest.mark.gpu


def test_main_fused_accumulation_with_bf16_storage_follows_the_micro_batch_recipe(tmp_path, monkeypatch):
    """Same loaders, same order, same optimiser steps; per epoch the training and validation MAE within the 5e-2 that
    test_main_jarvis_style_run_with_bf16_storage gives bf16 storage.  The fused run must reach the model as groups of 4
    inside batches of 16 with bf16 storage on."""
    import main as entry
    from cartnet_amd.config import cfg
    monkeypatch.chdir(tmp_path)
    seen = []
    create = entry.create_model

    def create_and_record(*a, **k):
        m = create(*a, **k)
        seen.append((int(m.bn_group_size), bool(m.half_storage), int(m.gemm_precision), int(cfg.bn_group_size),
                     bool(cfg.half_storage), int(cfg.batch), int(cfg.batch_accumulation)))
        return m

    monkeypatch.setattr(entry, "create_model", create_and_record)
    common = ["--synthetic", "40", "--atoms", "10", "30", "--dim_in", "256", "--num_layers", "2", "--epochs", "2",
              "--batch", "4", "--batch_accumulation", "4", "--gemm_precision", "2", "--bf16_storage"]
    a = entry.main(common + ["--name", "micro"])
    b = entry.main(common + ["--name", "fused", "--fused_accumulation"])
    assert seen == [(0, True, 2, 0, True, 4, 4), (4, True, 2, 4, True, 16, 1)]
    assert len(a["history"]) == len(b["history"]) == 2
    for ha, hb in zip(a["history"], b["history"]):
        print(f"train_mae {ha['train_mae']:.6g} / {hb['train_mae']:.6g}   val_mae {ha['val_mae']:.6g} / {hb['val_mae']:.6g}")
        for k in ("train_mae", "val_mae"):
            assert ha[k] == ha[k] and hb[k] == hb[k] and abs(ha[k]) < float("inf") and abs(hb[k]) < float("inf")
            assert abs(ha[k] - hb[k]) < 5e-2 * abs(ha[k]), (k, ha[k], hb[k])

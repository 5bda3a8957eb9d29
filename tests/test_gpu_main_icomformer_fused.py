"""main.py --model icomformer --fused_accumulation: the reference's iComformer recipe (scripts/train_icomformer_adp.sh:3,
batch x batch_accumulation micro-batches per optimiser step) as one grouped pass per step against the same recipe run
micro-batch by micro-batch (same loaders, same order)."""
import pytest

pytestmark = pytest.mark.gpu


def test_main_fused_accumulation_reproduces_the_icomformer_micro_batch_recipe(tmp_path, monkeypatch):
    import main as entry
    from cartnet_amd.config import cfg
    monkeypatch.chdir(tmp_path)
    common = ["--model", "icomformer", "--synthetic", "40", "--atoms", "10", "30", "--dim_in", "32", "--epochs", "2",
              "--batch", "4", "--batch_accumulation", "4", "--lr", "1e-3"]
    a = entry.main(common + ["--name", "micro"])
    assert cfg.bn_group_size == 0 and cfg.batch == 4 and cfg.batch_accumulation == 4
    b = entry.main(common + ["--name", "fused", "--fused_accumulation"])
    # the flag reached the model: whole optimiser steps from the loader, BatchNorm and loss per micro-batch of 4
    assert cfg.bn_group_size == 4 and cfg.batch == 16 and cfg.batch_accumulation == 1
    assert len(a["history"]) == len(b["history"]) == 2
    for ha, hb in zip(a["history"], b["history"]):
        print(f"train {ha['train_mae']:.6g} / {hb['train_mae']:.6g}  val {ha['val_mae']:.6g} / {hb['val_mae']:.6g}")
        assert abs(ha["train_mae"] - hb["train_mae"]) < 2e-3 * abs(ha["train_mae"])
        assert abs(ha["val_mae"] - hb["val_mae"]) < 2e-2 * abs(ha["val_mae"])

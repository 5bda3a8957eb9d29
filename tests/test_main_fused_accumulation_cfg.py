"""main.fill_cfg: --fused_accumulation turns batch x batch_accumulation micro-batches into one batch per optimiser step
with cfg.bn_group_size = the micro-batch size, for the models whose BatchNorm kernels take groups (CartNet, iComformer);
eComformer keeps the literal recipe.  No GPU needed."""
import pytest


def _cfg(model, fused=True):
    import main as entry
    from cartnet_amd.config import cfg
    argv = ["--model", model, "--batch", "4", "--batch_accumulation", "16"] + (["--fused_accumulation"] if fused else [])
    entry.fill_cfg(entry.build_parser().parse_args(argv))
    return cfg.batch, cfg.batch_accumulation, cfg.bn_group_size


@pytest.mark.parametrize("model", ["CartNet", "icomformer"])
def test_fused_accumulation_rewrites_the_recipe(model):
    assert _cfg(model) == (64, 1, 4)
    assert _cfg(model, fused=False) == (4, 16, 0)


def test_fused_accumulation_leaves_ecomformer_untouched():
    assert _cfg("ecomformer") == (4, 16, 0)


def test_fused_accumulation_needs_an_accumulation_count():
    import main as entry
    from cartnet_amd.config import cfg
    entry.fill_cfg(entry.build_parser().parse_args(["--model", "icomformer", "--batch", "8", "--batch_accumulation", "1",
                                                    "--fused_accumulation"]))
    assert (cfg.batch, cfg.batch_accumulation, cfg.bn_group_size) == (8, 1, 0)


def test_icomformer_module_carries_the_group_size():
    """the attribute master.create_model forwards cfg.bn_group_size into; the Python-sequenced path refuses groups before it
    touches the device"""
    from cartnet_amd.comformer import iComformer
    m = iComformer(32)
    assert m.bn_group_size == 0
    m.bn_group_size, m.native_sequence = 2, False
    with pytest.raises(ValueError, match="native_sequence"):
        m(object())

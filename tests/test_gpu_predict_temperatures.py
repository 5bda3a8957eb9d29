"""``predict_adps(temperatures=...)``: the replica batch against the collation kernel of a shard that stores each temperature,
bit for bit; one temperature equal to the stored one against the pass as it was; three temperatures against three plain
passes; the series keys against the fp64 restatement; and the composition with rotations, the rigid-bond test and riding
hydrogens.  Standardisation of the temperature is ON (the default): ``(T - mean) / std`` is part of what is compared."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from temp_series_utils import line_bounds, line_reference

pytestmark = pytest.mark.gpu

BATCH_TOL = 2 * 1e-5     # tests/test_gpu_predict.py:12: a crystal's prediction across batch compositions, norm-wise
EVAL_BATCH, SEED = 2, 11
STORED = 150.0
TEMPS = (100.0, 180.5, 300.0)
EPS24 = 2.0 ** -24


@pytest.fixture(scope="module")
def setup():
    """cfg, a fresh tiny model in eval mode and, per stored temperature, the same six unlabeled synthetic crystals of 10-30
    atoms as a resident shard with the recipe applied; the pass under test and the plain passes it is compared with, each
    run once: (entry, model, shards, (mean, std), result, plain passes)."""
    import main as entry
    from cartnet_amd.config import set_cfg
    from cartnet_amd.master import create_model
    from cartnet_amd.predict import predict_adps
    from cartnet_amd.shard import DeviceShard
    from cartnet_amd.synthetic import TEMP_MEAN, TEMP_STD, make_geometry
    entry.fill_cfg(entry.build_parser().parse_args(["--dim_in", "32", "--num_layers", "2"]))
    torch.manual_seed(0)
    model = create_model().eval()
    shards = {}
    for kelvin in (STORED,) + TEMPS:
        crystals = [make_geometry(700 + g, None, (10, 30)) for g in range(6)]
        for d in crystals:
            del d.y
            d.temperature = torch.tensor([kelvin], dtype=torch.float32)
        (shards[kelvin],), norm = entry.shard_recipe([DeviceShard.from_data_list(crystals)])
    assert norm == (TEMP_MEAN, TEMP_STD)
    res = predict_adps(model, _loader(shards[STORED], norm), "cuda:0", temperatures=TEMPS)
    plain = {k: predict_adps(model, _loader(shards[k], norm), "cuda:0") for k in (STORED,) + TEMPS}
    yield entry, model, shards, norm, res, plain
    set_cfg()


def _loader(shard, norm, n=EVAL_BATCH):
    from cartnet_amd.shard import ShardLoader
    return ShardLoader(shard, n, temp_mean=norm[0], temp_std=norm[1])


def _same(a, b, but=("name",)):
    assert list(a) == list(b)
    for k in a:
        if k in but:
            continue
        assert len(a[k]) == len(b[k]), k
        for x, y in zip(a[k], b[k]):
            if torch.is_tensor(x):
                assert x.dtype == y.dtype and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), k
            else:
                assert x == y or (x != x and y != y), k


def test_the_replica_batch_equals_the_collation_of_a_shard_that_stores_the_temperature(setup):
    from cartnet_amd.predict import replicate_temperatures, standardised
    _, _, shards, norm, _, _ = setup
    T = len(TEMPS)
    temps = standardised(TEMPS, *norm, "cuda:0")
    assert temps.dtype == torch.float32 and tuple(temps.shape) == (T,)
    for sel in ([4, 1], [2], [5, 0, 3]):
        B = len(sel)
        batch = shards[STORED].collate(sel, None, *norm)
        before = batch.clone()
        rep = replicate_temperatures(batch, temps)
        N, E = int(batch.x.shape[0]), int(batch.edge_index.shape[1])
        assert rep.num_graphs == T * B and int(rep.x.shape[0]) == T * N and int(rep.edge_index.shape[1]) == T * E
        for t, kelvin in enumerate(TEMPS):
            col = shards[kelvin].collate(sel, None, *norm)
            atoms, edges = slice(t * N, (t + 1) * N), slice(t * E, (t + 1) * E)
            got = {"temperature": rep.temperature[t * B:(t + 1) * B], "x": rep.x[atoms],
                   "ptr": rep.ptr[t * B:(t + 1) * B + 1] - t * N, "batch": rep.batch[atoms] - t * B,
                   "edge_index": rep.edge_index[:, edges] - t * N, "cart_dist": rep.cart_dist[edges],
                   "cart_dir": rep.cart_dir[edges], "pos": rep.pos[atoms]}
            for name, a in got.items():
                b = getattr(col, name)
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (name, kelvin)
                if a.is_floating_point():
                    assert a.contiguous().cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (name, kelvin)
        for name in before.keys():
            v = getattr(before, name)
            if torch.is_tensor(v):
                assert torch.equal(v, getattr(batch, name)), name            # the input batch is as it was
        assert batch.x.dtype == torch.int64


def test_one_temperature_equal_to_the_stored_one_is_the_pass_as_it_was(setup):
    from cartnet_amd.predict import KEYS, predict_adps
    _, model, shards, norm, _, plain = setup
    one = predict_adps(model, _loader(shards[STORED], norm), "cuda:0", temperatures=[STORED])
    assert tuple(one) == KEYS == tuple(plain[STORED]) and "series" not in one
    _same(plain[STORED], one)
    assert one["name"] == [f"{n}_150K" for n in plain[STORED]["name"]]
    assert one["temp"] == [150.0] * 6 == plain[STORED]["temp"]


def _export_bounds(u_cart):
    """Per crystal, for two predictions whose ``u_cart`` differ by at most ``BATCH_TOL max|u_cart|`` per element: a
    component of ``u_cif`` is ``a^T U b`` for two unit reciprocal axes and a principal value moves by at most ``||dU||_2``
    (Weyl), both <= ``||dU||_F`` <= 3 max|dU|; ``u_eq`` is the mean of three diagonal elements, so 1 max|dU|.  Each export
    adds its own fp32 rounding, 8 * 2^-24 max|u_cart| (the round-trip bound of tests/test_gpu_adp_export.py)."""
    scale = float(u_cart.abs().max())
    own = 2 * 8 * EPS24 * scale
    return 3 * BATCH_TOL * scale + own, BATCH_TOL * scale + own


def test_three_temperatures_against_three_plain_passes(setup):
    from cartnet_amd.predict import KEYS
    _, _, _, _, res, plain = setup
    T = len(TEMPS)
    assert tuple(res) == KEYS + ("series",)
    assert all(len(res[k]) == 6 * T for k in KEYS)
    for g in range(6):
        for t, kelvin in enumerate(TEMPS):
            k, ref = g * T + t, plain[kelvin]
            assert res["name"][k] == f"{ref['name'][g]}_{kelvin:g}K" and res["temp"][k] == kelvin
            assert res["name"][k].endswith(("_100K", "_180.5K", "_300K")[t])
            for key in ("atoms", "frac", "z", "cell"):
                assert torch.equal(res[key][k], ref[key][g]), key
            err = rel_err(res["u_cart"][k], ref["u_cart"][g])
            wide, narrow = _export_bounds(ref["u_cart"][g])
            errs = {key: float((res[key][k].double() - ref[key][g].double()).abs().max())
                    for key in ("u_cif", "u_eq", "principal")}
            print(f"crystal {g} at {kelvin:g} K: u_cart against the plain pass {err:.3e} (bound {BATCH_TOL:.1e}); u_cif "
                  f"{errs['u_cif']:.3e}, principal {errs['principal']:.3e} (bound {wide:.3e}); u_eq {errs['u_eq']:.3e} "
                  f"(bound {narrow:.3e})")
            assert err <= BATCH_TOL
            assert errs["u_cif"] <= wide and errs["principal"] <= wide and errs["u_eq"] <= narrow
            assert res["stats"][k].dtype == torch.float64 and tuple(res["axes"][k].shape) == tuple(ref["axes"][g].shape)


def test_the_temperature_is_read(setup):
    _, _, _, _, res, _ = setup
    T = len(TEMPS)
    for g in range(6):
        diff = rel_err(res["u_cart"][g * T + 0], res["u_cart"][g * T + 2])
        print(f"crystal {g}: u_cart at 100 K against 300 K differs by {diff:.3e} norm-wise (BATCH_TOL {BATCH_TOL:.1e})")
        assert diff > BATCH_TOL


def test_the_series_keys_restate_the_entries(setup):
    from cartnet_amd.predict import SERIES_KEYS
    _, _, _, _, res, plain = setup
    T, series = len(TEMPS), res["series"]
    assert tuple(series) == ("name", "temps") + SERIES_KEYS and all(len(v) == 6 for v in series.values())
    assert series["name"] == plain[STORED]["name"]
    for g in range(6):
        assert series["temps"][g].dtype == torch.float32 and series["temps"][g].tolist() == list(TEMPS)
        u_cif = np.stack([res["u_cif"][g * T + t].numpy() for t in range(T)])
        u_eq = np.stack([res["u_eq"][g * T + t].numpy() for t in range(T)])
        n = u_cif.shape[1]
        slope, intercept, resid, drops = line_reference(u_cif, u_eq, TEMPS)
        bs, bi, br = line_bounds(u_cif, u_eq, TEMPS, slope, intercept, resid)
        assert tuple(series["t_slope"][g].shape) == (n, 6) == tuple(series["t_intercept"][g].shape)
        assert series["t_drops"][g].dtype == torch.int32 and series["t_stats"][g].dtype == torch.float64
        got_s = np.concatenate([series["t_slope"][g].numpy(), series["t_ueq_slope"][g].numpy()[:, None]], axis=1)
        got_i = np.concatenate([series["t_intercept"][g].numpy(), series["t_ueq_intercept"][g].numpy()[:, None]], axis=1)
        errs = (np.abs(got_s.astype(np.float64) - slope).max(), np.abs(got_i.astype(np.float64) - intercept).max(),
                np.abs(series["t_resid"][g].numpy().astype(np.float64) - resid).max())
        print(f"crystal {g}: slope {errs[0]:.3e} (bound {bs:.3e}), intercept {errs[1]:.3e} (bound {bi:.3e}), resid "
              f"{errs[2]:.3e} (bound {br:.3e}); U_eq slope mean {slope[:, 6].mean():.3e} A^2/K")
        assert errs[0] <= bs and errs[1] <= bi and errs[2] <= br
        assert (series["t_drops"][g].numpy() == drops).all()
        st, us = series["t_stats"][g], series["t_ueq_slope"][g]
        assert tuple(st.shape) == (4,)
        assert st[0].item() == pytest.approx(us.double().sum().item(), rel=1e-12)
        assert st[1].item() == float((~(us > 0)).sum()) and st[2].item() == float((series["t_drops"][g] > 0).sum())
        assert st[3].item() == series["t_resid"][g].double().max().item()


def test_rotations_share_their_frames_among_the_temperatures(setup):
    from cartnet_amd.predict import KEYS, ROT_KEYS, predict_adps
    _, model, shards, norm, _, _ = setup
    res = predict_adps(model, _loader(shards[STORED], norm), "cuda:0", rotations=2, seed=SEED, temperatures=(100.0, 300.0))
    assert tuple(res) == KEYS + ROT_KEYS + ("series",) and len(res["name"]) == 12
    for g in range(6):
        a, b = 2 * g, 2 * g + 1
        assert tuple(res["frames"][a].shape) == (2, 3, 3) and torch.equal(res["frames"][a][0], torch.eye(3))
        assert torch.equal(res["frames"][a], res["frames"][b])
        n = int(res["u_cart"][a].shape[0])
        assert tuple(res["rot_spread"][a].shape) == (n,) == tuple(res["rot_spread"][b].shape)
        assert not torch.equal(res["rot_spread"][a], res["rot_spread"][b])    # each temperature has its own members
        assert res["rot_stats"][a][1].item() == res["rot_spread"][a].double().max().item()
    assert not torch.equal(res["frames"][0][1], res["frames"][2][1])          # one draw per crystal
    only = predict_adps(model, _loader(shards[STORED], norm), "cuda:0", rotations=2, seed=SEED)
    one = predict_adps(model, _loader(shards[STORED], norm), "cuda:0", rotations=2, seed=SEED, temperatures=[STORED])
    assert tuple(one) == KEYS + ROT_KEYS
    _same(only, one)                                                          # the same frames, the same bits
    assert all(torch.equal(res["frames"][2 * g], only["frames"][g]) for g in range(6))


def test_rigid_bond_and_riding_hydrogens_per_entry(setup):
    from cartnet_amd.predict import BOND_KEYS, H_KEYS, KEYS, predict_adps
    _, model, shards, norm, _, _ = setup
    res = predict_adps(model, _loader(shards[STORED], norm), "cuda:0", rigid_bond=(0.4, 1e-3), riding_h=(0.4, 1.2, 1.5),
                       temperatures=(100.0, 300.0))
    assert tuple(res) == KEYS + BOND_KEYS + H_KEYS + ("series",) and all(len(res[k]) == 12 for k in BOND_KEYS + H_KEYS)
    riding = 0
    for k in range(12):
        z, parent, mult = res["z"][k], res["h_parent"][k], res["h_mult"][k]
        n = int(res["u_cart"][k].shape[0])
        assert tuple(res["bond_count"][k].shape) == (n,) and tuple(res["u_iso"][k].shape) == tuple(z.shape)
        row = torch.cumsum((z != 1).to(torch.int64), 0) - 1                   # an atom's row among the non-hydrogen atoms
        for i in torch.nonzero((z == 1) & (parent >= 0)).flatten().tolist():
            want = mult[i].double() * res["u_eq"][k][row[parent[i]]].double()
            assert abs(res["u_iso"][k][i].item() - want.item()) <= EPS24 * abs(want.item())
            riding += 1
        heavy = z != 1
        assert torch.equal(res["u_iso"][k][heavy], res["u_eq"][k])            # a non-hydrogen atom's own U_eq
    assert riding > 0
    for g in range(6):                                                        # the graph is the crystal's, not the temperature's
        for key in ("bond_count", "h_parent", "h_count", "h_mult"):
            assert torch.equal(res[key][2 * g], res[key][2 * g + 1]), key
        assert not torch.equal(res["u_iso"][2 * g][res["z"][2 * g] != 1], res["u_iso"][2 * g + 1][res["z"][2 * g] != 1])


@pytest.mark.parametrize("bad", [[], [200.0, 100.0], [100.0, 100.0], [-5.0], [float("nan")]])
def test_errors(setup, bad):
    from cartnet_amd.predict import predict_adps
    _, model, shards, norm, _, _ = setup
    with pytest.raises(ValueError, match="temperatures"):
        predict_adps(model, _loader(shards[STORED], norm), "cuda:0", temperatures=bad)

"""``predict_adps(model_frame=...)``: iComformer reads every crystal in the frame of its reduced cell, and the result is in
the frame the crystal is stored in.

* parity: ``u_cart`` is ``R P R^T`` (tests/model_frame_utils.py's host form of the kernel, so bit for bit) of what
  ``evaluate.inference`` predicts for the same crystals in the reduced frame;
* oracle: ``u_cart`` against ``R oracle(reduced inputs) R^T`` in fp64, at the budget of tests/test_gpu_icomformer.py;
* two stored descriptions of the same crystals (rotated by Q, another integer basis): ``Q^T U Q`` against ``U'``, held to
  what the fp64 oracle gives for the same pair plus twice that budget.  The oracle's own figure is of the order of the
  prediction, not of rounding: the recipe rotates ``cart_dir`` by R and the cell by R^T (``data.optimize_cell``), so the
  reduced-frame prediction is (nearly) the same P for both descriptions while ``R`` and ``R Q`` take it back to different
  tensors.  ``u_eq`` and ``principal``, which no rotation changes, agree closely; they are also held to their own oracle
  figures;
* everything downstream is stored-frame: the keys that do not depend on U are those of a CartNet pass over the same shard,
  bit for bit; the U-dependent ones are the analyses' kernels on the returned ``u_cart`` and the stored batch, bit for
  bit, and the numpy rules of ``cartnet_amd/bonds.py`` on it and the stored edges (riding hydrogens, molecules, TLS fit,
  hydrogen tensors, bond table, angle and torsion tables; the rigid-bond and rigid-body figures have no numpy rule there);
* a second description that changes only the integer basis (Q = I) changes nothing beyond rounding;
* the temperature series runs on the view."""
import pickle

import numpy as np
import pytest
import torch

import angle_table_utils as at
import bond_table_utils as bu
import icomformer_utils as iu
import model_frame_utils as mf
import molecule_utils as mu
import predict_utils as pu
import tls_utils as tu
from conftest import rel_err
from test_gpu_model import PRED_TOL                    # the budget tests/test_gpu_icomformer.py uses

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EVAL_BATCH = 3                                         # batches of three crystals and of one
BATCH_TOL = 2 * 1e-5                                   # a crystal's prediction across batch compositions
ANALYSES = dict(rigid_bond=(0.4, 1e-3), riding_h=(0.4, 1.2, 1.5), rigid_molecule=(0.4, 1e-3), tls_fit=True,
                aniso_h=(0.005, 0.020), bond_table=0.4, angle_table=0.4)


def _loader(shard):
    from cartnet_amd.shard import ShardLoader
    return ShardLoader(shard, EVAL_BATCH, temp_mean=mf.TEMP_MEAN, temp_std=mf.TEMP_STD)


@pytest.fixture(scope="module")
def setup():
    """The model, the four crystals stored (labeled, unlabeled, and unlabeled in their second description), each with its
    reduced frame, and the plain pass over the unlabeled shard."""
    from cartnet_amd.comformer import iComformer
    from cartnet_amd.predict import predict_adps
    from cartnet_amd.shard import DeviceShard
    dim, sd = mf.model_and_weights()
    model = iComformer(dim)
    model.load_state_dict(sd, strict=True)
    model.validate_graph = True
    model = model.to(DEV).eval()
    s = {"labeled": DeviceShard.from_data_list(mf.crystals(True), DEV),
         "unlabeled": DeviceShard.from_data_list(mf.crystals(False), DEV),
         "restored": DeviceShard.from_data_list(mf.crystals(False, restored=True), DEV),
         "rebased": DeviceShard.from_data_list(mf.crystals(False, restored=True, rotate=False), DEV)}
    r = {k: v.with_optimized_cell() for k, v in s.items()}
    res = predict_adps(model, _loader(s["unlabeled"]), DEV, model_frame=r["unlabeled"])
    return model, sd, s, r, res


def _oracle(sd, reduced):
    """Per crystal fp64 ``(U = R P R^T, P)``: the oracle on the reduced shard's own batches (their fp32 values in fp64)."""
    from oracle import icomformer_ref as orc
    sd64 = iu.to64(sd)
    out = []
    for b in _loader(reduced):
        R = reduced.t["rotation"][torch.from_numpy(b._sel).to(DEV)].cpu().double().view(-1, 3, 3)
        rows = (b._meta[3 * b.num_graphs + 2:].cpu()).diff().tolist()
        b = b.to("cpu")
        P = orc.icomformer_forward(sd64, iu.batch64(b)).detach()
        for Rg, Pg in zip(R, torch.split(P, rows)):
            out.append(((Rg @ Pg @ Rg.T).numpy(), Pg.numpy()))
    return out


def test_the_result_has_the_two_new_keys_and_the_stored_geometry(setup):
    from cartnet_amd.predict import KEYS, MF_KEYS
    model, sd, s, r, res = setup
    assert tuple(res) == KEYS + MF_KEYS
    items = mf.crystals(False)
    rot, red = r["unlabeled"].t["rotation"].cpu().view(-1, 3, 3), r["unlabeled"].t["cell"].cpu().view(-1, 3, 3)
    for g, d in enumerate(items):
        assert torch.equal(res["cell"][g], d.cell[0]) and torch.equal(res["z"][g], d.x)       # the stored cell
        assert torch.allclose(res["frac"][g] @ d.cell[0], d.pos, atol=1e-4)
        assert mf.bits(res["cell_rotation"][g]) == mf.bits(rot[g]) and mf.bits(res["cell_reduced"][g]) == mf.bits(red[g])
        assert res["temp"][g] == pytest.approx(float(d.temperature))
        n = int((d.x != 1).sum())
        assert tuple(res["u_cart"][g].shape) == (n, 3, 3) and bool(torch.isfinite(res["u_cart"][g]).all())
    # without the keyword the pass is the one it was: CartNet's keys, and iComformer in the stored frame predicts otherwise
    from cartnet_amd.predict import predict_adps
    plain = predict_adps(model, _loader(s["unlabeled"]), DEV)
    assert tuple(plain) == KEYS
    assert rel_err(torch.cat(plain["u_cart"][1:3]), torch.cat(res["u_cart"][1:3])) > 100 * PRED_TOL
    with pytest.raises(ValueError, match="model_frame serves one frame only"):
        predict_adps(model, _loader(s["unlabeled"]), DEV, rotations=2, model_frame=r["unlabeled"])
    with pytest.raises(ValueError, match="must be the with_optimized_cell"):
        predict_adps(model, _loader(s["unlabeled"]), DEV, model_frame=s["unlabeled"])


def test_parity_with_inference_in_the_reduced_frame(setup, tmp_path):
    """The inputs of the two forwards are bit-equal (tests/test_gpu_model_frame_kernels.py) and the launches are the same,
    so ``u_cart`` is expected to be the host form's ``R P R^T`` of ``--inference``'s predictions bit for bit."""
    from cartnet_amd import evaluate
    from cartnet_amd.predict import predict_adps
    model, sd, s, r, res = setup
    path = str(tmp_path / "inference.pkl")
    evaluate.inference(model, _loader(r["labeled"]), DEV, path)
    with open(path, "rb") as f:
        reduced = pickle.load(f)["pred"]
    rot = r["labeled"].t["rotation"].cpu().view(-1, 3, 3).numpy()
    labeled = predict_adps(model, _loader(s["labeled"]), DEV, model_frame=r["labeled"])       # its y is ignored
    for g in range(4):
        P = reduced[g].numpy()
        want = mf.stored_frame_host(P, rot[g:g + 1], [0, len(P)])
        for name, got in (("unlabeled", res), ("labeled", labeled)):
            err = rel_err(got["u_cart"][g], torch.from_numpy(want))
            print(f"crystal {g}, {name}: u_cart against R P R^T of the reduced-frame inference: rel_err {err:.3e}")
            assert mf.bits(got["u_cart"][g]) == want.tobytes(), (g, name)
        plain = rot[g].astype(np.float64) @ P.astype(np.float64) @ rot[g].astype(np.float64).T   # numpy fp64, rounded once
        assert np.abs(res["u_cart"][g].numpy().astype(np.float64) - plain).max() <= 2.0 ** -23 * np.abs(plain).max()


def test_u_cart_against_the_fp64_oracle(setup):
    model, sd, s, r, res = setup
    ref = _oracle(sd, r["unlabeled"])
    want = torch.from_numpy(np.concatenate([u for u, _ in ref]))
    err = rel_err(torch.cat(res["u_cart"]), want)
    print(f"u_cart against R oracle(reduced inputs) R^T: rel_err {err:.3e} (budget {PRED_TOL:.1e})")
    assert err < PRED_TOL
    for g in range(4):
        assert rel_err(res["u_cart"][g], torch.from_numpy(ref[g][0])) < PRED_TOL * float(want.abs().max()) / float(
            np.abs(ref[g][0]).max()), g                                       # every crystal, at the batch's scale


def _sym_eig(u):
    return np.linalg.eigvalsh(0.5 * (u + u.transpose(0, 2, 1)))


def test_two_stored_descriptions_of_the_same_crystals(setup):
    """``Q^T U Q`` of the first description against ``U'`` of the second.  The bound: the same difference between the two
    fp64 oracle results (what the fp32 inputs and the recipe's convention cause) plus twice the parity budget, each side
    being within the budget of its oracle; for ``u_eq`` and ``principal`` also their own oracle figure plus twice the
    budget -- ``u_eq`` is a third of a trace, an eigenvalue moves by at most the spectral norm <= 3 max|.| of a change --
    plus the export's own fp32 rounding (a few units of 2^-23)."""
    from cartnet_amd.predict import predict_adps
    model, sd, s, r, res = setup
    other = predict_adps(model, _loader(s["restored"]), DEV, model_frame=r["restored"])
    oa, ob = _oracle(sd, r["unlabeled"]), _oracle(sd, r["restored"])
    Q = mf.restore_rotations()
    scale = max(float(np.abs(u).max()) for u, _ in ob)
    back = lambda u, q: q.T @ np.asarray(u, dtype=np.float64) @ q
    fig = {"oracle": {}, "gpu": {}}
    for name, A, Bv in (("oracle", [u for u, _ in oa], [u for u, _ in ob]),
                        ("gpu", [t.numpy() for t in res["u_cart"]], [t.numpy() for t in other["u_cart"]])):
        A, Bv = [np.asarray(a, dtype=np.float64) for a in A], [np.asarray(b, dtype=np.float64) for b in Bv]
        fig[name]["u"] = max(float(np.abs(back(a, q) - b).max()) for a, b, q in zip(A, Bv, Q))
        fig[name]["u_eq"] = max(float(np.abs(np.trace(a, axis1=1, axis2=2) - np.trace(b, axis1=1, axis2=2)).max()) / 3
                                for a, b in zip(A, Bv))
        fig[name]["principal"] = max(float(np.abs(_sym_eig(a) - _sym_eig(b)).max()) for a, b in zip(A, Bv))
    fig["gpu"]["u_eq"] = max(float((a.double() - b.double()).abs().max()) for a, b in zip(res["u_eq"], other["u_eq"]))
    fig["gpu"]["principal"] = max(float((a.double() - b.double()).abs().max())
                                  for a, b in zip(res["principal"], other["principal"]))
    p_diff = max(float(np.abs(pa - pb).max()) for (_, pa), (_, pb) in zip(oa, ob))
    budget, export = 2 * PRED_TOL * scale, 8 * 2.0 ** -23 * scale
    print(f"scale {scale:.4f}; oracle: {fig['oracle']}; gpu: {fig['gpu']}; reduced-frame P of the two descriptions differ by "
          f"{p_diff:.3e}; 2 x budget {budget:.3e}")
    bound = fig["oracle"]["u"] + budget
    assert fig["gpu"]["u"] <= bound
    assert fig["gpu"]["u_eq"] <= bound and fig["gpu"]["principal"] <= bound               # the same bound
    assert fig["gpu"]["u_eq"] <= fig["oracle"]["u_eq"] + budget + export                   # and their own
    assert fig["gpu"]["principal"] <= fig["oracle"]["principal"] + 3 * budget + export
    # both descriptions have the same reduced cell, and each side is within the budget of its own oracle
    for g in range(4):
        assert torch.allclose(res["cell_reduced"][g], other["cell_reduced"][g], rtol=0, atol=1e-5 * 10.0)
    assert rel_err(torch.cat(other["u_cart"]), torch.from_numpy(np.concatenate([u for u, _ in ob]))) < PRED_TOL


def test_another_basis_in_the_same_cartesian_frame_changes_nothing(setup):
    """The case a user meets: the same structure in two settings that differ only in the integer basis of the lattice (Q =
    I).  Both have the same reduced cell and the same R up to the fp32 rounding of the candidates, so ``u_cart``, ``u_eq``
    and ``principal`` agree to rounding: the bound is again the fp64 oracle's own difference for the pair (about 1e-8 of
    the scale) plus twice the parity budget, for an eigenvalue three times (its change is at most the spectral norm <= 3
    max|.| of the tensor's), plus the export's fp32 rounding for ``u_eq`` and ``principal``."""
    from cartnet_amd.predict import predict_adps
    model, sd, s, r, res = setup
    other = predict_adps(model, _loader(s["rebased"]), DEV, model_frame=r["rebased"])
    oa, ob = _oracle(sd, r["unlabeled"]), _oracle(sd, r["rebased"])
    scale = max(float(np.abs(u).max()) for u, _ in ob)
    budget, export = 2 * PRED_TOL * scale, 8 * 2.0 ** -23 * scale
    o_u = max(float(np.abs(a - b).max()) for (a, _), (b, _) in zip(oa, ob))
    o_eq = max(float(np.abs(np.trace(a, axis1=1, axis2=2) - np.trace(b, axis1=1, axis2=2)).max()) / 3
               for (a, _), (b, _) in zip(oa, ob))
    o_pr = max(float(np.abs(_sym_eig(a) - _sym_eig(b)).max()) for (a, _), (b, _) in zip(oa, ob))
    g_u = max(float((a.double() - b.double()).abs().max()) for a, b in zip(res["u_cart"], other["u_cart"]))
    g_eq = max(float((a.double() - b.double()).abs().max()) for a, b in zip(res["u_eq"], other["u_eq"]))
    g_pr = max(float((a.double() - b.double()).abs().max()) for a, b in zip(res["principal"], other["principal"]))
    print(f"scale {scale:.4f}; oracle: u {o_u:.3e}, u_eq {o_eq:.3e}, principal {o_pr:.3e}; gpu: u {g_u:.3e}, u_eq {g_eq:.3e}, "
          f"principal {g_pr:.3e}; 2 x budget {budget:.3e}")
    assert o_u <= 1e-6 * scale                                                # the oracle itself: rounding, not the recipe
    assert g_u <= o_u + budget
    assert g_eq <= o_eq + budget + export and g_pr <= o_pr + 3 * budget + export
    for g in range(4):
        assert not torch.equal(res["cell"][g], other["cell"][g])              # another stored cell ...
        assert torch.allclose(res["cell_reduced"][g], other["cell_reduced"][g], rtol=0, atol=1e-4)      # ... the same reduced
        assert torch.allclose(res["cell_rotation"][g], other["cell_rotation"][g], rtol=0, atol=1e-5)


INDEPENDENT = ("z", "atoms", "frac", "cell", "bond_count", "h_parent", "h_count", "h_mult", "mol", "mol_size", "mol_status",
               "mol_pos", "bonds_a", "bonds_b", "bonds_dir", "bonds_length", "angles_a", "angles_b", "angles_c",
               "angles_value", "torsions_a", "torsions_b", "torsions_c", "torsions_d", "torsions_value")


def _tls_params(res, k):
    pick = [0, 4, 8, 5, 2, 1]                                                 # 11 22 33 23 13 12 of a row-major 3x3
    n = int(res["tls_T"][k].shape[0])
    return np.concatenate([res["tls_T"][k].reshape(n, 9)[:, pick].numpy(), res["tls_L"][k].reshape(n, 9)[:, pick].numpy(),
                           res["tls_S"][k].reshape(n, 9).numpy(), res["tls_origin"][k].numpy()], axis=1)


TLS_BLOCKS = {"T": slice(0, 6), "L": slice(6, 12), "S": slice(12, 21), "origin": slice(21, 24)}


def _tls_against_the_rule(res, g, u, params, fit, mo, row) -> dict:
    """The TLS keys of crystal ``g`` against ``bonds.tls_fit_host`` (``fit``) on the host's own molecules ``mo``, as
    tests/test_gpu_tls_fit.py compares a kernel's rows: ranks exact, NaN where nothing is fitted, ``tls_u`` and
    ``tls_resid`` within 2^-22 max|U| of the molecule, ``tls_r`` within 1e-5 relative, every parameter block and both
    triples of principal values within 2^-22 of the block's largest entry for a fit of full rank whose normal matrix is
    well conditioned.  Returns the largest deviations as fractions of their bounds."""
    got = {"u_tls": res["tls_u"][g].numpy(), "resid": res["tls_resid"][g].numpy(), "rfac": res["tls_r"][g].numpy(),
           "rank": res["tls_rank"][g].numpy(), "params": params,
           "eig": np.concatenate([res["tls_T_principal"][g].numpy(), res["tls_L_principal"][g].numpy()], axis=1)}
    assert np.array_equal(got["rank"], fit["rank"]) and got["rank"].dtype == np.int32
    neutral = fit["rank"] == 0
    for k in ("u_tls", "params", "eig"):
        assert np.isnan(got[k][neutral]).all() and not np.isnan(got[k][~neutral]).any(), (g, k)
    assert (got["resid"][neutral] == 0).all() and (got["rfac"][neutral] == 0).all()
    U = u.astype(np.float64)
    worst = {"tls_u": 0.0, "tls_resid": 0.0, "tls_r": 0.0, "tls_params": 0.0, "tls_principal": 0.0}
    for root, f in fit["molecules"].items():
        rows = row[mo["label"] == root]
        bound = tu.EPS22 * np.abs(U[rows]).max()
        e_u = np.abs(got["u_tls"][rows].astype(np.float64) - fit["u_tls"][rows]).max()
        e_r = np.abs(got["resid"][rows].astype(np.float64) - fit["resid"][rows]).max()
        e_f = np.abs(got["rfac"][rows].astype(np.float64) - fit["rfac"][rows]).max() / fit["rfac"][rows[0]]
        worst.update(tls_u=max(worst["tls_u"], e_u / bound), tls_resid=max(worst["tls_resid"], e_r / bound),
                     tls_r=max(worst["tls_r"], e_f / 1e-5))
        assert e_u <= bound and e_r <= bound and e_f <= 1e-5, (g, root, e_u, e_r, e_f, bound)
        for k in ("params", "eig", "rank", "rfac"):                           # replicated on every row of the molecule
            assert (got[k][rows] == got[k][rows[0]]).all(), (g, root, k)
        kept = f["eigenvalues"][f["eigenvalues"] > 1e-10]
        if kept.min() < 1e-6 or f["rank"] < 20:
            continue                                                          # compared through tls_u alone
        for name, sl in TLS_BLOCKS.items():
            e = np.abs(got["params"][rows[0], sl].astype(np.float64) - fit["params"][rows[0], sl]).max()
            b = tu.EPS22 * np.abs(fit["params"][rows[0], sl]).max()
            worst["tls_params"] = max(worst["tls_params"], e / b)
            assert e <= b, (g, root, name, e, b)
        for sl in (slice(0, 3), slice(3, 6)):
            e = np.abs(got["eig"][rows[0], sl].astype(np.float64) - fit["eig"][rows[0], sl]).max()
            b = tu.EPS22 * np.abs(fit["eig"][rows[0], sl]).max()
            worst["tls_principal"] = max(worst["tls_principal"], e / b)
            assert e <= b, (g, root, sl, e, b)
    return worst


def test_everything_downstream_is_in_the_stored_frame(setup):
    import main as entry
    from cartnet_amd import predict as p
    from cartnet_amd.bonds import (angle_table_host, aniso_hydrogens_host, bond_table_host, molecules_host,
                                   riding_hydrogens_host, tls_fit_host)
    from cartnet_amd.config import set_cfg
    from cartnet_amd.master import create_model
    from cartnet_amd.metrics import target_row_ptr
    model, sd, s, r, plain = setup
    res = p.predict_adps(model, _loader(s["unlabeled"]), DEV, model_frame=r["unlabeled"], **ANALYSES)
    analyses = p.Analyses(*(ANALYSES[k] for k in p.Analyses._fields))
    assert tuple(res) == p.result_keys(analyses, False, 1, 0.4, 0.4, True)
    for g in range(4):                                                        # the analyses do not change the prediction
        assert torch.equal(res["u_cart"][g], plain["u_cart"][g])
    # (a) what does not depend on U: a CartNet pass over the same stored shard and graph, bit for bit
    try:
        entry.fill_cfg(entry.build_parser().parse_args(["--dim_in", "32", "--num_layers", "2"]))
        torch.manual_seed(0)
        cart = p.predict_adps(create_model().eval(), _loader(s["unlabeled"]), DEV, **ANALYSES)
    finally:
        set_cfg()
    assert tuple(cart) == p.result_keys(analyses, False, 1, 0.4, 0.4)
    for k in INDEPENDENT:
        for g in range(4):
            assert res[k][g].dtype == cart[k][g].dtype and mf.bits(res[k][g]) == mf.bits(cart[k][g]), (k, g)
    assert rel_err(torch.cat(cart["u_cart"]), torch.cat(res["u_cart"])) > 100 * PRED_TOL      # another model: another U
    # (b) what depends on U: the kernels of the pass on the returned u_cart and the STORED batch, bit for bit
    dependent = [k for k in res if k not in INDEPENDENT + p.MF_KEYS + ("name", "temp", "u_cart")]
    assert {"u_cif", "u_eq", "axes", "bond_delta_max", "u_iso", "mol_delta_max", "tls_u", "tls_L", "h_u_cart", "bonds_delta",
            "bonds_libration", "angles_libration", "torsions_libration"} <= set(dependent)
    first = 0
    for batch in _loader(s["unlabeled"]):
        B = int(batch.num_graphs)
        row_ptr = target_row_ptr(batch)
        u = torch.cat(res["u_cart"][first:first + B]).to(DEV)
        graph, mo, index, angles = p._of_the_graph(batch, row_ptr, int(u.shape[0]), analyses, 0.4, 0.4)
        dev = p._exported(u, batch, row_ptr, None, analyses, graph, mo, index, angles)
        dev.update(_row_ptr=row_ptr, _atom_ptr=batch.ptr, _bond_ptr=index.bond_ptr, _angle_ptr=angles.angle_ptr,
                   _torsion_ptr=angles.torsion_ptr)
        host = p.to_host(dev)
        counts = {n: (host[f"_{q}_ptr"][1:] - host[f"_{q}_ptr"][:-1]).tolist()
                  for n, q in (("row", "row"), ("atom", "atom"), ("bond", "bond"), ("angle", "angle"), ("torsion", "torsion"))}
        for k in dependent:
            pieces = list(host[k].unbind(0)) if p.CUT[k] == "crystal" else p.split_rows(host[k], counts[p.CUT[k]])
            for g in range(B):
                assert mf.bits(pieces[g]) == mf.bits(res[k][first + g]), (k, first + g)
        first += B
    # (c) the numpy rules of bonds.py on the returned u_cart and the stored edges
    worst = {}
    for g, d in enumerate(mf.crystals(False)):
        z, ei = d.x.numpy(), d.edge_index.numpy()
        dist, dirs, row = d.cart_dist.numpy(), d.cart_dir.numpy(), mu.atom_rows((d.x != 1).numpy())
        u, params, rank = res["u_cart"][g].numpy(), _tls_params(res, g), res["tls_rank"][g].numpy()
        parent, count, mult, u_iso = riding_hydrogens_host(z, ei, dist, row, res["u_eq"][g].numpy(), 0.4, 1.2, 1.5)
        assert np.array_equal(res["h_parent"][g].numpy(), parent) and np.array_equal(res["h_count"][g].numpy(), count)
        assert res["h_mult"][g].numpy().tobytes() == mult.tobytes()
        assert int(bu.ulps(res["u_iso"][g].numpy(), u_iso).max()) <= 1, g
        got = {c: res[f"bonds_{c}"][g].numpy() for c in bu.COLUMNS}
        w = bu.same_table(got, bond_table_host(u, z, ei, dist, dirs, row, None, 0.4, params, rank))
        got = {"angles": {c: res[f"angles_{c}"][g].numpy() for c in at.ANGLE_COLUMNS},
               "torsions": {c: res[f"torsions_{c}"][g].numpy() for c in at.TORSION_COLUMNS}}
        w.update(at.same_tables(got, angle_table_host(z, ei, dist, dirs, row, None, 0.4, params, rank)))
        # the molecules, the TLS fit and the hydrogen tensors: the host chain of tests/aniso_utils.py on the stored edges
        # and the returned u_cart, nothing of it taken from the pass; the bounds of tests/test_gpu_tls_fit.py and
        # tests/test_gpu_aniso_h.py
        mo = molecules_host(z, ei, dist, dirs, row, None, 0.4)
        heavy = row >= 0
        assert np.array_equal(res["mol_size"][g].numpy(), mo["size"]) and np.array_equal(res["mol_status"][g].numpy(),
                                                                                         mo["status"])
        want_pos = np.where((mo["status"] == 0)[:, None], mo["x"][heavy], np.nan)
        got_pos = res["mol_pos"][g].numpy()
        assert np.array_equal(np.isnan(got_pos), np.isnan(want_pos))
        assert np.nan_to_num(np.abs(got_pos - want_pos)).max() <= 2.0 ** -23 * max(1.0, np.nanmax(np.abs(want_pos), initial=0.0))
        fit = tls_fit_host(u, mo["label"], mo["x"], row, mo["status"], mo["size"])
        assert len(fit["molecules"]) == (1 if g == mf.HELIX[0] else 0)       # the chain of crystal 3, and nothing else
        w.update(_tls_against_the_rule(res, g, u, params, fit, mo, row))
        ref = aniso_hydrogens_host(u, z, ei, dist, dirs, row, parent, x=mo["x"], params=fit["params"], rank=fit["rank"],
                                   stretch=ANALYSES["aniso_h"][0], bend=ANALYSES["aniso_h"][1])
        u_h, source = res["h_u_cart"][g].numpy(), res["h_source"][g].numpy()
        assert np.array_equal(source, ref["source"]) and u_h.dtype == np.float32
        assert u_h[source == 1].tobytes() == u.tobytes() == ref["u_h"][source == 1].tobytes()          # bit for bit
        assert np.array_equal(np.isnan(u_h), np.isnan(ref["u_h"])) and np.isnan(u_h[source == 0]).all()
        hyd = source >= 2
        bound = tu.EPS22 * float(np.abs(u).max())
        w["h_u_cart"] = float(np.abs(u_h[hyd].astype(np.float64) - ref["u_h"][hyd].astype(np.float64)).max(initial=0.0)) / bound
        assert w["h_u_cart"] <= 1.0, (g, w["h_u_cart"])
        have = source >= 1              # and their export in the STORED cell, at the export's own bound (test_gpu_adp_export.py)
        cif, eq, _, _ = pu.export_reference(u_h[have], d.cell[0].numpy())
        assert np.abs(res["h_u_eq"][g].numpy()[have].astype(np.float64) - eq).max() <= 2.0 ** -23 * np.abs(eq).max()
        assert np.abs(res["h_u_cif"][g].numpy()[have].astype(np.float64) - cif).max() <= 2.0 ** -23 * np.abs(cif).max()
        assert np.isnan(res["h_u_eq"][g].numpy()[~have]).all()
        # the libration columns once more, with the host fit's parameters: a parameter within 2^-22 of its block moves the
        # fp64 length or angle by less than half an fp32 unit, so the stored value by at most one unit more
        hb = bond_table_host(u, z, ei, dist, dirs, row, None, 0.4, fit["params"], fit["rank"])
        ha = angle_table_host(z, ei, dist, dirs, row, None, 0.4, fit["params"], fit["rank"])
        for name, got_col, want_col in (("bonds", res["bonds_libration"][g], hb["libration"]),
                                        ("angles", res["angles_libration"][g], ha["angles"]["libration"]),
                                        ("torsions", res["torsions_libration"][g], ha["torsions"]["libration"])):
            dist_ulp = bu.ulps(got_col.numpy(), want_col)
            w[f"{name}_libration_host_fit"] = int(dist_ulp.max()) if dist_ulp.size else 0
            assert w[f"{name}_libration_host_fit"] <= 2, (g, name)
        worst[g] = w
    print(f"largest distance from the numpy rules in fp32 units in the last place, per crystal: {worst}")
    # the checks above are not empty: hydrogens ride, the chain of crystal 3 is fitted and its bonds and angles librate
    assert int((res["h_parent"][1] >= 0).sum()) == int((mf.crystals(False)[1].x == 1).sum()) > 0
    h = mf.HELIX
    assert res["tls_rank"][h[0]][:h[1]].tolist() == [int(res["tls_rank"][h[0]][0])] * h[1] and int(res["tls_rank"][h[0]][0]) > 0
    assert int(torch.isfinite(res["bonds_libration"][h[0]]).sum()) >= h[1] - 1
    assert int(torch.isfinite(res["angles_libration"][h[0]]).sum()) >= h[1] - 2
    assert int(torch.isfinite(res["torsions_libration"][h[0]]).sum()) >= h[1] - 3


def test_the_temperature_series_runs_on_the_view(setup):
    from cartnet_amd.predict import predict_adps
    model, sd, s, r, res = setup
    kelvin = [100.0, 200.0, 300.0]
    out = predict_adps(model, _loader(s["unlabeled"]), DEV, temperatures=kelvin, model_frame=r["unlabeled"])
    assert len(out["name"]) == 12 and out["temp"] == kelvin * 4 and out["name"][:3] == ["crystal0_100K", "crystal0_200K",
                                                                                       "crystal0_300K"]
    assert len(out["series"]["name"]) == 4 and tuple(out["series"]["t_slope"][1].shape) == (int(res["u_cart"][1].shape[0]), 6)
    for g in range(4):
        for t in range(3):
            e = 3 * g + t
            assert mf.bits(out["cell_rotation"][e]) == mf.bits(res["cell_rotation"][g])
            assert torch.equal(out["cell"][e], res["cell"][g])
    # crystal 1 is stored at 200 K: its entry at 200 K is its plain prediction, in another batch composition
    err = rel_err(out["u_cart"][3 * 1 + 1], res["u_cart"][1])
    print(f"crystal 1 at its stored 200 K, series against the plain pass: rel_err {err:.3e} (bound {BATCH_TOL:.1e})")
    assert err <= BATCH_TOL
    assert rel_err(out["u_cart"][3 * 1 + 0], res["u_cart"][1]) > 10 * BATCH_TOL            # the temperature is read

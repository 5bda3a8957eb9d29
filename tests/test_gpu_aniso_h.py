"""``cartnet_adp_aniso_h`` (csrc/aniso_h_ops.hip) against ``bonds.aniso_hydrogens_host`` on the arrays the kernel read:
eight crystals in one batch that hold every source code, a periodic molecule, hydrogens through a cell face, three
hydrogens on one parent, a crystal without rows in the middle, one without hydrogens, one whose tensors are not positive
definite, and two long interleaved molecules whose edge segments run past the sixteen lanes of a group.  ``molecules``,
``riding_h`` and ``tls_fit`` run on the GPU and their outputs are fed to both sides; both compute in fp64 and round once."""
import numpy as np
import pytest
import torch

import aniso_utils as au
import molecule_utils as mu
import tls_utils as tu
from test_gpu_bond_test import _make

pytestmark = pytest.mark.gpu

STRETCH, BEND = 0.005, 0.020
RADIUS = 10.0                    # at 5 A no edge segment of these crystals is longer than the 16 lanes of a group


def _host(t):
    return t.cpu().numpy()


def _rule(batch, u, rh, mo=None, tf=None):
    from cartnet_amd.bonds import aniso_hydrogens_host
    extra = dict(x=_host(mo.x), params=_host(tf.params), rank=_host(tf.rank)) if tf is not None else {}
    return aniso_hydrogens_host(_host(u), _host(batch["x"]), _host(batch["edge_index"]), _host(batch["cart_dist"]),
                                _host(batch["cart_dir"]), mu.atom_rows(_host(batch["non_H_mask"])), _host(rh.parent),
                                stretch=STRETCH, bend=BEND, ptr=_host(batch["ptr"]), **extra)


@pytest.fixture(scope="module")
def fixture():
    """The batch, what the three earlier kernels give for it, one ``aniso_h`` with and one without the TLS results, and
    the numpy rule on the same arrays; computed once."""
    from cartnet_amd import metrics as gm
    crystals, rows = au.gpu_crystals()
    batch, u, row_ptr = _make(crystals, 0, radius=RADIUS, u=torch.from_numpy(rows))
    ex_ueq = (u[:, 0, 0] + u[:, 1, 1] + u[:, 2, 2]) / 3
    rh = gm.riding_h(ex_ueq.contiguous(), batch)
    mo = gm.molecules(batch, row_ptr, mu.TOL, rows=int(u.shape[0]))
    tf = gm.tls_fit(u, batch, row_ptr, mo)
    res = gm.aniso_h(u, batch, row_ptr, rh, mo, tf, STRETCH, BEND)
    bare = gm.aniso_h(u, batch, row_ptr, rh, stretch=STRETCH, bend=BEND)
    return batch, u, row_ptr, rh, mo, tf, res, bare, _rule(batch, u, rh, mo, tf), _rule(batch, u, rh)


def test_the_fixture_holds_every_kind(fixture):
    batch, u, row_ptr, rh, mo, tf, res, bare, ref, ref_bare = fixture
    ptr, z = _host(batch["ptr"]), _host(batch["x"])
    per = [np.bincount(ref["source"][ptr[g]:ptr[g + 1]], minlength=5).tolist() for g in range(8)]
    assert per == [[1, 24, 3, 13, 8], [0, 8, 8, 0, 0], [0, 7, 0, 7, 0], [3, 0, 0, 0, 0], [0, 5, 0, 3, 0], [0, 5, 0, 0, 0],
                   [0, 6, 0, 6, 0], [0, 195, 0, 195, 0]]
    assert mo.crystal_counts[:, 2].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]           # the polymer is periodic
    assert int(row_ptr[4] - row_ptr[3]) == 0 and int(ptr[4] - ptr[3]) == 3                        # no rows in the middle
    parent = _host(rh.parent)
    assert np.bincount(parent[ptr[4]:ptr[5]][z[ptr[4]:ptr[5]] == 1] - ptr[4]).tolist() == [0, 0, 3]   # the methyl carbon
    pos_face = au.face_crystal(True)[0]
    assert (np.abs(pos_face - au.face_crystal(False)[0]).max(axis=1) > 1.0).sum() == 2             # through the face
    seg = np.bincount(_host(batch["edge_index"])[1], minlength=len(z))
    long = seg[ptr[7]:ptr[8]]
    assert long.min() < 16 and (long > 16).sum() > 300 and (long > 32).sum() > 100                 # one, two and three passes
    label = _host(mo.label)[ptr[7]:ptr[8]][0::2]
    assert len(set(label.tolist())) == 2 and (label[1:] != label[:-1]).sum() > 50                  # interleaved
    assert ref["crystal_stats"][:, 3].tolist() == [0, 0, 0, 0, 0, 0, 6.0, 0]                       # the negated rows
    assert ref_bare["crystal_stats"][:, 0].tolist() == ref["crystal_stats"][:, 0].tolist() == [24.0, 8, 7, 0, 3, 0, 6, 195]


@pytest.mark.parametrize("with_tls", [True, False], ids=["tls", "no_tls"])
def test_atoms_against_the_numpy_rule(fixture, with_tls):
    batch, u, row_ptr, rh, mo, tf, res, bare, ref, ref_bare = fixture
    got, want = (res, ref) if with_tls else (bare, ref_bare)
    N = int(batch["x"].shape[0])
    u_h, source = _host(got.u_h), _host(got.source)
    assert u_h.shape == (N, 3, 3) and u_h.dtype == np.float32 and source.shape == (N,) and source.dtype == np.int32
    assert np.array_equal(source, want["source"])
    if not with_tls:
        assert set(source.tolist()) == {0, 1, 2}
    copied = source == 1
    assert u_h[copied].tobytes() == _host(u).tobytes() == want["u_h"][copied].tobytes()            # bit for bit
    assert np.array_equal(np.isnan(u_h), np.isnan(want["u_h"])) and np.isnan(u_h[source == 0]).all()
    assert not np.isnan(u_h[source > 0]).any()
    h = source >= 2
    bound = tu.EPS22 * float(np.abs(_host(u)).max())
    err = float(np.abs(u_h[h].astype(np.float64) - want["u_h"][h].astype(np.float64)).max())
    print(f"largest |kernel - rule| over {int(h.sum())} hydrogens: {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert np.array_equal(u_h[h], u_h[h].transpose(0, 2, 1))                                       # exactly symmetric
    if with_tls:
        assert np.abs(want["lib"][source >= 3]).max() > 1e-4 and not np.array_equal(u_h, _host(bare.u_h))


@pytest.mark.parametrize("with_tls", [True, False], ids=["tls", "no_tls"])
def test_crystal_stats(fixture, with_tls):
    batch, u, row_ptr, rh, mo, tf, res, bare, ref, ref_bare = fixture
    from cartnet_amd.bonds import positive_definite
    got, want = (res, ref) if with_tls else (bare, ref_bare)
    stats = _host(got.crystal_stats)
    assert stats.shape == (8, 4) and stats.dtype == np.float64
    u_h, source, ptr = _host(got.u_h), _host(got.source), _host(batch["ptr"])
    for g in range(8):                                                         # from the values as stored
        a = np.arange(ptr[g], ptr[g + 1])
        a = a[source[a] >= 2]
        t = u_h[a].astype(np.float64)
        assert stats[g, 0] == len(a) and stats[g, 1] == (source[a] >= 3).sum()
        assert stats[g, 3] == (~positive_definite(u_h[a])).sum()
        assert stats[g, 2] == pytest.approx(np.trace(t, axis1=1, axis2=2).sum() / 3.0, rel=1e-12, abs=0.0 if len(a) else 1e-300)
    assert np.array_equal(stats[:, [0, 1, 3]], want["crystal_stats"][:, [0, 1, 3]])
    assert stats[3].tolist() == [0.0] * 4 and stats[5].tolist() == [0.0] * 4 and stats[6, 3] == 6.0


def test_two_calls_give_the_same_bytes(fixture):
    from cartnet_amd import metrics as gm
    batch, u, row_ptr, rh, mo, tf, res, bare, ref, ref_bare = fixture
    again = gm.aniso_h(u, batch, row_ptr, rh, mo, tf, STRETCH, BEND)
    for a, b in zip(res, again):
        assert _host(a).tobytes() == _host(b).tobytes()


def test_the_export_over_atoms_keeps_the_rows_of_the_pass(fixture):
    """``predict.aniso_entries``: one ``adp_export`` over atoms as rows; a non-hydrogen atom's ``h_u_cif`` is its row's
    ``u_cif`` of the pass bit for bit, and NaN rows stay NaN without harm."""
    from types import SimpleNamespace
    from cartnet_amd import metrics as gm
    from cartnet_amd.predict import AH_KEYS, aniso_entries
    batch, u, row_ptr, rh, mo, tf, res, bare, ref, ref_bare = fixture
    crystals, _ = au.gpu_crystals()
    cell = torch.tensor(np.stack([c[1] for c in crystals]), dtype=torch.float32).cuda()
    ex = gm.adp_export(u, row_ptr, cell, axes=False, stats=False, check=False)
    ent = aniso_entries(res, SimpleNamespace(ptr=batch["ptr"], cell=cell))
    assert tuple(ent) == AH_KEYS
    heavy = batch["non_H_mask"]
    assert _host(ent["h_u_cif"][heavy]).tobytes() == _host(ex.u_cif).tobytes()
    assert _host(ent["h_u_eq"][heavy]).tobytes() == _host(ex.u_eq).tobytes()
    none = res.source == 0
    assert bool(torch.isnan(ent["h_u_cif"][none]).all()) and not bool(torch.isnan(ent["h_u_cif"][~none]).any())
    t = res.u_h[res.source >= 2].double()
    eq = t.diagonal(dim1=1, dim2=2).sum(1) / 3
    assert float((ent["h_u_eq"][res.source >= 2].double() - eq).abs().max()) <= tu.EPS22 * float(eq.abs().max())


def test_argument_checks_and_no_atoms(fixture):
    from cartnet_amd import metrics as gm
    batch, u, row_ptr, rh, mo, tf, res, bare, ref, ref_bare = fixture
    with pytest.raises(ValueError, match="u must be"):
        gm.aniso_h(u.double(), batch, row_ptr, rh)
    with pytest.raises(ValueError, match="together"):
        gm.aniso_h(u, batch, row_ptr, rh, molecules=mo)
    with pytest.raises(ValueError, match="riding does not belong"):
        gm.aniso_h(u, batch, row_ptr, rh._replace(parent=rh.parent[:-1]))
    with pytest.raises(ValueError, match="do not belong"):
        gm.aniso_h(u, batch, row_ptr, rh, mo, tf._replace(params=tf.params[:, :20]))
    with pytest.raises(ValueError, match="batch.ptr"):
        gm.aniso_h(u, {k: v for k, v in batch.items() if k != "ptr"}, row_ptr, rh)
    # N == 0: nothing is launched
    dev = u.device
    zero = torch.zeros(2, dtype=torch.int64, device=dev)
    empty = {"x": torch.zeros(0, dtype=torch.int64, device=dev), "edge_index": torch.zeros((2, 0), dtype=torch.int64, device=dev),
             "cart_dist": torch.zeros(0, device=dev), "cart_dir": torch.zeros((0, 3), device=dev), "ptr": zero}
    none = gm.aniso_h(u[:0], empty, zero, gm.riding_h(u[:0, 0, 0].contiguous(), empty))
    assert tuple(none.u_h.shape) == (0, 3, 3) and none.crystal_stats.tolist() == [[0.0] * 4]
    # E == 0: every hydrogen is an orphan, the rows are still copied
    lone = dict(batch, edge_index=torch.zeros((2, 0), dtype=torch.int64, device=dev), cart_dist=torch.zeros(0, device=dev),
                cart_dir=torch.zeros((0, 3), device=dev))
    alone = gm.aniso_h(u, lone, row_ptr, gm.riding_h(u[:, 0, 0].contiguous(), lone))
    assert set(alone.source.tolist()) == {0, 1} and _host(alone.u_h[alone.source == 1]).tobytes() == _host(u).tobytes()
    assert float(alone.crystal_stats.abs().sum()) == 0.0

"""The per-crystal fp64 figures of ``adp_eval``, ``adp_export``, ``frame_mean``, ``bond_test`` and ``riding_h`` byte for byte
against a numpy emulation of the one-wave-per-crystal reduction they share (csrc/crystal_reduce.h): 64 fp64 lane
accumulators, lane ``l`` takes rows ``l, l + 64, ...`` in order, the lanes are folded by the butterfly ``o = 32 ... 1``
(``s = op(s, s[lane ^ o])``) and lane 0 is read.  The emulation starts from the per-row arrays the same call returned, so the
expectation follows from the documented order alone and needs no tolerance.  One batch of seven crystals whose row counts
are the smallest at which a wave-strided loop and a 64-lane fold can go wrong: an empty crystal first and in the middle, one
row, a wave minus one, a wave, a wave plus one, more than two waves."""
import numpy as np
import pytest
import torch

import test_gpu_bond_test as tb
import test_gpu_riding_h as tr
from test_gpu_adp_export import _cells, _tensors
from test_gpu_eval_batch import _spd_pair

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 63, 64, 65, 0, 130]
B, M = len(ROWS), sum(ROWS)
PTR = np.concatenate([[0], np.cumsum(ROWS)])
LANES = 64


def _add(acc, x):
    return acc + x


def _max_nan(hi, x):
    """The kernels' maximum: a NaN is kept, not dropped as fmax would."""
    return np.where((x > hi) | (x != x), x, hi)


def _wave(values, op, start):
    """Lane 0 after the strided accumulation and the butterfly.  ``values`` [n] or [n,k] fp64 in row order (the k elements
    of a row enter one after another); ``op(acc, x)`` elementwise."""
    acc = np.full(LANES, start, dtype=np.float64)
    values = np.asarray(values, dtype=np.float64)
    for r in range(len(values)):                                              # (an empty crystal: nothing is added)
        for x in values[r].reshape(-1):
            acc[r % LANES] = op(acc[r % LANES], x)
    with np.errstate(invalid="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            acc = op(acc, acc[np.arange(LANES) ^ o])
    return acc[0]


def _emulate(columns, ptr=PTR):
    """[B, len(columns)] fp64; ``columns``: (per-row values, op, start) each."""
    return np.array([[_wave(v[ptr[g]:ptr[g + 1]], op, start) for v, op, start in columns] for g in range(len(ptr) - 1)])


def _same_bytes(got: torch.Tensor, want: np.ndarray):
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), (got, want)


def _np(t):
    return t.cpu().numpy()


def _row_ptr():
    return torch.from_numpy(PTR).cuda()


def test_adp_eval():
    from cartnet_amd import metrics as gm
    pred, true = _spd_pair(M)
    res = gm.adp_eval(pred, true, _row_ptr(), num_points=16)
    assert res.rows.tolist() == ROWS
    _same_bytes(res.crystal_sums, _emulate([(_np(res.abs_err).reshape(M, 9), _add, 0.0)]
                                           + [(_np(t), _add, 0.0) for t in (res.volume_error, res.similarity_index, res.iou)]))
    part = gm.adp_eval(pred, true, _row_ptr(), volume=False, iou=False)       # a metric that was not computed leaves 0
    want = _emulate([(_np(part.abs_err).reshape(M, 9), _add, 0.0), (_np(part.similarity_index), _add, 0.0)])
    _same_bytes(part.crystal_sums, np.stack([want[:, 0], np.zeros(B), want[:, 1], np.zeros(B)], axis=1))


def test_adp_export():
    from cartnet_amd import metrics as gm
    u = _tensors(M, 31)
    u[PTR[3] + 5] = -u[PTR[3] + 5]                                            # one row with negative principal values
    res = gm.adp_export(u.cuda(), _row_ptr(), torch.from_numpy(_cells(B, 1)).cuda())
    low = _np(res.principal)[:, 0]
    want = _emulate([(_np(res.u_eq), _add, 0.0), (low, np.fmin, np.inf), ((low <= 0).astype(np.float64), _add, 0.0)])
    assert want[3, 2] == 1.0 and want[3, 1] < 0 and want[0].tolist() == [0.0, np.inf, 0.0]
    _same_bytes(res.crystal_stats, want)


def _frame_inputs():
    from cartnet_amd.shard import random_rotations
    rot = random_rotations(2 * B, torch.Generator(device="cuda:0").manual_seed(5), "cuda:0").view(2, B, 3, 3)
    return _tensors(2 * M, 22).cuda(), rot


def test_frame_mean():
    from cartnet_amd import metrics as gm
    pred, rot = _frame_inputs()
    res = gm.frame_mean(pred, rot, _row_ptr())
    spread = _np(res.spread)
    assert (spread > 0).all()
    _same_bytes(res.crystal_spread, _emulate([(spread, _add, 0.0), (spread, _max_nan, 0.0)]))


def test_frame_mean_keeps_a_nan():
    """A NaN prediction in one frame of one row of the 65-row crystal: that crystal's maximum (and sum) is NaN, every other
    crystal's bytes are as without it."""
    from cartnet_amd import metrics as gm
    pred, rot = _frame_inputs()
    clean = _np(gm.frame_mean(pred, rot, _row_ptr()).crystal_spread)
    pred[M + PTR[4] + 40, 1, 2] = float("nan")                                # frame 1, row 40 of crystal 4
    res = gm.frame_mean(pred, rot, _row_ptr())
    got, spread = _np(res.crystal_spread), _np(res.spread)
    assert np.isnan(spread).sum() == 1 and np.isnan(spread[PTR[4] + 40])
    assert np.isnan(got[4]).all()
    others = [g for g in range(B) if g != 4]
    assert got[others].tobytes() == clean[others].tobytes()
    want = _emulate([(spread, _add, 0.0), (spread, _max_nan, 0.0)])
    assert np.isnan(want[4]).all() and want[others].tobytes() == got[others].tobytes()


def _bond_inputs():
    crystals = [tb._random_crystal(n, h, 300 + k) for k, (n, h) in enumerate(zip(ROWS, (3, 2, 20, 30, 25, 2, 60)))]
    batch, u, row_ptr = tb._make(crystals, 4)
    assert row_ptr.tolist() == PTR.tolist()
    return batch, u, row_ptr


def _bond_columns(res):
    return [(_np(res.bonds), _add, 0.0), (_np(res.delta_sum), _add, 0.0), (_np(res.delta_max), _max_nan, 0.0),
            (_np(res.over), _add, 0.0)]


def test_bond_test():
    from cartnet_amd import metrics as gm
    batch, u, row_ptr = _bond_inputs()
    res = gm.bond_test(u, batch, row_ptr, tb.TOL, tb.THRESHOLD)
    want = _emulate(_bond_columns(res))
    assert (want[[2, 3, 4, 6], 0] > 0).all() and (want[[2, 3, 4, 6], 3] > 0).all()        # bonds, and some over the threshold
    _same_bytes(res.crystal_stats, want)


def test_bond_test_keeps_a_nan():
    """A NaN row of ``u`` inside the 65-row crystal: its bonds' ``|D|`` are NaN, so the crystal's maximum is; every other
    crystal's bytes are as without it."""
    from cartnet_amd import metrics as gm
    batch, u, row_ptr = _bond_inputs()
    first = gm.bond_test(u, batch, row_ptr, tb.TOL, tb.THRESHOLD)
    clean = _np(first.crystal_stats)
    row = int(PTR[4] + _np(first.bonds)[PTR[4]:PTR[5]].argmax())              # a row that has bonds
    u[row] = float("nan")
    res = gm.bond_test(u, batch, row_ptr, tb.TOL, tb.THRESHOLD)
    got = _np(res.crystal_stats)
    assert np.isnan(_np(res.delta_max)[row]) and np.isnan(got[4, 2]) and np.isnan(got[4, 1])
    others = [g for g in range(B) if g != 4]
    assert got[others].tobytes() == clean[others].tobytes()
    want = _emulate(_bond_columns(res))
    assert np.isnan(want[4, 2]) and want[others].tobytes() == got[others].tobytes()
    assert want[4, [0, 3]].tobytes() == got[4, [0, 3]].tobytes()              # the counts of the crystal stay numbers


def test_riding_h():
    """Here ``ROWS`` are atom counts.  A hydrogen counts; one without a parent that has a row is an orphan; the others add
    their finite ``u_iso`` and count a parent whose ``u_eq`` is not positive."""
    from cartnet_amd import metrics as gm
    z, edges, ptr = tr._random(ROWS, 9)
    assert ptr == PTR.tolist()
    n_rows = int((np.asarray(z) != 1).sum())
    u_eq = 0.02 + 0.03 * np.random.default_rng(9).random(n_rows)
    u_eq[::7] = -u_eq[::7]                                                    # parents that are not positive
    u_eq[5::11] = np.nan
    batch, u_eq = tr._batch(z, edges, ptr, u_eq=u_eq)
    res = gm.riding_h(u_eq, batch, tr.TOL, tr.F, tr.F_ROT)
    z, parent, u_iso, ueq = np.asarray(z), _np(res.parent), _np(res.u_iso), _np(u_eq)
    row = np.cumsum(z != 1) - 1                                               # of a non-hydrogen atom
    hydrogen = z == 1
    rider = hydrogen & (parent >= 0)                                          # the kernel gives a parent only if it has a row
    assert not hydrogen[parent[rider]].any()
    parent_ueq = np.where(rider, ueq[row[np.where(rider, parent, 0)]], 1.0)
    finite = rider & np.isfinite(u_iso)
    want = _emulate([(hydrogen.astype(np.float64), _add, 0.0), ((hydrogen & ~rider).astype(np.float64), _add, 0.0),
                     (np.where(finite, u_iso, np.float32(0.0)), _add, 0.0),
                     ((rider & ~(parent_ueq > 0)).astype(np.float64), _add, 0.0)])
    big = [2, 3, 4, 6]
    assert (want[big, 0] > want[big, 1]).all() and want[:, 1].sum() > 0 and want[:, 3].sum() > 0         # not vacuous
    assert (rider & ~finite).any()                                            # a NaN value stays out of the sum
    _same_bytes(res.crystal_stats, want)

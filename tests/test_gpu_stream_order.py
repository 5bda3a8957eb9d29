"""Stream order of the two-stream training step: the same bytes for any relative speed of the two streams.

Every training step runs on two HIP streams -- cartnet_model_forward / _backward and cartnet_icomformer_forward / _backward
order them through `Streams` (csrc/model_common.h), the Python-sequenced iComformer / eComformer backward with
`wait_stream`.  The kernels sum in fixed orders without atomics, so a correct schedule gives the same bytes whatever the
relative speed of the streams, and the bytes of the one-stream program.  A missing wait breaks that only when timing
exposes it; here timing is forced: each case runs the checked step of tests/stream_utils.py (a decoy step on the same
shapes first, so memory read too early holds another step's values) in four modes

  A  overlap_weight_gradients = False (one stream)          C  two streams, the side stream late at every section
  B  two streams, no skew                                   D  two streams, the main stream late at every section

and every returned tensor of B, C and D must equal A's bit for bit.  A is first run twice, so that the criterion is known
to hold for the one-stream schedule alone.  The spin length is measured per case: one mode-A step timed with HIP events,
usec = clamp(2 x step / sections, 100, 2000), so that each spin outlasts several of the small kernels it races against.

No tensor differs between the one-stream and the two-stream program at any case below (S.dual selects an order of
launches, never another kernel or summation order), so every comparison is bitwise.
"""
import functools

import pytest
import torch

import stream_utils as su
from test_gpu_model import _model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# Ordering calls executed per step, roughly (the spin length only needs the scale).  CartNet: forward 5 (constructor, two
# forks, two marks), backward 1 + 2 (head) + 5 per layer (three forks or marks and waits, side_done, the parity guard)
# + 4 (sort_done, the encoder's mark and wait, the join).  iComformer's C++ sequence: a fork per weight-gradient group,
# five rows_ready marks, three waits, three joins.  The Python sequence: one wait_stream per _wgrad / _side_branch /
# _join_wgrads call, 22 call sites, those of a layer once per layer.
SECTIONS_CARTNET = lambda L: 12 + 5 * L
SECTIONS_ICF_NATIVE = 40
SECTIONS_ICF_PYTHON = 60


def _usec(step_ms, sections):
    return int(min(2000, max(100, round(2.0 * step_ms * 1000.0 / sections))))


def _compare(m, sd, dsd, batch, sections, what, mode="train", opt=None, each=None, after_decoy=None, decoy=None):
    """Modes A (twice), B, C, D of one case; `each(tag, result)` runs after every mode's step.  Returns {tag: result}."""
    decoy = su.make_decoy(batch) if decoy is None else decoy
    kw = dict(mode=mode, opt=opt, after_decoy=after_decoy)
    res, ms = {}, {}

    def run(tag, which=su.OFF, usec=0):
        t = {}
        with su.skew(which, usec, m):
            res[tag] = su.step(m, sd, batch, decoy, dsd, timer=t, **kw)
        ms[tag] = t["ms"]
        if each is not None:
            each(tag, res[tag])

    m.overlap_weight_gradients = False
    run("A")
    run("A2")
    su.assert_same(res["A"], res["A2"], f"{what}: the one-stream step, repeated")
    usec = _usec(ms["A2"], sections)
    m.overlap_weight_gradients = True
    run("B")
    run("C", su.SIDE, usec)
    run("D", su.MAIN, usec)
    print(f"stream order [{what}]: spin {usec} us over ~{sections} sections; step A {ms['A2']:.3f} ms, B {ms['B']:.3f} ms, "
          f"C (side late) {ms['C']:.3f} ms, D (main late) {ms['D']:.3f} ms; {len(res['A'])} tensors")
    assert all(torch.isfinite(v.float()).all() for v in res["A"].values()), what
    for tag, name in (("B", "B, two streams"), ("C", "C, side stream late"), ("D", "D, main stream late")):
        su.assert_same(res["A"], res[tag], f"{what}: mode {name}")
    return res


# ------------------------------------------------------------------------------------------------------------------ CartNet
def _hp(**kw):
    hp = dict(dim_in=64, dim_rbf=16, num_layers=4, radius=5.0, invariant=False, temperature=True, use_envelope=True,
              atom_types=True, cholesky=True)
    hp.update(kw)
    return hp


@functools.lru_cache(maxsize=None)
def _crystals(first, sizes, adp=True):
    from cartnet_amd.data import Batch
    from cartnet_amd.synthetic import make_crystal
    return Batch.from_data_list([make_crystal(first + i, n, adp=adp) for i, n in enumerate(sizes)])


SMALL = (20, 33, 47, 60)      # 4 crystals of 20-60 atoms, ~2,300 edges: several row tiles, E < 32768


def _cartnet(hp, precision=0, seed=21):
    from cartnet_amd.model import make_state_dict
    args = (hp["dim_in"], hp["dim_rbf"], hp["num_layers"])
    kw = dict(cholesky=hp["cholesky"], temperature=hp["temperature"], atom_types=hp["atom_types"], invariant=hp["invariant"])
    sd, dsd = make_state_dict(*args, seed=seed, **kw), make_state_dict(*args, seed=seed + 100, **kw)
    return _model(hp, sd, precision), sd, dsd


def _small(hp):
    return su.clone_batch(_crystals(800, SMALL, hp["cholesky"])).to(DEV)


@pytest.mark.parametrize("precision", [0, 1])
def test_cartnet_four_layers(precision):
    """num_layers = 4: both parities of the write-after-read guard on dpre / dPn (`l + 2 < L`), the three forks per layer
    (precision 0) or the `pairs && S.dual` order with seg_first (precision 1, E < 32768), the deferred side jobs behind
    layer L - 1, sort_done."""
    hp = _hp()
    m, sd, dsd = _cartnet(hp, precision)
    b = _small(hp)
    assert int(b.edge_index.shape[1]) < 32768
    _compare(m, sd, dsd, b, SECTIONS_CARTNET(4), f"CartNet L=4 precision {precision}")


def test_cartnet_pairs_order_of_a_large_batch():
    """E >= 32768 at precision 1: the other side-stream order of the `pairs && S.dual` branch (apply_done, side_w2 queued
    under dpre)."""
    hp = _hp()
    m, sd, dsd = _cartnet(hp, 1)
    b = su.clone_batch(_crystals(700, (194,) * 12)).to(DEV)
    assert int(b.edge_index.shape[1]) >= 32768
    _compare(m, sd, dsd, b, SECTIONS_CARTNET(4), "CartNet L=4 precision 1, E >= 32768")


def test_cartnet_half_storage():
    hp = _hp(dim_in=256, dim_rbf=64)
    m, sd, dsd = _cartnet(hp, 2)
    m.half_storage = True
    _compare(m, sd, dsd, _small(hp), SECTIONS_CARTNET(4), "CartNet D=256 precision 2, bf16 storage")


@pytest.mark.parametrize("variant", ["no_atom_types", "scalar_head", "invariant", "bn_groups"])
def test_cartnet_variants(variant):
    """no_atom_types: the plain embedding path, no sort on the side stream; scalar_head: Scalar_head; invariant; bn_groups:
    bn_group_size = 2 on 4 crystals (w.groups)."""
    hp = _hp(**{"no_atom_types": dict(atom_types=False), "scalar_head": dict(cholesky=False, temperature=False),
                "invariant": dict(invariant=True), "bn_groups": {}}[variant])
    m, sd, dsd = _cartnet(hp)
    if variant == "bn_groups":
        m.bn_group_size = 2
    _compare(m, sd, dsd, _small(hp), SECTIONS_CARTNET(4), f"CartNet L=4 {variant}")


@pytest.mark.parametrize("mode", ["eval", "train_nograd", "dropped"])
def test_cartnet_forward_only_and_dropped_forward(mode):
    """eval / train_nograd: forward only (no CSC build aside).  dropped: a training-mode forward whose outputs are dropped
    without a backward, then at once a full step on another batch of the same shapes -- the dropped workspace went back
    to the allocator while the side stream may hold work on it."""
    hp = _hp()
    m, sd, dsd = _cartnet(hp)
    _compare(m, sd, dsd, _small(hp), 5 if mode != "dropped" else SECTIONS_CARTNET(4), f"CartNet L=4 {mode}", mode=mode)


def test_cartnet_deferred_graph_check():
    """validate_graph = False: the graph status word is copied on the side stream (model.py::_defer_graph_check).  One
    crystal of the decoy batch is malformed (its first edge starts in another crystal); flush_graph_checks() must report
    it in every mode, and the step after it must still equal mode A."""
    hp = _hp()
    m, sd, dsd = _cartnet(hp)
    m.validate_graph = False
    b = _small(hp)
    reported = []

    def flush():
        with pytest.raises(ValueError):
            m.flush_graph_checks()
        reported.append(True)

    decoy = su.make_decoy(b)
    ei = decoy.edge_index.clone()
    ei[0, 0] = int(decoy.x.shape[0]) - 1 if int(ei[1, 0]) == 0 else 0
    decoy.edge_index = ei
    _compare(m, sd, dsd, b, SECTIONS_CARTNET(4), "CartNet L=4 deferred graph check", after_decoy=flush, decoy=decoy)
    assert len(reported) == 5                                   # A, A again, B, C, D
    m.flush_graph_checks()                                      # the good batches left nothing behind


class _MirrorSync:
    """Stand-in for distributed.GradSync: bucket(lo, hi) copies the slice of the flat gradient on the stream it is
    announced on.  If the slice is final there, the mirror equals the flat gradient after the step."""

    def __init__(self, flat):
        self.flat = flat
        self.mirror = torch.full_like(flat, float("nan"))
        self.seen = 0

    def bucket(self, lo, hi):
        self.mirror[lo:hi].copy_(self.flat[lo:hi])
        self.seen += 1


def test_cartnet_gradient_buckets_are_final_on_the_stream_they_are_announced_on():
    from cartnet_amd.optim import FlatAdam
    hp = _hp()
    m, sd, dsd = _cartnet(hp)
    m.train()
    opt = FlatAdam(m, lr=1e-3)
    sync = _MirrorSync(opt.flat_grad)
    m.grad_sync = sync

    def each(tag, result):
        assert sync.seen == 2 * (hp["num_layers"] + 2), tag        # the decoy step and the step, head + layers + encoder
        assert torch.equal(sync.mirror, opt.flat_grad), f"mode {tag}: a bucket was announced before its gradient was final"
        sync.mirror.fill_(float("nan"))
        sync.seen = 0

    try:
        _compare(m, sd, dsd, _small(hp), SECTIONS_CARTNET(4) + 4, "CartNet L=4 gradient buckets", opt=opt, each=each)
    finally:
        m.grad_sync = None


# --------------------------------------------------------------------------------------------------------------- Comformer
def _icomformer(width, native, precision, groups=0):
    from cartnet_amd.comformer import iComformer, make_icomformer_state_dict
    sd, dsd = make_icomformer_state_dict(width, seed=11), make_icomformer_state_dict(width, seed=111)
    m = iComformer(width)
    m.load_state_dict(sd)
    m.native_sequence = native
    m.gemm_precision = precision
    m.bn_group_size = groups
    m.validate_graph = True
    return m.to(DEV), sd, dsd


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("groups", [0, 2])
def test_icomformer_native_sequence(groups, precision):
    """csrc/icomformer.hip at the smallest width of the golden fixtures; groups = 2 on 4 crystals is the 4 x 16
    BatchNorm-groups recipe in miniature."""
    m, sd, dsd = _icomformer(16, True, precision, groups)
    b = su.clone_batch(_crystals(960, (10, 17, 24, 13))).to(DEV)
    _compare(m, sd, dsd, b, SECTIONS_ICF_NATIVE, f"iComformer C++ sequence, precision {precision}, groups {groups}")


@pytest.mark.parametrize("precision", [0, 1])
def test_icomformer_python_sequence(precision):
    """native_sequence = False: `_wgrad`, `_side_branch`, `_join_wgrads` and the `_KEEP` list of cartnet_amd/comformer.py
    (one BatchNorm group: the Python sequence has no groups)."""
    m, sd, dsd = _icomformer(16, False, precision)
    b = su.clone_batch(_crystals(960, (10, 17, 24, 13))).to(DEV)
    _compare(m, sd, dsd, b, SECTIONS_ICF_PYTHON, f"iComformer Python sequence, precision {precision}")


def test_ecomformer():
    from cartnet_amd.comformer import eComformer, make_ecomformer_state_dict
    sd, dsd = make_ecomformer_state_dict(32, seed=4), make_ecomformer_state_dict(32, seed=104)
    m = eComformer(32)
    m.load_state_dict(sd)
    m.validate_graph = True
    b = su.clone_batch(_crystals(1000, (1, 2, 23, 11))).to(DEV)
    _compare(m.to(DEV), sd, dsd, b, SECTIONS_ICF_PYTHON, "eComformer width 32")


# ------------------------------------------------------------------------------------------------------ the seam itself
# One iteration of the spin's loop is a clock read and a sleep of 512 shader cycles (0.2 us at 2.4 GHz, 4 us at the lowest
# clock); the two events around it add the dispatch and the completion of one kernel, some 10 us.  Measured on an idle
# stream of the MI355X: 6.2 us for usec = 0, and 3.4 to 3.6 us more than asked at 100, 1000 and 5000 us.
SPIN_MARGIN_US = 50.0


def test_spin_lasts_what_was_asked():
    from cartnet_amd import ops
    s = torch.cuda.Stream(device=DEV)
    ops.debug_spin(100, s)                                       # (code object load, first launch)
    s.synchronize()
    for usec in (0, 100, 1000, 5000):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        ops.debug_spin(usec, s)
        e1.record(s)
        s.synchronize()
        got = 1000.0 * e0.elapsed_time(e1)
        print(f"debug_spin({usec}): {got:.1f} us between the events around it")
        assert usec <= got <= usec + SPIN_MARGIN_US, (usec, got)


def test_skew_queues_a_spin_at_every_section_of_a_backward():
    """CartNet, precision 0, L = 4, atom types, no gradient buckets.  The main stream's sections of cartnet_model_backward:
    the constructor, mark_main in the head, three forks per layer, the parity guard of layers 1 and 0, mark_main in the
    encoder, main_waits(sort_done), the join's wait: 1 + 1 + 12 + 2 + 1 + 1 + 1 = 19, all in the main stream's order, which
    the two events bracket.  The side stream's, between its first wait for the main stream and the join's mark that the main
    stream waits for: side_waits in the head, three forks and side_done per layer, sort_done, side_waits in the encoder:
    1 + 16 + 1 + 1 = 19 (the constructor's spin runs before the first event).  The main stream is held by one spin while
    the host queues the whole backward, so that no timing is paced by the host.

    What is asserted, with t_off the unskewed two-stream backward and n = 19: n * usec <= t_skew <= t_off + (n + 1) * usec.
    The spins of one stream run one after the other and each lasts at least usec (test_spin_lasts_what_was_asked), which
    gives the left side; on the right, a spin costs its length and a dispatch.  With usec = 2000 us, several times t_off
    (0.6 ms), the two sides admit exactly n spins: one fewer ends below n * usec, one more above the right side.
    `t_skew - t_off >= n * usec` alone does not hold in general: t_off contains the time the timed stream waits for the
    other one, and a late stream no longer waits.  MI355X, usec = 500: t_off 0.614 ms, main late 10.105 ms (9.491 more,
    against 9.500), side late 10.153 ms (9.539 more).  The difference is printed."""
    from cartnet_amd import ops
    hp = _hp()
    m, sd, _ = _cartnet(hp)
    m.train()
    b = _small(hp)
    usec, n = 2000, 19

    def backward_ms(which):
        m.zero_grad(set_to_none=True)
        with su.skew(which, usec, m):
            pred, true = m(su.clone_batch(b))
            loss = (pred - true).abs().mean()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ops.debug_spin(5000)
            e0.record()
            loss.backward()
            e1.record()
            torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    backward_ms(su.OFF)                                          # (first use of every kernel)
    t_off = backward_ms(su.OFF)
    assert t_off < 0.5 * usec / 1000.0, t_off                    # (what makes the two bounds admit exactly n spins)
    for which, name in ((su.MAIN, "main"), (su.SIDE, "side")):
        t = backward_ms(which)
        print(f"backward: {t_off:.3f} ms without skew, {t:.3f} ms with the {name} stream late by {n} spins of {usec} us: "
              f"{t - t_off:.3f} ms more")
        assert n * usec / 1000.0 <= t <= t_off + (n + 1) * usec / 1000.0, (name, t, t_off)


def test_skew_off_queues_nothing(monkeypatch):
    """With the skew off no spin is launched from the Python sequences (a counting wrapper around ops.debug_spin sees
    none); with it on, one per wait_stream between the two streams."""
    from cartnet_amd import ops
    calls = []
    real = ops.debug_spin
    monkeypatch.setattr(ops, "debug_spin", lambda usec, stream=None: (calls.append(usec), real(usec, stream))[1])
    m, sd, dsd = _icomformer(16, False, 0)
    b = su.clone_batch(_crystals(960, (10, 17, 24, 13))).to(DEV)
    with su.skew(su.OFF, 0, m) as state:
        su.step(m, sd, b, su.make_decoy(b), dsd)
        assert state["spins"] == 0
    su.step(m, sd, b, su.make_decoy(b), dsd)
    assert calls == []
    with su.skew(su.SIDE, 100, m) as state:
        su.step(m, sd, b, su.make_decoy(b), dsd)
        assert state["spins"] == len(calls) > 20

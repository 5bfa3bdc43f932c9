"""The proposal side (csrc/sst.hip, csrc/proposals.hip) in its TRAINED regime on the GPU (-m gpu): saturated gates, cell states far past +-1,
scores that are exactly 0.0 or 1.0 in float32.  Inputs and references: tests/proposal_regime_ref.py.

1. The criterion kernels on PLANTED scores and at their size boundaries, every entry through the C ABI, against oracle.tap_criterion in
   float64 (torch's binary_cross_entropy; its backward is (p - y) / max(p (1 - p), 1e-12) w / n).  Losses at 1e-5 relative; the gradient
   ELEMENT BY ELEMENT at |got - ref| <= 1e-5 |ref| + 1e-30 (the elements span 1e-9 .. 1e12: a max-norm would hide all but one).  Torch's formula
   in float32 numpy stays within 1.0e-7 of float64 on every planted value; the worst ratio the kernels show over all cases of this file is
   2.3e-7 (losses: 2.3e-7 relative).  The parent's gradient (-y / p + (1 - y) / (1 - p) with the clamped branch dropped) misses this gate at every
   planted score except 1 - 2^-24, 1 - 2^-23, 1.1e-12 and 1e-11: 0 for -3.5e11 at (p = 0, y = 1), inf at (1e-40, 1), 0.0197 for 0 at (0, 0).

2. The encoder VARIANTS on every route -- persistent (default) and wavefront (sst_persist = 0), one video and a batch, eval and train mode --
   against oracle.sst_forward in float64.  Gates: per output and per gradient tensor max(existing gate, 4 e_ref), never above
   the 1e-4 contract; existing gates 2e-5 absolute on tap / scores, 1e-5 relative loss, 1e-5 of the max-norm on gradients.  e_ref = float32 oracle
   against float64 oracle (CPU, tools/parity_report.py --sst), the largest of eval / train mode and of one video / batch.  4x: the other summation
   order and the 1-ulp hardware exp / rcp of fast_sigmoid / fast_tanh.  The relative loss gate applies to bce_chain only: the loss of the other
   variants is a signed sum of +-tap and +-scores terms whose relative error measures the cancellation of that sum, not a kernel.

   variant     e_ref: tap   scores    loss     grad     |  HIP path measured, persistent / wavefront (worst of eval, train, one video, batch)
   gates_sat        3.0e-6   3.7e-6   (3.3e-6)  2.7e-6   |  tap 4.5e-6 / 4.4e-6   scores 4.7e-6 / 4.6e-6   grad 5.1e-6 / 4.4e-6
   drift            1.5e-5   2.9e-6   (3.3e-6)  1.8e-5   |  tap 3.6e-5 / 3.6e-5   scores 5.9e-6 / 5.7e-6   grad 2.2e-5 / 1.9e-5
   bce_chain        3.0e-6   2.5e-6    1.8e-5   2.5e-6   |  tap 4.2e-6 / 4.3e-6   scores 3.3e-6 / 3.4e-6   grad 3.4e-6 / 3.7e-6   loss 1.7e-5 / 1.7e-5
   small_h          6.3e-7   8.6e-7   (2.0e-6)  3.1e-6   |  tap 6.2e-7 (wavefront)  scores 6.5e-7   grad 1.9e-6

   So the gates are the existing ones except: gates_sat gradients 1.1e-5; drift tap 6.0e-5 and gradients 7.2e-5 (cell states of 14 and 70 in
   the two layers cost the float32 reference itself 1.5e-5 over 100 steps); bce_chain loss 7.2e-5 (head logits up to 12.5: 1 - p = 3.7e-6 is known
   to 6e-8 in float32 there); small_h gradients 1.2e-5.

3. The selection (threshold form and NMS) on grids drawn from 1.0, its two float32 predecessors, 0.5, 2^-126, a denormal and 0.0, against
   oracle.top_proposals / top_proposals_nms, every output bit for bit.

Sensitivity (scratch builds, arithmetic altered only).  Group 1: on the parent's tap_bce_grad 33 of the 41 criterion cases fail (all but the
eight one-planted-score cases named above).  Group 2: with the arguments of fast_sigmoid clamped at +-8 in the persistent forward all twelve
persistent cases fail (and none of the wavefront's); with the argument of fast_tanh clamped at +-8 instead NONE fails -- tanh(8) = 1 - 2.3e-7
lies within rounding of the saturated value, an alteration no gate of this project can see.  Group 3: with `himask` of the radix select not
extended after pass 1 test_threshold_selection_on_saturated_scores[thres0] fails at its first topN (a rank inside the class of 1 - 2^-24 also
returns the class of 1 - 2^-23, whose key differs in the last bit).
"""
import functools

import numpy as np
import pytest
import torch

from tests import proposal_regime_ref as P
from tests import props_batch_ref as PB
from tests import sst_batch_ref as R
from tests import util as U
from tests.test_gpu_props_batch import assert_same, run_gpu

pytestmark = pytest.mark.gpu

TOL_OUT, TOL_LOSS, TOL_GRAD = 2e-5, 1e-5, 1e-5          # the existing gates (tests/test_gpu_sst_batch.py, tests/test_gpu_joint_batch.py)
CONTRACT = 1e-4


def _lib():
    from echr_amd import _lib as L
    return L, L.load()


def _dev():
    return torch.device('cuda')


# ---- 1. the criterion ---------------------------------------------------------------------------------------------------------------
SIZE_CASES = [(1, 1), (1, 3), (3, 21), (4, 16), (5, 13), (64, 64), (17, 241), (256, 256), (257, 256)]
BATCH_CASES = [(1, (1, 1, 2, 255, 1, 300, 3)), (3, (1, 85, 1, 86, 2)), (16, (1, 2, 5, 37, 5)), (300, (1, 2, 1, 3))]


@functools.lru_cache(maxsize=None)
def _bce_case(lengths, K, per_video=False, plant='all'):
    inp = P.bce_inputs(lengths, K, per_video, plant)
    return inp, P.bce_reference(inp)


def _upload(inp):
    dev = _dev()
    sc, mk, lb = (torch.from_numpy(inp[k]).to(dev) for k in ('scores', 'masks', 'labels'))
    ww = torch.from_numpy(np.ascontiguousarray(inp['w1'] if inp['per_video'] else inp['w1'][0])).to(dev)
    return sc, mk, lb, ww


def _single_entries(inp):
    """echr_tap_bce_fwd, echr_tap_bce_fwd_ws (twice) and echr_tap_bce_bwd on a one-video case: (loss, loss_ws, loss_ws again, d scores)."""
    L, lib = _lib()
    dev = _dev()
    assert len(inp['ro']) == 2
    T, K = inp['scores'].shape
    sc, mk, lb, ww = _upload(inp)
    one, a, b = (torch.full((n,), float('nan'), device=dev) for n in (1, 65, 65))
    gl, gs = torch.full((1,), P.G_LOSS, device=dev), torch.full((T, K), float('nan'), device=dev)
    L.check(lib.echr_tap_bce_fwd(L.ptr(sc), L.ptr(mk), L.ptr(lb), L.ptr(ww), L.ptr(one), T, K, L.stream_ptr()), 'tap_bce_fwd')
    for buf in (a, b):
        L.check(lib.echr_tap_bce_fwd_ws(L.ptr(sc), L.ptr(mk), L.ptr(lb), L.ptr(ww), L.ptr(buf[:1]), L.ptr(buf[1:]), T, K, L.stream_ptr()), 'tap_bce_fwd_ws')
    L.check(lib.echr_tap_bce_bwd(L.ptr(sc), L.ptr(mk), L.ptr(lb), L.ptr(ww), L.ptr(gl), L.ptr(gs), T, K, L.stream_ptr()), 'tap_bce_bwd')
    torch.cuda.synchronize()
    return one.cpu().numpy()[0], a.cpu().numpy()[0], b.cpu().numpy()[0], gs.cpu().numpy()


def _batch_entries(inp):
    """echr_tap_bce_fwd_batch / _bwd_batch as tests/test_gpu_joint_batch.py::_bce_gpu drives them: (per-video losses, their sum, d scores)."""
    L, lib = _lib()
    dev = _dev()
    ro = inp['ro']
    V, (T, K) = len(ro) - 1, inp['scores'].shape
    sc, mk, lb, ww = _upload(inp)
    ro_dev = torch.tensor(ro, dtype=torch.int32, device=dev)
    per, total, part = torch.zeros(V, device=dev), torch.zeros(1, device=dev), torch.zeros(64 * V, device=dev)
    gl, gs = torch.full((1,), P.G_LOSS, device=dev), torch.full((T, K), float('nan'), device=dev)
    ld = K if inp['per_video'] else 0
    L.check(lib.echr_tap_bce_fwd_batch(L.ptr(sc), L.ptr(mk), L.ptr(lb), L.ptr(ww), ld, L.ptr(ro_dev, torch.int32), V, K, L.ptr(per), L.ptr(total),
                                       L.ptr(part), L.stream_ptr()), 'tap_bce_fwd_batch')
    L.check(lib.echr_tap_bce_bwd_batch(L.ptr(sc), L.ptr(mk), L.ptr(lb), L.ptr(ww), ld, L.ptr(ro_dev, torch.int32), V, K, T, L.ptr(gl), L.ptr(gs),
                                       L.stream_ptr()), 'tap_bce_bwd_batch')
    torch.cuda.synchronize()
    return per.cpu().numpy(), total.cpu().numpy()[0], gs.cpu().numpy()


def _autograd(inp, batch):
    """TAPModelCriterion.forward / forward_batch behind autograd: (loss, d (G_LOSS * loss) / d scores)."""
    from echr_amd.misc.utils import TAPModelCriterion
    s = torch.from_numpy(inp['scores']).to(_dev()).requires_grad_(True)
    mk, lb = torch.from_numpy(inp['masks']), torch.from_numpy(inp['labels'])
    if batch:
        w1 = [torch.from_numpy(w) for w in inp['w1']] if inp['per_video'] else torch.from_numpy(inp['w1'][0])
        loss, _ = TAPModelCriterion().forward_batch(s, mk, lb, w1, inp['ro'])
    else:
        loss = TAPModelCriterion()(s, mk, lb, torch.from_numpy(inp['w1'][0]))
    (P.G_LOSS * loss).backward()
    torch.cuda.synchronize()
    return float(loss.detach()), s.grad.cpu().numpy()


def _loss_close(name, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref).max()
    print('%-40s %.3e (relative to %.6g)' % (name, err / max(np.abs(ref).max(), 1e-300), np.abs(ref).max()))
    assert np.isfinite(got).all() and err <= TOL_LOSS * np.abs(ref).max(), (name, got, ref)


def _grad_elems(name, got, ref, inp):
    """Every element of d scores; on a miss the message names the worst element's score, label and mask."""
    assert np.isfinite(got).all(), name
    ratio = np.abs(got.astype(np.float64) - ref) / (np.abs(ref) + 1e-30 / P.TOL_ELEM)
    i = int(np.argmax(ratio))
    at = 'score %.9g label %g mask %g: got %.9g, float64 %.9g' % (inp['scores'].reshape(-1)[i], inp['labels'].reshape(-1)[i], inp['masks'].reshape(-1)[i],
                                                                 got.reshape(-1)[i], ref.reshape(-1)[i])
    print('%-40s worst element ratio %.3e (%s)' % (name, ratio.max(), at))
    assert ratio.max() <= P.TOL_ELEM, (name, float(ratio.max()), at)


def _check_single(inp, ref):
    losses, g = ref
    one, ws, ws2, gs = _single_entries(inp)
    _loss_close('echr_tap_bce_fwd', one, losses[0])
    _loss_close('echr_tap_bce_fwd_ws', ws, losses[0])
    _grad_elems('echr_tap_bce_bwd', gs, g, inp)
    assert ws.tobytes() == ws2.tobytes()          # two runs of the two-launch form: the same bits
    per, total, gb = _batch_entries(inp)
    assert per[0].tobytes() == ws.tobytes() == total.tobytes()          # a one-video batch IS echr_tap_bce_fwd_ws
    _grad_elems('echr_tap_bce_bwd_batch, V = 1', gb, g, inp)
    loss, ga = _autograd(inp, False)
    assert np.float32(loss).tobytes() == ws.tobytes()
    _grad_elems('TAPModelCriterion.forward', ga, g, inp)


@pytest.mark.parametrize('T,K', SIZE_CASES)
def test_criterion_on_planted_scores_at_its_size_boundaries(T, K):
    """BCE_PARTS = 64 partial ranges of ceil(n / 64) elements, 256 threads x 4 per pass; the one-workgroup form takes 4096 per pass.  n = 1 and 3
    (almost every range empty), 63 / 64 / 65, 4096 / 4097, 65536 (each range exactly one pass), 65792 (one pass plus 4).  All 48 planted elements
    (cut to n) spread over the matrix."""
    inp, ref = _bce_case((T,), K)
    _check_single(inp, ref)


PLANT_ON = [i for i, (_, _, m) in enumerate(P.PLANT) if m == 1.0]


@pytest.mark.parametrize('i', PLANT_ON, ids=['%.9g-label%d' % (P.PLANT[i][0], P.PLANT[i][1]) for i in PLANT_ON])
def test_criterion_on_one_planted_score(i):
    """T = 1, K = 3, every mask 1: (the planted score, 0.3 under label 0, 0.7 under label 1) -- the planted value's own term is visible in the
    loss, not buried under the 100 w terms of the others."""
    inp = dict(P.bce_inputs((1,), 3, plant=i))
    inp['scores'][0, 1:], inp['labels'][0, 1:], inp['masks'][0, :] = (0.3, 0.7), (0.0, 1.0), 1.0
    _check_single(inp, P.bce_reference(inp))


@pytest.mark.parametrize('per_video', [False, True])
@pytest.mark.parametrize('K,lengths', BATCH_CASES)
def test_batched_criterion_on_planted_scores(K, lengths, per_video):
    """tap_bce_bwd_batch_kernel locates its video by a scan from the workgroup's first row.  K = 1: four videos inside the first 256-element
    block, a boundary at row 259, three rows behind a block edge; K = 3: rows straddle block edges; K = 16: the case of test_gpu_joint_batch;
    K = 300: a block is less than one row.  Per-video losses, their sum and d scores (video v divides by its own T_v)."""
    inp, (losses, g) = _bce_case(lengths, K, per_video)
    per, total, gs = _batch_entries(inp)
    _loss_close('per-video losses', per, losses)
    _loss_close('sum', total, losses.sum())
    _grad_elems('echr_tap_bce_bwd_batch', gs, g, inp)
    loss, ga = _autograd(inp, True)
    assert np.float32(loss).tobytes() == total.tobytes()
    _grad_elems('TAPModelCriterion.forward_batch', ga, g, inp)


# ---- 2. the encoder -----------------------------------------------------------------------------------------------------------------
# e_ref (tap absolute, scores absolute, loss relative, worst gradient tensor relative to its max-norm): float32 oracle vs float64 oracle on the
# CPU, the largest of eval / train mode and one video / batch (tools/parity_report.py --sst reprints the lines)
E_REF = {
    'gates_sat': (3.0e-6, 3.7e-6, 3.3e-6, 2.7e-6),          # scores.weight
    'drift': (1.5e-5, 2.9e-6, 3.3e-6, 1.8e-5),              # rnn.weight_hh_l1
    'bce_chain': (3.0e-6, 2.5e-6, 1.8e-5, 2.5e-6),          # rnn.weight_ih_l0
    'small_h': (6.3e-7, 8.6e-7, 2.0e-6, 3.1e-6),            # rnn.weight_hh_l0
}


def gates(name):
    e = E_REF[name]
    g = (max(TOL_OUT, 4 * e[0]), max(TOL_OUT, 4 * e[1]), max(TOL_LOSS, 4 * e[2]), max(TOL_GRAD, 4 * e[3]))
    assert max(g) <= CONTRACT, (name, g)
    return g


def _config(name, value):
    L, lib = _lib()
    L.check(lib.echr_config_set(name, value), 'config_set')


def gpu_run(name, train, batch, crit='forward_batch'):
    """The variant on the GPU: dict(tap, scores, grads, loss -- of bce_chain the criterion's part, as the reference reports it).  One video: SST.forward (+ TAPModelCriterion.forward for bce_chain); a batch:
    SST.forward_batch (+ TAPModelCriterion.forward_batch, or crit='per_video': misc.utils.tap_criterion_batch's loop over the videos)."""
    from echr_amd.misc import utils
    spec, params, inp = P.make_variant(name)
    r0, ro = P.rows(name, batch)
    sl = slice(r0, r0 + ro[-1])
    dev = _dev()
    m = R.module(params, spec['D'], spec['H'], spec['K'], train)
    x, wt, ws = (torch.from_numpy(inp[k][sl]).to(dev) for k in ('x', 'wt', 'ws'))
    tap, sc = m.forward_batch(x, ro) if batch else m(x)
    if spec['loss'] == 'sums':
        loss = rep = (tap * wt).sum() + (sc * ws).sum()
    else:
        mk, lb, w1 = torch.from_numpy(inp['masks'][sl]), torch.from_numpy(inp['labels'][sl]), torch.from_numpy(inp['w1'])
        C = utils.TAPModelCriterion()
        if not batch:
            l = C(sc, mk, lb, w1)
        elif crit == 'forward_batch':
            l, _ = C.forward_batch(sc, mk, lb, w1, ro)
        else:
            l, _ = utils.tap_criterion_batch(C, sc, mk.to(dev), lb.to(dev), w1.to(dev), ro)
        loss, rep = l + P.TAP_WEIGHT * (tap * wt).sum(), l
    loss.backward()
    torch.cuda.synchronize()
    return dict(tap=tap.detach().cpu().numpy(), scores=sc.detach().cpu().numpy(), loss=float(rep.detach()),
                grads={k: p.grad.cpu().numpy() for k, p in m.named_parameters()})


def _check_encoder(name, got, ref, what):
    t_tap, t_sc, t_loss, t_grad = gates(name)
    assert np.isfinite(got['tap']).all() and np.isfinite(got['scores']).all(), what
    e = P.errors(got, ref)
    print('%s %s: tap %.2e (gate %.1e) scores %.2e (gate %.1e) loss %.2e worst gradient %.2e (%s, gate %.1e)'
          % (name, what, e[0], t_tap, e[1], t_sc, e[2], e[3], e[4], t_grad))
    assert e[0] < t_tap and e[1] < t_sc, (what, e)
    if P.VARIANTS[name]['loss'] == 'bce':
        assert e[2] < t_loss, (what, got['loss'], ref['loss'])
    for k, g in ref['grads'].items():
        assert U.grad_close(k, got['grads'][k], g, t_grad), (what, k, U.relerr(got['grads'][k], g))


def _route(name, train, batch, persist, crit='forward_batch'):
    _, lib = _lib()
    try:
        _config(b'sst_persist', persist)
        got = gpu_run(name, train, batch, crit)
    finally:
        _config(b'sst_persist', 1)
    assert lib.echr_check_async() == 0, lib.echr_last_error()
    return got


@pytest.mark.parametrize('persist', [1, 0])
@pytest.mark.parametrize('batch', [False, True])
@pytest.mark.parametrize('train', [False, True])
@pytest.mark.parametrize('name', ['gates_sat', 'drift', 'bce_chain'])
def test_encoder_variant_vs_float64_oracle(name, train, batch, persist):
    """H = 512: the persistent recurrences (fast_sigmoid / fast_tanh on hardware exp and rcp) and the launch-per-step wavefront (tanhf), on one
    video and on the variant's batch, inter-layer dropout 0.5 in train mode; bce_chain's batch through TAPModelCriterion.forward_batch AND through
    the per-video loop of tap_criterion_batch."""
    ref = P.oracle64(name, train, batch)
    what = 'persist=%d batch=%d train=%d' % (persist, batch, train)
    _check_encoder(name, _route(name, train, batch, persist), ref, what)
    if batch and name == 'bce_chain':
        _check_encoder(name, _route(name, train, batch, persist, 'per_video'), ref, what + ' per-video criterion')


@pytest.mark.parametrize('batch', [False, True])
@pytest.mark.parametrize('train', [False, True])
def test_small_encoder_variant_vs_float64_oracle(train, batch):
    """D = 20, H = 24, K = 8 at the scales of gates_sat: the wavefront is the only route of a model with H != 512."""
    _check_encoder('small_h', _route('small_h', train, batch, 0), P.oracle64('small_h', train, batch), 'batch=%d train=%d' % (batch, train))


# ---- 3. the selection ---------------------------------------------------------------------------------------------------------------
T_SEL, K_SEL = 40, 32          # 1280 cells: more than one 1024-cell compaction chunk


def _grid():
    g = P.saturated_grid(T_SEL, K_SEL)
    c = P.class_counts(g)
    assert min(c) >= 8, c          # every class is there, with heavy repetition
    return g, c


def _topNs(c):
    """topN inside the tie class of 1.0, on its last element, inside the class of its predecessor (the next class differs from it in the key's
    last bit), on its last element, inside the class after, inside the denormal's class, and >= the number of cells."""
    d = P.I_DENORMAL
    return [c[0] // 2, c[0], c[0] + c[1] // 2, c[0] + c[1], c[0] + c[1] + c[2] // 2, sum(c[:d]) + c[d] // 2, T_SEL * K_SEL, 2000]


def _single_threshold(scores, mask, topN, thres):
    from echr_amd import eval_utils as EU
    ind, feat, conf = EU.top_proposals_device(torch.from_numpy(scores).cuda(), mask, topN, thres)
    return ind.cpu().numpy(), feat.cpu().numpy(), conf.cpu().numpy()


@pytest.mark.parametrize('thres', [0.0, float(P.PRED), 1.0], ids=['thres0', 'thres_pred', 'thres1'])
def test_threshold_selection_on_saturated_scores(thres):
    """val_thres 0.0, exactly 1 - 2^-24 (ties AT the threshold stay) and 1.0, at every topN of _topNs: the single-video entry, a one-video batch
    with the explicit causal mask and with NULL, and a batch of three with the grid in the middle."""
    grid, c = _grid()
    mask = PB.causal_mask([T_SEL], K_SEL)
    lengths = (7, T_SEL, 24)
    ro3 = PB.offsets(lengths)
    batch3 = np.concatenate([P.saturated_grid(7, K_SEL, 1), grid, P.saturated_grid(24, K_SEL, 2)], 0)
    for topN in _topNs(c):
        want = PB.select(grid, [0, T_SEL], topN, thres)
        if thres == 0.0 and topN == c[0] // 2:
            assert want['count'][0] == c[0] > topN          # the whole tie class of 1.0 comes back
        if thres == 0.0 and topN == c[0] + c[1] // 2:
            assert want['count'][0] == c[0] + c[1]          # ... of 1 - 2^-24, and nothing of 1 - 2^-23
        if thres == 0.0 and topN == sum(c[:P.I_DENORMAL]) + c[P.I_DENORMAL] // 2:
            assert want['count'][0] == sum(c[:P.I_DENORMAL + 1])          # the denormal's class, and not the zeros behind it
        if thres == float(P.PRED):
            assert want['count'][0] == (c[0] if topN <= c[0] else c[0] + c[1])
        ind, feat, conf = _single_threshold(grid, mask, topN, thres)
        assert np.array_equal(ind, want['ind']) and np.array_equal(feat, want['feat']), topN
        assert np.array_equal(conf.view(np.uint32), want['conf'].view(np.uint32)), topN
        assert_same(_as32(run_gpu(grid, [0, T_SEL], topN, thres, mask=mask)), _as32(want))
        assert_same(_as32(run_gpu(grid, [0, T_SEL], topN, thres)), _as32(want))
        want3 = _as32(PB.select(batch3, ro3, topN, thres))
        assert_same(_as32(run_gpu(batch3, ro3, topN, thres, mask=PB.causal_mask(lengths, K_SEL))), want3)
        assert_same(_as32(run_gpu(batch3, ro3, topN, thres)), want3)


def _as32(d):
    """The reference's int64 lists as the int32 the kernels write (assert_same compares dtype and values)."""
    return {k: (v.astype(np.int32) if v.dtype == np.int64 else v) for k, v in d.items()}


@pytest.mark.parametrize('T,K', [(33, 31), (32, 32), (41, 25)])
def test_threshold_selection_of_every_causal_cell_around_one_compaction_chunk(T, K):
    """T K = 1023, 1024 and 1025 cells, topN beyond them, val_thres 0: every causal cell (the zeros and the denormals too), in order."""
    grid = P.saturated_grid(T, K)
    want = _as32(PB.select(grid, [0, T], 100000, 0.0))
    assert want['count'][0] == sum(min(n + 1, K) for n in range(T))
    assert_same(_as32(run_gpu(grid, [0, T], 100000, 0.0, mask=PB.causal_mask([T], K))), want)
    assert_same(_as32(run_gpu(grid, [0, T], 100000, 0.0)), want)
    ind, feat, conf = _single_threshold(grid, PB.causal_mask([T], K), 100000, 0.0)
    assert np.array_equal(ind, want['ind']) and np.array_equal(feat, want['feat']) and np.array_equal(conf.view(np.uint32), want['conf'].view(np.uint32))


@pytest.mark.parametrize('topN', [12, 2000])
@pytest.mark.parametrize('overlap', [0.5, 0.95])
@pytest.mark.parametrize('kind', ['ones', 'mixed'])
def test_nms_on_saturated_scores(kind, overlap, topN):
    """A grid of all 1.0 -- every pick is decided by the tie rule (the later candidate) -- and the mixed grid: the single-video entry and a batch
    of three with the grid in the middle."""
    from echr_amd import eval_utils as EU
    grid = np.ones((T_SEL, K_SEL), np.float32) if kind == 'ones' else _grid()[0]
    want = _as32(PB.select(grid, [0, T_SEL], topN, overlap=overlap))
    assert want['count'][0] > 1
    _, props, _, _, conf = EU.gettop1000_nms(torch.from_numpy(grid).cuda(), None, [], 1.0, lambda s, e, n, d: 0, overlap=overlap, topN=topN)
    assert np.array_equal(props, want['feat']) and np.array_equal(conf.astype(np.float32).view(np.uint32), want['conf'].view(np.uint32))
    assert_same(_as32(run_gpu(grid, [0, T_SEL], topN, overlap=overlap)), want)
    lengths = (7, T_SEL, 24)
    batch3 = np.concatenate([P.saturated_grid(7, K_SEL, 1), grid, P.saturated_grid(24, K_SEL, 2)], 0)
    assert_same(_as32(run_gpu(batch3, PB.offsets(lengths), topN, overlap=overlap)), _as32(PB.select(batch3, PB.offsets(lengths), topN, overlap=overlap)))

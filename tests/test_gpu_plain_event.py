"""The event contexts without the event encoder, 'EC' and 'EH' (CaptionGenerator.py:106-137), on the GPU (-m gpu): the module path, the one-call
step (echr_train_step_args.event_direct) on its single-video and batch entries, d tap_feats, and the other entries (beam search,
self-critical training, the joint iteration, caption_videos) -- against the reference's own fixtures (tests/golden/case_ec.npz / case_eh.npz),
the oracle composition (tests/plain_event_ref.py) and the single-video calls.

Gates: the project's own (tests/test_gpu_parity.py:20-22) -- log-probs 2e-5 absolute, loss 1e-5 relative, every gradient tensor 1e-5 of its
max-norm, index outputs bit-exact.  Two HIP results compared with each other (batch against single-video calls, one-call against module
path) each carry that error: twice the gate, as tests/test_gpu_vbatch.py and tests/test_gpu_clip_batch.py do; the one-call step against the
autograd path is held to the limits of test_gpu_parity.test_fused_train_step_equals_autograd_path."""
import functools

import numpy as np
import pytest
import torch

from echr_amd import synth
from oracle import summary as SM
from tests import joint_batch_ref as J
from tests import plain_event_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

TOL_LOGP, TOL_LOSS, TOL_GRAD = 2e-5, 1e-5, 1e-5          # tests/test_gpu_parity.py:20-22
UNUSED = ('lm_model.core.fusion_layer.weight', 'lm_model.core.fusion_layer.bias')
KEYS = ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')


def _dev():
    return torch.device('cuda')


def _feats(vid):
    return tuple(torch.from_numpy(np.ascontiguousarray(vid[k])).to(_dev()) for k in ('tap', 'c3d', 'lda'))


def _labels(vid):
    return torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])


def _grads(m):
    return {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}


def _check_grads(grads, ref, tol):
    for k, g in ref.items():
        if g is None:
            assert k in UNUSED and (grads[k] is None or not np.any(grads[k])), k
        else:
            assert U.grad_close(k, grads[k], g, tol), (k, U.relerr(grads[k], g))


def _check_tap(got, ref, tol):
    assert np.abs(got - ref).max() <= tol * max(float(np.abs(ref).max()), U.GRAD_FLOOR) + 1e-9, U.relerr(got, ref, U.GRAD_FLOOR)


def _fused(opt, params, train_mode=True, lr=1e-3, clip=100.0):
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    m = U.build_gpu_model(opt, params, train_mode)
    o = ClampAdam(m.parameters(), lr=lr, arena=m.build_arena())
    return m, o, FusedTrainStep(m, o, grad_clip=clip)


@functools.lru_cache(maxsize=None)
def _case(case):
    return synth.make_case(case)


@functools.lru_cache(maxsize=None)
def _ref(case, train_mode):
    return R.run(*_case(case), train_mode)


# ---- 1. the module path on the reference's cases ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['ec', 'eh'])
@pytest.mark.parametrize('train_mode', [False, True])
def test_forward_train_matches_oracle_and_reference(case, train_mode):
    """forward(mode='train'): every log-prob, the loss and every parameter gradient against the oracle composition, and the summaries of the
    reference's own run (the checks test_gpu_parity.test_full_path_vs_reference_golden applies to case_er1)."""
    opt, params, vid = _case(case)
    pred, loss, grads, m = U.run_gpu(opt, params, vid, train_mode)
    assert not hasattr(m, 'fusion_model') and set(grads) == set(params)
    rpred, rloss, rgrads, _, _ = _ref(case, train_mode)
    assert pred.shape == rpred.shape and np.abs(pred - rpred).max() < TOL_LOGP, np.abs(pred - rpred).max()
    assert abs(loss - rloss) < TOL_LOSS * abs(rloss)
    _check_grads(grads, rgrads, TOL_GRAD)
    g, mode = U.gold('case_%s.npz' % case), 'train' if train_mode else 'eval'
    assert abs(loss - float(g[mode + '|loss'])) < TOL_LOSS * abs(float(g[mode + '|loss']))
    s = SM.summarize_logp(pred)
    assert np.abs(s['slice'] - g[mode + '|logp|slice']).max() < TOL_LOGP and np.abs(s['top1'] - g[mode + '|logp|top1']).max() < TOL_LOGP
    safe = g[mode + '|logp|margin'] > 1e-4
    assert np.array_equal(s['argmax'][safe], g[mode + '|logp|argmax'][safe])
    for key, v in SM.summarize_grads(grads).items():
        ref, name = g[mode + '|grad|' + key], key.split('|')[0]
        if name in U.NOISE_ONLY:
            assert np.abs(np.asarray(v)).max() < 1e-6 and np.abs(np.asarray(ref)).max() < 1e-6, key
            continue
        scale = max(float(g[mode + '|grad|' + name + '|linf']), U.GRAD_FLOOR)
        if key.endswith('|l2') or key.endswith('|linf'):
            assert abs(float(v) - float(ref)) < TOL_GRAD * max(abs(float(ref)), U.GRAD_FLOOR), key
        else:
            assert np.abs(v - ref).max() < TOL_GRAD * scale, (key, np.abs(v - ref).max() / scale)


@pytest.mark.parametrize('case', ['ec', 'eh'])
def test_greedy_decode_and_event_context_match_reference(case):
    opt, params, vid = _case(case)
    g = U.gold('case_%s.npz' % case)
    m = U.build_gpu_model(opt, params, False)
    tap, c3d, lda = _feats(vid)
    with torch.no_grad():
        seq, lp = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
        ev = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'])
    assert seq.dtype == torch.int64 and np.array_equal(seq.cpu().numpy(), g['sample|seq'])
    assert np.abs(lp.cpu().numpy() - g['sample|logp']).max() < TOL_LOGP
    assert tuple(ev.shape) == g['event_context'].shape and np.abs(ev.cpu().numpy() - g['event_context']).max() < 1e-6


# ---- 2. the one-call step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['ec', 'eh'])
@pytest.mark.parametrize('fixed', [False, True], ids=['atomic', 'fixed_order'])
def test_fused_train_step_equals_autograd_path(case, fixed):
    """step=False: loss and gradients against the autograd path (and the oracle); then ONE update from identical states against the autograd
    path + ClampAdam -- the limits of test_gpu_parity.test_fused_train_step_equals_autograd_path's first step."""
    import echr_amd
    from echr_amd.misc.utils import LanguageModelCriterion, clip_gradient
    opt, params, vid = _case(case)
    tap, c3d, lda = _feats(vid)
    labels, masks = _labels(vid)
    tgt, msk = labels[:, 1:].to(_dev()), masks[:, 1:].to(_dev())
    lr = 1e-3
    echr_amd.set_deterministic(fixed)
    try:
        ma, oa, _ = _fused(opt, params, lr=lr, clip=0.05)
        mb, ob, fb = _fused(opt, params, lr=lr, clip=0.05)
        assert fb.a.event_direct == {'ec': 1, 'eh': 2}[case] and not fb.a.tsrm.w_emb and not fb.a.tsrm_g.g_w_emb

        def autograd_iteration(step):
            oa.zero_grad()
            loss = LanguageModelCriterion()(ma(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train'), tgt, msk)
            loss.backward()
            clip_gradient(oa, 0.05)
            if step:
                oa.step()
            return float(loss)
        la = autograd_iteration(False)
        lb = float(fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], step=False))
        assert abs(la - lb) < 1e-6 * abs(la), (la, lb)
        assert abs(lb - _ref(case, True)[1]) < TOL_LOSS * abs(lb)
        assert 0 < fb.last_active_rows < labels.shape[0] * (labels.shape[1] - 1)
        for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
            assert (pa.grad is None) == (pb.grad is None) == (k in UNUSED), k
            if pa.grad is not None:
                assert U.grad_close(k, pb.grad.cpu().numpy(), pa.grad.cpu().numpy(), 2e-5), (k, U.relerr(pb.grad.cpu().numpy(), pa.grad.cpu().numpy()))
        _check_grads(_grads(mb), _ref(case, True)[2], TOL_GRAD)
        # one update from identical states (both dropout counters advanced once)
        la = autograd_iteration(True)
        lb = float(fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:]))
        assert abs(la - lb) < 1e-6 * abs(la), (la, lb)
        assert ob._flat['step'] == 1 and oa._flat['step'] == 1
        for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
            dp = (pa.detach() - pb.detach()).abs()
            assert float(dp.max()) <= 2.01 * lr, k
            if pa.grad is not None and k not in U.NOISE_ONLY:
                gg = pa.grad.abs()
                solid = gg > 1e-4 * gg.max()
                if bool(solid.any()):
                    assert float(dp[solid].max()) < 0.02 * lr, (k, float(dp[solid].max()))
            if k in UNUSED:
                assert np.array_equal(pb.detach().cpu().numpy(), params[k]), k
        # validation loss, and the two-call form is refused with a message instead of running the encoder's prepare half
        vb = float(fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], tgt, msk, forward_only=True))
        assert np.isfinite(vb)
        with pytest.raises(NotImplementedError, match='prepare'):
            fb.prepare(c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:])
    finally:
        echr_amd.set_deterministic(False)


# ---- 3. d tap_feats where the scatter can go wrong ----------------------------------------------------------------------------------------
SOI5 = np.array([[0, 6], [2, 6], [10, 11], [8, 20], [15, 24]], np.int64)          # events 0 and 1 end on segment 5; event 2 is one segment long


@functools.lru_cache(maxsize=None)
def _anchor_case(et):
    opt = synth.default_opt(event_context_type=et, CG_vocab_size=300, CG_seq_length=4)
    vid = synth.make_video(5, 12, 6, 301, seed=76, T_v=24)
    vid['soi'] = SOI5.copy()
    vid['ind'] = (SOI5[:, 1] - 1).astype(np.int64)
    params = synth.make_params(opt, 0)
    return opt, params, vid, R.run(opt, params, vid, True)


@pytest.mark.parametrize('fixed', [False, True], ids=['atomic', 'fixed_order'])
def test_d_tap_of_shared_anchors(fixed):
    """'EH', ECHR widths, T_v = 24, five events of which two share their anchor row (the scatter must add) and one is a single segment: d tap
    from the autograd path and from tap_grad of the one-call step against the oracle; with 'VL' every row that is no event's anchor is
    exactly zero.  Both forms of the scatter (atomic / fixed order)."""
    import echr_amd
    from echr_amd.misc.utils import LanguageModelCriterion
    opt, params, vid, ref = _anchor_case('EH')
    assert len(set(vid['ind'].tolist())) == 4 and (SOI5[:, 1] - SOI5[:, 0]).min() == 1 and vid['tap'].shape == (24, 512)
    want = ref[3]
    anchors = sorted(set(int(i) for i in vid['ind']))
    assert np.flatnonzero(np.abs(want).max(1) > 0).tolist() == anchors
    tap, c3d, lda = _feats(vid)
    labels, masks = _labels(vid)
    echr_amd.set_deterministic(fixed)
    try:
        m = U.build_gpu_model(opt, params, True)
        leaf = tap.clone().requires_grad_(True)
        pred = m(leaf, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
        LanguageModelCriterion()(pred, labels[:, 1:].to(_dev()), masks[:, 1:].to(_dev())).backward()
        assert np.abs(pred.detach().cpu().numpy() - ref[0]).max() < TOL_LOGP
        m2, _, f = _fused(opt, params)
        g_tap = torch.zeros_like(tap)
        loss = float(f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], step=False, tap_grad=g_tap))
        torch.cuda.synchronize()
    finally:
        echr_amd.set_deterministic(False)
    assert abs(loss - ref[1]) < TOL_LOSS * abs(ref[1])
    _check_grads(_grads(m2), ref[2], TOL_GRAD)
    rest = np.setdiff1d(np.arange(24), anchors)
    for got in (leaf.grad.cpu().numpy(), g_tap.cpu().numpy()):
        _check_tap(got, want, TOL_GRAD)
        assert not got[rest].any() and all(got[a].any() for a in anchors)


def test_d_tap_of_pooled_rows_is_zero():
    """'EC' with 'VL' and 'CC' reads no tap row: d tap is exactly zero on both paths."""
    from echr_amd.misc.utils import LanguageModelCriterion
    opt, params, vid, ref = _anchor_case('EC')
    assert not ref[3].any()
    tap, c3d, lda = _feats(vid)
    labels, masks = _labels(vid)
    m = U.build_gpu_model(opt, params, True)
    leaf = tap.clone().requires_grad_(True)
    pred = m(leaf, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    LanguageModelCriterion()(pred, labels[:, 1:].to(_dev()), masks[:, 1:].to(_dev())).backward()
    assert np.abs(pred.detach().cpu().numpy() - ref[0]).max() < TOL_LOGP
    assert leaf.grad is None or not bool(leaf.grad.any())
    m2, _, f = _fused(opt, params)
    g_tap = torch.zeros_like(tap)
    loss = float(f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], step=False, tap_grad=g_tap))
    assert abs(loss - ref[1]) < TOL_LOSS * abs(ref[1]) and not bool(g_tap.any())
    _check_grads(_grads(m2), ref[2], TOL_GRAD)


# ---- 4. batches ---------------------------------------------------------------------------------------------------------------------------
FULL = dict(event_context_type='EH', video_context_type='VLVH', clip_context_type='CC+CH', CG_init_feats_type='VE')
PLAIN_EC = dict(event_context_type='EC', video_context_type='VL', clip_context_type='CC', CG_init_feats_type='')
PLAIN_EH = dict(event_context_type='EH', video_context_type='VL', clip_context_type='CC', CG_init_feats_type='')


@functools.lru_cache(maxsize=None)
def _vb(form):
    """Three videos of 1, 4 and 2 events, T_v = 16, 40, 24, ragged label widths."""
    opt = synth.default_opt(CG_vocab_size=300, CG_seq_length=7, K=J.K, **dict(form))
    vids = [synth.make_video(N, A, L, 301, seed=2400 + i, T_v=T) for i, (N, A, L, T) in enumerate(((1, 10, 7, 16), (4, 24, 9, 40), (2, 12, 6, 24)))]
    assert [len(v['soi']) for v in vids] == [1, 4, 2] and [v['T_v'] for v in vids] == [16, 40, 24]
    return opt, synth.make_params(opt, 0), vids


@functools.lru_cache(maxsize=None)
def _vb_ref(form, train_mode):
    return R.run_batch(*_vb(form), train_mode)


def _batch(opt, vids, tap_leaves=False, labels=True):
    from echr_amd.batch import VideoBatch
    taps = [torch.from_numpy(v['tap']).to(_dev()).requires_grad_(tap_leaves) for v in vids]
    keys = ('c3d', 'lda', 'ind', 'soi') + (('labels', 'masks') if labels else ())
    b = VideoBatch.from_videos([dict({k: v[k] for k in keys}, tap=t) for v, t in zip(vids, taps)], device=_dev(),
                               clip_context_type=opt.clip_context_type, CG_init_feats_type=opt.CG_init_feats_type)
    return b, taps


def _FULL():
    return tuple(sorted(FULL.items()))


def test_forward_batch_rows_equal_the_single_video_calls():
    """'EH' with 'VLVH', 'CC+CH' and the initial state 'VE': the rows of forward_batch('train') / ('eval') against forward() per video (two
    HIP results), the teacher-forced rows also against the oracle per video."""
    opt, params, vids = _vb(_FULL())
    ref = _vb_ref(_FULL(), False)
    m = U.build_gpu_model(opt, params, False)
    b, _ = _batch(opt, vids)
    assert b.clip_parts == 3
    with torch.no_grad():
        logp = m.forward_batch(b, mode='train').cpu().numpy()
        seq, slp = m.forward_batch(b, mode='eval', event_group_rows=4)          # (accepted, no effect: there is no encoder pair work to bound)
        seq2, _ = m.forward_batch(b, mode='eval')
        assert torch.equal(seq, seq2)
        seq, slp = seq.cpu().numpy(), slp.cpu().numpy()
        for v, s in enumerate(b.event_slices):
            d = b.video(v)
            one = m(d['tap'], d['c3d'], d['lda'], d['labels'], d['ind'], d['soi'], mode='train').cpu().numpy()
            assert np.abs(logp[s, :one.shape[1]] - one).max() <= 2 * TOL_LOGP, v
            assert np.abs(logp[s, :one.shape[1]] - ref['logp'][v]).max() < TOL_LOGP, v
            s1, l1 = m(d['tap'], d['c3d'], d['lda'], [], d['ind'], d['soi'], mode='eval')
            w = 0 if isinstance(s1, list) else s1.shape[1]
            if w:
                assert np.array_equal(seq[s, :w], s1.cpu().numpy()) and np.abs(slp[s, :w] - l1.cpu().numpy()).max() <= 2 * TOL_LOGP, v
            assert not seq[s, w:].any(), v


@pytest.mark.parametrize('train_mode', [False, True])
def test_module_batch_gradients_match_the_oracle(train_mode):
    """forward_batch('train') + the per-video criterion + backward, every video's tap_feats a leaf: all four routes into d tap are active
    (anchors, the 'VH' mean, the attended rows, init_linear)."""
    from echr_amd.misc.utils import LanguageModelCriterion
    opt, params, vids = _vb(_FULL())
    ref = _vb_ref(_FULL(), train_mode)
    m = U.build_gpu_model(opt, params, train_mode)
    m.build_arena()
    b, taps = _batch(opt, vids, True)
    total, per = b.criterion(LanguageModelCriterion(), m.forward_batch(b, mode='train'))
    total.backward()
    assert abs(float(total) - ref['loss']) < TOL_LOSS * abs(ref['loss'])
    assert np.abs(per.detach().cpu().numpy() - ref['losses']).max() < TOL_LOSS * np.abs(ref['losses']).max()
    _check_grads(_grads(m), ref['grads'], TOL_GRAD)
    for t, want in zip(taps, ref['g_tap']):
        _check_tap(t.grad.cpu().numpy(), want, TOL_GRAD)
        assert np.count_nonzero(np.abs(want).max(1)) == len(want)          # (the 'VH' mean reaches every row)


def _per_video_steps(opt, params, vids, train_mode=False):
    """The sum of the per-video FusedTrainStep(step=False, tap_grad=) calls: (loss, per-video losses, flat gradient, [d tap per video])."""
    m, o, f = _fused(opt, params, train_mode, clip=None)
    flat, per, g_taps = torch.zeros_like(f.arena.flat_g), [], []
    for vid in vids:
        tap, c3d, lda = _feats(vid)
        labels, masks = _labels(vid)
        g = torch.zeros_like(tap)
        per.append(float(f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], step=False, tap_grad=g)))
        flat += f.arena.flat_g
        g_taps.append(g.cpu().numpy())
    return float(np.sum(per)), np.asarray(per), flat, g_taps, m


def _check_flat(m, ar, got, want, tol):
    for i, (k, p) in enumerate(m.named_parameters()):
        lo, n = ar.offsets[i], p.numel()
        a, r = got[lo:lo + n], want[lo:lo + n]
        if k in UNUSED:
            assert not bool(a.any()) and not bool(r.any()), k
        elif k in U.NOISE_ONLY:
            assert float(a.abs().max()) < 1e-6, k
        else:
            assert float((a - r).abs().max()) <= tol * max(float(r.abs().max()), U.GRAD_FLOOR) + 1e-9, (k, float((a - r).abs().max()), float(r.abs().max()))


@pytest.mark.parametrize('fixed', [False, True], ids=['atomic', 'fixed_order'])
def test_fused_batch_with_tap_gradient_equals_the_sum_of_the_per_video_steps(fixed):
    """echr_train_step_batch_clip with g_tap on the 'EH' / 'VLVH' / 'CC+CH' / 'VE' batch against the per-video echr_train_step_clip calls
    (two HIP results: twice the gate) and against the oracle (the gate)."""
    import echr_amd
    opt, params, vids = _vb(_FULL())
    ref = _vb_ref(_FULL(), False)
    echr_amd.set_deterministic(fixed)
    try:
        total, per1, flat1, g_taps, _ = _per_video_steps(opt, params, vids)
        m, o, f = _fused(opt, params, False, clip=None)
        b, _ = _batch(opt, vids)
        g_tap = torch.zeros_like(b.tap)
        per = torch.zeros(b.n_videos, device=_dev())
        loss = float(f._batch_tap(b, g_tap, b.dev('row_offset'), per, step=False))
        torch.cuda.synchronize()
    finally:
        echr_amd.set_deterministic(False)
    assert f.a.event_direct == 2 and f.a.w_init and f.a.vh_offset == opt.lda_dim
    assert abs(loss - total) < 2 * TOL_LOSS * abs(total) and np.abs(per.cpu().numpy() - per1).max() < 2 * TOL_LOSS * per1.max()
    assert abs(loss - ref['loss']) < TOL_LOSS * abs(ref['loss'])
    _check_flat(m, f.arena, f.arena.flat_g, flat1, 2 * TOL_GRAD)
    _check_grads(_grads(m), ref['grads'], TOL_GRAD)
    got = g_tap.cpu().numpy()
    for v, (one, want) in enumerate(zip(g_taps, ref['g_tap'])):
        a = got[int(b.row_offset[v]):int(b.row_offset[v + 1])]
        _check_tap(a, one, 2 * TOL_GRAD)
        _check_tap(a, want, TOL_GRAD)


def test_fused_batch_of_pooled_events_through_the_plain_batch_entry():
    """'EC', 'VL', 'CC', zero state: echr_train_step_batch (no g_tap) against the oracle's sum over the videos, training mode with the batch's
    dropout masks; then ONE update."""
    form = tuple(sorted(PLAIN_EC.items()))
    opt, params, vids = _vb(form)
    ref = _vb_ref(form, True)
    m, o, f = _fused(opt, params, True)
    b, _ = _batch(opt, vids)
    loss = float(f.batch(b, step=False))
    torch.cuda.synchronize()
    assert f.a.event_direct == 1 and not f.a.g_tap and not f.a.w_init
    assert abs(loss - ref['loss']) < TOL_LOSS * abs(ref['loss'])
    assert np.abs(f.last_video_losses.cpu().numpy() - ref['losses']).max() < TOL_LOSS * ref['losses'].max()
    _check_grads(_grads(m), ref['grads'], TOL_GRAD)
    m.set_dropout_state(U.SEED, U.OFFSET)
    loss = float(f.batch(b))
    assert abs(loss - ref['loss']) < TOL_LOSS * abs(ref['loss']) and o._flat['step'] == 1
    for k, p in m.named_parameters():
        d = np.abs(p.detach().cpu().numpy() - params[k]).max()
        assert (d == 0) if k in UNUSED else (d <= 1.01e-3 and (d > 0 or k in U.NOISE_ONLY)), (k, d)


# ---- 5. the other entries, 'EH' over the plain 'CC' form of the batch ---------------------------------------------------------------------
def _EH():
    return tuple(sorted(PLAIN_EH.items()))


def test_beam_batch_rows_equal_the_single_video_beam_search():
    opt, params, vids = _vb(_EH())
    m = U.build_gpu_model(opt, params, False)
    b, _ = _batch(opt, vids, labels=False)
    seq, lp, score, vw = m.beam_batch(b, 3, event_group_rows=2)
    seq, lp, score = seq.cpu().numpy(), lp.cpu().numpy(), score.cpu().numpy()
    assert seq.shape[1] == int(vw.max()) > 0
    for v, (s, vid) in enumerate(zip(b.event_slices, vids)):
        tap, c3d, lda = _feats(vid)
        s1, l1, sc1 = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval', beam_size=3, return_score=True)
        w = int(vw[v])
        assert w == (0 if isinstance(s1, list) else s1.shape[1]), v
        if w:
            assert np.array_equal(seq[s, :w], s1.cpu().numpy()), v
            assert np.abs(lp[s, :w] - l1.cpu().numpy()).max() <= 2 * TOL_LOGP, v
        assert not seq[s, w:].any(), v
        assert np.abs(score[s] - sc1.cpu().numpy()).max() <= 1e-4 * max(float(np.abs(score[s]).max()), 1.0), v


def _no_dropout(m):
    c = m.lm_model.core
    c.dropout0.p = c.dropout1.p = c.dropout2.p = 0.0
    m.lm_model.dropout.p = 0.0


def test_train_rl_batch_and_batch_step_equal_the_single_video_self_critical_steps():
    """A pinned gen_result of different widths per video and a signed reward, no dropout: train_rl_batch + VideoBatch.reward_criterion +
    backward, and SelfCriticalBatchStep, against the sum of V SelfCriticalStep(step=False) calls.  Two HIP results: twice the gates."""
    from echr_amd.fused import SelfCriticalBatchStep, SelfCriticalStep
    from echr_amd.misc.utils import RewardCriterion
    opt, params, vids = _vb(_EH())
    b, _ = _batch(opt, vids, labels=False)
    rs = np.random.RandomState(7)
    N = b.n_events
    gen = np.zeros((N, 5), np.int64)
    for v, s in enumerate(b.event_slices):
        wv = 2 + v
        for n in range(s.start, s.stop):
            ln = rs.randint(1, wv + 1)
            gen[n, :ln] = rs.randint(1, opt.CG_vocab_size + 1, size=ln)
        gen[s.start, :wv] = rs.randint(1, opt.CG_vocab_size + 1, size=wv)
    vw = b.caption_widths(gen)
    assert vw.tolist() == [2, 3, 4]
    gen = gen[:, :4]
    reward = rs.uniform(-1, 1, size=gen.shape).astype(np.float32)
    m1, o1, f1 = _fused(opt, params, clip=None)
    _no_dropout(m1)
    sc1 = SelfCriticalStep(f1)
    total, flat, per = 0.0, torch.zeros_like(f1.arena.flat_g), []
    for v, (vid, s) in enumerate(zip(vids, b.event_slices)):
        tap, c3d, lda = _feats(vid)
        w = int(vw[v])
        loss = float(sc1(tap, c3d, lda, vid['ind'], vid['soi'], gen_result=gen[s, :w], reward=reward[s, :w], step=False)[0])
        per.append(loss)
        total += loss
        flat += f1.arena.flat_g
    # the module path
    m2 = U.build_gpu_model(opt, params, True)
    _no_dropout(m2)
    ar2 = m2.build_arena()
    g2, slp, _, vw2 = m2.train_rl_batch(b, gen_result=torch.from_numpy(gen))
    la, per2 = b.reward_criterion(RewardCriterion(), slp, g2, reward, vw2)
    la.backward()
    assert np.array_equal(vw2, vw) and abs(float(la) - total) < 2 * TOL_LOSS * abs(total)
    assert np.abs(per2.detach().cpu().numpy() - np.asarray(per)).max() < 2 * TOL_LOSS * np.abs(per).max()
    for i, (k, p) in enumerate(m2.named_parameters()):
        lo, n = ar2.offsets[i], p.numel()
        r = flat[lo:lo + n].view(p.shape)
        if k in UNUSED:
            assert p.grad is None or not bool(p.grad.any()), k
        elif k in U.NOISE_ONLY:
            assert float(p.grad.abs().max()) < 1e-6, k
        else:
            assert float((p.grad - r).abs().max()) <= 2 * TOL_GRAD * max(float(r.abs().max()), U.GRAD_FLOOR) + 1e-9, k
    # the one-call path
    m, o, f = _fused(opt, params, clip=None)
    _no_dropout(m)
    sc = SelfCriticalBatchStep(f)
    loss, _, _, _, vw3 = sc(b, gen_result=gen, reward=reward, step=False)
    torch.cuda.synchronize()
    assert np.array_equal(vw3, vw) and abs(float(loss) - total) < 2 * TOL_LOSS * abs(total)
    assert np.abs(sc.last_video_losses.cpu().numpy() - np.asarray(per)).max() < 2 * TOL_LOSS * np.abs(per).max()
    _check_flat(m, f.arena, f.arena.flat_g, flat, 2 * TOL_GRAD)


def _tap_model(opt, sst_params):
    from echr_amd import models
    from echr_amd.optim import ClampAdam
    tm = models.setup_tap(opt)
    tm.load_state_dict({k: torch.from_numpy(v) for k, v in sst_params.items()})
    tm = tm.to(_dev())
    tm.eval()
    return tm, ClampAdam(tm.parameters(), lr=1e-9, arena=tm.build_arena())


def test_joint_batch_step_equals_the_per_video_joint_train_steps():
    """The proposal encoder in the loop (K = 16, eval mode, lr 1e-9): JointBatchStep(step=False) against the sum over the videos of
    JointTrainStep -- which, for a direct event context, runs without the prepare half and with the plain (not deferred) form -- in both losses
    and both models' gradients.  Two HIP results: twice the gates."""
    from echr_amd.fused import JointBatchStep, JointTrainStep
    opt, params, vids = _vb(_EH())
    sst_params, tap_in = synth.make_sst_params(opt), J.tap_inputs(vids, J.K)
    m1, o1, f1 = _fused(opt, params, False, lr=1e-9, clip=None)
    tm1, to1 = _tap_model(opt, sst_params)
    j1 = JointTrainStep(f1, tm1, to1, lambda1=J.LAMBDA1)
    assert j1.early is False
    cg, tl = 0.0, 0.0
    flat, tflat = torch.zeros_like(f1.arena.flat_g), torch.zeros_like(tm1._echr_arena.flat_g)
    for vid, (mk, lb, w1) in zip(vids, tap_in):
        labels, masks = _labels(vid)
        _, c3d, lda = _feats(vid)
        j1(c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], torch.from_numpy(mk), torch.from_numpy(lb), torch.from_numpy(w1))
        f1.join()
        assert not f1.mid_called
        cg, tl = cg + float(j1.cg_loss), tl + float(j1.tap_loss)
        flat += f1.arena.flat_g
        tflat += tm1._echr_arena.flat_g
    m, o, f = _fused(opt, params, False, lr=1e-9, clip=None)
    tm, to = _tap_model(opt, sst_params)
    js = JointBatchStep(f, tm, to, lambda1=J.LAMBDA1, lambda2=1.0)
    mk, lb, w1 = ([torch.from_numpy(t[i]).to(_dev()) for t in tap_in] for i in range(3))
    js([{k: v[k] for k in KEYS} for v in vids], mk, lb, w1, step=False)
    torch.cuda.synchronize()
    assert abs(float(js.cg_loss) - cg) < 2 * TOL_LOSS * abs(cg) and abs(float(js.tap_loss) - tl) < 2 * TOL_LOSS * abs(tl)
    _check_flat(m, f.arena, f.arena.flat_g, flat, 2 * TOL_GRAD)
    ar = tm._echr_arena
    for i, (k, p) in enumerate(tm.named_parameters()):
        lo, n = ar.offsets[i], p.numel()
        a, r = ar.flat_g[lo:lo + n], tflat[lo:lo + n]
        assert float((a - r).abs().max()) <= 2 * TOL_GRAD * max(float(r.abs().max()), U.GRAD_FLOOR) + 1e-9, (k, float((a - r).abs().max()), float(r.abs().max()))
    assert bool(tflat.any())


def test_caption_videos_give_each_video_its_own_records():
    """caption_videos on an 'EH' captioner: three short videos get the records caption_video gives each alone (the checks of
    tests/test_gpu_clip_batch.py's test of the same name)."""
    from echr_amd import eval_utils as EU
    from echr_amd import models as EM
    opt, params, _ = _vb(_EH())
    opt = synth.default_opt(CG_vocab_size=300, CG_seq_length=7, K=8, **PLAIN_EH)
    torch.manual_seed(3)
    tap = EM.setup_tap(opt)
    tap.eval()
    tap, cg = tap.cuda(), U.build_gpu_model(opt, params, False)
    f2t = lambda s, e, n, d: [round(float(s) / n * d, 3), round(float(e) / n * d, 3)]
    rs = np.random.RandomState(19)
    videos = [dict(c3d=torch.from_numpy(rs.standard_normal((T, opt.video_dim)).astype(np.float32)).cuda(),
                   lda=torch.from_numpy(rs.standard_normal(opt.lda_dim).astype(np.float32)).cuda(), duration=60.0) for T in (24, 9, 40)]
    infos, ex = EU.caption_videos(tap, cg, videos, f2t, topN=6)
    assert len(infos) == 3 and max(len(i) for i in infos) > 0
    for v, vid in enumerate(videos):
        one = EU.caption_video(tap, cg, vid['c3d'], vid['lda'], vid['duration'], f2t, topN=6)
        one = one[0] if isinstance(one, tuple) else one
        assert len(one) == len(infos[v]), v
        for rec, ref in zip(infos[v], one):
            assert rec['sentence'] == ref['sentence'] and rec['timestamp'] == ref['timestamp'] and rec['num'] == ref['num']
            assert abs(rec['proposal_score'] - ref['proposal_score']) < 1e-6
            assert abs(rec['sentence_confidence'] - ref['sentence_confidence']) < 1e-3

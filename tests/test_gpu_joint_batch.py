"""The joint 'tap_cg' iteration over a multi-video batch on the GPU (-m gpu): the batched proposal criterion (echr_tap_bce_fwd_batch /
_bwd_batch), the caption side with d loss / d batch.tap (echr_train_step_batch_tap) and fused.JointBatchStep against the CPU reference of the
contract (tests/joint_batch_ref.py: the oracle once per video, both models' gradients summed, sliced dropout masks), the reference's own
fixture (tests/golden/case_joint_batch.npz) and the unchanged single-video JointTrainStep.

Gates: the project's own -- losses 1e-5 relative, each gradient tensor U.grad_close(..., 1e-5) of its max-norm (the rule of DESIGN section 4l
is max(1e-5, 4 e_ref); e_ref, the oracle's float32-vs-float64 difference of the joint chain on vbctx, is at most 6.3e-7 on any SST gradient
tensor in eval and train mode, and 8.7e-7 on the nine-video case (enc_attn.query_1.bias), so the gate is the plain 1e-5 everywhere).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from echr_amd import synth
from oracle import echr_ref_cpu as O
from oracle import summary as SM
from tests import joint_batch_ref as J
from tests import util as U
from tests import vbatch_ref as VR

pytestmark = pytest.mark.gpu

TOL_LOSS = 1e-5
TOL_GRAD = 1e-5
KEYS = ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')
UNUSED = {'lm_model.core.fusion_layer.weight', 'lm_model.core.fusion_layer.bias', 'fusion_model.h2a_layer.weight', 'fusion_model.h2a_layer.bias'}


def _dev():
    return torch.device('cuda')


def _close(name, got, ref, tol=TOL_GRAD):
    print('%-48s %.3e' % (name, U.relerr(got, ref, U.GRAD_FLOOR)))
    assert U.grad_close(name, got, ref, tol), (name, U.relerr(got, ref))


def _loss_close(name, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    print('%-48s %.3e' % (name, np.abs(got - ref).max() / np.abs(ref).max()))
    assert np.abs(got - ref).max() < TOL_LOSS * np.abs(ref).max(), (name, got, ref)


# ---- 1. the criterion kernels -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bce_case(lengths, K, per_video):
    rs = np.random.RandomState(3 + len(lengths))
    ro = [0]
    for t in lengths:
        ro.append(ro[-1] + t)
    T, V = ro[-1], len(lengths)
    scores = rs.uniform(0.02, 0.98, size=(T, K)).astype(np.float32)
    labels = (rs.uniform(size=(T, K)) > 0.8).astype(np.float32)
    masks = np.concatenate([(np.arange(t)[:, None] >= np.arange(K)[None, :]).astype(np.float32) for t in lengths], 0)
    w1 = rs.uniform(0.05, 0.3, size=(V if per_video else 1, K)).astype(np.float32)
    g_loss = 0.37
    losses, g = [], []
    for v, (a, b) in enumerate(zip(ro[:-1], ro[1:])):
        s = torch.from_numpy(scores[a:b]).requires_grad_(True)
        loss = O.tap_criterion(s, torch.from_numpy(masks[a:b]), torch.from_numpy(labels[a:b]), torch.from_numpy(w1[v if per_video else 0]))
        (g_loss * loss).backward()
        losses.append(float(loss.detach()))
        g.append(s.grad.numpy())
    return ro, scores, masks, labels, w1, g_loss, np.asarray(losses), g


def _bce_gpu(ro, scores, masks, labels, w1, g_loss, per_video):
    from echr_amd import _lib as L
    lib, dev = L.load(), _dev()
    V, (T, K) = len(ro) - 1, scores.shape
    sc, mk, lb = (torch.from_numpy(x).to(dev) for x in (scores, masks, labels))
    ww = torch.from_numpy(np.ascontiguousarray(w1 if per_video else w1[0])).to(dev)
    ro_dev = torch.tensor(ro, dtype=torch.int32, device=dev)
    per, total, part = torch.zeros(V, device=dev), torch.zeros(1, device=dev), torch.zeros(64 * V, device=dev)
    gl, gs = torch.full((1,), g_loss, device=dev), torch.full((T, K), float('nan'), device=dev)
    ld = K if per_video else 0
    L.check(lib.echr_tap_bce_fwd_batch(L.ptr(sc), L.ptr(mk), L.ptr(lb), L.ptr(ww), ld, L.ptr(ro_dev, torch.int32), V, K, L.ptr(per), L.ptr(total),
                                       L.ptr(part), L.stream_ptr()), 'tap_bce_fwd_batch')
    L.check(lib.echr_tap_bce_bwd_batch(L.ptr(sc), L.ptr(mk), L.ptr(lb), L.ptr(ww), ld, L.ptr(ro_dev, torch.int32), V, K, T, L.ptr(gl), L.ptr(gs),
                                       L.stream_ptr()), 'tap_bce_bwd_batch')
    torch.cuda.synchronize()
    return per.cpu().numpy(), float(total), gs.cpu().numpy()


@pytest.mark.parametrize('per_video', [False, True])
def test_criterion_kernels_vs_oracle(per_video):
    """Lengths (1, 2, 5, 37, 5), K = 16 (video boundaries inside a workgroup's 256 elements, a one-row video, a video of more than one
    workgroup): per-video losses, their sum, d scores; two runs agree bit for bit; the autograd form returns the same."""
    from echr_amd.misc.utils import TAPModelCriterion
    ro, scores, masks, labels, w1, g_loss, losses, g = _bce_case((1, 2, 5, 37, 5), 16, per_video)
    per, total, gs = _bce_gpu(ro, scores, masks, labels, w1, g_loss, per_video)
    _loss_close('per-video losses', per, losses)
    _loss_close('sum', total, losses.sum())
    assert np.isfinite(gs).all()
    for v, (a, b) in enumerate(zip(ro[:-1], ro[1:])):
        _close('g_scores video %d' % v, gs[a:b], g[v])
    per2, total2, gs2 = _bce_gpu(ro, scores, masks, labels, w1, g_loss, per_video)
    assert np.array_equal(per, per2) and total == total2 and np.array_equal(gs, gs2)
    # misc.utils.TAPModelCriterion.forward_batch: the same two entries behind autograd
    dev = _dev()
    s = torch.from_numpy(scores).to(dev).requires_grad_(True)
    ww = [torch.from_numpy(w) for w in w1] if per_video else torch.from_numpy(w1[0])
    tot, pv = TAPModelCriterion().forward_batch(s, torch.from_numpy(masks), torch.from_numpy(labels), ww, ro)
    (g_loss * tot).backward()
    torch.cuda.synchronize()
    assert np.array_equal(pv.detach().cpu().numpy(), per) and float(tot.detach()) == total
    assert np.allclose(s.grad.cpu().numpy(), gs, rtol=1e-6, atol=1e-12)          # (g_loss * 1.0 arrives as the upstream gradient: the same product)


def test_one_video_batch_equals_the_single_video_criterion_bit_for_bit():
    from echr_amd import _lib as L
    lib, dev = L.load(), _dev()
    for T in (37, 300):          # 300 x 16 elements: every one of the 64 partial ranges is more than one pass of a workgroup's 4 x 256
        ro, scores, masks, labels, w1, g_loss, _, _ = _bce_case((T,), 16, False)
        per, total, gs = _bce_gpu(ro, scores, masks, labels, w1, g_loss, False)
        sc, mk, lb, ww = (torch.from_numpy(x).to(dev) for x in (scores, masks, labels, w1[0]))
        buf, gl, g1 = torch.zeros(65, device=dev), torch.full((1,), g_loss, device=dev), torch.empty(T, 16, device=dev)
        L.check(lib.echr_tap_bce_fwd_ws(L.ptr(sc), L.ptr(mk), L.ptr(lb), L.ptr(ww), L.ptr(buf[:1]), L.ptr(buf[1:]), T, 16, L.stream_ptr()), 'tap_bce_fwd_ws')
        L.check(lib.echr_tap_bce_bwd(L.ptr(sc), L.ptr(mk), L.ptr(lb), L.ptr(ww), L.ptr(gl), L.ptr(g1), T, 16, L.stream_ptr()), 'tap_bce_bwd')
        torch.cuda.synchronize()
        assert float(buf[0]) == float(per[0]) == total, T
        assert np.array_equal(g1.cpu().numpy(), gs), T


# ---- shared builders --------------------------------------------------------------------------------------------------------------
def _fused(opt, params, train_mode, lr=1e-9, clip=None):
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    m = U.build_gpu_model(opt, params, train_mode)
    o = ClampAdam(m.parameters(), lr=lr, arena=m.build_arena())
    return m, o, FusedTrainStep(m, o, grad_clip=clip)


def _tap_model(opt, sst_params, train_mode, lr=1e-9):
    from echr_amd import models
    from echr_amd.optim import ClampAdam
    tm = models.setup_tap(opt)
    tm.load_state_dict({k: torch.from_numpy(v) for k, v in sst_params.items()})
    tm = tm.to(_dev())
    tm.train() if train_mode else tm.eval()
    tm.set_dropout_state(U.SEED, U.OFFSET)
    return tm, ClampAdam(tm.parameters(), lr=lr, arena=tm.build_arena())


def _arena_grads(model, unused=()):
    ar = model._echr_arena
    out = {}
    for i, (k, p) in enumerate(model.named_parameters()):
        assert ar.params[i] is p
        gv = ar.grad_view(i).detach().cpu().numpy().copy()
        if k in unused:
            assert not gv.any(), k
            out[k] = None
        else:
            out[k] = gv
    return out


def _check_grads(got, ref, tol=TOL_GRAD):
    for k, g in ref.items():
        if g is None:
            assert got[k] is None or not np.any(got[k]), k
            continue
        _close(k, got[k], g, tol)


# ---- 2. echr_train_step_batch_tap -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vb_case(event_context_type=None, video_context_type=None):
    opt, params, vids = synth.make_vbatch('vbctx')
    if event_context_type is not None:
        opt.event_context_type, opt.video_context_type = event_context_type, video_context_type
        params = synth.make_params(opt, 0)
    return opt, params, vids


@functools.lru_cache(maxsize=None)
def _vb_ref(train_mode, event_context_type=None, video_context_type=None):
    opt, params, vids = _vb_case(event_context_type, video_context_type)
    return VR.run(opt, params, vids, train_mode)


def _batch(vids):
    from echr_amd.batch import VideoBatch
    dev = _dev()
    return VideoBatch.from_videos([dict({k: v[k] for k in KEYS}, tap=torch.from_numpy(v['tap']).to(dev)) for v in vids], device=dev)


def _tap_call(opt, params, vids, train_mode, g_loss=None):
    m, o, f = _fused(opt, params, train_mode)
    b = _batch(vids)
    g_tap = torch.zeros_like(b.tap)
    per = torch.zeros(b.n_videos, device=_dev())
    gl = None if g_loss is None else torch.full((1,), g_loss, device=_dev())
    loss = float(f._batch_tap(b, g_tap, b.dev('row_offset'), per, g_loss=gl, step=False))
    torch.cuda.synchronize()
    return loss, per.cpu().numpy(), g_tap.cpu().numpy(), _arena_grads(m, UNUSED), b


@pytest.mark.parametrize('train_mode', [False, True])
def test_batch_tap_call_on_vbctx(train_mode):
    """Scene context 'VLVCVH' (the 'VH' span goes back over each video's OWN rows), 'ER3' (the anchors' rows), a one-event video: d tap per
    video against vbatch_ref; loss and parameter gradients against vbatch_ref and against the same call without g_tap."""
    opt, params, vids = _vb_case()
    assert 'VH' in opt.video_context_type and opt.event_context_type == 'ER3' and min(len(v['soi']) for v in vids) == 1
    ref = _vb_ref(train_mode)
    loss, per, g_tap, grads, b = _tap_call(opt, params, vids, train_mode)
    _loss_close('loss', loss, ref['loss'])
    _loss_close('per-video losses', per, ref['losses'])
    ro = b.row_offset
    for v, r in enumerate(ref['g_tap']):
        _close('g_tap video %d' % v, g_tap[ro[v]:ro[v + 1]], r)
    _check_grads(grads, ref['grads'])
    m2, o2, f2 = _fused(opt, params, train_mode)
    loss2 = float(f2.batch(_batch(vids), step=False))
    torch.cuda.synchronize()
    assert abs(loss - loss2) < TOL_LOSS * abs(loss2)
    _loss_close('per-video losses, plain call', per, f2.last_video_losses.cpu().numpy())
    _check_grads(grads, _arena_grads(m2, UNUSED))
    # g_loss scales every gradient and d tap; the losses are reported unscaled
    loss3, per3, g_tap3, grads3, _ = _tap_call(opt, params, vids, train_mode, g_loss=0.5)
    assert abs(loss3 - loss) < TOL_LOSS * abs(loss) and np.abs(per3 - per).max() < TOL_LOSS * np.abs(per).max()
    for v, r in enumerate(ref['g_tap']):
        _close('g_tap video %d, g_loss 0.5' % v, g_tap3[ro[v]:ro[v + 1]], 0.5 * r)
    _check_grads(grads3, {k: (None if g is None else 0.5 * g) for k, g in ref['grads'].items()})


@pytest.mark.parametrize('video_context_type', ['VL', 'VH'])
def test_batch_tap_call_without_anchor_rows(video_context_type):
    """'ER1' reads no tap row: with 'VL' d tap stays exactly zero, with 'VH' it is the scene term alone (constant over a video's rows)."""
    opt, params, vids = _vb_case('ER1', video_context_type)
    loss, per, g_tap, grads, b = _tap_call(opt, params, vids, True)
    ref = _vb_ref(True, 'ER1', video_context_type)
    _loss_close('loss', loss, ref['loss'])
    ro = b.row_offset
    if video_context_type == 'VL':
        assert not g_tap.any()
        return
    for v, r in enumerate(ref['g_tap']):
        rows = g_tap[ro[v]:ro[v + 1]]
        assert rows.any() and np.array_equal(rows, np.broadcast_to(rows[:1], rows.shape)), v
        _close('g_tap video %d' % v, rows, r)
    _check_grads(grads, ref['grads'])


# ---- 3..7. JointBatchStep ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _joint_case(name):
    return J.setup('vbctx') if name == 'vbctx' else J.setup_wide()


@functools.lru_cache(maxsize=None)
def _joint_ref(name, train_mode, lambda2=1.0):
    opt, params, sst_params, vids, tap_in = _joint_case(name)
    return J.run(opt, params, sst_params, vids, tap_in, train_mode, J.LAMBDA1, lambda2)


def _joint_step(case, train_mode, lambda2=1.0, lr=1e-9, clip=None, step=True, vids=None, tap_in=None, concatenated=False):
    from echr_amd.fused import JointBatchStep
    opt, params, sst_params, all_vids, all_tap = case
    vids, tap_in = (all_vids, all_tap) if vids is None else (vids, tap_in)
    m, o, f = _fused(opt, params, train_mode, lr=lr, clip=clip)
    tm, to = _tap_model(opt, sst_params, train_mode, lr=lr)
    js = JointBatchStep(f, tm, to, lambda1=J.LAMBDA1, lambda2=lambda2, tap_grad_clip=clip)
    videos = [{k: v[k] for k in KEYS} for v in vids]
    mk, lb, w1 = ([torch.from_numpy(t[i]) for t in tap_in] for i in range(3))
    if concatenated:          # the other input form: a ready VideoBatch (its tap is ignored), [T_tot, K] matrices, w1 [V, K]
        videos = _batch(vids)
        mk, lb, w1 = torch.cat(mk, 0).to(_dev()), torch.cat(lb, 0), torch.stack(w1, 0)
    loss = js(videos, mk, lb, w1, step=step)
    assert loss.dim() == 0 and loss.is_cuda
    torch.cuda.synchronize()
    return dict(js=js, m=m, o=o, tm=tm, to=to, loss=float(loss), tap_losses=js.last_tap_losses.cpu().numpy(), cg_losses=js.last_video_losses.cpu().numpy(),
                tap_loss=float(js.tap_loss), cg_loss=float(js.cg_loss), grads=_arena_grads(m, UNUSED), sst_grads=_arena_grads(tm),
                g_tap=js._bufs['g_tap'].cpu().numpy())


def _check_joint(got, ref, lambda2=1.0):
    _loss_close('tap losses', got['tap_losses'], ref['tap_losses'])
    _loss_close('cg losses', got['cg_losses'], ref['cg_losses'])
    _loss_close('tap sum', got['tap_loss'], ref['tap_losses'].sum())
    _loss_close('cg sum', got['cg_loss'], ref['cg_losses'].sum())
    _loss_close('joint loss', got['loss'], J.LAMBDA1 * ref['tap_losses'].sum() + lambda2 * ref['cg_losses'].sum())
    _check_grads(got['grads'], ref['grads'])
    _check_grads(got['sst_grads'], ref['sst_grads'])


def _check_fixture(got):
    g = U.gold('case_joint_batch.npz')
    _loss_close('tap losses vs fixture', got['tap_losses'], g['eval|tap_losses'])
    _loss_close('cg losses vs fixture', got['cg_losses'], g['eval|cg_losses'])
    for tag, grads in (('eval|grad|', got['grads']), ('eval|sstgrad|', got['sst_grads'])):
        for k, v in grads.items():
            if v is None or k in U.NOISE_ONLY:
                continue
            ref = float(g[tag + k + '|linf'])
            assert abs(float(np.abs(v).max()) - ref) <= TOL_GRAD * max(ref, U.GRAD_FLOOR) + 1e-9, k
            head, strided = SM.grad_slices(v)          # elements of the reference's ACCUMULATED gradient
            for a, want in ((head, g[tag + k + '|head']), (strided, g[tag + k + '|strided'])):
                assert np.abs(a - want).max() <= TOL_GRAD * max(ref, U.GRAD_FLOOR) + 1e-9, k


@pytest.mark.parametrize('train_mode,lambda2', [(False, 1.0), (True, 1.0), (True, 0.5)])
def test_joint_batch_step_vs_reference(train_mode, lambda2):
    """vbctx, K = 16, lambda1 = 0.01: both per-video loss vectors and both models' summed gradients (read from the arenas; lr = 1e-9 and no
    clip, so the update does not disturb them) against joint_batch_ref; in eval mode also against the reference's own fixture."""
    got = _joint_step(_joint_case('vbctx'), train_mode, lambda2)
    assert got['o']._flat['step'] == 1 and got['to']._flat['step'] == 1
    _check_joint(got, _joint_ref('vbctx', train_mode, lambda2), lambda2)
    if not train_mode:
        _check_fixture(got)


def test_joint_batch_step_takes_a_ready_batch_and_concatenated_inputs():
    """step=False with a VideoBatch (whose tap is ignored), [T_tot, K] matrices and w1 [V, K]: the same gradients, left in the arenas as
    `.grad` views, no optimiser step."""
    got = _joint_step(_joint_case('vbctx'), True, step=False, concatenated=True)
    assert got['o']._flat is None or got['o']._flat['step'] == 0
    assert got['to']._flat is None or got['to']._flat['step'] == 0
    _check_joint(got, _joint_ref('vbctx', True))
    for model in (got['m'], got['tm']):
        ar = model._echr_arena
        assert ar.grads_in_arena() and any(p.grad is not None for p in model.parameters())
    assert all(p.grad is not None for p in got['tm'].parameters())


def _check_one_step(name, model, optim, params, ref_grads, lr, clip, tol=TOL_GRAD):
    """Parameters and both Adam moments after ONE step against vbatch_ref.step on the oracle's summed gradients (the gates of
    tests/test_gpu_vbatch.py's one-step test)."""
    rp, rm, rv = VR.step(params, ref_grads, lr=lr, clip=clip)
    ar = model._echr_arena
    for i, (k, p) in enumerate(model.named_parameters()):
        lo, n = ar.offsets[i], p.numel()
        mom = optim._flat['m'][lo:lo + n].view(p.shape).cpu().numpy()
        var = optim._flat['v'][lo:lo + n].view(p.shape).cpu().numpy()
        new = p.detach().cpu().numpy()
        rg = ref_grads[k]
        if rg is None:
            assert np.array_equal(new, params[k]) and not mom.any() and not var.any(), k
            continue
        if k in U.NOISE_ONLY:
            assert np.abs(new - params[k]).max() <= 1.01 * lr
            continue
        assert U.grad_close(k, mom, rm[k], tol), (name, k, 'exp_avg', U.relerr(mom, rm[k]))
        assert np.abs(var - rv[k]).max() <= 2.5 * tol * max(float(rv[k].max()), 1e-3 * U.GRAD_FLOOR ** 2) + 1e-20, (name, k, 'exp_avg_sq')
        dgpu, dref = new - params[k], rp[k] - params[k]
        assert np.abs(dgpu).max() <= 1.01 * lr and np.abs(dgpu - dref).max() <= 2.01 * lr, (name, k)
        solid = np.abs(rg) > 1e-4 * float(np.abs(rg).max())
        if solid.any():
            assert np.abs(dgpu - dref)[solid].max() < 0.02 * lr, (name, k, np.abs(dgpu - dref)[solid].max() / lr)


def test_joint_batch_one_step_matches_clamp_adam_on_the_summed_gradients():
    """ONE clamp + ONE Adam step per model on the SUM of the videos' gradients."""
    case = _joint_case('vbctx')
    opt, params, sst_params, _, _ = case
    lr, clip = 1e-3, 100.0
    got = _joint_step(case, True, lr=lr, clip=clip)
    ref = _joint_ref('vbctx', True)
    assert got['o']._flat['step'] == 1 and got['to']._flat['step'] == 1
    _check_one_step('caption', got['m'], got['o'], params, ref['grads'], lr, clip)
    _check_one_step('sst', got['tm'], got['to'], sst_params, ref['sst_grads'], lr, clip)


def test_one_video_batch_equals_joint_train_step():
    """V = 1: both losses and all gradients of both models against JointTrainStep(early_prepare=False) on that video."""
    from echr_amd.fused import JointTrainStep
    case = _joint_case('vbctx')
    opt, params, sst_params, vids, tap_in = case
    v = 4
    vid, (mk, lb, w1) = vids[v], tap_in[v]
    assert len(vid['soi']) > 1
    got = _joint_step(case, True, vids=[vid], tap_in=[tap_in[v]])
    m, o, f = _fused(opt, params, True)
    tm, to = _tap_model(opt, sst_params, True)
    js = JointTrainStep(f, tm, to, lambda1=J.LAMBDA1, early_prepare=False)
    dev = _dev()
    T = min(len(vid['c3d']), len(vid['tap']))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    loss = js(torch.from_numpy(vid['c3d'][:T]).to(dev), torch.from_numpy(vid['lda']).to(dev), labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:],
              torch.from_numpy(mk), torch.from_numpy(lb), torch.from_numpy(w1))
    f.join()
    torch.cuda.synchronize()
    _loss_close('tap loss', got['tap_loss'], float(js.tap_loss))
    _loss_close('cg loss', got['cg_loss'], float(js.cg_loss))
    _loss_close('joint loss', got['loss'], float(loss))
    _check_grads(got['grads'], _arena_grads(m, UNUSED))
    _check_grads(got['sst_grads'], _arena_grads(tm))


def test_nine_videos_of_eight_events():
    """72 events (> 64: launch-per-phase recurrences) in more videos than one persistent proposal-encoder launch carries."""
    from echr_amd import _lib
    case = _joint_case('wide')
    vids = case[3]
    assert len(vids) == 9 and all(len(v['soi']) == 8 for v in vids) and all(30 <= len(v['c3d']) <= 40 for v in vids)
    assert len(vids) > _lib.load().echr_sst_batch_group()
    got = _joint_step(case, True)
    assert got['js'].last_batch.n_events == 72
    _check_joint(got, _joint_ref('wide', True))


def test_deterministic_mode_is_bitwise():
    import echr_amd
    case = _joint_case('vbctx')
    echr_amd.set_deterministic(True)
    try:
        a = _joint_step(case, True, step=False)
        b = _joint_step(case, True, step=False)
    finally:
        echr_amd.set_deterministic(False)
    assert a['loss'] == b['loss'] and np.array_equal(a['tap_losses'], b['tap_losses']) and np.array_equal(a['cg_losses'], b['cg_losses'])
    assert np.array_equal(a['g_tap'], b['g_tap']) and a['g_tap'].any()
    for x, y in ((a['m'], b['m']), (a['tm'], b['tm'])):
        assert torch.equal(x._echr_arena.flat_g, y._echr_arena.flat_g) and bool(x._echr_arena.flat_g.any())
    _check_joint(a, _joint_ref('vbctx', True))


def test_joint_train_step_lambda2_scales_the_caption_term():
    """JointTrainStep(lambda2=0.5) on one video against joint_batch_ref on that video alone."""
    from echr_amd.fused import JointTrainStep
    opt, params, sst_params, vids, tap_in = _joint_case('vbctx')
    v = 4
    vid, (mk, lb, w1) = vids[v], tap_in[v]
    ref = J.run(opt, params, sst_params, [vid], [tap_in[v]], False, J.LAMBDA1, 0.5)
    m, o, f = _fused(opt, params, False)
    tm, to = _tap_model(opt, sst_params, False)
    js = JointTrainStep(f, tm, to, lambda1=J.LAMBDA1, lambda2=0.5, early_prepare=False)          # ('VH': the scene vector needs tap_feats)
    dev = _dev()
    T = min(len(vid['c3d']), len(vid['tap']))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    loss = js(torch.from_numpy(vid['c3d'][:T]).to(dev), torch.from_numpy(vid['lda']).to(dev), labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:],
              torch.from_numpy(mk), torch.from_numpy(lb), torch.from_numpy(w1))
    f.join()
    torch.cuda.synchronize()
    _loss_close('cg loss (unscaled)', float(js.cg_loss), ref['cg_losses'][0])
    _loss_close('joint loss', float(loss), J.LAMBDA1 * ref['tap_losses'][0] + 0.5 * ref['cg_losses'][0])
    _check_grads(_arena_grads(m, UNUSED), ref['grads'])
    _check_grads(_arena_grads(tm), ref['sst_grads'])
    assert f.a.g_loss == f.one.data_ptr()          # the caption call's own unit scalar is back in place


# ---- 8. the example ---------------------------------------------------------------------------------------------------------------
def test_example_joint_m_batch_runs_the_batch_step():
    """examples/train_synthetic.py --joint --m_batch 3 --iters 4 in a fresh child process: finite losses, through JointBatchStep."""
    root = os.path.dirname(os.path.dirname(U.GOLD))
    r = subprocess.run([sys.executable, os.path.join(root, 'examples', 'train_synthetic.py'), '--joint', '--m_batch', '3', '--iters', '4'],
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if 'JointBatchStep over 3 videos' in l]
    assert len(lines) >= 2, r.stdout
    for l in lines:
        vals = [float(l.split(key)[1].split()[0]) for key in ('joint_loss ', 'cg_loss ', 'tap_loss ')]
        assert np.isfinite(vals).all() and all(x > 0 for x in vals), l

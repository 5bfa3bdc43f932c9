"""Multi-video batches on the GPU (-m gpu): CaptionGenerator.forward_batch, FusedTrainStep.batch and the batched greedy decode against the CPU
reference of the batch contract (tests/vbatch_ref.py: the oracle once per video, losses and gradients summed, sliced dropout masks), the
reference's own fixture (tests/golden/case_vbatch.npz) and the unchanged single-video path.

Gates: the project's own -- log-probs 2e-5 absolute, loss 1e-5 relative, greedy `seq` bit-exact, each gradient tensor
max(1e-5, 4 * e_ref) of its max-norm (+1e-9 absolute), where e_ref is the float32-vs-float64 difference of the SUMMED-gradient oracle on the
same fixture (a sum over V videos can lose relative accuracy to cancellation; the rule of tests/test_gpu_attention_regime.py).  Measured on
the CPU (worst tensor; tools: tests/vbatch_ref.run in both precisions):

    vbctx  eval 1.0e-06 (core.attention.h2att.weight)   train 7.5e-07 (core.attention.h2att.bias)    d tap_feats 8.3e-07 / 7.8e-07
    vb24   eval 9.9e-07 (core.attention.ctx2att.bias)   train 1.15e-06 (enc_attn.pair_pos_fc2.bias)  d tap_feats 7.6e-07 / 7.1e-07
    vb16   eval 8.3e-07 (core.attention.h2att.bias)     train 8.8e-07 (enc_attn.query_1.weight)      d tap_feats 6.9e-07 / 8.2e-07
    (summed loss: <= 3.3e-08 relative; log-probs: <= 1.2e-06 absolute)

so 4 * e_ref stays below 1e-5 everywhere and the gate is the plain 1e-5.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from echr_amd import synth
from oracle import summary as SM
from tests import util as U
from tests import vbatch_ref as R

pytestmark = pytest.mark.gpu

TOL_LOGP = 2e-5
TOL_LOSS = 1e-5
E_REF = {'vbctx': 1.0e-6, 'vb24': 1.15e-6, 'vb16': 8.8e-7}          # worst tensor of the summed-gradient oracle, float32 vs float64 (header)


def tol_grad(case):
    return max(1e-5, 4 * E_REF[case])


@functools.lru_cache(maxsize=None)
def _ref(case, train_mode):
    opt, params, vids = synth.make_vbatch(case)
    return R.run(opt, params, vids, train_mode)


def _batch(vids, tap_leaves=False, labels=True):
    from echr_amd.batch import VideoBatch
    dev = torch.device('cuda')
    taps = [torch.from_numpy(v['tap']).to(dev).requires_grad_(tap_leaves) for v in vids]
    keys = ('c3d', 'lda', 'ind', 'soi') + (('labels', 'masks') if labels else ())
    b = VideoBatch.from_videos([dict({k: v[k] for k in keys}, tap=t) for v, t in zip(vids, taps)], device=dev)
    return b, taps


def _grads(m):
    return {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}


def _module_pass(opt, params, vids, train_mode, arena=False):
    """forward_batch(mode='train') + the per-video criterion + backward with every video's tap_feats as a leaf."""
    from echr_amd.misc.utils import LanguageModelCriterion
    m = U.build_gpu_model(opt, params, train_mode)
    if arena:
        m.build_arena()
    b, taps = _batch(vids, True)
    logp = m.forward_batch(b, mode='train')
    total, per = b.criterion(LanguageModelCriterion(), logp)
    total.backward()
    torch.cuda.synchronize()
    g_tap = [t.grad.detach().cpu().numpy() if t.grad is not None else np.zeros(tuple(t.shape), np.float32) for t in taps]
    return dict(logp=logp.detach().cpu().numpy(), loss=float(total.detach()), losses=per.detach().cpu().numpy(), grads=_grads(m), g_tap=g_tap,
                model=m, batch=b)


def _check_logp(b, logp, ref):
    assert logp.shape[0] == b.n_events and logp.shape[1] == b.S
    for v, s in enumerate(b.event_slices):
        Sv = ref['logp'][v].shape[1]
        assert Sv == b.steps[v]
        assert np.abs(logp[s, :Sv] - ref['logp'][v]).max() < TOL_LOGP, v


def _check_grads(case, grads, ref, tol=None):
    tol = tol_grad(case) if tol is None else tol
    for k, g in ref['grads'].items():
        if g is None:
            assert grads[k] is None or not np.any(grads[k]), k
            continue
        assert U.grad_close(k, grads[k], g, tol), (k, U.relerr(grads[k], g))


def _check_vs_ref(case, got, ref):
    _check_logp(got['batch'], got['logp'], ref)
    assert abs(got['loss'] - ref['loss']) < TOL_LOSS * abs(ref['loss']), (got['loss'], ref['loss'])
    assert np.abs(got['losses'] - ref['losses']).max() < TOL_LOSS * np.abs(ref['losses']).max()
    _check_grads(case, got['grads'], ref)
    for v, (a, r) in enumerate(zip(got['g_tap'], ref['g_tap'])):
        assert np.abs(a - r).max() <= tol_grad(case) * max(float(np.abs(r).max()), U.GRAD_FLOOR) + 1e-9, (v, U.relerr(a, r))


def _check_vs_fixture(case, mode, got):
    g = U.gold('case_vbatch.npz')
    key = case + '|' + mode
    cols = SM.logp_columns(got['logp'].shape[2])
    for v, s in enumerate(got['batch'].event_slices):
        want = g[key + '|logp|v%02d' % v]
        assert np.abs(got['logp'][s, :want.shape[1]][:, :, cols] - want).max() < TOL_LOGP, v
    assert abs(got['loss'] - float(g[key + '|loss'])) < TOL_LOSS * abs(float(g[key + '|loss']))
    assert np.abs(got['losses'] - g[key + '|losses']).max() < TOL_LOSS * np.abs(g[key + '|losses']).max()
    for k, v in got['grads'].items():
        if v is not None and k not in U.NOISE_ONLY and (key + '|grad|' + k + '|linf') in g:
            ref = float(g[key + '|grad|' + k + '|linf'])
            assert abs(float(np.abs(v).max()) - ref) <= tol_grad(case) * max(ref, U.GRAD_FLOOR) + 1e-9, k
            head, strided = SM.grad_slices(v)          # elements of the reference's ACCUMULATED gradient
            for a, want in ((head, g[key + '|grad|' + k + '|head']), (strided, g[key + '|grad|' + k + '|strided'])):
                assert np.abs(a - want).max() <= tol_grad(case) * max(ref, U.GRAD_FLOOR) + 1e-9, k


@pytest.mark.parametrize('case', ['vbctx', 'vb16'])
@pytest.mark.parametrize('train_mode', [False, True])
def test_module_path_matches_vbatch_ref_and_reference(case, train_mode):
    """Every log-prob, the summed loss, the per-video losses, every gradient element and d tap_feats (through 'ER3', and 'VH' in vbctx)."""
    opt, params, vids = synth.make_vbatch(case)
    got = _module_pass(opt, params, vids, train_mode, arena=(case == 'vbctx'))
    _check_vs_ref(case, got, _ref(case, train_mode))
    _check_vs_fixture(case, 'train' if train_mode else 'eval', got)


def _fused(opt, params, train_mode=True, lr=1e-3, clip=100.0):
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    m = U.build_gpu_model(opt, params, train_mode)
    o = ClampAdam(m.parameters(), lr=lr, arena=m.build_arena())
    return m, o, FusedTrainStep(m, o, grad_clip=clip)


@pytest.mark.parametrize('case', ['vbctx', 'vb16'])
@pytest.mark.parametrize('device_criterion', [False, True])
def test_fused_batch_gradients_match_vbatch_ref(case, device_criterion):
    """FusedTrainStep.batch(step=False): the summed loss, the per-video losses and the summed gradients; criterion inputs travelling with the
    index vectors (active rows compacted) and as device tensors (all rows)."""
    opt, params, vids = synth.make_vbatch(case)
    m, o, f = _fused(opt, params)
    b, _ = _batch(vids)
    loss = float(f.batch(b, step=False, device_criterion=device_criterion))
    torch.cuda.synchronize()
    ref = _ref(case, True)
    if not device_criterion:
        assert 0 < f.last_active_rows < b.n_events * b.S           # the compacted (active-row) form ran
    assert abs(loss - ref['loss']) < TOL_LOSS * abs(ref['loss']), (loss, ref['loss'])
    assert np.abs(f.last_video_losses.cpu().numpy() - ref['losses']).max() < TOL_LOSS * np.abs(ref['losses']).max()
    _check_grads(case, _grads(m), ref)
    assert o._flat is None or o._flat['step'] == 0
    # what the call staged with the index vectors: ... | active rows | targets | mask | weights | vid (host criterion), ... | vid (device)
    host, N, S = f._keep[2], b.n_events, b.S
    assert np.array_equal(host[-N:], b.vid)
    if not device_criterion:
        o0 = (3 + S) * N + f.last_active_rows
        assert host.size == o0 + 3 * N * S + N
        assert np.array_equal(host[o0:o0 + N * S], b.targets[:, :S].numpy().reshape(-1))
        assert np.array_equal(host[o0 + N * S:o0 + 2 * N * S].view(np.float32), b.crit_masks[:, :S].numpy().reshape(-1))
        assert np.array_equal(host[o0 + 2 * N * S:o0 + 3 * N * S].view(np.float32), b.criterion_weights().reshape(-1))
    else:
        assert host.size == (3 + S) * N + N


@pytest.mark.parametrize('case', ['vbctx', 'vb16'])
def test_fused_batch_one_step_matches_clamp_adam_on_the_summed_gradient(case):
    """ONE clamp, ONE Adam step on the SUM of the videos' gradients (m_batch = V): parameters and both moments against the oracle's
    clamp_adam_step (the gates of tests/test_gpu_timed_path.py's one-step test)."""
    from oracle import echr_ref_cpu as O
    opt, params, vids = synth.make_vbatch(case)
    lr, clip = 1e-3, 100.0
    m, o, f = _fused(opt, params, lr=lr, clip=clip)
    b, _ = _batch(vids)
    loss = float(f.batch(b))
    torch.cuda.synchronize()
    ref = _ref(case, True)
    assert abs(loss - ref['loss']) < TOL_LOSS * abs(ref['loss'])
    assert o._flat['step'] == 1
    ar = m._echr_arena
    tol = tol_grad(case)
    for i, (k, p) in enumerate(m.named_parameters()):
        assert ar.params[i] is p
        lo, n = ar.offsets[i], p.numel()
        mom = o._flat['m'][lo:lo + n].view(p.shape).cpu().numpy()
        var = o._flat['v'][lo:lo + n].view(p.shape).cpu().numpy()
        new = p.detach().cpu().numpy()
        rg = ref['grads'][k]
        if rg is None:
            assert np.array_equal(new, params[k]) and not mom.any() and not var.any(), k
            continue
        rp, rm, rv = (torch.from_numpy(x.copy()) for x in (params[k], np.zeros_like(params[k]), np.zeros_like(params[k])))
        O.clamp_adam_step(rp, torch.from_numpy(rg), rm, rv, 1, lr, clip=clip)
        if k in U.NOISE_ONLY:
            assert np.abs(new - params[k]).max() <= 1.01 * lr
            continue
        assert U.grad_close(k, mom, rm.numpy(), tol), (k, 'exp_avg', U.relerr(mom, rm.numpy()))
        assert np.abs(var - rv.numpy()).max() <= 2.5 * tol * max(float(rv.max()), 1e-3 * U.GRAD_FLOOR ** 2) + 1e-20, (k, 'exp_avg_sq')
        dgpu, dref = new - params[k], rp.numpy() - params[k]
        assert np.abs(dgpu).max() <= 1.01 * lr and np.abs(dgpu - dref).max() <= 2.01 * lr, k
        solid = np.abs(rg) > 1e-4 * float(np.abs(rg).max())
        if solid.any():
            assert np.abs(dgpu - dref)[solid].max() < 0.02 * lr, (k, np.abs(dgpu - dref)[solid].max() / lr)


@pytest.mark.parametrize('train_mode', [False, True])
def test_fused_batch_forward_only_loss(train_mode):
    opt, params, vids = synth.make_vbatch('vbctx')
    m, o, f = _fused(opt, params, train_mode)
    b, _ = _batch(vids)
    loss = float(f.batch(b, forward_only=True))
    ref = _ref('vbctx', train_mode)
    assert abs(loss - ref['loss']) < TOL_LOSS * abs(ref['loss']), (loss, ref['loss'])
    assert np.abs(f.last_video_losses.cpu().numpy() - ref['losses']).max() < TOL_LOSS * np.abs(ref['losses']).max()
    assert o._flat is None or o._flat['step'] == 0
    assert all(p.grad is None for p in m.parameters())


def test_unfused_criterion_keeps_the_weighted_loss():
    """forward_only (the criterion is then not fused behind the logits): the batched step without per-video losses returns the per-video
    sum, and the reward-weighted single-video step (echr_train_step_rw) returns sum(-logp[target] * w) / sum(mask), not the masked NLL."""
    from echr_amd import _lib as L
    opt, params, vids = synth.make_vbatch('vbctx')
    m, o, f = _fused(opt, params, False)
    b, _ = _batch(vids)
    loss = float(f.batch(b, forward_only=True, video_losses=False))
    ref = _ref('vbctx', False)
    assert f.last_video_losses is None
    assert abs(loss - ref['loss']) < TOL_LOSS * abs(ref['loss']), (loss, ref['loss'])
    # the single-video weighted step on video 0, eval mode, signed weights
    vid = vids[0]
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels, masks = torch.from_numpy(vid['labels']), vid['masks'][:, 1:]
    with torch.no_grad():
        logp = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train').cpu().numpy()
    S = logp.shape[1]
    w = (np.random.RandomState(5).uniform(-1, 1, size=(len(labels), S)).astype(np.float32) * masks[:, :S]).astype(np.float32)
    slot, _ = f._setup(tap, c3d, lda, labels, vid['ind'], vid['soi'], vid['labels'][:, 1:], masks, False, True, None, False, weights=w)
    f.a.prepared = f.a.handover = 0
    L.check(f.lib.echr_train_step_rw(C.byref(f.a), None, L.stream_ptr()), 'train_step_rw')
    torch.cuda.synchronize()
    nll = -np.take_along_axis(logp.astype(np.float64), vid['labels'][:, 1:1 + S][:, :, None], 2)[:, :, 0]
    want = float((nll * w).sum() / masks[:, :S].sum())
    assert abs(float(slot[0]) - want) < 1e-5 * abs(want) + 1e-7, (float(slot[0]), want)
    assert abs(float(slot[1]) - float(masks[:, :S].sum())) < 1e-3


def _sequential_logp(m, vids):
    dev = torch.device('cuda')
    out = []
    with torch.no_grad():
        for v in vids:
            tap, c3d, lda = (torch.from_numpy(v[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
            out.append(m(tap, c3d, lda, torch.from_numpy(v['labels']), v['ind'], v['soi'], mode='train').cpu().numpy())
    return out


@pytest.mark.parametrize('case', ['vbctx', 'vb16', 'vb33'])
def test_eval_batch_equals_sequential_single_video_calls(case):
    """Eval mode: the batched log-probs against V sequential CaptionGenerator.forward calls of the unchanged path (two HIP results: twice the
    log-prob gate).  vb33: 132 events -- the event encoder's row-softmax kernel and the launch-per-phase recurrences."""
    opt, params, vids = synth.make_vbatch(case)
    m = U.build_gpu_model(opt, params, False)
    b, _ = _batch(vids)
    with torch.no_grad():
        logp = m.forward_batch(b, mode='train').cpu().numpy()
    seq = _sequential_logp(m, vids)
    for v, s in enumerate(b.event_slices):
        assert np.abs(logp[s, :seq[v].shape[1]] - seq[v]).max() <= 2 * TOL_LOGP, v


def test_single_video_batch_equals_the_legacy_call():
    """V = 1 on case_c1: forward_batch against the oracle at the legacy gates and against forward(); FusedTrainStep.batch of one video
    against FusedTrainStep.__call__."""
    opt, params, vid = synth.make_case('c1')
    got = _module_pass(opt, params, [vid], True)
    rlogp, rloss, rgrads = U.run_oracle(opt, params, vid, True)
    assert np.abs(got['logp'] - rlogp).max() < TOL_LOGP
    assert abs(got['loss'] - rloss) < TOL_LOSS * abs(rloss)
    for k, g in rgrads.items():
        if g is not None:
            assert U.grad_close(k, got['grads'][k], g, 1e-5), (k, U.relerr(got['grads'][k], g))
    legacy = U.run_gpu(opt, params, vid, True)
    assert np.abs(got['logp'] - legacy[0]).max() <= 2 * TOL_LOGP
    # the one-call step
    dev = torch.device('cuda')
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    ma, oa, fa = _fused(opt, params)
    b, _ = _batch([vid])
    la = float(fa.batch(b, step=False))
    mb, ob, fb = _fused(opt, params)
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    lb = float(fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], step=False))
    torch.cuda.synchronize()
    assert abs(la - lb) < TOL_LOSS * abs(lb) and abs(la - rloss) < TOL_LOSS * abs(rloss)
    assert abs(float(fa.last_video_losses[0]) - lb) < TOL_LOSS * abs(lb)
    ga, gb = _grads(ma), _grads(mb)
    for k, g in gb.items():
        if g is not None:
            assert U.grad_close(k, ga[k], g, 2e-5), (k, U.relerr(ga[k], g))


@pytest.mark.parametrize('case', ['vbctx', 'vb16'])
def test_greedy_decode_of_a_batch(case):
    """`seq` bit-exact against the reference's per-video sequences (a video that stops earlier than the batch is zero padded), log-probs
    within the log-prob gate."""
    g = U.gold('case_vbatch.npz')
    opt, params, vids = synth.make_vbatch(case)
    m = U.build_gpu_model(opt, params, False)
    b, _ = _batch(vids, labels=False)
    with torch.no_grad():
        seq, logp = m.forward_batch(b, mode='eval')
    seq, logp = seq.cpu().numpy(), logp.cpu().numpy()
    T = max(g[case + '|sample|seq|v%02d' % v].shape[1] for v in range(len(vids)))
    assert seq.shape == (b.n_events, T)
    for v, s in enumerate(b.event_slices):
        want, wlp = g[case + '|sample|seq|v%02d' % v], g[case + '|sample|logp|v%02d' % v]
        Tv = want.shape[1]
        assert np.array_equal(seq[s, :Tv], want) and not seq[s, Tv:].any(), v
        assert np.abs(logp[s, :Tv] - wlp).max() < TOL_LOGP, v


def test_more_than_64_events_takes_the_launch_per_phase_path():
    """24 videos x 4 events = 96 rows: launch-per-phase recurrences, the event encoder's general softmax kernel."""
    opt, params, vids = synth.make_vbatch('vb24')
    got = _module_pass(opt, params, vids, True, arena=True)
    assert got['batch'].n_events == 96
    _check_vs_ref('vb24', got, _ref('vb24', True))
    m, o, f = _fused(opt, params)
    b, _ = _batch(vids)
    loss = float(f.batch(b, step=False))
    torch.cuda.synchronize()
    ref = _ref('vb24', True)
    assert abs(loss - ref['loss']) < TOL_LOSS * abs(ref['loss'])
    _check_grads('vb24', _grads(m), ref)


def _persist_launches(fn):
    from echr_amd import _lib as L
    lib = L.load()
    L.check(lib.echr_prof_enable(1), 'prof_enable')
    try:
        out = fn()
        torch.cuda.synchronize()
        ms, fl, by, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        L.check(lib.echr_prof_read(9, C.byref(ms), C.byref(fl), C.byref(by), C.byref(n)), 'prof_read')
    finally:
        L.check(lib.echr_prof_enable(0), 'prof_enable')
    return out, int(n.value)


def test_sixteen_videos_take_the_persistent_recurrences_and_fixed_order_mode_is_bitwise():
    import echr_amd
    opt, params, vids = synth.make_vbatch('vb16')
    m, o, f = _fused(opt, params)
    b, _ = _batch(vids)
    assert b.n_events <= 64
    _, launches = _persist_launches(lambda: f.batch(b, step=False))
    assert launches >= 2, launches                 # the forward and the reverse persistent launch (counted, not inferred from time)
    ref = _ref('vb16', True)
    runs = []
    echr_amd.set_deterministic(True)
    try:
        for _ in range(2):
            m2, o2, f2 = _fused(opt, params)
            (loss, n2) = _persist_launches(lambda: float(f2.batch(b, step=False)))
            assert n2 == 0                          # fixed-order mode runs launch per phase
            runs.append((loss, f2.last_video_losses.cpu().numpy(), _grads(m2)))
    finally:
        echr_amd.set_deterministic(False)
    (la, va, ga), (lb, vb, gb) = runs
    assert la == lb and np.array_equal(va, vb)
    for k, v in ga.items():
        assert (v is None and gb[k] is None) or np.array_equal(v, gb[k]), k
    assert abs(la - ref['loss']) < TOL_LOSS * abs(ref['loss'])
    _check_grads('vb16', ga, ref)


def test_cross_video_isolation_is_bitwise():
    """Scaling ONE video's features by 10 changes no other video's log-prob row: bit-identical in eval mode under the fixed-order mode (rows
    of different videos share no data-dependent quantity: block-diagonal softmax, per-video scene vector, row-wise products)."""
    import echr_amd
    opt, params, vids = synth.make_vbatch('vbctx')
    m = U.build_gpu_model(opt, params, False)
    hot = 1
    scaled = [dict(v) for v in vids]
    for k in ('c3d', 'tap', 'lda'):
        scaled[hot][k] = (vids[hot][k] * np.float32(10.0)).astype(np.float32)
    echr_amd.set_deterministic(True)
    try:
        with torch.no_grad():
            b0, _ = _batch(vids)
            b1, _ = _batch(scaled)
            a = m.forward_batch(b0, mode='train').cpu().numpy()
            c = m.forward_batch(b1, mode='train').cpu().numpy()
    finally:
        echr_amd.set_deterministic(False)
    for v, s in enumerate(b0.event_slices):
        if v == hot:
            assert not np.array_equal(a[s], c[s])
        else:
            assert np.array_equal(a[s], c[s]), v


def test_call_order_does_not_matter():
    """Nothing of one call survives into the next: six calls on 'vbctx' (5 videos incl. a one-event video, 'VLVCVH' scene vectors), computed
    once and then again in another order, every result bit-equal to its first value -- a single-video call behind a batched one runs as a
    single-video call, a batched one behind the per-row scene form (sample_train_batch) as the plain batched one, and so on.
    (a) eval forward of video 0, single-video entry; (b) eval forward of the batch; (c) greedy decode of the batch; (d) sample_train_batch,
    fixed seed and dropout state; (e) greedy decode of video 0; (f) the gradient arena of FusedTrainStep.batch(step=False).
    The decode chains are bitwise reproducible by construction, but the event encoder in front of them, the teacher-forced forward and the
    backward sum with atomics in the default mode: the whole test runs in the fixed-order mode, where two runs on the same inputs agree bit for
    bit (the rule of test_cross_video_isolation_is_bitwise; the greedy decodes take the same persistent launches in either mode)."""
    import echr_amd
    from echr_amd import functional as EF
    opt, params, vids = synth.make_vbatch('vbctx')
    m, o, f = _fused(opt, params, False)
    b, _ = _batch(vids)
    dev = torch.device('cuda')
    v0 = vids[0]
    tap, c3d, lda = (torch.from_numpy(v0[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    one = (tap, c3d, lda, torch.from_numpy(v0['labels']), v0['ind'], v0['soi'])
    lm = m.lm_model

    def host(xs):
        torch.cuda.synchronize()
        xs = xs if isinstance(xs, (tuple, list)) else (xs,)
        return tuple(x.detach().cpu().numpy().copy() if isinstance(x, torch.Tensor) else np.asarray(x).copy() for x in xs)

    def no_grad(fn):
        with torch.no_grad():
            return host(fn())

    def grad_arena():
        loss = f.batch(b, step=False)
        return host((loss, f.last_video_losses, m._echr_arena.flat_g))

    echr_amd.set_deterministic(True)
    try:
        with torch.no_grad():
            video, event, ev_start, ev_len, A, vid, drop = m._batch_contexts(b, None)
        drop.training = True          # (the sampled pass of training: the decoder's dropout under this one state, every time)
        sample_args = (video, event, b.clip_rows(), ev_start, ev_len, vid, A, lm.seq_length, lm.native_params(), drop)
        calls = {'a': lambda: no_grad(lambda: m(*one, mode='train')),
                 'b': lambda: no_grad(lambda: m.forward_batch(b, mode='train')),
                 'c': lambda: no_grad(lambda: m.forward_batch(b, mode='eval')),
                 'd': lambda: no_grad(lambda: EF.sample_train_batch(*sample_args, seed=1234)),
                 'e': lambda: no_grad(lambda: m(*one, mode='eval')),
                 'f': grad_arena}
        first = {k: calls[k]() for k in 'abcdef'}
        assert first['c'][0].any() and first['d'][0].any() and first['e'][0].any() and first['f'][2].any()
        for k in 'dafecba':
            again = calls[k]()
            assert len(again) == len(first[k])
            for i, (x, y) in enumerate(zip(first[k], again)):
                assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), (k, i)
    finally:
        echr_amd.set_deterministic(False)

"""The non-zero initial decoder state (CG_init_feats_type) over a multi-video batch on the GPU (-m gpu): echr_init_state_fwd_batch /
_bwd_batch alone against numpy, then CaptionGenerator.forward_batch / beam_batch / train_rl_batch, FusedTrainStep.batch / batch_handover /
_batch_tap, JointBatchStep, SelfCriticalBatchStep and eval_utils.caption_videos(_beam) against the CPU reference of the contract
(tests/init_batch_ref.py: the oracle once per video with init_feats_type, losses and gradients summed, sliced dropout masks), the
reference's own fixture (tests/golden/case_init_batch.npz) and the single-video path.

Gates: the project's own (tests/test_gpu_clip_batch.py, tests/test_gpu_vbatch.py) -- log-probs 2e-5 absolute, loss 1e-5 relative, index
outputs bit-exact (beam results against the oracle for events whose ORACLE margin is >= 1e-4, as in tests/test_gpu_clipctx.py, counted; and
EVERY beam row against the single-video HIP decode of its video), each gradient tensor
and d tap max(1e-5, 4 * e_ref) of its max-norm (+1e-9 absolute).  e_ref is the float32-vs-float64 difference of init_batch_ref on the same
case, measured on the CPU (init_batch_ref.e_ref; worst parameter gradient / worst video's d tap):

    vbinit    eval 1.5e-06 / 8.6e-07   train 1.1e-06 / 6.6e-07
    vbinitch  eval 1.1e-06 / 5.7e-07   train 8.7e-07 / 7.7e-07
    vbinit33  eval 1.1e-06 / 9.5e-07   train 1.0e-06 / 8.5e-07

so 4 * e_ref stays below 1e-5 everywhere and the gate is the plain 1e-5.  Two HIP GRADIENT results compared with each other (batch
against single-video steps, one-call against module path) each carry that error: twice the gradient gate, as tests/test_gpu_vbatch.py
does.  The eval rows of a batch against the single-video forward are held to the plain TOL_LOGP.  The kernel
pair alone is compared with float64 numpy on O(1) inputs at 1e-5 of each tensor's max-norm (fp32 sums of at most 60 terms)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from echr_amd import functional as EF
from echr_amd import synth
from oracle import summary as SM
from tests import init_batch_ref as R
from tests import joint_batch_ref as J
from tests import util as U
from tests import vbatch_ref as VR

pytestmark = pytest.mark.gpu

TOL_LOGP = 2e-5
TOL_LOSS = 1e-5
E_REF = {'vbinit': 1.54e-6, 'vbinitch': 1.14e-6, 'vbinit33': 1.10e-6}          # worst tensor, either mode (header)
BEAM_MARGIN = 1e-4
BEAM_MIN_GATED = {'vbinit': 9, 'vbinitch': 11}          # events whose oracle beam margin is >= 1e-4 (of 10 / 13), measured on the CPU
UNUSED = {'lm_model.core.fusion_layer.weight', 'lm_model.core.fusion_layer.bias', 'fusion_model.h2a_layer.weight', 'fusion_model.h2a_layer.bias'}
KEYS = ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')
INIT = ('lm_model.init_linear.weight', 'lm_model.init_linear.bias')


def tol_grad(case):
    return max(1e-5, 4 * E_REF[case])


def _dev():
    return torch.device('cuda')


@functools.lru_cache(maxsize=None)
def _case(case):
    return synth.make_vbatch(case)


@functools.lru_cache(maxsize=None)
def _ref(case, train_mode):
    opt, params, vids = _case(case)
    return R.run(opt, params, vids, train_mode)


def _batch(opt, vids, tap_leaves=False, labels=True):
    from echr_amd.batch import VideoBatch
    taps = [torch.from_numpy(v['tap']).to(_dev()).requires_grad_(tap_leaves) for v in vids]
    keys = ('c3d', 'lda', 'ind', 'soi') + (('labels', 'masks') if labels else ())
    b = VideoBatch.from_videos([dict({k: v[k] for k in keys}, tap=t) for v, t in zip(vids, taps)], device=_dev(),
                               CG_init_feats_type=opt.CG_init_feats_type, clip_context_type=opt.clip_context_type)
    return b, taps


def _grads(m):
    return {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}


def _arena_grads(model):
    ar = model._echr_arena
    out = {}
    for i, (k, p) in enumerate(model.named_parameters()):
        assert ar.params[i] is p
        gv = ar.grad_view(i).detach().cpu().numpy().copy()
        if k in UNUSED:
            assert not gv.any(), k
            gv = None
        out[k] = gv
    return out


def _check_grads(grads, ref_grads, tol):
    for k in INIT:
        assert ref_grads[k] is not None and grads[k] is not None and np.any(grads[k]), k
    for k, g in ref_grads.items():
        if g is None:
            assert grads[k] is None or not np.any(grads[k]), k
            continue
        print('%-55s rel err %.2e' % (k, U.relerr(grads[k], g, U.GRAD_FLOOR)))
        assert U.grad_close(k, grads[k], g, tol), (k, U.relerr(grads[k], g))


def _check_g_tap(got, ref_g_tap, row_offset, tol, scale=1.0):
    for v, r in enumerate(ref_g_tap):
        a, r = got[int(row_offset[v]):int(row_offset[v + 1])], scale * r
        print('d tap video %d: rel err %.2e' % (v, U.relerr(a, r, U.GRAD_FLOOR)))
        assert np.abs(a - r).max() <= tol * max(float(np.abs(r).max()), U.GRAD_FLOOR) + 1e-9, (v, U.relerr(a, r))


def _check_losses(loss, per, ref):
    assert abs(loss - ref['loss']) < TOL_LOSS * abs(ref['loss']), (loss, ref['loss'])
    assert np.abs(per - ref['losses']).max() < TOL_LOSS * np.abs(ref['losses']).max()


# ---- 1. the kernel pair alone -------------------------------------------------------------------------------------------------------
def _np_init(use, video, event, c3d, ev_start, ev_len, vid, w, b, g_h0):
    """float64 numpy: (h0, video_len, g_w, g_b, g_video, g_event) of the contract."""
    f8 = lambda x: np.asarray(x, np.float64)
    video, event, c3d, w, b, g_h0 = map(f8, (video, event, c3d, w, b, g_h0))
    V, N = video.shape[0], event.shape[0]
    vlen = np.asarray([ev_len[vid == v].max() for v in range(V)], np.int64)
    parts = []
    if use[0]:
        parts.append(video[vid])
    if use[1]:
        parts.append(event)
    if use[2]:
        parts.append(np.stack([c3d[s:s + l].sum(0) / vlen[v] for s, l, v in zip(ev_start, ev_len, vid)]))
    feats = np.concatenate(parts, 1)
    h0 = feats @ w.T + b
    dfeats = g_h0 @ w
    Dv, De = video.shape[1], event.shape[1]
    g_video = np.stack([dfeats[vid == v, :Dv].sum(0) for v in range(V)]) if use[0] else None
    o = Dv if use[0] else 0
    g_event = dfeats[:, o:o + De] if use[1] else None
    return h0, vlen, g_h0.T @ feats, g_h0.sum(0), g_video, g_event


def _kernel_case(counts, lens, Dv=7, De=10, D=13, H3=96, seed=3):
    """Videos of counts[v] events with the given event lengths (flat list); feature widths that are no multiple of 4."""
    rs = np.random.RandomState(seed)
    vid = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    ev_len = np.asarray(lens, np.int32)
    T = 12 * len(counts)
    ev_start = np.asarray([12 * v + rs.randint(0, 12 - l + 1) for v, l in zip(vid, ev_len)], np.int32)          # rows of the event's own video
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    return dict(vid=vid, ev_len=ev_len, ev_start=ev_start, video=f(len(counts), Dv), event=f(len(vid), De), c3d=f(T, D), H3=H3)


def _run_kernels(k, use, seed=11):
    rs = np.random.RandomState(seed)
    dev = _dev()
    Dtot = (k['video'].shape[1] if use[0] else 0) + (k['event'].shape[1] if use[1] else 0) + (k['c3d'].shape[1] if use[2] else 0)
    w = (rs.standard_normal((k['H3'], Dtot)) / np.sqrt(Dtot)).astype(np.float32)
    b = rs.standard_normal(k['H3']).astype(np.float32)
    g_h0 = rs.standard_normal((len(k['vid']), k['H3'])).astype(np.float32)
    t = lambda x, g=False: torch.from_numpy(x).to(dev).requires_grad_(g)
    video, event, wt, bt = t(k['video'], True), t(k['event'], True), t(w, True), t(b, True)
    args = (t(k['c3d']), t(k['ev_start']), t(k['ev_len']), t(k['vid']))
    h0 = EF.InitState.apply(video, event, *args[:3], 0, args[3], use, None, wt, bt)
    vlen = h0.grad_fn.video_len.cpu().numpy() if use[2] else None          # the padded clip lengths the device formed ('C' only)
    h0.backward(t(g_h0))
    torch.cuda.synchronize()
    got = dict(video_len=vlen, h0=h0.detach().cpu().numpy(), g_w=wt.grad.cpu().numpy(), g_b=bt.grad.cpu().numpy(),
               g_video=video.grad.cpu().numpy() if video.grad is not None else None,
               g_event=event.grad.cpu().numpy() if event.grad is not None else None)
    want = _np_init(use, k['video'], k['event'], k['c3d'], k['ev_start'], k['ev_len'], k['vid'], w, b, g_h0)
    return got, want, (w, b, g_h0)


def _close(a, r, what):
    err = float(np.abs(a - r).max())
    print('%-8s max err %.2e of %.2e' % (what, err, float(np.abs(r).max())))
    assert err <= 1e-5 * max(float(np.abs(r).max()), 1e-3), (what, err)


@pytest.mark.parametrize('use', [(True, False, False), (False, True, False), (False, False, True), (True, True, True)],
                         ids=['V', 'E', 'C', 'VEC'])
def test_init_state_batch_kernels_match_numpy(use):
    """Four videos of 3 / 1 / 2 / 4 events: a one-event video, a video whose longest event is ONE row (its divisor is 1), widths 7 / 10 / 13
    (no multiple of 4), per-video longest events 9 / 5 / 1 / 12."""
    k = _kernel_case([3, 1, 2, 4], [9, 2, 4, 5, 1, 1, 12, 3, 7, 1])
    got, want, _ = _run_kernels(k, use)
    h0, vlen, g_w, g_b, g_video, g_event = want
    assert vlen.tolist() == [9, 5, 1, 12]
    if use[2]:
        assert got['video_len'].tolist() == [9, 5, 1, 12]          # video_max_len_kernel's own output
    _close(got['h0'], h0, 'h0')
    _close(got['g_w'], g_w, 'd W')
    _close(got['g_b'], g_b, 'd b')
    if use[0]:
        _close(got['g_video'], g_video, 'd video')
    else:
        assert got['g_video'] is None
    if use[1]:
        _close(got['g_event'], g_event, 'd event')
    else:
        assert got['g_event'] is None


def test_one_video_batch_is_bit_equal_to_the_single_video_entry():
    k = _kernel_case([5], [9, 2, 12, 5, 1])
    dev = _dev()
    rs = np.random.RandomState(5)
    Dtot = 7 + 10 + 13
    w = torch.from_numpy((rs.standard_normal((k['H3'], Dtot)) / np.sqrt(Dtot)).astype(np.float32)).to(dev)
    b = torch.from_numpy(rs.standard_normal(k['H3']).astype(np.float32)).to(dev)
    t = lambda x: torch.from_numpy(x).to(dev)
    use = (True, True, True)
    with torch.no_grad():
        one = EF.InitState.apply(t(k['video'][0]), t(k['event']), t(k['c3d']), t(k['ev_start']), t(k['ev_len']), int(k['ev_len'].max()), None, use, None, w, b)
        bat = EF.InitState.apply(t(k['video']), t(k['event']), t(k['c3d']), t(k['ev_start']), t(k['ev_len']), 0, t(k['vid']), use, None, w, b)
    assert torch.equal(one, bat)


def test_d_video_is_bitwise_reproducible_in_deterministic_mode():
    import echr_amd
    k = _kernel_case([3, 1, 2, 4], [9, 2, 4, 5, 1, 1, 12, 3, 7, 1])
    echr_amd.set_deterministic(True)
    try:
        runs = [_run_kernels(k, (True, True, True))[0] for _ in range(2)]
    finally:
        echr_amd.set_deterministic(False)
    assert np.array_equal(runs[0]['g_video'], runs[1]['g_video']) and np.array_equal(runs[0]['h0'], runs[1]['h0'])
    assert np.array_equal(runs[0]['g_event'], runs[1]['g_event'])


# ---- 2. module path ---------------------------------------------------------------------------------------------------------------
def _module_pass(case, train_mode):
    """forward_batch(mode='train') + the per-video criterion + backward with every video's tap_feats as a leaf, arena on."""
    from echr_amd.misc.utils import LanguageModelCriterion
    opt, params, vids = _case(case)
    m = U.build_gpu_model(opt, params, train_mode)
    m.build_arena()
    b, taps = _batch(opt, vids, True)
    logp = m.forward_batch(b, mode='train')
    total, per = b.criterion(LanguageModelCriterion(), logp)
    total.backward()
    torch.cuda.synchronize()
    assert all(t.grad is not None for t in taps)
    return dict(logp=logp.detach().cpu().numpy(), loss=float(total.detach()), losses=per.detach().cpu().numpy(), grads=_grads(m),
                g_tap=np.concatenate([t.grad.cpu().numpy() for t in taps], 0), batch=b, model=m)


def _check_vs_ref(case, got, ref):
    b, logp = got['batch'], got['logp']
    assert logp.shape[0] == b.n_events and logp.shape[1] == b.S
    for v, s in enumerate(b.event_slices):
        Sv = ref['logp'][v].shape[1]
        assert Sv == b.steps[v]
        d = float(np.abs(logp[s, :Sv] - ref['logp'][v]).max())
        print('video %d: max |d logp| %.2e' % (v, d))
        assert d < TOL_LOGP, (v, d)
    _check_losses(got['loss'], got['losses'], ref)
    _check_grads(got['grads'], ref['grads'], tol_grad(case))
    _check_g_tap(got['g_tap'], ref['g_tap'], b.row_offset, tol_grad(case))


def _check_vs_fixture(case, mode, got):
    g = U.gold('case_init_batch.npz')
    key = case + '|' + mode
    tol = tol_grad(case)
    b = got['batch']
    cols, tcols = SM.logp_columns(got['logp'].shape[2]), SM.logp_columns(b.tap.shape[1])
    for v, s in enumerate(b.event_slices):
        want = g[key + '|logp|v%02d' % v]
        assert np.abs(got['logp'][s, :want.shape[1]][:, :, cols] - want).max() < TOL_LOGP, v
        wt = g[key + '|gtap|v%02d' % v]
        a = got['g_tap'][int(b.row_offset[v]):int(b.row_offset[v + 1])][:, tcols]
        assert np.abs(a - wt).max() <= tol * max(float(np.abs(wt).max()), U.GRAD_FLOOR) + 1e-9, v
    assert abs(got['loss'] - float(g[key + '|loss'])) < TOL_LOSS * abs(float(g[key + '|loss']))
    assert np.abs(got['losses'] - g[key + '|losses']).max() < TOL_LOSS * np.abs(g[key + '|losses']).max()
    assert (key + '|grad|lm_model.init_linear.weight|linf') in g
    for k, v in got['grads'].items():
        if v is not None and k not in U.NOISE_ONLY and (key + '|grad|' + k + '|linf') in g:
            ref = float(g[key + '|grad|' + k + '|linf'])
            assert abs(float(np.abs(v).max()) - ref) <= tol * max(ref, U.GRAD_FLOOR) + 1e-9, k
            head, strided = SM.grad_slices(v)
            for a, want in ((head, g[key + '|grad|' + k + '|head']), (strided, g[key + '|grad|' + k + '|strided'])):
                assert np.abs(a - want).max() <= tol * max(ref, U.GRAD_FLOOR) + 1e-9, k


@pytest.mark.parametrize('case', ['vbinit', 'vbinitch'])
@pytest.mark.parametrize('train_mode', [False, True])
def test_module_path_matches_oracle_and_reference(case, train_mode):
    """Every log-prob, the summed loss, the per-video losses, every parameter gradient -- init_linear's over all rows of all videos -- and
    d batch.tap per video: with 'VH' init_linear's d video reaches each video's own rows beside the decoder's, the anchors' rows and (vbinitch)
    the attended rows."""
    got = _module_pass(case, train_mode)
    assert got['batch'].CG_init_feats_type == ('VEC' if case == 'vbinit' else 'VE')
    _check_vs_ref(case, got, _ref(case, train_mode))
    _check_vs_fixture(case, 'train' if train_mode else 'eval', got)


@pytest.mark.parametrize('train_mode', [False, True])
def test_module_path_132_rows_matches_oracle(train_mode):
    """33 videos x 4 events with 'VEC': the general event-encoder kernels, 33 different padded clip lengths."""
    got = _module_pass('vbinit33', train_mode)
    assert got['batch'].n_events == 132
    _check_vs_ref('vbinit33', got, _ref('vbinit33', train_mode))


@pytest.mark.parametrize('case', ['vbinit', 'vbinitch'])
def test_eval_rows_equal_the_single_video_forward(case):
    opt, params, vids = _case(case)
    m = U.build_gpu_model(opt, params, False)
    b, _ = _batch(opt, vids)
    with torch.no_grad():
        logp = m.forward_batch(b, mode='train').cpu().numpy()
        for v, s in enumerate(b.event_slices):
            d = b.video(v)
            one = m(d['tap'], d['c3d'], d['lda'], d['labels'], d['ind'], d['soi'], mode='train').cpu().numpy()
            err = float(np.abs(logp[s, :one.shape[1]] - one).max())
            print('video %d: batch rows vs single-video forward %.2e' % (v, err))
            assert err < TOL_LOGP, (v, err)


# ---- 3. one-call path -------------------------------------------------------------------------------------------------------------
def _fused(opt, params, train_mode=True, lr=1e-3, clip=100.0):
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    m = U.build_gpu_model(opt, params, train_mode)
    o = ClampAdam(m.parameters(), lr=lr, arena=m.build_arena())
    return m, o, FusedTrainStep(m, o, grad_clip=clip)


@pytest.mark.parametrize('case', ['vbinit', 'vbinitch', 'vbinit33'])
def test_fused_batch_gradients_then_one_step(case):
    """FusedTrainStep.batch(step=False): the summed loss, per-video losses and summed gradients, init_linear's included; then ONE clamp +
    Adam step against vbatch_ref.step on the oracle's sum."""
    opt, params, vids = _case(case)
    ref = _ref(case, True)
    m, o, f = _fused(opt, params)
    b, _ = _batch(opt, vids)
    loss = float(f.batch(b, step=False))
    torch.cuda.synchronize()
    assert 0 < f.last_active_rows < b.n_events * b.S
    _check_losses(loss, f.last_video_losses.cpu().numpy(), ref)
    _check_grads(_grads(m), ref['grads'], tol_grad(case))
    assert o._flat is None or o._flat['step'] == 0
    lr, clip = 1e-3, 100.0
    m, o, f = _fused(opt, params, lr=lr, clip=clip)
    loss = float(f.batch(b))
    torch.cuda.synchronize()
    assert abs(loss - ref['loss']) < TOL_LOSS * abs(ref['loss']) and o._flat['step'] == 1
    want_p, want_m, want_v = VR.step(params, ref['grads'], lr=lr, clip=clip)
    ar, tol = m._echr_arena, tol_grad(case)
    for i, (k, p) in enumerate(m.named_parameters()):
        lo, n = ar.offsets[i], p.numel()
        mom = o._flat['m'][lo:lo + n].view(p.shape).cpu().numpy()
        var = o._flat['v'][lo:lo + n].view(p.shape).cpu().numpy()
        new = p.detach().cpu().numpy()
        rg = ref['grads'][k]
        if rg is None:
            assert np.array_equal(new, params[k]) and not mom.any() and not var.any(), k
            continue
        if k in U.NOISE_ONLY:
            assert np.abs(new - params[k]).max() <= 1.01 * lr
            continue
        assert U.grad_close(k, mom, want_m[k], tol), (k, 'exp_avg', U.relerr(mom, want_m[k]))
        assert np.abs(var - want_v[k]).max() <= 2.5 * tol * max(float(want_v[k].max()), 1e-3 * U.GRAD_FLOOR ** 2) + 1e-20, (k, 'exp_avg_sq')
        dgpu, dref = new - params[k], want_p[k] - params[k]
        assert np.abs(dgpu).max() <= 1.01 * lr and np.abs(dgpu - dref).max() <= 2.01 * lr, k
        solid = np.abs(rg) > 1e-4 * float(np.abs(rg).max())
        if solid.any():
            assert np.abs(dgpu - dref)[solid].max() < 0.02 * lr, (k, np.abs(dgpu - dref)[solid].max() / lr)


def _tap_call(opt, params, vids, train_mode=True, g_loss=None):
    m, o, f = _fused(opt, params, train_mode)
    b, _ = _batch(opt, vids)
    g_tap = torch.zeros_like(b.tap)
    per = torch.zeros(b.n_videos, device=_dev())
    gl = None if g_loss is None else torch.full((1,), g_loss, device=_dev())
    loss = float(f._batch_tap(b, g_tap, b.dev('row_offset'), per, g_loss=gl, step=False))
    torch.cuda.synchronize()
    return loss, per.cpu().numpy(), g_tap.cpu().numpy(), _arena_grads(m), b, f


@pytest.mark.parametrize('case', ['vbinit', 'vbinitch'])
def test_batch_tap_call_fills_g_tap(case):
    """echr_train_step_batch_tap / _batch_clip with g_tap and an initial state: init_linear's d video goes through echr_seg_col_mean_bwd into
    each video's own rows ('VH') beside the decoder's; g_loss scales it like every other contribution."""
    opt, params, vids = _case(case)
    ref = _ref(case, True)
    loss, per, g_tap, grads, b, f = _tap_call(opt, params, vids)
    _check_losses(loss, per, ref)
    _check_grads(grads, ref['grads'], tol_grad(case))
    _check_g_tap(g_tap, ref['g_tap'], b.row_offset, tol_grad(case))
    if case == 'vbinit':
        loss2, per2, g_tap2, grads2, _, _ = _tap_call(opt, params, vids, g_loss=0.5)
        assert abs(loss2 - loss) < TOL_LOSS * abs(loss)
        _check_g_tap(g_tap2, ref['g_tap'], b.row_offset, tol_grad(case), scale=0.5)


def _tap_model(opt, sst_params, arena):
    from echr_amd import models
    from echr_amd.optim import ClampAdam
    tm = models.setup_tap(opt)
    tm.load_state_dict({k: torch.from_numpy(v) for k, v in sst_params.items()})
    tm = tm.to(_dev())
    tm.eval()
    return tm, (ClampAdam(tm.parameters(), lr=1e-9, arena=tm.build_arena()) if arena else None)


def test_joint_batch_step_equals_the_module_path():
    """'VEC' with the proposal encoder in the loop (eval mode): JointBatchStep on a list of video dicts -- it builds the batch for the model's
    initial state itself -- against SST.forward_batch + forward_batch('train') + autograd.  Two HIP results: twice the gradient gate."""
    from echr_amd.batch import VideoBatch
    from echr_amd.fused import JointBatchStep
    from echr_amd.misc import utils
    opt, params, sst_params, vids, tap_in = J.setup('vbinit')
    mk, lb, w1 = ([torch.from_numpy(t[i]).to(_dev()) for t in tap_in] for i in range(3))
    rows = J.row_offsets(vids)
    m2 = U.build_gpu_model(opt, params, False)
    tm2, _ = _tap_model(opt, sst_params, False)
    c3d_all = torch.cat([torch.from_numpy(v['c3d']) for v in vids], 0).to(_dev())
    tap_all, scores = tm2.forward_batch(c3d_all, rows)
    b2 = VideoBatch.from_videos([dict({k: v[k] for k in KEYS}, tap=tap_all[rows[i]:rows[i + 1]]) for i, v in enumerate(vids)], device=_dev(),
                                CG_init_feats_type='VEC')
    cg, cg_per = b2.criterion(utils.LanguageModelCriterion(), m2.forward_batch(b2, mode='train'))
    tl, tl_per = utils.tap_criterion_batch(utils.TAPModelCriterion(), scores, torch.cat(mk, 0), torch.cat(lb, 0), w1, rows)
    (J.LAMBDA1 * tl + cg).backward()
    torch.cuda.synchronize()
    cg, tl = cg.detach(), tl.detach()
    m, o, f = _fused(opt, params, False, lr=1e-9, clip=None)
    tm, to = _tap_model(opt, sst_params, True)
    js = JointBatchStep(f, tm, to, lambda1=J.LAMBDA1, lambda2=1.0)
    loss = js([{k: v[k] for k in KEYS} for v in vids], mk, lb, w1, step=False)
    torch.cuda.synchronize()
    assert js.last_batch.CG_init_feats_type == 'VEC'
    assert abs(float(js.cg_loss) - float(cg)) < 2 * TOL_LOSS * abs(float(cg)) and abs(float(js.tap_loss) - float(tl)) < 2 * TOL_LOSS * abs(float(tl))
    assert abs(float(loss) - float(J.LAMBDA1 * tl + cg)) < 2 * TOL_LOSS * abs(float(cg))
    tol = 2 * tol_grad('vbinit')
    ar = tm._echr_arena
    for i, ((k, p), (_, p2)) in enumerate(zip(tm.named_parameters(), tm2.named_parameters())):
        got, want = ar.grad_view(i).detach().cpu().numpy(), p2.grad.cpu().numpy()
        print('sst %-30s rel err %.2e' % (k, U.relerr(got, want, U.GRAD_FLOOR)))
        assert np.abs(got - want).max() <= tol * max(float(np.abs(want).max()), U.GRAD_FLOOR) + 1e-9, (k, U.relerr(got, want))
    _check_grads(_arena_grads(m), _grads(m2), tol)
    # a ready batch built without the initial state is refused and names the keyword
    with pytest.raises(NotImplementedError, match='CG_init_feats_type='):
        js(VideoBatch.from_videos([dict({k: v[k] for k in KEYS}, tap=torch.from_numpy(v['tap'])) for v in vids], device=_dev()), mk, lb, w1)


@pytest.mark.parametrize('case', ['vbinit', 'vbinitch'])
def test_batch_handover_hands_final_ranges_and_init_linear_matches_the_plain_call(case):
    """batch_handover with a callback: a snapshot queued on the stream each hand-over point hands over is bit-equal to the final range
    (logit layer, LSTM layers); init_linear's slots lie in neither range and equal the plain batch(step=False) gradients."""
    import echr_amd
    opt, params, vids = _case(case)
    echr_amd.set_deterministic(True)          # the two calls are compared bit for bit
    try:
        m0, o0, f0 = _fused(opt, params)
        b, _ = _batch(opt, vids)
        f0.batch(b, step=False)
        torch.cuda.synchronize()
        plain = _arena_grads(m0)
        m, o, f = _fused(opt, params)
        ar, lm = f.arena, m.lm_model
        lstm = [p for k in range(3) for p in getattr(lm.core, 'layer%d' % k).parameters()]
        ranges = {}
        for which, ps in ((0, [lm.logit.weight, lm.logit.bias]), (1, lstm)):
            slots = sorted(ar.slot(p) for p in ps)
            assert slots == list(range(slots[0], slots[-1] + 1))
            ranges[which] = tuple(ar.span(slots))
        for p in (lm.init_linear.weight, lm.init_linear.bias):
            lo = ar.offsets[ar.slot(p)]
            assert all(not (r[0] <= lo < r[1]) for r in ranges.values())
        snaps, ext = {}, {}

        def cb(which, stream_ptr):
            lo, hi = ranges[which]
            st = ext.setdefault(stream_ptr, torch.cuda.ExternalStream(stream_ptr, device=_dev()))
            with torch.cuda.stream(st):
                snaps[which] = ar.flat_g[lo:hi].clone()
        f.batch_handover(b, cb)
        torch.cuda.synchronize()
        assert set(snaps) == {0, 1}
        for which, (lo, hi) in ranges.items():
            final = ar.flat_g[lo:hi]
            assert float(final.abs().max()) > 0 and torch.equal(snaps[which], final), which
        got = _arena_grads(m)
    finally:
        echr_amd.set_deterministic(False)
    for k in INIT:
        assert np.any(got[k]) and np.array_equal(got[k], plain[k]), k
    _check_grads(got, _ref(case, True)['grads'], tol_grad(case))


# ---- 4. decodes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['vbinit', 'vbinitch'])
def test_greedy_and_beam_decodes_equal_the_per_video_oracle(case):
    """forward_batch(mode='eval'): seq bit-exact against the reference's per-video sequences (the fixture; the oracle's are asserted equal
    on the CPU), log-probs within the gate.  beam_batch(B = 3), as one decode and as run-local row slices (max_rows = 12: h0 is sliced with
the rows): seq bit-exact against the oracle for every event whose oracle margin is >= 1e-4 (counted), and EVERY row's seq and width
    bit-exact (score within 1e-4) against the single-video HIP beam decode of its video, so the events the oracle cannot decide are pinned too."""
    g = U.gold('case_init_batch.npz')
    opt, params, vids = _case(case)
    m = U.build_gpu_model(opt, params, False)
    b, _ = _batch(opt, vids, labels=False)
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
    refs = R.beam(opt, params, vids, 3)
    gated = sum(int((np.asarray(r['margin']) >= BEAM_MARGIN).sum()) for r in refs)
    assert gated >= BEAM_MIN_GATED[case], gated
    singles = []
    with torch.no_grad():
        for v in range(b.n_videos):
            d = b.video(v)
            singles.append(m(d['tap'], d['c3d'], d['lda'], [], d['ind'], d['soi'], mode='eval', beam_size=3, return_score=True))
    for kw in (dict(), dict(max_rows=12)):
        bseq, blp, score, vw = m.beam_batch(b, 3, **kw)
        bseq, blp, score = bseq.cpu().numpy(), blp.cpu().numpy(), score.cpu().numpy()
        for v, (s, (sseq, slp, sscore)) in enumerate(zip(b.event_slices, singles)):          # all rows, against the single-video HIP decode
            w = 0 if isinstance(sseq, list) else sseq.shape[1]
            assert int(vw[v]) == w, (v, int(vw[v]), w)
            if w:
                assert np.array_equal(bseq[s, :w], sseq.cpu().numpy()), v
            assert not bseq[s, w:].any(), v
            ss = sscore.cpu().numpy()
            assert np.all(np.abs(score[s] - ss) <= 1e-4 * np.maximum(np.abs(ss), 1.0)), v
        for v, (s, r) in enumerate(zip(b.event_slices, refs)):
            ok = np.asarray(r['margin']) >= BEAM_MARGIN
            rseq, w = np.asarray(r['seq']), int(vw[v])
            if ok.all():
                assert w == int(np.asarray(r['words']).max()), (v, w)
            k = min(w, rseq.shape[1])
            assert np.array_equal(bseq[s, :k][ok], rseq[:, :k][ok]) and not bseq[s, w:].any(), v
            rs = np.asarray(r['score'])[ok]
            assert np.all(np.abs(score[s][ok] - rs) <= 1e-4 * np.maximum(np.abs(rs), 1.0)), v
    assert len(b.beam_groups(3, 12)) > 1


def test_greedy_decode_of_132_rows_equals_the_per_video_oracle():
    """vbinit33: the chain sampler over 132 rows from 33 videos' own initial states; seq bit-exact where the oracle's decode is decided by
    more than the log-prob gate at every step of the row, log-probs within the gate on those rows."""
    opt, params, vids = _case('vbinit33')
    m = U.build_gpu_model(opt, params, False)
    b, _ = _batch(opt, vids, labels=False)
    with torch.no_grad():
        seq, logp = m.forward_batch(b, mode='eval')
    seq, logp = seq.cpu().numpy(), logp.cpu().numpy()
    refs = R.sample(opt, params, vids)
    want = R.stack_sample(refs, vids)
    assert seq.shape == want.shape
    assert np.array_equal(seq, want)
    for (s_ref, lp_ref), s in zip(refs, b.event_slices):
        assert np.abs(logp[s, :lp_ref.shape[1]] - lp_ref.numpy()).max() < TOL_LOGP


def _rl_mask(gen, widths, vid):
    mask = np.zeros(gen.shape, dtype=bool)
    mask[:, 0] = True
    mask[:, 1:] = gen[:, :-1] > 0
    return mask & (np.arange(gen.shape[1])[None, :] < np.asarray(widths)[np.asarray(vid)][:, None])


@pytest.mark.parametrize('case', ['vbinit', 'vbinitch'])
def test_train_rl_batch_sample_equals_its_teacher_forced_recompute(case):
    """Dropout on: the log-probs the batched sampled decode emits from the batch's initial state equal train_rl_batch's teacher-forced
    recompute of the same draw under the same dropout state."""
    opt, params, vids = _case(case)
    m = U.build_gpu_model(opt, params, True)
    b, _ = _batch(opt, vids, labels=False)
    m.set_dropout_state(U.SEED, U.OFFSET)
    gen, slp_tf, greedy, vw = m.train_rl_batch(b, seed=1234)
    assert isinstance(gen, torch.Tensor) and gen.shape[1] > 0 and slp_tf.requires_grad
    m.set_dropout_state(U.SEED, U.OFFSET)
    lm = m.lm_model
    with torch.no_grad():
        video, event, ev_start, ev_len, A, vid, drop = m._batch_contexts(b, None)
        h0 = m._batch_initial_state(b, video, event, ev_start, ev_len, vid)
        assert h0 is not None and tuple(h0.shape) == (b.n_events, 3 * lm.rnn_size)
        gen2, slp, vw2 = EF.sample_train_batch(video, event, b.clip_rows(), ev_start, ev_len, vid, A, lm.seq_length, lm.native_params(), drop,
                                               seed=1234, h0=h0)
    assert torch.equal(gen, gen2) and np.array_equal(vw, vw2)
    g = gen.cpu().numpy()
    assert np.array_equal(vw, b.caption_widths(g)) and g.shape[1] == int(vw.max())
    mask = _rl_mask(g, vw, b.vid)
    err = np.abs(slp.cpu().numpy() - slp_tf.detach().cpu().numpy())[mask].max()
    print('sampled vs teacher-forced log-probs: %.2e' % err)
    assert err < TOL_LOGP, err
    assert isinstance(greedy, torch.Tensor) and greedy.shape[0] == b.n_events


def _no_dropout(m):
    m.fusion_model.enc_attn.dropout.p = 0.0
    c = m.lm_model.core
    c.dropout0.p = c.dropout1.p = c.dropout2.p = 0.0
    m.lm_model.dropout.p = 0.0


@pytest.mark.parametrize('case', ['vbinit', 'vbinitch'])
def test_self_critical_batch_step_equals_the_sum_of_single_video_steps(case):
    """Without dropout, on given captions of different widths per video and a signed reward: loss, per-video losses and the summed flat
    gradient (init_linear's slots included) against V SelfCriticalStep(step=False) calls.  Two HIP results: twice the gradient gate."""
    from echr_amd.fused import SelfCriticalBatchStep, SelfCriticalStep
    opt, params, vids = _case(case)
    rs = np.random.RandomState(7)
    N = sum(len(v['soi']) for v in vids)
    b, _ = _batch(opt, vids, labels=False)
    gen = np.zeros((N, 6), np.int64)
    for v, s in enumerate(b.event_slices):
        wv = 2 + (v % 4)
        for n in range(s.start, s.stop):
            ln = rs.randint(1, wv + 1)
            gen[n, :ln] = rs.randint(1, opt.CG_vocab_size + 1, size=ln)
        gen[s.start, :wv] = rs.randint(1, opt.CG_vocab_size + 1, size=wv)
    vw = b.caption_widths(gen)
    assert len(set(vw.tolist())) > 1
    T = int(vw.max())
    gen = gen[:, :T]
    reward = rs.uniform(-1, 1, size=(N, T)).astype(np.float32)
    m1, o1, f1 = _fused(opt, params, clip=None)
    _no_dropout(m1)
    sc1 = SelfCriticalStep(f1)
    total, flat, per = 0.0, torch.zeros_like(f1.arena.flat_g), []
    for v, (vid, s) in enumerate(zip(vids, b.event_slices)):
        tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
        w = int(vw[v])
        loss = sc1(tap, c3d, lda, vid['ind'], vid['soi'], gen_result=gen[s, :w], reward=reward[s, :w], step=False)[0]
        per.append(float(loss))
        total += float(loss)
        flat += f1.arena.flat_g
    m, o, f = _fused(opt, params, clip=None)
    _no_dropout(m)
    sc = SelfCriticalBatchStep(f)
    loss, _, _, _, vw2 = sc(b, gen_result=gen, reward=reward, step=False)
    torch.cuda.synchronize()
    assert np.array_equal(vw2, vw)
    assert abs(float(loss) - total) < 2 * TOL_LOSS * abs(total), (float(loss), total)
    assert np.abs(sc.last_video_losses.cpu().numpy() - np.asarray(per)).max() < 2 * TOL_LOSS * np.abs(per).max()
    ar, tol = f.arena, 2 * tol_grad(case)
    names = [k for k, _ in m.named_parameters()]
    seen_init = 0
    for i, p in enumerate(ar.params):
        lo, n = ar.offsets[i], p.numel()
        a, r = ar.flat_g[lo:lo + n], flat[lo:lo + n]
        scale = float(r.abs().max())
        if names[i] in U.NOISE_ONLY:
            assert float(a.abs().max()) < 1e-6
            continue
        if names[i] in INIT:
            seen_init += 1
            assert scale > 0
        assert float((a - r).abs().max()) <= tol * max(scale, U.GRAD_FLOOR) + 1e-9, (names[i], float((a - r).abs().max()), scale)
    assert seen_init == 2


# ---- the stream order of a returned d video -------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,tap_leaves,want', [('vbinit', True, 1), ('vbctx', True, 1), ('vbctx', False, 2), ('vbinit', False, 2)])
def test_d_video_wanted_keeps_the_lstm_stage_on_the_callers_stream(monkeypatch, case, tap_leaves, want):
    """The rule of functional._decoder_backward: d video is formed by the LSTM-layer stage, which async_tail = 2 puts on a helper stream that
    nobody joins before the scene mean's backward (or autograd's sum with InitStateBatch's d video) reads the returned tensor.  A node whose
    d video is wanted ('VH' with tap leaves) must therefore run echr_decoder_bwd_batch with async_tail = 1; every other arena node keeps 2.
    The form is read off the argument struct of the library call itself."""
    from echr_amd import _lib as L
    from echr_amd.batch import VideoBatch
    from echr_amd.misc.utils import LanguageModelCriterion
    lib = L.load()
    seen = []
    real = lib.echr_decoder_bwd_batch

    def spy(a, g, d, x, st):
        seen.append((int(g._obj.async_tail), bool(x._obj.g_video)))
        return real(a, g, d, x, st)
    opt, params, vids = _case(case)
    m = U.build_gpu_model(opt, params, True)
    m.build_arena()
    taps = [torch.from_numpy(v['tap']).to(_dev()).requires_grad_(tap_leaves) for v in vids]
    b = VideoBatch.from_videos([dict({k: v[k] for k in KEYS}, tap=t) for v, t in zip(vids, taps)], device=_dev(),
                               CG_init_feats_type=opt.CG_init_feats_type, clip_context_type=opt.clip_context_type)
    monkeypatch.setattr(lib, 'echr_decoder_bwd_batch', spy)
    total, _ = b.criterion(LanguageModelCriterion(), m.forward_batch(b, mode='train'))
    total.backward()
    torch.cuda.synchronize()
    assert seen == [(want, tap_leaves)], seen


# ---- 5. evaluation pass -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def eval_models():
    from echr_amd import models as EM
    _, params, _ = _case('vbinit')
    opt = synth.default_opt(**dict(synth.VBATCH['vbinit']['opt'], K=8))
    torch.manual_seed(3)
    tap = EM.setup_tap(opt)
    tap.eval()
    return opt, tap.cuda(), U.build_gpu_model(opt, params, False)


@pytest.mark.parametrize('beam', [None, 3])
def test_caption_videos_give_each_video_its_own_records(eval_models, beam):
    """caption_videos / caption_videos_beam build their batch for the model's initial state ('VEC'): three short videos get the records
    caption_video gives each alone (sentences and timestamps equal, confidences within 1e-3 as in tests/test_gpu_eval_batch.py)."""
    from echr_amd import eval_utils as EU
    opt, tap, cg = eval_models
    f2t = lambda s, e, n, d: [round(float(s) / n * d, 3), round(float(e) / n * d, 3)]
    rs = np.random.RandomState(19)
    videos = [dict(c3d=torch.from_numpy(rs.standard_normal((T, opt.video_dim)).astype(np.float32)).cuda(),
                   lda=torch.from_numpy(rs.standard_normal(opt.lda_dim).astype(np.float32)).cuda(), duration=60.0) for T in (24, 9, 40)]
    if beam is None:
        infos, ex = EU.caption_videos(tap, cg, videos, f2t, topN=6)
    else:
        infos, ex = EU.caption_videos_beam(tap, cg, videos, f2t, beam, topN=6)
    assert ex['batch'].CG_init_feats_type == 'VEC' and len(infos) == 3 and max(len(i) for i in infos) > 0
    for v, vid in enumerate(videos):
        one = EU.caption_video(tap, cg, vid['c3d'], vid['lda'], vid['duration'], f2t, topN=6, beam_size=beam or 1)
        one = one[0] if isinstance(one, tuple) else one
        assert len(one) == len(infos[v]), v
        for rec, ref in zip(infos[v], one):
            assert rec['sentence'] == ref['sentence'] and rec['timestamp'] == ref['timestamp'] and rec['num'] == ref['num']
            assert abs(rec['proposal_score'] - ref['proposal_score']) < 1e-6
            assert abs(rec['sentence_confidence'] - ref['sentence_confidence']) < 1e-3


# ---- 6. the zero-state dispatch is unchanged --------------------------------------------------------------------------------------
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


def test_zero_state_batch_still_takes_the_persistent_recurrences_and_an_initial_state_does_not():
    """vbctx without an initial state: the forward and the reverse persistent launch, as before (counted).  vbinit -- the same construction,
    <= 64 rows -- with its initial state: none, the launch-per-phase recurrences honour h0."""
    from echr_amd.batch import VideoBatch
    opt, params, vids = _case('vbctx')
    m, o, f = _fused(opt, params)
    b = VideoBatch.from_videos([dict({k: v[k] for k in KEYS}, tap=torch.from_numpy(v['tap'])) for v in vids], device=_dev())
    assert b.n_events <= 64 and b.CG_init_feats_type == ''
    _, launches = _persist_launches(lambda: f.batch(b, step=False))
    assert launches >= 2, launches
    opt, params, vids = _case('vbinit')
    m, o, f = _fused(opt, params)
    b, _ = _batch(opt, vids)
    assert b.n_events <= 64
    _, launches = _persist_launches(lambda: f.batch(b, step=False))
    assert launches == 0, launches

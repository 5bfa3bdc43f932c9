"""Frame-level contexts 'CH' / 'CC+CH' over a multi-video batch on the GPU (-m gpu): CaptionGenerator.forward_batch / beam_batch /
train_rl_batch, FusedTrainStep.batch and its joint form (echr_train_step_batch_clip), JointBatchStep, SelfCriticalBatchStep and
eval_utils.caption_videos(_beam) against the CPU reference of the contract (tests/clip_batch_ref.py: the clip oracle once per video, losses
and gradients summed, sliced dropout masks), the reference's own fixture (tests/golden/case_clip_batch.npz) and the single-video path.

Gates: the project's own (tests/test_gpu_clipctx.py, tests/test_gpu_vbatch.py) -- log-probs 2e-5 absolute, loss 1e-5 relative, index outputs
bit-exact (beam results for events whose ORACLE margin is >= 1e-4, as in tests/test_gpu_clipctx.py; counted), each gradient tensor and d tap
max(1e-5, 4 * e_ref) of its max-norm (+1e-9 absolute).  e_ref is the float32-vs-float64 difference of clip_batch_ref on the same case,
measured on the CPU (clip_batch_ref.e_ref; worst parameter gradient / worst video's d tap):

    vbch    eval 6.4e-07 / 4.8e-07   train 7.7e-07 / 5.6e-07
    vbcch   eval 9.7e-07 / 5.7e-07   train 9.4e-07 / 5.6e-07
    vbch33  eval 8.4e-07 / 5.8e-07   train 8.7e-07 / 6.6e-07

so 4 * e_ref stays below 1e-5 everywhere and the gate is the plain 1e-5.  Two HIP results compared with each other (batch against
single-video calls, one-call against module path) each carry that error: twice the gate, as tests/test_gpu_vbatch.py does."""
import functools

import numpy as np
import pytest
import torch

from echr_amd import functional as EF
from echr_amd import synth
from oracle import summary as SM
from tests import clip_batch_ref as R
from tests import joint_batch_ref as J
from tests import util as U
from tests import vbatch_ref as VR

pytestmark = pytest.mark.gpu

TOL_LOGP = 2e-5
TOL_LOSS = 1e-5
E_REF = {'vbch': 7.7e-7, 'vbcch': 9.7e-7, 'vbch33': 8.7e-7}          # worst tensor, either mode (header)
BEAM_MARGIN = 1e-4
BEAM_MIN_GATED = {'vbch': 13, 'vbcch': 12}          # events whose oracle beam margin is >= 1e-4 (of 14 / 13), measured on the CPU
UNUSED = {'lm_model.core.fusion_layer.weight', 'lm_model.core.fusion_layer.bias', 'fusion_model.h2a_layer.weight', 'fusion_model.h2a_layer.bias'}
KEYS = ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')


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
                               clip_context_type=opt.clip_context_type)
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


# ---- 1. module path ---------------------------------------------------------------------------------------------------------------
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
        assert np.abs(logp[s, :Sv] - ref['logp'][v]).max() < TOL_LOGP, v
    _check_losses(got['loss'], got['losses'], ref)
    _check_grads(got['grads'], ref['grads'], tol_grad(case))
    _check_g_tap(got['g_tap'], ref['g_tap'], b.row_offset, tol_grad(case))


def _check_vs_fixture(case, mode, got):
    g = U.gold('case_clip_batch.npz')
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
    for k, v in got['grads'].items():
        if v is not None and k not in U.NOISE_ONLY and (key + '|grad|' + k + '|linf') in g:
            ref = float(g[key + '|grad|' + k + '|linf'])
            assert abs(float(np.abs(v).max()) - ref) <= tol * max(ref, U.GRAD_FLOOR) + 1e-9, k
            head, strided = SM.grad_slices(v)
            for a, want in ((head, g[key + '|grad|' + k + '|head']), (strided, g[key + '|grad|' + k + '|strided'])):
                assert np.abs(a - want).max() <= tol * max(ref, U.GRAD_FLOOR) + 1e-9, k


@pytest.mark.parametrize('case', ['vbch', 'vbcch'])
@pytest.mark.parametrize('train_mode', [False, True])
def test_module_path_matches_oracle_and_reference(case, train_mode):
    """Every log-prob, the summed loss, the per-video losses, every parameter gradient and d batch.tap per video -- the anchors' rows
    ('ER3'), the scene mean ('VH') and the attended rows (echr_decoder_row_grad behind echr_decoder_bwd_batch) together."""
    got = _module_pass(case, train_mode)
    assert got['batch'].clip_parts == (2 if case == 'vbch' else 3)
    _check_vs_ref(case, got, _ref(case, train_mode))
    _check_vs_fixture(case, 'train' if train_mode else 'eval', got)


@pytest.mark.parametrize('train_mode', [False, True])
def test_module_path_132_rows_matches_oracle(train_mode):
    """33 videos x 4 events: the launch-per-phase recurrences and the event encoder's general kernels."""
    got = _module_pass('vbch33', train_mode)
    assert got['batch'].n_events == 132
    _check_vs_ref('vbch33', got, _ref('vbch33', train_mode))


@pytest.mark.parametrize('case', ['vbch', 'vbcch'])
def test_eval_rows_equal_the_single_video_forward(case):
    opt, params, vids = _case(case)
    m = U.build_gpu_model(opt, params, False)
    b, _ = _batch(opt, vids)
    with torch.no_grad():
        logp = m.forward_batch(b, mode='train').cpu().numpy()
        for v, s in enumerate(b.event_slices):
            d = b.video(v)
            one = m(d['tap'], d['c3d'], d['lda'], d['labels'], d['ind'], d['soi'], mode='train').cpu().numpy()
            assert np.abs(logp[s, :one.shape[1]] - one).max() <= 2 * TOL_LOGP, v


# ---- 2. one-call path -------------------------------------------------------------------------------------------------------------
def _fused(opt, params, train_mode=True, lr=1e-3, clip=100.0):
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    m = U.build_gpu_model(opt, params, train_mode)
    o = ClampAdam(m.parameters(), lr=lr, arena=m.build_arena())
    return m, o, FusedTrainStep(m, o, grad_clip=clip)


@pytest.mark.parametrize('case', ['vbch', 'vbcch', 'vbch33'])
def test_fused_batch_gradients_then_one_step(case):
    """FusedTrainStep.batch(step=False): the summed loss, per-video losses and summed gradients (the compacted active-row form: captions end
    at different steps and videos have different step counts); then ONE clamp + Adam step against vbatch_ref.step on the oracle's sum."""
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
    """FusedTrainStep._batch_tap(step=False) into a zero-filled g_tap: (loss, per-video losses, g_tap, arena gradients, batch, step object)."""
    m, o, f = _fused(opt, params, train_mode)
    b, _ = _batch(opt, vids)
    g_tap = torch.zeros_like(b.tap)
    per = torch.zeros(b.n_videos, device=_dev())
    gl = None if g_loss is None else torch.full((1,), g_loss, device=_dev())
    loss = float(f._batch_tap(b, g_tap, b.dev('row_offset'), per, g_loss=gl, step=False))
    torch.cuda.synchronize()
    return loss, per.cpu().numpy(), g_tap.cpu().numpy(), _arena_grads(m), b, f


@pytest.mark.parametrize('case', ['vbch', 'vbcch', 'vbch33'])
def test_batch_tap_call_fills_g_tap(case):
    """echr_train_step_batch_clip with g_tap: the anchors' rows, the 'VH' span over each video's own rows (vbch / vbcch) and the clip-row
    gradient through the list-form scatter, which meets dead rows (the compacted path; atomic mode: the events overlap)."""
    opt, params, vids = _case(case)
    ref = _ref(case, True)
    loss, per, g_tap, grads, b, f = _tap_call(opt, params, vids)
    assert 0 < f.last_active_rows < b.n_events * b.S and f.a.dec.rows_disjoint == 0
    assert len(set(b.steps)) > 1          # videos of different step counts; captions that end at different steps (the active rows say so)
    _check_losses(loss, per, ref)
    _check_grads(grads, ref['grads'], tol_grad(case))
    _check_g_tap(g_tap, ref['g_tap'], b.row_offset, tol_grad(case))
    if case == 'vbch':          # g_loss scales all three contributions to g_tap; the losses are reported unscaled
        loss2, per2, g_tap2, grads2, _, _ = _tap_call(opt, params, vids, g_loss=0.5)
        assert abs(loss2 - loss) < TOL_LOSS * abs(loss)
        _check_g_tap(g_tap2, ref['g_tap'], b.row_offset, tol_grad(case), scale=0.5)


def test_flag_form_of_the_scatter_gives_the_same_entry():
    """"row_grad_list" = 0: the batch entry with the flag form of the single-video entries -- the same gates; under the fixed-order mode the
    two forms agree bit for bit (the same sums in the same order)."""
    import echr_amd
    from echr_amd import _lib as L
    lib = L.load()
    opt, params, vids = _case('vbch')
    ref = _ref('vbch', True)
    try:
        lib.echr_config_set(b'row_grad_list', 0)
        loss, per, g_tap, grads, b, _ = _tap_call(opt, params, vids)
        _check_g_tap(g_tap, ref['g_tap'], b.row_offset, tol_grad('vbch'))
        echr_amd.set_deterministic(True)
        flag = _tap_call(opt, params, vids)
        lib.echr_config_set(b'row_grad_list', 1)
        lst = _tap_call(opt, params, vids)
    finally:
        lib.echr_config_set(b'row_grad_list', 1)
        echr_amd.set_deterministic(False)
    assert flag[0] == lst[0] and np.array_equal(flag[2], lst[2])
    _check_g_tap(lst[2], ref['g_tap'], b.row_offset, tol_grad('vbch'))


def test_disjoint_rows_take_the_plain_mode():
    """Three videos of make_video(disjoint=True) with N = 4, A = 8 and different label widths: no two events of the batch share a row, the
    scatter updates g_tap with plain read-modify-writes.  Against the oracle on the same videos."""
    opt, params, _ = _case('vbch')
    vids = [synth.make_video(4, 8, L, opt.CG_vocab_size + 1, seed=1800 + i, disjoint=True, video_dim=opt.video_dim, hidden_dim=opt.hidden_dim,
                             lda_dim=opt.lda_dim) for i, L in enumerate((6, 9, 7))]
    ref = R.run(opt, params, vids, True)
    loss, per, g_tap, grads, b, f = _tap_call(opt, params, vids)
    assert f.a.dec.rows_disjoint == 1 and 0 < f.last_active_rows < b.n_events * b.S
    _check_losses(loss, per, ref)
    _check_grads(grads, ref['grads'], tol_grad('vbch'))
    _check_g_tap(g_tap, ref['g_tap'], b.row_offset, tol_grad('vbch'))


@pytest.mark.parametrize('case', ['vbch', 'vbcch'])
def test_fixed_order_mode_is_bitwise(case):
    """set_deterministic(True) on overlapping events (per-event slabs + row_grad_fold_kernel): two runs agree bit for bit in loss, every
    gradient and d tap, and still meet the oracle."""
    import echr_amd
    opt, params, vids = _case(case)
    echr_amd.set_deterministic(True)
    try:
        runs = [_tap_call(opt, params, vids) for _ in range(2)]
    finally:
        echr_amd.set_deterministic(False)
    (la, pa, ta, ga, b, _), (lb, pb, tb, gb, _, _) = runs
    assert la == lb and np.array_equal(pa, pb) and np.array_equal(ta, tb)
    for k, v in ga.items():
        assert (v is None and gb[k] is None) or np.array_equal(v, gb[k]), k
    ref = _ref(case, True)
    _check_losses(la, pa, ref)
    _check_grads(ga, ref['grads'], tol_grad(case))
    _check_g_tap(ta, ref['g_tap'], b.row_offset, tol_grad(case))


# ---- 3. JointBatchStep ------------------------------------------------------------------------------------------------------------
def _tap_model(opt, sst_params, arena):
    from echr_amd import models
    from echr_amd.optim import ClampAdam
    tm = models.setup_tap(opt)
    tm.load_state_dict({k: torch.from_numpy(v) for k, v in sst_params.items()})
    tm = tm.to(_dev())
    tm.eval()
    return tm, (ClampAdam(tm.parameters(), lr=1e-9, arena=tm.build_arena()) if arena else None)


def test_joint_batch_step_equals_the_module_path():
    """'CH' with the proposal encoder in the loop (T_v <= 60, K = 16, eval mode): JointBatchStep's proposal-encoder and caption gradients
    against SST.forward_batch + forward_batch('train') + autograd on the same parameters -- all three paths of the caption loss into the
    encoder through d tap.  Two HIP results: twice the gradient gate."""
    from echr_amd.batch import VideoBatch
    from echr_amd.fused import JointBatchStep
    from echr_amd.misc import utils
    opt, params, sst_params, vids, tap_in = J.setup('vbch')
    assert opt.clip_context_type == 'CH' and max(len(v['c3d']) for v in vids) <= 64
    mk, lb, w1 = ([torch.from_numpy(t[i]).to(_dev()) for t in tap_in] for i in range(3))
    rows = J.row_offsets(vids)
    # module path
    m2 = U.build_gpu_model(opt, params, False)
    tm2, _ = _tap_model(opt, sst_params, False)
    c3d_all = torch.cat([torch.from_numpy(v['c3d']) for v in vids], 0).to(_dev())
    tap_all, scores = tm2.forward_batch(c3d_all, rows)
    b2 = VideoBatch.from_videos([dict({k: v[k] for k in KEYS}, tap=tap_all[rows[i]:rows[i + 1]]) for i, v in enumerate(vids)], device=_dev(),
                                clip_context_type='CH')
    cg, cg_per = b2.criterion(utils.LanguageModelCriterion(), m2.forward_batch(b2, mode='train'))
    tl, tl_per = utils.tap_criterion_batch(utils.TAPModelCriterion(), scores, torch.cat(mk, 0), torch.cat(lb, 0), w1, rows)
    (J.LAMBDA1 * tl + cg).backward()
    torch.cuda.synchronize()
    cg, tl = cg.detach(), tl.detach()
    # one-call path: the list of video dicts becomes a batch built for the model's clip context
    m, o, f = _fused(opt, params, False, lr=1e-9, clip=None)
    tm, to = _tap_model(opt, sst_params, True)
    js = JointBatchStep(f, tm, to, lambda1=J.LAMBDA1, lambda2=1.0)
    loss = js([{k: v[k] for k in KEYS} for v in vids], mk, lb, w1, step=False)
    torch.cuda.synchronize()
    assert js.last_batch.clip_parts == 2
    assert abs(float(js.cg_loss) - float(cg)) < 2 * TOL_LOSS * abs(float(cg)) and abs(float(js.tap_loss) - float(tl)) < 2 * TOL_LOSS * abs(float(tl))
    assert abs(float(loss) - float(J.LAMBDA1 * tl + cg)) < 2 * TOL_LOSS * abs(float(cg))
    assert np.abs(js.last_video_losses.cpu().numpy() - cg_per.detach().cpu().numpy()).max() < 2 * TOL_LOSS * float(cg_per.max())
    tol = 2 * tol_grad('vbch')
    ar = tm._echr_arena
    for i, ((k, p), (_, p2)) in enumerate(zip(tm.named_parameters(), tm2.named_parameters())):
        got, want = ar.grad_view(i).detach().cpu().numpy(), p2.grad.cpu().numpy()
        print('sst %-30s rel err %.2e' % (k, U.relerr(got, want, U.GRAD_FLOOR)))
        assert np.abs(got - want).max() <= tol * max(float(np.abs(want).max()), U.GRAD_FLOOR) + 1e-9, (k, U.relerr(got, want))
    _check_grads(_arena_grads(m), _grads(m2), tol)
    # a ready batch built for another clip context is refused
    with pytest.raises(NotImplementedError):
        js(VideoBatch.from_videos([dict({k: v[k] for k in KEYS}, tap=torch.from_numpy(v['tap'])) for v in vids], device=_dev()), mk, lb, w1)


# ---- 4. decodes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['vbch', 'vbcch'])
def test_greedy_and_beam_decodes_equal_the_per_video_oracle(case):
    """forward_batch(mode='eval'): seq bit-exact against the reference's per-video sequences (the fixture; the oracle's are asserted equal
    on the CPU), log-probs within the gate.  beam_batch(B = 3), as one decode and as run-local row slices (max_rows = 12): seq bit-exact for
    every event whose oracle margin is >= 1e-4."""
    g = U.gold('case_clip_batch.npz')
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
    for kw in (dict(), dict(max_rows=12)):
        bseq, blp, score, vw = m.beam_batch(b, 3, **kw)
        bseq, blp, score = bseq.cpu().numpy(), blp.cpu().numpy(), score.cpu().numpy()
        for v, (s, r) in enumerate(zip(b.event_slices, refs)):
            ok = np.asarray(r['margin']) >= BEAM_MARGIN
            rseq, w = np.asarray(r['seq']), int(vw[v])
            if ok.all():
                assert w == int(np.asarray(r['words']).max()), (v, w)
            k = min(w, rseq.shape[1])
            assert np.array_equal(bseq[s, :k][ok], rseq[:, :k][ok]) and not bseq[s, w:].any(), v
            rs = np.asarray(r['score'])[ok]
            assert np.all(np.abs(score[s][ok] - rs) <= 1e-4 * np.maximum(np.abs(rs), 1.0)), v
    assert len(b.beam_groups(3, 12)) > 1          # the second decode ran on run-local slices of the row source


def _rl_mask(gen, widths, vid):
    mask = np.zeros(gen.shape, dtype=bool)
    mask[:, 0] = True
    mask[:, 1:] = gen[:, :-1] > 0
    return mask & (np.arange(gen.shape[1])[None, :] < np.asarray(widths)[np.asarray(vid)][:, None])


@pytest.mark.parametrize('case', ['vbch', 'vbcch'])
def test_train_rl_batch_sample_equals_its_teacher_forced_recompute(case):
    """Dropout on: the log-probs the batched sampled decode emits over the clip rows equal train_rl_batch's teacher-forced recompute of the
    same draw under the same dropout state; video_words are each video's own width."""
    opt, params, vids = _case(case)
    m = U.build_gpu_model(opt, params, True)
    b, _ = _batch(opt, vids, labels=False)
    lm = m.lm_model
    m.set_dropout_state(U.SEED, U.OFFSET)
    gen, slp_tf, greedy, vw = m.train_rl_batch(b, seed=1234)
    assert isinstance(gen, torch.Tensor) and gen.shape[1] > 0 and slp_tf.requires_grad
    m.set_dropout_state(U.SEED, U.OFFSET)
    with torch.no_grad():
        video, event, ev_start, ev_len, A, vid, drop = m._batch_contexts(b, None)
        gen2, slp, vw2 = EF.sample_train_batch(video, event, b.clip_rows(), ev_start, ev_len, vid, A, lm.seq_length, lm.native_params(), drop,
                                               seed=1234)
    assert torch.equal(gen, gen2) and np.array_equal(vw, vw2)
    g = gen.cpu().numpy()
    assert np.array_equal(vw, b.caption_widths(g)) and g.shape[1] == int(vw.max())
    mask = _rl_mask(g, vw, b.vid)
    assert mask.any()
    err = np.abs(slp.cpu().numpy() - slp_tf.detach().cpu().numpy())[mask].max()
    print('sampled vs teacher-forced log-probs: %.2e' % err)
    assert err < TOL_LOGP, err
    assert isinstance(greedy, torch.Tensor) and greedy.shape[0] == b.n_events


def _no_dropout(m):
    m.fusion_model.enc_attn.dropout.p = 0.0
    c = m.lm_model.core
    c.dropout0.p = c.dropout1.p = c.dropout2.p = 0.0
    m.lm_model.dropout.p = 0.0


@pytest.mark.parametrize('case', ['vbch', 'vbcch'])
def test_self_critical_batch_step_equals_the_sum_of_single_video_steps(case):
    """Without dropout, on given captions of different widths per video and a signed reward: loss, per-video losses and the summed flat
    gradient against V SelfCriticalStep(step=False) calls.  Two HIP results: twice the gradient gate."""
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
    for i, p in enumerate(ar.params):
        lo, n = ar.offsets[i], p.numel()
        a, r = ar.flat_g[lo:lo + n], flat[lo:lo + n]
        scale = float(r.abs().max())
        if names[i] in U.NOISE_ONLY:
            assert float(a.abs().max()) < 1e-6
            continue
        assert float((a - r).abs().max()) <= tol * max(scale, U.GRAD_FLOOR) + 1e-9, (names[i], float((a - r).abs().max()), scale)


@pytest.fixture(scope='module')
def eval_models():
    from echr_amd import models as EM
    _, params, _ = _case('vbch')
    opt = synth.default_opt(**dict(synth.VBATCH['vbch']['opt'], K=8))
    torch.manual_seed(3)
    tap = EM.setup_tap(opt)
    tap.eval()
    return opt, tap.cuda(), U.build_gpu_model(opt, params, False)


@pytest.mark.parametrize('beam', [None, 3])
def test_caption_videos_give_each_video_its_own_records(eval_models, beam):
    """caption_videos / caption_videos_beam build their batch for the model's clip context ('CH'): three short videos get the records
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
    assert ex['batch'].clip_parts == 2 and len(infos) == 3 and max(len(i) for i in infos) > 0
    for v, vid in enumerate(videos):
        one = EU.caption_video(tap, cg, vid['c3d'], vid['lda'], vid['duration'], f2t, topN=6, beam_size=beam or 1)
        one = one[0] if isinstance(one, tuple) else one
        assert len(one) == len(infos[v]), v
        for rec, ref in zip(infos[v], one):
            assert rec['sentence'] == ref['sentence'] and rec['timestamp'] == ref['timestamp'] and rec['num'] == ref['num']
            assert abs(rec['proposal_score'] - ref['proposal_score']) < 1e-6
            assert abs(rec['sentence_confidence'] - ref['sentence_confidence']) < 1e-3

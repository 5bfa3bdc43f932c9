"""The criterion chain of a training iteration (late-fusion logits -> row log-softmax -> masked NLL or the reward-weighted criterion ->
d logits) at the vocabulary widths where csrc/core.hip changes kernels (-m gpu), against the float64 oracle.

Dispatch (parity status): logsoftmax_rows holds a row in registers for cols <= 2048 / 5120 / 10240 (<8> / <20> / <40>) and streams
beyond; logsoftmax_nll_dlg (the one-pass criterion of echr_train_step) picks the same forms by ldo = rup(V1, 4) and is switched off by
logsoftmax_nll_dlg_ok for ldo > 10240, where echr_train_step takes its unfused branch (logits on all S*N rows, logsoftmax_rows, the
separate loss kernels, the target form of logsoftmax_bwd over every row, active rows dropped).  WIDTHS puts a row on each side of every
limit: 2047 (ldo = 2048: the zero-padding column is the last live register slot) | 2048 | 2049, 5120 | 5121, 10239 (ldo = 10240) | 10240 |
10241 (the smallest width of the unfused branch).

Everything else is as small as the kernels allow (3 events, 4 segments, 3 decoder steps, 9 feature rows).  The synthetic labels are edited
so that the edges are live: one active target is the LAST word (column V1 - 1), event 1 has a hole in its mask before the caption's end,
event 2 has an all-zero mask (no active row).  Train mode with dropout (the masks tests/util.py injects).

Gates: those of tests/test_gpu_parity.py, under the same measures (U.grad_close / U.relerr).  Float32-vs-float64 distance of the oracle
itself at these cases, measured on the CPU (worst of the widths): log-probs 1.4e-6 absolute (10239), loss 6.6e-8 relative (2047; reward-
weighted 1.9e-7 at 10240), worst gradient tensor 2.1e-6 of its max-norm (10240, enc_attn.query_1.weight; two-video batch 2.1e-6 at 10240,
reward-weighted 1.4e-6 at 2048, with the dense second consumer 1.4e-6 at 2049), d tap_feats 7.8e-7 (5121) -- four times each stays below
its gate, so none is widened.

Beyond the four paths of the plan, DENSE_WIDTHS run the module path with a second consumer of the log-probs: the decoder's backward then
takes logsoftmax_bwd with a dense G, whose register forms switch at ldo 2048 and 5120.

The paths of one width run back to back (the parametrisation is width-major), so the module-level oracle cache holds one width at a time:
the float64 gradients of a 10241-word model are ~170 MB.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from echr_amd import synth
from tests import util as U
from tests import vbatch_ref as R

pytestmark = pytest.mark.gpu

TOL_LOGP = 2e-5     # absolute on log-probs
TOL_LOSS = 1e-5     # relative
TOL_GRAD = 1e-5     # relative to the tensor's max-norm

WIDTHS = [2047, 2048, 2049, 5120, 5121, 10239, 10240, 10241]
RW_WIDTHS = [2048, 5121, 10240, 10241]
BATCH_WIDTHS = [2049, 10240, 10241]
DENSE_WIDTHS = [2047, 2048, 2049, 5120, 5121]          # logsoftmax_bwd with a dense G: <8> for ldo <= 2048, <20> <= 5120, streaming beyond
UNFUSED = 10241          # rup(V1, 4) > 256 * 40: logsoftmax_nll_dlg_ok declines
N_EV, SEG, L, T_V = 3, 4, 4, 9


def _edit_labels(vid, V1, zero_event=True):
    """The label edits of the module docstring, in place."""
    labels, masks = vid['labels'], vid['masks']
    labels[0, 1] = V1 - 1                       # event 0's first word: unmasked, not the caption's final position (the <eos> target follows)
    if labels.shape[0] > 1:
        masks[1, 1] = 0.0                       # a hole before the caption's end (column 2 stays 1: every caption has >= 1 word + <eos>)
    if zero_event and labels.shape[0] > 2:
        masks[2, :] = 0.0
    return vid


def _case(V1):
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=L - 2)
    params = synth.make_params(opt, 3)
    vid = _edit_labels(synth.make_video(N_EV, SEG, L, V1, seed=V1, T_v=T_V, min_len=1), V1)
    return opt, params, vid


def _batch_case(V1):
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=L - 2)
    params = synth.make_params(opt, 3)
    vids = [_edit_labels(synth.make_video(n, SEG, L, V1, seed=V1 + 100 * (i + 1), T_v=T_V, min_len=1), V1, zero_event=False)
            for i, n in enumerate((2, 1))]
    # video 0 deterministically: event 0 a full caption (two words + <eos>: the video keeps its three steps), event 1 one word + <eos> with
    # the hole on its word -- its last step is behind the caption's end, so the host form lists fewer than S * N active rows
    lab, msk = vids[0]['labels'], vids[0]['masks']
    lab[0, 2] = lab[0, 2] if lab[0, 2] else 1
    msk[0, :] = 1.0
    lab[1, 2], msk[1, 2], msk[1, 3] = 0, 1.0, 0.0
    return opt, params, vids


def _assert_edges(vid, V1):
    tg, mk = vid['labels'][:, 1:], vid['masks'][:, 1:]
    assert ((tg == V1 - 1) & (mk != 0)).any()                                     # an active target in the last column
    assert mk[1, 0] == 0 and mk[1, 1:].any()                                      # a hole before the end of caption 1
    assert not mk[2].any() and mk[0].any()                                        # event 2 contributes no active row
    assert tg.max() == V1 - 1 and tg.min() == 0


def _rw_weight(vid):
    """reward * mask [N, S] with both signs on active positions (RewardCriterion's numerator weight)."""
    mk = vid['masks'][:, 1:]
    reward = np.random.RandomState(7).uniform(0.25, 1.0, size=mk.shape).astype(np.float32)
    reward[:, ::2] *= -1.0
    w = (reward * mk).astype(np.float32)
    assert (w > 0).any() and (w < 0).any()
    return w


def _dense_weight(shape):
    """A second consumer of the log-probs: loss += sum(logp * weight), every column of every row with a gradient of its own."""
    return (1e-3 * np.random.RandomState(11).uniform(-1.0, 1.0, size=shape)).astype(np.float32)


_CACHE = {}          # one width at a time: {'V1': width, ...results of that width}


def _slot(V1):
    if _CACHE.get('V1') != V1:
        _CACHE.clear()
        _CACHE['V1'] = V1
    return _CACHE


def _np_grads(leaves, gs):
    return {k: (None if g is None else g.numpy().copy()) for k, g in zip(leaves, gs)}


def _oracle(V1):
    """The float64 oracle of width V1 (cached): the case, log-probs, LanguageModelCriterion loss / gradients / d tap_feats and, at RW_WIDTHS,
    the reward-weighted loss sum(-logp[target] * reward * mask) / sum(mask) back-propagated through the same graph."""
    c = _slot(V1)
    if 'single' not in c:
        opt, params, vid = _case(V1)
        P = {k: torch.from_numpy(v.copy()).to(torch.float64).requires_grad_(True) for k, v in params.items()}
        logp, loss, tap = R.run_video(opt, P, vid, U.oracle_drop(opt), torch.float64)
        names = list(P) + ['tap']
        leaves = list(P.values()) + [tap]
        rw, dense = V1 in RW_WIDTHS, V1 in DENSE_WIDTHS
        out = dict(opt=opt, params=params, vid=vid, logp=logp.detach().numpy(), loss=float(loss.detach()))
        g = _np_grads(names, torch.autograd.grad(loss, leaves, retain_graph=rw or dense, allow_unused=True))
        out['g_tap'], out['grads'] = g.pop('tap'), g
        if dense:
            total = loss + (logp * torch.from_numpy(_dense_weight(tuple(logp.shape))).double()).sum()
            g = _np_grads(names, torch.autograd.grad(total, leaves, retain_graph=rw, allow_unused=True))
            g.pop('tap')
            out['grads_dense'] = g
        if rw:
            w = _rw_weight(vid)
            tg = torch.from_numpy(vid['labels'][:, 1:])
            picked = logp.gather(2, tg[:, :logp.shape[1], None])[:, :, 0]
            loss_rw = (-picked * torch.from_numpy(w).double()).sum() / torch.from_numpy(vid['masks'][:, 1:]).double().sum()
            g = _np_grads(names, torch.autograd.grad(loss_rw, leaves, allow_unused=True))
            g.pop('tap')
            out.update(w=w, loss_rw=float(loss_rw.detach()), grads_rw=g)
        c['single'] = out
    return c['single']


def _batch_oracle(V1):
    c = _slot(V1)
    if 'batch' not in c:
        opt, params, vids = _batch_case(V1)
        c['batch'] = dict(opt=opt, params=params, vids=vids, ref=R.run(opt, params, vids, True, dtype=torch.float64))
    return c['batch']


def _check_grads(grads, ref, tag=''):
    worst = max([(U.relerr(grads[k], g, U.GRAD_FLOOR), k) for k, g in ref.items() if g is not None and grads[k] is not None and k not in U.NOISE_ONLY])
    print('   %s: worst gradient %.3g (%s)' % ((tag,) + worst))
    for k, g in ref.items():
        if g is None:
            assert grads[k] is None or not np.any(grads[k]), (tag, k)
        else:
            assert grads[k] is not None, (tag, k)
            assert U.grad_close(k, grads[k], g, TOL_GRAD), (tag, k, U.relerr(grads[k], g))


def _model_grads(m):
    return {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}


def _fused(opt, params):
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
    return m, FusedTrainStep(m, o, grad_clip=None)


def _inputs(vid):
    return tuple(torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))


def _gemm_flops(fn):
    """(fn's result, the products' FLOPs the library's profiler counted while fn ran: echr_prof_read kinds 0 / 6 / 7 = fp32, bf16x3, h2)."""
    from echr_amd import _lib
    lib = _lib.load()
    _lib.check(lib.echr_prof_enable(1), 'prof_enable')
    try:
        out = fn()
        torch.cuda.synchronize()
        total = 0.0
        for kind in (0, 6, 7):
            ms, fl, by, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
            _lib.check(lib.echr_prof_read(kind, C.byref(ms), C.byref(fl), C.byref(by), C.byref(n)), 'prof_read')
            total += fl.value
    finally:
        _lib.check(lib.echr_prof_enable(0), 'prof_enable')
    return out, total


# ---- the four paths ----------------------------------------------------------------------------------------------------------------

def _path_module(V1):
    """(a) CaptionGenerator forward + LanguageModelCriterion + autograd backward: log-probs (logsoftmax_rows), loss, every gradient."""
    r = _oracle(V1)
    _assert_edges(r['vid'], V1)
    pred, loss, grads, _ = U.run_gpu(r['opt'], r['params'], r['vid'], True)
    assert pred.shape == r['logp'].shape
    err = np.abs(pred - r['logp']).max()
    print('V1 %d module: logp %.3g loss %.3g' % (V1, err, abs(loss - r['loss']) / abs(r['loss'])))
    assert err < TOL_LOGP, err
    assert abs(loss - r['loss']) < TOL_LOSS * abs(r['loss']), (loss, r['loss'])
    _check_grads(grads, r['grads'], 'module')


def _path_module_dense(V1):
    """(a) with a second consumer of the log-probs, sum(logp * weight): the criterion's sparse gradient is added back in dense form and the
    decoder's backward runs logsoftmax_bwd with a dense G over all V1 columns (its register forms switch at ldo 2048 / 5120)."""
    from echr_amd.misc.utils import LanguageModelCriterion
    r = _oracle(V1)
    vid = r['vid']
    m = U.build_gpu_model(r['opt'], r['params'], True)
    tap, c3d, lda = _inputs(vid)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    nll = LanguageModelCriterion()(pred, labels[:, 1:].cuda(), masks[:, 1:].cuda())
    (nll + (pred * torch.from_numpy(_dense_weight(tuple(pred.shape))).cuda()).sum()).backward()
    torch.cuda.synchronize()
    assert abs(float(nll.detach()) - r['loss']) < TOL_LOSS * abs(r['loss'])
    _check_grads(_model_grads(m), r['grads_dense'], 'module, dense G')


def _one_call(V1, device_criterion=False):
    r = _oracle(V1)
    vid = r['vid']
    m, f = _fused(r['opt'], r['params'])
    tap, c3d, lda = _inputs(vid)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    tg, mk = labels[:, 1:], masks[:, 1:]
    if device_criterion:
        tg, mk = tg.cuda(), mk.cuda()
    g_tap = torch.zeros_like(tap)
    loss = float(f(tap, c3d, lda, labels, vid['ind'], vid['soi'], tg, mk, step=False, tap_grad=g_tap))
    torch.cuda.synchronize()
    return r, m, f, loss, g_tap.cpu().numpy()


def _path_one_call(V1):
    """(b) FusedTrainStep(step=False, tap_grad=...): loss, every gradient and d tap_feats element-wise.  Host criterion inputs: the active
    rows are listed (fused branch: compact logits + logsoftmax_nll_dlg on them; unfused branch: the list is dropped)."""
    r, m, f, loss, g_tap = _one_call(V1)
    _assert_edges(r['vid'], V1)
    assert 0 < f.last_active_rows < N_EV * (L - 1)
    print('V1 %d one-call: loss %.3g d tap %.3g' % (V1, abs(loss - r['loss']) / abs(r['loss']), U.relerr(g_tap, r['g_tap'])))
    assert abs(loss - r['loss']) < TOL_LOSS * abs(r['loss']), (loss, r['loss'])
    _check_grads(_model_grads(m), r['grads'], 'one-call')
    assert g_tap.shape == r['g_tap'].shape and float(np.abs(r['g_tap']).max()) > 0
    assert U.grad_close('tap_feats', g_tap, r['g_tap'], TOL_GRAD), U.relerr(g_tap, r['g_tap'])


def _path_one_call_native(V1):
    """(b) once more with the native products (gemm_h2 = 0): the unfused branch's fp32 / bf16x3 logit product over all rows."""
    from echr_amd import _lib
    lib = _lib.load()
    assert lib.echr_config_set(b'gemm_h2', 0) == 0
    try:
        _path_one_call(V1)
    finally:
        lib.echr_config_set(b'gemm_h2', 1)


def _path_rw(V1):
    """(c) echr_train_step_rw with the signed weight reward * mask: in host_index (active rows listed) and through the device weight entry
    (all rows) -- logsoftmax_nll_dlg_kernel<EPT, true> up to 10240, nll_loss_rw + logsoftmax_bwd_kernel<true> at 10241."""
    from echr_amd import _lib
    r = _oracle(V1)
    vid, w = r['vid'], r['w']
    m, f = _fused(r['opt'], r['params'])
    tap, c3d, lda = _inputs(vid)
    labels, masks = vid['labels'], vid['masks']
    slot, st = f._setup(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], False, False, None, False, weights=w)
    a, lib = f.a, f.lib
    a.prepared = a.handover = 0
    a.handover_cb = a.handover_user = a.mid_cb = a.mid_user = None
    assert 0 < a.n_active < N_EV * (L - 1)
    _lib.check(lib.echr_train_step_rw(C.byref(a), None, _lib.stream_ptr()), 'train_step_rw')
    loss = float(f._finish(slot, st, False))
    print('V1 %d reward-weighted (host): loss %.3g' % (V1, abs(loss - r['loss_rw']) / abs(r['loss_rw'])))
    assert abs(loss - r['loss_rw']) < TOL_LOSS * abs(r['loss_rw']), (loss, r['loss_rw'])
    _check_grads(_model_grads(m), r['grads_rw'], 'rw host')
    # the device weight entry: targets / mask / weight [N, S] in device memory, every row (the same argument struct, so the same dropout state)
    N, S = a.dec.N, a.dec.S
    tgt_d = torch.from_numpy(np.ascontiguousarray(labels[:, 1:1 + S], dtype=np.int32)).cuda()
    mask_d = torch.from_numpy(np.ascontiguousarray(masks[:, 1:1 + S], dtype=np.float32)).cuda()
    w_d = torch.from_numpy(np.ascontiguousarray(w[:, :S])).cuda()
    a.host_nll, a.n_active = 0, 0
    a.nll_target, a.nll_target_i64, a.nll_mask = tgt_d.data_ptr(), 0, mask_d.data_ptr()
    _lib.check(lib.echr_train_step_rw(C.byref(a), w_d.data_ptr(), _lib.stream_ptr()), 'train_step_rw')
    torch.cuda.synchronize()
    loss = float(slot[0])
    print('V1 %d reward-weighted (device): loss %.3g' % (V1, abs(loss - r['loss_rw']) / abs(r['loss_rw'])))
    assert abs(loss - r['loss_rw']) < TOL_LOSS * abs(r['loss_rw']), (loss, r['loss_rw'])
    _check_grads(_model_grads(m), r['grads_rw'], 'rw device')


def _path_batch(V1, device_criterion):
    """(d) FusedTrainStep.batch over V = 2 videos (2 + 1 events) against tests/vbatch_ref.py: summed loss, per-video losses (video_loss_rows
    on the fused branch, video_loss_logp on the unfused one) and the summed gradients."""
    from echr_amd.batch import VideoBatch
    c = _batch_oracle(V1)
    ref, vids = c['ref'], c['vids']
    for v in vids:
        assert ((v['labels'][:, 1:] == V1 - 1) & (v['masks'][:, 1:] != 0)).any()
    assert vids[0]['masks'][1, 1] == 0 and vids[0]['masks'][1, 2] != 0
    m, f = _fused(c['opt'], c['params'])
    b = VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi', 'labels', 'masks')} for v in vids], device=torch.device('cuda'))
    assert b.n_videos == 2 and b.n_events == 3
    loss = float(f.batch(b, step=False, device_criterion=device_criterion))
    torch.cuda.synchronize()
    if not device_criterion:
        assert 0 < f.last_active_rows < b.n_events * b.S
    per = f.last_video_losses.cpu().numpy()
    print('V1 %d batch: loss %.3g per-video %.3g' % (V1, abs(loss - ref['loss']) / abs(ref['loss']), np.abs(per - ref['losses']).max() / np.abs(ref['losses']).max()))
    assert abs(loss - ref['loss']) < TOL_LOSS * abs(ref['loss']), (loss, ref['loss'])
    assert np.abs(per - ref['losses']).max() < TOL_LOSS * np.abs(ref['losses']).max(), (per, ref['losses'])
    _check_grads(_model_grads(m), ref['grads'], 'batch')


def _plan():
    plan = []
    for V1 in WIDTHS:
        plan += [(V1, 'module'), (V1, 'one_call')]
        if V1 in DENSE_WIDTHS:
            plan.append((V1, 'module_dense'))
        if V1 == UNFUSED:
            plan.append((V1, 'one_call_native'))
        if V1 in RW_WIDTHS:
            plan.append((V1, 'reward_weighted'))
        if V1 in BATCH_WIDTHS:
            plan += [(V1, 'batch_host'), (V1, 'batch_device')]
    return plan


@pytest.mark.parametrize('V1,path', _plan())
def test_criterion_chain_at_dispatch_widths(V1, path):
    """Every width under (a) the module path and (b) the one-call path; RW_WIDTHS under (c) the reward-weighted one-call path; BATCH_WIDTHS
    under (d) the batched one-call path with host and device criterion inputs; 10241 once more under (b) with the native products;
    DENSE_WIDTHS under (a) with a dense upstream gradient."""
    {'module': _path_module, 'module_dense': _path_module_dense, 'one_call': _path_one_call, 'one_call_native': _path_one_call_native, 'reward_weighted': _path_rw,
     'batch_host': lambda v: _path_batch(v, False), 'batch_device': lambda v: _path_batch(v, True)}[path](V1)


def test_plan_covers_every_width_and_subset():
    plan = _plan()
    assert [v for v, p in plan if p == 'module'] == WIDTHS and [v for v, p in plan if p == 'one_call'] == WIDTHS
    assert [v for v, p in plan if p == 'reward_weighted'] == RW_WIDTHS and [v for v, p in plan if p == 'module_dense'] == DENSE_WIDTHS
    assert [v for v, p in plan if p == 'batch_host'] == BATCH_WIDTHS == [v for v, p in plan if p == 'batch_device']


@pytest.mark.parametrize('V1', [10240, UNFUSED])
def test_width_10241_takes_the_unfused_branch(V1):
    """What the library exposes that tells the branches apart: the FLOPs its profiler counts for the products (echr_prof_read).  With host
    criterion inputs the call lists the active rows (FusedTrainStep.last_active_rows: fewer than S * N here).  On the fused branch the logit
    product, d OUTD and d W_logit then run on those rows only, so the call counts FEWER product FLOPs than the same call with device
    criterion inputs (all rows).  On the unfused branch the list is dropped in front of the logit product and for the backward pass: both
    forms count exactly the same.  (last_active_rows alone does not tell: Python sets it before the library chooses.)"""
    (_, _, f_host, _, _), fl_host = _gemm_flops(lambda: _one_call(V1, False))
    (_, _, f_dev, _, _), fl_dev = _gemm_flops(lambda: _one_call(V1, True))
    assert 0 < f_host.last_active_rows < N_EV * (L - 1) and f_dev.last_active_rows == 0
    assert fl_host > 0 and fl_dev > 0
    if V1 == UNFUSED:
        assert fl_host == fl_dev, (fl_host, fl_dev)
    else:
        assert fl_host < fl_dev, (fl_host, fl_dev)


def test_all_zero_mask_gives_exact_zeros_then_recovers():
    """V1 = 301, every mask entry zero: the reference's 0 / (0 + 1e-6) -- loss and every gradient of the LanguageModelCriterion path are
    exactly 0 and nothing is NaN; the next call on the same model with the normal mask matches the oracle."""
    from echr_amd.misc.utils import LanguageModelCriterion
    V1 = 301
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=L - 2)
    params = synth.make_params(opt, 3)
    vid = synth.make_video(N_EV, SEG, L, V1, seed=V1, T_v=T_V, min_len=1)
    zero = dict(vid, masks=np.zeros_like(vid['masks']))
    pred, loss, grads, m = U.run_gpu(opt, params, zero, True)
    assert np.isfinite(pred).all()
    assert loss == 0.0
    for k, g in grads.items():
        assert g is None or (np.isfinite(g).all() and not np.any(g)), k
    rpred, rloss, rgrads = U.run_oracle(opt, params, vid, True, dtype=torch.float64)
    for p in m.parameters():
        p.grad = None
    m.set_dropout_state(U.SEED, U.OFFSET)
    tap, c3d, lda = _inputs(vid)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    loss = LanguageModelCriterion()(pred, labels[:, 1:].cuda(), masks[:, 1:].cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert np.abs(pred.detach().cpu().numpy() - rpred).max() < TOL_LOGP
    assert abs(float(loss.detach()) - rloss) < TOL_LOSS * abs(rloss)
    _check_grads(_model_grads(m), rgrads, 'after the all-zero mask')

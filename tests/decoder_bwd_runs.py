"""The decoder backward passes that tests/golden/decoder_bwd.json pins (tools/make_golden_decoder_bwd.py records them,
tests/test_gpu_decoder_bwd_stages.py replays them): one run per schedule and arm of echr::decoder_bwd_parts (the table at the head of the
backward section of csrc/decoder.hip), on the existing small cases only.

    autograd|h2, |native      no arena: gradients overwrite (`zeroed` 0), everything on the caller's stream
    arena|h2, |native         arena, no hook: async_tail 2
    arena_d_video             'vbinit' batch, tap_feats leaves: d video wanted -> async_tail 1; batch arm of the scene gradients; g_h0
    hook_staged               arena.early_grad_hook: phases 1, 3, 4
    hook_onecall              ... with early_staged False: async_tail 1
    step|h2, |native          FusedTrainStep, one call, captions that end at different steps: d logits ready, active rows, scratch ahead
    joint                     JointTrainStep ('c5'): the two-piece form, parts 1 and 2 (asserted: the library called mid_cb)
    step_batch, forward_batch FusedTrainStep.batch / forward_batch under autograd on 'vbctx': batch arm of the scene gradients
    arena_init, step_init     'initc': g_h0
    shared_rows               'vctx' through the one-call step with tap_grad: events share video rows (d P_all fold), 'VH' d video
    sat                       one show_attend_tell training backward: the fixed-order att_post helper shared with csrc/sat.hip

run(name) returns the bits of one run in deterministic mode: `loss` and, where the path exposes them, `d_event`, `d_video`, `g_h0`, `d_tap`
as the hex of their fp32 bytes' sha256 (loss: the bytes themselves), `grads` as the sha256 of the flat gradient arena or of the concatenated
per-tensor gradients, `floats` with the number of floats behind each hash; `joint` adds both models' parameters behind its update.  The autograd runs read d event / d video / g_h0 off what
functional._decoder_backward returns; the one-call step keeps d event in its workspace, so its runs pin d tap_feats, formed from d event.
launches(name) is the same run outside deterministic mode with the library's profile on around the backward (or the one call): the
`launches` figure of echr_prof_read for every kind."""
import contextlib
import ctypes as C
import hashlib
import os

import numpy as np
import torch

from echr_amd import synth
from tests import util as U

RUNS = ('autograd|h2', 'autograd|native', 'arena|h2', 'arena|native', 'arena_d_video', 'hook_staged', 'hook_onecall', 'step|h2', 'step|native',
        'joint', 'step_batch', 'forward_batch', 'arena_init', 'step_init', 'shared_rows', 'sat')
PROF_KINDS = 11
_prof = dict(on=False, counts=None)


def _pin(rec, key, *ts):
    """rec[key] = sha256 of the tensors' fp32 bytes, rec['floats'][key] = how many floats that was (the record's sanity test compares the hash
    with that of as many zeros)."""
    torch.cuda.synchronize()
    h, n = hashlib.sha256(), 0
    for t in ts:
        x = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        h.update(x.tobytes())
        n += x.size
    rec[key] = h.hexdigest()
    rec.setdefault('floats', {})[key] = n
    return rec


def _hex(x):
    return np.ascontiguousarray(x.detach().cpu().numpy(), dtype=np.float32).tobytes().hex()


@contextlib.contextmanager
def _profiled():
    """The library's profile around the block when launches() asked for it; the counts of every kind land in _prof['counts']."""
    if not _prof['on']:
        yield
        return
    from echr_amd import _lib as L
    lib = L.load()
    torch.cuda.synchronize()
    L.check(lib.echr_prof_enable(1), 'prof_enable')
    try:
        yield
        torch.cuda.synchronize()
        out = []
        for k in range(PROF_KINDS):
            ms, fl, by, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
            L.check(lib.echr_prof_read(k, C.byref(ms), C.byref(fl), C.byref(by), C.byref(n)), 'prof_read')
            out.append(int(n.value))
        _prof['counts'] = out
    finally:
        L.check(lib.echr_prof_enable(0), 'prof_enable')


@contextlib.contextmanager
def _gemm_h2(on):
    """The named product path for the block, then the process's own again: the library has no getter, its value at load is ECHR_GEMM_H2
    (default 1), and every other user of this switch puts that back as well."""
    from echr_amd import _lib as L
    lib = L.load()
    L.check(lib.echr_config_set(b'gemm_h2', 1 if on else 0), 'config_set')
    try:
        yield
    finally:
        L.check(lib.echr_config_set(b'gemm_h2', int(os.environ.get('ECHR_GEMM_H2', '1'))), 'config_set')


@contextlib.contextmanager
def _node_outputs(seen):
    """What functional._decoder_backward returns (d video, d event, g_h0, d tap, parameter gradients), kept for the record."""
    from echr_amd import functional as EF
    real = EF._decoder_backward

    def spy(ctx, g_logp):
        out = real(ctx, g_logp)
        seen.append(out[:4])
        return out
    EF._decoder_backward = spy
    try:
        yield
    finally:
        EF._decoder_backward = real


def _node_record(rec, seen):
    assert len(seen) == 1, len(seen)
    for key, t in zip(('d_video', 'd_event', 'g_h0', 'd_tap'), seen[0]):
        if t is not None:
            _pin(rec, key, t)
    return rec


def _grads(rec, m):
    ar = getattr(m, '_echr_arena', None)
    if ar is not None and ar.grads_in_arena():
        return _pin(rec, 'grads', ar.flat_g)
    return _pin(rec, 'grads', *[p.grad for _, p in m.named_parameters() if p.grad is not None])


def _inputs(vid, tap_grad=False):
    tap, c3d, lda = (torch.from_numpy(np.ascontiguousarray(vid[k])).cuda() for k in ('tap', 'c3d', 'lda'))
    return tap.requires_grad_(tap_grad), c3d, lda


def _autograd(case, arena, hook=None, staged=True, tap_grad=False, sat=False):
    """forward(mode='train') + LanguageModelCriterion + backward on one video."""
    from echr_amd.misc.utils import LanguageModelCriterion
    opt, params, vid = synth.make_sat_case(case) if sat else synth.make_case(case)
    m = U.build_gpu_model(opt, params, True)
    if arena:
        ar = m.build_arena()
        if hook:
            ar.early_grad_hook = lambda ps, after_recurrence=False: None
            ar.early_staged = staged
    tap, c3d, lda = _inputs(vid, tap_grad)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    loss = LanguageModelCriterion()(m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train'), labels[:, 1:].cuda(), masks[:, 1:].cuda())
    seen = []
    with _node_outputs(seen), _profiled():
        loss.backward()
    rec = _grads(dict(loss=_hex(loss)), m)
    if tap.grad is not None:
        _pin(rec, 'd_tap', tap.grad)
    return rec if sat else _node_record(rec, seen)


def _vbatch(case, tap_leaves=False):
    from echr_amd.batch import VideoBatch
    opt, params, vids = synth.make_vbatch(case)
    taps = [torch.from_numpy(v['tap']).cuda().requires_grad_(tap_leaves) for v in vids]
    b = VideoBatch.from_videos([dict({k: v[k] for k in ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')}, tap=t) for v, t in zip(vids, taps)],
                               device=torch.device('cuda'), CG_init_feats_type=opt.CG_init_feats_type, clip_context_type=opt.clip_context_type)
    return opt, params, b, taps


def _autograd_batch(case, tap_leaves):
    from echr_amd.misc.utils import LanguageModelCriterion
    opt, params, b, taps = _vbatch(case, tap_leaves)
    m = U.build_gpu_model(opt, params, True)
    m.build_arena()
    total, _ = b.criterion(LanguageModelCriterion(), m.forward_batch(b, mode='train'))
    seen = []
    with _node_outputs(seen), _profiled():
        total.backward()
    rec = _node_record(_grads(dict(loss=_hex(total)), m), seen)
    if tap_leaves:
        _pin(rec, 'd_tap', *[t.grad for t in taps])
    return rec


def _fused(opt, params):
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
    return m, o, FusedTrainStep(m, o, grad_clip=opt.grad_clip)


def _step(case):
    """FusedTrainStep(step=False) on one video with host targets / masks, as bench.py hands them over; d tap_feats asked for."""
    opt, params, vid = synth.make_case(case)
    m, o, f = _fused(opt, params)
    tap, c3d, lda = _inputs(vid)
    labels = torch.from_numpy(vid['labels'])
    g_tap = torch.zeros_like(tap)
    with _profiled():
        loss = f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:].numpy(), vid['masks'][:, 1:], step=False, tap_grad=g_tap)
    return _pin(_pin(dict(loss=_hex(loss), active_rows=int(f.last_active_rows)), 'grads', f.arena.flat_g), 'd_tap', g_tap)


def _step_batch(case):
    opt, params, b, _ = _vbatch(case)
    m, o, f = _fused(opt, params)
    with _profiled():
        loss = f.batch(b, step=False)
    return _pin(dict(loss=_hex(loss), video_losses=_hex(f.last_video_losses)), 'grads', f.arena.flat_g)


def _joint():
    from echr_amd import models as EM
    from echr_amd.fused import JointTrainStep
    from echr_amd.optim import ClampAdam
    opt, params, sst_params, vid = synth.make_c5()
    torch.manual_seed(7)
    m, o, f = _fused(opt, params)
    tapm = EM.setup_tap(opt)
    tapm.load_state_dict({k: torch.from_numpy(v) for k, v in sst_params.items()})
    tapm = tapm.cuda()
    tapm.eval()
    tap_o = ClampAdam(tapm.parameters(), lr=1e-3, arena=tapm.build_arena())
    # (order='hook': the library calls back from between the two pieces, which is the proof below that it took that form)
    j = JointTrainStep(f, tapm, tap_o, lambda1=opt.lambda1, tap_grad_clip=opt.grad_clip, order='hook')
    _, c3d, lda = _inputs(dict(vid, tap=np.zeros((1, 1), np.float32)))
    labels = torch.from_numpy(vid['labels'])
    tl, tm, tw = (torch.from_numpy(vid[k]).cuda() for k in ('tap_labels', 'tap_masks', 'w1'))
    with _profiled():
        total = j(c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:].numpy(), vid['masks'][:, 1:], tm, tl, tw)
        f.join()
    assert f.mid_called          # the library took the two-piece form
    rec = dict(loss=_hex(torch.stack([total.reshape(()), j.tap_loss.reshape(()), j.cg_loss.reshape(())])))
    return _pin(_pin(_pin(rec, 'grads', f.arena.flat_g), 'params', f.arena.flat_p), 'tap_params', tapm._echr_arena.flat_p)


def _run(name):
    what, _, arm = name.partition('|')
    with _gemm_h2(arm != 'native'):
        if what == 'autograd':
            return _autograd('c1', False)
        if what == 'arena':
            return _autograd('c1', True)
        if what == 'arena_d_video':
            return _autograd_batch('vbinit', True)
        if what in ('hook_staged', 'hook_onecall'):
            return _autograd('c1', True, hook=True, staged=what == 'hook_staged')
        if what == 'step':
            return _step('er2')
        if what == 'joint':
            return _joint()
        if what == 'step_batch':
            return _step_batch('vbctx')
        if what == 'forward_batch':
            return _autograd_batch('vbctx', False)
        if what == 'arena_init':
            return _autograd('initc', True)
        if what == 'step_init':
            return _step('initc')
        if what == 'shared_rows':
            return _step('vctx')
        if what == 'sat':
            return _autograd('sat_vec_init', False, tap_grad=True, sat=True)
    raise KeyError(name)


def run(name):
    """The bits of one run.  The caller has deterministic mode on."""
    _prof['on'] = False
    return _run(name)


def launches(name):
    """The launch count of every profile kind for one run.  The caller has deterministic mode off."""
    _prof['on'], _prof['counts'] = True, None
    try:
        _run(name)
    finally:
        _prof['on'] = False
    return _prof['counts']

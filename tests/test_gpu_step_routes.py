"""Which library entry each training mode runs (-m gpu): the one-call step has six entries (echr_train_step, _rw, _clip, _batch, _batch_tap,
_batch_clip) and every step object of echr_amd/fused.py reaches exactly one of them per iteration.  A recording proxy sits in front of
`FusedTrainStep.lib`; it notes every echr_train_step* call with the scalar fields of the argument struct at that moment, so the per-call
fields (prepared, mid_cb, the hand-over fields, g_loss) are checked as the library saw them, and after the call g_loss must be the
object's unit scalar again.

Shapes: the smallest the batch tests use (tests/test_gpu_criterion_widths.py): two videos of 2 and 1 events, 4 segments, 9 feature rows,
label width 4 (S = 3), 31 words.  Nothing numerical is checked here; the parity suites do that.
"""
import functools

import numpy as np
import pytest
import torch

from echr_amd import synth
from tests import util as U

pytestmark = pytest.mark.gpu

V1, L_, SEG, T_V, K = 31, 4, 4, 9, 8
KEYS = ('c3d', 'tap', 'lda', 'ind', 'soi', 'labels', 'masks')
SCALARS = ('prepared', 'defer_update', 'handover', 'do_step', 'forward_only', 'host_nll')
POINTERS = ('handover_cb', 'handover_user', 'mid_cb', 'mid_user', 'g_tap', 'g_loss')


class Recorder(object):
    """Delegates every attribute to the library; an echr_train_step* entry is noted first (`fail`: that entry returns -22 instead of running)."""

    def __init__(self, lib):
        self._lib, self.calls, self.fail = lib, [], None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('echr_train_step') or name.endswith('_ws_floats') or name == 'echr_train_step_prepare':
            return fn

        def entry(*args):
            from echr_amd import _lib as L
            a = args[0]._obj
            rec = dict(entry=name[len('echr_train_step'):])
            rec.update({k: int(getattr(a, k)) for k in SCALARS})
            rec.update({k: getattr(a, k) for k in POINTERS})
            for arg in args[1:]:
                if isinstance(getattr(arg, '_obj', None), L.ClipStepArgs):
                    rec['x.rw'] = int(arg._obj.rw)
            self.calls.append(rec)
            return -22 if self.fail == name else fn(*args)
        return entry


@functools.lru_cache(maxsize=None)
def _case(clip):
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=L_ - 2, clip_context_type=clip, K=K)
    params = synth.make_params(opt, 3)
    vids = [synth.make_video(n, SEG, L_, V1, seed=77 + 100 * i, T_v=T_V, min_len=1) for i, n in enumerate((2, 1))]
    return opt, params, synth.make_sst_params(opt, 7), vids


def _fused(clip):
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    opt, params, sst_params, vids = _case(clip)
    m = U.build_gpu_model(opt, params, True)
    f = FusedTrainStep(m, ClampAdam(m.parameters(), lr=1e-9, arena=m.build_arena()), grad_clip=None)
    f.lib = Recorder(f.lib)          # in front of the library BEFORE any wrapping step object copies `f.lib`
    return f, f.lib, opt, sst_params, vids


def _joint(f, opt, sst_params, lambda2=1.0):
    from echr_amd import models
    from echr_amd.fused import JointBatchStep
    from echr_amd.optim import ClampAdam
    tm = models.setup_tap(opt)
    tm.load_state_dict({k: torch.from_numpy(v) for k, v in sst_params.items()})
    tm = tm.cuda()
    tm.train()
    tm.set_dropout_state(U.SEED, U.OFFSET)
    return JointBatchStep(f, tm, ClampAdam(tm.parameters(), lr=1e-9, arena=tm.build_arena()), lambda1=0.01, lambda2=lambda2)


def _batch(opt, vids):
    from echr_amd.batch import VideoBatch
    return VideoBatch.from_videos([{k: v[k] for k in KEYS} for v in vids], device=torch.device('cuda'), clip_context_type=opt.clip_context_type)


def _one(f, vid, **kw):
    tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    return f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], **kw)


def _scst(f, vid):
    from echr_amd.fused import SelfCriticalStep
    tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
    gen = vid['labels'][:, 1:L_ - 1].copy()
    gen[gen == 0] = 1
    return SelfCriticalStep(f)(tap, c3d, lda, vid['ind'], vid['soi'], gen_result=gen, reward=np.linspace(-1.0, 1.0, len(gen)).astype(np.float32))


def _scst_batch(f, opt, vids):
    from echr_amd.fused import SelfCriticalBatchStep
    gen = np.concatenate([v['labels'][:, 1:L_ - 1] for v in vids], 0).copy()
    gen[gen == 0] = 1
    return SelfCriticalBatchStep(f)(_batch(opt, vids), gen_result=gen, reward=np.linspace(-1.0, 1.0, len(gen)).astype(np.float32))


def _joint_call(js, vids, **kw):
    T = sum(min(len(v['c3d']), len(v['tap'])) for v in vids)
    videos = [{k: v[k] for k in KEYS if k != 'tap'} for v in vids]
    return js(videos, torch.ones(T, K), torch.zeros(T, K), torch.full((K,), 0.5), **kw)


def _expect(f, rec, entry, g_loss=None, **fields):
    """Exactly one entry ran, the named one; the per-call fields are what the case asked for (everything not named: off / NULL); g_loss
    was the unit scalar (or `g_loss`) during the call and is the unit scalar after it."""
    torch.cuda.synchronize()
    assert [c['entry'] for c in rec.calls] == [entry], rec.calls
    c = rec.calls.pop()
    unit = f.one.data_ptr()
    want = dict(prepared=0, defer_update=0, handover=0, handover_cb=False, mid_cb=False, g_tap=False)
    want.update(fields)
    for k, v in want.items():
        got = bool(c[k]) if isinstance(v, bool) else c[k]
        assert got == v, (entry, k, c[k], v)
    assert c['handover_user'] is None and c['mid_user'] is None
    assert c['g_loss'] == (unit if g_loss is None else g_loss.data_ptr())
    assert f.a.g_loss == unit
    return c


# ---- the configurations: what runs, the entry that must run, the fields that must be set --------------------------------------------
def _cc_one(f, rec, opt, sst, vids):
    _one(f, vids[0])
    _expect(f, rec, '', do_step=1)


def _cc_scst(f, rec, opt, sst, vids):
    _scst(f, vids[0])
    _expect(f, rec, '_rw', do_step=1, host_nll=1)


def _ch_one(f, rec, opt, sst, vids):
    _one(f, vids[0])
    assert _expect(f, rec, '_clip', do_step=1)['x.rw'] == 0


def _cch_scst(f, rec, opt, sst, vids):
    _scst(f, vids[0])
    assert _expect(f, rec, '_clip', do_step=1)['x.rw'] == 1


def _cc_batch(f, rec, opt, sst, vids):
    f.batch(_batch(opt, vids))
    _expect(f, rec, '_batch', do_step=1)


def _cc_scst_batch(f, rec, opt, sst, vids):
    _scst_batch(f, opt, vids)
    _expect(f, rec, '_batch', do_step=1)


def _cc_joint(f, rec, opt, sst, vids):
    js = _joint(f, opt, sst)
    _joint_call(js, vids)
    _expect(f, rec, '_batch_tap', do_step=1, g_tap=True, g_loss=js.lam[1:])          # (lambda2 travels as the call's g_loss, 1.0 too)


def _ch_batch(f, rec, opt, sst, vids):
    f.batch(_batch(opt, vids))
    _expect(f, rec, '_batch_clip', do_step=1, g_tap=False)


def _ch_joint(f, rec, opt, sst, vids):
    js = _joint(f, opt, sst)
    _joint_call(js, vids)
    _expect(f, rec, '_batch_clip', do_step=1, g_tap=True, g_loss=js.lam[1:])


def _handover(entry):
    def run(f, rec, opt, sst, vids):
        seen = []
        f.batch_handover(_batch(opt, vids), lambda which, stream: seen.append(which))
        _expect(f, rec, entry, do_step=0, handover=1, handover_cb=True)
        f.batch_handover(_batch(opt, vids))          # the event form: no callback
        _expect(f, rec, entry, do_step=0, handover=1, handover_cb=False)
    return run


CASES = {'CC one video': ('CC', _cc_one), 'SelfCriticalStep': ('CC', _cc_scst), 'CH one video': ('CH', _ch_one),
         'SelfCriticalStep on CC+CH': ('CC+CH', _cch_scst), 'batch()': ('CC', _cc_batch), 'SelfCriticalBatchStep': ('CC', _cc_scst_batch),
         'JointBatchStep on CC': ('CC', _cc_joint), 'batch() on CH': ('CH', _ch_batch), 'JointBatchStep on CH': ('CH', _ch_joint),
         'batch_handover': ('CC', _handover('_batch')), 'batch_handover on CH': ('CH', _handover('_batch_clip'))}


@pytest.mark.parametrize('name', list(CASES))
def test_each_configuration_runs_its_entry(name):
    clip, run = CASES[name]
    f, rec, opt, sst, vids = _fused(clip)
    run(f, rec, opt, sst, vids)


@pytest.mark.parametrize('clip', ['CC', 'CH'])
def test_nothing_is_left_over_from_the_previous_call(clip):
    """ONE object through hand-over with a callback, a joint step with lambda2 = 0.5, a plain batch, one video with tap_grad, one video
    plain: each call's fields are its own."""
    f, rec, opt, sst, vids = _fused(clip)
    one, many, tap = ('', '_batch', '_batch_tap') if clip == 'CC' else ('_clip', '_batch_clip', '_batch_clip')
    f.batch_handover(_batch(opt, vids), lambda which, stream: None)
    _expect(f, rec, many, do_step=0, handover=1, handover_cb=True)
    js = _joint(f, opt, sst, lambda2=0.5)
    _joint_call(js, vids, step=False)
    _expect(f, rec, tap, do_step=0, g_tap=True, g_loss=js.lam[1:])
    assert float(js.lam[1]) == 0.5
    f.batch(_batch(opt, vids), forward_only=True)
    _expect(f, rec, many, do_step=0, forward_only=1)
    tap_feats = torch.from_numpy(vids[0]['tap']).cuda()
    _one(f, vids[0], step=False, handover=True, tap_grad=torch.zeros_like(tap_feats))
    _expect(f, rec, one, do_step=0, handover=1, g_tap=True)
    _one(f, vids[0])
    _expect(f, rec, one, do_step=1)
    f.batch(_batch(opt, vids))
    _expect(f, rec, many, do_step=1)


def test_a_refused_call_propagates_and_restores_g_loss():
    """The proxy answers -22 for echr_train_step_batch_tap without running it: EchrHipError reaches the caller of JointBatchStep, and the
    argument struct holds the unit scalar again although lambda2 = 0.5 was in place for the call."""
    from echr_amd._lib import EchrHipError
    f, rec, opt, sst, vids = _fused('CC')
    js = _joint(f, opt, sst, lambda2=0.5)
    rec.fail = 'echr_train_step_batch_tap'
    with pytest.raises(EchrHipError):
        _joint_call(js, vids)
    torch.cuda.synchronize()
    assert [c['entry'] for c in rec.calls] == ['_batch_tap']
    assert rec.calls[0]['g_loss'] == js.lam[1:].data_ptr() != f.one.data_ptr()
    assert f.a.g_loss == f.one.data_ptr()
    rec.fail, rec.calls = None, []
    f.batch(_batch(opt, vids))          # the object goes on working
    _expect(f, rec, '_batch', do_step=1)

"""CPU: the refusals of the self-critical entries -- fused.SelfCriticalStep, fused.SelfCriticalBatchStep (__call__ and handover),
CaptionGenerator.forward(mode='train_rl') and train_rl_batch -- against the ones recorded BEFORE the two step classes shared one
iteration and the two module paths one body (tests/golden/scst_contract.json; `python -m tests.test_scst_contract_host` rewrites it).

Every call runs on CPU tensors, where each path ends in a Python refusal or in EchrHipError before any kernel runs.  One valid argument
set per entry with ONE thing wrong -- or two, where the record pins which of two refusals comes first (each class keeps its own order
among the batch-option check, the reference rules and the pending-prepare check); a record is (entry, variation, exception type,
message) and both are compared.

Not recordable here, because today they are raised only behind the decodes' device calls, so that on the CPU the device refusal comes
first (their variations are recorded all the same, as the EchrHipError they end in today): 'needs reward_fn or an explicit reward', the
reward-shape refusals ('reward must be [N, T] or [N]', 'reward must be [N_tot, T] or [N_tot]', 'reward_fn must return [N_v, T_v] or
[N_v]'), gen_result with the wrong row count, the T == 0 refusal, and train_rl_batch's scheduled-sampling refusal.  The reward-shape
messages are asserted on the host function itself in tests/test_sampled_criterion_host.py, SelfCriticalStep's two refusals of a pinned
gen_result with a row too many on the GPU in tests/test_gpu_scst_unify.py.
"""
import json
import os

import numpy as np
import torch

import echr_amd
from echr_amd import functional as EF
from echr_amd import reward as RW
from echr_amd import synth
from echr_amd.batch import VideoBatch
from echr_amd.fused import FusedTrainStep, SelfCriticalBatchStep, SelfCriticalStep

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scst_contract.json')
KEYS = ('c3d', 'tap', 'lda', 'ind', 'soi')
T = 3


def _model(**options):
    opt, _, videos = synth.make_vbatch('vbscst')
    for k, v in options.items():
        setattr(opt, k, v)
    return echr_amd.CaptionGenerator(opt), videos


def base():
    """A valid argument set on the CPU: the 'vbscst' videos as a batch, its first video for the single-video entries, and a FusedTrainStep
    as far as the steps read it ahead of the device (the library has no CPU path: the real constructor needs the GPU)."""
    m, videos = _model()
    f = object.__new__(FusedTrainStep)
    f.model, f.lib, f.dev, f._prepared, f._pending_deferred = m, EF.L.load(), torch.device('cpu'), False, False
    docs = [[lab] for v in videos for lab in np.asarray(v['labels'])]
    v0 = videos[0]
    return dict(model=m, videos=videos, fused=f, reward_fn=lambda gen, greedy: np.zeros(len(gen), np.float32), reward=None, gen_result=None,
                refs=None, docs=docs, scorer=RW.CiderD.from_corpus(docs, m.opt.CG_seq_length, m.opt.CG_vocab_size),
                batch=VideoBatch.from_videos([{k: v[k] for k in KEYS} for v in videos]), n0=len(v0['soi']),
                video=tuple(torch.from_numpy(v0[k]) for k in ('tap', 'c3d', 'lda')) + (v0['ind'], v0['soi']))


def _step(a):
    tap, c3d, lda, ind, soi = a['video']
    refs = a['refs'] if a['refs'] is None else a['scorer'].pack_refs(a['docs'][:a['n0']])
    return SelfCriticalStep(a['fused'], a['reward_fn'])(tap, c3d, lda, ind, soi, gen_result=_rows(a, a['n0']), reward=_rows(a, a['n0'], 'reward'),
                                                        refs=refs)


def _rows(a, n, key='gen_result'):
    """The variation's gen_result / reward (built for the batch's N_tot rows) cut for an entry of `n` rows, its row surplus kept."""
    x = a[key]
    return x if x is None else x[:n + len(x) - a['batch'].n_events]


def _batch_step(a, handover=False):
    a['batch'].refs = a['refs']
    s = SelfCriticalBatchStep(a['fused'], a['reward_fn'])
    if handover:
        return s.handover(a['batch'], gen_result=a['gen_result'], reward=a['reward'])
    return s(a['batch'], gen_result=a['gen_result'], reward=a['reward'])


def _train_rl(a):
    tap, c3d, lda, ind, soi = a['video']
    return a['model'](tap, c3d, lda, [], ind, soi, mode='train_rl', gen_result=_rows(a, a['n0']))


CALLS = {
    'SelfCriticalStep': _step,
    'SelfCriticalBatchStep': _batch_step,
    'SelfCriticalBatchStep.handover': lambda a: _batch_step(a, True),
    "forward(mode='train_rl')": _train_rl,
    'train_rl_batch': lambda a: a['model'].train_rl_batch(a['batch'], gen_result=a['gen_result']),
    'SelfCriticalStep.batch': lambda a: SelfCriticalStep(a['fused']).batch(a['batch']),
    "forward_batch(mode='train_rl')": lambda a: a['model'].forward_batch(a['batch'], mode='train_rl'),
}
STEPS = ('SelfCriticalStep', 'SelfCriticalBatchStep', 'SelfCriticalBatchStep.handover')
BATCH_STEPS = STEPS[1:]
BATCHED = BATCH_STEPS + ('train_rl_batch',)
LIVE = STEPS + ("forward(mode='train_rl')", 'train_rl_batch')
EVERY = tuple(CALLS)


def _other_model(a, **options):
    a['model'] = a['fused'].model = _model(**options)[0]


def _other_batch(a, **options):
    a['batch'] = VideoBatch.from_videos([{k: v[k] for k in KEYS} for v in a['videos']], **options)


def _gen(a, rows=0):
    a['gen_result'] = np.ones((a['batch'].n_events + rows, T), np.int64)


def _ciderd(a, refs):
    a['reward_fn'] = RW.CiderDReward(a['scorer'])
    a['refs'] = a['scorer'].pack_refs(a['docs']) if refs else None


def _both(*edits):
    return lambda a: [e(a) for e in edits]


_no_refs = lambda a: _ciderd(a, False)
_prepared = lambda a: setattr(a['fused'], '_prepared', True)
_init_model = lambda a: _other_model(a, CG_init_feats_type='V')
# (variation, the entries it is applied to, the edit of the valid argument set)
VARIATIONS = [
    ('valid arguments on the CPU', EVERY, lambda a: None),
    ('wrapping a non-FusedTrainStep', STEPS, lambda a: a.update(fused=object())),
    ('CiderDReward without refs', STEPS, _no_refs),
    ('CiderDReward with refs', STEPS, lambda a: _ciderd(a, True)),
    ('CiderDReward without refs, an explicit reward', STEPS, _both(_no_refs, lambda a: a.update(reward=np.zeros(a['batch'].n_events, np.float32)))),
    ('refs with a plain callable', STEPS, lambda a: a.update(refs=a['scorer'].pack_refs(a['docs']))),
    ('refs with no reward_fn', STEPS, lambda a: a.update(reward_fn=None, refs=a['scorer'].pack_refs(a['docs']))),
    ('no reward_fn and no reward', STEPS, lambda a: a.update(reward_fn=None)),
    ('reward [N+1]', STEPS, _both(_gen, lambda a: a.update(reward=np.zeros(a['batch'].n_events + 1, np.float32)))),
    ('reward [N, T-1]', STEPS, _both(_gen, lambda a: a.update(reward=np.zeros((a['batch'].n_events, T - 1), np.float32)))),
    ('gen_result one row too many', LIVE, lambda a: _gen(a, 1)),
    ('a pending prepare()', STEPS, _prepared),
    ('a pending prepare(), CiderDReward without refs', STEPS, _both(_prepared, _no_refs)),
    ('a plain batch, the model has CG_init_feats_type', BATCHED, _init_model),
    ('a batch for CG_init_feats_type, a plain model', BATCHED, lambda a: _other_batch(a, CG_init_feats_type='V')),
    ('a plain batch, the model has clip_context_type CH', BATCHED, lambda a: _other_model(a, clip_context_type='CH')),
    ('a batch for clip_context_type CH, a plain model', BATCHED, lambda a: _other_batch(a, clip_context_type='CH')),
    ('a plain batch for an init model, CiderDReward without refs', BATCH_STEPS, _both(_init_model, _no_refs)),
    ('a plain batch for an init model, a pending prepare()', BATCH_STEPS, _both(_init_model, _prepared)),
]


def record(calls=CALLS):
    out = []
    for variation, entries, edit in VARIATIONS:
        for e in entries:
            a = base()
            edit(a)
            try:
                calls[e](a)
                out.append([e, variation, '', ''])
            except Exception as ex:          # noqa: BLE001 (the record IS the exception)
                out.append([e, variation, type(ex).__name__, str(ex)])
    return out


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_every_recorded_call_was_refused():
    """The fixture itself: every call ended in an exception, the valid ones in the library's EchrHipError or the standing
    NotImplementedError of the two closed forms, and the Python refusals come ahead of the device in each class's own order."""
    want = _fixture()
    assert len(want) == sum(len(entries) for _, entries, _ in VARIATIONS) and all(r[2] for r in want)
    by = {(e, v): (t, m) for e, v, t, m in want}
    assert all(by[e, 'valid arguments on the CPU'][0] == 'EchrHipError' for e in LIVE)
    assert by['SelfCriticalStep.batch', 'valid arguments on the CPU'][0] == by["forward_batch(mode='train_rl')", 'valid arguments on the CPU'][0] \
        == 'NotImplementedError'
    assert 'SelfCriticalBatchStep(fused)(batch)' in by['SelfCriticalStep.batch', 'valid arguments on the CPU'][1]
    assert by['SelfCriticalStep', 'wrapping a non-FusedTrainStep'] == ('TypeError', 'SelfCriticalStep wraps a FusedTrainStep')
    assert all(by[e, 'wrapping a non-FusedTrainStep'] == ('TypeError', 'SelfCriticalBatchStep wraps a FusedTrainStep') for e in BATCH_STEPS)
    for e in STEPS:
        assert by[e, 'CiderDReward without refs'][0] == 'ValueError' and by[e, 'refs with a plain callable'][0] == 'TypeError'
        assert by[e, 'refs with no reward_fn'][0] == 'TypeError'
        assert by[e, 'CiderDReward without refs, an explicit reward'][0] == 'EchrHipError'          # (allowed: the reward is not called)
        assert by[e, 'a pending prepare(), CiderDReward without refs'][0] == 'ValueError'          # the reference rules come ahead of _begin
    assert by['SelfCriticalStep', 'a pending prepare()'][0] == 'RuntimeError'
    for e in BATCH_STEPS:
        assert by[e, 'a pending prepare()'][0] == 'NotImplementedError' and 'a batch step' in by[e, 'a pending prepare()'][1]
        # the batch-option check comes ahead of both
        assert by[e, 'a plain batch for an init model, CiderDReward without refs'] == by[e, 'a plain batch, the model has CG_init_feats_type']
        assert by[e, 'a plain batch for an init model, a pending prepare()'] == by[e, 'a plain batch, the model has CG_init_feats_type']
    for e in BATCHED:
        assert by[e, 'a plain batch, the model has CG_init_feats_type'][0] == 'NotImplementedError'
        assert by[e, 'a plain batch, the model has clip_context_type CH'][0] == 'NotImplementedError'
        assert by[e, 'a batch for CG_init_feats_type, a plain model'][0] == 'ValueError'
        assert by[e, 'a batch for clip_context_type CH, a plain model'][0] == 'ValueError'


def test_refusals_are_the_recorded_ones():
    got, want = record(), _fixture()
    assert [r[:2] for r in got] == [r[:2] for r in want]
    for g, w in zip(got, want):
        assert g == w, (g, w)


if __name__ == '__main__':
    with open(FIXTURE, 'w') as f:
        json.dump(record(), f, indent=1)
        f.write('\n')
    print('wrote', FIXTURE)

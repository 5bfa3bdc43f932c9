"""The six self-critical runs that tests/golden/scst_unify.json pins bit for bit (tools/make_golden_scst_unify.py records them,
tests/test_gpu_scst_unify.py replays them): SelfCriticalStep and SelfCriticalBatchStep, each with a host callable and with a device
CiderDReward, and the two module paths with their criteria and a backward pass.  Deterministic mode, a fixed dropout seed and call count,
so the captions are really drawn; the existing tiny cases only ('tiny_eos' for one video, 'vbscst' for the batch).

A record holds: gen / greedy (integer lists), video_words, the loss and the reward as the hex of their fp32 bytes, a sha256 of the flat
gradient arena, and for the step classes a sha256 of the flat parameters after one more call with step=True and the optimiser's
applied-step count behind it.  The event's references of the CIDEr-D runs are its own label and the two captions the reference's fixture
holds for it (a random model's captions share next to nothing with the random labels alone)."""
import hashlib

import numpy as np
import torch

from echr_amd import reward as RW
from echr_amd import synth
from tests import util as U

SEED, CALLS = 0x5C57, 11
RUNS = ('step|callable', 'step|ciderd', 'batch_step|callable', 'batch_step|ciderd', 'train_rl', 'train_rl_batch')


def reward_fn(gen, greedy):
    """A fixed host reward per caption: sampled captions longer than the baseline's are rewarded."""
    lg = (gen > 0).sum(1).float()
    lb = (greedy > 0).sum(1).float() if greedy.numel() else torch.zeros(gen.shape[0])
    return (lg - lb) / 4.0 - 0.1


def _sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def _hex(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).tobytes().hex()


def _ints(x):
    return x.cpu().numpy().tolist() if isinstance(x, torch.Tensor) else np.asarray(x).tolist()


def _single():
    opt, params, vid = synth.make_case('tiny_eos')
    g = U.gold('case_scst_eos.npz')
    docs = [[lab, [int(t) for t in a if t], [int(t) for t in b if t]] for lab, a, b in zip(np.asarray(vid['labels']), g['gen_result'], g['greedy_res'])]
    return opt, params, vid, docs


def _videos():
    from tests import scst_batch_ref as R
    opt, params, videos = synth.make_vbatch('vbscst')
    gens, _, greedys, _, _ = R.load_fixture(U.gold('case_scst_batch.npz'), len(videos))
    docs = [[lab, [int(t) for t in a if t], [int(t) for t in b if t]]
            for v, vid in enumerate(videos) for lab, a, b in zip(np.asarray(vid['labels']), gens[v], greedys[v])]
    return opt, params, videos, docs


def _model(opt, params):
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
    return m, o, FusedTrainStep(m, o, grad_clip=0.1)


def _batch(videos):
    from echr_amd.batch import VideoBatch
    return VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi')} for v in videos], device=torch.device('cuda'))


def _scorer(opt, docs):
    return RW.CiderD.from_corpus(docs, opt.CG_seq_length, opt.CG_vocab_size).cuda()


def _step_record(m, o, f, call):
    """`call(step)` is one iteration of a step class: once with step=False (its outputs and gradients), once with step=True (the update)."""
    m.set_dropout_state(SEED, CALLS)
    out = call(False)
    rec = dict(loss=_hex(out[0]), gen=_ints(out[1]), greedy=_ints(out[2]), reward=_hex(out[3]), video_words=_ints(out[4]) if len(out) > 4 else None,
               grads=_sha(f.arena.flat_g))
    m.set_dropout_state(SEED, CALLS)
    call(True)
    rec['params'], rec['applied_steps'] = _sha(f.arena.flat_p), int(o._flat['step'])
    return rec


def _module_record(f, gen, greedy, reward, loss, vw=None):
    loss.backward()
    return dict(loss=_hex(loss), gen=_ints(gen), greedy=_ints(greedy), reward=_hex(reward), video_words=None if vw is None else _ints(vw),
                grads=_sha(f.arena.flat_g))


def run(name):
    from echr_amd.fused import SelfCriticalBatchStep, SelfCriticalStep
    from echr_amd.misc.utils import RewardCriterion
    what, _, source = name.partition('|')
    if what in ('step', 'train_rl'):
        opt, params, vid, docs = _single()
        m, o, f = _model(opt, params)
        args = tuple(torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
        if what == 'train_rl':
            m.set_dropout_state(SEED, CALLS)
            gen, slp, greedy = m(*args, [], vid['ind'], vid['soi'], mode='train_rl')
            r = reward_fn(gen.cpu(), torch.as_tensor(greedy).cpu() if isinstance(greedy, torch.Tensor) else torch.zeros(len(gen), 0))
            return _module_record(f, gen, greedy, r, RewardCriterion()(slp, gen, r.cuda()))
        if source == 'ciderd':
            sc = _scorer(opt, docs)
            step, refs = SelfCriticalStep(f, RW.CiderDReward(sc, weight=2.0)), sc.pack_refs(docs).cuda()
            return _step_record(m, o, f, lambda s: step(*args, vid['ind'], vid['soi'], refs=refs, step=s))
        step = SelfCriticalStep(f, reward_fn)
        return _step_record(m, o, f, lambda s: step(*args, vid['ind'], vid['soi'], step=s))
    opt, params, videos, docs = _videos()
    m, o, f = _model(opt, params)
    b = _batch(videos)
    if what == 'train_rl_batch':
        m.set_dropout_state(SEED, CALLS)
        gen, slp, greedy, vw = m.train_rl_batch(b)
        gen_h, greedy_h = gen.cpu(), greedy.cpu() if isinstance(greedy, torch.Tensor) else torch.zeros(len(gen), 0, dtype=torch.int64)
        r = np.zeros(tuple(gen_h.shape), np.float32)
        for s, w in zip(b.event_slices, vw.tolist()):
            if w:
                r[s, :w] = reward_fn(gen_h[s, :w], greedy_h[s]).numpy()[:, None]
        total, _ = b.reward_criterion(RewardCriterion(), slp, gen, r, vw)
        return _module_record(f, gen, greedy, r, total, vw)
    if source == 'ciderd':
        sc = _scorer(opt, docs)
        b.refs = sc.pack_refs(docs).cuda()
        step = SelfCriticalBatchStep(f, RW.CiderDReward(sc, weight=0.5))
    else:
        step = SelfCriticalBatchStep(f, reward_fn)
    return _step_record(m, o, f, lambda s: step(b, step=s))


def run_all():
    import echr_amd
    echr_amd.set_deterministic(True)
    try:
        return {name: run(name) for name in RUNS}
    finally:
        echr_amd.set_deterministic(False)

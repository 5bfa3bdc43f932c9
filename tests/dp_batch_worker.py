"""Worker of tests/test_gpu_dp_batch.py: one data-parallel rank of fused.DataParallelBatchStep (gloo transport, both ranks on cuda:0 -- or,
with backend 'nccl' and world size 1, the RCCL code path of every collective), modelled on tests/dp_worker.py.  The builders below are the
test's too: the single-process references run the same models on the same rank batches under the same pinned dropout states.

usage: dp_batch_worker.py RANK WORLD PORT OUT SPEC   (SPEC: the JSON of `spec(...)`)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K_TAP = 16
LR, CLIP = 1e-3, 0.05
LAMBDA1, LAMBDA2 = 0.01, 1.0
KEYS = ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')
# (events, T_v) of the global video i of an update: 1-3 events, T_v 24-40, neighbours in a shard differ in both
SHAPES = ((2, 24), (3, 32), (1, 40), (2, 28))


def spec(kind='caption', clip='CC', mode='lpp', n_videos=4, steps=2, reduce_loss=False, via='callback', algo=None, backend='gloo'):
    """kind: 'caption' | 'joint' | 'scst' | 'single' (DataParallelStep, one video per rank); mode: 'lpp' (staged, launch-per-phase
    recurrences) | 'coop' (staged, cooperative persistent launches) | 'one' (ONE collective, launch-per-phase)."""
    return dict(kind=kind, clip=clip, mode=mode, n_videos=n_videos, steps=steps, reduce_loss=reduce_loss, via=via, algo=algo, backend=backend)


def case(clip='CC'):
    """synth.make_case('c1')'s model for the frame-level context `clip` (+ the proposal encoder's parameters, K = 16)."""
    from echr_amd import synth
    opt, _, _ = synth.make_case('c1')
    opt.clip_context_type = clip
    opt.K = K_TAP
    return opt, synth.make_params(opt, 0), synth.make_sst_params(opt)


def videos(opt, step, n):
    """The n global videos of update `step` (synth.make_video, label width 11), each with its proposal-criterion and self-critical inputs."""
    from echr_amd import synth
    out = []
    for i in range(n):
        N, T = SHAPES[i % len(SHAPES)]
        v = synth.make_video(N, 16, 11, opt.CG_vocab_size + 1, seed=700 + 50 * step + i, T_v=T, video_dim=opt.video_dim,
                             hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
        rs = np.random.RandomState(900 + 50 * step + i)
        v['tap_labels'] = (rs.uniform(size=(T, K_TAP)) > 0.9).astype(np.float32)
        v['tap_masks'] = (np.arange(T)[:, None] >= np.arange(K_TAP)[None, :]).astype(np.float32)
        v['w1'] = rs.uniform(0.05, 0.3, size=(K_TAP,)).astype(np.float32)
        # a pinned sample of 1..6 words per caption (the rows end at different steps) and a signed reward per caption
        gen = np.zeros((N, opt.CG_seq_length), np.int64)
        for n_ in range(N):
            w = rs.randint(1, 7)
            gen[n_, :w] = rs.randint(1, opt.CG_vocab_size + 1, size=w)
        v['gen'], v['reward'] = gen, rs.uniform(-1.0, 1.0, size=N).astype(np.float32)
        out.append(v)
    return out


def build(opt, params, sst_params, kind):
    """(caption model, its optimiser, FusedTrainStep, inner step, proposal encoder or None)"""
    from echr_amd import models
    from echr_amd.fused import FusedTrainStep, JointBatchStep, SelfCriticalBatchStep
    from echr_amd.optim import ClampAdam
    from tests import util as U
    model = U.build_gpu_model(opt, params, True)
    optim = ClampAdam(model.parameters(), lr=LR, arena=model.build_arena())
    fused = FusedTrainStep(model, optim, grad_clip=CLIP)
    tm = None
    if kind == 'joint':
        tm = models.setup_tap(opt)
        tm.load_state_dict({k: torch.from_numpy(v) for k, v in sst_params.items()})
        tm = tm.cuda()
        tm.train()
        inner = JointBatchStep(fused, tm, ClampAdam(tm.parameters(), lr=LR, arena=tm.build_arena()), lambda1=LAMBDA1, lambda2=LAMBDA2, tap_grad_clip=CLIP)
    elif kind == 'scst':
        inner = SelfCriticalBatchStep(fused)
    else:
        inner = fused
    return model, optim, fused, inner, tm


def pin_dropout(model, tm, step, rank):
    from tests import util as U
    model.set_dropout_state(U.SEED, U.OFFSET + 10 * step + rank)
    if tm is not None:
        tm.set_dropout_state(U.SEED, U.OFFSET + 10 * step + rank)


def call_args(opt, kind, shard, dev):
    """(positional, keyword) arguments of the inner step -- and of DataParallelBatchStep -- for the videos `shard` (None when it is empty)."""
    from echr_amd.batch import VideoBatch
    if not shard:
        if kind == 'joint':
            return (None, None, None, None), {}
        return (None,), (dict(gen_result=None, reward=None) if kind == 'scst' else {})
    if kind == 'joint':
        return ([{k: v[k] for k in KEYS} for v in shard], [torch.from_numpy(v['tap_masks']) for v in shard],
                [torch.from_numpy(v['tap_labels']) for v in shard], [torch.from_numpy(v['w1']) for v in shard]), {}
    keys = KEYS[:4] if kind == 'scst' else KEYS
    b = VideoBatch.from_videos([dict({k: v[k] for k in keys}, tap=torch.from_numpy(v['tap']).to(dev)) for v in shard], device=dev,
                               clip_context_type=opt.clip_context_type)
    if kind == 'scst':
        return (b,), dict(gen_result=np.concatenate([v['gen'] for v in shard], 0), reward=np.concatenate([v['reward'] for v in shard], 0))
    return (b,), {}


def arena_grads(model, tag):
    ar = model._echr_arena
    return {tag + k: ar.grad_view(i).detach().cpu().numpy().copy() for i, (k, p) in enumerate(model.named_parameters())}


def main():
    import torch.distributed as dist
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    sp = json.loads(sys.argv[5])
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', port
    if sp['backend'] == 'nccl':          # RCCL wants one device per rank: world size 1 on a one-GPU box
        torch.cuda.set_device(0)
        dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', 0))
    else:
        dist.init_process_group('gloo', rank=rank, world_size=world)
    from echr_amd import _lib, parallel
    from echr_amd.fused import DataParallelBatchStep, DataParallelStep
    dev = torch.device('cuda', 0)
    # both ranks share cuda:0: two plain persistent grids must never be half-resident beside each other -- launch-per-phase recurrences (and
    # proposal encoder), or persistent grids launched cooperatively
    lib = _lib.load()
    if sp['mode'] == 'coop':
        lib.echr_config_set(b'persist_coop', 1)
    else:
        for key in (b'persist', b'persist_bwd', b'sst_persist'):
            lib.echr_config_set(key, 0)
    opt, params, sst_params = case(sp['clip'])
    kind = sp['kind']
    model, optim, fused, inner, tm = build(opt, params, sst_params, 'caption' if kind == 'single' else kind)
    kw = dict(overlap=sp['mode'] != 'one', algo=sp['algo'], via=sp['via'])
    dp = DataParallelStep(fused, **kw) if kind == 'single' else DataParallelBatchStep(inner, reduce_loss=sp['reduce_loss'], **kw)
    losses, grads, vloss = [], {}, np.zeros(0, np.float32)
    for step in range(sp['steps']):
        vids = videos(opt, step, sp['n_videos'])
        shard = parallel.shard_batch(vids, rank, world)
        pin_dropout(model, tm, step, rank)
        if kind == 'single':
            v = shard[0]
            tap, c3d, lda = (torch.from_numpy(v[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
            labels = torch.from_numpy(v['labels'])
            loss = dp(tap, c3d, lda, labels, v['ind'], v['soi'], labels[:, 1:].numpy(), v['masks'][:, 1:])
        else:
            args, kwargs = call_args(opt, kind, shard, dev)
            loss = dp(*args, n_videos=sp['n_videos'] if sp['reduce_loss'] else None, **kwargs)
        assert loss.dim() == 0 and loss.is_cuda
        torch.cuda.synchronize()          # (clamp + Adam read the gradient arenas, they do not write them)
        losses.append(float(loss))
        if step == 0:
            grads = arena_grads(model, 'grad|')
            if tm is not None:
                grads.update(arena_grads(tm, 'sstgrad|'))
            if kind != 'single' and dp.last_video_losses is not None:
                vloss = dp.last_video_losses.detach().cpu().numpy()
    state = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    if tm is not None:
        state.update({'sst|' + k: v.detach().cpu().numpy() for k, v in tm.state_dict().items()})
    np.savez(out, n_collectives=dp.n_collectives, n_early=dp.n_early, losses=np.asarray(losses), vloss=vloss, **grads, **state)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()

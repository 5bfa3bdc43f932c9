"""Data-parallel training over multi-video batches on the GPU (-m gpu): the hand-over points of the batched one-call steps, and
fused.DataParallelBatchStep over two ranks that share cuda:0 (gloo transport; tests/dp_batch_worker.py) against single-process batch calls.

The semantics are the reference's m_batch protocol (train.py:281-283,313-317) with the videos on R ranks: gradients and loss are the SUM
over all videos of all ranks (no 1/R, no 1/V), the clamp runs after the reduce, the update is identical on every rank.

Gates: replicas bitwise identical; reduced gradients against the sum of single-process calls at U.grad_close(k, ., ., 1e-5), the bound of
test_two_rank_data_parallel_on_one_gpu (two runs of the same kernels differ by the order of their split-K atomics only); losses at 1e-5
relative, the bound of the criterion's batch tests (tests/test_gpu_vbatch.py, tests/test_gpu_joint_batch.py: TOL_LOSS)."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dp_batch_worker as W
from tests import util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_GRAD = 1e-5
TOL_LOSS = 1e-5
WORKER_TIMEOUT = 300


def _dev():
    return torch.device('cuda')


# ---- 1. / 7. hand-over points see final ranges -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _snapshot_case(clip, vctx):
    from echr_amd import synth
    opt, params, sst_params = W.case(clip)
    if vctx is not None:
        opt.video_context_type = vctx
        params = synth.make_params(opt, 0)
    vids = W.videos(opt, 0, 3)          # 2 / 3 / 1 events, T_v 24 / 32 / 40
    assert [len(v['soi']) for v in vids] == [2, 3, 1] and len({v['T_v'] for v in vids}) == 3
    return opt, params, sst_params, vids


def _set_config(cfg):
    import echr_amd
    from echr_amd import _lib
    lib = _lib.load()
    lpp = cfg == 'lpp'
    for key, env in ((b'persist', 'ECHR_PERSIST'), (b'persist_bwd', 'ECHR_PERSIST_BWD')):
        assert lib.echr_config_set(key, 0 if lpp else int(os.environ.get(env, '1'))) == 0
    echr_amd.set_deterministic(cfg == 'det' or os.environ.get('ECHR_DETERMINISTIC', '0') == '1')


@pytest.mark.parametrize('path,clip,vctx,cfg', [
    ('batch', 'CC', None, 'default'), ('batch', 'CH', None, 'default'), ('batch', 'CC+CH', None, 'default'),
    ('batch', 'CC', None, 'lpp'), ('batch', 'CH', None, 'lpp'), ('batch', 'CC+CH', None, 'lpp'),
    ('tap', 'CC', None, 'default'), ('tap', 'CC', None, 'lpp'),
    ('tap', 'CC+CH', None, 'default'), ('tap', 'CC+CH', None, 'lpp'),          # the compacted clip-row gradient joins g_tap
    ('tap', 'CC', 'VLVCVH', 'default'),                                          # the 'VH' span goes into g_tap
    ('scst', 'CC', None, 'default'),                                             # reward weights
    ('batch', 'CC', None, 'det'), ('tap', 'CC+CH', None, 'det'),                 # fixed-order mode
    ('single', 'CC+CH', None, 'default'), ('single', 'CC+CH', None, 'lpp'), ('single', 'CH', None, 'default'),          # echr_train_step_clip
])
def test_handover_points_see_final_ranges_over_a_batch(path, clip, vctx, cfg):
    """test_handover_points_see_final_ranges for the batched entries (and echr_train_step_clip): a snapshot copy queued on the stream the
    hand-over callback receives -- exactly where DataParallelBatchStep queues its collective -- must be bit-equal to the final range.  Three
    videos of 2 / 3 / 1 events and different T_v, captions that end at different steps (the active-row compaction is live), three
    repetitions, the default configuration and the launch-per-phase recurrences."""
    from echr_amd.fused import DataParallelBatchStep, DataParallelStep
    opt, params, sst_params, vids = _snapshot_case(clip, vctx)
    dev = _dev()
    _set_config(cfg)
    try:
        model, optim, f, inner, _ = W.build(opt, params, sst_params, 'scst' if path == 'scst' else 'caption')
        ar = f.arena
        ranges = (DataParallelStep(f) if path == 'single' else DataParallelBatchStep(inner))._range
        assert set(ranges) == {0, 1}
        (b,), kw = W.call_args(opt, 'scst' if path == 'scst' else 'caption', vids, dev)
        for rep in range(3):          # (the first call also builds workspaces; later calls run with every stream warm)
            snaps, ext = {}, {}

            def cb(which, stream_ptr):
                lo, hi = ranges[which]
                st = ext.setdefault(stream_ptr, torch.cuda.ExternalStream(stream_ptr, device=dev))
                with torch.cuda.stream(st):
                    snaps[which] = ar.flat_g[lo:hi].clone()
            if path == 'batch':
                f.batch_handover(b, cb)
            elif path == 'tap':
                g_tap = torch.zeros_like(b.tap)
                f._batch_tap(b, g_tap, b.dev('row_offset'), torch.zeros(b.n_videos, device=dev), step=False, handover=True, handover_cb=cb)
            elif path == 'scst':
                inner.handover(b, cb, **kw)
            else:
                v = vids[1]
                tap, c3d, lda = (torch.from_numpy(v[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
                labels = torch.from_numpy(v['labels'])
                f(tap, c3d, lda, labels, v['ind'], v['soi'], labels[:, 1:].numpy(), v['masks'][:, 1:], step=False, handover=True, handover_cb=cb)
            torch.cuda.synchronize()
            assert f.last_active_rows > 0          # some caption ends early: the late-fusion stage ran on the compacted rows
            assert set(snaps) == {0, 1}, snaps.keys()
            for which, (lo, hi) in ranges.items():
                final = ar.flat_g[lo:hi]
                assert float(final.abs().max()) > 0
                assert torch.equal(snaps[which], final), (rep, which, float((snaps[which] - final).abs().max()))
            if path == 'tap':
                assert float(g_tap.abs().max()) > 0
    finally:
        _set_config(None)


# ---- the two-rank runs ----------------------------------------------------------------------------------------------------------------------
def _run_ranks(tmp_path, sp, world=2, tag=''):
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = str(s.getsockname()[1]); s.close()
    outs = [str(tmp_path / ('%srank%d.npz' % (tag, r))) for r in range(world)]
    env = dict(os.environ, ECHR_DP_STAGED='0')
    for k in ('ECHR_DP_VIA', 'ECHR_DP_ALGO', 'ECHR_DP_WAIT_ALL'):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', 'dp_batch_worker.py'), str(r), str(world), port, outs[r], json.dumps(sp)],
                              cwd=ROOT, env=env) for r in range(world)]
    try:
        for p in procs:
            assert p.wait(timeout=WORKER_TIMEOUT) == 0          # (a non-zero exit fails the test: no retry)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [np.load(o) for o in outs]


@functools.lru_cache(maxsize=None)
def _reference(kind, clip, n_videos, world=2):
    """Step 0 in ONE process: per rank a fresh model on the rank's batch under the rank's pinned dropout state, step=False; the gradients
    (both models') and losses summed over the ranks.  Launch-per-phase or persistent makes no difference to these sums beyond the bound."""
    from echr_amd import parallel
    opt, params, sst_params = W.case(clip)
    vids = W.videos(opt, 0, n_videos)
    dev = _dev()
    total, loss, vloss = {}, 0.0, []
    for rank in range(world):
        shard = parallel.shard_batch(vids, rank, world)
        if not shard:
            continue
        model, optim, f, inner, tm = W.build(opt, params, sst_params, 'caption' if kind == 'single' else kind)
        W.pin_dropout(model, tm, 0, rank)
        if kind == 'single':
            v = shard[0]
            tap, c3d, lda = (torch.from_numpy(v[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
            labels = torch.from_numpy(v['labels'])
            l = f(tap, c3d, lda, labels, v['ind'], v['soi'], labels[:, 1:].numpy(), v['masks'][:, 1:], step=False)
        else:
            args, kw = W.call_args(opt, kind, shard, dev)
            if kind == 'caption':
                l, vl = f.batch(*args, step=False), None
                vl = f.last_video_losses
            elif kind == 'scst':
                l, vl = inner(*args, step=False, **kw)[0], None
                vl = inner.last_video_losses
            else:
                l = inner(*args, step=False)
                vl = W.LAMBDA1 * inner.last_tap_losses + W.LAMBDA2 * inner.last_video_losses
            vloss.append(vl.detach().cpu().numpy())
        torch.cuda.synchronize()
        loss += float(l)
        g = W.arena_grads(model, 'grad|')
        if tm is not None:
            g.update(W.arena_grads(tm, 'sstgrad|'))
        for k, x in g.items():
            total[k] = total[k] + x.astype(np.float64) if k in total else x.astype(np.float64)
    return total, loss, (np.concatenate(vloss) if vloss else None)


def _check(res, kind, clip, n_videos, staged, reduce_loss=False):
    r0, r1 = res
    assert int(r0['n_collectives']) == int(r1['n_collectives']) == (4 if staged else 1) + (1 if kind == 'joint' else 0) + (1 if reduce_loss else 0)
    if staged:
        assert int(r0['n_early']) == int(r1['n_early']) == 2          # both hand-over points were recorded and used (or queued by an empty rank)
    state = [k for k in r0.files if not k.startswith(('grad|', 'sstgrad|')) and k not in ('n_collectives', 'n_early', 'losses', 'vloss')]
    assert any(k.startswith('lm_model.') for k in state) and (kind != 'joint' or any(k.startswith('sst|') for k in state))
    for k in state:
        assert np.array_equal(r0[k], r1[k]), k                               # replicas stay bitwise identical after two steps
    total, loss, vloss = _reference(kind, clip, n_videos)
    assert any(k.startswith('grad|') for k in total)
    for k, ref in total.items():
        assert np.array_equal(r0[k], r1[k]), k
        name = k.split('|', 1)[1]
        print('%-56s %.3e' % (k, U.relerr(r0[k], ref, U.GRAD_FLOOR)))
        assert U.grad_close(name, r0[k], ref, TOL_GRAD), (k, U.relerr(r0[k], ref))          # SUM over ranks and videos, no 1/R, no 1/V
    return total, loss, vloss


@pytest.mark.parametrize('mode', ['lpp', 'coop', 'one'])
@pytest.mark.parametrize('clip', ['CC', 'CC+CH'])
def test_two_ranks_caption_step(tmp_path, clip, mode):
    """Each rank runs FusedTrainStep's batch form on two videos of different lengths, two optimiser steps: staged with the launch-per-phase
    recurrences, staged with cooperative persistent launches, and as one collective."""
    res = _run_ranks(tmp_path, W.spec('caption', clip, mode, n_videos=4))
    _check(res, 'caption', clip, 4, mode != 'one')


@pytest.mark.parametrize('n_videos,mode,via', [(3, 'lpp', 'callback'), (1, 'lpp', 'callback'), (1, 'coop', 'event')])
def test_uneven_and_empty_shards(tmp_path, n_videos, mode, via):
    """Three videos over two ranks (2 + 1) and one video over two ranks (rank 1 passes None): the same identities, the reduced gradients equal
    the single-process batches of the videos that exist, and with reduce_loss both ranks return the same loss -- the single-process sum --
    and the global per-video losses in rank-major shard order."""
    res = _run_ranks(tmp_path, W.spec('caption', 'CC', mode, n_videos=n_videos, reduce_loss=True, via=via))
    _, loss, vloss = _check(res, 'caption', 'CC', n_videos, True, reduce_loss=True)
    for r in res:
        print('loss %.7f reference %.7f' % (r['losses'][0], loss))
        assert abs(float(r['losses'][0]) - loss) < TOL_LOSS * abs(loss)
        assert r['vloss'].shape == (n_videos,) and np.abs(r['vloss'] - vloss).max() < TOL_LOSS * np.abs(vloss).max()
    assert np.array_equal(res[0]['losses'], res[1]['losses']) and np.array_equal(res[0]['vloss'], res[1]['vloss'])


def test_two_ranks_joint_step(tmp_path):
    """JointBatchStep inside (lambda1 = 0.01, lambda2 = 1): both models' replicas bitwise identical after two steps, the captioner's and the
    proposal encoder's reduced gradients equal to the sums over the two rank batches; five collectives (the proposal encoder's arena is one)."""
    res = _run_ranks(tmp_path, W.spec('joint', 'CC', 'lpp', n_videos=4))
    total, _, _ = _check(res, 'joint', 'CC', 4, True)
    assert any(k.startswith('sstgrad|') for k in total)


def test_two_ranks_self_critical_step(tmp_path):
    """SelfCriticalBatchStep inside with gen_result and reward passed explicitly (the decodes are out of the comparison)."""
    res = _run_ranks(tmp_path, W.spec('scst', 'CC', 'lpp', n_videos=4))
    _check(res, 'scst', 'CC', 4, True)


def test_two_ranks_single_video_step_with_clip_rows(tmp_path):
    """DataParallelStep around a FusedTrainStep built for 'CC+CH' (echr_train_step_clip): one video per rank, staged."""
    res = _run_ranks(tmp_path, W.spec('single', 'CC+CH', 'lpp', n_videos=2))
    _check(res, 'single', 'CC+CH', 2, True)


@pytest.mark.parametrize('mode,algo,via', [('coop', 'allreduce', 'callback'), ('coop', 'rs_ag', 'callback'), ('coop', 'rs_ag', 'event')])
def test_single_rank_rccl_batch_path(tmp_path, mode, algo, via):
    """test_single_rank_rccl_one_call_path for the batch form: ONE rank on RCCL (backend 'nccl') with cooperative persistent launches against
    the same worker over gloo, with that test's bounds -- a sum over one rank is the identity, so the first step's gradients agree to the
    run-to-run noise of the split-K atomics (1e-5 of the tensor's maximum) and the parameters after two Adam steps to 2 x 2 x lr.  This pins
    the nccl-only branches (asynchronous reduce-scatter + all-gather on the collective stream, the ONE wait, both hand-over forms) as far as
    one rank can; no RCCL run with more than one rank exists."""
    res = {}
    for backend in ('nccl', 'gloo'):
        res[backend] = _run_ranks(tmp_path, W.spec('caption', 'CC', mode, n_videos=2, via=via, algo=algo, backend=backend, reduce_loss=True),
                                  world=1, tag=backend)[0]
    a, b = res['nccl'], res['gloo']
    assert int(a['n_collectives']) == int(b['n_collectives']) == 5 and int(a['n_early']) == int(b['n_early']) == 2
    assert set(a.files) == set(b.files)
    assert np.abs(a['losses'][0] - b['losses'][0]) < TOL_LOSS * abs(b['losses'][0])
    for k in a.files:
        if k.startswith('grad|'):
            assert U.grad_close(k[5:], a[k], b[k], 1e-5), (k, U.relerr(a[k], b[k]))
        elif a[k].dtype.kind == 'f' and k not in ('losses', 'vloss'):
            assert np.abs(a[k] - b[k]).max() <= 4.1e-3, k          # (lr = 1e-3: Adam's first steps move a parameter by <= lr, whatever the gradient's size)
            if k not in U.NOISE_ONLY:                              # (a true gradient of exactly zero: the update is a coin flip of +-lr)
                assert np.mean(np.abs(a[k] - b[k]) > 1e-4) < 0.02, k   # ... and only elements whose gradient is at the noise floor differ at all


@pytest.mark.parametrize('stage', [(), ('--joint',), ('--self_critical',)])
def test_driver_under_a_two_rank_gloo_launch(stage):
    """examples/train_synthetic.py under `torchrun --nproc_per_node 2` on one GPU (gloo, launch-per-phase recurrences): --m_batch 3 (an
    uneven 2 + 1 shard) runs DataParallelBatchStep for the caption, joint and self-critical stages, and rank 0 reports a finite loss with the
    staged exchange (2 early collectives)."""
    import re
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--standalone', '--nproc_per_node', '2',
                        os.path.join(ROOT, 'examples', 'train_synthetic.py'), '--dist_backend', 'gloo', '--iters', '2', '--m_batch', '3',
                        '--events', '3', '--segments', '16', '--vocab', '300'] + list(stage),
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=WORKER_TIMEOUT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if 'DataParallelBatchStep(' in l]
    assert lines, r.stdout[-2000:]
    m = re.search(r'loss (-?[0-9.]+(?:e-?[0-9]+)?) .*?(\d+) collectives, (\d+) early', lines[-1])
    assert m and np.isfinite(float(m.group(1))) and int(m.group(3)) == 2, lines[-1]
    assert int(m.group(2)) == 4 + (1 if stage == ('--joint',) else 0) + 1          # + the reduced loss

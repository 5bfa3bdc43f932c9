"""Host side of the data-parallel batch step (no GPU): the shard helper, the shared collective sequencer (parallel.StagedExchange) over a
world-size-2 gloo group on CPU tensors, and the refusal that names the new class.  train.py:281-283,313-317: SUM over all videos of all
ranks, no 1/R and no 1/V."""
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from echr_amd import parallel

N_FLAT = 640          # the stub arena: ten 64-float slots (every range of it qualifies for reduce-scatter + all-gather over two ranks)
EARLY = ((448, 640), (128, 320))          # the two early ranges, in the order the stub step hands them over (the later range first)


@pytest.mark.parametrize('world', [1, 2, 3, 8])
@pytest.mark.parametrize('n_videos', [0, 1, 2, 3, 7, 16, 17])
def test_shard_batch_partitions_without_loss_or_overlap(n_videos, world):
    videos = [dict(name=i) for i in range(n_videos)]
    shards = [parallel.shard_batch(videos, r, world) for r in range(world)]
    got = [v['name'] for s in shards for v in s]
    assert sorted(got) == list(range(n_videos))                              # nothing lost, nothing twice
    for r, s in enumerate(shards):
        names = [v['name'] for v in s]
        assert names == sorted(names)                                        # order kept within a shard
        assert names == parallel.shard_videos(n_videos, r, world)            # the round-robin indices
        assert all(a is b for a, b in zip(s, (videos[i] for i in names)))    # the dicts themselves, not copies
    assert max(len(s) for s in shards) - min(len(s) for s in shards) <= 1
    assert got == parallel.shard_order(n_videos, world)                      # rank-major shard order
    assert parallel.shard_batch(iter(videos), 0, world) == shards[0]         # any iterable


def _video_grad(i):
    return np.random.RandomState(100 + i).standard_normal(N_FLAT).astype(np.float32)


def _stub_step(shard, flat, early):
    """A stand-in for the inner step: fills the flat CPU 'arena' with the sum of its shard's per-video gradients and hands the two early
    ranges over through `early(lo, hi)` once they are final; returns (loss, per-video losses).  An empty shard: zeros, the same hand-overs."""
    flat.zero_()
    for i in shard:
        flat += torch.from_numpy(_video_grad(i))
    for lo, hi in EARLY:
        early(lo, hi)
    losses = torch.tensor([1.0 + i for i in shard], dtype=torch.float32)
    return losses.sum().reshape(1), losses


def _worker(rank, world, port, q, algo, n_videos, staged):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    shard = parallel.shard_videos(n_videos, rank, world)
    ex = parallel.StagedExchange(None, algo)
    out = []
    for rep in range(2):          # (begin() resets the object: a second update counts from zero again)
        flat = torch.empty(N_FLAT)
        ex.begin()
        dist.barrier()
        t0 = time.time()
        loss, losses = _stub_step(shard, flat, (lambda lo, hi: ex.reduce_early(flat, lo, hi)) if staged else (lambda lo, hi: None))
        n_rest = ex.reduce_rest(flat)
        # reduce_loss: the loss and the per-video losses at their rank-major slots as ONE further collective
        n, lo = parallel.loss_slots(n_videos, rank, world, len(losses))          # the layout DataParallelBatchStep uses
        buf = torch.zeros(n)
        buf[0] = loss[0]
        buf[lo:lo + len(losses)] = losses
        ex.reduce_rest(buf)
        ex.wait()
        out = (rank, flat.numpy().copy(), buf.numpy().copy(), ex.n_collectives, ex.n_early, n_rest, [dict(r) for r in ex.ranges],
               [w.algo for w in ex.works], time.time() - t0)
    q.put(out)
    dist.destroy_process_group()


def _run(algo, n_videos, staged):
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = socket.socket()
    port.bind(('127.0.0.1', 0))
    pn = port.getsockname()[1]
    port.close()
    ps = [ctx.Process(target=_worker, args=(r, world, pn, q, algo, n_videos, staged)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize('algo', ['allreduce', 'rs_ag'])
def test_early_plus_remainder_equals_one_collective(algo):
    """Three videos over two ranks (2 + 1): the staged exchange (two early ranges, three remainder ranges) and the single collective leave
    the same buffer on both ranks -- the sum of the three videos' gradients, no 1/R, no 1/V."""
    staged, single = _run(algo, 3, True), _run(algo, 3, False)
    want = _video_grad(0) + _video_grad(1) + _video_grad(2)
    for r in range(2):
        _, flat, buf, n, n_early, n_rest, ranges, algos, _ = staged[r]
        assert (n, n_early, n_rest) == (5, 2, 2)          # two early, [0,128) and [320,448) (nothing is left behind 640), then the loss buffer
        assert [(x['lo'], x['hi'], x['early']) for x in ranges[:4]] == [(448, 640, True), (128, 320, True), (0, 128, False), (320, 448, False)]
        assert sum(x['bytes'] for x in ranges[:-1]) == 4 * N_FLAT
        assert algos[:4] == [algo] * 4          # every arena range is 64-float aligned: rs_ag runs as reduce-scatter + all-gather
        _, flat1, buf1, n1, n_early1, n_rest1, _, _, _ = single[r]
        assert (n1, n_early1, n_rest1) == (2, 0, 1)
        # three float32 addends, summed in two groupings (shard sums first, then ranks): each add rounds by at most 2^-24 relative, so
        # 1e-6 of the max-norm bounds the difference to the plain left-to-right sum
        assert np.abs(flat - want).max() <= 1e-6 * np.abs(want).max()
        assert np.abs(flat - flat1).max() <= 1e-6 * np.abs(want).max()
        assert np.array_equal(buf, buf1)
    assert np.array_equal(staged[0][1], staged[1][1])          # identical on both ranks


def test_exchange_counts_remainder_ranges(tmp_path):
    """The ranges the remainder consists of, over a one-rank gloo group in this process (a sum over one rank is the identity)."""
    dist.init_process_group('gloo', init_method='file://' + str(tmp_path / 'rdzv'), rank=0, world_size=1)
    try:
        flat = torch.arange(640, dtype=torch.float32)
        ex = parallel.StagedExchange()
        for lo, hi in EARLY:
            ex.reduce_early(flat, lo, hi)
        assert ex.reduce_rest(flat) == 2
        assert [(r['lo'], r['hi'], r['early']) for r in ex.ranges] == [(448, 640, True), (128, 320, True), (0, 128, False), (320, 448, False)]
        other = torch.ones(64)
        assert ex.reduce_rest(other) == 1 and (ex.n_collectives, ex.n_early) == (5, 2)          # a further buffer rides behind, whole
        ex.wait()
        assert torch.equal(flat, torch.arange(640, dtype=torch.float32)) and torch.equal(other, torch.ones(64))
        ex.begin()
        assert ex.reduce_rest(flat) == 1 and [(r['lo'], r['hi']) for r in ex.ranges] == [(0, 640)] and ex.n_early == 0
        ex.wait(in_order=True)
    finally:
        dist.destroy_process_group()


def test_loss_slots_layout_and_shard_length_check():
    """parallel.loss_slots: element 0 the loss, then the videos in rank-major shard order; a batch that is not the rank's shard is refused."""
    for n, world in ((3, 2), (1, 2), (7, 3), (16, 8)):
        slots = []
        for r in range(world):
            mine = len(parallel.shard_videos(n, r, world))
            size, lo = parallel.loss_slots(n, r, world, mine)
            assert size == 1 + n
            slots += list(range(lo, lo + mine))
            with pytest.raises(ValueError):
                parallel.loss_slots(n, r, world, mine + 1)
        assert slots == list(range(1, 1 + n))          # disjoint, complete, rank-major
    assert parallel.loss_slots(None, 1, 2, 5) == (1, 1)


@pytest.mark.parametrize('algo', ['allreduce', 'rs_ag'])
def test_empty_shard_rank_contributes_zeros_and_does_not_block(algo):
    """One video over two ranks: rank 1's shard is empty.  It queues the same collectives on a zero-filled buffer, both ranks end with rank
    0's gradient, and both return (the run would time out otherwise) within the same second."""
    res = _run(algo, 1, True)
    want = _video_grad(0)
    for r in range(2):
        assert np.array_equal(res[r][1], want)          # x + 0 is exact
        assert res[r][3] == res[0][3] == 5 and res[r][4] == 2
    assert abs(res[0][8] - res[1][8]) < 1.0


def test_reduce_loss_sums_and_orders_the_video_losses_rank_major():
    res = _run('allreduce', 3, True)
    for r in range(2):
        buf = res[r][2]
        assert buf[0] == (1.0 + 0) + (1.0 + 2) + (1.0 + 1)          # rank 0 ran videos 0 and 2, rank 1 video 1
        assert buf[1:].tolist() == [1.0 + i for i in parallel.shard_order(3, 2)] == [1.0, 3.0, 2.0]


def test_data_parallel_step_batch_names_the_batch_class():
    from echr_amd.fused import DataParallelBatchStep, DataParallelStep
    with pytest.raises(NotImplementedError, match='DataParallelBatchStep'):
        object.__new__(DataParallelStep).batch(None)
    with pytest.raises(TypeError):
        DataParallelBatchStep(object())

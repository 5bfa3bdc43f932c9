#!/usr/bin/env python3
"""Self-critical training over a multi-video batch against V sequential single-video iterations (GPU box only).  V = 1 / 4 / 16 videos of 4
events on 120 feature rows each, V1 = 5001, seq_length 20, a pinned per-caption reward.  Prints ONE JSON line (kept in
profiles/scst_batch_bench.json), per V:

  batch_iteration_ms   one SelfCriticalBatchStep call           sequential_ms   V SelfCriticalStep calls, one per video, same process
  sample_decode_ms / greedy_decode_ms / step_ms                 the batched iteration's phases, each timed alone
  sample_step_us: the sampled decode per decoder step with the one-launch multinomial step (echr_decoder_sample_train_batch) and with the
  slab-sum + draw pair (echr_decoder_sample_train on the same rows), alternated in the same process.  Not a gate.

Usage:  python tools/scst_batch_bench.py [--reps 20]"""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402

from echr_amd import _lib as L, synth                     # noqa: E402
from echr_amd import functional as EF                     # noqa: E402
from echr_amd.batch import VideoBatch                     # noqa: E402
from echr_amd.fused import FusedTrainStep, SelfCriticalBatchStep, SelfCriticalStep          # noqa: E402
from echr_amd.optim import ClampAdam                      # noqa: E402
from tests import util as U                               # noqa: E402

SEQ_LENGTH, V1, T_V, EVENTS = 20, 5001, 120, 4


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    try:
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    finally:
        gc.enable()
    return (time.perf_counter() - t0) / reps * 1e3


def bench_v(V, m, f, reps):
    opt = m.opt
    vids = synth.make_vbatch_videos(V, (EVENTS, EVENTS), (8, 60), (T_V, T_V), (SEQ_LENGTH + 2, SEQ_LENGTH + 2), V1, 2000 + V, max_events=EVENTS * V,
                                    video_dim=opt.video_dim, hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
    dev = torch.device('cuda')
    b = VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi')} for v in vids], device=dev)
    singles = [tuple(torch.from_numpy(v[k]).to(dev) for k in ('tap', 'c3d', 'lda')) + (v['ind'], v['soi']) for v in vids]
    N = b.n_events
    reward = np.random.RandomState(7).uniform(-1.0, 1.0, size=N).astype(np.float32)          # pinned, one value per caption
    scb, sc1 = SelfCriticalBatchStep(f), SelfCriticalStep(f)
    lm = m.lm_model

    def sequential():
        for (tap, c3d, lda, ind, soi), s in zip(singles, b.event_slices):
            sc1(tap, c3d, lda, ind, soi, reward=reward[s])
    t_seq = timed(sequential, reps)
    t_batch = timed(lambda: scb(b, reward=reward), reps)
    # the phases of the batched iteration, each alone on the contexts of one call
    with torch.no_grad():
        video, event, ev_start, ev_len, A, vid, drop = m._batch_contexts(b, None)
        video = EF._f32c(video)
        ps = lm.native_params()
        new = lambda: EF.sample_train_batch(video, event, b.c3d, ev_start, ev_len, vid, A, SEQ_LENGTH, ps, drop, seed=11)
        # the existing pair on the same rows: the single-video entry (one scene vector for all rows; the per-step work is the same)
        pair = lambda: EF.greedy_sample(video[0], event, b.c3d, ev_start, ev_len, A, SEQ_LENGTH, ps, multinomial=True, seed=11, drop=drop)
        t_new, t_pair = [], []
        for _ in range(3):          # alternated: other work shares the machine
            t_new.append(timed(new, reps))
            t_pair.append(timed(pair, reps))
        t_greedy = timed(lambda: EF.greedy_sample(video, event, b.c3d, ev_start, ev_len, A, SEQ_LENGTH, ps, table_cache=lm._sample_tables, vid=vid), reps)
    scb(b, reward=reward)
    st = L.stream_ptr()
    t_step = timed(lambda: L.check(f.lib.echr_train_step_batch(C.byref(f.a), C.byref(f.bx), None, L.ptr(scb.last_video_losses), st), 'train_step_batch'),
                   reps)
    return {'V': V, 'N': N, 'batch_iteration_ms': round(t_batch, 4), 'sequential_ms': round(t_seq, 4), 'speedup': round(t_seq / t_batch, 3),
            'sample_decode_ms': round(min(t_new), 4), 'greedy_decode_ms': round(t_greedy, 4), 'step_ms': round(t_step, 4),
            'sample_step_us': {'one_launch': [round(t / SEQ_LENGTH * 1e3, 2) for t in t_new],
                               'slab_sum_plus_draw': [round(t / SEQ_LENGTH * 1e3, 2) for t in t_pair]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=SEQ_LENGTH)
    m = U.build_gpu_model(opt, synth.make_params(opt, 0), True)
    o = ClampAdam(m.parameters(), lr=1e-6, arena=m.build_arena())
    f = FusedTrainStep(m, o, grad_clip=0.1)
    out = [bench_v(V, m, f, args.reps) for V in (1, 4, 16)]
    print(json.dumps({'shape': {'events_per_video': EVENTS, 'T_v': T_V, 'V1': V1, 'seq_length': SEQ_LENGTH}, 'reps': args.reps, 'cases': out}),
          flush=True)


if __name__ == '__main__':
    main()

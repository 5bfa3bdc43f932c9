#!/usr/bin/env python3
"""Self-critical training at the bench shapes (64 events x 128 segments, 20 decoder steps, V1 = 5001; GPU box only).  Prints ONE JSON line:
ms per sampled decode (training-mode multinomial chain, echr_decoder_sample_train), per greedy decode (persistent), per reward-weighted
step (echr_train_step_rw), per whole SelfCriticalStep iteration, and per plain echr_train_step on the same tokens.  Not a gate.

Usage:  python tools/scst_bench.py [--reps 20]"""
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
from echr_amd.fused import FusedTrainStep, SelfCriticalStep          # noqa: E402
from echr_amd.optim import ClampAdam                      # noqa: E402
from tests import util as U                               # noqa: E402


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


def reward_fn(gen, greedy):
    lb = (greedy > 0).sum(1).float() if greedy.numel() else torch.zeros(gen.shape[0])
    return ((gen > 0).sum(1).float() - lb) / 20.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    opt, params, vid = synth.make_case('c3bench')
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-6, arena=m.build_arena())
    f = FusedTrainStep(m, o, grad_clip=0.1)
    sc = SelfCriticalStep(f, reward_fn)
    tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
    ind, soi = vid['ind'], vid['soi']
    lm = m.lm_model
    with torch.no_grad():
        ev = EF.event_index_tensors(soi, ind, c3d.device, min(c3d.shape[0], tap.shape[0]))
        drop = lm.next_drop_state(m.encoder_dropout_p())
        drop.training = True
        video = m.get_video_context(tap, c3d, lda, ind, soi)
        clip, cm = m.get_clip_context(tap, c3d, lda, ind, soi, _ev=ev)
        event = m.get_event_context(tap, c3d, lda, ind, soi, _ev=ev, _drop=drop)
        t_sample = timed(lambda: lm.sample_train(video, event, clip, cm, drop), args.reps)
        lm.eval()
        t_greedy = timed(lambda: lm.sample(video, event, clip, cm), args.reps)
        lm.train()
    t_iter = timed(lambda: sc(tap, c3d, lda, ind, soi), args.reps)
    gen = sc(tap, c3d, lda, ind, soi)[1]
    lib, st = f.lib, L.stream_ptr()
    # the reward-weighted step alone: re-issue the last iteration's call (same inputs, same tokens)
    t_rw = timed(lambda: L.check(lib.echr_train_step_rw(C.byref(f.a), None, st), 'train_step_rw'), args.reps)
    # the plain step on the same tokens [0 | gen | 0] and the same mask
    N, T = gen.shape
    labels = np.zeros((N, T + 2), dtype=np.int64)
    labels[:, 1:T + 1] = gen.numpy()
    mask = np.zeros((N, T + 1), dtype=np.float32)
    mask[:, 0] = 1.0
    mask[:, 1:T] = labels[:, 1:T] > 0
    f(tap, c3d, lda, labels, ind, soi, labels[:, 1:], mask)
    t_plain = timed(lambda: L.check(lib.echr_train_step(C.byref(f.a), st), 'train_step'), args.reps)
    print(json.dumps({'shape': {'N': N, 'A': 128, 'steps': opt.CG_seq_length + 1, 'V1': opt.CG_vocab_size + 1, 'gen_T': T},
                      'reps': args.reps, 'sample_decode_ms': round(t_sample, 4), 'greedy_decode_ms': round(t_greedy, 4),
                      'rw_step_ms': round(t_rw, 4), 'scst_iteration_ms': round(t_iter, 4), 'plain_step_ms': round(t_plain, 4),
                      'active_rows': f.last_active_rows}), flush=True)


if __name__ == '__main__':
    main()

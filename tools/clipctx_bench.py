#!/usr/bin/env python3
"""Frame-level contexts 'CC' / 'CH' / 'CC+CH' at the bench shapes (GPU box only).  Prints ONE JSON line:
  * the one-call training iteration (FusedTrainStep with tap_grad: echr_train_step for 'CC', echr_train_step_clip otherwise) at the c3bench
    layout (64 disjoint 128-segment events, T_v = 8192, 20 decoder steps, V1 = 5001), timed as bench.py times it: `--warmup` iterations,
    a device sync, then `--steps` back-to-back iterations as one region divided by the step count;
  * the greedy caption pass, CaptionGenerator.forward(mode='eval') (event context + OldModel.sample), for 'CC' / 'CH' at 64 events (the c3bench
    layout) and at 1000 ragged proposals on a 256-segment video.
Not a gate.

Usage:  python tools/clipctx_bench.py [--steps 50 --warmup 10 --reps 10]"""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                              # noqa: E402

import echr_amd                                           # noqa: E402
from echr_amd import synth                                # noqa: E402
from echr_amd.fused import FusedTrainStep                 # noqa: E402
from echr_amd.optim import ClampAdam                      # noqa: E402
from tests import util as U                               # noqa: E402


def region(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    try:
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    finally:
        gc.enable()
    return (time.perf_counter() - t0) / steps * 1e3


def iteration_ms(ct, steps, warmup):
    opt, _, vid = synth.make_case('c3bench')
    opt.clip_context_type = ct
    params = synth.make_params(opt, 0)
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-6, arena=m.build_arena())
    f = FusedTrainStep(m, o, grad_clip=0.1)
    tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    g_tap = torch.zeros_like(tap)
    ms = region(lambda: f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], tap_grad=g_tap), steps, warmup)
    f.join()
    return ms


def decode_ms(ct, N, reps):
    dev = torch.device('cuda')
    opt = synth.default_opt(vocab_size=5000, seq_length=19, clip_context_type=ct)
    params = synth.make_params(opt, 0)
    m = echr_amd.CaptionGenerator(opt)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev).eval()
    vid = synth.make_video(N, 128, 21, 5001, seed=7, T_v=None if N <= 64 else 256, full_len=(N <= 64), disjoint=(N <= 64))
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    with torch.no_grad():
        return region(lambda: m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval'), reps, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--contexts', default='CC,CH,CC+CH', help='training iterations to time')
    ap.add_argument('--skip-decode', action='store_true', help='training iterations only (a profiler run)')
    args = ap.parse_args()
    res = {'layout': 'c3bench (N 64 x A 128 disjoint, T_v 8192, S 20, V1 5001)', 'steps': args.steps, 'warmup': args.warmup}
    for ct in args.contexts.split(','):
        res['iter_ms|' + ct] = round(iteration_ms(ct, args.steps, args.warmup), 4)
        torch.cuda.empty_cache()
    res['decode_reps'] = args.reps
    for N in (() if args.skip_decode else (64, 1000)):
        for ct in ('CC', 'CH'):
            res['greedy_ms|%s|N%d' % (ct, N)] = round(decode_ms(ct, N, args.reps), 4)
            torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()

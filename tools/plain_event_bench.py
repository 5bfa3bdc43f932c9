#!/usr/bin/env python3
"""Event contexts 'ER3' (through the TSRM event encoder) / 'EC' / 'EH' (the event vector itself: echr_train_step_args.event_direct) at the
bench shapes (GPU box only).  Prints ONE JSON line, also written to profiles/plain_event_bench.json:
  * the one-call training iteration (FusedTrainStep, no tap_grad) at the c3bench layout (64 disjoint 128-segment events, T_v = 8192, 20
    decoder steps, V1 = 5001): the three models live in ONE process and are timed ALTERNATED -- `--rounds` rounds, each timing `--steps`
    back-to-back iterations per context as one region divided by the step count; reported are every round's figure, the minimum and the
    spread (max - min) per context;
  * the greedy caption pass, CaptionGenerator.forward(mode='eval') (event context + OldModel.sample), per context at 64 events (the c3bench
    layout) and at 1000 ragged proposals on a 256-segment video.
Not a gate.

Usage:  python tools/plain_event_bench.py [--steps 20 --warmup 10 --rounds 3 --reps 10]"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                              # noqa: E402

import echr_amd                                           # noqa: E402
from echr_amd import synth                                # noqa: E402
from echr_amd.fused import FusedTrainStep                 # noqa: E402
from echr_amd.optim import ClampAdam                      # noqa: E402
from tests import util as U                               # noqa: E402

CONTEXTS = ('ER3', 'EC', 'EH')


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


def iteration_fn(et):
    opt, _, vid = synth.make_case('c3bench')
    opt.event_context_type = et
    params = synth.make_params(opt, 0)
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-6, arena=m.build_arena())
    f = FusedTrainStep(m, o, grad_clip=0.1)
    tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    return lambda: f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:])


def decode_ms(et, N, reps):
    dev = torch.device('cuda')
    opt = synth.default_opt(vocab_size=5000, seq_length=19, event_context_type=et)
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
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--skip-decode', action='store_true', help='training iterations only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'plain_event_bench.json'))
    args = ap.parse_args()
    res = {'layout': 'c3bench (N 64 x A 128 disjoint, T_v 8192, S 20, V1 5001)', 'steps': args.steps, 'warmup': args.warmup, 'rounds': args.rounds}
    fns = {et: iteration_fn(et) for et in CONTEXTS}
    for et in CONTEXTS:          # (every model warm before the first timed round)
        region(fns[et], 1, args.warmup)
    rounds = {et: [] for et in CONTEXTS}
    for _ in range(args.rounds):
        for et in CONTEXTS:
            rounds[et].append(region(fns[et], args.steps, 2))
    for et in CONTEXTS:
        res['iter_ms_rounds|' + et] = [round(x, 4) for x in rounds[et]]
        res['iter_ms|' + et] = round(min(rounds[et]), 4)
        res['iter_ms_spread|' + et] = round(max(rounds[et]) - min(rounds[et]), 4)
    del fns
    torch.cuda.empty_cache()
    res['decode_reps'] = args.reps
    for N in (() if args.skip_decode else (64, 1000)):
        for et in CONTEXTS:
            res['greedy_ms|%s|N%d' % (et, N)] = round(decode_ms(et, N, args.reps), 4)
            torch.cuda.empty_cache()
    line = json.dumps(res)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()

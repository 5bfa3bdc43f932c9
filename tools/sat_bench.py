#!/usr/bin/env python3
"""The one-stream decoder (caption_model='show_attend_tell', one LSTM layer: csrc/sat.hip) beside the three-stream decoder at the bench
shapes (GPU box only).  Prints ONE JSON line, also written to profiles/sat_bench.json:
  * the autograd training iteration -- CaptionGenerator.forward(mode='train'), LanguageModelCriterion, backward, clip_gradient, ClampAdam.step
    over the flat arena -- at the c3bench layout (64 disjoint 128-segment events, T_v = 8192, 20 decoder steps, V1 = 5001) for the
    one-stream models 'VEC' and 'C' and for the three-stream model on the SAME path with its persistent recurrences on and off.  The models
    live in ONE process and are timed ALTERNATED: `--rounds` rounds, each timing `--steps` back-to-back iterations per model as one region
    divided by the step count; reported are every round's figure, the minimum and the spread (max - min);
  * the greedy pass, CaptionGenerator.forward(mode='eval'), at 64 events (that layout) and at 1000 ragged proposals on a 256-segment video;
  * the two new kernels per launch, from device events around them (echr_prof_enable; forward-only pass, then forward + backward).
Not a gate.

Usage:  python tools/sat_bench.py [--steps 20 --warmup 10 --rounds 3 --reps 5]"""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                              # noqa: E402

import echr_amd                                           # noqa: E402
from echr_amd import _lib as L                            # noqa: E402
from echr_amd import synth                                # noqa: E402
from echr_amd.misc.utils import LanguageModelCriterion, clip_gradient          # noqa: E402
from echr_amd.optim import ClampAdam                      # noqa: E402
from tests import util as U                               # noqa: E402

MODELS = ('sat_VEC', 'sat_C', 'three_stream', 'three_stream_launch')


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


def model_opt(name, **over):
    opt = synth.default_opt(vocab_size=5000, seq_length=19, **over)
    if name.startswith('sat_'):
        opt.caption_model, opt.CG_num_layers, opt.CG_input_feats_type = 'show_attend_tell', 1, name[4:]
    return opt


def build(name, train):
    opt = model_opt(name)
    shapes = echr_amd.CaptionGenerator(model_opt(name)).state_dict()
    params = (synth.make_sat_params if name.startswith('sat_') else synth.make_params)(opt, 0)
    assert set(params) == set(shapes)
    return U.build_gpu_model(opt, params, train)


def persist(on):
    lib = L.load()
    lib.echr_config_set(b'persist', on)
    lib.echr_config_set(b'persist_bwd', on)


def iteration_fn(name):
    _, _, vid = synth.make_case('c3bench')
    m = build(name, True)
    o = ClampAdam(m.parameters(), lr=1e-6, arena=m.build_arena())
    crit = LanguageModelCriterion()
    tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
    labels = torch.from_numpy(vid['labels'])
    tgt, msk = labels[:, 1:].cuda(), torch.from_numpy(vid['masks'])[:, 1:].cuda()

    def fn():
        if name.startswith('three_stream'):
            persist(0 if name.endswith('_launch') else 1)
        try:
            o.zero_grad()
            loss = crit(m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train'), tgt, msk)
            loss.backward()
            clip_gradient(o, 0.1)
            o.step()
        finally:
            persist(1)
    return fn, m, (tap, c3d, lda, labels, vid)


def kernel_us(m, inputs):
    """(forward cell, reverse cell) microseconds per launch, from the library's device events around them (kind 4)."""
    lib = L.load()
    tap, c3d, lda, labels, vid = inputs

    def timed(backward):
        L.check(lib.echr_prof_enable(1), 'prof_enable')
        try:
            with torch.set_grad_enabled(backward):
                pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
                if backward:
                    pred.sum().backward()
            torch.cuda.synchronize()
            ms, fl, by, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
            L.check(lib.echr_prof_read(4, C.byref(ms), C.byref(fl), C.byref(by), C.byref(n)), 'prof_read')
        finally:
            L.check(lib.echr_prof_enable(0), 'prof_enable')
        return ms.value, n.value
    timed(True)
    f_ms, f_n = timed(False)
    b_ms, b_n = timed(True)
    m.zero_grad()
    return round(f_ms / f_n * 1e3, 2), round((b_ms - f_ms) / (b_n - f_n) * 1e3, 2)


def decode_ms(name, N, reps):
    m = build(name, False)
    vid = synth.make_video(N, 128, 21, 5001, seed=7, T_v=None if N <= 64 else 256, full_len=(N <= 64), disjoint=(N <= 64))
    tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
    with torch.no_grad():
        return region(lambda: m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval'), reps, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip-decode', action='store_true', help='training iterations only')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sat_bench.json'))
    args = ap.parse_args()
    res = {'layout': 'c3bench (N 64 x A 128 disjoint, T_v 8192, S 20, V1 5001)', 'step': 'autograd forward + backward + clamp + Adam',
           'steps': args.steps, 'warmup': args.warmup, 'rounds': args.rounds}
    built = {name: iteration_fn(name) for name in MODELS}
    for name in MODELS:          # (every model warm before the first timed round)
        region(built[name][0], 1, args.warmup)
    rounds = {name: [] for name in MODELS}
    for _ in range(args.rounds):
        for name in MODELS:
            rounds[name].append(region(built[name][0], args.steps, 2))
    for name in MODELS:
        res['iter_ms_rounds|' + name] = [round(x, 4) for x in rounds[name]]
        res['iter_ms|' + name] = round(min(rounds[name]), 4)
        res['iter_ms_spread|' + name] = round(max(rounds[name]) - min(rounds[name]), 4)
    for name in ('sat_VEC', 'sat_C'):
        res['cell_fwd_us|' + name], res['cell_bwd_us|' + name] = kernel_us(built[name][1], built[name][2])
    del built
    torch.cuda.empty_cache()
    res['decode_reps'] = args.reps
    for N in (() if args.skip_decode else (64, 1000)):
        for name in ('sat_VEC', 'sat_C', 'three_stream'):
            res['greedy_ms|%s|N%d' % (name, N)] = round(decode_ms(name, N, args.reps), 4)
            torch.cuda.empty_cache()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()

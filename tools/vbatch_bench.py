#!/usr/bin/env python3
"""Multi-video batches against sequential single-video calls, on the GPU (one JSON line; profiles/vbatch_bench.json).

For V in {1, 4, 16} videos of 4 events (8..40 segments, T_v = 120, 20 decoder steps, V1 = 5001, full-length captions -- the shape of caption
pre-training on ground-truth events, train.py:268-271):

  train  (a) V sequential FusedTrainStep calls (one clamp + Adam each: the unchanged path)   (b) ONE FusedTrainStep.batch call
  eval   (a) V sequential CaptionGenerator.forward(mode='eval') calls                        (b) ONE forward_batch(mode='eval') call

Each figure is a host clock around `reps` repetitions that end in a device synchronise, after a warm-up of every shape; (a) and (b) alternate
inside one process, `rounds` times, and the spread over the rounds is reported (min / median / max ms per repetition).  (a) and (b) are NOT
the same optimisation trajectory -- (a) takes V Adam steps, (b) one step on the summed gradient (the reference's m_batch = V) -- the
comparison is of the time to push V videos through the iteration.

Usage: python tools/vbatch_bench.py [--reps 30] [--rounds 5] [--out profiles/vbatch_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import echr_amd                                              # noqa: E402
from echr_amd import synth                                   # noqa: E402
from echr_amd.batch import VideoBatch                        # noqa: E402
from echr_amd.fused import FusedTrainStep                    # noqa: E402
from echr_amd.optim import ClampAdam                         # noqa: E402

EVENTS, SEG, T_V, L, V1 = 4, (8, 40), 120, 21, 5001          # L = 21 label columns: <bos> + 19 words + <eos> slot -> S = L - 1 = 20 decoder steps


def videos(V, seed=4000):
    """V videos of EVENTS events of SEG segments on T_V rows; every caption uses all its token slots (S = L - 1 = 20 steps, no masked rows)."""
    vids = synth.make_vbatch_videos(V, (EVENTS, EVENTS), SEG, (T_V, T_V), (L, L), V1, seed, max_events=EVENTS * V)
    rs = np.random.RandomState(seed + 7)
    for v in vids:
        n, w = v['labels'].shape
        v['labels'][:, 1:w - 1] = rs.randint(1, V1, size=(n, w - 2))
        v['masks'][:] = 1.0
    return vids


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def stats(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vbatch_bench needs the GPU: a timing taken anywhere else says nothing (no fallback)')
    dev = torch.device('cuda')
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=L - 2)
    params = synth.make_params(opt, 0)
    res = dict(tool='vbatch_bench', device=torch.cuda.get_device_name(0), events_per_video=EVENTS, steps=L - 1, V1=V1, reps=args.reps,
               rounds=args.rounds, cases=[])
    for V in (1, 4, 16):
        vids = videos(V)
        m = echr_amd.CaptionGenerator(opt)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        m = m.to(dev).train()
        o = ClampAdam(m.parameters(), lr=opt.lr, arena=m.build_arena())
        f = FusedTrainStep(m, o, grad_clip=opt.grad_clip)
        b = VideoBatch.from_videos(vids, device=dev)
        dv = [dict(tap=torch.from_numpy(v['tap']).to(dev), c3d=torch.from_numpy(v['c3d']).to(dev), lda=torch.from_numpy(v['lda']).to(dev),
                   labels=torch.from_numpy(v['labels']), tg=v['labels'][:, 1:], mk=v['masks'][:, 1:], ind=v['ind'], soi=v['soi']) for v in vids]

        def seq_train():
            for d in dv:
                f(d['tap'], d['c3d'], d['lda'], d['labels'], d['ind'], d['soi'], d['tg'], d['mk'])

        def bat_train():
            f.batch(b)

        def seq_eval():
            with torch.no_grad():
                for d in dv:
                    m(d['tap'], d['c3d'], d['lda'], [], d['ind'], d['soi'], mode='eval')

        def bat_eval():
            with torch.no_grad():
                m.forward_batch(b, mode='eval')

        case = dict(V=V, n_events=b.n_events, S=b.S)
        for name, fa, fb, train in (('train', seq_train, bat_train, True), ('eval', seq_eval, bat_eval, False)):
            m.train(train)
            for _ in range(args.warmup):
                fa()
                fb()
            ta, tb = [], []
            for _ in range(args.rounds):          # alternating, in one process
                ta.append(timed(fa, args.reps))
                tb.append(timed(fb, args.reps))
            sa, sb = stats(ta), stats(tb)
            case[name] = dict(sequential_ms=sa, batch_ms=sb,
                              sequential_ms_per_video=round(sa['median'] / V, 4), batch_ms_per_video=round(sb['median'] / V, 4),
                              sequential_events_per_s=round(1e3 * b.n_events / sa['median'], 1), batch_events_per_s=round(1e3 * b.n_events / sb['median'], 1),
                              speedup_median=round(sa['median'] / sb['median'], 3))
        echr_amd._lib.check(echr_amd._lib.load().echr_check_async(), 'vbatch_bench')
        res['cases'].append(case)
        del f, o, m
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""The non-zero initial decoder state (CG_init_feats_type = 'VEC') over a multi-video batch against sequential single-video calls with the
same option, on the GPU (one JSON line; profiles/init_batch_bench.json).

Shapes: tools/vbatch_bench.py's -- V in {1, 4, 16} videos of 4 events (8..40 segments, T_v = 120, 20 decoder steps, V1 = 5001, full-length
captions), clip context 'CC'.

  train   (a) V sequential FusedTrainStep calls (echr_train_step with w_init)      (b) ONE FusedTrainStep.batch call (echr_train_step_batch)
  greedy  (a) V sequential CaptionGenerator.forward(mode='eval') calls             (b) ONE forward_batch(mode='eval') call

Both sides take the launch-per-phase recurrences and the per-step sampler chain: the persistent kernels decline an initial state.  Each
figure is a host clock around `reps` repetitions that end in a device synchronise, after a warm-up of every shape; the two sides of a
comparison alternate inside one process, `rounds` times, and the spread over the rounds is reported (min / median / max ms per repetition).
(a) takes V Adam steps, (b) one step on the summed gradient (the reference's m_batch = V): the comparison is of the time to push V videos
through the iteration.

Usage: python tools/init_batch_bench.py [--reps 20] [--rounds 5] [--out profiles/init_batch_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import echr_amd                                              # noqa: E402
import vbatch_bench as VB                                    # noqa: E402  (videos, timed, stats: the same shapes and clock)
from clip_batch_bench import alternate                       # noqa: E402
from echr_amd import synth                                   # noqa: E402
from echr_amd.batch import VideoBatch                        # noqa: E402
from echr_amd.fused import FusedTrainStep                    # noqa: E402
from echr_amd.optim import ClampAdam                         # noqa: E402

INIT = 'VEC'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'init_batch_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('init_batch_bench needs the GPU: a timing taken anywhere else says nothing (no fallback)')
    dev = torch.device('cuda')
    lib = echr_amd._lib.load()
    res = dict(tool='init_batch_bench', device=torch.cuda.get_device_name(0), CG_init_feats_type=INIT, events_per_video=VB.EVENTS, steps=VB.L - 1,
               V1=VB.V1, reps=args.reps, rounds=args.rounds, cases=[])
    opt = synth.default_opt(vocab_size=VB.V1 - 1, seq_length=VB.L - 2, CG_init_feats_type=INIT)
    params = synth.make_params(opt, 0)
    for V in (1, 4, 16):
        vids = VB.videos(V)
        m = echr_amd.CaptionGenerator(opt)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        m = m.to(dev).train()
        o = ClampAdam(m.parameters(), lr=opt.lr, arena=m.build_arena())
        f = FusedTrainStep(m, o, grad_clip=opt.grad_clip)
        b = VideoBatch.from_videos(vids, device=dev, CG_init_feats_type=INIT)
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
        for name, fa, fb, train in (('train', seq_train, bat_train, True), ('greedy', seq_eval, bat_eval, False)):
            m.train(train)
            sa, sb = alternate(fa, fb, args)
            case[name] = dict(sequential_ms=sa, batch_ms=sb,
                              sequential_ms_per_video=round(sa['median'] / V, 4), batch_ms_per_video=round(sb['median'] / V, 4),
                              speedup_median=round(sa['median'] / sb['median'], 3))
        echr_amd._lib.check(lib.echr_check_async(), 'init_batch_bench')
        res['cases'].append(case)
        del f, o, m
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()

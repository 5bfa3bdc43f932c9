#!/usr/bin/env python3
"""The frame-level contexts 'CH' / 'CC+CH' over a multi-video batch against sequential single-video calls, on the GPU (one JSON line;
profiles/clip_batch_bench.json).

Shapes: tools/vbatch_bench.py's -- V in {1, 4, 16} videos of 4 events (8..40 segments, T_v = 120, 20 decoder steps, V1 = 5001, full-length
captions).  Per clip context:

  train   (a) V sequential FusedTrainStep calls (echr_train_step_clip)          (b) ONE FusedTrainStep.batch call (echr_train_step_batch_clip)
  greedy  (a) V sequential CaptionGenerator.forward(mode='eval') calls          (b) ONE forward_batch(mode='eval') call
  scatter the batch entry with d tap (the joint form, FusedTrainStep._batch_tap) on RAGGED captions -- the compacted path, where the
          clip-row gradient's context term meets dead rows -- with "row_grad_list" 1 (the list-form scatter) against 0 (fill + mark + the
          flag-form scatter); with full-length captions nothing is compacted and the two forms launch the same loop

Each figure is a host clock around `reps` repetitions that end in a device synchronise, after a warm-up of every shape; the two sides of a
comparison alternate inside one process, `rounds` times, and the spread over the rounds is reported (min / median / max ms per repetition).
(a) takes V Adam steps, (b) one step on the summed gradient (the reference's m_batch = V): the comparison is of the time to push V videos
through the iteration.

Usage: python tools/clip_batch_bench.py [--reps 30] [--rounds 5] [--out profiles/clip_batch_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import echr_amd                                              # noqa: E402
import vbatch_bench as VB                                    # noqa: E402  (videos, timed, stats: the same shapes and clock)
from echr_amd import synth                                   # noqa: E402
from echr_amd.batch import VideoBatch                        # noqa: E402
from echr_amd.fused import FusedTrainStep                    # noqa: E402
from echr_amd.optim import ClampAdam                         # noqa: E402


def ragged(vids, seed=11):
    """The same videos with captions of 1 .. 19 words (one full-length caption per video keeps S = 20): rows behind a caption's end are dead."""
    rs = np.random.RandomState(seed)
    out = []
    for v in vids:
        v = dict(v, labels=v['labels'].copy(), masks=v['masks'].copy())
        n, w = v['labels'].shape
        for i in range(1, n):
            ln = int(rs.randint(1, w - 1))
            v['labels'][i, 1 + ln:] = 0
            v['masks'][i, ln + 2:] = 0.0
        out.append(v)
    return out


def alternate(fa, fb, args):
    for _ in range(args.warmup):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(VB.timed(fa, args.reps))
        tb.append(VB.timed(fb, args.reps))
    return VB.stats(ta), VB.stats(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_batch_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('clip_batch_bench needs the GPU: a timing taken anywhere else says nothing (no fallback)')
    dev = torch.device('cuda')
    lib = echr_amd._lib.load()
    res = dict(tool='clip_batch_bench', device=torch.cuda.get_device_name(0), events_per_video=VB.EVENTS, steps=VB.L - 1, V1=VB.V1, reps=args.reps,
               rounds=args.rounds, cases=[])
    for ct in ('CH', 'CC+CH'):
        opt = synth.default_opt(vocab_size=VB.V1 - 1, seq_length=VB.L - 2, clip_context_type=ct)
        params = synth.make_params(opt, 0)
        for V in (1, 4, 16):
            vids = VB.videos(V)
            m = echr_amd.CaptionGenerator(opt)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
            m = m.to(dev).train()
            o = ClampAdam(m.parameters(), lr=opt.lr, arena=m.build_arena())
            f = FusedTrainStep(m, o, grad_clip=opt.grad_clip)
            b = VideoBatch.from_videos(vids, device=dev, clip_context_type=ct)
            br = VideoBatch.from_videos(ragged(vids), device=dev, clip_context_type=ct)
            dv = [dict(tap=torch.from_numpy(v['tap']).to(dev), c3d=torch.from_numpy(v['c3d']).to(dev), lda=torch.from_numpy(v['lda']).to(dev),
                       labels=torch.from_numpy(v['labels']), tg=v['labels'][:, 1:], mk=v['masks'][:, 1:], ind=v['ind'], soi=v['soi']) for v in vids]
            g_tap = torch.zeros_like(br.tap)
            per = torch.zeros(V, device=dev)
            ro_dev = br.dev('row_offset')

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

            def tap_form(on):
                def run():
                    lib.echr_config_set(b'row_grad_list', on)
                    g_tap.zero_()
                    f._batch_tap(br, g_tap, ro_dev, per)
                return run

            case = dict(clip_context_type=ct, V=V, n_events=b.n_events, S=b.S, D=opt.clip_context_dim)
            for name, fa, fb, train in (('train', seq_train, bat_train, True), ('greedy', seq_eval, bat_eval, False)):
                m.train(train)
                sa, sb = alternate(fa, fb, args)
                case[name] = dict(sequential_ms=sa, batch_ms=sb,
                                  sequential_ms_per_video=round(sa['median'] / V, 4), batch_ms_per_video=round(sb['median'] / V, 4),
                                  speedup_median=round(sa['median'] / sb['median'], 3))
            m.train(True)
            try:
                sl, sf = alternate(tap_form(1), tap_form(0), args)
            finally:
                lib.echr_config_set(b'row_grad_list', 1)
            case['scatter'] = dict(active_rows=f.last_active_rows, rows=br.n_events * br.S, list_ms=sl, flag_ms=sf,
                                   flag_over_list_median=round(sf['median'] / sl['median'], 4))
            echr_amd._lib.check(lib.echr_check_async(), 'clip_batch_bench')
            res['cases'].append(case)
            del f, o, m
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()

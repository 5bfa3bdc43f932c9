#!/usr/bin/env python3
"""The one-stream decoder (caption_model='show_attend_tell', 'VEC') over multi-video batches against V single-video calls (GPU box only).
Prints ONE JSON line, also written to profiles/sat_batch_bench.json.  Workload: videos of 4 events on T_v = 120 rows, 20 decoder steps,
V1 = 5001, the ECHR widths; V = 1 / 4 / 16 videos.

  * train: the autograd iteration -- forward_batch, batch.criterion, backward, clip_gradient, ClampAdam.step over the flat arena -- on ONE
    batch of V videos, against V sequential single-video iterations (forward, LanguageModelCriterion, backward, clip_gradient,
    ClampAdam.step each) on a second model with the same parameters;
  * greedy: forward_batch(mode='eval') against V forward(mode='eval') calls;
  * caption_videos over 16 videos at topN = 100 against 16 caption_video passes.

Both sides live in ONE process and are timed ALTERNATED: `--rounds` rounds, each timing `--steps` back-to-back repetitions per side as one
region divided by the step count; reported are every round's figure, the minimum and the spread (max - min), in ms per V videos.
The criterion's targets and masks are on the device on both sides, the label tensor the tokens are cut from on the host.  Not a gate.

Usage:  python tools/sat_batch_bench.py [--steps 20 --warmup 5 --rounds 3]"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402

import echr_amd                                           # noqa: E402
from echr_amd import eval_utils as EU                     # noqa: E402
from echr_amd import synth                                # noqa: E402
from echr_amd.batch import VideoBatch                     # noqa: E402
from echr_amd.misc.utils import LanguageModelCriterion, clip_gradient          # noqa: E402
from echr_amd.optim import ClampAdam                      # noqa: E402
from tests import util as U                               # noqa: E402

SAT = 'show_attend_tell'
EVENTS, ROWS, SEGMENTS, LABEL_WIDTH = 4, 120, 32, 21


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


def alternated(sides, steps, warmup, rounds):
    """{name: dict(rounds=[ms], min=, spread=)} of the callables `sides`, one region each per round, in turn."""
    out = {k: [] for k in sides}
    for r in range(rounds):
        for k, fn in sides.items():
            out[k].append(region(fn, steps, warmup if r == 0 else 1))
    return {k: dict(rounds=[round(x, 4) for x in v], min=round(min(v), 4), spread=round(max(v) - min(v), 4)) for k, v in out.items()}


def make_opt():
    return synth.default_opt(vocab_size=5000, seq_length=19, caption_model=SAT, CG_num_layers=1, CG_input_feats_type='VEC')


def make_videos(opt, V, seed=4000):
    return [synth.make_video(EVENTS, SEGMENTS, LABEL_WIDTH, opt.CG_vocab_size + 1, seed=seed + v, T_v=ROWS, video_dim=opt.video_dim,
                             hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim) for v in range(V)]


def train_sides(opt, params, videos):
    dev = torch.device('cuda')
    crit = LanguageModelCriterion()
    mb, ms = U.build_gpu_model(opt, params, True), U.build_gpu_model(opt, params, True)
    ob = ClampAdam(mb.parameters(), lr=1e-6, arena=mb.build_arena())
    os_ = ClampAdam(ms.parameters(), lr=1e-6, arena=ms.build_arena())
    batch = VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi', 'labels', 'masks')} for v in videos], device=dev,
                                   caption_model=SAT)
    tg_all, mk_all = batch.targets.to(dev), batch.crit_masks.to(dev)          # (batch.criterion's tensors, uploaded once as the other side's are)
    single = []
    for v in videos:
        labels = torch.from_numpy(v['labels'])
        single.append((torch.from_numpy(v['tap']).to(dev), torch.from_numpy(v['c3d']).to(dev), torch.from_numpy(v['lda']).to(dev), labels,
                       v['ind'], v['soi'], labels[:, 1:].to(dev), torch.from_numpy(v['masks'])[:, 1:].to(dev)))

    def batched():
        ob.zero_grad()
        logp = mb.forward_batch(batch, mode='train')
        loss = torch.stack([crit(logp[s], tg_all[s], mk_all[s]) for s in batch.event_slices]).sum()          # batch.criterion on device tensors
        loss.backward()
        clip_gradient(ob, opt.grad_clip)
        ob.step()

    def sequential():
        for tap, c3d, lda, labels, ind, soi, tgt, msk in single:
            os_.zero_grad()
            loss = crit(ms(tap, c3d, lda, labels, ind, soi, mode='train'), tgt, msk)
            loss.backward()
            clip_gradient(os_, opt.grad_clip)
            os_.step()
    return dict(batch=batched, sequential=sequential)


def greedy_sides(opt, params, videos):
    dev = torch.device('cuda')
    m = U.build_gpu_model(opt, params, False)
    batch = VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi')} for v in videos], device=dev, caption_model=SAT)
    single = [(torch.from_numpy(v['tap']).to(dev), torch.from_numpy(v['c3d']).to(dev), torch.from_numpy(v['lda']).to(dev), v['ind'], v['soi'])
              for v in videos]

    def batched():
        with torch.no_grad():
            m.forward_batch(batch, mode='eval')

    def sequential():
        with torch.no_grad():
            for tap, c3d, lda, ind, soi in single:
                m(tap, c3d, lda, [], ind, soi, mode='eval')
    return dict(batch=batched, sequential=sequential)


def caption_sides(opt, params, videos, topN=100):
    dev = torch.device('cuda')
    torch.manual_seed(3)
    tap = echr_amd.models.setup_tap(opt).to(dev)
    tap.eval()
    m = U.build_gpu_model(opt, params, False)
    f2t = lambda s, e, n, d: [round(float(s) / n * d, 3), round(float(e) / n * d, 3)]
    vids = [dict(c3d=torch.from_numpy(v['c3d']).to(dev), lda=torch.from_numpy(v['lda']).to(dev), duration=60.0) for v in videos]
    counts = [len(i) for i in EU.caption_videos(tap, m, vids, f2t, topN=topN)[0]]

    def batched():
        EU.caption_videos(tap, m, vids, f2t, topN=topN)

    def sequential():
        for v in vids:
            EU.caption_video(tap, m, v['c3d'], v['lda'], 60.0, f2t, topN=topN)
    return dict(batch=batched, sequential=sequential), counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--videos', type=int, nargs='+', default=[1, 4, 16])
    a = ap.parse_args()
    opt = make_opt()
    params = synth.make_sat_params(opt, 0)
    out = dict(workload=dict(events_per_video=EVENTS, rows_per_video=ROWS, steps=LABEL_WIDTH - 1, V1=opt.CG_vocab_size + 1, feats='VEC',
                             timed='min of %d rounds of %d, alternated; ms per V videos' % (a.rounds, a.steps)), train={}, greedy={})
    for V in a.videos:
        videos = make_videos(opt, V)
        out['train'][str(V)] = alternated(train_sides(opt, params, videos), a.steps, a.warmup, a.rounds)
        out['greedy'][str(V)] = alternated(greedy_sides(opt, params, videos), a.steps, a.warmup, a.rounds)
        for part in ('train', 'greedy'):
            r = out[part][str(V)]
            r['sequential_over_batch'] = round(r['sequential']['min'] / r['batch']['min'], 3)
        gc.collect()
        torch.cuda.empty_cache()
    sides, counts = caption_sides(opt, params, make_videos(opt, 16))
    out['caption_videos_16x100'] = alternated(sides, max(1, a.steps // 4), 2, a.rounds)
    out['caption_videos_16x100']['events'] = int(np.sum(counts))
    r = out['caption_videos_16x100']
    r['sequential_over_batch'] = round(r['sequential']['min'] / r['batch']['min'], 3)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'sat_batch_bench.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""The joint 'tap_cg' iteration over a batch (fused.JointBatchStep) against V sequential single-video calls (fused.JointTrainStep), in one process.

V = 1 / 4 / 16 videos of 4 events and T_v = 120 rows, and one mixed batch of eight videos of 32..256 rows; S = 20 decoder steps, a vocabulary
of 5001 words, K = 256 anchors, D = 500, H = 512, training mode.  Both forms share the models and optimisers (lr = 1e-9: the parameters stay
put); the sequential form is V calls with an update each, the batched form ONE call with one update per model.  The two alternate: five
pairs of timed regions of `--iters` iterations each (device events around a region, the device synchronised between regions, one warm-up
region of each form first); a figure is the median of its five regions, `spread` their (max - min) / median.  Prints ONE JSON line; --out
writes it to a file as well.

usage: python tools/joint_batch_bench.py [--iters 10] [--out profiles/joint_batch_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import echr_amd
from echr_amd import _lib, models, synth
from echr_amd.fused import FusedTrainStep, JointBatchStep, JointTrainStep
from echr_amd.optim import ClampAdam

N_EVENTS, L, V1, K = 4, 21, 5001, 256
KEYS = ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')


def make_videos(opt, lengths, seed):
    rs = np.random.RandomState(seed)
    vids = []
    for i, T in enumerate(lengths):
        v = synth.make_video(N_EVENTS, min(T, 60), L, V1, seed=seed + i, T_v=T, video_dim=opt.video_dim, hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
        v['tap_labels'] = (rs.uniform(size=(T, K)) > 0.9).astype(np.float32)
        v['tap_masks'] = (np.arange(T)[:, None] >= np.arange(K)[None, :]).astype(np.float32)
        v['w1'] = rs.uniform(0.05, 0.3, size=(K,)).astype(np.float32)
        vids.append(v)
    return vids


def region(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def summary(ms):
    med = float(np.median(ms))
    return dict(ms=round(med, 4), spread=round((max(ms) - min(ms)) / med, 4))


def bench_case(opt, seq, bat, lengths, iters, seed, regions=5):
    dev = torch.device('cuda')
    vids = make_videos(opt, lengths, seed)
    on = lambda x: torch.from_numpy(x).to(dev)
    single = [(on(v['c3d']), on(v['lda']), torch.from_numpy(v['labels']), v['ind'], v['soi'], torch.from_numpy(v['labels'])[:, 1:],
               torch.from_numpy(v['masks'])[:, 1:], on(v['tap_masks']), on(v['tap_labels']), on(v['w1'])) for v in vids]
    videos = [dict({k: v[k] for k in KEYS}, c3d=on(v['c3d']), lda=on(v['lda'])) for v in vids]
    mk, lb = torch.cat([s[7] for s in single], 0), torch.cat([s[8] for s in single], 0)
    w1 = torch.stack([s[9] for s in single], 0)

    def run_seq():
        for s in single:
            seq(*s)
        seq.fused.join()

    def run_bat():
        bat(videos, mk, lb, w1)
    region(run_seq, 2)
    region(run_bat, 2)
    ms_seq, ms_bat = [], []
    for _ in range(regions):
        ms_seq.append(region(run_seq, iters))
        ms_bat.append(region(run_bat, iters))
    r = dict(videos=len(lengths), rows=int(sum(lengths)), events=N_EVENTS * len(lengths), sequential=summary(ms_seq), batched=summary(ms_bat))
    r['speedup'] = round(r['sequential']['ms'] / r['batched']['ms'], 3)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args(argv)
    lib = _lib.load()
    torch.manual_seed(0)
    dev = torch.device('cuda')
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=L - 2, K=K)
    cg = echr_amd.CaptionGenerator(opt).to(dev)
    cg.train()
    tap = models.setup_tap(opt).to(dev)
    tap.train()
    cg_opt = ClampAdam(cg.parameters(), lr=1e-9, arena=cg.build_arena())
    tap_opt = ClampAdam(tap.parameters(), lr=1e-9, arena=tap.build_arena())
    fused = FusedTrainStep(cg, cg_opt, grad_clip=opt.grad_clip)
    seq = JointTrainStep(fused, tap, tap_opt, lambda1=0.01, tap_grad_clip=opt.grad_clip)
    bat = JointBatchStep(fused, tap, tap_opt, lambda1=0.01, lambda2=1.0, tap_grad_clip=opt.grad_clip)
    cases = [('V1', [120]), ('V4', [120] * 4), ('V16', [120] * 16), ('mixed8', [32, 64, 96, 128, 160, 192, 224, 256])]
    res = dict(tool='joint_batch_bench', events_per_video=N_EVENTS, S=L - 1, vocab=V1, K=K, T_v=120, iters=a.iters, device=torch.cuda.get_device_name(0))
    for i, (name, lengths) in enumerate(cases):
        res[name] = bench_case(opt, seq, bat, lengths, a.iters, 100 * (i + 1))
    res['check_async'] = int(lib.echr_check_async())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""What building a batch's proposal targets costs on the device against a vectorised host builder (GPU box only).  V = 1 / 4 / 16 videos of
T_v = 256 rows at K = 256 with 4 ground-truth segments each, prop_sample_num = 64.  Two forms on the same inputs, alternated in one process,
the minimum of the rounds reported (each round: the mean of --reps calls, wall time, synchronised):

  device_ms       echr_amd.targets.build: the upload of offsets and segments, echr_tap_targets_batch, echr_prop_events_batch and the one
                  host read of n_good / n_events / the event lists; the [T_tot, K] matrices stay on the device
  host_numpy_ms   tests/targets_ref.video_targets per video (float64, broadcast over (t, k), a loop over the segments), a
                  numpy-permutation sample of the good proposals, and the upload of the concatenated tap_masks and tap_labels -- the two
                  matrices the training step reads.  A vectorised baseline, not the reference's loop.

loop_v1_ms is the per-cell Python loop (the form the reference's get_vid_data has) on ONE video, timed once, for the record.
With --driver, driver_ms gives the iteration time of examples/train_synthetic.py --joint --m_batch 16 with and without --gt_targets:
(wall time of --iters 44 minus --iters 4) / 40 each after one untimed warm-up run, the minimum of the rounds.  The two loaders differ (ready-made
lists of 16 events per video against 16 events sampled from 4 segments), so the pair shows what the stage costs in place, not a ratio.

Prints ONE JSON line and writes it to --out (kept in profiles/targets_bench.json).

Usage:  python tools/targets_bench.py [--rounds 3] [--reps 10] [--driver] [--out profiles/targets_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402

from echr_amd import targets as TG                        # noqa: E402
from tests import targets_ref as R                        # noqa: E402

T_V, K, SEGMENTS, CAP, BATCHES = 256, 256, 4, 64, (1, 4, 16)


def make_videos(V, seed=0):
    rs = np.random.RandomState(seed)
    vids = []
    for _ in range(V):
        st = []
        for _ in range(SEGMENTS):
            n = int(rs.randint(8, 200))
            s = int(rs.randint(0, T_V - n))
            st.append((s, s + n))
        vids.append((T_V, st))
    return vids


def host_build(videos, dev, rs):
    masks, labels, events = [], [], []
    for T, st in videos:
        o = R.video_targets(T, K, st)
        ev = R.all_events(o['good_gt'])
        events.append(ev[rs.permutation(len(ev))[:CAP]])
        masks.append(o['tap_masks'])
        labels.append(o['tap_labels'])
    up = torch.from_numpy(np.stack([np.concatenate(masks, 0), np.concatenate(labels, 0)])).to(dev)
    return up, events


def loop_build(T, stamps):
    """The per-cell form: a Python loop over (t, k) and the segments."""
    iou = np.zeros((T, K), np.float32)
    idx = np.zeros((T, K), np.float32)
    for t in range(T):
        for k in range(K):
            if t >= k + 1:
                a, best, bi = t - k - 1, 0.0, -1
                for i, (start, end) in enumerate(stamps):
                    s, e = start - 0.01, end + 0.01
                    inter = max(0, min(e, t) - max(s, a))
                    union = min(max(e, t) - min(s, a), e - s + t - a)
                    ov = float(inter) / (union + 1e-8)
                    if ov >= best:
                        best, bi = ov, i
                iou[t, k], idx[t, k] = best, bi
    return iou, idx


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def driver_iteration_ms(extra):
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import train_synthetic as TS
    base = ['--joint', '--m_batch', '16', '--quiet'] + extra
    t = {}
    for iters in (4, 44):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        TS.main(base + ['--iters', str(iters)])
        torch.cuda.synchronize()
        t[iters] = time.perf_counter() - t0
    return (t[44] - t[4]) / 40 * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--driver', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'targets_bench.json'))
    args = ap.parse_args()
    dev = torch.device('cuda')
    rs = np.random.RandomState(1)
    shapes = {}
    for V in BATCHES:
        videos = make_videos(V)
        t = {'device_ms': [], 'host_numpy_ms': []}
        for _ in range(args.rounds):          # alternated: other work shares the machine
            t['device_ms'].append(wall(lambda: TG.build(videos, K, prop_sample_num=CAP, seed=7, device=dev), args.reps))
            t['host_numpy_ms'].append(wall(lambda: host_build(videos, dev, rs), max(1, args.reps // 5)))
        got = TG.build(videos, K, prop_sample_num=CAP, seed=7, device=dev)
        up, _ = host_build(videos, dev, rs)
        mn = {k: min(v) for k, v in t.items()}
        shapes['V%d' % V] = {'device_ms': round(mn['device_ms'], 4), 'host_numpy_ms': round(mn['host_numpy_ms'], 3),
                             'host_over_device': round(mn['host_numpy_ms'] / mn['device_ms'], 1),
                             'rounds_ms': {k: [round(x, 4) for x in v] for k, v in t.items()}, 'n_good': got.n_good.tolist(),
                             'matrices_equal': bool(torch.equal(up[0], got.tap_masks) and torch.equal(up[1], got.tap_labels))}
    T, st = make_videos(1)[0]
    t0 = time.perf_counter()
    iou, _ = loop_build(T, st)
    loop_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(iou, R.video_targets(T, K, st)['iou'])
    out = {'tool': 'targets_bench', 'device': torch.cuda.get_device_name(0),
           'shape': {'T_v': T_V, 'K': K, 'segments': SEGMENTS, 'prop_sample_num': CAP, 'videos': list(BATCHES)},
           'rounds': args.rounds, 'reps': args.reps, 'host_form': 'vectorised numpy (tests/targets_ref.py) + upload of tap_masks and tap_labels',
           'batches': shapes, 'loop_v1_ms': round(loop_ms, 1)}
    if args.driver:
        d = {'default': [], 'gt_targets': []}
        driver_iteration_ms([])          # untimed: the process's first iterations carry one-time set-up
        driver_iteration_ms(['--gt_targets'])
        for _ in range(args.rounds):
            d['default'].append(driver_iteration_ms([]))
            d['gt_targets'].append(driver_iteration_ms(['--gt_targets']))
        out['driver_ms'] = {k: round(min(v), 3) for k, v in d.items()}
        out['driver_rounds_ms'] = {k: [round(x, 3) for x in v] for k, v in d.items()}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

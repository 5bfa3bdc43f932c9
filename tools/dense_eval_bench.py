#!/usr/bin/env python3
"""What dense-caption scoring costs on the device against the pure-Python oracle of the tests (GPU box only).  16 synthetic videos x 1000
proposals, 4-8 ground truths each, seq_length 20, V1 = 5001, thresholds 0.3 / 0.5 / 0.7 / 0.9; three quarters of the proposals are
jittered copies of a ground truth, captions are random words or a reference with one word replaced.  Two forms on the same inputs,
alternated, the minimum of the rounds reported:

  device_ms        echr_amd.densecap.evaluate without a CIDEr-D scorer, inputs on the device, the result read to the host (wall time);
                   device_events_ms is the same call between two device events
  host_python_ms   tests/densecap_ref.evaluate without CIDEr-D -- what a user does today with a pure-Python scorer; NOT a tuned host baseline

device_ciderd_ms is the device form with the CIDEr-D column (echr_ciderd_score over every pair); the oracle is not run with it.
max_rel_diff is the largest relative difference of the Bleu_n / ROUGE_L means between the two forms, and detection_equal whether Recall
and Precision agree bit for bit.  Prints ONE JSON line and writes it to --out (kept in profiles/dense_eval_bench.json).

Usage:  python tools/dense_eval_bench.py [--rounds 3] [--reps 5] [--out profiles/dense_eval_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402

from echr_amd import densecap as D                        # noqa: E402
from echr_amd.reward import CiderD                        # noqa: E402
from tests import densecap_ref as R                       # noqa: E402

SEQ_LENGTH, V1, VIDEOS, PROPOSALS, TIOUS = 20, 5001, 16, 1000, (0.3, 0.5, 0.7, 0.9)


def make_inputs(seed=0):
    rs = np.random.RandomState(seed)
    vids, pst, caps = [], [], []
    for _ in range(VIDEOS):
        G = rs.randint(4, 9)
        start = np.sort(rs.uniform(0.0, 90.0, G))
        ts = np.stack([start, start + rs.uniform(5.0, 40.0, G)], 1)
        sents = [rs.randint(1, V1, size=rs.randint(6, SEQ_LENGTH + 1)).tolist() for _ in range(G)]
        vids.append(dict(timestamps=ts, sentences=sents))
        for i in range(PROPOSALS):
            g = rs.randint(G)
            if i % 4 == 0:
                s = rs.uniform(0.0, 100.0)
                pst.append([s, s + rs.uniform(1.0, 40.0)])
                row = rs.randint(1, V1, size=rs.randint(0, SEQ_LENGTH + 1)).tolist()
            else:
                w = (1.0, 4.0, 12.0)[i % 4 - 1]
                pst.append([ts[g, 0] + rs.uniform(-w, w), ts[g, 1] + rs.uniform(-w, w)])
                row = list(sents[g])
                row[rs.randint(len(row))] = int(rs.randint(1, V1))
            caps.append((row + [0] * SEQ_LENGTH)[:SEQ_LENGTH])
    gt = D.pack_ground_truth(vids, SEQ_LENGTH, V1 - 1)
    sc = CiderD.from_corpus([[s] for v in vids for s in v['sentences']], SEQ_LENGTH, V1 - 1)
    p_off = np.arange(VIDEOS + 1, dtype=np.int32) * PROPOSALS
    return gt, sc, np.asarray(pst, np.float64), np.asarray(caps, np.int64), p_off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dense_eval_bench.json'))
    args = ap.parse_args()
    gt, sc, pst, caps, p_off = make_inputs()
    gt_d, pst_d, caps_d = gt.cuda(), torch.from_numpy(pst).cuda(), torch.from_numpy(caps).cuda()
    sc.cuda()
    refs_h, gst_h, g_off = gt.refs.numpy(), gt.stamps.numpy(), gt.offset.numpy()

    def device(scorer=None):
        res = D.evaluate(pst_d, p_off, caps_d, gt_d, TIOUS, scorer=scorer)
        res.as_dict()                                      # the result on the host
        return res

    def wall(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    def events(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for _ in range(reps):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return min(out)

    t = {'device_ms': [], 'device_events_ms': [], 'device_ciderd_ms': [], 'host_python_ms': []}
    for _ in range(args.rounds):          # alternated: other work shares the machine
        t['device_ms'].append(wall(device, args.reps))
        t['device_events_ms'].append(events(device, args.reps))
        t['device_ciderd_ms'].append(wall(lambda: device(sc), args.reps))
        t0 = time.perf_counter()
        o = R.evaluate(pst, p_off, caps, gst_h, g_off, refs_h, TIOUS)
        t['host_python_ms'].append((time.perf_counter() - t0) * 1e3)
    res = device()
    rel = 0.0
    for name in ('Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L'):
        got, want = getattr(res, name), np.asarray(o[name])
        rel = max(rel, float((np.abs(got - want) / np.abs(want)).max()))
    mn = {k: min(v) for k, v in t.items()}
    out = {'tool': 'dense_eval_bench', 'device': torch.cuda.get_device_name(0),
           'shape': {'videos': VIDEOS, 'proposals_per_video': PROPOSALS, 'ground_truths': int(g_off[-1]), 'seq_length': SEQ_LENGTH, 'V1': V1, 'tious': TIOUS},
           'pairs_per_tiou': np.asarray(o['n_pairs']).sum(1).tolist(), 'unmatched_per_tiou': np.asarray(o['n_unmatched']).sum(1).tolist(),
           'rounds': args.rounds, 'reps': args.reps, 'host_form': 'pure-Python scorer (tests/densecap_ref.py), not a tuned host baseline',
           'device_ms': round(mn['device_ms'], 4), 'device_events_ms': round(mn['device_events_ms'], 4),
           'device_ciderd_ms': round(mn['device_ciderd_ms'], 4), 'host_python_ms': round(mn['host_python_ms'], 1),
           'host_over_device': round(mn['host_python_ms'] / mn['device_ms'], 1),
           'rounds_ms': {k: [round(x, 4) for x in v] for k, v in t.items()},
           'scores': {k: [round(float(x), 6) for x in getattr(res, k)] for k in ('Recall', 'Precision', 'Bleu_4', 'ROUGE_L')},
           'max_rel_diff': rel, 'detection_equal': bool(np.array_equal(res.Recall, np.asarray(o['Recall'])) and np.array_equal(res.Precision, np.asarray(o['Precision'])))}
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

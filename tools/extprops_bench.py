#!/usr/bin/env python3
"""What selecting external proposals (flag_eval_what = 'SOTA_TEP') costs on the device against the host path (GPU box only).  V = 1 / 4 / 16
videos of P = 1000 proposals each (T_v = 256 rows, K = 256), at nms_threshold 0 and 0.8, topN = 1000.  Two forms on the same inputs,
alternated in one process, the minimum of the rounds reported (each round: the mean of the reps, wall time, synchronised):

  device_ms   echr_amd.extprops.select: the host checks, the packed upload, echr_nms_segments_batch (at 0.8), echr_ext_proposals_batch and
              the one host read
  host_ms     tests/extprops_ref.select per video: eval_utils.gettopN_nms (one numpy pass per pick), the filter loop, targets.featstamps
              (a Python loop per segment) and the crop -- what the host half did before

caption_ms gives what the selection adds in place: eval_utils.caption_videos over V = 16 videos with flag_eval_what='SOTA_TEP' (topN = 100,
nms_threshold 0.8) against the same pass fed the selected events as 'cg', alternated the same way.

Prints ONE JSON line and writes it to --out (kept in profiles/extprops_bench.json).

Usage:  python tools/extprops_bench.py [--rounds 3] [--reps 10] [--no-caption] [--out profiles/extprops_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402

from echr_amd import extprops as XP                       # noqa: E402
from tests import extprops_ref as R                       # noqa: E402

T_V, K, P, TOPN, DURATION, BATCHES, THRESHOLDS = 256, 256, 1000, 1000, 120.0, (1, 4, 16), (0.0, 0.8)
CAPTION_V, CAPTION_TOPN, CAPTION_NMS, V1, SEQ = 16, 100, 0.8, 5001, 20


def make_videos(V, seed=0):
    rs = np.random.RandomState(seed)
    vids = []
    for _ in range(V):
        start = rs.uniform(0.0, DURATION * 0.9, size=P)
        st = np.stack([start, start + rs.uniform(0.5, DURATION * 0.5, size=P)], 1)
        vids.append(dict(SOTA_timestamps=st, SOTA_Prop_score=(rs.permutation(P) + 1.0) / P, duration=DURATION, nfeats=T_V))
    return vids


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def caption_pair(args, dev):
    import echr_amd
    from echr_amd import eval_utils as EU, models, synth
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=SEQ)
    params = synth.make_params(opt, 0)
    cg = echr_amd.CaptionGenerator(opt)
    cg.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    cg = cg.to(dev).eval()
    torch.manual_seed(5)
    tap = models.setup_tap(opt).to(dev)
    tap.eval()
    f2t = lambda s, e, n, d: [s, e]
    rs = np.random.RandomState(9)
    vids = make_videos(CAPTION_V, seed=3)
    for v in vids:
        v['c3d'] = torch.from_numpy(rs.standard_normal((T_V, opt.video_dim)).astype(np.float32)).to(dev)
        v['lda'] = torch.from_numpy(rs.standard_normal(opt.lda_dim).astype(np.float32)).to(dev)
    kw = dict(topN=CAPTION_TOPN, nms_threshold=CAPTION_NMS)
    sel = XP.select(vids, opt.K, seed=1, device=dev, **kw)
    given = [dict(v, ind=sel.ind[i], soi=sel.soi[i], timestamps=sel.timestamps[i].tolist()) for i, v in enumerate(vids)]
    ext = lambda: EU.caption_videos(tap, cg, vids, f2t, flag_eval_what='SOTA_TEP', ext_seed=1, **kw)
    plain = lambda: EU.caption_videos(tap, cg, given, f2t, flag_eval_what='cg')
    t = {'sota_tep_ms': [], 'cg_ms': []}
    for _ in range(args.rounds):
        t['sota_tep_ms'].append(wall(ext, max(1, args.reps // 2)))
        t['cg_ms'].append(wall(plain, max(1, args.reps // 2)))
    out = {k: round(min(v), 3) for k, v in t.items()}
    out.update(V=CAPTION_V, topN=CAPTION_TOPN, nms_threshold=CAPTION_NMS, n_events=int(sel.event_offset[-1]),
               added_ms=round(out['sota_tep_ms'] - out['cg_ms'], 3), rounds_ms={k: [round(x, 3) for x in v] for k, v in t.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-caption', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'extprops_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('extprops_bench needs the GPU: a timing taken anywhere else says nothing (no fallback)')
    dev = torch.device('cuda')
    shapes = {}
    for V in BATCHES:
        videos = make_videos(V)
        for thr in THRESHOLDS:
            dev_fn = lambda: XP.select(videos, K, topN=TOPN, nms_threshold=thr, seed=7, device=dev)
            host_fn = lambda: [R.select(vid, K, topN=TOPN, nms_threshold=thr, seed=7, draw=v) for v, vid in enumerate(videos)]
            t = {'device_ms': [], 'host_ms': []}
            for _ in range(args.rounds):          # alternated: other work shares the machine
                t['device_ms'].append(wall(dev_fn, args.reps))
                t['host_ms'].append(wall(host_fn, 1))
            got, want = dev_fn(), host_fn()
            equal = all(np.array_equal(got.pick[v], want[v]['pick']) and np.array_equal(got.soi[v], want[v]['soi']) for v in range(V))
            mn = {k: min(v) for k, v in t.items()}
            shapes['V%d_nms%g' % (V, thr)] = {'device_ms': round(mn['device_ms'], 4), 'host_ms': round(mn['host_ms'], 3),
                                              'host_over_device': round(mn['host_ms'] / mn['device_ms'], 1),
                                              'rounds_ms': {k: [round(x, 4) for x in v] for k, v in t.items()},
                                              'kept': [len(p) for p in got.pick], 'lists_equal': bool(equal)}
    out = {'tool': 'extprops_bench', 'device': torch.cuda.get_device_name(0),
           'shape': {'T_v': T_V, 'K': K, 'P': P, 'topN': TOPN, 'videos': list(BATCHES), 'nms_threshold': list(THRESHOLDS)},
           'rounds': args.rounds, 'reps': args.reps,
           'host_form': 'tests/extprops_ref.select per video: eval_utils.gettopN_nms + the filter loop + targets.featstamps + crop',
           'batches': shapes}
    if not args.no_caption:
        out['caption_ms'] = caption_pair(args, dev)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

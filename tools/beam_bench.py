#!/usr/bin/env python3
"""Beam-search decode (mode='eval', beam_size = B) against the greedy decode at the benchmark and evaluation sizes (GPU box only): 64
events in the c3bench layout (8192-segment video, disjoint clips) and 1000 proposals over a 256-segment video, V1 = 5001, seq_length 19.
Prints ONE JSON line: ms per decode of the greedy path (as it is: persistent at 64 events, the launch-per-step chain at 1000), of beam
search at B = 1 (the launch-per-step chain over N rows), B = 3 and B = 5.  Not a gate.

Usage:  python tools/beam_bench.py [--reps 5] [--sizes 64,1000] [--beams 1,3,5] [--skip-greedy]"""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                              # noqa: E402

import echr_amd                                           # noqa: E402
from echr_amd import functional as EF, synth             # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()          # (a generation-2 collection of the interpreter would otherwise land in a timed decode)
    try:
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
    finally:
        gc.enable()
    return (time.perf_counter() - t0) / reps * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sizes', default='64,1000')
    ap.add_argument('--beams', default='1,3,5')
    ap.add_argument('--skip-greedy', action='store_true', help='beam decodes only (a profiler run of the beam chain)')
    args = ap.parse_args()
    dev = torch.device('cuda')
    opt = synth.default_opt(vocab_size=5000, seq_length=19)
    params = synth.make_params(opt, 0)
    m = echr_amd.CaptionGenerator(opt)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev).eval()
    lm = m.lm_model
    res = {'V1': 5001, 'seq_length': 19, 'reps': args.reps}
    for N in (int(s) for s in args.sizes.split(',')):
        T_v = 8192 if N <= 64 else 256
        vid = synth.make_video(N, 128, 21, 5001, seed=7, T_v=T_v if N > 64 else None, full_len=(N == 64), disjoint=(N == 64))
        tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
        got = {}

        def grab(video, event, clip, clip_mask, opt={}):
            got.update(video=video, event=event, clip=clip, clip_mask=clip_mask)
            return [], []
        lm.sample = grab
        with torch.no_grad():
            m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
        del lm.sample
        cv = lm._clip_view(got['clip'], got['clip_mask'])
        row = {'events': N, 'T_v': T_v}
        if not args.skip_greedy:
            with torch.no_grad():
                ms, (seq, _) = timed(lambda: lm.sample(got['video'], got['event'], got['clip'], got['clip_mask']), args.reps)
            row.update(greedy_ms=round(ms, 3), greedy_T=int(seq.shape[1]) if len(seq) else 0)
        for B in (int(b) for b in args.beams.split(',')):
            with torch.no_grad():
                ms, (seq, _, _) = timed(lambda: EF.beam_search(got['video'], got['event'], cv.feats, cv.ev_start, cv.ev_len, cv.max_len,
                                                               lm.seq_length, lm.native_params(), B), args.reps)
            row['beam%d_ms' % B] = round(ms, 3)
            row['beam%d_T' % B] = int(seq.shape[1]) if len(seq) else 0
        res['N%d' % N] = row
        del got, cv
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Beam search over a batch of videos against sequential single-video beam decodes, on the GPU (one JSON line;
profiles/beam_batch_bench.json).  Protocol and shapes of tools/eval_batch_bench.py.

For V in {1, 4, 16} videos (V1 = 5001, seq_length 20, K = 256) and beam_size B in {3, 5}, two workloads:

  cg      ground-truth events, 4 per video of 8..40 segments on T_v = 120 rows (flag_eval_what='cg')
          (a) per video: SST.forward + CaptionGenerator.forward(mode='eval', beam_size=B, return_score=True) + the reads caption_video
              makes                                                                            (b) ONE caption_videos_beam call
  tap_cg  proposals by greedy NMS (overlap 0.8, topN = 100) on T_v = 120..256 rows
          (a) V sequential eval_utils.caption_video(beam_size=B) calls                         (b) ONE caption_videos_beam call

(a) is code this tool's subject does not touch: it is the baseline.  Each figure is a host clock around `reps` repetitions that end in a
device synchronise, after a warm-up of every shape; (a) and (b) alternate inside one process, `rounds` times, and the spread over the rounds
is reported (min / median / max ms per repetition).  peak_bytes: the allocator's peak above the resident tensors during one (b) call (the
decode's workspaces dominate it), rows = events * B of its largest run.  Times and ratios only: nothing is asserted.

Usage: python tools/beam_batch_bench.py [--reps 5] [--rounds 3] [--out profiles/beam_batch_bench.json]
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
from echr_amd import eval_utils as EU, models, synth         # noqa: E402

EVENTS, SEG, T_CG, T_TAP, V1, SEQ, TOPN, NMS, BEAMS, MAX_ROWS = 4, (8, 40), 120, (120, 256), 5001, 20, 100, 0.8, (3, 5), 8192
f2t = lambda s, e, n, d: [round(float(s) / n * d, 3), round(float(e) / n * d, 3)]


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


def compare(fa, fb, args):
    """(stats of fa, stats of fb) with fa and fb alternating."""
    for _ in range(args.warmup):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(timed(fa, args.reps))
        tb.append(timed(fb, args.reps))
    return stats(ta), stats(tb)


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('beam_batch_bench needs the GPU: a timing taken anywhere else says nothing (no fallback)')
    dev = torch.device('cuda')
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=SEQ)
    params = synth.make_params(opt, 0)
    cg = echr_amd.CaptionGenerator(opt)
    cg.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    cg = cg.to(dev).eval()
    torch.manual_seed(5)
    tap = models.setup_tap(opt).to(dev)
    tap.eval()
    res = dict(tool='beam_batch_bench', device=torch.cuda.get_device_name(0), V1=V1, seq_length=SEQ, K=opt.K, topN=TOPN, nms=NMS, reps=args.reps,
               rounds=args.rounds, event_group_rows=EU.EVENT_GROUP_ROWS, max_rows=MAX_ROWS, cases=[])
    for V in (1, 4, 16):
        vids = synth.make_vbatch_videos(V, (EVENTS, EVENTS), SEG, (T_CG, T_CG), (SEQ + 1, SEQ + 1), V1, 4000, max_events=EVENTS * V)
        dv = [dict(c3d=torch.from_numpy(v['c3d']).to(dev), lda=torch.from_numpy(v['lda']).to(dev), duration=60.0, ind=v['ind'], soi=v['soi'],
                   timestamps=[f2t(s, e, T_CG, 60.0) for s, e in np.asarray(v['soi']).tolist()]) for v in vids]
        rs = np.random.RandomState(4100 + V)
        Ts = [T_TAP[0]] + rs.randint(T_TAP[0], T_TAP[1] + 1, size=V - 1).tolist() if V > 1 else [T_TAP[1]]
        tv = [dict(c3d=torch.from_numpy(rs.standard_normal((T, opt.video_dim)).astype(np.float32)).to(dev),
                   lda=torch.from_numpy(rs.standard_normal(opt.lda_dim).astype(np.float32)).to(dev), duration=60.0) for T in Ts]
        for B in BEAMS:
            # ---- cg: given events ----
            def seq_cg():
                with torch.no_grad():
                    for d in dv:
                        tf, _ = tap(d['c3d'])
                        seq, lp, score = cg(tf, d['c3d'], d['lda'], [], d['ind'], d['soi'], mode='eval', beam_size=B, return_score=True)
                        if len(seq):
                            score.cpu(), seq.cpu()

            def bat_cg():
                return EU.caption_videos_beam(tap, cg, dv, f2t, B, flag_eval_what='cg', max_rows=MAX_ROWS)

            sa, sb = compare(seq_cg, bat_cg, args)
            pk, _ = peak_bytes(bat_cg)
            case = dict(V=V, B=B, cg=dict(n_events=EVENTS * V, rows=EVENTS * V * B, sequential_ms=sa, batch_ms=sb,
                                          speedup_median=round(sa['median'] / sb['median'], 3), peak_bytes=pk))

            # ---- tap_cg: NMS proposals ----
            def seq_tap():
                for d in tv:
                    EU.caption_video(tap, cg, d['c3d'], d['lda'], d['duration'], f2t, topN=TOPN, nms_threshold=NMS, beam_size=B)

            def bat_tap():
                return EU.caption_videos_beam(tap, cg, tv, f2t, B, topN=TOPN, nms_threshold=NMS, max_rows=MAX_ROWS)

            sa, sb = compare(seq_tap, bat_tap, args)
            pk, (infos, ex) = peak_bytes(bat_tap)
            runs = ex['batch'].beam_groups(B, MAX_ROWS)
            case['tap_cg'] = dict(T=Ts, n_events=ex['batch'].n_events, n_captioned=sum(len(i) for i in infos), runs=len(runs), rows=max(e1 - e0 for _, _, e0, e1 in runs) * B,
                                  sequential_ms=sa, batch_ms=sb, speedup_median=round(sa['median'] / sb['median'], 3), peak_bytes=pk)
            echr_amd._lib.check(echr_amd._lib.load().echr_check_async(), 'beam_batch_bench')
            res['cases'].append(case)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()

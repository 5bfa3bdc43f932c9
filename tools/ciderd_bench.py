#!/usr/bin/env python3
"""What the CIDEr-D reward costs inside a self-critical iteration (GPU box only).  The workload of tools/scst_batch_bench.py: V = 1 / 4 / 16
videos of 4 events on 120 feature rows each, V1 = 5001, seq_length 20; the corpus table holds about 10^6 n-grams (synthetic documents plus
the batch's own references; an event's references are its own label and a perturbed copy of the untrained model's greedy caption).  Three forms of the SelfCriticalBatchStep
iteration, alternated in the same process:

  pinned_ms       reward= given: the floor, the reward costs nothing
  device_ms       reward_fn = CiderDReward (echr_ciderd_score queued behind the two decodes, read behind the iteration's one drain)
  host_python_ms  reward_fn = a callable that scores the host captions with tests/ciderd_ref.py -- what a user does today with a
                  pure-Python scorer; NOT a tuned host baseline

Per V it reports each form's rounds (min and all), device_cost_ms = device - pinned and host_python_cost_ms = host - pinned (on the minima),
the score launches' own time from device events (reward_pair_us: the greedy and the sampled launch of one reward; median and min), and
max_abs_diff_vs_host, the device reward of one iteration against the oracle on the captions that iteration returned.  Prints ONE JSON line
(kept in profiles/ciderd_bench.json).

Usage:  python tools/ciderd_bench.py [--reps 20] [--rounds 3] [--docs 12000]"""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402

from echr_amd import synth                                # noqa: E402
from echr_amd.batch import VideoBatch                     # noqa: E402
from echr_amd.fused import FusedTrainStep, SelfCriticalBatchStep          # noqa: E402
from echr_amd.optim import ClampAdam                      # noqa: E402
from echr_amd.reward import CiderD, CiderDReward          # noqa: E402
from tests import ciderd_ref as R                         # noqa: E402
from tests import util as U                               # noqa: E402

SEQ_LENGTH, V1, T_V, EVENTS = 20, 5001, 120, 4


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    try:
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    finally:
        gc.enable()
    return (time.perf_counter() - t0) / reps * 1e3


def bench_v(V, m, f, corpus, reps, rounds):
    opt = m.opt
    vids = synth.make_vbatch_videos(V, (EVENTS, EVENTS), (8, 60), (T_V, T_V), (SEQ_LENGTH + 2, SEQ_LENGTH + 2), V1, 2000 + V, max_events=EVENTS * V,
                                    video_dim=opt.video_dim, hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
    b = VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi')} for v in vids], device=torch.device('cuda'))
    N = b.n_events
    rs = np.random.RandomState(100 + V)
    # an event's second reference: the greedy caption of the untrained model with one word replaced (random labels share next to nothing
    # with a random model's captions at V1 = 5001: every reward would be 0)
    greedy0 = SelfCriticalBatchStep(f)(b, reward=np.zeros(N, np.float32), step=False)[2].numpy()
    docs = []
    for lab, cap in zip([lab for v in vids for lab in np.asarray(v['labels'])], greedy0):
        words = [int(x) for x in R.sequence(cap, SEQ_LENGTH) if x] or [1]
        words[rs.randint(len(words))] = int(rs.randint(1, V1))
        docs.append([list(lab), words])
    t0 = time.perf_counter()
    sc = CiderD.from_corpus(corpus + docs, SEQ_LENGTH, V1 - 1).cuda()
    t_table = time.perf_counter() - t0
    seqs_all = [[(R.label_sequence(r, SEQ_LENGTH) if len(r) > 1 and r[0] == 0 else R.sequence(r, SEQ_LENGTH)) for r in d] for d in corpus + docs]
    df, n_docs = R.document_frequency(seqs_all)
    assert len(df) == len(sc.keys) and n_docs == sc.n_docs
    seqs = seqs_all[len(corpus):]
    packed = sc.pack_refs(docs).cuda()
    bd = VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi')} for v in vids], device=torch.device('cuda'))
    bd.refs = packed
    pinned = rs.uniform(-1.0, 1.0, size=N).astype(np.float32)
    step_pinned = SelfCriticalBatchStep(f)
    step_device = SelfCriticalBatchStep(f, CiderDReward(sc))
    step_host = SelfCriticalBatchStep(f, None)

    def host_reward(gen_v, greedy_v):
        s = b.event_slices[step_host.current_video]
        return np.asarray(R.reward_rows(gen_v.numpy(), greedy_v.numpy(), seqs[s], df, n_docs, SEQ_LENGTH), np.float32)
    step_host.reward_fn = host_reward
    forms = {'pinned_ms': lambda: step_pinned(b, reward=pinned), 'device_ms': lambda: step_device(bd),
             'host_python_ms': lambda: step_host(b)}
    t = {k: [] for k in forms}
    for _ in range(rounds):          # alternated: other work shares the machine
        for k, fn in forms.items():
            t[k].append(timed(fn, reps))
    # the device reward of one iteration against the oracle on the captions it returned
    _, gen_h, greedy_h, reward, vw = step_device(bd, step=False)
    want = np.asarray(R.reward_rows(gen_h.numpy(), greedy_h.numpy(), seqs, df, n_docs, SEQ_LENGTH))
    diff = max(float(np.abs(reward.numpy()[s, :w] - want[s, None]).max()) for s, w in zip(b.event_slices, vw.tolist()) if w)
    # the two score launches alone, from device events
    gen_d, greedy_d = gen_h.cuda(), greedy_h.cuda()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    pair = []
    for _ in range(reps + 3):
        e0.record()
        sc.reward(gen_d, greedy_d, packed)
        e1.record()
        e1.synchronize()
        pair.append(e0.elapsed_time(e1) * 1e3)
    pair = pair[3:]
    mn = {k: min(v) for k, v in t.items()}
    return {'V': V, 'N': N, 'table_keys': int(len(sc.keys)), 'table_build_s': round(t_table, 2),
            'pinned_ms': round(mn['pinned_ms'], 4), 'device_ms': round(mn['device_ms'], 4), 'host_python_ms': round(mn['host_python_ms'], 4),
            'device_cost_ms': round(mn['device_ms'] - mn['pinned_ms'], 4), 'host_python_cost_ms': round(mn['host_python_ms'] - mn['pinned_ms'], 4),
            'rounds_ms': {k: [round(x, 4) for x in v] for k, v in t.items()},
            'reward_pair_us': {'median': round(float(np.median(pair)), 2), 'min': round(float(min(pair)), 2)},
            'reward_nonzero_rows': int((want != 0).sum()), 'max_abs_diff_vs_host': diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--docs', type=int, default=12000)
    args = ap.parse_args()
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=SEQ_LENGTH)
    m = U.build_gpu_model(opt, synth.make_params(opt, 0), True)
    o = ClampAdam(m.parameters(), lr=1e-6, arena=m.build_arena())
    f = FusedTrainStep(m, o, grad_clip=0.1)
    rs = np.random.RandomState(1)
    corpus = [[rs.randint(1, V1, size=rs.randint(8, SEQ_LENGTH + 1)).tolist() for _ in range(2)] for _ in range(args.docs)]
    out = [bench_v(V, m, f, corpus, args.reps, args.rounds) for V in (1, 4, 16)]
    print(json.dumps({'shape': {'events_per_video': EVENTS, 'T_v': T_V, 'V1': V1, 'seq_length': SEQ_LENGTH, 'corpus_documents': args.docs},
                      'reps': args.reps, 'rounds': args.rounds, 'host_form': 'pure-Python scorer (tests/ciderd_ref.py), not a tuned host baseline',
                      'cases': out}), flush=True)


if __name__ == '__main__':
    main()

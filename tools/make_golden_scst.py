#!/usr/bin/env python3
"""Generate the self-critical training fixtures from the REFERENCE's own code (build container only).

Runs the reference's CaptionGenerator.forward(mode='train_rl') (CaptionGenerator.py:32-37) on CPU in training mode -- the decoder's and the
event encoder's dropout fed with the build's Philox masks in the reference's own call order (tools/make_golden.py's MaskFeeder), the draws
from a seeded torch.multinomial -- applies a fixed synthetic reward (stored in the fixture) through the reference's RewardCriterion
(misc/utils.py:48-59) and runs backward.  Writes tests/golden/case_scst.npz (the 'tiny' case) and tests/golden/case_scst_eos.npz (a case
whose rows finish at different steps, one of them at the first draw, with a non-empty greedy baseline):

    gen_result int64 [N,T] | sample_logprobs [N,T] | greedy_res int64 [N,T'] | reward [N,T] | loss | grad|<parameter> ...

The shims and the mask feeder are imported from tools/make_golden.py (which imports the reference in place; nothing of it is copied).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_scst.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG                     # noqa: E402  (shims, MaskFeeder, build_ref; imports the reference)

from echr_amd import synth                   # noqa: E402

F = MG.F


def run_train_rl(m, opt, vid, draw_seed):
    tap, c3d, lda = (torch.from_numpy(vid[k]) for k in ('tap', 'c3d', 'lda'))
    m.zero_grad()
    m.train()
    orig = F.dropout
    F.dropout = MG.MaskFeeder(opt.CG_drop_prob)
    torch.manual_seed(draw_seed)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            gen, slp, greedy = m(tap, c3d, lda, [], vid['ind'], vid['soi'].tolist(), mode='train_rl')
    finally:
        F.dropout = orig
    return gen, slp, greedy


def finish_steps(gen):
    g = gen.numpy()
    return np.array([(np.nonzero(r == 0)[0][0] if (r == 0).any() else g.shape[1]) for r in g])


def do_case(out_name, opt, params, vid, want_mix):
    m = MG.build_ref(opt, params)
    for draw_seed in range(200):
        gen, slp, greedy = run_train_rl(m, opt, vid, draw_seed)
        if not isinstance(gen, torch.Tensor):
            continue
        fin = finish_steps(gen)
        # the mixed case: rows finish at three or more different steps, one of them at the first draw (mask [1, 0, ...]) and at least one
        # row never (it sets the trimmed length)
        if not want_mix or (len(set(fin.tolist())) >= 3 and fin.min() == 0 and fin.max() == gen.shape[1] and isinstance(greedy, torch.Tensor)):
            break
    else:
        raise SystemExit('%s: no draw seed gave the wanted finish pattern' % out_name)
    N, T = gen.shape
    if not isinstance(greedy, torch.Tensor):          # every greedy row ended at its first step: OldModel.sample returns [] (:186-187)
        greedy = torch.zeros(N, 0, dtype=torch.int64)
    rs = np.random.RandomState(1234)
    reward = torch.from_numpy(rs.uniform(-1.0, 1.0, size=(N, T)).astype(np.float32))          # signed, per position
    loss = MG.ref_utils.RewardCriterion()(slp, gen, reward)
    loss.backward()
    out = {'gen_result': gen.numpy().astype(np.int64), 'sample_logprobs': slp.detach().numpy().astype(np.float32),
           'greedy_res': greedy.numpy().astype(np.int64), 'reward': reward.numpy(), 'loss': np.float64(float(loss.detach())),
           'draw_seed': np.int64(draw_seed)}
    for k, p in m.named_parameters():
        if p.grad is not None:
            out['grad|' + k] = p.grad.detach().numpy().astype(np.float32)
    path = os.path.join(MG.GOLD, out_name)
    np.savez_compressed(path, **out)
    print('[%s] draw seed %d  gen %s  finish steps %s  greedy %s  loss %.6f  -> %d bytes'
          % (out_name, draw_seed, tuple(gen.shape), finish_steps(gen).tolist(), tuple(greedy.shape), float(loss), os.path.getsize(path)))


def main():
    opt, params, vid = synth.make_case('tiny')
    do_case('case_scst.npz', opt, params, vid, False)
    opt, params, vid = synth.make_case('tiny_eos')
    do_case('case_scst_eos.npz', opt, params, vid, True)


if __name__ == '__main__':
    main()

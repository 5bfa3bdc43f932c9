#!/usr/bin/env python3
"""Generate the fixture of self-critical training over a multi-video batch from the REFERENCE's own code (build container only).

The reference runs one video per call and sums the gradients of `m_batch` videos before one clamp + step (train.py:281-283,313-317); past
--self_critical_after every one of those calls is CaptionGenerator.forward(mode='train_rl') (CaptionGenerator.py:32-37, train.py:303-308).
This tool runs exactly that on echr_amd.synth.VBATCH['vbscst'], video by video in training mode: the decoder's and the event encoder's
dropout fed with the matching SLICES of the batch's Philox masks in the reference's own call order (tools/make_golden_vbatch.py's
SlicedMaskFeeder), the draws from a seeded torch.multinomial (one seed per video), a fixed signed per-position reward through the
reference's RewardCriterion (misc/utils.py:48-59), backward accumulated over the videos.  Writes tests/golden/case_scst_batch.npz:

    gen_result|v<k> int64 [N_v,T_v] | sample_logprobs|v<k> | greedy_res|v<k> int64 [N_v,T'_v] | reward|v<k> [N_v,T_v] | losses [V] | loss
    | draw_seeds [V] | grad|<parameter> of the ACCUMULATED gradient

The draw seeds are searched and nothing is written unless the draws contain at least two different video widths, a video narrower than
the batch whose widest row has no <eos> inside its width (at the batch's width that row would gain a criterion position its own call does
not have), and a row that draws <eos> first.  tests/scst_batch_ref.py (the CPU reference of the batch contract) is checked against the
reference before anything is written.  The shims, build_ref and the mask feeder come from tools/make_golden.py / make_golden_vbatch.py,
which import the reference in place; nothing of it is copied.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_scst_batch.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG                     # noqa: E402  (shims, build_ref; imports the reference)
import make_golden_vbatch as MV              # noqa: E402  (SlicedMaskFeeder)

from echr_amd import synth                   # noqa: E402
from tests import scst_batch_ref as R        # noqa: E402
from tests import vbatch_ref as VR           # noqa: E402

F = MG.F
CASE = 'vbscst'
MAX_SEEDS = 5000


def run_train_rl(m, vid, n_tot, e0, e1, draw_seed):
    tap, c3d, lda = (torch.from_numpy(vid[k]) for k in ('tap', 'c3d', 'lda'))
    m.train()
    orig = F.dropout
    F.dropout = MV.SlicedMaskFeeder(n_tot, e0, e1)
    torch.manual_seed(draw_seed)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return m(tap, c3d, lda, [], vid['ind'], vid['soi'].tolist(), mode='train_rl')
    finally:
        F.dropout = orig


def widths(gen):
    """(width of the video = its tensor's width, per-row number of words)."""
    if not isinstance(gen, torch.Tensor):
        return 0, np.zeros(0, np.int64)
    return gen.shape[1], (gen.numpy() != 0).sum(1)


def wanted(gens):
    """The coverage the fixture promises, on the per-video samples of one seed choice."""
    ws = [widths(g) for g in gens]
    T = max(w for w, _ in ws)
    different = len({w for w, _ in ws}) >= 2
    # a video narrower than the batch whose widest row fills its width: no <eos> inside, so mask[n, T_v] would be 1 at the batch's width
    narrow_full = any(0 < w < T and int(rows.max()) == w for w, rows in ws)
    eos_first = any(w > 0 and int(rows.min()) == 0 for w, rows in ws)
    return different and narrow_full and eos_first


def main():
    opt, params, videos = synth.make_vbatch(CASE)
    m = MG.build_ref(opt, params)
    eo = VR.offsets(videos)
    V = len(videos)
    def first_seed(v, ok):
        """First draw seed 10000 * v + k of video v whose sample satisfies ok(width, words per row) (forward only)."""
        for k in range(MAX_SEEDS):
            with torch.no_grad():
                gen, _, _ = run_train_rl(m, videos[v], eo[-1], eo[v], eo[v + 1], 10000 * v + k)
            if ok(*widths(gen)):
                return 10000 * v + k
        raise SystemExit('video %d: none of %d draw seeds gave the wanted sample' % (v, MAX_SEEDS))

    L = opt.CG_seq_length
    narrow = int(np.argmin(np.diff(eo)))          # the video with the fewest events is the likeliest to finish early
    first = (narrow + 1) % V                      # another video supplies the row that draws <eos> first, at the full width
    seeds = []
    for v in range(V):
        if v == narrow:
            seeds.append(first_seed(v, lambda w, rows: 0 < w < L))
        elif v == first:
            seeds.append(first_seed(v, lambda w, rows: w == L and int(rows.min()) == 0))
        else:
            seeds.append(first_seed(v, lambda w, rows: w > 0))
    m.zero_grad()
    out, gens, rewards, losses, slps, greedys = {}, [], [], [], [], []
    rs = np.random.RandomState(4321)
    for v, vid in enumerate(videos):
        gen, slp, greedy = run_train_rl(m, vid, eo[-1], eo[v], eo[v + 1], seeds[v])
        n = len(vid['soi'])
        greedy = greedy.numpy().astype(np.int64) if isinstance(greedy, torch.Tensor) else np.zeros((n, 0), np.int64)
        if not isinstance(gen, torch.Tensor):          # every row drew <eos> first: the call returns [] and the video trains nothing
            gen_a, slp_a, rew, loss = np.zeros((n, 0), np.int64), np.zeros((n, 0), np.float32), np.zeros((n, 0), np.float32), 0.0
        else:
            rew = rs.uniform(-1.0, 1.0, size=tuple(gen.shape)).astype(np.float32)          # signed, per position
            l = MG.ref_utils.RewardCriterion()(slp, gen, torch.from_numpy(rew))
            l.backward()          # accumulates over the videos
            gen_a, slp_a, loss = gen.numpy().astype(np.int64), slp.detach().numpy().astype(np.float32), float(l.detach())
        gens.append(gen_a); slps.append(slp_a); rewards.append(rew); losses.append(loss); greedys.append(greedy)
        for name, a in (('gen_result', gen_a), ('sample_logprobs', slp_a), ('greedy_res', greedy), ('reward', rew)):
            out['%s|v%02d' % (name, v)] = a
    assert wanted([torch.from_numpy(g) if g.shape[1] else [] for g in gens])
    grads = {k: (p.grad.detach().numpy().copy() if p.grad is not None else None) for k, p in m.named_parameters()}
    out['losses'] = np.asarray(losses, np.float64)
    out['loss'] = np.float64(np.sum(np.asarray(losses, np.float64)))
    out['draw_seeds'] = np.asarray(seeds, np.int64)
    for k, g in grads.items():
        if g is not None:
            out['grad|' + k] = g.astype(np.float32)
    # the CPU reference of the batch contract against the reference itself, before anything is written
    ref = R.run(opt, params, videos, gens, rewards)
    mask = [np.concatenate([np.ones((len(g), 1), bool), g[:, :-1] > 0], 1) if g.shape[1] else np.zeros(g.shape, bool) for g in gens]
    dl = max([float(np.abs(a - b)[k].max()) for a, b, k in zip(ref['slp'], slps, mask) if k.any()])
    dev = max(MG.rel(ref['grads'][k], grads[k]) for k in grads if grads[k] is not None and not k.endswith('alpha_net.bias'))
    print('[%s] scst_batch_ref-vs-ref: max|dlogp| %.2e  max dloss_v %.2e  max rel grad %.2e'
          % (CASE, dl, float(np.abs(ref['losses'] - np.asarray(losses)).max()), dev))
    assert dl < 2e-5 and float(np.abs(ref['losses'] - np.asarray(losses)).max()) < 1e-5 and dev < 1e-4
    assert all(np.array_equal(a, b) for a, b in zip(ref['greedy'], greedys)), 'oracle greedy baseline differs'
    path = os.path.join(MG.GOLD, 'case_scst_batch.npz')
    np.savez_compressed(path, **out)
    print('[%s] draw seeds %s  widths %s  words per row %s  greedy widths %s  losses %s -> %d bytes'
          % (CASE, seeds, [g.shape[1] for g in gens], [(g != 0).sum(1).tolist() for g in gens], [g.shape[1] for g in greedys],
             np.round(losses, 6).tolist(), os.path.getsize(path)))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Generate the fixture of the frame-level contexts 'CH' / 'CC+CH' over a multi-video batch from the REFERENCE's own code (build container only).

The reference's CaptionGenerator runs video by video on the cases 'vbch' and 'vbcch' of echr_amd.synth.VBATCH with gradient accumulation over the
V videos (tools/make_golden_vbatch.py's protocol: eval and training mode, the latter under the matching slices of the batch's Philox dropout
masks), with tap_feats a leaf, then its greedy decode per video.  Writes tests/golden/case_clip_batch.npz (summaries only):

    <case>|<mode>|loss, |losses [V], |logp|v<k> [N_v, S_v, 64 columns], |grad|<parameter>|<summary> of the ACCUMULATED gradient,
    <case>|<mode>|gtap|v<k> [T_v, 64 columns of Ht] and |gtap_l2|v<k>: d loss / d tap_feats of video k
    <case>|sample|seq|v<k> int64, |sample|logp|v<k>, |sample|min_margin

tests/clip_batch_ref.py is checked against the reference before anything is written (2e-5 / 1e-5 / 1e-4 for log-probs / losses / gradients, d tap
included), and every greedy step's top-1 / top-2 margin must exceed 2e-5.  The shims and build_ref come from tools/make_golden.py, which imports
the reference in place; nothing of it is copied.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_clip_batch.py
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
import make_golden_vbatch as MV              # noqa: E402  (SlicedMaskFeeder, decode)

from echr_amd import synth                   # noqa: E402
from oracle import summary as SM             # noqa: E402
from tests import clip_batch_ref as R        # noqa: E402
from tests import vbatch_ref as VR           # noqa: E402

F = MG.F
MIN_MARGIN = 2e-5
MAX_BYTES = 750 * 1024


def run_ref(m, videos, train_mode):
    """The reference video by video, gradients accumulated: (per-video log-probs, per-video losses, accumulated gradients, d tap per video)."""
    eo = VR.offsets(videos)
    m.zero_grad()
    logps, losses, g_taps = [], [], []
    for v, vid in enumerate(videos):
        tap = torch.from_numpy(vid['tap'].copy()).requires_grad_(True)
        c3d, lda = (torch.from_numpy(vid[k]) for k in ('c3d', 'lda'))
        labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
        orig = F.dropout
        if train_mode:
            m.train()
            F.dropout = MV.SlicedMaskFeeder(eo[-1], eo[v], eo[v + 1])
        else:
            m.eval()
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'].tolist(), mode='train')
        finally:
            F.dropout = orig
        loss = MG.ref_utils.LanguageModelCriterion()(pred, labels[:, 1:], masks[:, 1:])
        loss.backward()
        logps.append(pred.detach().numpy())
        losses.append(float(loss))
        g_taps.append(tap.grad.numpy().copy())
    grads = {k: (p.grad.detach().numpy().copy() if p.grad is not None else None) for k, p in m.named_parameters()}
    return logps, np.asarray(losses), grads, g_taps


def do_case(name, out):
    opt, params, videos = synth.make_vbatch(name)
    m = MG.build_ref(opt, params)
    cols = SM.logp_columns(opt.CG_vocab_size + 1)
    tcols = SM.logp_columns(opt.hidden_dim)
    for mode in ('eval', 'train'):
        logps, losses, grads, g_taps = run_ref(m, videos, mode == 'train')
        ref = R.run(opt, params, videos, mode == 'train')
        dl = max(float(np.abs(a - b).max()) for a, b in zip(ref['logp'], logps))
        dev = max(MG.rel(ref['grads'][k], grads[k]) for k in grads if grads[k] is not None)
        dtap = max(MG.rel(a, b) for a, b in zip(ref['g_tap'], g_taps))
        print('[%s/%s] V %d N_tot %d loss %.6f | clip_batch_ref-vs-ref: max|dlogp| %.2e  max dloss_v %.2e  max rel grad %.2e  max rel d tap %.2e'
              % (name, mode, len(videos), VR.offsets(videos)[-1], losses.sum(), dl, float(np.abs(ref['losses'] - losses).max()), dev, dtap))
        assert dl < 2e-5 and float(np.abs(ref['losses'] - losses).max()) < 1e-5 and dev < 1e-4 and dtap < 1e-4
        key = name + '|' + mode
        out[key + '|loss'] = np.float64(np.sum(losses.astype(np.float64)))
        out[key + '|losses'] = losses.astype(np.float64)
        for v, lp in enumerate(logps):
            out[key + '|logp|v%02d' % v] = lp[:, :, cols].astype(np.float32)
            out[key + '|gtap|v%02d' % v] = g_taps[v][:, tcols].astype(np.float32)
            out[key + '|gtap_l2|v%02d' % v] = np.float64(np.sqrt((g_taps[v].astype(np.float64) ** 2).sum()))
        for k, v in SM.summarize_grads(grads).items():
            out[key + '|grad|' + k] = v
    m.eval()
    osamp = R.sample(opt, params, videos)
    margin = np.inf
    for v, vid in enumerate(videos):
        seq, slp, mg = MV.decode(m, vid)
        margin = min(margin, mg)
        oseq = osamp[v][0]
        if isinstance(seq, list):
            assert isinstance(oseq, list)
            out[name + '|sample|seq|v%02d' % v] = np.zeros((len(vid['soi']), 0), np.int64)
            out[name + '|sample|logp|v%02d' % v] = np.zeros((len(vid['soi']), 0), np.float32)
            continue
        assert torch.equal(seq, oseq), 'oracle greedy seq differs (video %d)' % v
        out[name + '|sample|seq|v%02d' % v] = seq.numpy().astype(np.int64)
        out[name + '|sample|logp|v%02d' % v] = slp.numpy().astype(np.float32)
    print('[%s/sample] smallest top-1 / top-2 margin over all decoded steps: %.3e; lengths %s'
          % (name, margin, [out[name + '|sample|seq|v%02d' % v].shape[1] for v in range(len(videos))]))
    assert margin > MIN_MARGIN, 'greedy margin %.3e does not exceed %.1e: pick another case seed (echr_amd.synth.VBATCH)' % (margin, MIN_MARGIN)
    out[name + '|sample|min_margin'] = np.float64(margin)


def main():
    out = {}
    for name in ('vbch', 'vbcch'):
        do_case(name, out)
    path = os.path.join(MG.GOLD, 'case_clip_batch.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote %s (%d arrays, %d bytes)' % (os.path.basename(path), len(out), size))
    assert size < MAX_BYTES, 'the fixture must stay below the largest existing one'


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Generate the frame-level context fixtures ('CH', 'CC+CH') from the REFERENCE's own code (build container only).

Runs the reference's CaptionGenerator (clip_context_type 'CH' / 'CC+CH', CaptionGenerator.py:140-167) on CPU with tap_feats as a leaf that
requires grad -- eval mode and training mode with the build's Philox dropout masks in the reference's own call order (tools/make_golden.py's
MaskFeeder) -- through LanguageModelCriterion and backward, then its greedy decode.  Writes tests/golden/case_ch.npz and case_cch.npz:

    <mode>|loss | <mode>|logp|<summary> | <mode>|grad|<parameter>|<summary> | train|g_tap [T_v, 512] (d tap_feats in full) | eval|g_tap|<summary>
    sample|seq int64 | sample|logp | state_dict|keys (names) | state_dict|shapes (int64 [n, 4], -1 padded)

tests/clipctx_ref.py (the CPU oracle of these contexts) is checked against the reference here before anything is written.  The shims and
the mask feeder come from tools/make_golden.py (which imports the reference in place; nothing of it is copied).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_clipctx.py
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
import make_golden as MG                     # noqa: E402  (shims, MaskFeeder, build_ref; imports the reference)

from echr_amd import synth                   # noqa: E402
from oracle import summary as SM             # noqa: E402
from tests import clipctx_ref as R           # noqa: E402

F = MG.F


def run_ref(m, opt, vid, train_mode):
    tap = torch.from_numpy(vid['tap'].copy()).requires_grad_(True)
    c3d, lda = (torch.from_numpy(vid[k]) for k in ('c3d', 'lda'))
    labels = torch.from_numpy(vid['labels'])
    masks = torch.from_numpy(vid['masks'])
    m.zero_grad()
    orig = F.dropout
    if train_mode:
        m.train()
        F.dropout = MG.MaskFeeder(opt.CG_drop_prob)
    else:
        m.eval()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'].tolist(), mode='train')
    finally:
        F.dropout = orig
    loss = MG.ref_utils.LanguageModelCriterion()(pred, labels[:, 1:], masks[:, 1:])
    loss.backward()
    grads = {k: (p.grad.detach().numpy().copy() if p.grad is not None else None) for k, p in m.named_parameters()}
    return pred.detach().numpy(), float(loss), grads, tap.grad.numpy().copy()


def do_case(name):
    opt, params, vid = synth.make_case(name)
    m = MG.build_ref(opt, params)
    out = {}
    for mode in ('eval', 'train'):
        pred, loss, grads, g_tap = run_ref(m, opt, vid, mode == 'train')
        opred, oloss, ograds, og_tap = R.run(opt, params, vid, mode == 'train')
        dev = max(MG.rel(ograds[k], grads[k]) for k in grads if grads[k] is not None)
        print('[%s/%s] loss %.6f | oracle-vs-ref: max|dlogp| %.2e  dloss %.2e  max rel grad %.2e  rel d tap %.2e'
              % (name, mode, loss, np.abs(opred - pred).max(), abs(oloss - loss), dev, MG.rel(og_tap, g_tap)))
        assert np.abs(opred - pred).max() < 2e-5 and abs(oloss - loss) < 1e-5 and dev < 1e-4 and MG.rel(og_tap, g_tap) < 1e-4
        out[mode + '|loss'] = np.float64(loss)
        for k, v in SM.summarize_logp(pred).items():
            out[mode + '|logp|' + k] = v
        for k, v in SM.summarize_grads(grads).items():
            out[mode + '|grad|' + k] = v
        if mode == 'train':
            out[mode + '|g_tap'] = g_tap.astype(np.float32)
        else:
            for k, v in SM.summarize_grads({'g_tap': g_tap}).items():
                out[mode + '|' + k] = v
    m.eval()
    tap, c3d, lda = (torch.from_numpy(vid[k]) for k in ('tap', 'c3d', 'lda'))
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        seq, slp = m(tap, c3d, lda, [], vid['ind'], vid['soi'].tolist(), mode='eval')
    oseq, oslp = R.sample(opt, params, vid)
    assert torch.equal(seq, oseq), 'oracle greedy seq differs'
    out['sample|seq'] = seq.numpy().astype(np.int64)
    out['sample|logp'] = slp.numpy().astype(np.float32)
    sd = m.state_dict()
    out['state_dict|keys'] = np.array(list(sd.keys()))
    shp = np.full((len(sd), 4), -1, dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shp[i, :v.dim()] = v.shape
    out['state_dict|shapes'] = shp
    path = os.path.join(MG.GOLD, 'case_%s.npz' % name)
    np.savez_compressed(path, **out)
    print('  wrote %s (%d arrays, %d bytes); greedy seq %s' % (os.path.basename(path), len(out), os.path.getsize(path), tuple(seq.shape)))


def main():
    for name in ('ch', 'cch'):
        do_case(name)


if __name__ == '__main__':
    main()

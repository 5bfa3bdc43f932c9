#!/usr/bin/env python3
"""Generate the fixture of the non-zero initial decoder state (CG_init_feats_type) over a multi-video batch from the REFERENCE's own code
(build container only).

The reference's CaptionGenerator, built with CG_init_feats_type, runs video by video on the cases 'vbinit' ('VEC' over 'CC' rows) and
'vbinitch' ('VE' over 'CH' rows) of echr_amd.synth.VBATCH with gradient accumulation over the V videos (tools/make_golden_clip_batch.py's
protocol: eval and training mode, the latter under the matching slices of the batch's Philox dropout masks, tap_feats a leaf), then its greedy
decode per video.  Every video is a call of its own, so its clip.mean(1) runs over the padded slots of ITS clip tensor.  Writes
tests/golden/case_init_batch.npz (summaries only), keyed like case_clip_batch.npz:

    <case>|<mode>|loss, |losses [V], |logp|v<k> [N_v, S_v, 64 columns], |grad|<parameter>|<summary> of the ACCUMULATED gradient
    (init_linear included), <case>|<mode>|gtap|v<k> [T_v, 64 columns of Ht] and |gtap_l2|v<k>
    <case>|sample|seq|v<k> int64, |sample|logp|v<k>, |sample|min_margin, <case>|video_len int64 [V]

tests/init_batch_ref.py is checked against the reference before anything is written (2e-5 / 1e-5 / 1e-4 for log-probs / losses / gradients,
d tap included), and every greedy step's top-1 / top-2 margin must exceed 2e-5.  The shims and build_ref come from tools/make_golden.py,
which imports the reference in place; nothing of it is copied.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_init_batch.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG                     # noqa: E402  (shims, build_ref; imports the reference)
import make_golden_vbatch as MV              # noqa: E402  (decode)
import make_golden_clip_batch as MC          # noqa: E402  (run_ref: the reference video by video, gradients accumulated, tap a leaf)

from echr_amd import synth                   # noqa: E402
from oracle import summary as SM             # noqa: E402
from tests import init_batch_ref as R        # noqa: E402

MIN_MARGIN = 2e-5
MAX_BYTES = 750 * 1024


def do_case(name, out):
    opt, params, videos = synth.make_vbatch(name)
    assert opt.CG_init_feats_type, name
    m = MG.build_ref(opt, params)
    cols = SM.logp_columns(opt.CG_vocab_size + 1)
    tcols = SM.logp_columns(opt.hidden_dim)
    out[name + '|video_len'] = R.video_max_len(videos)
    for mode in ('eval', 'train'):
        logps, losses, grads, g_taps = MC.run_ref(m, videos, mode == 'train')
        ref = R.run(opt, params, videos, mode == 'train')
        assert grads['lm_model.init_linear.weight'] is not None and float(np.abs(grads['lm_model.init_linear.weight']).max()) > 0
        dl = max(float(np.abs(a - b).max()) for a, b in zip(ref['logp'], logps))
        dev = max(MG.rel(ref['grads'][k], grads[k]) for k in grads if grads[k] is not None)
        dtap = max(MG.rel(a, b) for a, b in zip(ref['g_tap'], g_taps))
        print('[%s/%s] V %d N_tot %d loss %.6f | init_batch_ref-vs-ref: max|dlogp| %.2e  max dloss_v %.2e  max rel grad %.2e  max rel d tap %.2e'
              % (name, mode, len(videos), R.offsets(videos)[-1], losses.sum(), dl, float(np.abs(ref['losses'] - losses).max()), dev, dtap))
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
    for name in ('vbinit', 'vbinitch'):
        do_case(name, out)
    path = os.path.join(MG.GOLD, 'case_init_batch.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print('wrote %s (%d arrays, %d bytes)' % (os.path.basename(path), len(out), size))
    assert size < MAX_BYTES, 'the fixture must stay below the largest existing one'


if __name__ == '__main__':
    main()

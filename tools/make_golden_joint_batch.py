#!/usr/bin/env python3
"""Generate the joint multi-video fixture from the REFERENCE's own code (build container only).

The reference's stage 3 (finetune.sh, training_mode 'tap_cg', train.py:292-329) runs one video per call and sums the gradients of `m_batch`
videos before one clamp + step per model.  This tool runs the reference's own SST, CaptionGenerator, TAPModelCriterion and
LanguageModelCriterion video by video on echr_amd.synth's 'vbctx' (K = 16 anchors, lambda1 = 0.01, lambda2 = 1), both models in eval mode as
case_c5.npz, with gradient accumulation over the V videos.  Writes tests/golden/case_joint_batch.npz (summaries only):

    eval|tap_losses [V], eval|cg_losses [V], eval|grad|<caption parameter>|<summary>, eval|sstgrad|<SST parameter>|<summary>
    (summary: l2, linf, head, strided of the ACCUMULATED gradient -- oracle/summary.py)

tests/joint_batch_ref.py (the CPU reference of the joint batch contract) is checked against the reference here before anything is written.
The shims and build_ref come from tools/make_golden.py, which imports the reference in place; nothing of it is copied.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_joint_batch.py
"""
import contextlib
import copy
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

from oracle import summary as SM             # noqa: E402
from tests import joint_batch_ref as J       # noqa: E402

LAMBDA2 = 1.0


def run_ref(opt, params, sst_params, vids, tap_in):
    """The reference video by video, gradients of both models accumulated over the videos."""
    m = MG.build_ref(opt, params)
    tapm = MG.models.setup_tap(copy.copy(opt))
    tapm.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sst_params.items()})
    m.eval()
    tapm.eval()
    m.zero_grad()
    tapm.zero_grad()
    ro = J.row_offsets(vids)
    tl, cl = [], []
    for v, vid in enumerate(vids):
        T = ro[v + 1] - ro[v]
        c3d, lda = torch.from_numpy(np.ascontiguousarray(vid['c3d'][:T])), torch.from_numpy(vid['lda'])
        labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
        mk, lab, w1 = (torch.from_numpy(x) for x in tap_in[v])
        with contextlib.redirect_stdout(io.StringIO()):
            tap_feats, props = tapm(c3d)
            pred = m(tap_feats, c3d, lda, labels, vid['ind'], vid['soi'].tolist(), mode='train')
        tap_loss = MG.ref_utils.TAPModelCriterion()(props, mk, lab, w1)
        cg_loss = MG.ref_utils.LanguageModelCriterion()(pred, labels[:, 1:], masks[:, 1:])
        (J.LAMBDA1 * tap_loss + LAMBDA2 * cg_loss).backward()
        tl.append(float(tap_loss))
        cl.append(float(cg_loss))
    grads = {k: (p.grad.detach().numpy().copy() if p.grad is not None else None) for k, p in m.named_parameters()}
    sgrads = {k: p.grad.detach().numpy().copy() for k, p in tapm.named_parameters()}
    return np.asarray(tl), np.asarray(cl), grads, sgrads


def main():
    opt, params, sst_params, vids, tap_in = J.setup('vbctx')
    tl, cl, grads, sgrads = run_ref(opt, params, sst_params, vids, tap_in)
    ref = J.run(opt, params, sst_params, vids, tap_in, False, J.LAMBDA1, LAMBDA2)
    dev = max(MG.rel(ref['grads'][k], grads[k]) for k in grads if grads[k] is not None and not k.endswith('alpha_net.bias'))
    sdev = max(MG.rel(ref['sst_grads'][k], sgrads[k]) for k in sgrads)
    dl = max(float(np.abs(ref['tap_losses'] - tl).max() / np.abs(tl).max()), float(np.abs(ref['cg_losses'] - cl).max() / np.abs(cl).max()))
    print('[vbctx/eval] V %d rows %d events %d tap %s cg %s | joint_batch_ref-vs-ref: max rel dloss %.2e  max rel grad %.2e (cg) %.2e (sst)'
          % (len(vids), ref['row_offset'][-1], ref['event_offset'][-1], np.round(tl, 4), np.round(cl, 4), dl, dev, sdev))
    assert dl < 1e-5 and dev < 1e-4 and sdev < 1e-4
    out = {'eval|tap_losses': tl.astype(np.float64), 'eval|cg_losses': cl.astype(np.float64), 'lambda': np.asarray([J.LAMBDA1, LAMBDA2])}
    for k, v in SM.summarize_grads(grads).items():
        out['eval|grad|' + k] = v
    for k, v in SM.summarize_grads(sgrads).items():
        out['eval|sstgrad|' + k] = v
    path = os.path.join(MG.GOLD, 'case_joint_batch.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d arrays, %d bytes)' % (os.path.basename(path), len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()

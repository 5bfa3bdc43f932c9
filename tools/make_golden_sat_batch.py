#!/usr/bin/env python3
"""Generate the fixture of the one-stream decoder over a multi-video batch from the REFERENCE's own code (build container only).

The reference takes one video per call and sums the gradients of m_batch videos before one step (train.py:281-283,313-317).  Its
CaptionGenerator (caption_model='show_attend_tell', the parameters of echr_amd.synth.make_sat_params) runs the videos of a case of
tests/sat_batch_ref.CASES one after the other WITHOUT clearing the gradients in between: the per-video log-probs and losses, the summed
gradients, d tap_feats per video.  Training mode runs under the build's Philox masks fed through the patched F.dropout (as
tools/make_golden_sat.py does): video v gets rows [e0:e1] of the batch's [N_tot, H] output masks and [e0:e1, :, e0:e1] of the event
encoder's [N_tot, G, N_tot] mask -- a batched call keys every site by the batch-global element.  Each video is decoded greedily, with the
margins of the reference's own get_logprobs_state chain.  tests/sat_batch_ref.py is checked against all of it (1e-5 relative) before
anything is written.  Writes tests/golden/case_sat_batch.npz, data only:

  fixture|<mode>|loss, |losses [V], |logp|<v>, |gtap|<v>, |grad|<parameter>; fixture|sample|seq|<v>, |logp|<v>, |margin|<v>
                              full tensors of 'fixture' (V = 3, TINY widths)
  widths|<mode>|loss, |losses, |logp|<v>|<summary>, |gtap|<v>|<summary>, |grad|<parameter>|<summary>
                              summaries (oracle/summary.py) of 'widths' (V = 2 at the ECHR widths)

The shims and build_ref come from tools/make_golden.py, which imports the reference in place; nothing of it is copied.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_sat_batch.py
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
import make_golden_sat as MGS                # noqa: E402  (decode)
import torch.nn.functional as F              # noqa: E402

from echr_amd import philox                  # noqa: E402
from oracle import summary as SM             # noqa: E402
from tests import sat_batch_ref as B         # noqa: E402
from tests import sat_ref as R               # noqa: E402
from tests import util as U                  # noqa: E402

TOL = 1e-5
MIN_MARGIN, MIN_SHARE = 1e-4, 0.9


class BatchFeeder:
    """Replaces F.dropout for video [e0, e1) of a batch of n_tot events: the event encoder's mask first (when there is an encoder), then
    one output mask per step, each the video's slice of the batch-global mask."""

    def __init__(self, encoder, n_tot, e0, e1):
        self.calls = 0 if encoder else 1
        self.n_tot, self.e0, self.e1 = n_tot, e0, e1

    def __call__(self, x, p=0.5, training=True, inplace=False):
        if not training:
            return x
        e0, e1 = self.e0, self.e1
        if self.calls == 0:
            m = philox.scale_mask((self.n_tot, x.shape[1], self.n_tot), p, U.SEED, U.OFFSET, philox.SITE_TSRM, 0)[e0:e1, :, e0:e1]
        else:
            m = philox.scale_mask((self.n_tot, x.shape[1]), p, U.SEED, U.OFFSET, philox.SITE_OUT, self.calls - 1)[e0:e1]
        self.calls += 1
        assert tuple(m.shape) == tuple(x.shape), (m.shape, x.shape)
        return x * torch.from_numpy(np.ascontiguousarray(m))


def run_ref(m, videos, train_mode):
    """The m_batch protocol: one forward / backward per video, the gradients accumulating."""
    eo = B.offsets(videos)
    m.zero_grad()
    m.train(train_mode)
    logps, losses, g_taps = [], [], []
    for v, vid in enumerate(videos):
        tap = torch.from_numpy(vid['tap'].copy()).requires_grad_(True)
        c3d, lda = torch.from_numpy(vid['c3d']), torch.from_numpy(vid['lda'])
        labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
        orig = F.dropout
        feeder = BatchFeeder(hasattr(m, 'fusion_model'), eo[-1], eo[v], eo[v + 1])
        if train_mode:
            F.dropout = feeder
        try:
            pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'].tolist(), mode='train')
        finally:
            F.dropout = orig
        if train_mode:
            assert feeder.calls - 1 == pred.shape[1], (feeder.calls, pred.shape)
        loss = MG.ref_utils.LanguageModelCriterion()(pred, labels[:, 1:], masks[:, 1:])
        loss.backward()
        logps.append(pred.detach().numpy())
        losses.append(float(loss))
        g_taps.append(tap.grad.numpy().copy() if tap.grad is not None else np.zeros_like(vid['tap']))
    grads = {k: (p.grad.detach().numpy().copy() if p.grad is not None else None) for k, p in m.named_parameters()}
    return dict(logp=logps, loss=float(np.sum(np.asarray(losses, np.float64))), losses=np.asarray(losses), grads=grads, g_tap=g_taps)


def check(name, mode, ref, got):
    unused = sorted(k for k in ref['grads'] if ref['grads'][k] is None)
    assert unused == sorted(k for k in got['grads'] if got['grads'][k] is None)
    dl = max(MG.rel(a, b) for a, b in zip(got['logp'], ref['logp']))
    dloss = float(np.abs(got['losses'] - ref['losses']).max() / np.abs(ref['losses']).max())
    assert all(float(np.abs(x['grads'][k]).max()) < 1e-6 for x in (ref, got) for k in R.NOISE_ONLY if x['grads'][k] is not None)
    dev = max(U.relerr(got['grads'][k], g, U.GRAD_FLOOR) for k, g in ref['grads'].items() if g is not None and k not in R.NOISE_ONLY)
    dtap = max(U.relerr(a, b, U.GRAD_FLOOR) for a, b in zip(got['g_tap'], ref['g_tap']))
    print('[%s/%s] loss %.6f | sat_batch_ref-vs-ref (relative): logp %.2e  losses %.2e  max grad %.2e  d tap %.2e | no gradient: %s'
          % (name, mode, ref['loss'], dl, dloss, dev, dtap, unused))
    assert max(dl, dloss, dev, dtap) < TOL, (name, mode)


def do_case(name, out, full):
    opt, params, videos = B.make_case(name)
    m = MG.build_ref(opt, params)
    for mode in ('eval', 'train'):
        ref = run_ref(m, videos, mode == 'train')
        check(name, mode, ref, B.run(opt, params, videos, mode == 'train'))
        key = '%s|%s' % (name, mode)
        out[key + '|loss'], out[key + '|losses'] = np.float64(ref['loss']), ref['losses'].astype(np.float64)
        for v in range(len(videos)):
            if full:
                out['%s|logp|%d' % (key, v)], out['%s|gtap|%d' % (key, v)] = ref['logp'][v], ref['g_tap'][v]
            else:
                for k, x in SM.summarize_logp(ref['logp'][v]).items():
                    out['%s|logp|%d|%s' % (key, v, k)] = x
                for k, x in SM.summarize_grads({'tap': ref['g_tap'][v]}).items():
                    out['%s|gtap|%d|%s' % (key, v, k.split('|', 1)[1])] = x
        if full:
            for k, g in ref['grads'].items():
                if g is not None:
                    out[key + '|grad|' + k] = g
        else:
            for k, x in SM.summarize_grads(ref['grads']).items():
                out[key + '|grad|' + k] = x
    if not full:
        return
    got = B.sample(opt, params, videos)
    share = []
    for v, vid in enumerate(videos):
        seq, slp, margin = MGS.decode(m, vid)
        ok = np.logical_and.accumulate(margin > MIN_MARGIN, axis=1)
        share.append(ok.reshape(-1))
        assert np.array_equal(got[v][0][ok], seq[ok]) and float(np.abs(got[v][1] - slp)[ok].max()) < 1e-5
        out['%s|sample|seq|%d' % (name, v)], out['%s|sample|logp|%d' % (name, v)], out['%s|sample|margin|%d' % (name, v)] = seq, slp, margin
    share = float(np.concatenate(share).mean())
    print('[%s] greedy positions resolvable at %.0e: %.3f' % (name, MIN_MARGIN, share))
    assert share >= MIN_SHARE


def main():
    out = {}
    do_case('fixture', out, True)
    do_case('widths', out, False)
    path = os.path.join(MG.GOLD, 'case_sat_batch.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == '__main__':
    main()

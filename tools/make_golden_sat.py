#!/usr/bin/env python3
"""Generate the fixtures of the one-stream decoder (caption_model='show_attend_tell', CG_num_layers 1) from the REFERENCE's own code
(build container only).

The reference's CaptionGenerator, built with the deterministic parameters of echr_amd.synth.make_sat_params, runs the cases of
synth.SAT_CASES in eval and in training mode (tap_feats a leaf; training mode under the build's Philox masks, fed through the patched
F.dropout: for this model the reference draws the event encoder's mask once, if there is an encoder, and then exactly ONE mask per step, the
[N, H] output mask) and decodes them greedily.  tests/sat_ref.py is checked against it before anything is written (1e-5 relative for
log-probs, loss, every gradient, d tap_feats).  Writes

  tests/golden/case_sat_tiny.npz   full tensors of 'sat_tiny': <mode>|logp, |loss, |grad|<parameter>, |gtap; sample|seq, |logp, |margin;
                                   state_dict|<name> = the shapes of the reference's state_dict
  tests/golden/case_sat.npz        summaries (oracle/summary.py) of the five N = 12 variants, keys '<variant>|...'; <variant>|seed = the video seed

Greedy margins: <variant>|sample|margin [N, T] is the reference's top-1 / top-2 margin at the step that chose seq[:, t].  The video seed of a
variant is the first of its SAT_CASES seed, + 1000, + 2000, ... for which at least 90 % of the decoded positions have a margin above 1e-4
(asserted); the GPU test compares indices at those positions only.

The shims and build_ref come from tools/make_golden.py, which imports the reference in place; nothing of it is copied.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_sat.py
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
import torch.nn.functional as F              # noqa: E402

from echr_amd import philox, synth           # noqa: E402
from oracle import summary as SM             # noqa: E402
from tests import sat_ref as R               # noqa: E402
from tests import util as U                  # noqa: E402

MIN_MARGIN, MIN_SHARE = 1e-4, 0.9
TOL = 1e-5
VARIANTS = ('sat_c', 'sat_e', 'sat_ve', 'sat_vec_init', 'sat_vec_eh')
assert (MG.SEED, MG.OFFSET) == (U.SEED, U.OFFSET)


class OneSiteFeeder:
    """Replaces F.dropout: the event encoder's mask first (when there is an encoder), then one output mask per step."""

    def __init__(self, encoder):
        self.calls = 0 if encoder else 1

    def __call__(self, x, p=0.5, training=True, inplace=False):
        if not training:
            return x
        site, step = (philox.SITE_TSRM, 0) if self.calls == 0 else (philox.SITE_OUT, self.calls - 1)
        self.calls += 1
        return x * torch.from_numpy(philox.scale_mask(tuple(x.shape), p, U.SEED, U.OFFSET, site, step))


def run_ref(m, vid, train_mode):
    tap = torch.from_numpy(vid['tap'].copy()).requires_grad_(True)
    c3d, lda = torch.from_numpy(vid['c3d']), torch.from_numpy(vid['lda'])
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    m.zero_grad()
    orig = F.dropout
    feeder = OneSiteFeeder(hasattr(m, 'fusion_model'))
    if train_mode:
        m.train()
        F.dropout = feeder
    else:
        m.eval()
    try:
        pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'].tolist(), mode='train')
    finally:
        F.dropout = orig
    if train_mode:          # one mask per step and nothing else
        assert feeder.calls - 1 == pred.shape[1], (feeder.calls, pred.shape)
    loss = MG.ref_utils.LanguageModelCriterion()(pred, labels[:, 1:], masks[:, 1:])
    loss.backward()
    grads = {k: (p.grad.detach().numpy().copy() if p.grad is not None else None) for k, p in m.named_parameters()}
    g_tap = tap.grad.numpy().copy() if tap.grad is not None else np.zeros_like(vid['tap'])
    return pred.detach().numpy(), float(loss), grads, g_tap


def decode(m, vid):
    """The reference's greedy decode and, from its own get_logprobs_state chain, the margin of the step that chose each position."""
    tap, c3d, lda = (torch.from_numpy(vid[k]) for k in ('tap', 'c3d', 'lda'))
    soi, ind = vid['soi'].tolist(), vid['ind']
    m.eval()
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        seq, slp = m(tap, c3d, lda, [], ind, soi, mode='eval')
        assert not isinstance(seq, list), 'nothing decoded'
        video = m.get_video_context(tap, c3d, lda, ind, soi)
        event = m.get_event_context(tap, c3d, lda, ind, soi)
        clip, mask = m.get_clip_context(tap, c3d, lda, ind, soi)
        lm = m.lm_model
        state = lm.init_hidden(video, event, clip)
        it = torch.zeros(len(soi), dtype=torch.long)
        margins = []
        for t in range(seq.shape[1]):
            lp, state = lm.get_logprobs_state(it, video, event, clip, mask, state)
            top = lp.topk(2, dim=1)
            it = top.indices[:, 0]
            margins.append((top.values[:, 0] - top.values[:, 1]).numpy())
    return seq.numpy().astype(np.int64), slp.numpy(), np.stack(margins, 1).astype(np.float32)


def check(name, mode, ref, got):
    pred, loss, grads, g_tap = ref
    opred, oloss, ograds, og_tap = got
    unused = sorted(k for k in grads if grads[k] is None)
    assert unused == sorted(k for k in ograds if ograds[k] is None), (unused, sorted(k for k in ograds if ograds[k] is None))
    dl, dloss = MG.rel(opred, pred), abs(oloss - loss) / abs(loss)
    # (d alpha_net.bias is exactly zero in real arithmetic -- the softmax is shift invariant: rounding noise on both sides, tests/util.NOISE_ONLY)
    noise = R.NOISE_ONLY
    assert all(float(np.abs(x[k]).max()) < 1e-6 for x in (grads, ograds) for k in noise if x[k] is not None)
    dev = max(U.relerr(ograds[k], grads[k], U.GRAD_FLOOR) for k in grads if grads[k] is not None and k not in noise)
    dtap = U.relerr(og_tap, g_tap, U.GRAD_FLOOR)
    print('[%s/%s] loss %.6f | sat_ref-vs-ref (relative): logp %.2e  loss %.2e  max grad %.2e  d tap %.2e | no gradient: %s'
          % (name, mode, loss, dl, dloss, dev, dtap, unused))
    assert max(dl, dloss, dev, dtap) < TOL, (name, mode)


def pick(name):
    """(opt, params, video, seed, reference model, decode) at the first seed whose greedy margins qualify."""
    base = synth.SAT_CASES[name]['video']['seed']
    for seed in range(base, base + 20000, 1000):
        opt, params, vid = synth.make_sat_case(name, video_seed=seed)
        m = MG.build_ref(opt, params)
        seq, slp, margin = decode(m, vid)
        share = float((margin > MIN_MARGIN).mean())
        print('[%s] seed %d: decoded %s, margins above %.0e: %.3f (min %.2e)' % (name, seed, seq.shape, MIN_MARGIN, share, float(margin.min())))
        if share >= MIN_SHARE:
            return opt, params, vid, seed, m, (seq, slp, margin)
    raise AssertionError('no seed of %s qualifies' % name)


def do_variant(name, out, full):
    opt, params, vid, seed, m, (seq, slp, margin) = pick(name)
    assert float((margin > MIN_MARGIN).mean()) >= MIN_SHARE
    pre = '' if full else name + '|'
    out[pre + 'seed'] = np.int64(seed)
    assert pred_rows_sum_to_one(m, vid)
    for mode in ('eval', 'train'):
        ref = run_ref(m, vid, mode == 'train')
        check(name, mode, ref, R.run(opt, params, vid, mode == 'train'))
        pred, loss, grads, g_tap = ref
        att = [k for k in grads if any(s in k for s in ('ctx2att', 'h2att', 'alpha_net'))]
        if 'C' not in opt.CG_input_feats_type:          # the attention is computed and never read
            assert all(grads[k] is None for k in att), name
        key = pre + mode
        out[key + '|loss'] = np.float64(loss)
        if full:
            out[key + '|logp'] = pred
            out[key + '|gtap'] = g_tap
            for k, g in grads.items():
                if g is not None:
                    out[key + '|grad|' + k] = g
        else:
            for k, v in SM.summarize_logp(pred).items():
                out[key + '|logp|' + k] = v
            for k, v in SM.summarize_grads(grads).items():
                out[key + '|grad|' + k] = v
            for k, v in SM.summarize_grads({'tap': g_tap}).items():
                out[key + '|gtap|' + k.split('|', 1)[1]] = v
    oseq, oslp = R.sample(opt, params, vid)
    ok = margin > MIN_MARGIN
    assert np.array_equal(oseq.numpy()[ok], seq[ok]) and float(np.abs(oslp.numpy() - slp)[ok].max()) < 1e-5
    out[pre + 'sample|seq'], out[pre + 'sample|logp'], out[pre + 'sample|margin'] = seq, slp, margin
    if full:
        for k, v in m.state_dict().items():
            out['state_dict|' + k] = np.asarray(tuple(v.shape), np.int64)


def pred_rows_sum_to_one(m, vid):
    m.eval()
    with torch.no_grad():
        pred = m(torch.from_numpy(vid['tap']), torch.from_numpy(vid['c3d']), torch.from_numpy(vid['lda']), torch.from_numpy(vid['labels']),
                 vid['ind'], vid['soi'].tolist(), mode='train')
    return bool((pred.double().exp().sum(2) - 1).abs().max() < 1e-5)


def main():
    tiny = {}
    do_variant('sat_tiny', tiny, True)
    np.savez_compressed(os.path.join(MG.GOLD, 'case_sat_tiny.npz'), **tiny)
    out = {}
    for name in VARIANTS:
        do_variant(name, out, False)
    path = os.path.join(MG.GOLD, 'case_sat.npz')
    np.savez_compressed(path, **out)
    for p in (os.path.join(MG.GOLD, 'case_sat_tiny.npz'), path):
        print('wrote %s (%d bytes)' % (p, os.path.getsize(p)))
        assert os.path.getsize(p) < 1024 * 1024


if __name__ == '__main__':
    main()

"""CPU reference of the frame-level contexts 'CH' / 'CC+CH' over a multi-video batch: tests/clipctx_ref.contexts and O.decoder_forward run
ONCE PER VIDEO under the batch's dropout slices (tests/vbatch_ref.sliced_drop), then the batch contract of tests/vbatch_ref.py --

  * log-probs per video [N_v, S_v, V1]; loss = the sum of the per-video LanguageModelCriterion (own normalisers, no 1/V);
  * parameter gradients summed over the videos; d tap per video [T_v, Ht] -- the anchors' rows ('ER2' / 'ER3'), the scene mean ('VH') and the
    attended rows together;
  * greedy and beam decodes per video (clipctx_ref.sample / beam).
"""
import numpy as np
import torch

from oracle import echr_ref_cpu as O
from tests import clipctx_ref as CR
from tests import vbatch_ref as VR


def run(opt, params, videos, train_mode, dtype=torch.float32, backward=True):
    """dict(logp=[per video], loss=sum, losses=[V], grads={name: summed gradient or None}, g_tap=[per video [T_v, Ht]])."""
    P = {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_(backward) for k, v in params.items()}
    eo = VR.offsets(videos)
    logps, losses, g_taps = [], [], []
    for v, vid in enumerate(videos):
        drop = VR.sliced_drop(opt, eo[-1], eo[v], eo[v + 1]) if train_mode else None
        tap = torch.from_numpy(np.ascontiguousarray(vid['tap'])).to(dtype).requires_grad_(backward)
        c3d, lda = (torch.from_numpy(np.ascontiguousarray(vid[k])).to(dtype) for k in ('c3d', 'lda'))
        labels = torch.from_numpy(np.ascontiguousarray(vid['labels']))
        masks = torch.from_numpy(np.ascontiguousarray(vid['masks'])).to(dtype)
        video, event, cl, mask = CR.contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi'], drop)
        logp = O.decoder_forward(P, video, event, cl, mask, labels, drop, opt.CG_init_feats_type)
        loss = O.lm_criterion(logp, labels[:, 1:], masks[:, 1:])
        if backward:
            loss.backward()          # accumulates into P[k].grad: the sum over the videos
            g_taps.append(tap.grad.numpy().copy())
        logps.append(logp.detach().numpy())
        losses.append(float(loss.detach()))
    grads = {k: (p.grad.numpy().copy() if p.grad is not None else None) for k, p in P.items()} if backward else None
    return dict(logp=logps, loss=float(np.sum(np.asarray(losses, np.float64))), losses=np.asarray(losses), grads=grads, g_tap=g_taps)


def sample(opt, params, videos):
    """Greedy decode per video (eval mode): [(seq int64 [N_v, T_v], logp)] -- ([], []) for a video that generates nothing."""
    return [CR.sample(opt, params, vid) for vid in videos]


def beam(opt, params, videos, beam_size):
    """Host beam search per video (eval mode): what clipctx_ref.beam returns, one entry per video."""
    return [CR.beam(opt, params, vid, beam_size) for vid in videos]


def e_ref(opt, params, videos, train_mode):
    """The float32-vs-float64 difference of this oracle on a case, relative to each tensor's max-norm: (max over the parameter gradients, max over
    the videos' d tap) -- the e_ref of the tests' gradient bound max(1e-5, 4 e_ref)."""
    from tests import util as U
    a, b = run(opt, params, videos, train_mode), run(opt, params, videos, train_mode, dtype=torch.float64)
    eg = max(U.relerr(a['grads'][k], b['grads'][k], U.GRAD_FLOOR) for k in a['grads'] if a['grads'][k] is not None and k not in U.NOISE_ONLY)
    et = max(U.relerr(x, y, U.GRAD_FLOOR) for x, y in zip(a['g_tap'], b['g_tap']))
    return eg, et

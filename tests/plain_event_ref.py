"""CPU oracle of the event contexts without the event encoder, 'EC' and 'EH' (CaptionGenerator.py:106-137): the pieces of
oracle/echr_ref_cpu.py composed as the reference composes them --

    event = O.event_pool(c3d, soi)   ('EC': the mean of the event's C3D rows, [N, video_dim])
    event = tap[ind]                 ('EH': the proposal encoder's state at the event's anchor, [N, hidden_dim])

then O.video_context, the clip (tests/clipctx_ref.clip: 'CC' / 'CH' / 'CC+CH') and O.decoder_forward / O.decoder_sample.  No dropout site
of an event encoder is drawn.  tap_feats is a leaf that requires grad: the loss reaches it through the anchors ('EH'), the scene mean
('VH'), the attended rows ('CH') and, through either of the first two, init_linear.  Batches: once per video, with the matching slices of the
batch's dropout masks (tests/vbatch_ref.sliced_drop), losses and gradients summed."""
import numpy as np
import torch

from oracle import echr_ref_cpu as O
from tests import beam_ref, clipctx_ref, vbatch_ref
from tests import util as U


def event(opt, tap, c3d, ind, soi):
    et = opt.event_context_type
    assert et in ('EC', 'EH'), et
    if et == 'EC':
        return O.event_pool(c3d, soi)                                                   # CaptionGenerator.py:111-115
    return tap[torch.as_tensor(np.asarray(ind), dtype=torch.long)]                       # :121-122


def contexts(opt, tap, c3d, lda, ind, soi):
    """(video, event, clip, mask) as CaptionGenerator.forward builds them (CaptionGenerator.py:17-30)."""
    video = O.video_context(lda, c3d, tap, opt.video_context_type)
    cl, mask = clipctx_ref.clip(tap, c3d, soi, opt.clip_context_type)
    return video, event(opt, tap, c3d, ind, soi), cl, mask


def _leaves(params, vid, dtype, grad):
    P = {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_(grad) for k, v in params.items()}
    tap = torch.from_numpy(np.ascontiguousarray(vid['tap']).copy()).to(dtype).requires_grad_(grad)
    c3d, lda = (torch.from_numpy(np.ascontiguousarray(vid[k])).to(dtype) for k in ('c3d', 'lda'))
    return P, tap, c3d, lda


def _tap_grad(tap):
    return tap.grad.numpy().copy() if tap.grad is not None else np.zeros(tuple(tap.shape), tap.detach().numpy().dtype)


def forward(opt, P, tap, c3d, lda, vid, drop, dtype=torch.float32, labels=None, masks=None, weights=None):
    """Teacher-forced log-probs and the criterion of one video on given leaves: (logp, loss tensor, event).  `weights` [N, S]: the
    reward-weighted criterion sum(-logp[target] * w) / sum(mask) (RewardCriterion, misc/utils.py:48-59) instead of LanguageModelCriterion."""
    labels = torch.from_numpy(np.ascontiguousarray(vid['labels'] if labels is None else labels))
    masks = torch.from_numpy(np.ascontiguousarray(vid['masks'] if masks is None else masks)).to(dtype)
    video, ev, cl, mask = contexts(opt, tap, c3d, lda, vid['ind'], vid['soi'])
    logp = O.decoder_forward(P, video, ev, cl, mask, labels, drop, opt.CG_init_feats_type)
    if weights is None:
        return logp, O.lm_criterion(logp, labels[:, 1:], masks[:, 1:]), ev
    S = logp.shape[1]
    w = torch.from_numpy(np.ascontiguousarray(weights)).to(dtype)[:, :S]
    nll = -logp.gather(2, labels[:, 1:1 + S].unsqueeze(2)).squeeze(2) * w
    return logp, nll.sum() / masks[:, 1:1 + S].sum(), ev


def run(opt, params, vid, train_mode, backward=True, dtype=torch.float32):
    """(log-probs [N,S,V1], loss, parameter gradients, d tap_feats, event context [N, De])."""
    P, tap, c3d, lda = _leaves(params, vid, dtype, backward)
    logp, loss, ev = forward(opt, P, tap, c3d, lda, vid, U.oracle_drop(opt) if train_mode else None, dtype)
    grads = g_tap = None
    if backward:
        loss.backward()
        grads = {k: (p.grad.numpy().copy() if p.grad is not None else None) for k, p in P.items()}
        g_tap = _tap_grad(tap)
    return logp.detach().numpy(), float(loss.detach()), grads, g_tap, ev.detach().numpy()


def sample(opt, params, vid):
    """Greedy OldModel.sample in eval mode: (seq int64 [N,T], logp [N,T])."""
    P, tap, c3d, lda = _leaves(params, vid, torch.float32, False)
    with torch.no_grad():
        video, ev, cl, mask = contexts(opt, tap, c3d, lda, vid['ind'], vid['soi'])
        return O.decoder_sample(P, video, ev, cl, mask, opt.CG_seq_length, opt.CG_init_feats_type)


def beam(opt, params, vid, beam_size):
    """Host beam search (tests/beam_ref.py) over this composition, eval mode."""
    P, tap, c3d, lda = _leaves(params, vid, torch.float32, False)
    with torch.no_grad():
        video, ev, cl, mask = contexts(opt, tap, c3d, lda, vid['ind'], vid['soi'])
        state0 = O.init_hidden(P, video, ev, cl, opt.CG_init_feats_type)
    step, rep_state = beam_ref.oracle_step(P, video, ev, cl, mask, beam_size)
    return beam_ref.beam_search(step, rep_state(state0), ev.shape[0], beam_size, opt.CG_seq_length)


def run_batch(opt, params, videos, train_mode, dtype=torch.float32):
    """Per video: dict(logp=[per video], loss=sum, losses=[V], grads={name: summed gradient or None}, g_tap=[per video [T_v, Ht]])."""
    P = {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_(True) for k, v in params.items()}
    eo = vbatch_ref.offsets(videos)
    logps, losses, g_taps = [], [], []
    for v, vid in enumerate(videos):
        _, tap, c3d, lda = _leaves({}, vid, dtype, True)
        drop = vbatch_ref.sliced_drop(opt, eo[-1], eo[v], eo[v + 1]) if train_mode else None
        logp, loss, _ = forward(opt, P, tap, c3d, lda, vid, drop, dtype)
        loss.backward()          # accumulates into P[k].grad: the sum over the videos
        g_taps.append(_tap_grad(tap))
        logps.append(logp.detach().numpy())
        losses.append(float(loss.detach()))
    grads = {k: (p.grad.numpy().copy() if p.grad is not None else None) for k, p in P.items()}
    return dict(logp=logps, loss=float(np.sum(np.asarray(losses, np.float64))), losses=np.asarray(losses), grads=grads, g_tap=g_taps)

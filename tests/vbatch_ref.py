"""CPU reference of the multi-video batch contract (echr_amd/batch.py): oracle/echr_ref_cpu.py run ONCE PER VIDEO, then

  * log-probs: per video, [N_v, S_v, V1] (the batched output's rows of video v, cut to the video's own step count);
  * loss = sum over the videos of LanguageModelCriterion of video v (each with its own normaliser; no 1/V), and the per-video losses;
  * gradients = the sum over the videos (the reference's m_batch accumulation, train.py:281-283,313-317); `step` applies
    clamp_adam_step ONCE to the sum;
  * training mode: video v is fed the matching SLICES of the batch's dropout masks -- rows [e0:e1] of the [N_tot, H] sites,
    [e0:e1, :, e0:e1] of the event encoder's [N_tot, G, N_tot] site -- generated with echr_amd/philox.py for the batch-global shapes.
"""
import numpy as np
import torch

from oracle import echr_ref_cpu as O
from tests import util as U


def offsets(videos):
    eo = [0]
    for v in videos:
        eo.append(eo[-1] + len(v['soi']))
    return eo


def sliced_drop(opt, n_tot, e0, e1):
    """The oracle's `drop` callable for the events [e0, e1) of a batch of n_tot events."""
    base = U.oracle_drop(opt)

    def drop(site, step, shape):
        if site == 'tsrm':
            return base(site, step, (n_tot, shape[1], n_tot))[e0:e1, :, e0:e1].contiguous()
        return base(site, step, (n_tot, shape[1]))[e0:e1].contiguous()
    return drop


def run_video(opt, P, vid, drop, dtype=torch.float32, backward=True, tap_grad=True):
    """One video through the oracle: (log-probs, loss tensor, tap leaf)."""
    tap = torch.from_numpy(np.ascontiguousarray(vid['tap'])).to(dtype).requires_grad_(backward and tap_grad)
    c3d, lda = (torch.from_numpy(np.ascontiguousarray(vid[k])).to(dtype) for k in ('c3d', 'lda'))
    labels = torch.from_numpy(np.ascontiguousarray(vid['labels']))
    masks = torch.from_numpy(np.ascontiguousarray(vid['masks'])).to(dtype)
    logp = O.caption_forward(P, tap, c3d, lda, labels, vid['ind'], vid['soi'], 'train', drop, opt.n_head,
                             video_context_type=opt.video_context_type, event_context_type=opt.event_context_type,
                             fST_type=getattr(opt, 'fST_type', 'fST0'), use_posit=opt.use_posit, init_feats_type=opt.CG_init_feats_type)
    loss = O.lm_criterion(logp, labels[:, 1:], masks[:, 1:])
    return logp, loss, tap


def run(opt, params, videos, train_mode, dtype=torch.float32, backward=True):
    """dict(logp=[per video [N_v,S_v,V1]], loss=sum, losses=[V], grads={name: summed gradient or None}, g_tap=[per video [T_v,Ht]])."""
    P = {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_(backward) for k, v in params.items()}
    eo = offsets(videos)
    logps, losses, g_taps = [], [], []
    for v, vid in enumerate(videos):
        drop = sliced_drop(opt, eo[-1], eo[v], eo[v + 1]) if train_mode else None
        logp, loss, tap = run_video(opt, P, vid, drop, dtype, backward)
        if backward:
            loss.backward()          # accumulates into P[k].grad: the sum over the videos
            g_taps.append(tap.grad.numpy().copy() if tap.grad is not None else np.zeros(tuple(tap.shape), np.float64 if dtype == torch.float64 else np.float32))
        logps.append(logp.detach().numpy())
        losses.append(float(loss.detach()))
    grads = {k: (p.grad.numpy().copy() if p.grad is not None else None) for k, p in P.items()} if backward else None
    return dict(logp=logps, loss=float(np.sum(np.asarray(losses, np.float64))), losses=np.asarray(losses), grads=grads, g_tap=g_taps)


def step(params, grads, lr=1e-3, clip=100.0, step_no=1):
    """ONE clamp + Adam update on the summed gradient from zero moments: (params', m, v) as float32 dicts (never-used parameters untouched)."""
    out, ms, vs = {}, {}, {}
    for k, p in params.items():
        p = p.astype(np.float32).copy()
        m, v = np.zeros_like(p), np.zeros_like(p)
        if grads[k] is not None:
            O.clamp_adam_step(p, grads[k].astype(np.float32), m, v, step_no, lr, clip=clip)
        out[k], ms[k], vs[k] = p, m, v
    return out, ms, vs


def sample(opt, params, videos):
    """Greedy decode per video (eval mode): [(seq int64 [N_v,T_v], logp)] -- ([], []) for a video that generates nothing."""
    P = {k: torch.from_numpy(v.copy()) for k, v in params.items()}
    out = []
    with torch.no_grad():
        for vid in videos:
            tap, c3d, lda = (torch.from_numpy(np.ascontiguousarray(vid[k])) for k in ('tap', 'c3d', 'lda'))
            out.append(O.caption_forward(P, tap, c3d, lda, None, vid['ind'], vid['soi'], 'eval', None, opt.n_head, seq_length=opt.CG_seq_length,
                                         video_context_type=opt.video_context_type, event_context_type=opt.event_context_type,
                                         fST_type=getattr(opt, 'fST_type', 'fST0'), use_posit=opt.use_posit))
    return out


def stack_sample(per_video, videos):
    """The batched decode's `seq` from the per-video ones: int64 [N_tot, T] with T the longest video's length; a video that stopped earlier
    has every row finished from there on (zeros), as OldModel.sample pads finished rows (OldModel_NEW.py:171-183)."""
    eo = offsets(videos)
    T = max([int(s.shape[1]) for s, _ in per_video if not isinstance(s, list)] or [0])
    seq = np.zeros((eo[-1], T), np.int64)
    for v, (s, _) in enumerate(per_video):
        if not isinstance(s, list):
            seq[eo[v]:eo[v + 1], :s.shape[1]] = s.numpy()
    return seq

"""CPU reference of the non-zero initial decoder state (CG_init_feats_type) over a multi-video batch: the oracle run ONCE PER VIDEO with
`init_feats_type` under the batch's dropout slices (tests/vbatch_ref.sliced_drop), then the batch contract of tests/vbatch_ref.py --

  * log-probs per video [N_v, S_v, V1]; loss = the sum of the per-video LanguageModelCriterion (own normalisers, no 1/V);
  * parameter gradients summed over the videos, `lm_model.init_linear.*` included; d tap per video [T_v, Ht];
  * greedy and beam decodes per video that start from the video's own initial state (tests/vbatch_ref.sample does not pass it).

Every video is its own oracle call, so `clip.mean(1)` runs over the padded slots of THAT video's clip tensor: the divisor is the video's
longest event.  `run(..., batch_wide_divisor=True)` is the wrong variant -- every clip tensor padded to the batch's longest event -- that the
host test uses to show the cases can tell the two apart.  The per-video composition itself is tests/clip_batch_ref.py's (it passes
opt.CG_init_feats_type to the oracle for any frame-level context); this module adds the divisor variant and the error measure.
"""
import numpy as np
import torch

from oracle import echr_ref_cpu as O
from tests import clip_batch_ref as CB
from tests import clipctx_ref as CR
from tests import vbatch_ref as VR

step = VR.step
stack_sample = VR.stack_sample
offsets = VR.offsets


def video_max_len(videos):
    """The padded clip length of every video: its longest event (int64 [V])."""
    return np.asarray([int((np.asarray(v['soi'])[:, 1] - np.asarray(v['soi'])[:, 0]).max()) for v in videos], np.int64)


def run(opt, params, videos, train_mode, dtype=torch.float32, backward=True, batch_wide_divisor=False):
    """dict(logp=[per video], loss=sum, losses=[V], grads={name: summed gradient or None}, g_tap=[per video [T_v, Ht]])."""
    if not batch_wide_divisor:
        return CB.run(opt, params, videos, train_mode, dtype, backward)
    A_max = int(video_max_len(videos).max())
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
        pad = A_max - cl.shape[1]          # masked-out zero slots: the attention is unchanged, clip.mean(1) divides by A_max
        cl = torch.cat([cl, cl.new_zeros(cl.shape[0], pad, cl.shape[2])], 1)
        mask = torch.cat([mask, mask.new_zeros(mask.shape[0], pad)], 1)
        logp = O.decoder_forward(P, video, event, cl, mask, labels, drop, opt.CG_init_feats_type)
        loss = O.lm_criterion(logp, labels[:, 1:], masks[:, 1:])
        if backward:
            loss.backward()
            g_taps.append(tap.grad.numpy().copy() if tap.grad is not None else np.zeros(tuple(tap.shape), np.float32))
        logps.append(logp.detach().numpy())
        losses.append(float(loss.detach()))
    grads = {k: (p.grad.numpy().copy() if p.grad is not None else None) for k, p in P.items()} if backward else None
    return dict(logp=logps, loss=float(np.sum(np.asarray(losses, np.float64))), losses=np.asarray(losses), grads=grads, g_tap=g_taps)


def sample(opt, params, videos):
    """Greedy decode per video from its own initial state (eval mode): [(seq int64 [N_v, T_v], logp)] -- ([], []) for an empty decode."""
    return [CR.sample(opt, params, vid) for vid in videos]


def beam(opt, params, videos, beam_size):
    """Host beam search per video from its own initial state (eval mode): what clipctx_ref.beam returns, one entry per video."""
    return [CR.beam(opt, params, vid, beam_size) for vid in videos]


def e_ref(opt, params, videos, train_mode):
    """The float32-vs-float64 difference of this oracle on a case, relative to each tensor's max-norm: (max over the parameter gradients,
    max over the videos' d tap) -- the e_ref of the tests' gradient bound max(1e-5, 4 e_ref)."""
    return CB.e_ref(opt, params, videos, train_mode)


def greedy_margin(opt, params, videos):
    """The smallest top-1 / top-2 log-prob margin over every decoded step of every unfinished row of the oracle's own greedy decodes (eval
    mode, per video): a case whose margin exceeds the log-prob tolerance has ONE right token sequence."""
    P = {k: torch.from_numpy(v.copy()) for k, v in params.items()}
    margin = np.inf
    with torch.no_grad():
        for vid in videos:
            tap, c3d, lda = (torch.from_numpy(vid[k]) for k in ('tap', 'c3d', 'lda'))
            video, event, cl, mask = CR.contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi'])
            N = event.shape[0]
            state = O.init_hidden(P, video, event, cl, opt.CG_init_feats_type)
            it = torch.zeros(N, dtype=torch.long)
            alive = torch.ones(N, dtype=torch.bool)
            for t in range(opt.CG_seq_length):
                logprobs, state = O.logprobs_state(P, it, video, event, cl, mask, state)
                top = torch.topk(logprobs, 2, 1).values
                if alive.any():
                    margin = min(margin, float((top[:, 0] - top[:, 1])[alive].min()))
                it = torch.max(logprobs, 1)[1]
                alive = alive & (it > 0)
                if not alive.any():
                    break
                it = it * alive.type_as(it)
    return margin

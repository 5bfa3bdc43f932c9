"""CPU oracle of the frame-level contexts 'CH' and 'CC+CH' (CaptionGenerator.py:140-167): the pieces of oracle/echr_ref_cpu.py composed with
the clip built over the proposal encoder's states -- clip_context(tap, soi) for 'CH', the C3D and tap clips concatenated on the feature axis
(C3D first) for 'CC+CH'.  tap_feats may be a leaf that requires grad: the loss then reaches it through the event context ('ER2' / 'ER3'),
the scene mean ('VH') and the attended clip."""
import torch

from oracle import echr_ref_cpu as O
from tests import beam_ref
from tests import util as U


def clip(tap, c3d, soi, clip_context_type):
    parts = []
    if 'CC' in clip_context_type:
        parts.append(O.clip_context(c3d, soi))
    if 'CH' in clip_context_type:
        parts.append(O.clip_context(tap, soi))
    if len(parts) == 1:
        return parts[0]
    return torch.cat([parts[0][0], parts[1][0]], 2), parts[0][1]


def contexts(opt, P, tap, c3d, lda, ind, soi, drop=None):
    """(video, event, clip, mask) as CaptionGenerator.forward builds them (CaptionGenerator.py:17-30)."""
    video = O.video_context(lda, c3d, tap, opt.video_context_type)
    dmask = drop('tsrm', 0, (len(soi), opt.n_head, len(soi))) if drop is not None else None
    event = O.event_context(P, tap, c3d, ind, soi, opt.n_head, dmask, opt.event_context_type, getattr(opt, 'fST_type', 'fST0'), opt.use_posit)
    cl, mask = clip(tap, c3d, soi, opt.clip_context_type)
    return video, event, cl, mask


def run(opt, params, vid, train_mode, backward=True, dtype=torch.float32):
    """Teacher-forced pass + LanguageModelCriterion (and its backward): (log-probs [N,S,V1], loss, parameter gradients, d tap_feats)."""
    P = {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_(backward) for k, v in params.items()}
    tap = torch.from_numpy(vid['tap'].copy()).to(dtype).requires_grad_(backward)
    c3d, lda = (torch.from_numpy(vid[k]).to(dtype) for k in ('c3d', 'lda'))
    labels = torch.from_numpy(vid['labels'])
    masks = torch.from_numpy(vid['masks']).to(dtype)
    drop = U.oracle_drop(opt) if train_mode else None
    video, event, cl, mask = contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi'], drop)
    logp = O.decoder_forward(P, video, event, cl, mask, labels, drop, opt.CG_init_feats_type)
    loss = O.lm_criterion(logp, labels[:, 1:], masks[:, 1:])
    grads = g_tap = None
    if backward:
        loss.backward()
        grads = {k: (p.grad.numpy().copy() if p.grad is not None else None) for k, p in P.items()}
        g_tap = tap.grad.numpy().copy()
    return logp.detach().numpy(), float(loss.detach()), grads, g_tap


def sample(opt, params, vid):
    """Greedy OldModel.sample in eval mode: (seq int64 [N,T], logp [N,T])."""
    P = {k: torch.from_numpy(v.copy()) for k, v in params.items()}
    tap, c3d, lda = (torch.from_numpy(vid[k]) for k in ('tap', 'c3d', 'lda'))
    with torch.no_grad():
        video, event, cl, mask = contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi'])
        return O.decoder_sample(P, video, event, cl, mask, opt.CG_seq_length, opt.CG_init_feats_type)


def beam(opt, params, vid, beam_size):
    """Host beam search (tests/beam_ref.py) over the clip-context oracle, eval mode."""
    P = {k: torch.from_numpy(v.copy()) for k, v in params.items()}
    tap, c3d, lda = (torch.from_numpy(vid[k]) for k in ('tap', 'c3d', 'lda'))
    with torch.no_grad():
        video, event, cl, mask = contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi'])
        state0 = O.init_hidden(P, video, event, cl, opt.CG_init_feats_type)
    step, rep_state = beam_ref.oracle_step(P, video, event, cl, mask, beam_size)
    return beam_ref.beam_search(step, rep_state(state0), event.shape[0], beam_size, opt.CG_seq_length)

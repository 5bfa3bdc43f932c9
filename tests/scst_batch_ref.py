"""CPU reference of self-critical training over a multi-video batch (CaptionGenerator.train_rl_batch, fused.SelfCriticalBatchStep):
oracle/echr_ref_cpu.py run ONCE PER VIDEO on that video's own sample, as the reference's m_batch = V protocol does, then

  * contexts: the training-mode event context of video v under the matching SLICES of the batch's dropout masks (tests/vbatch_ref.py);
  * sample_logprobs of video v: the teacher-forced decoder on [0 | gen_v | 0] under the sliced masks, gathered at gen_v [N_v, T_v] -- what
    the reference's sampling loop emits at those tokens under those masks;
  * greedy baseline of video v: the eval-mode decode on the same event context;
  * loss = sum over the videos of RewardCriterion of video v (misc/utils.py:48-59: mask [1 | gen_v > 0][:, :-1], its own normaliser, no
    epsilon, no 1/V); a video whose sample is empty contributes nothing;
  * gradients = the sum over the videos.
"""
import numpy as np
import torch

from oracle import echr_ref_cpu as O
from tests import vbatch_ref as VR


def reward_loss(slp, gen, reward):
    """RewardCriterion.forward on one video's tensors [N_v, T_v]."""
    mask = (gen > 0).to(slp.dtype)
    mask = torch.cat([mask.new_ones(mask.shape[0], 1), mask[:, :-1]], 1)
    return torch.sum(-slp * reward.to(slp.dtype) * mask) / torch.sum(mask)


def run_video(opt, P, vid, gen, reward, drop, dtype=torch.float32):
    """One video: (sample_logprobs [N_v,T_v] with graph or None, greedy seq or [], loss tensor or None)."""
    tap, c3d, lda = (torch.from_numpy(np.ascontiguousarray(vid[k])).to(dtype) for k in ('tap', 'c3d', 'lda'))
    soi, ind = vid['soi'], vid['ind']
    N = len(soi)
    video = O.video_context(lda, c3d, tap, opt.video_context_type)
    event = O.event_context(P, tap, c3d, ind, soi, opt.n_head, drop('tsrm', 0, (N, opt.n_head, N)), opt.event_context_type,
                            getattr(opt, 'fST_type', 'fST0'), opt.use_posit)
    clip, mask = O.clip_context(c3d, soi)
    with torch.no_grad():
        greedy, _ = O.decoder_sample(P, video, event, clip, mask, opt.CG_seq_length)
    gen = torch.as_tensor(np.asarray(gen, dtype=np.int64))
    T = gen.shape[1]
    if T == 0:
        return None, greedy, None
    labels = torch.zeros(N, T + 2, dtype=torch.int64)
    labels[:, 1:T + 1] = gen
    logp = O.decoder_forward(P, video, event, clip, mask, labels, drop)          # [N, T+1, V1]
    slp = logp[:, :T].gather(2, gen.unsqueeze(2)).squeeze(2)
    return slp, greedy, reward_loss(slp, gen, torch.as_tensor(np.asarray(reward, dtype=np.float32)))


def run(opt, params, videos, gens, rewards, dtype=torch.float32):
    """gens / rewards: per video [N_v, T_v] (T_v = 0: an empty sample).  dict(slp=[per video], greedy=[per video int64 [N_v,T']],
    losses=[V], loss=sum, grads={name: summed gradient or None})."""
    P = {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_(True) for k, v in params.items()}
    eo = VR.offsets(videos)
    slps, greedys, losses = [], [], []
    for v, vid in enumerate(videos):
        slp, greedy, loss = run_video(opt, P, vid, gens[v], rewards[v], VR.sliced_drop(opt, eo[-1], eo[v], eo[v + 1]), dtype)
        n = len(vid['soi'])
        greedys.append(np.zeros((n, 0), np.int64) if isinstance(greedy, list) else greedy.numpy().astype(np.int64))
        if loss is None:
            slps.append(np.zeros((n, 0), np.float32))
            losses.append(0.0)
            continue
        loss.backward()          # accumulates into P[k].grad: the sum over the videos
        slps.append(slp.detach().numpy())
        losses.append(float(loss.detach()))
    grads = {k: (p.grad.numpy().copy() if p.grad is not None else None) for k, p in P.items()}
    return dict(slp=slps, greedy=greedys, losses=np.asarray(losses), loss=float(np.sum(np.asarray(losses, np.float64))), grads=grads)


def stack(per_video, videos, dtype):
    """Per-video [N_v, T_v] arrays as one zero-padded [N_tot, max T_v] array (the batched layout)."""
    eo = VR.offsets(videos)
    T = max(int(a.shape[1]) for a in per_video)
    out = np.zeros((eo[-1], T), dtype)
    for v, a in enumerate(per_video):
        out[eo[v]:eo[v + 1], :a.shape[1]] = a
    return out


def load_fixture(g, V):
    """(gens, slps, greedys, rewards, losses) per video from tests/golden/case_scst_batch.npz."""
    pick = lambda name: [g['%s|v%02d' % (name, v)] for v in range(V)]
    return pick('gen_result'), pick('sample_logprobs'), pick('greedy_res'), pick('reward'), g['losses']

"""The criterion arrays of the self-critical steps as the two steps formed them before echr_amd.batch.sampled_criterion: the formulas of
fused.SelfCriticalStep.__call__ and of VideoBatch.reward_weights (with VideoBatch._reward_matrix) at that commit, copied verbatim apart
from the names of their inputs -- tests/test_sampled_criterion_host.py asserts bit equality with them -- and an independent float64
statement of RewardCriterion (misc/utils.py:48-59) per group of rows."""
import numpy as np


def single_step_arrays(gen_h, reward):
    """SelfCriticalStep.__call__: gen_h int64 [N, T] (host), reward [N] or [N, T].  (labels, mask, w, r)."""
    N, T = gen_h.shape
    r = np.asarray(reward, dtype=np.float32)
    if r.ndim == 1:
        r = np.repeat(r[:, None], T, 1)
    if r.shape != (N, T):
        raise ValueError('reward must be [N, T] or [N] (got %s for gen_result %s)' % (r.shape, (N, T)))
    g = gen_h
    labels = np.zeros((N, T + 2), dtype=np.int64)
    labels[:, 1:T + 1] = g
    mask = np.zeros((N, T + 1), dtype=np.float32)
    mask[:, 0] = 1.0
    mask[:, 1:T] = g[:, :T - 1] > 0
    w = np.zeros((N, T + 1), dtype=np.float32)
    w[:, :T] = r * mask[:, :T]
    return labels, mask, w, r


def _reward_matrix(reward, N, T):
    r = np.asarray(reward, np.float32)
    if r.ndim == 1:
        r = np.repeat(r[:, None], T, 1)
    if r.shape[0] != N or r.ndim != 2 or r.shape[1] < T:
        raise ValueError('reward must be [N_tot, T] or [N_tot] (got %s for gen_result %s)' % (r.shape, (N, T)))
    return r[:, :T]


def batch_step_arrays(gen_result, reward, video_words, event_slices):
    """VideoBatch.reward_weights: (labels, mask, w)."""
    g = np.asarray(gen_result, np.int64)
    vw = np.asarray(video_words, dtype=np.int64).reshape(-1)
    T = int(vw.max()) if len(vw) else 0
    if T > g.shape[1]:
        raise ValueError('video_words %s exceed gen_result %s' % (vw.tolist(), g.shape))
    g = g[:, :T]
    N = g.shape[0]
    r = _reward_matrix(reward, N, T)
    labels = np.zeros((N, T + 2), np.int64)
    labels[:, 1:T + 1] = g
    mask = np.zeros((N, T + 1), np.float32)
    w = np.zeros((N, T + 1), np.float32)
    for s, wv in zip(event_slices, vw.tolist()):
        if wv == 0:
            continue
        mask[s, 0] = 1.0
        mask[s, 1:wv] = g[s, :wv - 1] > 0
        w[s, :wv] = r[s, :wv] * mask[s, :wv] / mask[s, :wv].sum(dtype=np.float32)
    return labels, mask, w


def reward_criterion(logp, gen, reward):
    """RewardCriterion on one group's own tensors [N_v, T_v] in float64: (loss, its mask [1 | gen > 0][:, :-1])."""
    gen = np.asarray(gen)
    mask = np.concatenate([np.ones((gen.shape[0], 1)), (gen > 0)[:, :-1].astype(np.float64)], 1)
    return float((-np.asarray(logp, np.float64) * np.asarray(reward, np.float64) * mask).sum() / mask.sum()), mask

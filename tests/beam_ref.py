"""Host beam search: the rules of echr_decoder_beam (include/echr_hip.h) over a step callback, scores accumulated in float64.

step(it LongTensor [N*B], state) -> (log-probs [N*B, V1], state'); row n*B + j is slot j of event n.  permute(state, idx) gives the
state whose row r is row idx[r] of `state` (default: a tuple of tensors indexed on dim 1, the oracle's (h, c) [3, rows, H]).

Besides the result, every event's `margin`: the smallest gap, over its steps, between the B-th kept and the best dropped candidate,
and between its best and runner-up finished hypotheses -- the room a float32 decode has before it may legitimately choose differently."""
import numpy as np
import torch


def _permute_dim1(state, idx):
    ix = torch.as_tensor(idx, dtype=torch.long)
    return tuple(s.index_select(1, ix) for s in state)


def beam_search(step, state, N, B, L, permute=_permute_dim1):
    M = N * B
    it = np.zeros(M, np.int64)
    alive = np.zeros((N, B), bool)
    alive[:, 0] = True
    score = np.zeros((N, B))
    htok = np.zeros((N, B, L), np.int64)
    hlp = np.zeros((N, B, L))
    best = [None] * N                     # (score, words, tokens [L], log-probs [L])
    finished = [[] for _ in range(N)]
    margin = np.full(N, np.inf)
    for t in range(L):
        if not alive.any():
            break
        lp, state = step(torch.from_numpy(it), state)
        lp = lp.detach().double().cpu().numpy().reshape(N, B, -1)
        V1 = lp.shape[2]
        parent = np.tile(np.arange(B), (N, 1))
        nit = it.reshape(N, B).copy()
        for n in range(N):
            if not alive[n].any():
                continue
            js = np.nonzero(alive[n])[0]
            flat = (score[n, js][:, None] + lp[n, js]).ravel()          # (slot, token) order: a stable sort keeps the tie rule
            order = np.argsort(-flat, kind='stable')
            if len(order) > B:
                margin[n] = min(margin[n], flat[order[B - 1]] - flat[order[B]])
            ntok, nlp = htok[n].copy(), hlp[n].copy()
            for k in range(B):
                q = order[k]
                j, v = js[q // V1], int(q % V1)
                c = flat[q]
                ntok[k, :t], nlp[k, :t] = htok[n, j, :t], hlp[n, j, :t]
                ntok[k, t], nlp[k, t] = v, lp[n, j, v]
                fin = v == 0 or t == L - 1
                if fin:
                    finished[n].append(c)
                    if best[n] is None or c > best[n][0]:
                        best[n] = (c, t if v == 0 else L, ntok[k].copy(), nlp[k].copy())
                score[n, k] = c
                alive[n, k] = not fin
                parent[n, k] = j
                nit[n, k] = v
            htok[n], hlp[n] = ntok, nlp
        it = nit.reshape(M)
        idx = (np.arange(N)[:, None] * B + parent).reshape(M)
        state = permute(state, idx)
    words = np.array([b[1] for b in best], np.int64)
    T = int(words.max())
    seq = np.zeros((N, T), np.int64)
    logp = np.zeros((N, T))
    for n, (c, w, tok, lps) in enumerate(best):
        seq[n, :w] = tok[:w]
        m = min(w + 1, T)
        logp[n, :m] = lps[:m]
        fs = sorted(finished[n], reverse=True)
        if len(fs) > 1:
            margin[n] = min(margin[n], fs[0] - fs[1])
    return dict(seq=seq, logp=logp, score=np.array([b[0] for b in best]), words=words, margin=margin)


def rescore(step, state, seq, L):
    """Sum of the token log-probs of given captions seq [N, T] (words, then zeros), <eos> included when a caption ends inside L steps:
    the teacher-forced decode of [0 | words | 0]."""
    seq = np.asarray(seq)
    N = seq.shape[0]
    T = seq.shape[1] if seq.ndim == 2 else 0
    words = np.array([int(np.argmax(r == 0)) if (r == 0).any() else T for r in seq], np.int64) if T else np.zeros(N, np.int64)
    total = np.zeros(N)
    it = np.zeros(N, np.int64)
    for t in range(min(int(words.max()) + 1, L)):
        lp, state = step(torch.from_numpy(it), state)
        lp = lp.detach().double().cpu().numpy()
        tok = np.array([seq[n, t] if t < words[n] else 0 for n in range(N)], np.int64)
        for n in range(N):
            if t <= words[n] and t < L:
                total[n] += lp[n, tok[n]]
        it = tok
    return total, words


def oracle_contexts(opt, params, vid, soi=None, ind=None):
    """(P, video, event, clip, mask, state0) of the CPU oracle for a fixture (CaptionGenerator.forward in eval mode up to the decoder)."""
    from oracle import echr_ref_cpu as O
    P = {k: torch.from_numpy(v) for k, v in params.items()}
    tap, c3d, lda = (torch.from_numpy(vid[k]) for k in ('tap', 'c3d', 'lda'))
    soi = vid['soi'] if soi is None else soi
    ind = vid['ind'] if ind is None else ind
    with torch.no_grad():
        video = O.video_context(lda, c3d, tap, opt.video_context_type)
        event = O.event_context(P, tap, c3d, ind, soi, opt.n_head, None, opt.event_context_type, getattr(opt, 'fST_type', 'fST0'),
                                opt.use_posit)
        clip, mask = O.clip_context(c3d, soi)
        state0 = O.init_hidden(P, video, event, clip, opt.CG_init_feats_type)
    return P, video, event, clip, mask, state0


def oracle_step(P, video, event, clip, mask, B):
    """(step, state-replicator) over B event-major copies of every event for beam_search / rescore."""
    from oracle import echr_ref_cpu as O
    rep = lambda x: x.repeat_interleave(B, dim=0)
    ev, cl, mk = rep(event), rep(clip), rep(mask)

    def step(it, state):
        with torch.no_grad():
            return O.logprobs_state(P, it, video, ev, cl, mk, state)
    return step, (lambda st: tuple(s.repeat_interleave(B, dim=1) for s in st))


def oracle_beam(opt, params, vid, B, soi=None, ind=None):
    P, video, event, clip, mask, state0 = oracle_contexts(opt, params, vid, soi, ind)
    step, rep_state = oracle_step(P, video, event, clip, mask, B)
    return beam_search(step, rep_state(state0), event.shape[0], B, opt.CG_seq_length)


def oracle_rescore(opt, params, vid, seq, soi=None, ind=None):
    P, video, event, clip, mask, state0 = oracle_contexts(opt, params, vid, soi, ind)
    step, _ = oracle_step(P, video, event, clip, mask, 1)
    return rescore(step, state0, seq, opt.CG_seq_length)

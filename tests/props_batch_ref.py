"""CPU statement of the batched evaluation contract: the oracle's pieces, run once per video.

  * select(): oracle.top_proposals / top_proposals_nms on every video's own rows (n, k local to the video), then the layout of
    echr_top_proposals_batch / _nms_batch -- lists concatenated in video order, event_offset, vid, the batch-absolute copies
    (+ row_offset[vid]) and count [V+2] = picks per video, their total, the largest interval length;
  * caption_flow(): eval_utils.caption_videos' flow for one video -- selection on given scores -> the oracle's greedy captions -> the
    records of result.json -- as tests/test_gpu_parity.py::test_eval_flow_sst_to_captions_vs_oracle builds it, plus the smallest
    top-1 / top-2 margin of the oracle's log-probs over every decoded position.
"""
import numpy as np
import torch

from oracle import echr_ref_cpu as O


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def causal_mask(lengths, K):
    """[T_tot, K] float32: n_local >= k for every video."""
    return np.concatenate([(np.arange(T)[:, None] >= np.arange(K)[None, :]).astype(np.float32) for T in lengths], 0)


def select(scores, ro, topN, val_thres=0.0, overlap=0.0, mask=None):
    """dict(count [V+2], event_offset [V+1], vid, ind, ind_abs [N], feat, feat_abs [N,2] -- all int64 -- and conf float32 [N]).
    overlap != 0: greedy NMS; else the score threshold under `mask` (None: the causal mask)."""
    scores = np.asarray(scores, np.float32)
    V, K = len(ro) - 1, scores.shape[1]
    cnt, vid, ind, feat, conf, ind_abs, feat_abs = [], [], [], [], [], [], []
    for v in range(V):
        a, b = int(ro[v]), int(ro[v + 1])
        sc = scores[a:b]
        if overlap != 0:
            _, props, c = O.top_proposals_nms(sc, overlap, topN)
            props = np.asarray(props, np.int64).reshape(-1, 2)
            i, f = props[:, 1] - 1, props
        else:
            m = causal_mask([b - a], K) if mask is None else np.asarray(mask, np.float32)[a:b]
            i, f, c = O.top_proposals(sc, m, topN, val_thres)
            i, f = np.asarray(i, np.int64).reshape(-1), np.asarray(f, np.int64).reshape(-1, 2)
        cnt.append(len(i)); vid.append(np.full(len(i), v, np.int64)); ind.append(i); feat.append(f)
        conf.append(np.asarray(c, np.float64).astype(np.float32).reshape(-1)); ind_abs.append(i + a); feat_abs.append(f + a)
    feat = np.concatenate(feat, 0)
    maxlen = int((feat[:, 1] - feat[:, 0]).max()) if len(feat) else 0
    return dict(count=np.array(cnt + [sum(cnt), maxlen], np.int64), event_offset=offsets(cnt), vid=np.concatenate(vid), ind=np.concatenate(ind),
                feat=feat, ind_abs=np.concatenate(ind_abs), feat_abs=np.concatenate(feat_abs, 0), conf=np.concatenate(conf))


def greedy_with_margin(P, tap, c3d, lda, ind, soi, opt):
    """oracle.caption_forward(mode='eval') step by step: (seq int64 [N,T], logp [N,T], smallest top-1 / top-2 margin over all rows and
    decoded steps) -- ([], [], inf) when the first step ends every row."""
    with torch.no_grad():
        video = O.video_context(lda, c3d, tap, opt.video_context_type)
        event = O.event_context(P, tap, c3d, ind, soi, opt.n_head, None, opt.event_context_type, getattr(opt, 'fST_type', 'fST0'), opt.use_posit)
        clip, mask = O.clip_context(c3d, soi)
        N = event.shape[0]
        state = O.init_hidden(P, video, event, clip, opt.CG_init_feats_type)
        seq, slp, margin = [], [], np.inf
        logprobs = unfinished = None
        for t in range(opt.CG_seq_length + 1):
            if t == 0:
                it = torch.zeros(N, dtype=torch.long)
            else:
                top = logprobs.topk(2, dim=1)
                sample_lp, it = torch.max(logprobs, 1)
                step_margin = float((top.values[:, 0] - top.values[:, 1]).min())
            logprobs, state = O.logprobs_state(P, it, video, event, clip, mask, state)
            if t >= 1:
                margin = min(margin, step_margin)          # (the step that ends the video decides <eos> against the runner-up: counted too)
                unfinished = (it > 0) if t == 1 else unfinished & (it > 0)
                if int(unfinished.sum()) == 0:
                    break
                seq.append(it * unfinished.type_as(it)); slp.append(sample_lp)
    if not seq:
        return [], [], margin
    return torch.stack(seq, 1).numpy(), torch.stack(slp, 1).numpy(), margin


def caption_flow(opt, P, scores, tap, c3d, lda, duration, f2t, topN, nms_threshold=0.0, val_score_thres=0.0, flag_eval_what='tap_cg', given=None):
    """One video through caption_videos' flow on the host.  `scores` [T,K] / `tap` [T,H]: the proposal encoder's outputs the selection and the
    captions read (the device's own: selection is discontinuous in them); `given` = (ind, soi, timestamps) for flag_eval_what='cg'.
    Returns dict(info = the records, ind, soi, conf, seq, logp, margin)."""
    T = c3d.shape[0]
    if flag_eval_what == 'cg':
        ind, soi, stamps = given
        ind, soi = np.asarray(ind, np.int64).tolist(), np.asarray(soi, np.int64).reshape(-1, 2).tolist()
        conf = [1] * len(ind)
    else:
        sel = select(scores, [0, T], topN, val_score_thres, nms_threshold)
        ind, soi, conf = sel['ind'].tolist(), sel['feat'].tolist(), sel['conf'].tolist()
        stamps = [f2t(s, e, T, duration) for s, e in soi]
    out = dict(info=[], ind=ind, soi=soi, conf=conf, seq=[], logp=[], margin=np.inf)
    if not ind:
        return out
    if flag_eval_what == 'tap':
        sents, score = [0] * len(ind), [0] * len(ind)
    else:
        seq, lp, out['margin'] = greedy_with_margin(P, torch.as_tensor(tap), torch.as_tensor(c3d), torch.as_tensor(lda), ind, soi, opt)
        if len(seq) == 0:
            return out
        out['seq'], out['logp'] = seq, lp
        sents, score = [[int(t) for t in row if t > 0] for row in seq], lp.sum(1).astype('float')
    out['info'] = [{'sentence': s, 'timestamp': stamps[i], 'sentence_confidence': score[i], 'proposal_score': float(conf[i]),
                    're_score': 10 * float(conf[i]) + score[i], 'num': [i, len(sents)]} for i, s in enumerate(sents)]
    return out

"""Proposal selection for evaluation -- the index-producing part of the reference's eval_utils.py.

`gettop1000` keeps the reference's signature and return tuple (eval_utils.py:259-287) but runs the threshold search and the
ordered enumeration in one HIP kernel (echr_top_proposals) instead of a numpy sort + an O(T*K) python double loop; the
device tensors it produced are also returned by `top_proposals_device` so the caption path can consume them without a
round trip through python lists.

`caption_videos` is the same flow over V videos in one pass: one batched SST call, one batched selection launch
(echr_top_proposals_batch / _nms_batch, a workgroup per video), one caption pass over a VideoBatch.  `caption_videos_beam` is that flow
with the captions decoded by beam search (CaptionGenerator.beam_batch).  With flag_eval_what='SOTA_TEP' the events of both come from an
external proposal list instead of the score grid (echr_amd.extprops.select).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import functional as EF
from .batch import VideoBatch
from .misc import utils

EVENT_GROUP_ROWS = 128          # caption_videos' default event_group_rows: a tuning constant, not a correctness condition


def top_proposals_device(pred_proposals, tap_masks, topN=1000, val_score_thres=0.0):
    """(ind [M] int32, featstamps [M,2] int32, confidence [M] fp32) device tensors; one D2H sync for M."""
    lib = L.load()
    dev = pred_proposals.device
    scores = pred_proposals.detach().to(torch.float32).contiguous()
    masks = torch.as_tensor(np.asarray(tap_masks) if not isinstance(tap_masks, torch.Tensor) else tap_masks).to(dev, torch.float32).contiguous()
    T, K = scores.shape
    ind = torch.empty(T * K, device=dev, dtype=torch.int32)
    feat = torch.empty(T * K, 2, device=dev, dtype=torch.int32)
    conf = torch.empty(T * K, device=dev, dtype=torch.float32)
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)
    L.check(lib.echr_top_proposals(L.ptr(scores), L.ptr(masks), T, K, int(topN), float(val_score_thres), L.ptr(ind, torch.int32),
                                   L.ptr(feat, torch.int32), L.ptr(conf), L.ptr(cnt, torch.int32), L.stream_ptr()), 'top_proposals')
    m = int(cnt.item())
    return ind[:m], feat[:m], conf[:m]


def gettop1000(pred_proposals, tap_masks, cg_gts, duration, featstamp_to_time, val_score_thres=0, topN=1000):
    """Same outputs as the reference: (index_select_list, featstamp_list, cg_select_list, timestamp_list, confidence)."""
    if not isinstance(pred_proposals, torch.Tensor):
        pred_proposals = torch.as_tensor(np.asarray(pred_proposals, dtype=np.float32))
    if not pred_proposals.is_cuda:
        raise L.EchrHipError('gettop1000 runs on the GPU: pass the SST scores as a CUDA tensor')
    nfeats = pred_proposals.shape[0]
    ind, feat, conf = top_proposals_device(pred_proposals, tap_masks, topN, float(val_score_thres))
    ind_l, feat_l, conf_l = ind.cpu().tolist(), feat.cpu().tolist(), conf.cpu().tolist()
    cg_l = [cg_gts[n, n - s] for n, (s, _) in zip(ind_l, feat_l)] if len(cg_gts) else []
    time_l = [featstamp_to_time(s, e, nfeats, duration) for s, e in feat_l]
    return ind_l, feat_l, cg_l, time_l, conf_l


def gettop1000_nms(pred_proposals, tap_masks, cg_gts, duration, featstamp_to_time, overlap=0.8, topN=1000):
    """Same outputs as the reference (eval_utils.py:290-331): (index_select_list, nms_props [M,2], prop_gts, timestamp_list,
    nms_scores), with the candidate enumeration, the score ordering and the greedy suppression in one HIP kernel
    (echr_top_proposals_nms).  `tap_masks` is unused, as in the reference."""
    lib = L.load()
    if not isinstance(pred_proposals, torch.Tensor):
        pred_proposals = torch.as_tensor(np.asarray(pred_proposals, dtype=np.float32))
    if not pred_proposals.is_cuda:
        raise L.EchrHipError('gettop1000_nms runs on the GPU: pass the SST scores as a CUDA tensor')
    scores = pred_proposals.detach().to(torch.float32).contiguous()
    dev = scores.device
    T, K = scores.shape
    scratch = torch.empty(T * K, device=dev, dtype=torch.float32)
    feat = torch.empty(int(topN), 2, device=dev, dtype=torch.int32)
    conf = torch.empty(int(topN), device=dev, dtype=torch.float32)
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)
    L.check(lib.echr_top_proposals_nms(L.ptr(scores), T, K, int(topN), float(overlap), L.ptr(scratch), L.ptr(feat, torch.int32), L.ptr(conf),
                                       L.ptr(cnt, torch.int32), L.stream_ptr()), 'top_proposals_nms')
    m = int(cnt.item())
    props = feat[:m].cpu().numpy().astype(np.int64)
    nms_scores = conf[:m].cpu().numpy().astype(np.float64)
    prop_gts = np.array([cg_gts[e - 1, e - 1 - s] for s, e in props]) if len(cg_gts) else np.array([])
    timestamp_list = [featstamp_to_time(s, e, T, duration) for (s, e) in props]
    return props[:, 1] - 1, props, prop_gts, timestamp_list, nms_scores


def caption_video(tap_model, cg_model, c3d_feats, lda_feats, duration, featstamp_to_time, vocab=None, tap_masks=None, cg_gts=(),
                  topN=1000, nms_threshold=0.0, val_score_thres=0.0, flag_eval_what='tap_cg', beam_size=1, *, ext_proposals=None, ext_seed=0):
    """One video through the reference's evaluation flow (eval_utils.py:51-53,106-167 for flag_eval_what 'tap_cg' / 'tap'):
    SST -> proposal selection (greedy NMS when nms_threshold != 0, else score threshold) -> greedy captions -> the per-proposal
    records of result.json.  Everything between the two host reads (proposal count, caption lengths) stays on the GPU.

    Returns (vid_info, extras): vid_info is the reference's list of dicts (sentence, timestamp, sentence_confidence, proposal_score,
    re_score, num); extras carries the tensors (tap_feats, pred_proposals, seq, ind_select_list, soi_select_list).
    beam_size > 1 captions by beam search (the reference's --beam_size); sentence_confidence is then each caption's beam score (the sum
    of its token log-probs, <eos> included).

    flag_eval_what='SOTA_TEP' with ext_proposals=(timestamps [P, 2] in seconds, scores [P]) captions external proposals instead
    (extprops.select on this one video, draw id 0, the crop keyed by `ext_seed`; see caption_videos): 'timestamp' is the external segment,
    proposal_score the external score, cg_select_list = cg_gts[e, e - s - 1].  scores None: the reference skips the video ([])."""
    if (flag_eval_what == 'SOTA_TEP') != (ext_proposals is not None):
        raise ValueError("flag_eval_what='SOTA_TEP' and ext_proposals=(timestamps, scores) go together")
    if not c3d_feats.is_cuda:
        raise L.EchrHipError('caption_video runs on the GPU: move the models and features with .cuda()')
    nfeats = c3d_feats.shape[0]
    with torch.no_grad():
        tap_feats, pred_proposals = tap_model(c3d_feats)
        if tap_masks is None:
            K = pred_proposals.shape[1]
            tap_masks = (np.arange(nfeats)[:, None] >= np.arange(K)[None, :]).astype(np.float32)
        if ext_proposals is not None:
            from . import extprops
            sel = extprops.select([dict(SOTA_timestamps=ext_proposals[0], SOTA_Prop_score=ext_proposals[1], duration=duration, nfeats=nfeats)],
                                  int(pred_proposals.shape[1]), topN, nms_threshold, val_score_thres, seed=ext_seed, device=c3d_feats.device)
            ind_select_list, soi_select_list = sel.ind[0].tolist(), sel.soi[0].tolist()
            cg_select_list = [cg_gts[e, e - s - 1] for e, (s, _) in zip(ind_select_list, soi_select_list)] if len(cg_gts) else []
            good_time_stamps, tap_prob = sel.timestamps[0].tolist(), sel.scores[0].tolist()
        elif nms_threshold != 0:
            ind_select_list, soi_select_list, cg_select_list, good_time_stamps, tap_prob = gettop1000_nms(
                pred_proposals, tap_masks, cg_gts, duration, featstamp_to_time, overlap=nms_threshold, topN=topN)
        else:
            ind_select_list, soi_select_list, cg_select_list, good_time_stamps, tap_prob = gettop1000(
                pred_proposals, tap_masks, cg_gts, duration, featstamp_to_time, val_score_thres=val_score_thres, topN=topN)
        extras = dict(tap_feats=tap_feats, pred_proposals=pred_proposals, ind_select_list=ind_select_list, soi_select_list=soi_select_list,
                      seq=None, cg_prob=None)
        n = len(ind_select_list)
        if n == 0:
            return [], extras
        if flag_eval_what == 'tap':
            sents, cg_score = [0] * n, [0] * n
        else:
            if beam_size != 1:
                seq, cg_prob, beam_score = cg_model(tap_feats, c3d_feats, lda_feats, [], ind_select_list, soi_select_list, mode='eval',
                                                    beam_size=beam_size, return_score=True)
            else:
                seq, cg_prob = cg_model(tap_feats, c3d_feats, lda_feats, [], ind_select_list, soi_select_list, mode='eval')
            if len(seq) == 0:
                return [], extras
            extras['seq'], extras['cg_prob'] = seq, cg_prob
            if beam_size != 1:
                cg_score = beam_score.cpu().numpy().astype('float')
            else:
                cg_score = cg_prob.sum(1).cpu().numpy().astype('float')
            sents = utils.decode_sequence(vocab, seq) if vocab is not None else [row[row > 0].tolist() for row in seq.cpu().numpy()]
    vid_info = []
    for i, sent in enumerate(sents):
        vid_info.append({'sentence': sent, 'timestamp': good_time_stamps[i], 'sentence_confidence': cg_score[i],
                         'proposal_score': float(tap_prob[i]), 're_score': 10 * float(tap_prob[i]) + cg_score[i], 'num': [i, len(sents)]})
    return vid_info, extras


def top_proposals_batch_device(pred_proposals, row_offset, tap_masks=None, topN=1000, val_score_thres=0.0, nms_threshold=0.0):
    """Proposal selection of V videos in one call, no host synchronisation: `pred_proposals` [T_tot, K] is SST.forward_batch's score matrix,
    `row_offset` [V+1] (host integers) its video boundaries, `tap_masks` [T_tot, K] or None for the causal mask n_local >= k (threshold
    mode only; the NMS ignores masks, as the reference does).  nms_threshold != 0 selects by greedy NMS, else by score threshold.
    Returns a dict of device tensors: count int32 [V+2] (picks per video, their total, the largest interval length), event_offset int32
    [V+1], and -- allocated for the worst case, valid in their first count[V] entries -- vid, ind, ind_abs int32 [cap], feat, feat_abs
    int32 [cap, 2], conf fp32 [cap]; `row_offset` is the int32 device copy."""
    lib = L.load()
    if not isinstance(pred_proposals, torch.Tensor) or not pred_proposals.is_cuda:
        raise L.EchrHipError('top_proposals_batch_device runs on the GPU: pass the SST scores as a CUDA tensor')
    scores = pred_proposals.detach().to(torch.float32).contiguous()
    dev = scores.device
    T_tot, K = scores.shape
    ro = EF.sst_row_offsets(row_offset, T_tot)
    V = len(ro) - 1
    ro_dev = EF.upload(torch.from_numpy(ro), dev)
    i32 = dict(device=dev, dtype=torch.int32)
    nms = nms_threshold != 0
    topN = int(topN)
    if nms:
        topN = max(1, min(topN, int(np.diff(ro).max()) * K))          # a video has at most T_v*K candidates: the picks are the same
    cap = V * topN if nms else T_tot * K
    out = dict(count=torch.empty(V + 2, **i32), event_offset=torch.empty(V + 1, **i32), vid=torch.empty(cap, **i32), ind=torch.empty(cap, **i32),
               feat=torch.empty(cap, 2, **i32), ind_abs=torch.empty(cap, **i32), feat_abs=torch.empty(cap, 2, **i32),
               conf=torch.empty(cap, device=dev, dtype=torch.float32), row_offset=ro_dev)
    tail = [L.ptr(out[k], torch.int32) for k in ('count', 'event_offset', 'vid', 'ind', 'feat', 'ind_abs', 'feat_abs')] + [L.ptr(out['conf']), L.stream_ptr()]
    if nms:
        live = torch.empty(T_tot * K, device=dev, dtype=torch.float32)
        L.check(lib.echr_top_proposals_nms_batch(L.ptr(scores), L.ptr(ro_dev, torch.int32), T_tot, V, K, topN, float(nms_threshold), L.ptr(live),
                                                 *tail), 'top_proposals_nms_batch')
    else:
        masks = None
        if tap_masks is not None:
            masks = torch.as_tensor(np.asarray(tap_masks) if not isinstance(tap_masks, torch.Tensor) else tap_masks).to(dev, torch.float32).contiguous()
            if tuple(masks.shape) != (T_tot, K):
                raise ValueError('tap_masks must be [%d, %d] like the scores (got %s)' % (T_tot, K, tuple(masks.shape)))
        L.check(lib.echr_top_proposals_batch(L.ptr(scores), L.ptr(masks), L.ptr(ro_dev, torch.int32), T_tot, V, K, topN, float(val_score_thres),
                                             *tail), 'top_proposals_batch')
    return out


def _to_dev(x, dev):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=dev, dtype=torch.float32)


def caption_videos(tap_model, cg_model, videos, featstamp_to_time, vocab=None, topN=1000, nms_threshold=0.0, val_score_thres=0.0,
                   flag_eval_what='tap_cg', event_group_rows=EVENT_GROUP_ROWS, *, ext_seed=0):
    """`caption_video` over V videos in ONE evaluation pass: SST.forward_batch over the concatenated features -> batched proposal selection
    (a workgroup per video; greedy NMS when nms_threshold != 0, else score threshold) -> one greedy caption pass over a VideoBatch
    (forward_batch(mode='eval', event_group_rows=...)).  Runs under no_grad with both models switched to eval mode for the call.

    `videos`: a list of dicts with 'c3d' [T_v, D] (CUDA tensor), 'lda', 'duration' and optionally 'tap_masks' [T_v, K] (all videos or none)
    and 'cg_gts'.  flag_eval_what='cg' captions given events instead of selected ones: every video then carries 'ind', 'soi' and
    'timestamps' (the reference's gts_ind_select_list / gts_soi_select_list / gt_timestamps; proposal_score is 1).  'tap' skips the
    caption pass (sentence 0).

    flag_eval_what='SOTA_TEP' captions EXTERNAL proposals (eval_utils.py:76-104): every video carries 'SOTA_timestamps'
    [P_v, 2] in seconds and 'SOTA_Prop_score' [P_v], optionally 'SOTA_draw' (its crop stream id, default its position).  The SST still runs
    (its states feed the VH / EH / CH contexts); the events come from extprops.select with K the encoder's anchor count and topN,
    nms_threshold, val_score_thres passed through (greedy cluster NMS over the timestamps when nms_threshold > 0, score threshold, topN,
    featstamps, crop of over-long proposals keyed by `ext_seed`).  'timestamp' is the external segment, proposal_score the external score.
    cg_select_list = cg_gts[e, e - s - 1] for rows (s, e): the reference's own off-by-one against the anchor convention cg_gts[n, n - s] of
    the other modes (dataloader.py:522 indexes k = e - s - 1 where anchor k of row e starts at e - k), reproduced as it is.  A video whose
    score list is None or missing, or with at most one row, is skipped as in the reference: [] and listed in extras['bad'].

    Returns (vid_infos, extras).  vid_infos[v] is the list caption_video returns for video v alone (sentence, timestamp,
    sentence_confidence, proposal_score, re_score, num); a video without a pick, or whose rows all emit <eos> first, gets [].  The batched
    decode stops when nobody in the BATCH is unfinished, so every video's sequences and log-probs are cut to the width that video alone
    would have produced before the confidence is summed.  extras: 'batch' (the VideoBatch of the videos that have events, 'kept' their
    indices), 'pred_proposals', 'tap_feats', 'row_offset', 'selection' (the device tensors of top_proposals_batch_device), 'seq' /
    'cg_prob' of the batch and 'per_video' (ind_select_list, soi_select_list, cg_select_list, seq, cg_prob of each video).

    Host reads per call, whatever V is: the selection counts, the selected lists (one packed copy), the decoder's step counts, and the
    sequences / log-probs of the batch.  Beam search over the batch is caption_videos_beam.
    The batch is built for the model's decoder (opt.caption_model): a one-stream model ('show_attend_tell') gets the same one-pass
    evaluation through its batched greedy decode; caption_videos_beam refuses it, as beam_batch does.

    The validation loss of the same batch (eval_split's get_eval_loss), with labels stacked into the batch:
        logp = cg_model.forward_batch(extras['batch'], mode='train')
        cg_loss, _ = extras['batch'].criterion(cg_crit, logp)
        tap_loss, _ = utils.tap_criterion_batch(tap_crit, extras['pred_proposals'], tap_masks, tap_labels, w1, extras['row_offset'])"""
    return _caption_videos_checked(tap_model, cg_model, videos, featstamp_to_time, vocab, topN, nms_threshold, val_score_thres, flag_eval_what,
                                   event_group_rows, ext_seed=ext_seed)


def caption_videos_beam(tap_model, cg_model, videos, featstamp_to_time, beam_size, vocab=None, topN=1000, nms_threshold=0.0, val_score_thres=0.0,
                        flag_eval_what='tap_cg', event_group_rows=EVENT_GROUP_ROWS, max_rows=8192, *, ext_seed=0):
    """`caption_videos` with the captions decoded by beam search (the reference's eval.py --beam_size): the same SST call, selection call
    and VideoBatch, then CaptionGenerator.beam_batch(batch, beam_size, event_group_rows, max_rows) instead of the greedy pass.  `max_rows`
    bounds the decode's workspace: it runs once per run of consecutive videos with at most that many events * beam_size rows (None: once).
    flag_eval_what='SOTA_TEP' runs the same external-proposal selection as caption_videos (`ext_seed` keys its crop).

    vid_infos[v] is what caption_video(beam_size=) returns for video v alone: seq / cg_prob cut to the video's own width
    video_words[v], sentence_confidence the beam score (the sum of the caption's token log-probs, <eos> included).  A video whose
    results are all empty (video_words[v] == 0) gets [] and per_video[v]['seq'] None.  extras additionally carries 'score' [N_tot]
    (device) and 'video_words' (host int64, one entry per kept video).

    Host reads per call do not grow with V: the selection reads, one video_words read per run, the batch's sequences and scores."""
    B = EF._check_beam_size(beam_size, cg_model.lm_model.vocab_size + 1)
    return _caption_videos_checked(tap_model, cg_model, videos, featstamp_to_time, vocab, topN, nms_threshold, val_score_thres, flag_eval_what,
                                   event_group_rows, B, max_rows, ext_seed=ext_seed)


def _caption_videos_checked(tap_model, cg_model, videos, featstamp_to_time, vocab, topN, nms_threshold, val_score_thres, flag_eval_what,
                            event_group_rows, beam=None, max_rows=None, ext_seed=0):
    """The argument checks of caption_videos / caption_videos_beam, then _caption_videos under no_grad with both models in eval mode."""
    if flag_eval_what not in ('tap_cg', 'tap', 'cg', 'SOTA_TEP'):
        raise ValueError("flag_eval_what=%r: caption_videos runs 'tap_cg', 'tap', 'cg' and 'SOTA_TEP'" % (flag_eval_what,))
    videos = list(videos)
    if not videos:
        raise ValueError('a batch needs at least one video')
    if any(not (isinstance(v['c3d'], torch.Tensor) and v['c3d'].is_cuda) for v in videos):
        raise L.EchrHipError('caption_videos runs on the GPU: move the models and features with .cuda()')
    if flag_eval_what == 'cg':
        for i, v in enumerate(videos):
            missing = [k for k in ('ind', 'soi', 'timestamps') if k not in v]
            if missing or not (len(v['ind']) == len(v['soi']) == len(v['timestamps'])):
                raise ValueError("video %d: flag_eval_what='cg' takes the given events as 'ind', 'soi' and 'timestamps' of one length" % i)
    V, dev = len(videos), videos[0]['c3d'].device
    rows = np.concatenate([[0], np.cumsum([int(v['c3d'].shape[0]) for v in videos])]).astype(np.int64)
    sst_dropout, cg_training = tap_model.rnn.dropout, cg_model.training
    tap_model.eval()
    cg_model.eval()
    try:
        with torch.no_grad():
            return _caption_videos(tap_model, cg_model, videos, featstamp_to_time, vocab, topN, nms_threshold, val_score_thres, flag_eval_what,
                                   event_group_rows, V, dev, rows, beam, max_rows, ext_seed)
    finally:
        tap_model.rnn.dropout = sst_dropout
        cg_model.train(cg_training)


def _caption_videos(tap_model, cg_model, videos, featstamp_to_time, vocab, topN, nms_threshold, val_score_thres, flag_eval_what, event_group_rows,
                    V, dev, rows, beam=None, max_rows=None, ext_seed=0):
    c3d_all = torch.cat([_to_dev(v['c3d'], dev) for v in videos], 0)
    lda_all = torch.stack([_to_dev(v['lda'], dev).reshape(-1) for v in videos], 0)
    tap_all, scores = tap_model.forward_batch(c3d_all, rows)
    extras = dict(tap_feats=tap_all, pred_proposals=scores, row_offset=rows, selection=None, batch=None, kept=[], seq=None, cg_prob=None)
    if beam is not None:
        extras.update(score=None, video_words=None)
    # ---- events per video: (soi [N_v,2] local, tap_prob [N_v], timestamps) ----
    if flag_eval_what == 'cg':
        sois = [np.asarray(v['soi'], dtype=np.int64).reshape(-1, 2) for v in videos]
        inds = [np.asarray(v['ind'], dtype=np.int64).reshape(-1) for v in videos]
        probs = [[1] * len(s) for s in sois]
        stamps = [list(v['timestamps']) for v in videos]
    elif flag_eval_what == 'SOTA_TEP':
        from . import extprops
        ext = [dict(SOTA_timestamps=v.get('SOTA_timestamps'), SOTA_Prop_score=v.get('SOTA_Prop_score'), duration=v['duration'],
                    nfeats=int(rows[i + 1] - rows[i])) for i, v in enumerate(videos)]
        sel = extras['selection'] = extprops.select(ext, int(scores.shape[1]), topN, nms_threshold, val_score_thres, seed=ext_seed,
                                                    draw=[int(v.get('SOTA_draw', i)) for i, v in enumerate(videos)], device=dev)
        extras['bad'] = sel.bad
        sois, inds = sel.soi, sel.ind
        probs = [s.tolist() for s in sel.scores]
        stamps = [t.tolist() for t in sel.timestamps]
    else:
        masks = [v.get('tap_masks') for v in videos]
        if any(m is not None for m in masks) and not all(m is not None for m in masks):
            raise ValueError('either every video carries tap_masks or none does')
        tap_masks = None
        if masks[0] is not None and nms_threshold == 0:
            tap_masks = torch.cat([_to_dev(m, dev) for m in masks], 0)
        sel = extras['selection'] = top_proposals_batch_device(scores, rows, tap_masks, topN, val_score_thres, nms_threshold)
        cnt = sel['count'].cpu().numpy()                                   # host read 1: the counts
        n_tot = int(cnt[V])
        eo = np.concatenate([[0], np.cumsum(cnt[:V])]).astype(np.int64)
        # host read 2: the lists (intervals and scores; anchors, vid and the absolute indices follow from them), as one packed copy
        packed = torch.cat([sel['feat'][:n_tot].reshape(-1), sel['conf'][:n_tot].view(torch.int32)]).cpu().numpy()
        feat, conf = packed[:2 * n_tot].reshape(-1, 2).astype(np.int64), packed[2 * n_tot:].view(np.float32)
        sois = [feat[eo[v]:eo[v + 1]] for v in range(V)]
        inds = [s[:, 1] - 1 for s in sois]
        if nms_threshold != 0:
            probs = [conf[eo[v]:eo[v + 1]].astype(np.float64) for v in range(V)]
        else:
            probs = [conf[eo[v]:eo[v + 1]].tolist() for v in range(V)]
        stamps = [[featstamp_to_time(int(s), int(e), int(rows[v + 1] - rows[v]), videos[v]['duration']) for s, e in sois[v]] for v in range(V)]
    per_video = []
    sota = 1 if flag_eval_what == 'SOTA_TEP' else 0          # dataloader.py:522 reads cg_gts[e, e - s - 1]
    for v in range(V):
        gts = videos[v].get('cg_gts', ())
        cg_sel = [gts[n, n - s - sota] for n, (s, _) in zip(inds[v].tolist(), sois[v].tolist())] if len(gts) else []
        per_video.append(dict(ind_select_list=inds[v].tolist(), soi_select_list=sois[v].tolist(), cg_select_list=cg_sel, seq=None, cg_prob=None))
    extras['per_video'] = per_video
    vid_infos = [[] for _ in range(V)]
    kept = extras['kept'] = [v for v in range(V) if len(sois[v])]
    if not kept:
        return vid_infos, extras
    # ---- the batch of the videos that have events (VideoBatch.validate refuses a video without one) ----
    if len(kept) == V:
        c3d_b, tap_b, lda_b, rows_b = c3d_all, tap_all, lda_all, rows
    else:                                                                  # rare: re-gather the kept videos' rows
        c3d_b = torch.cat([c3d_all[rows[v]:rows[v + 1]] for v in kept], 0)
        tap_b = torch.cat([tap_all[rows[v]:rows[v + 1]] for v in kept], 0)
        lda_b = lda_all[torch.as_tensor(kept, device=dev)]
        rows_b = np.concatenate([[0], np.cumsum([rows[v + 1] - rows[v] for v in kept])]).astype(np.int64)
    eo_b = np.concatenate([[0], np.cumsum([len(sois[v]) for v in kept])]).astype(np.int64)
    batch = extras['batch'] = VideoBatch(c3d_b, tap_b, lda_b, rows_b, eo_b, np.concatenate([sois[v] + rows_b[i] for i, v in enumerate(kept)], 0),
                                         np.concatenate([inds[v] + rows_b[i] for i, v in enumerate(kept)], 0),
                                         clip_context_type=cg_model.opt.clip_context_type,
                                         CG_init_feats_type=getattr(cg_model.opt, 'CG_init_feats_type', ''),
                                         caption_model=getattr(cg_model.opt, 'caption_model', None))
    if flag_eval_what == 'tap':
        for v in kept:
            n = len(sois[v])
            vid_infos[v] = _records([0] * n, stamps[v], [0] * n, probs[v])
        return vid_infos, extras
    if beam is not None:
        # beam search: the per-video widths come back with the decode (one read per run), the confidence is the beam score
        seq, cg_prob, score, video_words = cg_model.beam_batch(batch, beam, event_group_rows=event_group_rows, max_rows=max_rows)
        extras['score'], extras['video_words'] = score, video_words
        if len(seq) == 0:
            return vid_infos, extras
        extras['seq'], extras['cg_prob'] = seq, cg_prob
        seq_h, score_h = seq.cpu().numpy(), score.cpu().numpy().astype('float')
        for i, v in enumerate(kept):
            s, width = batch.event_slices[i], int(video_words[i])
            if width == 0:
                continue
            per_video[v]['seq'], per_video[v]['cg_prob'] = seq[s, :width], cg_prob[s, :width]
            sents = utils.decode_sequence(vocab, seq[s, :width]) if vocab is not None else [row[row > 0].tolist() for row in seq_h[s, :width]]
            vid_infos[v] = _records(sents, stamps[v], score_h[s], probs[v])
        return vid_infos, extras
    seq, cg_prob = cg_model.forward_batch(batch, mode='eval', event_group_rows=event_group_rows)
    if len(seq) == 0:
        return vid_infos, extras
    extras['seq'], extras['cg_prob'] = seq, cg_prob
    seq_h, lp_h = seq.cpu().numpy(), cg_prob.cpu()
    for i, v in enumerate(kept):
        s = batch.event_slices[i]
        width = int((seq_h[s] > 0).any(0).sum())          # the steps video v alone would have run (OldModel_NEW.py:176-181): nonzero columns form a prefix
        if width == 0:
            continue
        per_video[v]['seq'], per_video[v]['cg_prob'] = seq[s, :width], cg_prob[s, :width]
        cg_score = lp_h[s, :width].contiguous().sum(1).numpy().astype('float')
        sents = utils.decode_sequence(vocab, seq[s, :width]) if vocab is not None else [row[row > 0].tolist() for row in seq_h[s, :width]]
        vid_infos[v] = _records(sents, stamps[v], cg_score, probs[v])
    return vid_infos, extras


def _records(sents, stamps, cg_score, tap_prob):
    return [{'sentence': sent, 'timestamp': stamps[i], 'sentence_confidence': cg_score[i], 'proposal_score': float(tap_prob[i]),
             're_score': 10 * float(tap_prob[i]) + cg_score[i], 'num': [i, len(sents)]} for i, sent in enumerate(sents)]


def gettopN_nms(props, prop_scores, sent_score, nms_overlap=0.999, topN=1000):
    """Host-side greedy temporal NMS over already materialised proposals (eval_utils.py:230-256; called from the per-video loop at
    :89 with sent_score = prop_scores).  Proposals are visited by descending `prop_scores`; every proposal whose IoU (with the
    reference's +1e-3 interval closure) with the current best reaches `nms_overlap` forms its cluster, the cluster is represented by
    its member with the highest `sent_score`, and only proposals with IoU <= nms_overlap stay for the next round.  Returns
    (props[pick], prop_scores[pick], pick) like the reference.  A handful of proposals per video: numpy on the host, as there."""
    props = np.asarray(props)
    prop_scores = np.asarray(prop_scores)
    sent_score = np.asarray(sent_score)
    start, end = props[:, 0], props[:, 1]
    length = (end - start + 1e-3).astype(float)
    # ascending; the current best is the last entry.  The reference's np.argsort is its unstable default; a stable sort is one of that
    # call's possible outcomes on tied scores, the only one on distinct scores, and the rule the device states (extprops.nms)
    alive = np.argsort(prop_scores, kind='stable')
    pick = []
    while alive.size and len(pick) < topN:
        best = alive[-1]
        inter = np.maximum(0., np.minimum(end[best], end[alive]) - np.maximum(start[best], start[alive]) + 1e-3)
        iou = inter / (length[best] + length[alive] - inter)
        cluster = alive[np.nonzero(iou >= nms_overlap)[0]]
        pick.append(cluster[np.argmax(sent_score[cluster])])
        alive = alive[np.nonzero(iou <= nms_overlap)[0]]
    return props[pick, :], prop_scores[pick], pick


def reranking(vid_info):
    """Keep the videos whose 're_score' reaches the 10th largest one (all of them when there are fewer than 10): eval_utils.py:334-345."""
    scores = np.sort(np.array([v['re_score'] for v in vid_info]))
    threshold = scores[-min(len(scores), 10)]
    return [v for v in vid_info if v['re_score'] >= threshold]


def ciderd_of(extras_or_seq, scorer, refs):
    """Mean CIDEr-D (a float; echr_amd.reward.CiderD.score) of the captions of a `caption_video` / `caption_videos`
    result -- its `extras` dict (the batch's 'seq') or the seq [N, T] itself -- against `refs`, the packed references of the N caption rows
    in row order (echr_amd.reward.pack_refs).  A result without captions ([] / None: every row emitted <eos> first) scores the empty
    captions.  A validation score with nothing installed; one host read."""
    seq = extras_or_seq.get('seq') if isinstance(extras_or_seq, dict) else extras_or_seq
    width = None
    if not isinstance(seq, torch.Tensor) or seq.numel() == 0:
        n = torch.as_tensor(refs[2]).numel() - 1
        scorer.cuda()
        seq, width = torch.zeros(n, 1, dtype=torch.int64, device=scorer.device), 0
    return float(scorer.score(seq, refs, width=width).mean().cpu())


def dense_scores(vid_infos, extras, gt, tious=None, scorer=None):
    """The dense-captioning scores (echr_amd.densecap.evaluate) of what caption_videos / caption_videos_beam /
    caption_video returned: tIoU matching of the records' 'timestamp' against `gt` (densecap.pack_ground_truth(...).cuda(), the videos in
    the call's order), Recall / Precision / f1() and BLEU-1..4, ROUGE-L and -- with a reward.CiderD `scorer` -- CIDEr-D over the matched
    pairs.  The caption rows are those of extras['batch'].event_slices over extras['kept']; a video that was not kept, or that has no
    record, counts as a video without predictions.  A flag_eval_what='tap' result (no captions) gives detection only."""
    from . import densecap
    single = isinstance(extras, dict) and 'per_video' not in extras          # caption_video: one flat list of records
    infos = [vid_infos] if single else list(vid_infos)
    V = gt.offset.numel() - 1
    if len(infos) != V:
        raise ValueError('%d videos were captioned, the ground truth has %d' % (len(infos), V))
    dev = gt.stamps.device
    stamps = [r['timestamp'] for info in infos for r in info]
    off = np.concatenate([[0], np.cumsum([len(info) for info in infos])]).astype(np.int32)
    pst = torch.from_numpy(np.asarray(stamps, dtype=np.float64).reshape(-1, 2)).to(dev)
    seq = extras.get('seq')
    if not isinstance(seq, torch.Tensor) or seq.numel() == 0:
        seq = None
    elif not single:
        slices = dict(zip(extras['kept'], extras['batch'].event_slices))
        rows = [np.arange(slices[v].start, slices[v].stop) for v in range(V) if len(infos[v])]
        rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        if rows.size != seq.shape[0] or (rows != np.arange(rows.size)).any():
            seq = seq.index_select(0, torch.from_numpy(rows).to(seq.device))
    if seq is not None and seq.shape[0] != int(off[-1]):
        raise ValueError('%d records, %d caption rows' % (int(off[-1]), seq.shape[0]))
    return densecap.evaluate(pst, off, seq, gt, densecap.TIOUS if tious is None else tious, scorer=scorer)

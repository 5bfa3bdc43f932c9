"""Dense-caption scoring over token ids on the device: the ANETcaptions protocol of the reference's
external_tool/densevid_eval/evaluate.py without METEOR -- tIoU matching of predicted against ground-truth events, Recall / Precision
(whose F1 is train.py's proposal-stage score), and BLEU-1..4, ROUGE-L and CIDEr-D over the matched (prediction, ground truth) pairs.

The kernels are csrc/densecap.hip (echr_densecap_match / _fill / _pair_stats / _reduce); CIDEr-D goes through echr_ciderd_score on the
pair-major gathered rows.  There is no host fallback: CPU tensors raise EchrHipError.

One ground-truth set per call.  With several annotator files the reference takes the per-video maximum of precision / recall over the
files and pools the language pairs; a caller with several files calls evaluate once per file and combines the results itself.

A caption's words, for BLEU and ROUGE-L, are the tokens before its first 0 among its columns, all of them when there is none; there is
no end token.  CIDEr-D keeps section 4s's sequence rule (an end token iff the caption is shorter than seq_length).  A prediction that
no ground truth reaches at a threshold contributes one unmatched pair: zero n-gram matches against a reference of length 1, ROUGE-L 0,
CIDEr-D 0 -- the reference's comparison with its garbage string, defined directly."""
import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import reward as RW

TIOUS = (0.3, 0.5, 0.7, 0.9)
MAX_TIOUS = 8                # ECHR_DENSECAP_MAX_TAU
VIDEO_COLS = 10              # ECHR_DENSECAP_VIDEO_COLS: Recall, Precision, Bleu_1..4, ROUGE_L, CIDErD, pairs, unmatched pairs
MEAN_COLS = 8                # ECHR_DENSECAP_MEAN_COLS
STATS = 7                    # ECHR_DENSECAP_STATS: match_1..4, len_c, len_r, lcs
SCORES = ('Recall', 'Precision', 'Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L', 'CIDErD')
LANGUAGE = SCORES[2:]


class GroundTruth(NamedTuple):
    """The ground truth of V videos in the kernels' form: stamps fp64 [G_tot, 2] (seconds), offset int32 [V + 1], refs int32 [G_tot, L]
    (one reference per event, section 4s's zero-padded sequences) and ref_len int32 [G_tot]."""
    stamps: torch.Tensor
    offset: torch.Tensor
    refs: torch.Tensor
    ref_len: torch.Tensor

    def to(self, device):
        return GroundTruth(self.stamps.to(device), self.offset, self.refs.to(device), self.ref_len.to(device))

    def cuda(self, device=None):
        return self.to(torch.device('cuda') if device is None else device)


def pack_ground_truth(videos, seq_length, vocab_size=None):
    """videos: per video a dict (or pair) of 'timestamps' [G_v, 2] in seconds and 'sentences', one per event, as label rows or token lists
    (what reward.pack_refs takes).  Returns GroundTruth (host tensors; .cuda() uploads it once -- offset stays on the host, evaluate sizes its
    loops from it).  ValueError for a video without an event, a count mismatch, a malformed stamp, a sentence longer than seq_length or a
    token outside the vocabulary; seq_length above 63 and vocab_size + 1 above 65535 are refused as in section 4s."""
    seq_length = int(seq_length)
    if not 1 <= seq_length <= RW.MAX_SEQ_LENGTH:
        raise ValueError('seq_length must be in [1, %d] (got %d)' % (RW.MAX_SEQ_LENGTH, seq_length))
    if vocab_size is not None and int(vocab_size) + 1 > RW.MAX_V1:
        raise ValueError('exact n-gram keys hold token ids up to %d: vocab_size + 1 = %d is refused' % (RW.MAX_V1 - 1, int(vocab_size) + 1))
    stamps, sents, offs = [], [], [0]
    for v, vid in enumerate(videos):
        ts, ss = (vid['timestamps'], vid['sentences']) if isinstance(vid, dict) else vid
        ts = np.asarray(ts.cpu() if isinstance(ts, torch.Tensor) else ts, dtype=np.float64)
        ss = list(ss)
        if ts.size == 0 or not ss:
            raise ValueError('video %d has no ground-truth event' % v)
        if ts.ndim != 2 or ts.shape[1] != 2 or not np.isfinite(ts).all():
            raise ValueError('video %d: timestamps must be finite [G, 2] (got shape %s)' % (v, ts.shape))
        if len(ss) != ts.shape[0]:
            raise ValueError('video %d: %d timestamps, %d sentences' % (v, ts.shape[0], len(ss)))
        stamps.append(ts)
        sents.extend([s] for s in ss)
        offs.append(offs[-1] + len(ss))
    if not stamps:
        raise ValueError('the ground truth has no video')
    packed = RW.pack_refs(sents, seq_length, vocab_size)
    return GroundTruth(torch.from_numpy(np.concatenate(stamps, 0)), torch.from_numpy(np.asarray(offs, np.int32)), packed.refs, packed.ref_len)


class DenseScores(object):
    """The result of evaluate.  Per threshold (float64 arrays [n_tau], None for a score that was not computed): Recall, Precision,
    Bleu_1 .. Bleu_4, ROUGE_L, CIDErD -- each the mean over all V videos; per_video[name] [n_tau, V]; n_pairs / n_unmatched int64
    [n_tau, V]; f1().  The numbers stay on the device (`video`, `mean`) until the first of these is read: one copy."""

    def __init__(self, tious, n_videos, video, mean, language, ciderd, pairs=None):
        self.tious, self.n_videos, self.video, self.mean = tuple(tious), int(n_videos), video, mean
        self.language, self.ciderd = bool(language), bool(ciderd)
        self.pairs = pairs          # device tensors of the call: pair_pred, pair_gt, stats (None without captions), start
        self._h = None

    def _host(self):
        if self._h is None:
            T, V = len(self.tious), self.n_videos
            flat = torch.cat([self.video.reshape(-1), self.mean.reshape(-1)]).cpu().numpy()
            self._h = (flat[:T * V * VIDEO_COLS].reshape(T, V, VIDEO_COLS), flat[T * V * VIDEO_COLS:].reshape(T, MEAN_COLS))
        return self._h

    def _has(self, name):
        return name in SCORES[:2] or (self.language and (name != 'CIDErD' or self.ciderd))

    def __getattr__(self, name):
        if name in SCORES:
            return self._host()[1][:, SCORES.index(name)].copy() if self._has(name) else None
        raise AttributeError(name)

    @property
    def per_video(self):
        v = self._host()[0]
        return {name: (v[:, :, i].copy() if self._has(name) else None) for i, name in enumerate(SCORES)}

    @property
    def n_pairs(self):
        return self._host()[0][:, :, 8].astype(np.int64)

    @property
    def n_unmatched(self):
        return self._host()[0][:, :, 9].astype(np.int64)

    def f1(self):
        """2 P R / (P + R) per threshold, 0 where P + R = 0: the proposal-stage validation score of the reference's train.py."""
        p, r = self.Precision, self.Recall
        return np.asarray([2.0 * a * b / (a + b) if a + b > 0 else 0.0 for a, b in zip(p.tolist(), r.tolist())])

    def as_dict(self):
        d = {name: getattr(self, name) for name in SCORES}
        d.update(tious=self.tious, F1=self.f1())
        return d


def _offsets(off, name):
    off = np.asarray(off.cpu() if isinstance(off, torch.Tensor) else off).reshape(-1)
    if off.size < 1 or off[0] != 0 or (np.diff(off) < 0).any():
        raise ValueError('%s must start at 0 and never decrease' % name)
    return off.astype(np.int32)


def _stamps(t, n, dev, name):
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.float64).reshape(-1, 2)))
    if not t.is_cuda and t.numel():
        raise L.EchrHipError('%s must live on the GPU (got %s); echr_amd has no CPU path' % (name, t.device))
    if t.dtype != torch.float64 or tuple(t.shape) != (n, 2):
        raise ValueError('%s must be float64 [%d, 2] (got %s %s)' % (name, n, t.dtype, tuple(t.shape)))
    return t.to(dev).contiguous()


def evaluate(pred_stamps, pred_offset, seq, gt, tious=TIOUS, seq_length=None, scorer=None):
    """Score the predictions of V videos against `gt` (a GroundTruth on the device: pack_ground_truth(...).cuda()).

    pred_stamps fp64 [N_tot, 2] (device, seconds); pred_offset [V + 1] host integers (a device tensor is read back): video v owns rows
    pred_offset[v] .. pred_offset[v + 1] - 1, possibly none; seq [N_tot, T] int32 / int64 (device, any strides, T <= seq_length) the
    captions, or None for detection only (Recall / Precision / f1; the language scores are None).  `tious`: up to 8 thresholds, passed to
    the device as fp64.  `seq_length` defaults to the width of gt.refs.  `scorer`: a reward.CiderD for the CIDErD column.

    Detection is strict (iou > tau), pairing is not (iou >= tau), as in the reference.  Everything is bitwise reproducible and a video's
    numbers do not depend on which videos share the call.  One host read inside the call (the pair totals, to size the pair buffers);
    the scores are copied when the result is first read.  Returns DenseScores."""
    if not isinstance(gt, GroundTruth):
        raise TypeError('gt must be a densecap.GroundTruth (pack_ground_truth)')
    for name, t in (('pred_stamps', pred_stamps), ('seq', seq), ('gt.stamps', gt.stamps), ('gt.refs', gt.refs)):
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise L.EchrHipError('%s must live on the GPU (got %s); echr_amd has no CPU path' % (name, t.device))
    lib = L.load()
    dev = gt.stamps.device
    g_off, p_off = _offsets(gt.offset, 'gt.offset'), _offsets(pred_offset, 'pred_offset')
    V = g_off.size - 1
    if V < 1 or p_off.size != V + 1:
        raise ValueError('pred_offset names %d videos, the ground truth has %d' % (p_off.size - 1, V))
    if (np.diff(g_off) < 1).any():
        raise ValueError('every video needs at least one ground-truth event')
    N, G = int(p_off[-1]), int(g_off[-1])
    Lr = int(gt.refs.shape[1]) if seq_length is None else int(seq_length)
    if not 1 <= Lr <= RW.MAX_SEQ_LENGTH:
        raise ValueError('seq_length must be in [1, %d] (got %d)' % (RW.MAX_SEQ_LENGTH, Lr))
    if tuple(gt.refs.shape) != (G, Lr) or gt.ref_len.numel() != G:
        raise ValueError('gt.refs must be [%d, %d] with one length each (got %s)' % (G, Lr, tuple(gt.refs.shape)))
    tious = tuple(float(t) for t in tious)
    if not 1 <= len(tious) <= MAX_TIOUS:
        raise ValueError('between 1 and %d thresholds per call (got %d)' % (MAX_TIOUS, len(tious)))
    if seq is not None:
        if not isinstance(seq, torch.Tensor) or seq.dtype not in (torch.int32, torch.int64) or seq.dim() != 2 or seq.shape[0] != N:
            raise ValueError('seq must be an int32 or int64 tensor [%d, T]' % N)
        if seq.shape[1] > Lr:
            raise ValueError('captions of %d columns do not fit seq_length = %d' % (seq.shape[1], Lr))
        if N and seq.device != dev:
            raise L.EchrHipError('captions on %s, the ground truth on %s' % (seq.device, dev))
    if scorer is not None:
        if not isinstance(scorer, RW.CiderD):
            raise TypeError('scorer must be a reward.CiderD')
        if scorer.seq_length != Lr:
            raise ValueError('the scorer was built for seq_length = %d, the ground truth for %d' % (scorer.seq_length, Lr))
    nt = len(tious)
    pst = _stamps(pred_stamps, N, dev, 'pred_stamps')
    gst = _stamps(gt.stamps, G, dev, 'gt.stamps')
    refs = gt.refs if gt.refs.dtype == torch.int32 and gt.refs.is_contiguous() else gt.refs.to(torch.int32).contiguous()
    i32, f64 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float64)
    head = torch.from_numpy(np.concatenate([p_off, g_off])).to(dev)          # one upload for both offset vectors
    p_off_d, g_off_d = head[:V + 1], head[V + 1:]
    tau = torch.tensor(tious, dtype=torch.float64).to(dev)
    count, flag, gt_hit = torch.empty(nt, N, **i32), torch.empty(nt, N, **i32), torch.empty(nt, G, **i32)
    start = torch.zeros(nt * N + 1, device=dev, dtype=torch.int64)
    video, mean = torch.empty(nt, V, VIDEO_COLS, **f64), torch.empty(nt, MEAN_COLS, **f64)
    a = L.DensecapArgs()
    a.V, a.n_tau, a.N_tot, a.G_tot = V, nt, N, G
    a.pred_stamps, a.gt_stamps = pst.data_ptr() if N else None, gst.data_ptr()
    a.pred_offset, a.gt_offset, a.tau = p_off_d.data_ptr(), g_off_d.data_ptr(), tau.data_ptr()
    a.count, a.pred_flag, a.gt_hit = (count.data_ptr() if N else None), (flag.data_ptr() if N else None), gt_hit.data_ptr()
    a.start, a.L, a.video, a.mean = start.data_ptr(), Lr, video.data_ptr(), mean.data_ptr()
    st = L.stream_ptr()
    L.check(lib.echr_densecap_match(C.byref(a), st), 'densecap_match')
    pairs = None
    language = seq is not None
    if N:
        start[1:] = torch.cumsum(count.reshape(-1), 0, dtype=torch.int64)          # the exclusive scan: plumbing
        totals = start[N::N].cpu().tolist()                                   # the call's host read: pairs up to and including each threshold
        P = int(totals[-1])
        if P >= 2 ** 31:
            raise ValueError('%d pairs in one call (at most 2^31 - 1): split the videos over several calls' % P)
        pair_pred, pair_gt = torch.empty(P, **i32), torch.empty(P, **i32)
        a.P_tot, a.pair_pred, a.pair_gt = P, pair_pred.data_ptr(), pair_gt.data_ptr()
        L.check(lib.echr_densecap_fill(C.byref(a), st), 'densecap_fill')
        pairs = dict(pair_pred=pair_pred, pair_gt=pair_gt, start=start, totals=[0] + [int(t) for t in totals], stats=None, rouge=None, cider=None)
        if language:
            stats, rouge = torch.empty(P, STATS, **i32), torch.empty(P, **f64)
            a.T, a.cand, a.cand_i32 = int(seq.shape[1]), (seq.data_ptr() if seq.numel() else None), 1 if seq.dtype == torch.int32 else 0
            a.ld, a.cs = seq.stride(0), seq.stride(1)
            a.refs, a.stats, a.rouge = refs.data_ptr(), stats.data_ptr(), rouge.data_ptr()
            L.check(lib.echr_densecap_pair_stats(C.byref(a), st), 'densecap_pair_stats')
            pairs.update(stats=stats, rouge=rouge)
            if scorer is not None:
                cider = _pair_ciderd(scorer, seq, refs, gt.ref_len, pair_pred, pair_gt, dev)
                a.cider = cider.data_ptr()
                pairs['cider'] = cider
    L.check(lib.echr_densecap_reduce(C.byref(a), st), 'densecap_reduce')
    return DenseScores(tious, V, video, mean, language, language and scorer is not None, pairs)


def _pair_ciderd(scorer, seq, refs, ref_len, pair_pred, pair_gt, dev):
    """fp32 [P]: echr_ciderd_score of every pair's candidate row against its one reference, 0 at the unmatched pairs."""
    scorer.to(dev)
    P = pair_pred.numel()
    g = pair_gt.clamp(min=0).long()
    cand = seq.to(torch.int32).index_select(0, pair_pred.long())
    packed = RW.PackedRefs(refs.index_select(0, g), ref_len.to(device=dev, dtype=torch.int32).index_select(0, g),
                           torch.arange(P + 1, device=dev, dtype=torch.int32))
    if cand.shape[1] == 0:
        cand, width = torch.zeros(P, 1, device=dev, dtype=torch.int32), 0
    else:
        width = None
    score = scorer.score(cand, packed, width=width)
    return torch.where(pair_gt >= 0, score, torch.zeros_like(score)).contiguous()

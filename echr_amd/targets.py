"""Proposal targets and caption-event samples from ground-truth segments, built on the device: the step between a
dataset's annotations and the training entries -- dataloader.get_vid_data / get_data / get_shuffle_list of the reference.

From the ground-truth featstamps of V videos, `build` gives the dense [T_tot, K] matrices the proposal criterion reads (tap_masks,
tap_labels; also iou, gts_index and good_gt = tap_gts_for_good_proposal) in the concatenated layout of JointBatchStep and
utils.tap_criterion_batch, and per video the caption events (ind, soi, cg): a sample of prop_sample_num good proposals, or all of them.
The kernels are csrc/targets.hip (echr_tap_targets_batch, echr_prop_events_batch).  There is no host fallback.

The sample is not numpy's shuffle: every good cell (t, k) draws a Philox word keyed by (seed, the video's draw id) at site
philox.SITE_PROP, and the prop_sample_num cells with the smallest (word, position) are listed in that order -- a uniform subset in uniform
order, reproducible, and the same for a video alone and inside any batch."""
import math

import numpy as np
import torch

from . import _lib as L

MAX_GT = 1024                # ECHR_TARGETS_MAX_GT: ground-truth segments per video
MAX_SAMPLE = 1024            # ECHR_PROP_MAX_SAMPLE: prop_sample_num
MAX_VIDEOS = 65535           # ECHR_TARGETS_MAX_VIDEOS
MAX_K = 65536                # ECHR_TARGETS_MAX_K


def _round_half_away(x):
    f = math.floor(abs(x))
    r = f + 1 if abs(x) - f >= 0.5 else f          # (abs(x) - floor is exact)
    return int(-r if x < 0 else r)


def featstamps(timestamps, nfeats, duration):
    """[(start, end)] in feature rows of the `timestamps` [(start, end)] in seconds of a video of `nfeats` rows and `duration` seconds
    (dataloader.timestamp_to_featstamp, dataloader.py:292-296): start = clamp(round(start / duration * nfeats), 0, nfeats - 2),
    end = clamp(round(end / duration * nfeats), start + 1, nfeats - 1).

    `round` is half away from zero.  The reference is Python 2 code (xrange, cPickle), whose round() does that; Python 3's round() goes to
    the even neighbour at exact halves (round(2.5) = 2), so it is not used here."""
    nfeats = int(nfeats)
    out = []
    for start, end in timestamps:
        s = max(min(_round_half_away(start / duration * nfeats), nfeats - 2), 0)
        e = min(max(_round_half_away(end / duration * nfeats), s + 1), nfeats - 1)
        out.append((s, e))
    return out


def gt_events(stamps):
    """The ground-truth event lists of one video (`gts_*_select_list`, dataloader.py:497-499): cg = 0 .. G - 1, ind = end, soi = [start, end + 1]."""
    st = np.asarray(stamps, dtype=np.int64).reshape(-1, 2)
    return dict(cg=np.arange(len(st), dtype=np.int64), ind=st[:, 1].copy(), soi=np.stack([st[:, 0], st[:, 1] + 1], 1))


def check_offsets(row_offset, gt_offset, gt):
    """The contract of the device vectors, checked on their host copies (the library cannot see them): both offset vectors start at 0,
    row_offset grows strictly, gt_offset never decreases, a video has at most MAX_GT segments and every segment has
    0 <= start < end <= T_v - 1.  ValueError names the first violation.  Returns (row_offset, gt_offset, gt) as int32 arrays."""
    ro, go = np.asarray(row_offset, dtype=np.int64).reshape(-1), np.asarray(gt_offset, dtype=np.int64).reshape(-1)
    g = np.asarray(gt, dtype=np.int64).reshape(-1, 2)
    if ro.size < 2 or ro.size != go.size:
        raise ValueError('row_offset and gt_offset must hold V + 1 entries each, V >= 1 (got %d and %d)' % (ro.size, go.size))
    if ro[0] != 0 or (np.diff(ro) < 1).any():
        raise ValueError('row_offset must start at 0 and grow strictly: every video has at least one feature row')
    if go[0] != 0 or (np.diff(go) < 0).any() or go[-1] != len(g):
        raise ValueError('gt_offset must start at 0, never decrease and end at the number of segments (%d)' % len(g))
    if ro[-1] >= 2 ** 31:
        raise ValueError('%d rows in one call (at most 2^31 - 1)' % ro[-1])
    for v in range(ro.size - 1):
        T, n = int(ro[v + 1] - ro[v]), int(go[v + 1] - go[v])
        if n > MAX_GT:
            raise ValueError('video %d has %d ground-truth segments (at most %d)' % (v, n, MAX_GT))
        for s, e in g[go[v]:go[v + 1]].tolist():
            if e <= s:
                raise ValueError('video %d: segment (%d, %d) has end <= start' % (v, s, e))
            if s < 0 or e > T - 1:
                raise ValueError('video %d: segment (%d, %d) lies outside the video (rows 0 .. %d)' % (v, s, e, T - 1))
    return ro.astype(np.int32), go.astype(np.int32), g.astype(np.int32)


def _video(vid, v):
    """(nfeats, featstamps) of a pair or a dict ('featstamps' plus 'nfeats', 'T_v' or the rows of 'c3d')."""
    if isinstance(vid, dict):
        if 'featstamps' not in vid:
            raise ValueError("video %d carries no 'featstamps'" % v)
        n = vid['nfeats'] if 'nfeats' in vid else (vid['T_v'] if 'T_v' in vid else len(vid['c3d']))
        return int(n), vid['featstamps']
    n, st = vid
    return int(n), st


class Targets(object):
    """The result of `build`.  Device tensors [T_tot, K] in the concatenated layout: iou fp32, gts_index int32, tap_masks fp32, tap_labels
    fp32, good_gt int32 (the ground-truth index at a good proposal, else -1).  Host: row_offset int32 [V + 1]; n_good, n_events int64 [V];
    per video v the event lists ind[v] = t, soi[v] = [t - k, t + 1], cg[v] = gt (int64 arrays, get_shuffle_list's layout; events='all' lists
    at most prop_sample_num of the n_events[v] good proposals); keep: the videos with at least one good proposal and more than one row
    (train.py:261 skips the others)."""

    def __init__(self, K, row_offset, iou, gts_index, tap_masks, tap_labels, good_gt, n_good, n_events, events, mode):
        self.K, self.row_offset, self.mode = int(K), row_offset, mode
        self.iou, self.gts_index, self.tap_masks, self.tap_labels, self.good_gt = iou, gts_index, tap_masks, tap_labels, good_gt
        self.n_good, self.n_events = n_good, n_events
        self.ind, self.soi, self.cg = [], [], []
        for v in range(len(n_good)):
            e = events[v, :min(int(n_events[v]), events.shape[1])].astype(np.int64)
            self.ind.append(e[:, 0].copy())
            self.soi.append(np.stack([e[:, 0] - e[:, 1], e[:, 0] + 1], 1))
            self.cg.append(e[:, 2].copy())
        self.keep = [v for v in range(len(n_good)) if n_good[v] > 0 and row_offset[v + 1] - row_offset[v] > 1]

    @property
    def n_videos(self):
        return len(self.n_good)

    def kept(self, x):
        """The rows of the kept videos of a concatenated [T_tot, ...] tensor, in order (the tensor itself when every video is kept)."""
        if len(self.keep) == self.n_videos:
            return x
        ro = self.row_offset
        if not self.keep:
            return x[:0]
        return torch.cat([x[int(ro[v]):int(ro[v + 1])] for v in self.keep], 0)

    def videos(self, videos, gt_labels, gt_masks):
        """The kept videos as the dicts VideoBatch.from_videos and JointBatchStep take: a copy of videos[v] with 'ind', 'soi',
        'labels' = gt_labels[v][cg] and 'masks' = gt_masks[v][cg] filled -- one caption row per listed event, the row of its ground truth."""
        out = []
        for v in self.keep:
            d = dict(videos[v])
            cg = self.cg[v]
            d['ind'], d['soi'] = self.ind[v], self.soi[v]
            d['labels'], d['masks'] = np.asarray(gt_labels[v])[cg], np.asarray(gt_masks[v])[cg]
            out.append(d)
        return out


def build(videos, K, iou_threshold=0.5, iou_threshold_good=0.8, prop_sample_num=64, seed=0, device=None, events='sampled', draw=None):
    """Targets of V videos.  `videos`: per video a pair (nfeats, featstamps) or a dict with 'featstamps' and 'nfeats' / 'T_v' / 'c3d';
    featstamps are integer (start, end) rows, local to the video, possibly none (a one-row video admits none).  `K` anchors per row.
    `prop_sample_num` in 1 .. 1024 caps every video's event list.  events='sampled': the training list, keyed by the 64-bit `seed` and per
    video by draw[v] (default: v) -- a new seed or draw id per iteration gives a new sample; events='all': every good proposal in (t, k) order
    (`*_select_list_eval`), cut at prop_sample_num with n_events the uncut count.

    The host checks its copies (check_offsets), uploads offsets, draw ids and segments in one copy, runs the two entries and reads n_good,
    n_events and the event lists in ONE device-to-host copy.  Returns Targets."""
    if events not in ('sampled', 'all'):
        raise ValueError("events must be 'sampled' or 'all' (got %r)" % (events,))
    K, cap = int(K), int(prop_sample_num)
    if not 1 <= K <= MAX_K:
        raise ValueError('K must be in [1, %d] (got %d)' % (MAX_K, K))
    if not 1 <= cap <= MAX_SAMPLE:
        raise ValueError('prop_sample_num must be in [1, %d] (got %d)' % (MAX_SAMPLE, cap))
    thr, thr_good = float(iou_threshold), float(iou_threshold_good)
    if not (thr > 0.0 and thr_good > 0.0):
        raise ValueError('the IoU thresholds must be positive (got %g, %g): an anchor outside the mask has IoU 0' % (thr, thr_good))
    pairs = [_video(vid, v) for v, vid in enumerate(videos)]
    V = len(pairs)
    if not 1 <= V <= MAX_VIDEOS:
        raise ValueError('between 1 and %d videos per call (got %d)' % (MAX_VIDEOS, V))
    stamps = [np.asarray(st, dtype=np.int64).reshape(-1, 2) for _, st in pairs]
    ro, go, gt = check_offsets(np.concatenate([[0], np.cumsum([n for n, _ in pairs])]), np.concatenate([[0], np.cumsum([len(s) for s in stamps])]),
                               np.concatenate(stamps, 0) if stamps else np.zeros((0, 2)))
    T, G = int(ro[-1]), int(go[-1])
    if T * K >= 2 ** 31:
        raise ValueError('T_tot * K = %d * %d cells in one call (below 2^31): split the videos over several calls' % (T, K))
    dr = np.arange(V, dtype=np.int64) if draw is None else np.asarray(draw, dtype=np.int64).reshape(-1)
    if dr.size != V or (dr < 0).any() or (dr >= 2 ** 31).any():
        raise ValueError('draw must hold one stream id in [0, 2^31) per video (%d videos)' % V)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    dev = torch.device('cuda') if device is None else torch.device(device)
    if dev.type != 'cuda':
        raise L.EchrHipError('targets.build runs on the GPU only (got %s); echr_amd has no CPU path' % dev)
    lib = L.load()
    with torch.cuda.device(dev):
        head = torch.from_numpy(np.concatenate([ro, go, dr.astype(np.int32), gt.reshape(-1)])).to(dev)          # one upload
        ro_d, go_d, dr_d, gt_d = head[:V + 1], head[V + 1:2 * V + 2], head[2 * V + 2:3 * V + 2], head[3 * V + 2:]
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        iou, masks, labels = torch.empty(T, K, **f32), torch.empty(T, K, **f32), torch.empty(T, K, **f32)
        index, good = torch.empty(T, K, **i32), torch.empty(T, K, **i32)
        out = torch.empty(2 * V + V * cap * 3, **i32)          # n_good | n_events | events: the call's one host read
        n_good, n_events, ev = out[:V], out[V:2 * V], out[2 * V:]
        st = L.stream_ptr()
        L.check(lib.echr_tap_targets_batch(ro_d.data_ptr(), go_d.data_ptr(), gt_d.data_ptr() if G else None, V, T, G,
                                           int(np.diff(go).max()), K, thr, thr_good, iou.data_ptr(), index.data_ptr(), masks.data_ptr(),
                                           labels.data_ptr(), good.data_ptr(), n_good.data_ptr(), st), 'tap_targets_batch')
        L.check(lib.echr_prop_events_batch(good.data_ptr(), ro_d.data_ptr(), V, T, K, cap, 1 if events == 'sampled' else 0, seed,
                                           dr_d.data_ptr(), ev.data_ptr(), n_events.data_ptr(), st), 'prop_events_batch')
        host = out.cpu().numpy()
    return Targets(K, ro, iou, index, masks, labels, good, host[:V].astype(np.int64), host[V:2 * V].astype(np.int64),
                   host[2 * V:].reshape(V, cap, 3), events)

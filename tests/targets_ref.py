"""The suite's own statement of proposal-target building (echr_tap_targets_batch / echr_prop_events_batch, include/echr_hip.h), in numpy on
the host: the float64 IoU of every anchor against every ground-truth segment in the stated operation order, the float32 thresholds, the
good-proposal list and the Philox sampling rule.  tests/golden/targets.npz (tools/make_golden_targets.py: the reference's own loops) pins
the matrices and the unsampled lists; the sampled list is this project's own rule and is stated here over philox.philox4x32_10."""
import numpy as np

from echr_amd import philox


def video_targets(T, K, stamps, iou_threshold=0.5, iou_threshold_good=0.8):
    """dict of one video's [T, K] matrices: iou float32, gts_index int32, tap_masks float32, tap_labels float32, good_gt int32, and n_good.
    `stamps`: integer (start, end) featstamps.  Broadcast over (t, k), a loop over the segments in order."""
    t = np.arange(T, dtype=np.float64)[:, None] + np.zeros((1, K))
    a = t - np.arange(K, dtype=np.float64)[None, :] - 1.0                 # the anchor is [a, t]
    valid = np.arange(T)[:, None] >= np.arange(K)[None, :] + 1
    best = np.zeros((T, K), np.float64)
    index = np.full((T, K), -1, np.int64)
    for i, (start, end) in enumerate(np.asarray(stamps, np.int64).reshape(-1, 2).tolist()):
        s, e = start - 0.01, end + 0.01
        inter = np.maximum(0.0, np.minimum(e, t) - np.maximum(s, a))
        union = np.minimum(np.maximum(e, t) - np.minimum(s, a), ((e - s) + t) - a)
        ov = inter / (union + 1e-8)
        take = ov >= best                                                  # a tie goes to the later segment
        best = np.where(take, ov, best)
        index = np.where(take, i, index)
    iou = np.where(valid, best, 0.0).astype(np.float32)
    gts_index = np.where(valid, index, 0).astype(np.int32)
    labels = iou >= np.float32(iou_threshold)
    good = valid & (iou >= np.float32(iou_threshold_good)) & (gts_index >= 0)
    good_gt = np.where(good, gts_index, -1).astype(np.int32)
    return dict(iou=iou, gts_index=gts_index, tap_masks=valid.astype(np.float32), tap_labels=labels.astype(np.float32), good_gt=good_gt,
                n_good=int(good.sum()))


def all_events(good_gt):
    """int64 [n_good, 3]: (t, k, gt) of every good proposal in row-major order."""
    t, k = np.nonzero(good_gt >= 0)
    return np.stack([t, k, good_gt[t, k]], 1).astype(np.int64)


def sample_words(positions, seed, draw):
    """uint32 words of the cells at flat `positions` p = t * K + k: output p & 3 of Philox-4x32-10 with counter (p >> 2, draw, SITE_PROP, 0)."""
    p = np.asarray(positions, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = np.stack(philox.philox4x32_10(p >> np.uint64(2), int(draw), philox.SITE_PROP, 0, seed & 0xFFFFFFFF, seed >> 32), axis=-1)
    return w[np.arange(len(p)), (p & np.uint64(3)).astype(np.int64)]


def sampled_events(good_gt, cap, seed, draw):
    """int64 [min(n_good, cap), 3]: the good proposals with the smallest (word, position), in ascending (word, position) order."""
    K = good_gt.shape[1]
    ev = all_events(good_gt)
    p = ev[:, 0] * K + ev[:, 1]
    w = sample_words(p, seed, draw)
    order = np.lexsort((p, w))[:min(len(p), int(cap))]
    return ev[order]


def lists(ev):
    """(ind, soi, cg) of an event array: get_shuffle_list's layout."""
    return ev[:, 0].copy(), np.stack([ev[:, 0] - ev[:, 1], ev[:, 0] + 1], 1), ev[:, 2].copy()

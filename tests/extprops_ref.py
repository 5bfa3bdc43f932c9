"""The suite's own statement of the external-proposal selection (echr_nms_segments_batch / echr_ext_proposals_batch, include/echr_hip.h),
on the host, composed of what is already pinned to the reference: eval_utils.gettopN_nms (tests/golden/proposals.npz and extprops.npz:
the reference's own picks), targets.featstamps (Python 2 rounding, a literal table in tests/test_targets_host.py), philox.philox4x32_10
(the Random123 known answers) for the crop draw, and the literal filter loop of the reference's eval_utils.py:88-104."""
import numpy as np

from echr_amd import eval_utils as EU
from echr_amd import philox, targets

CROP_SEED, CROP_DRAW = 0x0123ABCD5EED4567, 5          # the key of the crop-uniformity check (both halves of the seed are non-zero)


def nms(props, prop_scores, sent_score, nms_overlap, topN=1000):
    """The picks of eval_utils.gettopN_nms in round order (a list of ints); none for an empty list."""
    if len(prop_scores) == 0:
        return []
    return [int(i) for i in EU.gettopN_nms(np.asarray(props, np.float64).reshape(-1, 2), np.asarray(prop_scores, np.float64),
                                           np.asarray(sent_score, np.float64), nms_overlap=nms_overlap, topN=topN)[2]]


def overlap(a, b):
    """o of two segments in the reference's operation order (eval_utils.py:239-246), float64."""
    (a1, a2), (b1, b2) = (np.float64(x) for x in a), (np.float64(x) for x in b)
    wh = np.maximum(0., np.minimum(a2, b2) - np.maximum(a1, b1) + 1e-3)
    return wh / ((a2 - a1 + 1e-3) + (b2 - b1 + 1e-3) - wh)


def crop_words(index, seed, draw):
    """uint64 words of the proposals at video-local `index`: output i & 3 of Philox-4x32-10 with counter (i >> 2, draw, SITE_CROP, 0)."""
    i = np.asarray(index, dtype=np.uint64).reshape(-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = np.stack(philox.philox4x32_10(i >> np.uint64(2), int(draw), philox.SITE_CROP, 0, seed & 0xFFFFFFFF, seed >> 32), axis=-1)
    return w[np.arange(len(i)), (i & np.uint64(3)).astype(np.int64)].astype(np.uint64)


def crop(s, e, K, word):
    """dataloader.py:515-520 with the project's draw: rows (s, e) with e - s >= K + 1 are cut to K rows at offset (word * n) >> 32 of the
    n = e - s - K + 1 admissible ones."""
    if e - s >= K + 1:
        s = s + ((int(word) * (e - s - K + 1)) >> 32)
        e = s + K
    return s, e


def select(video, K, topN=1000, nms_threshold=0.0, val_score_thres=0.0, nms_rounds=1000, seed=0, draw=0, do_crop=True):
    """One video's selection: dict of pick (kept original indices), ind, soi (int64), scores, timestamps (float64).  `video`: 'SOTA_timestamps',
    'SOTA_Prop_score' (None: a bad video, nothing), 'duration', 'nfeats'."""
    scores, T = video.get('SOTA_Prop_score'), int(video['nfeats'])
    kept = []
    if scores is not None and T > 1:
        stamps = np.asarray(video['SOTA_timestamps'], np.float64).reshape(-1, 2)
        scores = np.asarray(scores, np.float64).reshape(-1)
        if nms_threshold > 0:                                      # eval_utils.py:88-91
            pick = set(nms(stamps, scores, scores, nms_threshold, nms_rounds))
        else:
            pick = set(range(len(scores)))
        for i, p_score in enumerate(scores):                       # eval_utils.py:93-104
            if i not in pick:
                continue
            if p_score >= val_score_thres:
                kept.append(i)
            if len(kept) >= topN:
                break
    kept = np.asarray(kept, np.int64)
    if not len(kept):
        return dict(pick=kept, ind=np.zeros(0, np.int64), soi=np.zeros((0, 2), np.int64), scores=np.zeros(0), timestamps=np.zeros((0, 2)))
    feat = targets.featstamps(stamps[kept].tolist(), T, float(video['duration']))
    if do_crop:
        feat = [crop(s, e, K, w) for (s, e), w in zip(feat, crop_words(kept, seed, draw))]
    feat = np.asarray(feat, np.int64).reshape(-1, 2)
    return dict(pick=kept, ind=feat[:, 1].copy(), soi=np.stack([feat[:, 0], feat[:, 1] + 1], 1), scores=scores[kept], timestamps=stamps[kept])

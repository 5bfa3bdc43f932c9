#!/usr/bin/env python3
"""Generate the fixture of proposal-target building from the REFERENCE's own code (build container only; CPU).

Runs dataloader.DataLoader.get_vid_data (with its iou) and get_shuffle_list on a handful of small videos and writes
tests/golden/targets.npz -- data only:

    n | iou_threshold | iou_threshold_good
    c<i>|T  c<i>|K  c<i>|stamps [G, 2] (integer featstamps)
    c<i>|iou_scores [T, K] f32 | c<i>|tap_masks [T, K] f32 | c<i>|gts_index [T, K] f32 (as the reference stores it)
    c<i>|tap_gts_for_good_proposal [T, K] int64 (dataloader.py:109,124 on the arrays above)
    c<i>|ind [n] | c<i>|cg [n] | c<i>|soi [n, 2]          get_shuffle_list's unsampled lists (`*_select_list_eval`)

The cases start from featstamps, not timestamps: the reference is Python 2 code and its round() differs from Python 3's at exact halves,
which stays out of the fixture (echr_amd.targets.featstamps states the Python 2 rule and is tested against a literal table).

The reference module is imported in place (nothing of it is copied).  It imports cPickle, h5py and pandas at module level and uses xrange:
empty stand-in modules are put into sys.modules, xrange = range is set in the imported module, and the methods are called on a stub
object that carries the few attributes they read.  The sampled list (np.random.shuffle) is not recorded: the project samples with its own
counter-based generator (tests/targets_ref.py).

The tool asserts that no IoU lies within 1e-6 of either threshold, so that a threshold flip cannot hide behind rounding.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_targets.py --reference <checkout of the reference>
        (or ECHR_REFERENCE in the environment)
"""
import argparse
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
IOU_THRESHOLD, IOU_THRESHOLD_GOOD = 0.5, 0.8          # opts.py defaults

# (T, K, featstamps): T < K, T = K, T = K + 1, one and two rows, no annotation, identical segments (the tie goes to the later index), a
# segment that overlaps no anchor of most rows (the all-zero rows get G - 1), K on and off a wave
CASES = [
    (40, 16, [(3, 9), (3, 9), (20, 31), (36, 38)]),
    (5, 8, [(0, 3)]),
    (8, 8, [(1, 6), (2, 4)]),
    (9, 8, [(0, 7), (5, 8)]),
    (1, 5, []),
    (2, 5, [(0, 1)]),
    (30, 5, []),
    (70, 64, [(0, 12), (10, 40), (10, 40), (33, 69), (50, 51), (2, 66)]),
    (96, 32, [(5, 20), (18, 30), (60, 95), (61, 94), (40, 41)]),
]


def load_reference(ref):
    for name in ('cPickle', 'h5py', 'pandas'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, ref)
    import dataloader as DL          # (reference)
    DL.xrange = range
    return DL


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('ECHR_REFERENCE'))
    a = ap.parse_args()
    if not a.reference or not os.path.exists(os.path.join(a.reference, 'dataloader.py')):
        raise SystemExit('--reference (or ECHR_REFERENCE) must name a checkout of the reference')
    DL = load_reference(a.reference)

    class Stub(object):
        iou = DL.DataLoader.iou
        get_vid_data = DL.DataLoader.get_vid_data
        get_shuffle_list = DL.DataLoader.get_shuffle_list
        use_SOTA_tep = False
        prop_sample_num = 64

        def timestamp_to_featstamp(self, timestamp, nfeats, duration):          # the cases ARE featstamps
            return int(timestamp[0]), int(timestamp[1])

    out = {'n': np.int64(len(CASES)), 'iou_threshold': np.float64(IOU_THRESHOLD), 'iou_threshold_good': np.float64(IOU_THRESHOLD_GOOD)}
    for i, (T, K, stamps) in enumerate(CASES):
        s = Stub()
        s.K = K
        s.data = {'v': {'duration': float(T), 'timestamps': [list(x) for x in stamps]}}
        iou_scores, tap_masks, gts_index, featstamps, _ = s.get_vid_data('v', T)
        assert [tuple(f) for f in featstamps] == [tuple(x) for x in stamps]
        for thr in (IOU_THRESHOLD, IOU_THRESHOLD_GOOD):
            assert (np.abs(iou_scores.astype(np.float64) - thr) > 1e-6).all(), (i, thr)
        good = (iou_scores >= IOU_THRESHOLD_GOOD)                                  # dataloader.py:109
        tap_gts = (good * (gts_index + 1) - 1).astype('int')                       # dataloader.py:124
        np.random.seed(0)
        tap_list, lm_list, soi_list, _ = s.get_shuffle_list(tap_gts, featstamps, method='random')
        n = len(tap_list)
        print('[case %d] T %d K %d G %d: %d labels, %d good proposals' % (i, T, K, len(stamps), int((iou_scores >= IOU_THRESHOLD).sum()), n))
        p = 'c%d|' % i
        out.update({p + 'T': np.int64(T), p + 'K': np.int64(K), p + 'stamps': np.asarray(stamps, np.int64).reshape(-1, 2),
                    p + 'iou_scores': iou_scores, p + 'tap_masks': tap_masks, p + 'gts_index': gts_index,
                    p + 'tap_gts_for_good_proposal': tap_gts.astype(np.int64),
                    p + 'ind': np.asarray(tap_list, np.int64).reshape(-1), p + 'cg': np.asarray(lm_list, np.int64).reshape(-1),
                    p + 'soi': np.asarray(soi_list, np.int64).reshape(-1, 2)})
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, 'targets.npz')
    np.savez_compressed(path, **out)
    print('wrote targets.npz (%d bytes)' % os.path.getsize(path))


if __name__ == '__main__':
    main()

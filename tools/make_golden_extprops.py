#!/usr/bin/env python3
"""Generate the fixture of the external-proposal NMS from the REFERENCE's own code (build container only; CPU).

Runs eval_utils.gettopN_nms (eval_utils.py:230-256) on seeded lists of real-valued segments and writes tests/golden/extprops.npz -- data
only:

    n
    c<i>|stamps [P, 2] f32 (seconds; the test widens them to float64, which is exact)   c<i>|pscore [P] f32   c<i>|sscore [P] f32
    c<i>|thr (float64)   c<i>|topN
    c<i>|pick_p   the reference's picks with sent_score = prop_scores (the SOTA_TEP call, eval_utils.py:89)
    c<i>|pick_s   the reference's picks with the separate sent_score

P = 1, 2, 7, 1023, 1025 and 1100.  The P = 1100 case is pairwise disjoint segments: nothing is ever suppressed but the best itself, so the
1000-round cap of the SOTA_TEP call bites.  Scores are distinct (the reference's argsort is unstable on ties).  The tool asserts that no
pairwise o lies within 1e-9 of the case's threshold, so that a flip cannot hide behind rounding.

The reference module is imported in place (nothing of it is copied), the way tools/make_golden.py do_proposals does.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_extprops.py --reference <checkout of the reference>
        (or ECHR_REFERENCE in the environment)
"""
import argparse
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')

# (P, threshold, topN, disjoint)
CASES = [(1, 0.5, 1000, False), (2, 0.5, 1000, False), (7, 0.3, 1000, False), (1023, 0.8, 1000, False), (1025, 0.5, 1000, False),
         (1100, 0.7, 1000, True)]


def make_case(i, P, disjoint):
    rs = np.random.RandomState(500 + i)
    if disjoint:
        start = np.arange(P) * 3.0 + rs.uniform(0.0, 0.5, size=P)
        stamps = np.stack([start, start + rs.uniform(0.5, 2.0, size=P)], 1)[rs.permutation(P)]
    else:
        start = rs.uniform(0.0, 180.0, size=P)
        stamps = np.stack([start, start + rs.uniform(0.5, 60.0, size=P)], 1)
    stamps = stamps.astype(np.float32)
    pscore = ((rs.permutation(P) + 1.0) / P).astype(np.float32)
    sscore = (-(rs.permutation(P) + 1.0) / 7.0).astype(np.float32)
    assert len(np.unique(pscore)) == P and len(np.unique(sscore)) == P and (stamps[:, 1] > stamps[:, 0]).all()
    return stamps, pscore, sscore


def margin(stamps, thr):
    """The smallest |o - thr| over all pairs, in the reference's operation order."""
    t1, t2 = stamps[:, 0], stamps[:, 1]
    area = t2 - t1 + 1e-3
    best = np.inf
    for i in range(len(t1)):
        wh = np.maximum(0., np.minimum(t2[i], t2) - np.maximum(t1[i], t1) + 1e-3)
        best = min(best, float(np.abs(wh / (area[i] + area - wh) - thr).min()))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('ECHR_REFERENCE'))
    a = ap.parse_args()
    if not a.reference or not os.path.exists(os.path.join(a.reference, 'eval_utils.py')):
        raise SystemExit('--reference (or ECHR_REFERENCE) must name a checkout of the reference')
    sys.path.insert(0, a.reference)
    import eval_utils as ref_eval          # (reference)

    out = {'n': np.int64(len(CASES))}
    for i, (P, thr, topN, disjoint) in enumerate(CASES):
        stamps, pscore, sscore = make_case(i, P, disjoint)
        st, ps, ss = stamps.astype(np.float64), pscore.astype(np.float64), sscore.astype(np.float64)
        m = margin(st, thr)
        assert m > 1e-9, (i, m)
        pick_p = ref_eval.gettopN_nms(st, ps, ps, nms_overlap=thr, topN=topN)[2]
        pick_s = ref_eval.gettopN_nms(st, ps, ss, nms_overlap=thr, topN=topN)[2]
        if disjoint:
            assert len(pick_p) == topN < P
        print('[case %d] P %d thr %g: %d / %d picks, smallest |o - thr| %.3e' % (i, P, thr, len(pick_p), len(pick_s), m))
        p = 'c%d|' % i
        out.update({p + 'stamps': stamps, p + 'pscore': pscore, p + 'sscore': sscore, p + 'thr': np.float64(thr), p + 'topN': np.int64(topN),
                    p + 'pick_p': np.asarray(pick_p, np.int32), p + 'pick_s': np.asarray(pick_s, np.int32)})
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, 'extprops.npz')
    np.savez_compressed(path, **out)
    print('wrote extprops.npz (%d bytes)' % os.path.getsize(path))


if __name__ == '__main__':
    main()

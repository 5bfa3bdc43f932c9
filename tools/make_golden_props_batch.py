#!/usr/bin/env python3
"""Generate the fixture of the batched proposal selection from the REFERENCE's own code (build container only).

One batch of five videos with a shared K (lengths 1, 40, 7, 24, 96; K = 32): the reference's gettop1000 (eval_utils.py:259-287) and
gettop1000_nms (:290-331) run VIDEO BY VIDEO on the video's own rows, their outputs concatenated in video order -- what
echr_top_proposals_batch / echr_top_proposals_nms_batch must reproduce in one launch.  Writes tests/golden/props_batch.npz:

    lengths | K
    t<i>|scores [T_tot,K] | t<i>|topN | t<i>|thres | t<i>|count [V] | t<i>|ind [N] | t<i>|feat [N,2] | t<i>|conf [N]      threshold cases
    n|scores [T_tot,K] | n<j>|overlap | n<j>|topN | n<j>|count [V] | n<j>|props [N,2] | n<j>|conf [N]                     NMS cases

Threshold cases: 0 plain (topN 50), 1 scores quantised to 1/16 (ties push counts above topN), 2 a val_score_thres above every score of
video 2 (an empty video in the middle), 3 topN = 100000 (more than any video has).  The mask is the causal one, n_local >= k.
NMS grids use distinct scores per video (a permutation / size), as tools/make_golden.py::do_proposals does: the reference's argsort is
unstable on ties.  The reference's gettop1000_nms cannot run on a one-row video (it indexes an empty candidate array; eval_split skips such
videos, eval_utils.py:44): its count is recorded as 0.  Every video is also checked against oracle.top_proposals / top_proposals_nms.

The reference is imported in place through tools/make_golden.py (nothing of it is copied).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_props_batch.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG                     # noqa: E402  (imports the reference)

O, ref_eval = MG.O, MG.ref_eval
LENGTHS, K = (1, 40, 7, 24, 96), 32
F2T = lambda s, e, n, d: [s, e]


def causal(T):
    return (np.arange(T)[:, None] >= np.arange(K)[None, :]).astype(np.float32)


def main():
    ro = np.concatenate([[0], np.cumsum(LENGTHS)])
    T_tot = int(ro[-1])
    out = {'lengths': np.array(LENGTHS, np.int64), 'K': np.int64(K)}
    rs = np.random.RandomState(700)
    base = rs.uniform(0, 1, size=(T_tot, K)).astype(np.float32)
    quant = (np.round(rs.uniform(0, 1, size=(T_tot, K)) * 16) / 16).astype(np.float32)
    above_v2 = float((base[ro[2]:ro[3]] * causal(LENGTHS[2])).max()) + 1e-3
    for i, (scores, topN, thres) in enumerate(((base, 50, 0.0), (quant, 50, 0.0), (base, 50, above_v2), (base, 100000, 0.0))):
        cnt, inds, feats, confs = [], [], [], []
        for v, T in enumerate(LENGTHS):
            sc, m = scores[ro[v]:ro[v + 1]], causal(T)
            ind, feat, _, _, conf = ref_eval.gettop1000(sc, m, [], 100.0, F2T, val_score_thres=thres, topN=topN)
            oind, ofeat, oconf = O.top_proposals(sc, m, topN, thres)
            assert ind == oind and feat == ofeat and np.array_equal(np.float32(conf), np.float32(oconf)), (i, v)
            cnt.append(len(ind)); inds += ind; feats += feat; confs += conf
        print('[threshold %d] topN %d thres %.4f counts %s' % (i, topN, thres, cnt))
        out['t%d|scores' % i] = scores
        out['t%d|topN' % i] = np.int64(topN)
        out['t%d|thres' % i] = np.float32(thres)
        out['t%d|count' % i] = np.array(cnt, np.int64)
        out['t%d|ind' % i] = np.array(inds, np.int64)
        out['t%d|feat' % i] = np.array(feats, np.int64).reshape(-1, 2)
        out['t%d|conf' % i] = np.array(confs, np.float32)
    assert out['t1|count'].max() > 50 and out['t2|count'][2] == 0 and out['t2|count'][3] > 0
    rs = np.random.RandomState(710)
    nsc = np.concatenate([rs.permutation(T * K).reshape(T, K).astype(np.float32) / np.float32(T * K) for T in LENGTHS], 0)
    out['n|scores'] = nsc
    for j, (ov, topN) in enumerate(((0.5, 12), (0.5, 1000), (0.9, 12), (0.9, 1000))):
        cnt, props, confs = [], [], []
        for v, T in enumerate(LENGTHS):
            sc = nsc[ro[v]:ro[v + 1]]
            _, oprops, osc = O.top_proposals_nms(sc, ov, topN)
            if T > 1:
                ind, rprops, _, _, rsc = ref_eval.gettop1000_nms(sc, None, [], 100.0, F2T, overlap=ov, topN=topN)
                assert np.array_equal(rprops, oprops) and np.array_equal(rsc, osc) and np.array_equal(ind, oprops[:, 1] - 1), (j, v)
                cnt.append(len(rprops)); props.append(np.asarray(rprops, np.int64)); confs.append(np.asarray(rsc, np.float64))
            else:
                assert len(osc) == 0
                cnt.append(0)
        print('[nms %d] overlap %.2f topN %d counts %s' % (j, ov, topN, cnt))
        out['n%d|overlap' % j] = np.float64(ov)
        out['n%d|topN' % j] = np.int64(topN)
        out['n%d|count' % j] = np.array(cnt, np.int64)
        out['n%d|props' % j] = np.concatenate(props, 0)
        out['n%d|conf' % j] = np.concatenate(confs, 0)
    path = os.path.join(MG.GOLD, 'props_batch.npz')
    np.savez_compressed(path, **out)
    print('wrote props_batch.npz (%d bytes)' % os.path.getsize(path))


if __name__ == '__main__':
    main()

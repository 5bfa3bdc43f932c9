"""Proposal-target building (echr_amd.targets, csrc/targets.hip) without a GPU: the suite's oracle against the reference's recorded outputs,
featstamps against a literal table, the sampling rule's properties, the ABI and every refusal that runs ahead of the launches."""
import os
import re

import numpy as np
import pytest
import torch

from tests import targets_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'targets.npz')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _cases(z):
    for i in range(int(z['n'])):
        p = 'c%d|' % i
        yield i, int(z[p + 'T']), int(z[p + 'K']), z[p + 'stamps'], {k[len(p):]: z[k] for k in z.files if k.startswith(p)}


def test_oracle_equals_the_reference_exactly(gold):
    thr, good = float(gold['iou_threshold']), float(gold['iou_threshold_good'])
    seen_tie = seen_empty = seen_short = False
    for i, T, K, stamps, ref in _cases(gold):
        o = R.video_targets(T, K, stamps, thr, good)
        assert np.array_equal(o['iou'].view(np.uint32), ref['iou_scores'].view(np.uint32)), i
        assert np.array_equal(o['tap_masks'], ref['tap_masks']), i
        assert np.array_equal(o['gts_index'], ref['gts_index'].astype(np.int32)), i
        assert np.array_equal(o['tap_labels'], (ref['iou_scores'] >= thr).astype(np.float32)), i          # dataloader.py:107
        assert np.array_equal(o['good_gt'], ref['tap_gts_for_good_proposal']), i
        ev = R.all_events(o['good_gt'])
        ind, soi, cg = R.lists(ev)
        assert np.array_equal(ind, ref['ind']) and np.array_equal(soi, ref['soi']) and np.array_equal(cg, ref['cg']), i
        assert o['n_good'] == len(ref['ind'])
        st = [tuple(s) for s in stamps.tolist()]
        if len(set(st)) < len(st):          # identical segments: the later index wins everywhere
            first = min(j for j, s in enumerate(st) if st.count(s) > 1)
            assert not (ref['gts_index'][ref['tap_masks'] > 0] == first).any()
            seen_tie = True
        if len(st) == 0:
            assert (ref['gts_index'][ref['tap_masks'] > 0] == -1).all() and o['n_good'] == 0
            seen_empty = True
        if len(st) and ((ref['iou_scores'] == 0) & (ref['tap_masks'] > 0)).any():          # an anchor that overlaps nothing gets G - 1
            z = (ref['iou_scores'] == 0) & (ref['tap_masks'] > 0)
            assert (ref['gts_index'][z] == len(st) - 1).all()
        seen_short = seen_short or T < K
    assert seen_tie and seen_empty and seen_short


def test_no_fixture_iou_sits_at_a_threshold(gold):
    """A threshold flip cannot hide behind rounding: every recorded IoU is further than 1e-6 from both thresholds."""
    for i, T, K, stamps, ref in _cases(gold):
        for thr in (float(gold['iou_threshold']), float(gold['iou_threshold_good'])):
            assert (np.abs(ref['iou_scores'].astype(np.float64) - thr) > 1e-6).all(), (i, thr)


def test_featstamps_table():
    from echr_amd import targets as TG
    table = [  # (timestamp, nfeats, duration) -> featstamp; x / 8 * 8 and x / 8 * 16 are exact
        ((2.5, 6.5), 8, 8.0, (3, 7)),          # exact halves go away from zero (Python 3's round gives 2, 6)
        ((0.5, 1.5), 8, 8.0, (1, 2)),          # (Python 3: 0, 2)
        ((1.5, 2.5), 8, 8.0, (2, 3)),
        ((1.25, 3.75), 16, 8.0, (3, 8)),       # 2.5 and 7.5 rows
        ((3.49, 3.51), 8, 8.0, (3, 4)),
        ((7.9, 20.0), 8, 8.0, (6, 7)),         # start clamped to nfeats - 2, end to nfeats - 1
        ((-3.0, 0.2), 8, 8.0, (0, 1)),         # start clamped to 0, end lifted to start + 1
        ((4.0, 4.0), 8, 8.0, (4, 5)),
        ((0.0, 8.0), 8, 8.0, (0, 7)),
    ]
    for ts, n, d, want in table:
        assert TG.featstamps([ts], n, d) == [want], ts
    assert TG.featstamps([t[0] for t in table[:3]], 8, 8.0) == [t[3] for t in table[:3]]
    assert 'Python 2' in TG.featstamps.__doc__ and 'half away from zero' in TG.featstamps.__doc__
    ev = TG.gt_events([(3, 7), (0, 2)])
    assert ev['cg'].tolist() == [0, 1] and ev['ind'].tolist() == [7, 2] and ev['soi'].tolist() == [[3, 8], [0, 3]]


def test_sampling_rule(gold):
    from echr_amd import philox
    assert philox.SITE_PROP == 7
    i, T, K, stamps, ref = [c for c in _cases(gold) if c[1] == 70][0]
    good_gt = ref['tap_gts_for_good_proposal']
    every = {tuple(e) for e in R.all_events(good_gt).tolist()}
    n = len(every)
    assert n > 64
    for cap in (1, 64, n, n + 5, 1024):
        ev = R.sampled_events(good_gt, cap, seed=5, draw=0)
        assert len(ev) == min(n, cap) and len({tuple(e) for e in ev.tolist()}) == len(ev)
        assert {tuple(e) for e in ev.tolist()} <= every
        p = ev[:, 0] * K + ev[:, 1]
        key = (R.sample_words(p, 5, 0).astype(np.uint64) << np.uint64(32)) + p.astype(np.uint64)
        assert (key[1:] > key[:-1]).all()                                   # ascending (word, position)
        rest = np.array([e[0] * K + e[1] for e in every - {tuple(e) for e in ev.tolist()}], np.int64)
        if len(rest):                                                      # nothing left out has a smaller key
            assert ((R.sample_words(rest, 5, 0).astype(np.uint64) << np.uint64(32)) + rest.astype(np.uint64)).min() > key.max()
    a = R.sampled_events(good_gt, 64, seed=5, draw=0)
    assert not np.array_equal(a, R.sampled_events(good_gt, 64, seed=6, draw=0))
    assert not np.array_equal(a, R.sampled_events(good_gt, 64, seed=5, draw=1))
    assert not np.array_equal(a, R.sampled_events(good_gt, 64, seed=5 + (1 << 32), draw=0))          # the high half of the seed is part of the key
    assert np.array_equal(a, R.sampled_events(good_gt, 64, seed=5, draw=0))
    # the words are the documented counter layout
    w = philox.philox4x32_10(np.array([9 >> 2], np.uint32), 3, 7, 0, 5, 0)
    assert int(R.sample_words([9], 5, 3)[0]) == int(w[9 & 3][0])


ENTRIES = ('echr_tap_targets_batch', 'echr_prop_events_batch')


def test_new_symbols_are_declared_bound_and_exported():
    from echr_amd import _lib, build, targets as TG
    assert 'targets.hip' in build.SOURCES
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'echr_hip.h')).read()
    declared = set(re.findall(r'\b(echr_[a-z0-9_]+)\s*\(', hdr))
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert name in declared and name in bound and hasattr(lib, name), name
    for macro, value in (('TARGETS_MAX_GT', TG.MAX_GT), ('PROP_MAX_SAMPLE', TG.MAX_SAMPLE), ('TARGETS_MAX_VIDEOS', TG.MAX_VIDEOS),
                         ('TARGETS_MAX_K', TG.MAX_K)):
        assert int(re.search(r'#define ECHR_%s (\d+)' % macro, hdr).group(1)) == value
    common = open(os.path.join(ROOT, 'echr_amd', 'csrc', 'echr_common.h')).read()
    assert re.search(r'SITE_PROP\s*=\s*7u?;', common)


def test_entry_points_validate_before_any_launch():
    """The argument checks run on the host ahead of the launches: they need no GPU."""
    from echr_amd import _lib
    lib = _lib.load()
    tgt, evt = lib.echr_tap_targets_batch, lib.echr_prop_events_batch
    err = lambda: lib.echr_last_error()
    N = None

    def targets(V=1, T=4, G=1, Gmax=1, K=4, thr=0.5, good=0.8):
        return tgt(N, N, N, V, T, G, Gmax, K, thr, good, N, N, N, N, N, N, N)

    def events(V=1, T=4, K=4, cap=64, sampled=1):
        return evt(N, N, V, T, K, cap, sampled, 0, N, N, N, N)

    for fn, name in ((targets, b'echr_tap_targets_batch'), (events, b'echr_prop_events_batch')):
        assert fn(V=0) == -22 and name in err() and b'videos' in err()
        assert fn(V=65536, T=65536) == -22 and b'videos' in err()
        assert fn(K=0) == -22 and b'K = 0' in err()
        assert fn(K=65537) == -22 and b'K = 65537' in err()
        assert fn(V=3, T=2) == -22 and b'T_tot' in err()
        assert fn(T=1 << 20, K=1 << 11) == -22 and b'2^31' in err()
        assert fn() == -22 and b'required' in err()                    # null pointers
    assert targets(G=1, Gmax=2) == -22 and b'G_max' in err()
    assert targets(G=-1, Gmax=0) == -22 and b'G_tot' in err()
    assert targets(G=2000, Gmax=1025) == -22 and b'at most 1024' in err()
    assert targets(thr=0.0) == -22 and b'positive' in err()
    assert targets(good=-1.0) == -22 and b'positive' in err()
    for cap in (0, -1, 1025):
        assert events(cap=cap) == -22 and b'prop_sample_num' in err()
    assert events(sampled=2) == -22 and b'sampled' in err()


def test_host_refusals_by_name():
    from echr_amd import targets as TG
    from echr_amd._lib import EchrHipError
    ok = TG.check_offsets([0, 4, 9], [0, 1, 1], [[0, 3]])
    assert [a.dtype for a in ok] == [np.int32] * 3 and ok[2].shape == (1, 2)
    with pytest.raises(ValueError, match='row_offset must start at 0 and grow'):
        TG.check_offsets([0, 4, 4], [0, 1, 1], [[0, 3]])
    with pytest.raises(ValueError, match='row_offset must start at 0 and grow'):
        TG.check_offsets([1, 4], [0, 0], [])
    with pytest.raises(ValueError, match='gt_offset must start at 0, never decrease'):
        TG.check_offsets([0, 4, 9], [0, 1, 0], [[0, 3]])
    with pytest.raises(ValueError, match='gt_offset must start at 0, never decrease'):
        TG.check_offsets([0, 4], [0, 2], [[0, 3]])
    with pytest.raises(ValueError, match='V \\+ 1 entries'):
        TG.check_offsets([0, 4, 9], [0, 1], [[0, 3]])
    with pytest.raises(ValueError, match='end <= start'):
        TG.check_offsets([0, 4], [0, 1], [[2, 2]])
    with pytest.raises(ValueError, match='end <= start'):
        TG.build([(9, [(5, 3)])], K=4)
    with pytest.raises(ValueError, match='outside the video'):
        TG.build([(9, [(5, 9)])], K=4)                                # end = T: the last row is T - 1
    with pytest.raises(ValueError, match='outside the video'):
        TG.build([(9, [(0, 3)]), (4, [(-1, 2)])], K=4)
    with pytest.raises(ValueError, match='outside the video'):
        TG.build([(1, [(0, 1)])], K=4)                                # a one-row video admits no segment
    with pytest.raises(ValueError, match='grow strictly'):
        TG.build([(9, []), (0, [])], K=4)
    for cap in (0, 1025):
        with pytest.raises(ValueError, match='prop_sample_num must be in \\[1, 1024\\]'):
            TG.build([(9, [(0, 3)])], K=4, prop_sample_num=cap)
    with pytest.raises(ValueError, match='1025 ground-truth segments'):
        TG.build([(2000, [(i, i + 1) for i in range(1025)])], K=4)
    with pytest.raises(ValueError, match='K must be'):
        TG.build([(9, [(0, 3)])], K=0)
    with pytest.raises(ValueError, match='positive'):
        TG.build([(9, [(0, 3)])], K=4, iou_threshold_good=0.0)
    with pytest.raises(ValueError, match="'sampled' or 'all'"):
        TG.build([(9, [(0, 3)])], K=4, events='some')
    with pytest.raises(ValueError, match='draw'):
        TG.build([(9, [(0, 3)])], K=4, draw=[0, 1])
    with pytest.raises(ValueError, match='at least 1|between 1 and'):
        TG.build([], K=4)
    with pytest.raises(EchrHipError, match='GPU only'):               # behind every host check, ahead of any device work
        TG.build([(9, [(0, 3)])], K=4, device='cpu')


def test_targets_videos_drops_videos_without_a_good_proposal():
    from echr_amd import targets as TG
    K, cap = 4, 3
    ro = np.array([0, 5, 6, 12, 20], np.int32)                        # video 1 has one row; video 2 no good proposal
    n_good = np.array([2, 0, 0, 5], np.int64)
    n_events = np.array([2, 0, 0, 3], np.int64)
    ev = -np.ones((4, cap, 3), np.int32)
    ev[0, :2] = [[4, 1, 1], [3, 0, 0]]
    ev[3] = [[7, 3, 0], [5, 0, 2], [6, 2, 0]]
    x = torch.arange(20 * K, dtype=torch.float32).reshape(20, K)
    t = TG.Targets(K, ro, x, x.int(), x, x, x.int(), n_good, n_events, ev, 'sampled')
    assert t.keep == [0, 3] and t.n_videos == 4
    assert t.ind[0].tolist() == [4, 3] and t.soi[0].tolist() == [[3, 5], [3, 4]] and t.cg[0].tolist() == [1, 0]
    assert t.ind[1].size == 0 and t.soi[2].shape == (0, 2)
    assert t.soi[3].tolist() == [[4, 8], [5, 6], [4, 7]]
    assert torch.equal(t.kept(x), torch.cat([x[0:5], x[12:20]]))
    vids = [dict(c3d=np.zeros((int(ro[v + 1] - ro[v]), 2), np.float32), lda=np.zeros(3, np.float32), name=v) for v in range(4)]
    labels = [np.arange(3 * 6).reshape(3, 6) + 100 * v for v in range(4)]
    masks = [np.ones((3, 6), np.float32) * v for v in range(4)]
    out = t.videos(vids, labels, masks)
    assert [d['name'] for d in out] == [0, 3]
    assert np.array_equal(out[0]['labels'], labels[0][[1, 0]]) and np.array_equal(out[1]['labels'], labels[3][[0, 2, 0]])
    assert np.array_equal(out[1]['masks'], masks[3][[0, 2, 0]]) and np.array_equal(out[1]['ind'], [7, 5, 6])
    assert 'ind' not in vids[0]                                       # the callers' dicts are left alone
    y = x[:5]
    every = TG.Targets(K, ro[:2], y, y.int(), y, y, y.int(), n_good[:1], n_events[:1], ev[:1], 'all')
    assert every.keep == [0] and every.kept(y) is y                   # every video kept: no copy

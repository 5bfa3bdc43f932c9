"""Host-side contract of the batched evaluation pass (no GPU): the two exports of the batched proposal selection, tests/props_batch_ref.py
against the reference's own per-video outputs (tests/golden/props_batch.npz, tools/make_golden_props_batch.py), the run cutting of
VideoBatch.event_groups, and the argument checks of forward_batch(event_group_rows=) / eval_utils.caption_videos."""
import os
import re

import numpy as np
import pytest
import torch

from echr_amd import _lib, synth
from echr_amd.batch import VideoBatch
from tests import props_batch_ref as R
from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ('echr_top_proposals_batch', 'echr_top_proposals_nms_batch')


def test_header_declares_and_library_exports_the_batched_selection():
    hdr = open(os.path.join(ROOT, 'include', 'echr_hip.h')).read()
    declared = {n: a for n, _, a in _lib.SYMBOLS}
    lib = _lib.load()
    for name in EXPORTS:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in declared and len(declared[name]) == 17, name
        assert getattr(lib, name) is not None
    assert lib.echr_version() == 3                       # no struct was added or changed: the ABI version stays
    for cname, cls in _lib.ABI_STRUCTS.items():
        assert lib.echr_abi_sizeof(cname.encode()) == __import__('ctypes').sizeof(cls), cname


def test_ref_reproduces_the_reference_fixture():
    g = U.gold('props_batch.npz')
    lengths, K = g['lengths'].tolist(), int(g['K'])
    ro = R.offsets(lengths)
    assert lengths == [1, 40, 7, 24, 96] and K == 32
    for i in range(4):
        for mask in (None, R.causal_mask(lengths, K)):
            r = R.select(g['t%d|scores' % i], ro, int(g['t%d|topN' % i]), float(g['t%d|thres' % i]), mask=mask)
            assert r['count'][:5].tolist() == g['t%d|count' % i].tolist() and r['count'][5] == len(g['t%d|ind' % i])
            assert np.array_equal(r['ind'], g['t%d|ind' % i]) and np.array_equal(r['feat'], g['t%d|feat' % i])
            assert np.array_equal(r['conf'], g['t%d|conf' % i])
            assert np.array_equal(r['event_offset'], R.offsets(g['t%d|count' % i])) and np.array_equal(r['vid'], np.repeat(np.arange(5), r['count'][:5]))
            assert np.array_equal(r['ind_abs'], r['ind'] + ro[r['vid']]) and np.array_equal(r['feat_abs'], r['feat'] + ro[r['vid']][:, None])
            assert r['count'][6] == (r['feat'][:, 1] - r['feat'][:, 0]).max()
    assert g['t1|count'].max() > 50 and g['t2|count'].tolist()[2] == 0 and g['t3|count'].tolist() == [min(T, K) * (min(T, K) + 1) // 2 + max(T - K, 0) * K for T in lengths]
    for j in range(4):
        r = R.select(g['n|scores'], ro, int(g['n%d|topN' % j]), overlap=float(g['n%d|overlap' % j]))
        assert r['count'][:5].tolist() == g['n%d|count' % j].tolist() and r['count'][0] == 0
        assert np.array_equal(r['feat'], g['n%d|props' % j]) and np.array_equal(r['conf'], g['n%d|conf' % j].astype(np.float32))
        assert np.array_equal(r['ind'], r['feat'][:, 1] - 1) and np.array_equal(r['feat_abs'], r['feat'] + ro[r['vid']][:, None])


def _batch(counts, T=12):
    vids = []
    for i, n in enumerate(counts):
        v = synth.make_video(n, 8, 6, 301, seed=3 + i, T_v=T, video_dim=20, hidden_dim=24, lda_dim=10)
        vids.append({k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi')})
    return VideoBatch.from_videos(vids)


@pytest.mark.parametrize('G', [1, 2, 3, 4, 5, 7, 8, 11, 12, 19, 20, 1000])
def test_event_groups_cut_the_video_axis_into_bounded_consecutive_runs(G):
    counts = [3, 1, 4, 9, 2, 2, 5, 1]
    b = _batch(counts)
    runs = b.event_groups(G)
    eo = b.event_offset
    assert runs[0][0] == 0 and runs[-1][1] == len(counts)
    for (v0, v1, e0, e1), nxt in zip(runs, runs[1:] + [None]):
        assert v0 < v1 and (e0, e1) == (eo[v0], eo[v1])
        assert e1 - e0 <= G or v1 - v0 == 1                      # only a video of its own may exceed G
        if nxt is not None:
            assert nxt[0] == v1 and nxt[2] == e1                 # consecutive and ordered: every video in exactly one run
            assert e1 - e0 + counts[v1] > G                      # greedy: the next video did not fit
    if G < min(counts) or G == 1:
        assert len(runs) == len(counts)
    if G >= sum(counts):
        assert runs == [(0, len(counts), 0, sum(counts))]


def test_event_groups_refuses_a_non_positive_bound():
    b = _batch([2, 3])
    for G in (0, -4):
        with pytest.raises(ValueError):
            b.event_groups(G)
    assert b.event_groups(2) == [(0, 1, 0, 2), (1, 2, 2, 5)] and b.event_groups(5) == [(0, 2, 0, 5)]


def test_event_group_rows_is_taken_by_eval_mode_only():
    import echr_amd
    opt, params, _ = synth.make_case('tiny')
    m = echr_amd.CaptionGenerator(opt)
    b = _batch([2, 3])
    with pytest.raises(ValueError, match='event_group_rows'):
        m.forward_batch(b, mode='train', event_group_rows=4)
    with pytest.raises(_lib.EchrHipError):                        # accepted for 'eval'; a host batch then fails at the device check
        m.forward_batch(b, mode='eval', event_group_rows=4)


def test_caption_videos_on_cpu_tensors_raises():
    import echr_amd
    from echr_amd import eval_utils as EU, models
    opt, params, _ = synth.make_case('tiny')
    cg = echr_amd.CaptionGenerator(opt)
    tap = models.setup_tap(opt)
    vids = [dict(c3d=torch.zeros(6, opt.video_dim), lda=torch.zeros(opt.video_context_dim), duration=10.0) for _ in range(2)]
    with pytest.raises(_lib.EchrHipError):
        EU.caption_videos(tap, cg, vids, lambda s, e, n, d: [s, e])
    with pytest.raises(ValueError):
        EU.caption_videos(tap, cg, vids, lambda s, e, n, d: [s, e], flag_eval_what='cg_extend')
    with pytest.raises(_lib.EchrHipError):
        EU.top_proposals_batch_device(torch.zeros(6, 4), [0, 2, 6])
    assert EU.EVENT_GROUP_ROWS == 128 and 'beam_size' not in EU.caption_videos.__code__.co_varnames

"""External-proposal selection on the GPU (-m gpu): echr_amd.extprops.nms / select (echr_nms_segments_batch, echr_ext_proposals_batch) against
the reference's recorded picks and against tests/extprops_ref.py, which tests/test_extprops_host.py pins to them, and the 'SOTA_TEP' mode of
the evaluation entries.  Every index output is compared EXACTLY: the overlap is correctly rounded fp64 without a product, the featstamp is
one correctly rounded divide and product under round(), and the crop is a pure function of integer keys -- there is no tolerance to state.
The captions of the last test go through the decoder and carry the suite's existing gates (see there)."""
import numpy as np
import pytest
import torch

from tests import extprops_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD5EED0123          # (both halves of the key are non-zero)


def _nms(st, ps, ss, thr, topN=1000):
    from echr_amd import extprops as XP
    props, scores, pick = XP.nms(st, ps, ss, thr, topN)
    assert np.array_equal(props, np.asarray(st)[pick]) and np.array_equal(scores, np.asarray(ps)[pick])
    return pick


def _random_list(rs, P, span=180.0, longest=60.0):
    start = rs.uniform(0.0, span, size=P)
    return np.stack([start, start + rs.uniform(0.5, longest, size=P)], 1), (rs.permutation(P) + 1.0) / P


def test_nms_equals_the_reference_fixtures():
    """extprops.npz (P = 1 .. 1100, both sent_score forms, the 1000-round cap) and the m0..m2 lists of proposals.npz: pick order included."""
    g = U.gold('extprops.npz')
    for i in range(int(g['n'])):
        p = 'c%d|' % i
        st, ps, ss = (g[p + k].astype(np.float64) for k in ('stamps', 'pscore', 'sscore'))
        thr, topN = float(g[p + 'thr']), int(g[p + 'topN'])
        assert _nms(st, ps, ps, thr, topN) == g[p + 'pick_p'].tolist(), i
        assert _nms(st, ps, ss, thr, topN) == g[p + 'pick_s'].tolist(), i
    m = U.gold('proposals.npz')
    for i in range(3):
        pick = _nms(m['m%d|props' % i], m['m%d|pscore' % i], m['m%d|sscore' % i], float(m['m%d|thr' % i]), int(m['m%d|topN' % i]))
        assert pick == m['m%d|pick' % i].tolist(), i


def test_nms_ties_and_the_threshold_itself():
    # two identical segments: the higher score leads, the other is clustered (o = 1) and leaves with it
    st = np.array([[3.0, 9.5], [3.0, 9.5], [20.0, 21.0]])
    assert _nms(st, [0.2, 0.7, 0.5], [0.2, 0.7, 0.5], 0.5) == R.nms(st, [0.2, 0.7, 0.5], [0.2, 0.7, 0.5], 0.5) == [1, 2]
    # tied scores as well: the larger index leads, and the tied cluster is represented by its first member in ascending (score, index) order
    assert _nms(st, [0.7, 0.7, 0.5], [0.7, 0.7, 0.5], 0.5) == R.nms(st, [0.7, 0.7, 0.5], [0.7, 0.7, 0.5], 0.5) == [0, 2]
    assert _nms(st, [0.2, 0.7, 0.5], [0.9, 0.1, 0.5], 0.5) == [0, 2]          # ... and the cluster is represented by its best sent_score
    # o exactly at the threshold: the partner is in the cluster AND stays alive, so it is picked again
    a, b = (0.0, 10.0), (2.0, 9.0)
    thr = float(R.overlap(a, b))
    assert 0.5 < thr < 1.0
    st, ps, ss = np.array([a, b, (50.0, 51.0)]), [0.9, 0.5, 0.1], [0.1, 0.8, 0.3]
    want = R.nms(st, ps, ss, thr)
    assert want == [1, 1, 2]                                        # round 1: best 0, the pick is its partner 1; round 2: 1 itself
    assert _nms(st, ps, ss, thr) == want
    assert _nms(st, ps, ss, np.nextafter(thr, 0.0)) == R.nms(st, ps, ss, np.nextafter(thr, 0.0)) == [1, 2]          # just below: 1 leaves with 0
    assert _nms(st, ps, ss, np.nextafter(thr, 1.0)) == R.nms(st, ps, ss, np.nextafter(thr, 1.0)) == [0, 1, 2]       # just above: not clustered
    # tied prop_scores over more than one wave: the stable rule (ascending (score, index), the best is the last)
    rs = np.random.RandomState(41)
    st, _ = _random_list(rs, 150, span=60.0, longest=20.0)
    ps = rs.randint(0, 4, size=150) / 4.0
    ss = rs.permutation(150) / 150.0
    for thr in (0.3, 0.7):
        assert _nms(st, ps, ps, thr) == R.nms(st, ps, ps, thr)
        assert _nms(st, ps, ss, thr) == R.nms(st, ps, ss, thr)
    # tied sent_score: the member that comes first in ascending (prop_score, index) order
    ps = (rs.permutation(150) + 1.0) / 150
    ss = rs.randint(0, 3, size=150) / 3.0
    assert _nms(st, ps, ss, 0.3) == R.nms(st, ps, ss, 0.3)
    assert _nms(st, np.zeros(150), np.zeros(150), 0.3) == R.nms(st, np.zeros(150), np.zeros(150), 0.3)
    # threshold 0: everything that touches the best is clustered, what is disjoint from it stays
    assert _nms(st, ps, ss, 0.0) == R.nms(st, ps, ss, 0.0)
    assert _nms(st, ps, ss, 0.5, topN=3) == R.nms(st, ps, ss, 0.5, topN=3)


@pytest.mark.parametrize('P', [1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096])
def test_nms_at_the_slot_and_staging_sizes(P):
    """A thread holds the proposals of ranks t, t + 1024, ...: P around every slot boundary and at the bound ECHR_EXTPROPS_MAX_P = 4096."""
    rs = np.random.RandomState(P)
    st, ps = _random_list(rs, P)
    ss = rs.permutation(P) / float(P)
    assert _nms(st, ps, ss, 0.6) == R.nms(st, ps, ss, 0.6)
    if P == 4096:
        from echr_amd import extprops as XP
        with pytest.raises(ValueError, match='ECHR_EXTPROPS_MAX_P'):
            XP.nms(np.concatenate([st, st[:1]]), np.concatenate([ps, ps[:1]]), np.concatenate([ss, ss[:1]]), 0.6)


def _ragged():
    """P_v = None, 0, 1, 7, 300, 1025 with other row counts and durations each; many segments are longer than K = 16 rows."""
    rs = np.random.RandomState(77)
    out = []
    for v, P in enumerate((None, 0, 1, 7, 300, 1025)):
        T, dur = 90 + 13 * v, 100.0 + 7.5 * v
        if P is None:
            out.append(dict(SOTA_timestamps=None, SOTA_Prop_score=None, duration=dur, nfeats=T))
            continue
        st, ps = _random_list(rs, P, span=dur * 0.9, longest=dur * 0.4)
        out.append(dict(SOTA_timestamps=st, SOTA_Prop_score=ps, duration=dur, nfeats=T))
    return out


def _same(sel, v, want):
    assert np.array_equal(sel.pick[v], want['pick']) and sel.pick[v].dtype == np.int64, v
    assert np.array_equal(sel.ind[v], want['ind']) and np.array_equal(sel.soi[v], want['soi']), v
    assert np.array_equal(sel.scores[v], want['scores']) and np.array_equal(sel.timestamps[v], want['timestamps']), v


@pytest.mark.parametrize('nms', [0.0, 0.5, 0.999])
def test_select_on_a_ragged_batch(nms):
    from echr_amd import extprops as XP
    videos, K = _ragged(), 16
    draw = [3, 1, 4, 1, 5, 9]
    for kw in (dict(), dict(val_score_thres=0.4), dict(topN=5), dict(topN=250, val_score_thres=0.1)):
        sel = XP.select(videos, K, nms_threshold=nms, seed=SEED, draw=draw, **kw)
        assert sel.bad == [0] and sel.n_videos == 6
        want = [R.select(vid, K, nms_threshold=nms, seed=SEED, draw=draw[v], **kw) for v, vid in enumerate(videos)]
        for v in range(6):
            _same(sel, v, want[v])
        assert sel.event_offset.tolist() == np.concatenate([[0], np.cumsum([len(w['pick']) for w in want])]).tolist()
        n = [len(w['pick']) for w in want]
        if not kw:
            assert n[:3] == [0, 0, 1] and (n[5] == 1000) == (nms != 0.5)          # the 1025: cut by topN at 0, by the 1000 rounds at 0.999
            assert any((w['soi'][:, 1] - w['soi'][:, 0] == K + 1).any() for w in want)                    # cropped events are there
        if kw == dict(val_score_thres=0.4):
            full = [len(R.select(vid, K, nms_threshold=nms, seed=SEED, draw=draw[v])['pick']) for v, vid in enumerate(videos)]
            assert n[4] < full[4] and n[5] < full[5]                                                     # the threshold cuts
        if kw == dict(topN=5):
            assert n[3:] == [5, 5, 5]                                                                    # fewer than the picks
    # each video alone gives the list it gives inside the batch
    sel = XP.select(videos, K, nms_threshold=nms, seed=SEED, draw=draw)
    for v in range(6):
        alone = XP.select(videos[v:v + 1], K, nms_threshold=nms, seed=SEED, draw=draw[v:v + 1])
        assert alone.bad == ([0] if v == 0 else [])
        _same(alone, 0, dict(pick=sel.pick[v], ind=sel.ind[v], soi=sel.soi[v], scores=sel.scores[v], timestamps=sel.timestamps[v]))


def test_featstamps_halves_and_clamps():
    """duration 8 and 16 rows (both powers of two: x.5 rows are exact): exact halves go away from zero, start clamps to 0 and to T - 2, end
    to start + 1 and to T - 1, a start beyond the duration, an end that rounds to the start."""
    from echr_amd import extprops as XP, targets as TG
    st = [(1.25, 3.75), (0.25, 0.75), (2.25, 6.25), (-3.0, 0.1), (7.9, 20.0), (9.0, 12.0), (100.0, 1e9), (4.0, 4.0), (4.1, 4.2), (0.0, 8.0),
          (3.75, 3.76), (-2.0, -1.0)]
    want = TG.featstamps(st, 16, 8.0)
    assert want[:5] == [(3, 8), (1, 2), (5, 13), (0, 1), (14, 15)] and want[5] == want[6] == (14, 15) and want[7] == (8, 9) and want[8] == (8, 9)
    vid = dict(SOTA_timestamps=st, SOTA_Prop_score=np.linspace(0.1, 0.9, len(st)), duration=8.0, nfeats=16)
    sel = XP.select([vid], 64, crop=False)
    assert sel.pick[0].tolist() == list(range(len(st)))
    assert [tuple(x) for x in np.stack([sel.soi[0][:, 0], sel.soi[0][:, 1] - 1], 1).tolist()] == want and sel.ind[0].tolist() == [e for _, e in want]
    # a two-row video: everything is (0, 1)
    sel = XP.select([dict(vid, nfeats=2)], 64)
    assert sel.soi[0].tolist() == [[0, 2]] * len(st)
    # other row counts and durations against the host function
    rs = np.random.RandomState(8)
    vids = []
    for T, dur in ((37, 61.3), (256, 211.7), (3, 5.0)):
        s, ps = _random_list(rs, 200, span=dur * 1.1, longest=dur * 0.5)
        vids.append(dict(SOTA_timestamps=s, SOTA_Prop_score=ps, duration=dur, nfeats=T))
    sel = XP.select(vids, 8, crop=False)
    for v, vid in enumerate(vids):
        f = np.asarray(TG.featstamps(vid['SOTA_timestamps'].tolist(), vid['nfeats'], vid['duration']), np.int64)
        assert np.array_equal(sel.soi[v], np.stack([f[:, 0], f[:, 1] + 1], 1)) and np.array_equal(sel.ind[v], f[:, 1])


def test_crop_at_k4():
    from echr_amd import extprops as XP, targets as TG
    K, T, dur = 4, 64, 64.0
    rs = np.random.RandomState(12)
    st, ps = _random_list(rs, 500, span=50.0, longest=30.0)
    vid = dict(SOTA_timestamps=st, SOTA_Prop_score=ps, duration=dur, nfeats=T)
    plain = np.asarray(TG.featstamps(st.tolist(), T, dur), np.int64)
    sel = XP.select([vid], K, seed=SEED, draw=[6])
    want = R.select(vid, K, seed=SEED, draw=6)
    _same(sel, 0, want)
    s0, e0, s1, e1 = plain[:, 0], plain[:, 1], sel.soi[0][:, 0], sel.soi[0][:, 1] - 1
    long = e0 - s0 >= K + 1
    assert 100 < long.sum() < 500
    assert (s1[long] >= s0[long]).all() and (e1[long] == s1[long] + K).all() and (e1[long] <= e0[long]).all()
    assert np.array_equal(s1[~long], s0[~long]) and np.array_equal(e1[~long], e0[~long])
    assert (s1[long] > s0[long]).any() and (e1[long] < e0[long]).any() and np.array_equal(sel.ind[0], e1)
    for kw in (dict(seed=SEED + 1, draw=[6]), dict(seed=SEED, draw=[7]), dict(seed=SEED + (1 << 32), draw=[6])):
        other = XP.select([vid], K, **kw)
        assert not np.array_equal(other.soi[0], sel.soi[0]) and np.array_equal(other.soi[0][~long], sel.soi[0][~long])
    again = XP.select([vid], K, seed=SEED, draw=[6])
    assert np.array_equal(again.soi[0], sel.soi[0])
    off = XP.select([vid], K, seed=SEED, draw=[6], crop=False)
    assert np.array_equal(off.soi[0], np.stack([s0, e0 + 1], 1))
    # 4096 proposals of rows (2, 10): 5 admissible offsets, every count within 5 sigma of uniform (the key is checked on the host first)
    P = 4096
    same = dict(SOTA_timestamps=np.tile([[2.0, 10.0]], (P, 1)), SOTA_Prop_score=np.full(P, 0.5), duration=16.0, nfeats=16)
    sel = XP.select([same], K, topN=P, seed=R.CROP_SEED, draw=[R.CROP_DRAW])
    r = sel.soi[0][:, 0] - 2
    assert len(r) == P and np.array_equal(r, (R.crop_words(np.arange(P), R.CROP_SEED, R.CROP_DRAW) * np.uint64(5) >> np.uint64(32)).astype(np.int64))
    counts = np.bincount(r, minlength=5)
    assert len(counts) == 5 and (np.abs(counts - P / 5.0) < 5 * np.sqrt(P * 0.2 * 0.8)).all(), counts
    assert (sel.soi[0][:, 1] == sel.soi[0][:, 0] + K + 1).all()


def test_caption_videos_on_external_proposals():
    """flag_eval_what='SOTA_TEP' on 3 small videos (one without a proposal list), vocabulary and widths of tests/test_gpu_eval_batch.py.  The
    selection is compared exactly with the oracle; the records equal those of flag_eval_what='cg' fed the oracle's selection in every field
    but proposal_score and re_score, which follow from the external scores.  Both runs share the code behind the selection and run with
    fixed-order accumulation, so the sentences are compared exactly; sentence_confidence carries the suite's 1e-3 gate, also against
    caption_video alone (whose encoder call is the single-video one)."""
    import echr_amd
    from echr_amd import eval_utils as EU
    from tests import test_gpu_eval_batch as EB
    opt, params = EB.make_opt()
    K = opt.K
    tap, cg = EB.make_tap(opt).cuda(), U.build_gpu_model(opt, params, False)
    rs = np.random.RandomState(23)
    lengths, counts = (24, 9, 40), (6, None, 9)
    videos = []
    for T, P in zip(lengths, counts):
        v = dict(c3d=rs.standard_normal((T, opt.video_dim)).astype(np.float32), lda=rs.standard_normal(opt.lda_dim).astype(np.float32),
                 duration=EB.DURATION)
        if P is not None:
            v['SOTA_timestamps'], v['SOTA_Prop_score'] = _random_list(rs, P, span=45.0, longest=40.0)
        videos.append(v)
    videos[2]['cg_gts'] = rs.randint(0, 5, size=(40, K))
    kw = dict(topN=5, nms_threshold=0.7, val_score_thres=0.15)
    ext = [dict(SOTA_timestamps=v.get('SOTA_timestamps'), SOTA_Prop_score=v.get('SOTA_Prop_score'), duration=v['duration'], nfeats=T)
           for v, T in zip(videos, lengths)]
    echr_amd.set_deterministic(True)
    try:
        for draws in (None, [0, 0, 0]):
            vids = [dict(v) if draws is None else dict(v, SOTA_draw=draws[i]) for i, v in enumerate(videos)]
            want = [R.select(e, K, seed=SEED, draw=(i if draws is None else draws[i]), **kw) for i, e in enumerate(ext)]
            assert [len(w['pick']) for w in want] == [5, 0, 5]
            assert any((w['soi'][:, 1] - w['soi'][:, 0] == K + 1).any() for w in want)
            infos, ex = EU.caption_videos(tap, cg, EB.to_dev(vids), EB.f2t, flag_eval_what='SOTA_TEP', ext_seed=SEED, **kw)
            assert ex['bad'] == [1] and infos[1] == [] and ex['kept'] == [0, 2]
            for v in range(3):
                pv = ex['per_video'][v]
                assert pv['ind_select_list'] == want[v]['ind'].tolist() and pv['soi_select_list'] == want[v]['soi'].tolist()
            gts = videos[2]['cg_gts']
            assert ex['per_video'][2]['cg_select_list'] == [gts[e, e - s - 1] for e, (s, _) in zip(want[2]['ind'].tolist(), want[2]['soi'].tolist())]
            assert ex['per_video'][0]['cg_select_list'] == []
            # (without cg_gts: the 'cg' mode reads cg_gts[n, n - s], one column further -- the off-by-one the docstring names)
            given = [dict({k: x for k, x in v.items() if k != 'cg_gts'}, ind=w['ind'], soi=w['soi'], timestamps=w['timestamps'].tolist())
                     for v, w in zip(videos, want)]
            infos_cg, ex_cg = EU.caption_videos(tap, cg, EB.to_dev(given), EB.f2t, flag_eval_what='cg')
            assert np.array_equal(ex['seq'].cpu().numpy(), ex_cg['seq'].cpu().numpy())
            for v in (0, 2):
                assert len(infos[v]) == len(infos_cg[v]) == len(want[v]['pick']) > 0
                for i, (a, b) in enumerate(zip(infos[v], infos_cg[v])):
                    assert set(a) == set(b) and a['sentence'] == b['sentence'] and a['num'] == b['num'] == [i, len(infos[v])]
                    assert a['timestamp'] == b['timestamp'] == want[v]['timestamps'][i].tolist()
                    assert abs(a['sentence_confidence'] - b['sentence_confidence']) < 1e-3
                    assert a['proposal_score'] == float(want[v]['scores'][i]) and b['proposal_score'] == 1.0
                    assert abs(a['re_score'] - (10 * a['proposal_score'] + a['sentence_confidence'])) < 1e-9
        # (draw id 0 everywhere:) each video equals caption_video(..., ext_proposals=...) alone
        dv = EB.to_dev(videos)
        for v in range(3):
            props = (videos[v].get('SOTA_timestamps'), videos[v].get('SOTA_Prop_score'))
            info1, ex1 = EU.caption_video(tap, cg, dv[v]['c3d'], dv[v]['lda'], EB.DURATION, EB.f2t, cg_gts=videos[v].get('cg_gts', ()),
                                          flag_eval_what='SOTA_TEP', ext_proposals=props, ext_seed=SEED, **kw)
            assert ex1['ind_select_list'] == want[v]['ind'].tolist() and ex1['soi_select_list'] == want[v]['soi'].tolist()
            assert len(info1) == len(infos[v])
            for a, b in zip(info1, infos[v]):
                assert a['sentence'] == b['sentence'] and a['timestamp'] == b['timestamp'] and a['num'] == b['num']
                assert a['proposal_score'] == b['proposal_score'] and abs(a['sentence_confidence'] - b['sentence_confidence']) < 1e-3
        # beam search over the batch runs the same selection
        infos_b, ex_b = EU.caption_videos_beam(tap, cg, EB.to_dev(vids), EB.f2t, 2, flag_eval_what='SOTA_TEP', ext_seed=SEED, **kw)
        assert ex_b['bad'] == [1] and infos_b[1] == []
        for v in range(3):
            assert ex_b['per_video'][v]['soi_select_list'] == want[v]['soi'].tolist()
        for v in (0, 2):
            assert len(infos_b[v]) == len(want[v]['pick'])
            for i, a in enumerate(infos_b[v]):
                assert a['timestamp'] == want[v]['timestamps'][i].tolist() and a['proposal_score'] == float(want[v]['scores'][i])
    finally:
        echr_amd.set_deterministic(False)

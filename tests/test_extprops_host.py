"""External-proposal selection (echr_amd.extprops, csrc/extprops.hip; flag_eval_what = 'SOTA_TEP') without a GPU: the suite's oracle against
the reference's recorded picks, every refusal that runs ahead of the upload, the bad-video rule, the crop draw's site and the ABI."""
import os
import re

import numpy as np
import pytest
import torch

from tests import extprops_ref as R
from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vid(P=3, **kw):
    st = np.stack([np.arange(P) * 2.0, np.arange(P) * 2.0 + 1.5], 1)
    d = dict(SOTA_timestamps=st, SOTA_Prop_score=(np.arange(P) + 1.0) / P, duration=10.0, nfeats=20)
    d.update(kw)
    return d


def test_oracle_equals_the_reference_picks():
    g = U.gold('extprops.npz')
    sizes = []
    for i in range(int(g['n'])):
        p = 'c%d|' % i
        st, ps, ss = (g[p + k].astype(np.float64) for k in ('stamps', 'pscore', 'sscore'))
        thr, topN = float(g[p + 'thr']), int(g[p + 'topN'])
        assert len(np.unique(ps)) == len(ps) and len(np.unique(ss)) == len(ss)
        assert R.nms(st, ps, ps, thr, topN) == g[p + 'pick_p'].tolist(), i
        assert R.nms(st, ps, ss, thr, topN) == g[p + 'pick_s'].tolist(), i
        sizes.append(len(ps))
    assert sizes == [1, 2, 7, 1023, 1025, 1100]
    assert len(g['c5|pick_p']) == 1000 < 1100                      # disjoint segments: the 1000-round cap bites
    assert not np.array_equal(g['c3|pick_p'], g['c3|pick_s'])      # the separate sent_score changes the representatives
    m = U.gold('proposals.npz')
    for i in range(3):
        pick = R.nms(m['m%d|props' % i], m['m%d|pscore' % i], m['m%d|sscore' % i], float(m['m%d|thr' % i]), int(m['m%d|topN' % i]))
        assert pick == m['m%d|pick' % i].tolist(), i


def test_no_fixture_overlap_sits_at_its_threshold():
    g = U.gold('extprops.npz')
    for i in range(int(g['n'])):
        st, thr = g['c%d|stamps' % i].astype(np.float64), float(g['c%d|thr' % i])
        t1, t2 = st[:, 0], st[:, 1]
        area = t2 - t1 + 1e-3
        for j in range(len(st)):
            wh = np.maximum(0., np.minimum(t2[j], t2) - np.maximum(t1[j], t1) + 1e-3)
            assert (np.abs(wh / (area[j] + area - wh) - thr) > 1e-9).all(), (i, j)


def test_oracle_selection_rules():
    """The filter loop of eval_utils.py:88-104 and the conversion behind it, on a hand-checked list."""
    st = [(0.0, 4.0), (0.1, 4.1), (5.0, 6.0), (8.0, 9.5), (2.0, 2.0)]
    sc = [0.9, 0.8, 0.3, 0.7, 0.6]
    vid = dict(SOTA_timestamps=st, SOTA_Prop_score=sc, duration=10.0, nfeats=20)
    o = R.select(vid, K=64)
    assert o['pick'].tolist() == [0, 1, 2, 3, 4] and o['soi'].tolist() == [[0, 9], [0, 9], [10, 13], [16, 20], [4, 6]]
    assert o['ind'].tolist() == [8, 8, 12, 19, 5] and np.array_equal(o['timestamps'], np.asarray(st)) and o['scores'].tolist() == sc
    o = R.select(vid, K=64, nms_threshold=0.5)                     # 1 is suppressed by 0 (o = 3.901 / 4.101)
    assert o['pick'].tolist() == [0, 2, 3, 4]
    assert R.select(vid, K=64, nms_threshold=0.5, val_score_thres=0.6)['pick'].tolist() == [0, 3, 4]
    assert R.select(vid, K=64, nms_threshold=0.5, topN=2)['pick'].tolist() == [0, 2]
    assert R.select(vid, K=64, nms_threshold=0.5, nms_rounds=2)['pick'].tolist() == [0, 3]          # the two best clusters
    for bad in (dict(vid, SOTA_Prop_score=None), dict(vid, nfeats=1)):
        assert len(R.select(bad, K=64)['pick']) == 0
    # the crop: (0, 8) at K = 4 has 5 admissible offsets
    o = R.select(vid, K=4, seed=11, draw=3)
    w = R.crop_words([0, 1, 2, 3, 4], 11, 3)
    r0 = (int(w[0]) * 5) >> 32
    assert 0 <= r0 <= 4 and o['soi'][0].tolist() == [r0, r0 + 5] and o['ind'][0] == r0 + 4
    assert o['soi'][2].tolist() == [10, 13] and o['soi'][4].tolist() == [4, 6]          # e - s <= K: left alone
    assert R.select(vid, K=4, seed=11, draw=3, do_crop=False)['soi'].tolist() == R.select(vid, K=64)['soi'].tolist()


def test_crop_site_and_draw():
    from echr_amd import philox
    assert philox.SITE_CROP == 8 and philox.SITE_PROP == 7
    src = open(os.path.join(ROOT, 'echr_amd', 'csrc', 'echr_common.h')).read()
    assert re.search(r'constexpr unsigned SITE_CROP = 8u;', src) and re.search(r'constexpr unsigned SITE_PROP = 7u;', src)
    w = philox.philox4x32_10(np.array([9 >> 2], np.uint32), 3, 8, 0, 5, 0)
    assert int(R.crop_words([9], 5, 3)[0]) == int(w[9 & 3][0])
    assert int(R.crop_words([9], 5 + (1 << 32), 3)[0]) != int(R.crop_words([9], 5, 3)[0])          # the high half of the seed is part of the key
    # the seed the GPU suite uses: 4096 draws over 5 offsets, every count within 5 sigma of uniform
    r = (R.crop_words(np.arange(4096), R.CROP_SEED, R.CROP_DRAW) * np.uint64(5)) >> np.uint64(32)
    counts = np.bincount(r.astype(np.int64), minlength=5)
    assert counts.sum() == 4096 and len(counts) == 5
    assert (np.abs(counts - 4096 / 5.0) < 5 * np.sqrt(4096 * 0.2 * 0.8)).all(), counts


ENTRIES = ('echr_nms_segments_batch', 'echr_ext_proposals_batch')


def test_new_symbols_are_declared_bound_and_exported():
    from echr_amd import _lib, build, extprops as XP
    assert 'extprops.hip' in build.SOURCES
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'echr_hip.h')).read()
    declared = set(re.findall(r'\b(echr_[a-z0-9_]+)\s*\(', hdr))
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert name in declared and name in bound and hasattr(lib, name), name
    assert lib.echr_version() == _lib.ABI_VERSION == 3
    m = re.search(r'#define ECHR_EXTPROPS_MAX_P (\d+)', hdr)
    assert m and int(m.group(1)) == XP.MAX_P >= 4096
    assert int(re.search(r'#define ECHR_EXTPROPS_MAX_VIDEOS (\d+)', hdr).group(1)) == XP.MAX_VIDEOS


def test_library_refusals_name_their_argument():
    """The checks in front of the launches (null pointers never reach a kernel)."""
    from echr_amd import _lib
    lib = _lib.load()
    assert lib.echr_nms_segments_batch(None, None, None, None, 1, 5000, 4097, 0.5, 10, None, None, None) == -22
    assert b'ECHR_EXTPROPS_MAX_P' in lib.echr_last_error()
    assert lib.echr_nms_segments_batch(None, None, None, None, 1, 4, 4, 1.0, 10, None, None, None) == -22 and b'nms_overlap' in lib.echr_last_error()
    assert lib.echr_nms_segments_batch(None, None, None, None, 1, 4, 4, 0.5, 0, None, None, None) == -22 and b'rounds' in lib.echr_last_error()
    assert lib.echr_nms_segments_batch(None, None, None, None, 1, 4, 4, 0.5, 10, None, None, None) == -22 and b'required' in lib.echr_last_error()
    z = (None,) * 7
    assert lib.echr_ext_proposals_batch(*z, 10, 1, 5000, 4097, 4, 10, 0.0, 1, 0, None, None, 0, None, None, None, None, None, None) == -22
    assert b'ECHR_EXTPROPS_MAX_P' in lib.echr_last_error()
    assert lib.echr_ext_proposals_batch(*z, 10, 1, 4, 4, 4, 0, 0.0, 1, 0, None, None, 0, None, None, None, None, None, None) == -22
    assert b'topN' in lib.echr_last_error()
    assert lib.echr_ext_proposals_batch(*z, 10, 1, 4, 4, 4, 10, 0.0, 2, 0, None, None, 0, None, None, None, None, None, None) == -22
    assert b'crop' in lib.echr_last_error()
    assert lib.echr_ext_proposals_batch(*z, 10, 0, 4, 4, 4, 10, 0.0, 1, 0, None, None, 0, None, None, None, None, None, None) == -22
    assert b'videos' in lib.echr_last_error()


def test_select_refuses_bad_input_before_the_upload():
    from echr_amd import extprops as XP
    ok = _vid()
    bad_st = np.array(ok['SOTA_timestamps'])
    bad_st[1, 1] = np.inf
    with pytest.raises(ValueError, match='video 1: proposal 1 is not finite'):
        XP.select([ok, _vid(SOTA_timestamps=bad_st)], 8)
    with pytest.raises(ValueError, match='not finite'):
        XP.select([_vid(SOTA_Prop_score=[0.1, np.nan, 0.3])], 8)
    rev = np.array(ok['SOTA_timestamps'])
    rev[2] = [5.0, 4.0]
    with pytest.raises(ValueError, match='proposal 2 has end < start'):
        XP.select([_vid(SOTA_timestamps=rev)], 8)
    for d in (0.0, -1.0, np.inf):
        with pytest.raises(ValueError, match='duration'):
            XP.select([_vid(duration=d)], 8)
    with pytest.raises(ValueError, match='re-picks the same proposal'):
        XP.select([ok], 8, nms_threshold=1.0)
    with pytest.raises(ValueError, match='empty cluster'):
        XP.select([ok], 8, nms_threshold=1.5)
    with pytest.raises(ValueError, match='nms_threshold'):
        XP.select([ok], 8, nms_threshold=-0.1)
    with pytest.raises(ValueError, match='topN'):
        XP.select([ok], 8, topN=0)
    with pytest.raises(ValueError, match='ECHR_EXTPROPS_MAX_P'):
        XP.select([_vid(P=XP.MAX_P + 1)], 8)
    for dr in ([-1], [2 ** 31], [0, 1]):
        with pytest.raises(ValueError, match='draw'):
            XP.select([ok], 8, draw=dr)
    with pytest.raises(ValueError, match='3 segments and 2 scores'):
        XP.select([_vid(SOTA_Prop_score=[0.1, 0.2])], 8)
    with pytest.raises(ValueError):
        XP.select([], 8)
    with pytest.raises(ValueError, match='K'):
        XP.select([ok], 0)
    # nms: the same checks on one list
    st, sc = ok['SOTA_timestamps'], ok['SOTA_Prop_score']
    with pytest.raises(ValueError, match='nms_threshold'):
        XP.nms(st, sc, sc, 1.0, 10)
    with pytest.raises(ValueError, match='topN'):
        XP.nms(st, sc, sc, 0.5, 0)
    with pytest.raises(ValueError, match='sent_score'):
        XP.nms(st, sc, sc[:2], 0.5, 10)
    with pytest.raises(ValueError, match='end < start'):
        XP.nms(rev, sc, sc, 0.5, 10)


def test_bad_videos_select_nothing_without_a_device():
    """A call whose videos are all bad (score list None or missing, at most one row) never reaches the device: empty lists, all in `bad`."""
    from echr_amd import extprops as XP
    missing = _vid()
    del missing['SOTA_Prop_score']
    sel = XP.select([_vid(SOTA_Prop_score=None), missing, _vid(nfeats=1), _vid(P=0)], 8)
    assert sel.bad == [0, 1, 2] and sel.n_videos == 4
    for v in range(4):
        assert len(sel.pick[v]) == len(sel.ind[v]) == len(sel.scores[v]) == 0 and sel.soi[v].shape == sel.timestamps[v].shape == (0, 2)
    assert sel.event_offset.tolist() == [0] * 5
    props, scores, pick = XP.nms(np.zeros((0, 2)), [], [], 0.5, 10)
    assert pick == [] and len(props) == 0
    from echr_amd._lib import EchrHipError
    with pytest.raises(EchrHipError):
        XP.select([_vid()], 8, device='cpu')


def test_sota_tep_is_accepted_and_reaches_the_device_check():
    """caption_videos(flag_eval_what='SOTA_TEP') on CPU tensors gets past the mode check to the GPU-only error; the unsupported modes keep
    raising ValueError, and the crop key is keyword-only."""
    import echr_amd
    from echr_amd import _lib, eval_utils as EU, models, synth
    opt, params, _ = synth.make_case('tiny')
    cg = echr_amd.CaptionGenerator(opt)
    tap = models.setup_tap(opt)
    f2t = lambda s, e, n, d: [s, e]
    vids = [dict(c3d=torch.zeros(6, opt.video_dim), lda=torch.zeros(opt.video_context_dim), duration=10.0,
                 SOTA_timestamps=[[0.0, 4.0]], SOTA_Prop_score=[0.5]) for _ in range(2)]
    with pytest.raises(_lib.EchrHipError):
        EU.caption_videos(tap, cg, vids, f2t, flag_eval_what='SOTA_TEP')
    with pytest.raises(_lib.EchrHipError):
        EU.caption_videos_beam(tap, cg, vids, f2t, 2, flag_eval_what='SOTA_TEP', ext_seed=3)
    for flag in ('cg_extend', 'gt_tap_cg'):
        with pytest.raises(ValueError, match='SOTA_TEP'):
            EU.caption_videos(tap, cg, vids, f2t, flag_eval_what=flag)
    with pytest.raises(TypeError):
        EU.caption_videos(tap, cg, vids, f2t, None, 1000, 0.0, 0.0, 'SOTA_TEP', 128, 0)          # ext_seed is keyword-only
    with pytest.raises(ValueError, match='go together'):
        EU.caption_video(tap, cg, vids[0]['c3d'], vids[0]['lda'], 10.0, f2t, flag_eval_what='SOTA_TEP')
    with pytest.raises(ValueError, match='go together'):
        EU.caption_video(tap, cg, vids[0]['c3d'], vids[0]['lda'], 10.0, f2t, ext_proposals=([[0.0, 4.0]], [0.5]))
    with pytest.raises(_lib.EchrHipError):
        EU.caption_video(tap, cg, vids[0]['c3d'], vids[0]['lda'], 10.0, f2t, flag_eval_what='SOTA_TEP', ext_proposals=([[0.0, 4.0]], [0.5]))
    assert 'off-by-one' in EU.caption_videos.__doc__ and 'SOTA_TEP' in EU.caption_videos.__doc__

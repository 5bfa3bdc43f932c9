"""Multi-video batches on the host (no GPU): VideoBatch's index arithmetic and validation, the documented refusals, the CPU reference of the
batch contract (tests/vbatch_ref.py) against the reference's own video-by-video run with gradient accumulation
(tests/golden/case_vbatch.npz), the position embedding under a row offset, the ABI additions and the criterion weights of the one-call step."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from echr_amd import synth
from echr_amd.batch import VideoBatch
from oracle import echr_ref_cpu as O
from oracle import summary as SM
from tests import util as U
from tests import vbatch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _videos(name='vbctx'):
    return synth.make_vbatch(name)


# ---- VideoBatch -------------------------------------------------------------------------------------------------------------------
def test_index_arithmetic_and_split():
    opt, params, vids = _videos()
    b = VideoBatch.from_videos(vids)
    V = len(vids)
    assert b.n_videos == V and b.n_events == sum(len(v['soi']) for v in vids)
    assert b.row_offset[0] == 0 and b.event_offset[0] == 0
    assert np.array_equal(np.diff(b.row_offset), [min(len(v['c3d']), len(v['tap'])) for v in vids])
    assert np.array_equal(np.diff(b.event_offset), [len(v['soi']) for v in vids])
    assert b.vid.dtype == np.int32 and np.all(np.diff(b.vid) >= 0) and b.vid[0] == 0 and b.vid[-1] == V - 1
    assert tuple(b.lda.shape) == (V, opt.lda_dim) and b.c3d.shape[0] == b.tap.shape[0] == b.row_offset[-1]
    for v, (vid, s) in enumerate(zip(vids, b.event_slices)):
        r0 = b.row_offset[v]
        assert np.array_equal(b.soi[s] - r0, vid['soi']) and np.array_equal(b.ind[s] - r0, vid['ind'])
        assert np.all(b.vid[s] == v)
        assert np.array_equal(b.c3d[r0:b.row_offset[v + 1]].numpy(), vid['c3d'])
        one = b.video(v)
        assert np.array_equal(one['soi'], vid['soi']) and np.array_equal(one['c3d'].numpy(), vid['c3d'])
    x = torch.arange(b.n_events * 3).reshape(b.n_events, 3)
    parts = b.split(x)
    assert [len(p) for p in parts] == [len(v['soi']) for v in vids] and torch.equal(torch.cat(parts), x)
    with pytest.raises(ValueError):
        b.split(x[:-1])
    # parallel lists are the same batch
    b2 = VideoBatch.from_videos({k: [v[k] for v in vids] for k in ('c3d', 'tap', 'lda', 'ind', 'soi', 'labels', 'masks')})
    assert np.array_equal(b2.soi, b.soi) and torch.equal(b2.labels, b.labels) and torch.equal(b2.masks, b.masks)


def test_features_are_cut_to_the_rows_both_cover():
    opt, params, vids = _videos()
    vids = [dict(v) for v in vids]
    vids[1]['tap'] = np.concatenate([vids[1]['tap'], vids[1]['tap'][:3]])          # three rows more than c3d
    b = VideoBatch.from_videos(vids)
    assert b.row_offset[2] - b.row_offset[1] == len(vids[1]['c3d'])


def test_ragged_label_widths_and_step_counts():
    opt, params, vids = _videos()
    b = VideoBatch.from_videos(vids)
    widths = [v['labels'].shape[1] for v in vids]
    assert len(set(widths)) > 1                                     # the case is ragged
    assert b.labels.shape[1] == max(widths) and b.S == max(b.steps) == O.n_decoder_steps(b.labels.numpy())
    for v, (vid, s) in enumerate(zip(vids, b.event_slices)):
        Sv = O.n_decoder_steps(vid['labels'])
        assert b.steps[v] == Sv
        w = vid['labels'].shape[1]
        assert np.array_equal(b.labels[s, :w].numpy(), vid['labels']) and not b.labels[s, w:].any()
        # the video's mask up to ITS step count, zero behind it: the criterion's normaliser is the per-video one
        assert np.array_equal(b.crit_masks[s, :Sv].numpy(), vid['masks'][:, 1:1 + Sv]) and not b.crit_masks[s, Sv:].any()
        one = b.video(v)
        assert O.n_decoder_steps(one['labels'].numpy()) == Sv


def test_mask_is_cut_to_the_videos_own_step_count():
    """A mask that is non-zero behind the video's last decoder step does not count (LanguageModelCriterion cuts target and mask to the
    log-probs' step count, misc/utils.py:66-75): the stacked mask is zero there."""
    opt, params, vids = _videos()
    vids = [dict(v) for v in vids]
    short = int(np.argmin([v['labels'].shape[1] for v in vids]))
    m = vids[short]['masks'].copy()
    lab = np.concatenate([vids[short]['labels'], np.zeros((len(m), 2), np.int64)], 1)
    vids[short]['labels'], vids[short]['masks'] = lab, np.concatenate([m, np.ones((len(m), 2), np.float32)], 1)
    b = VideoBatch.from_videos(vids)
    s, Sv = b.event_slices[short], b.steps[short]
    assert not b.crit_masks[s, Sv:].any()


def test_value_errors():
    opt, params, vids = _videos()
    with pytest.raises(ValueError):
        VideoBatch.from_videos([])
    bad = [dict(v) for v in vids]
    bad[0]['soi'] = np.zeros((0, 2), np.int64)
    bad[0]['ind'] = np.zeros((0,), np.int64)
    with pytest.raises(ValueError):
        VideoBatch.from_videos(bad)                                  # a video without an event
    bad = [dict(v) for v in vids]
    bad[1]['ind'] = bad[1]['ind'][:-1]
    with pytest.raises(ValueError):
        VideoBatch.from_videos(bad)                                  # ind / soi lengths
    bad = [dict(v) for v in vids]
    bad[1]['soi'] = bad[1]['soi'].copy()
    bad[1]['soi'][0, 1] = len(bad[1]['c3d']) + 1
    with pytest.raises(ValueError):
        VideoBatch.from_videos(bad)                                  # an event beyond ITS video's rows (the next video's rows would cover it)
    bad = [dict(v) for v in vids]
    bad[0]['soi'] = bad[0]['soi'].copy()
    bad[0]['soi'][0] = [3, 3]
    with pytest.raises(ValueError):
        VideoBatch.from_videos(bad)                                  # an empty event
    bad = [dict(v) for v in vids]
    bad[2]['lda'] = bad[2]['lda'][:-1]
    with pytest.raises(ValueError):
        VideoBatch.from_videos(bad)                                  # feature widths
    bad = [dict(v) for v in vids]
    del bad[3]['labels']
    with pytest.raises(ValueError):
        VideoBatch.from_videos(bad)                                  # labels for some videos only
    bad = [dict(v) for v in vids]
    bad[3]['labels'] = bad[3]['labels'][:-1] if len(bad[3]['labels']) > 1 else np.concatenate([bad[3]['labels']] * 2)
    with pytest.raises(ValueError):
        VideoBatch.from_videos(bad)                                  # label rows
    bad = [dict(v) for v in vids]
    del bad[0]['tap']
    with pytest.raises(ValueError):
        VideoBatch.from_videos(bad)
    # the layout contract: events of a video contiguous, videos in order
    b = VideoBatch.from_videos(vids)
    b.vid = b.vid[::-1].copy()
    with pytest.raises(ValueError):
        b.validate()
    b = VideoBatch.from_videos(vids)
    b.vid = b.vid.copy()
    b.vid[0], b.vid[-1] = b.vid[-1], b.vid[0]
    with pytest.raises(ValueError):
        b.validate()
    b = VideoBatch.from_videos(vids)
    b.ind = b.ind.copy()
    b.ind[0] = b.row_offset[1]                                       # an anchor inside the NEXT video
    with pytest.raises(ValueError):
        b.validate()
    nolab = VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi')} for v in vids])
    assert nolab.labels is None
    with pytest.raises(ValueError):
        nolab.criterion(O.lm_criterion, torch.zeros(nolab.n_events, 2, 5))


def test_single_video_batch_is_the_video():
    opt, params, vid = synth.make_case('tiny')
    b = VideoBatch.from_videos([vid])
    assert b.n_videos == 1 and np.array_equal(b.soi, vid['soi']) and np.array_equal(b.ind, vid['ind']) and not b.vid.any()
    assert torch.equal(b.labels, torch.from_numpy(vid['labels'])) and b.S == O.n_decoder_steps(vid['labels'])


# ---- documented refusals ----------------------------------------------------------------------------------------------------------
def _model(**over):
    import echr_amd
    opt, params, vids = _videos()
    for k, v in over.items():
        setattr(opt, k, v)
    return echr_amd.CaptionGenerator(opt), VideoBatch.from_videos(vids)


def test_forward_batch_refusals():
    m, b = _model()
    with pytest.raises(NotImplementedError):
        m.forward_batch(b, mode='train_rl')
    with pytest.raises(NotImplementedError):
        m.forward_batch(b, mode='eval', beam_size=3)
    with pytest.raises(NotImplementedError):
        m.forward_batch(b, mode='sample')
    m, b = _model(CG_init_feats_type='V')
    with pytest.raises(NotImplementedError):
        m.forward_batch(b, mode='train')
    m, b = _model(CG_init_feats_type='VEC')
    with pytest.raises(NotImplementedError):
        m.forward_batch(b, mode='eval')
    for ct in ('CH', 'CC+CH'):
        m, b = _model(clip_context_type=ct)
        with pytest.raises(NotImplementedError):
            m.forward_batch(b, mode='train')
    # a model whose arena hands gradients to the data-parallel reducer from inside the backward pass (one video per rank and call)
    from types import SimpleNamespace
    m, b = _model()
    m._echr_arena = SimpleNamespace(early_grad_hook=lambda *a, **k: None, early_reducer=None)
    with pytest.raises(NotImplementedError):
        m.forward_batch(b, mode='train')


def test_step_refusals():
    from echr_amd.fused import DataParallelStep, FusedTrainStep, JointTrainStep, SelfCriticalStep
    m, b = _model()
    for cls in (SelfCriticalStep, JointTrainStep, DataParallelStep):
        with pytest.raises(NotImplementedError):
            object.__new__(cls).batch(b)
    f = object.__new__(FusedTrainStep)
    for kw in (dict(tap_grad=torch.zeros(1)), dict(defer_update=True), dict(prepared=True), dict(handover=True)):
        with pytest.raises(NotImplementedError):
            f.batch(b, **kw)
    with pytest.raises(NotImplementedError):
        f.prepare(b, None, None, None, None, None, None)
    # option refusals reach the one-call step as well
    f.model, _ = _model(CG_init_feats_type='V')
    with pytest.raises(NotImplementedError):
        f.batch(b)
    f.model, _ = _model(clip_context_type='CH')
    with pytest.raises(NotImplementedError):
        f.batch(b)


# ---- the contract against the reference -------------------------------------------------------------------------------------------
TOL_LOGP, TOL_LOSS, TOL_GRAD = 2e-5, 1e-5, 1e-5


@pytest.mark.parametrize('case', ['vbctx', 'vb16'])
@pytest.mark.parametrize('train_mode', [False, True])
def test_vbatch_ref_matches_the_reference_fixture(case, train_mode):
    """Sum, no 1/V, per-video normaliser, gradient accumulation over the videos: the reference's own numbers."""
    g = U.gold('case_vbatch.npz')
    opt, params, vids = synth.make_vbatch(case)
    ref = R.run(opt, params, vids, train_mode)
    key = case + '|' + ('train' if train_mode else 'eval')
    cols = SM.logp_columns(opt.CG_vocab_size + 1)
    for v, lp in enumerate(ref['logp']):
        assert np.abs(lp[:, :, cols] - g[key + '|logp|v%02d' % v]).max() < TOL_LOGP, v
    assert np.abs(ref['losses'] - g[key + '|losses']).max() < TOL_LOSS * np.abs(g[key + '|losses']).max()
    assert abs(ref['loss'] - float(g[key + '|loss'])) < TOL_LOSS * abs(float(g[key + '|loss']))
    assert abs(float(g[key + '|loss']) - g[key + '|losses'].sum()) < 1e-12 * len(vids) * abs(float(g[key + '|loss']))          # the SUM
    for k, gr in ref['grads'].items():
        if gr is None or k in U.NOISE_ONLY:
            continue
        linf = float(g[key + '|grad|' + k + '|linf'])
        head, strided = SM.grad_slices(gr)
        for got, want in ((head, g[key + '|grad|' + k + '|head']), (strided, g[key + '|grad|' + k + '|strided'])):
            assert np.abs(got - want).max() <= 1e-4 * max(linf, U.GRAD_FLOOR) + 1e-9, k          # (the oracle-vs-reference bar of tools/make_golden*.py)


def test_reference_greedy_margin_is_recorded():
    g = U.gold('case_vbatch.npz')
    for case in ('vb16', 'vbctx'):
        assert float(g[case + '|sample|min_margin']) > 2e-5


def test_position_embedding_is_unchanged_by_a_row_offset():
    """Contract point 4: batch-absolute row indices give the per-video position embedding bit for bit (centre differences and length
    ratios are differences / ratios of integers + 0.5 in float64)."""
    opt, params, vids = synth.make_vbatch('vb16')
    b = VideoBatch.from_videos(vids)
    for v, (vid, s) in enumerate(zip(vids, b.event_slices)):
        pm_local, pm_abs = O.position_matrix(vid['soi']), O.position_matrix(b.soi[s])
        assert np.array_equal(pm_local, pm_abs), v
        assert np.array_equal(O.position_embedding(pm_local, opt.d_feats), O.position_embedding(pm_abs, opt.d_feats)), v
    # and the block of the whole batch's matrix that belongs to a video is that video's matrix
    full = O.position_embedding(O.position_matrix(b.soi), opt.d_feats)
    for vid, s in zip(vids, b.event_slices):
        assert np.array_equal(full[s, s], O.position_embedding(O.position_matrix(vid['soi']), opt.d_feats))


# ---- ABI --------------------------------------------------------------------------------------------------------------------------
def test_abi_additions():
    from echr_amd import _lib
    lib = _lib.load()
    assert lib.echr_abi_sizeof(b'echr_batch_ext') == C.sizeof(_lib.BatchExt) == 40
    assert lib.echr_version() == _lib.ABI_VERSION == 3
    assert lib.echr_batch_ws_floats(12, 5, 32) >= (12 + 2 * 5) * 4 * 32 and lib.echr_batch_ws_floats(4, 5, 32) == -1
    new = ['echr_batch_ws_floats', 'echr_seg_col_mean_fwd', 'echr_seg_col_mean_bwd', 'echr_tsrm_fwd_batch', 'echr_tsrm_bwd_batch', 'echr_decoder_fwd_batch',
           'echr_decoder_bwd_batch', 'echr_decoder_sample_batch', 'echr_train_step_batch_ws_floats', 'echr_train_step_batch']
    bound = {s[0] for s in _lib.SYMBOLS}
    hdr = open(os.path.join(ROOT, 'include', 'echr_hip.h')).read()
    for name in new:
        assert name in bound and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    # the existing structs keep their sizes (no field was added to them)
    for cname, cls in _lib.ABI_STRUCTS.items():
        assert lib.echr_abi_sizeof(cname.encode()) == C.sizeof(cls), cname
    assert lib.echr_abi_sizeof(b'echr_train_step_args') == C.sizeof(_lib.TrainStepArgs)


# ---- the one-call step's criterion weights ----------------------------------------------------------------------------------------
def test_criterion_weights_carry_the_per_video_normalisers():
    opt, params, vids = synth.make_vbatch('vbctx')
    b = VideoBatch.from_videos(vids)
    w = b.criterion_weights()
    assert w.dtype == np.float32 and w.shape == (b.n_events, b.S)
    for vid, s, Sv in zip(vids, b.event_slices, b.steps):
        mk = vid['masks'][:, 1:1 + Sv].astype(np.float32)
        want = mk / (np.float32(mk.sum()) + np.float32(1e-6))
        assert np.array_equal(w[s, :Sv], want) and not w[s, Sv:].any()
    # sum(-logp[target] * w) IS the sum of the per-video criteria, and criterion() returns both
    rs = np.random.RandomState(0)
    V1 = opt.CG_vocab_size + 1
    logp = torch.log_softmax(torch.from_numpy(rs.standard_normal((b.n_events, b.S, V1)).astype(np.float32)), 2)
    total, per = b.criterion(O.lm_criterion, logp)
    want = [float(O.lm_criterion(logp[s, :Sv], torch.from_numpy(v['labels'])[:, 1:], torch.from_numpy(v['masks'])[:, 1:]))
            for v, s, Sv in zip(vids, b.event_slices, b.steps)]
    assert np.allclose(per.numpy(), want, rtol=1e-6, atol=0) and abs(float(total) - sum(want)) < 1e-5 * sum(want)
    tg = b.targets[:, :b.S].numpy()
    nll = -np.take_along_axis(logp.numpy(), tg[:, :, None], 2)[:, :, 0]
    assert abs(float((nll.astype(np.float64) * w).sum()) - sum(want)) < 1e-5 * sum(want)

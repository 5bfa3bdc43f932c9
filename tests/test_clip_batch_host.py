"""Frame-level contexts 'CH' / 'CC+CH' over a multi-video batch, host side (no GPU): the VideoBatch keyword, the mismatch rules of the batched
entry points, the CPU reference of the contract (tests/clip_batch_ref.py) against the reference's own fixture
(tests/golden/case_clip_batch.npz), and the C ABI's new symbols."""
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import echr_amd
from echr_amd import functional as EF
from echr_amd import synth
from echr_amd.batch import VideoBatch
from oracle import summary as SM
from tests import clip_batch_ref as R
from tests import util as U

TOL_LOGP, TOL_LOSS, TOL_GRAD = 2e-5, 1e-5, 1e-5


def _videos(case='vbch'):
    return synth.make_vbatch(case)


# ---- VideoBatch -------------------------------------------------------------------------------------------------------------------
def test_clip_context_keyword_and_clip_parts():
    opt, params, vids = _videos()
    assert list(inspect.signature(VideoBatch.from_videos).parameters)[-1] == 'clip_context_type'
    assert list(inspect.signature(VideoBatch.__init__).parameters)[-1] == 'clip_context_type'
    assert VideoBatch.from_videos(vids).clip_parts == 1 and VideoBatch.from_videos(vids).clip_context_type == 'CC'
    for ct, parts in (('CC', 1), ('CH', 2), ('CC+CH', 3), ('CCCH', 3)):
        b = VideoBatch.from_videos(vids, clip_context_type=ct)          # fails on the parent commit: no such keyword
        assert b.clip_parts == parts and b.clip_context_type == ct
    with pytest.raises(ValueError):
        VideoBatch.from_videos(vids, clip_context_type='EC')
    b = VideoBatch.from_videos(vids, clip_context_type='CH')
    assert b.clip_rows() is b.tap and b.clip_col0 == 0
    b1 = VideoBatch.from_videos(vids)
    assert b1.clip_rows() is b1.c3d
    assert VideoBatch.from_videos(vids, clip_context_type='CC+CH').clip_col0 == opt.video_dim


def test_video_round_trip_carries_the_setting():
    opt, params, vids = _videos()
    b = VideoBatch.from_videos(vids, clip_context_type='CC+CH')
    ones = [b.video(v) for v in range(b.n_videos)]
    assert all(o['clip_context_type'] == 'CC+CH' for o in ones)
    for o, vid in zip(ones, vids):
        assert np.array_equal(o['soi'], vid['soi']) and np.array_equal(o['tap'].numpy(), vid['tap'])
    b2 = VideoBatch.from_videos(ones, clip_context_type=ones[0]['clip_context_type'])
    assert b2.clip_parts == 3 and np.array_equal(b2.soi, b.soi) and np.array_equal(b2.row_offset, b.row_offset)
    assert torch.equal(b2.labels, b.labels) and torch.equal(b2.masks, b.masks) and torch.equal(b2.tap, b.tap)


def test_cases_are_ragged():
    """The shapes the GPU tests rely on: a one-event video, label widths and step counts that differ between videos, captions that end at
    different steps, at most 16 events; vbch33 has 132 rows."""
    for case in ('vbch', 'vbcch'):
        opt, params, vids = _videos(case)
        b = VideoBatch.from_videos(vids, clip_context_type=opt.clip_context_type)
        assert b.n_videos == 5 and b.n_events <= 16 and 1 in [len(v['soi']) for v in vids]
        assert len(set(b.steps)) > 1 and len({v['labels'].shape[1] for v in vids}) > 1
        assert len(set((b.crit_masks.numpy() != 0).sum(1).tolist())) > 2
        assert opt.video_context_type == 'VLVCVH' and opt.event_context_type == 'ER3'
    opt, params, vids = _videos('vbch33')
    assert sum(len(v['soi']) for v in vids) == 132 and opt.clip_context_type == 'CH'


# ---- the contract against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['vbch', 'vbcch'])
@pytest.mark.parametrize('train_mode', [False, True])
def test_clip_batch_ref_matches_the_reference_fixture(case, train_mode):
    g = U.gold('case_clip_batch.npz')
    opt, params, vids = _videos(case)
    ref = R.run(opt, params, vids, train_mode)
    key = case + '|' + ('train' if train_mode else 'eval')
    cols, tcols = SM.logp_columns(opt.CG_vocab_size + 1), SM.logp_columns(opt.hidden_dim)
    for v, lp in enumerate(ref['logp']):
        assert np.abs(lp[:, :, cols] - g[key + '|logp|v%02d' % v]).max() < TOL_LOGP, v
        want = g[key + '|gtap|v%02d' % v]
        scale = max(float(np.abs(want).max()), U.GRAD_FLOOR)
        assert np.abs(ref['g_tap'][v][:, tcols] - want).max() <= TOL_GRAD * scale + 1e-9, v
        l2 = float(g[key + '|gtap_l2|v%02d' % v])
        assert abs(float(np.sqrt((ref['g_tap'][v].astype(np.float64) ** 2).sum())) - l2) <= TOL_GRAD * l2
    assert np.abs(ref['losses'] - g[key + '|losses']).max() < TOL_LOSS * np.abs(g[key + '|losses']).max()
    assert abs(ref['loss'] - float(g[key + '|loss'])) < TOL_LOSS * abs(float(g[key + '|loss']))
    for k, gr in ref['grads'].items():
        if gr is None or k in U.NOISE_ONLY:
            continue
        linf = float(g[key + '|grad|' + k + '|linf'])
        head, strided = SM.grad_slices(gr)
        for a, want in ((head, g[key + '|grad|' + k + '|head']), (strided, g[key + '|grad|' + k + '|strided'])):
            assert np.abs(a - want).max() <= TOL_GRAD * max(linf, U.GRAD_FLOOR) + 1e-9, k


@pytest.mark.parametrize('case', ['vbch', 'vbcch'])
def test_clip_batch_ref_greedy_matches_the_reference_fixture(case):
    g = U.gold('case_clip_batch.npz')
    opt, params, vids = _videos(case)
    assert float(g[case + '|sample|min_margin']) > 2e-5
    for v, (seq, lp) in enumerate(R.sample(opt, params, vids)):
        assert np.array_equal(seq.numpy(), g[case + '|sample|seq|v%02d' % v]), v
        assert np.abs(lp.numpy() - g[case + '|sample|logp|v%02d' % v]).max() < TOL_LOGP, v


# ---- option rules -----------------------------------------------------------------------------------------------------------------
def _model(clip='CH', **over):
    opt, params, vids = _videos()
    opt.clip_context_type = clip
    for k, v in over.items():
        setattr(opt, k, v)
    return echr_amd.CaptionGenerator(opt), vids


def _entries(m, b):
    return (lambda: m.forward_batch(b, mode='train'), lambda: m.forward_batch(b, mode='eval'), lambda: m.beam_batch(b, 3),
            lambda: m.train_rl_batch(b))


def test_plain_batch_with_a_ch_model_names_the_keyword():
    for ct in ('CH', 'CC+CH'):
        m, vids = _model(ct)
        m.eval()
        b = VideoBatch.from_videos(vids)
        for call in _entries(m, b):
            with pytest.raises(NotImplementedError, match='clip_context_type='):
                call()


def test_other_mismatches_are_value_errors():
    m, vids = _model('CC')
    m.eval()
    for ct in ('CH', 'CC+CH'):
        b = VideoBatch.from_videos(vids, clip_context_type=ct)
        for call in _entries(m, b):
            with pytest.raises(ValueError):
                call()
    m, vids = _model('CC+CH')
    with pytest.raises(ValueError):
        m.forward_batch(VideoBatch.from_videos(vids, clip_context_type='CH'), mode='train')
    # the one-call steps apply the same rule
    from echr_amd.fused import FusedTrainStep, JointBatchStep
    f = object.__new__(FusedTrainStep)
    f.model, _ = _model('CC')
    with pytest.raises(ValueError):
        f.batch(VideoBatch.from_videos(vids, clip_context_type='CH'))
    s = object.__new__(JointBatchStep)
    s.fused, s.lib, s.tap_model = f, None, None
    with pytest.raises(ValueError):
        s(VideoBatch.from_videos(vids, clip_context_type='CH'), None, None, None)


def test_matching_batch_on_cpu_tensors_fails_like_every_other_mode():
    for ct in ('CH', 'CC+CH', 'CCCH'):
        m, vids = _model(ct)
        m.eval()
        b = VideoBatch.from_videos(vids, clip_context_type=ct)
        for call in _entries(m, b):
            with pytest.raises(EF.L.EchrHipError):
                call()


def test_init_state_and_data_parallel_refusals_hold_with_a_matching_batch():
    m, vids = _model('CH', CG_init_feats_type='V')
    b = VideoBatch.from_videos(vids, clip_context_type='CH')
    for call in _entries(m, b)[:2]:
        with pytest.raises(NotImplementedError, match='CG_init_feats_type'):
            call()
    m, vids = _model('CH')
    m._echr_arena = SimpleNamespace(early_grad_hook=lambda *a, **k: None, early_reducer=None)
    with pytest.raises(NotImplementedError, match='data-parallel'):
        m.forward_batch(b, mode='train')


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exist_and_are_bound():
    from echr_amd import _lib as L
    lib = L.load()
    names = [s[0] for s in L.SYMBOLS]
    for name in ('echr_train_step_batch_clip_ws_floats', 'echr_train_step_batch_clip'):
        assert name in names and hasattr(lib, name)
    assert L.ABI_VERSION == 3
    assert lib.echr_train_step_batch_clip_ws_floats(None, None, None) == -1
    assert lib.echr_config_set(b'row_grad_list', 0) == 0 and lib.echr_config_set(b'row_grad_list', 1) == 0

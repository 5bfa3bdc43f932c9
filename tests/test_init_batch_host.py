"""The non-zero initial decoder state (CG_init_feats_type) over a multi-video batch, host side (no GPU): the VideoBatch keyword, the
refusal / mismatch rules of the batched entry points and one-call steps, the CPU reference of the contract (tests/init_batch_ref.py)
against the reference's own fixture (tests/golden/case_init_batch.npz), the guard that the cases can tell a batch-wide divisor of the
clip mean from the per-video one, and the C ABI's new symbols."""
import inspect

import numpy as np
import pytest
import torch

import echr_amd
from echr_amd import synth
from echr_amd.batch import VideoBatch
from oracle import summary as SM
from tests import init_batch_ref as R
from tests import util as U

TOL_LOGP, TOL_LOSS, TOL_GRAD = 2e-5, 1e-5, 1e-5


def _videos(case='vbinit'):
    return synth.make_vbatch(case)


# ---- VideoBatch -------------------------------------------------------------------------------------------------------------------
def test_keyword_round_trips_through_from_videos_video_and_the_groups():
    opt, params, vids = _videos()
    assert 'CG_init_feats_type' in inspect.signature(VideoBatch.from_videos).parameters
    assert 'CG_init_feats_type' in inspect.signature(VideoBatch.__init__).parameters
    assert VideoBatch.from_videos(vids).CG_init_feats_type == ''
    for t in ('V', 'E', 'C', 'VE', 'VEC'):
        b = VideoBatch.from_videos(vids, CG_init_feats_type=t)          # fails on the parent commit: no such keyword
        assert b.CG_init_feats_type == t and b.clip_parts == 1
    for bad in ('VX', 'CC', 'VEV'):          # unknown letters, repeated letters ('CC' is a clip context, not an initial state)
        with pytest.raises(ValueError):
            VideoBatch.from_videos(vids, CG_init_feats_type=bad)
    # both options are keyword-only: a positional value cannot land in the wrong one
    kinds = inspect.signature(VideoBatch.from_videos).parameters
    assert kinds['CG_init_feats_type'].kind is inspect.Parameter.KEYWORD_ONLY and kinds['clip_context_type'].kind is inspect.Parameter.KEYWORD_ONLY
    with pytest.raises(TypeError):
        VideoBatch.from_videos(vids, None, None, None, 'CH')
    b = VideoBatch.from_videos(vids, CG_init_feats_type='VEC', clip_context_type='CC')
    ones = [b.video(v) for v in range(b.n_videos)]
    assert all(o['CG_init_feats_type'] == 'VEC' and o['clip_context_type'] == 'CC' for o in ones)
    b2 = VideoBatch.from_videos(ones, CG_init_feats_type=ones[0]['CG_init_feats_type'])
    assert b2.CG_init_feats_type == 'VEC' and np.array_equal(b2.soi, b.soi) and torch.equal(b2.labels, b.labels)
    # the group helpers cut the video axis of the SAME batch: the setting is the batch's
    assert b.event_groups(4)[0][0] == 0 and b.beam_groups(3, 12)[-1][1] == b.n_videos and b.CG_init_feats_type == 'VEC'
    # the direct constructor takes it too
    b3 = VideoBatch(b.c3d, b.tap, b.lda, b.row_offset, b.event_offset, b.soi, b.ind, b.labels, b.masks, CG_init_feats_type='VE')
    assert b3.CG_init_feats_type == 'VE'


def test_cases_have_the_shapes_the_gpu_tests_rely_on():
    """5 videos incl. a one-event video, ragged label widths, at most 16 events (<= 64 rows: a zero-state batch would go persistent);
    the per-video longest events differ, and the longest of the batch sits in a one-event video, so EVERY multi-event video has a
    padded clip length below the batch-wide one; vbinit33 has 132 rows."""
    for case, init, clip in (('vbinit', 'VEC', 'CC'), ('vbinitch', 'VE', 'CH')):
        opt, params, vids = _videos(case)
        b = VideoBatch.from_videos(vids, CG_init_feats_type=opt.CG_init_feats_type, clip_context_type=opt.clip_context_type)
        assert opt.CG_init_feats_type == init and opt.clip_context_type == clip
        assert b.n_videos == 5 and b.n_events <= 16 and 1 in [len(v['soi']) for v in vids]
        assert len(set(b.steps)) > 1 and len({v['labels'].shape[1] for v in vids}) > 1
        assert opt.video_context_type == 'VLVCVH' and opt.event_context_type == 'ER3'
        assert 'lm_model.init_linear.weight' in params
    opt, params, vids = _videos('vbinit')
    lens = R.video_max_len(vids)
    assert len(set(lens.tolist())) == len(vids), lens
    assert len(vids[int(np.argmax(lens))]['soi']) == 1
    assert np.array_equal(lens, U.gold('case_init_batch.npz')['vbinit|video_len'])
    opt, params, vids = _videos('vbinit33')
    assert sum(len(v['soi']) for v in vids) == 132 and opt.CG_init_feats_type == 'VEC' and opt.clip_context_type == 'CC'
    assert len(set(R.video_max_len(vids).tolist())) > 8


# ---- the contract against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['vbinit', 'vbinitch'])
@pytest.mark.parametrize('train_mode', [False, True])
def test_init_batch_ref_matches_the_reference_fixture(case, train_mode):
    g = U.gold('case_init_batch.npz')
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
    assert ref['grads']['lm_model.init_linear.weight'] is not None and (key + '|grad|lm_model.init_linear.weight|linf') in g
    for k, gr in ref['grads'].items():
        if gr is None or k in U.NOISE_ONLY:
            continue
        linf = float(g[key + '|grad|' + k + '|linf'])
        head, strided = SM.grad_slices(gr)
        for a, want in ((head, g[key + '|grad|' + k + '|head']), (strided, g[key + '|grad|' + k + '|strided'])):
            assert np.abs(a - want).max() <= TOL_GRAD * max(linf, U.GRAD_FLOOR) + 1e-9, k


@pytest.mark.parametrize('case', ['vbinit', 'vbinitch'])
def test_init_batch_ref_greedy_matches_the_reference_fixture(case):
    g = U.gold('case_init_batch.npz')
    opt, params, vids = _videos(case)
    assert float(g[case + '|sample|min_margin']) > 2e-5
    for v, (seq, lp) in enumerate(R.sample(opt, params, vids)):
        assert np.array_equal(seq.numpy(), g[case + '|sample|seq|v%02d' % v]), v
        assert np.abs(lp.numpy() - g[case + '|sample|logp|v%02d' % v]).max() < TOL_LOGP, v


def test_vbinit33_has_one_right_greedy_sequence():
    """vbinit33 is compared against the oracle only: its own greedy decode is decided by more than the log-prob tolerance at every step."""
    opt, params, vids = _videos('vbinit33')
    assert R.greedy_margin(opt, params, vids) > TOL_LOGP


@pytest.mark.parametrize('train_mode', [False, True])
def test_a_batch_wide_divisor_is_far_outside_the_tolerance(train_mode):
    """The guard that the case can detect the wrong divisor: the clip mean over the BATCH's longest event instead of the video's own moves
    the log-probs of every multi-event video of vbinit by more than 100 x 2e-5."""
    opt, params, vids = _videos('vbinit')
    good = R.run(opt, params, vids, train_mode, backward=False)
    bad = R.run(opt, params, vids, train_mode, backward=False, batch_wide_divisor=True)
    multi = [v for v, vid in enumerate(vids) if len(vid['soi']) > 1]
    assert len(multi) >= 3
    for v in multi:
        d = float(np.abs(good['logp'][v] - bad['logp'][v]).max())
        print('video %d (%d events, padded length %d): %.3f' % (v, len(vids[v]['soi']), R.video_max_len(vids)[v], d))
        assert d > 100 * TOL_LOGP, (v, d)


# ---- option rules -----------------------------------------------------------------------------------------------------------------
def _model(init='VEC', clip='CC', **over):
    opt, params, vids = _videos()
    opt.CG_init_feats_type, opt.clip_context_type = init, clip
    for k, v in over.items():
        setattr(opt, k, v)
    return echr_amd.CaptionGenerator(opt), vids


def _entries(m, b):
    return (lambda: m.forward_batch(b, mode='train'), lambda: m.forward_batch(b, mode='eval'), lambda: m.beam_batch(b, 3),
            lambda: m.train_rl_batch(b))


def _steps(m):
    """The three one-call steps around `m`, as far as the option check needs them (it runs ahead of everything that touches the device)."""
    from echr_amd import functional as EF
    from echr_amd.fused import FusedTrainStep, JointBatchStep, SelfCriticalBatchStep
    f = object.__new__(FusedTrainStep)
    f.model, f.lib = m, EF.L.load()
    s = object.__new__(JointBatchStep)
    s.fused, s.lib, s.tap_model = f, None, None
    sc = SelfCriticalBatchStep(f)
    return f, s, sc


def test_plain_batch_with_an_init_model_names_the_keyword():
    for init in ('V', 'VEC'):
        m, vids = _model(init)
        m.eval()
        b = VideoBatch.from_videos(vids)
        for call in _entries(m, b):
            with pytest.raises(NotImplementedError, match='CG_init_feats_type='):
                call()
        f, s, sc = _steps(m)
        with pytest.raises(NotImplementedError, match='CG_init_feats_type='):
            f.batch(b)
        with pytest.raises(NotImplementedError, match='CG_init_feats_type='):
            f.batch_handover(b)
        with pytest.raises(NotImplementedError, match='CG_init_feats_type='):
            s(b, None, None, None)
        with pytest.raises(NotImplementedError, match='CG_init_feats_type='):
            sc(b)
    # the clip one-call step ('VE' over 'CH' rows: echr_train_step_batch_clip) applies the rule to both keywords
    m, vids = _model('VE', 'CH')
    f, s, sc = _steps(m)
    for b in (VideoBatch.from_videos(vids), VideoBatch.from_videos(vids, clip_context_type='CH')):
        for call in (lambda: f.batch(b), lambda: s(b, None, None, None), lambda: sc(b)):
            with pytest.raises(NotImplementedError, match='CG_init_feats_type='):
                call()
    with pytest.raises(NotImplementedError, match='clip_context_type='):
        f.batch(VideoBatch.from_videos(vids, CG_init_feats_type='VE'))


def test_other_mismatches_are_value_errors():
    m, vids = _model('')
    m.eval()
    b = VideoBatch.from_videos(vids, CG_init_feats_type='VEC')
    for call in _entries(m, b):
        with pytest.raises(ValueError):
            call()
    f, s, sc = _steps(m)
    with pytest.raises(ValueError):
        f.batch(b)
    with pytest.raises(ValueError):
        s(b, None, None, None)
    with pytest.raises(ValueError):
        sc(b)
    m, vids = _model('VE', 'CH')          # the clip one-call step
    f, s, sc = _steps(m)
    for bad in (VideoBatch.from_videos(vids, CG_init_feats_type='V', clip_context_type='CH'),
                VideoBatch.from_videos(vids, CG_init_feats_type='VE', clip_context_type='CC+CH')):
        for call in (lambda: f.batch(bad), lambda: s(bad, None, None, None), lambda: sc(bad)):
            with pytest.raises(ValueError):
                call()
    m, vids = _model('VE')
    m.eval()
    for call in _entries(m, VideoBatch.from_videos(vids, CG_init_feats_type='VEC')):
        with pytest.raises(ValueError):
            call()
    f, s, sc = _steps(m)
    with pytest.raises(ValueError):
        f.batch(VideoBatch.from_videos(vids, CG_init_feats_type='V'))
    with pytest.raises(ValueError):
        sc(VideoBatch.from_videos(vids, CG_init_feats_type='V'))


def test_matching_batch_passes_the_option_check_and_fails_on_cpu_tensors_like_every_other_mode():
    from echr_amd import functional as EF
    for init in ('V', 'VEC', 'CEV'):
        m, vids = _model(init)
        m.eval()
        b = VideoBatch.from_videos(vids, CG_init_feats_type='VEC' if init == 'CEV' else init)
        m._check_batch_options(b)          # fails on the parent commit: NotImplementedError
        for call in _entries(m, b):
            with pytest.raises(EF.L.EchrHipError):
                call()


def test_clip_mean_with_ch_rows_keeps_the_constructors_refusal():
    with pytest.raises(NotImplementedError):
        _model('C', 'CH')
    with pytest.raises(NotImplementedError):
        _model('VEC', 'CC+CH')


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exist_and_are_bound():
    from echr_amd import _lib as L
    lib = L.load()
    names = [s[0] for s in L.SYMBOLS]
    for name in ('echr_init_state_fwd_batch', 'echr_init_state_bwd_batch'):
        assert name in names and hasattr(lib, name)
    assert L.ABI_VERSION == 3 and lib.echr_version() == 3
    assert lib.echr_init_state_fwd_batch(None, None, None, None) != 0
    assert lib.echr_init_state_bwd_batch(None, None, None, None) != 0
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'echr_hip.h')).read()
    assert 'int echr_init_state_fwd_batch(' in header and 'int echr_init_state_bwd_batch(' in header

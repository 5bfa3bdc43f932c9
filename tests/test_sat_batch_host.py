"""CPU: the one-stream decoder over multi-video batches -- tests/sat_batch_ref.py against the fixture the reference itself produced
(tools/make_golden_sat_batch.py -> tests/golden/case_sat_batch.npz), the C ABI of the batch entries of csrc/sat.hip (host functions and
argument checks only), the refusal matrix of the batch's `caption_model` keyword, and the conditions on the inputs of the GPU tests' greedy
cases (tests/test_gpu_sat_batch.py): float64 margins that leave at least 90 % of the decoded positions resolvable at 1e-4."""
import ctypes as C

import numpy as np
import pytest
import torch

import echr_amd
from echr_amd import _lib as L
from echr_amd import sat, synth
from echr_amd.batch import VideoBatch
from oracle import summary as SM
from tests import sat_batch_ref as B
from tests import sat_ref as R
from tests import util as U

TOL = 1e-5          # sat_batch_ref in float32 against the reference's float32 run (relative), as tests/test_sat_host.py
MARGIN, SHARE = 1e-4, 0.9
SAT = 'show_attend_tell'


# ---- the fixture --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_sat_batch_ref_reproduces_the_full_fixture(mode):
    g = U.gold('case_sat_batch.npz')
    opt, params, videos = B.make_case('fixture')
    got = B.run(opt, params, videos, mode == 'train')
    key = 'fixture|' + mode
    assert abs(got['loss'] - float(g[key + '|loss'])) < TOL * abs(got['loss']) and U.relerr(got['losses'], g[key + '|losses']) < TOL
    assert abs(got['loss'] - float(g[key + '|losses'].sum())) < TOL * abs(got['loss'])          # the sum over the videos, no 1/V
    for v in range(len(videos)):
        assert got['logp'][v].shape == g['%s|logp|%d' % (key, v)].shape
        assert U.relerr(got['logp'][v], g['%s|logp|%d' % (key, v)]) < TOL
        assert U.relerr(got['g_tap'][v], g['%s|gtap|%d' % (key, v)], U.GRAD_FLOOR) < TOL
    for k, x in got['grads'].items():
        ref = g.get(key + '|grad|' + k)
        if ref is None:
            assert x is None, k
        elif k in R.NOISE_ONLY:
            assert float(np.abs(x).max()) < 1e-6 and float(np.abs(ref).max()) < 1e-6
        else:
            assert U.relerr(x, ref, U.GRAD_FLOOR) < TOL, k
    if mode == 'train':          # the masks are the batch-global ones: a video's own [N_v, H] masks give another loss
        own = sum(R.run(opt, params, vid, True, backward=False)[1] for vid in videos)
        assert abs(own - got['loss']) > 1e-4 * abs(got['loss'])


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_sat_batch_ref_reproduces_the_summaries(mode):
    g = U.gold('case_sat_batch.npz')
    opt, params, videos = B.make_case('widths')
    assert opt.CG_rnn_size == 512 and opt.video_dim == 500
    got = B.run(opt, params, videos, mode == 'train')
    key = 'widths|' + mode
    assert abs(got['loss'] - float(g[key + '|loss'])) < TOL * abs(got['loss']) and U.relerr(got['losses'], g[key + '|losses']) < TOL
    for v in range(len(videos)):
        s = SM.summarize_logp(got['logp'][v])
        pre = '%s|logp|%d|' % (key, v)
        assert U.relerr(s['slice'], g[pre + 'slice']) < TOL and np.array_equal(s['shape'], g[pre + 'shape'])
        safe = g[pre + 'margin'] > MARGIN
        assert np.array_equal(s['argmax'][safe], g[pre + 'argmax'][safe])
        for k, x in SM.summarize_grads({'tap': got['g_tap'][v]}).items():
            part = k.split('|', 1)[1]
            assert U.relerr(x, g['%s|gtap|%d|%s' % (key, v, part)], U.GRAD_FLOOR) < TOL, (v, part)
    for k, x in SM.summarize_grads(got['grads']).items():
        ref = g[key + '|grad|' + k]
        if k.split('|')[0] in R.NOISE_ONLY:
            assert float(np.abs(x).max()) < 1e-6 and float(np.abs(ref).max()) < 1e-6
            continue
        pname, part = k.split('|')
        scale = max(abs(float(ref)) if part in ('l2', 'linf') else float(g[key + '|grad|' + pname + '|linf']), U.GRAD_FLOOR)
        assert float(np.abs(np.asarray(x, np.float64) - ref).max()) < TOL * scale, k


def test_sat_batch_ref_greedy_reproduces_the_fixture():
    g = U.gold('case_sat_batch.npz')
    opt, params, videos = B.make_case('fixture')
    per = B.sample(opt, params, videos)
    shares = []
    for v, (seq, slp, _) in enumerate(per):
        ok = np.logical_and.accumulate(g['fixture|sample|margin|%d' % v] > MARGIN, axis=1)
        shares.append(ok.reshape(-1))
        assert seq.shape == g['fixture|sample|seq|%d' % v].shape
        assert np.array_equal(seq[ok], g['fixture|sample|seq|%d' % v][ok]) and U.relerr(slp[ok], g['fixture|sample|logp|%d' % v][ok]) < TOL
    assert np.concatenate(shares).mean() >= SHARE


@pytest.mark.parametrize('case', ['fixture', 'eos'])
def test_greedy_cases_are_resolvable_in_float64(case):
    """The condition on the inputs of tests/test_gpu_sat_batch.py's greedy cases, on the float64 margins of tests/sat_ref.sample."""
    opt, params, videos = B.make_case(case)
    per = B.sample(opt, params, videos, torch.float64)
    ok = np.concatenate([o.reshape(-1) for o in B.resolvable(per, MARGIN)])
    _, _, widths = B.stack_sample(per, videos)
    print('[%s] widths %s, resolvable %.3f of %d positions' % (case, widths.tolist(), ok.mean(), ok.size))
    assert widths.min() > 0 and ok.mean() >= SHARE
    if case == 'eos':
        assert len(set(widths.tolist())) > 1          # captions end at different steps across the videos


def test_case_shapes():
    """What the GPU tests' edge batches are there for."""
    _, _, v3 = B.make_case('edge3')
    assert [len(v['soi']) for v in v3] == [1, 3, 2] and [v['T_v'] for v in v3] == [9, 14, 11]
    lens = [v['soi'][:, 1] - v['soi'][:, 0] for v in v3]
    assert max(int(l.max()) for l in lens) == 7 and 1 in lens[1] and len({int(l.max()) for l in lens}) == 3
    assert [R.O.n_decoder_steps(v['labels']) for v in v3] == [6, 6, 3]
    _, _, v65 = B.make_case('tile65')
    eo = B.offsets(v65)
    assert eo[-1] == 65 and eo[-2] < 64 < eo[-1] and 0 < eo[1] < 64          # a video boundary inside the first tile, the tile boundary inside a video
    opt, params, _ = B.make_case('edge3', 'VEC', lda_dim=10)
    assert params['lm_model.core.rnn.weight_ih_l0'].shape[1] % 4 != 0          # the unaligned W_ih rows


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
BATCH_SYMBOLS = {'echr_sat_batch_ws_floats': (L.i64, [L.i32, L.i32, L.i32]),
                 'echr_sat_fwd_batch': (L.i32, [C.POINTER(L.SatArgs), C.POINTER(L.Dropout), C.POINTER(L.BatchExt), C.c_void_p]),
                 'echr_sat_bwd_batch': (L.i32, [C.POINTER(L.SatArgs), C.POINTER(L.SatGrads), C.POINTER(L.Dropout), C.POINTER(L.BatchExt), C.c_void_p]),
                 'echr_sat_sample_batch': (L.i32, [C.POINTER(L.SatSampleArgs), C.POINTER(L.BatchExt), C.c_void_p])}


def test_c_symbols_and_struct_layouts():
    lib = L.load()
    table = {n: (r, a) for n, r, a in L.SYMBOLS}
    header = open(L.os.path.join(L.os.path.dirname(L._HERE), 'include', 'echr_hip.h')).read()
    for name, (res, args) in BATCH_SYMBOLS.items():
        assert table[name] == (res, args), name
        assert getattr(lib, name).restype is res and name + '(' in header
    for cname, cls in (('echr_sat_args', L.SatArgs), ('echr_sat_grads', L.SatGrads), ('echr_sat_sample_args', L.SatSampleArgs),
                       ('echr_batch_ext', L.BatchExt)):
        assert lib.echr_abi_sizeof(cname.encode()) == C.sizeof(cls), cname
    assert 'n * H + u with n the BATCH-GLOBAL row' in header          # the dropout key of a batch is stated


def test_batch_workspace_size_is_positive_and_grows():
    lib = L.load()
    f = lib.echr_sat_batch_ws_floats
    assert f(3, 1, 32) >= (3 + 2) * 4 * 32 and f(64, 16, 512) >= (64 + 2 * 16) * 4 * 512
    assert f(65, 5, 32) > f(64, 5, 32) > 0 and f(64, 6, 32) > f(64, 5, 32) and f(64, 5, 64) > f(64, 5, 32)
    assert f(0, 1, 32) == -1 and f(3, 0, 32) == -1 and f(3, 1, 0) == -1


def _shape_args(feats=7):
    a = L.SatArgs()
    a.N, a.A, a.Tv, a.D, a.H, a.E, a.Ha, a.De, a.Dv, a.V1, a.S, a.feats = 6, 7, 30, 20, 32, 16, 24, 32, 12, 31, 6, feats
    return a


def test_entries_check_the_batch_extension_before_the_device():
    """NULL stream and buffers: every entry returns -EINVAL from its argument checks and names what is wrong; nothing reaches the device.
    (The one non-NULL pointer below is never read: the next check fails first.)"""
    lib = L.load()
    a, d, g = _shape_args(), L.Dropout(), L.SatGrads()
    sa = L.SatSampleArgs()
    sa.dec, sa.seq_len = a, 5
    calls = {'sat_fwd_batch': lambda x: lib.echr_sat_fwd_batch(C.byref(a), C.byref(d), x, None),
             'sat_bwd_batch': lambda x: lib.echr_sat_bwd_batch(C.byref(a), C.byref(g), C.byref(d), x, None),
             'sat_sample_batch': lambda x: lib.echr_sat_sample_batch(C.byref(sa), x, None)}
    fake = 64
    for who, call in calls.items():
        assert call(None) == -22 and who.encode() in lib.echr_last_error()
        x = L.BatchExt()
        for n in (0, -1, 7):          # fewer than one video, more videos than events
            x.n_videos = n
            assert call(C.byref(x)) == -22 and b'n_videos' in lib.echr_last_error() and who.encode() in lib.echr_last_error()
        x.n_videos = 2
        assert call(C.byref(x)) == -22 and b'vid' in lib.echr_last_error()
        x.vid = fake
        assert call(C.byref(x)) == -22 and b"'V' needs the batch's video" in lib.echr_last_error()


def test_vid_is_checked_on_the_host():
    assert sat.check_vid([0, 0, 1, 2], 3).dtype == np.int32
    for vid, V, word in (([0, 1, 0], 2, 'decreas'), ([0, 1], 0, 'n_videos'), ([0], 2, 'n_videos'), ([0, 2], 2, 'outside'), ([-1, 0], 1, 'outside')):
        with pytest.raises(ValueError) as e:
            sat.check_vid(np.asarray(vid), V)
        assert word in str(e.value), (vid, V)
    with pytest.raises(ValueError):
        sat.BatchVid([1, 0], 2, dev=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError):
        sat._sat_batch_ext(torch.zeros(2, dtype=torch.int32), None, 7, 2, 32)


# ---- the refusal matrix ---------------------------------------------------------------------------------------------------------------------
def _opt(**over):
    return synth.default_opt(vocab_size=30, seq_length=5, **over)


def _cpu_batch(opt, **kw):
    vids = [synth.make_video(2, 5, 6, 31, seed=900 + i, T_v=8, min_len=2, video_dim=opt.video_dim, hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
            for i in range(2)]
    return VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi', 'labels', 'masks')} for v in vids], **kw)


def test_refusal_matrix_of_the_batch_decoder():
    one = echr_amd.CaptionGenerator(_opt(caption_model=SAT, CG_num_layers=1, CG_input_feats_type='VEC'))
    three = echr_amd.CaptionGenerator(_opt())
    plain, built = _cpu_batch(one.opt), _cpu_batch(one.opt, caption_model=SAT)
    assert built.one_stream and built.caption_model == SAT and not plain.one_stream and plain.caption_model is None
    assert not _cpu_batch(one.opt, caption_model='three_stream').one_stream
    # a plain (or missing) batch with a one-stream model: NotImplementedError naming the keyword
    for b in (plain, None):
        for call in (lambda: one.forward_batch(b), lambda: one.forward_batch(b, mode='eval'), lambda: one._batch_contexts(b, None)):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert SAT in str(e.value) and 'caption_model' in str(e.value) and 'batch' in str(e.value)
    # a one-stream batch with a three-stream model
    for call in (lambda: three.forward_batch(built), lambda: three.forward_batch(built, mode='eval'), lambda: three.beam_batch(built, 2),
                 lambda: three.train_rl_batch(built)):
        three.eval()
        with pytest.raises(ValueError) as e:
            call()
        assert 'caption_model' in str(e.value) and SAT in str(e.value)
    # 'CH' rows: refused when the batch is built
    for ct in ('CH', 'CC+CH'):
        with pytest.raises(NotImplementedError) as e:
            _cpu_batch(one.opt, caption_model=SAT, clip_context_type=ct)
        assert SAT in str(e.value) and 'CH' in str(e.value) and 'clip_context_type' in str(e.value)
    with pytest.raises(ValueError) as e:
        _cpu_batch(one.opt, caption_model='two_stream')
    assert 'caption_model' in str(e.value)
    # the entries the one-stream decoder does not have keep refusing, a batch built for it included
    one.eval()
    for call, word in ((lambda: one.beam_batch(built, 2), 'beam'), (lambda: one.train_rl_batch(built), 'train_rl_batch'),
                       (lambda: one.forward_batch(built, mode='train_rl'), 'train_rl'), (lambda: one.forward_batch(built, beam_size=2), 'beam')):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert word in str(e.value)
    # a batch built for the decoder reaches the device check
    for mode in ('train', 'eval'):
        with pytest.raises(L.EchrHipError) as e:
            one.forward_batch(built, mode=mode)
        assert 'GPU' in str(e.value)
    # the batch still follows the model's other options
    init = echr_amd.CaptionGenerator(_opt(caption_model=SAT, CG_num_layers=1, CG_input_feats_type='VEC', CG_init_feats_type='VE'))
    with pytest.raises(NotImplementedError) as e:
        init.forward_batch(built)
    assert 'CG_init_feats_type' in str(e.value)


def test_the_fused_and_data_parallel_steps_keep_refusing():
    from echr_amd import fused
    from echr_amd.optim import ClampAdam

    class _Arena(object):
        pass
    m = echr_amd.CaptionGenerator(_opt(caption_model=SAT, CG_num_layers=1, CG_input_feats_type='VEC'))
    opt = ClampAdam.__new__(ClampAdam)
    opt.arena = _Arena()
    with pytest.raises(NotImplementedError) as e:
        fused.FusedTrainStep(m, opt)
    assert SAT in str(e.value)

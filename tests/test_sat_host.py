"""CPU: the one-stream decoder (caption_model='show_attend_tell', one LSTM layer) -- tests/sat_ref.py against the fixtures the reference
itself produced (tools/make_golden_sat.py -> tests/golden/case_sat_tiny.npz, case_sat.npz), the liveness matrix of the module (what
constructs and runs, what constructs and is refused by name), its state dict, and the C ABI of csrc/sat.hip (host functions only).

Float32-against-float64 gap of tests/sat_ref.py (measured by test_sat_ref_float32_gap on 'sat_vec_init': the largest of log-probs, loss,
every gradient and d tap_feats, each relative to its tensor's max-norm): 9.7e-7 in eval mode, 9.0e-7 in training mode; the test holds it
below 2e-5."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import echr_amd
from echr_amd import _lib as L
from echr_amd import synth
from echr_amd.sat import feats_bits
from oracle import summary as SM
from tests import sat_ref as R
from tests import util as U

TOL = 1e-5          # sat_ref in float32 against the reference's float32 run (relative)
VARIANTS = ('sat_c', 'sat_e', 'sat_ve', 'sat_vec_init', 'sat_vec_eh')
ATT = ('ctx2att', 'h2att', 'alpha_net')


def _case(name, g, prefix):
    return synth.make_sat_case(name, video_seed=int(g[prefix + 'seed']))


def _close(a, b, tol=TOL):
    return U.relerr(a, b, U.GRAD_FLOOR) < tol


def test_sat_ref_reproduces_the_tiny_fixture():
    g = U.gold('case_sat_tiny.npz')
    opt, params, vid = _case('sat_tiny', g, '')
    for mode in ('eval', 'train'):
        pred, loss, grads, g_tap = R.run(opt, params, vid, mode == 'train')
        assert U.relerr(pred, g[mode + '|logp']) < TOL and abs(loss - float(g[mode + '|loss'])) < TOL * abs(loss)
        assert np.abs(np.exp(pred.astype(np.float64)).sum(2) - 1).max() < 1e-5
        assert _close(g_tap, g[mode + '|gtap'])
        want = {k[len(mode + '|grad|'):] for k in g if k.startswith(mode + '|grad|')}
        assert want == {k for k, v in grads.items() if v is not None}
        for k in want:
            if k in R.NOISE_ONLY:
                assert float(np.abs(grads[k]).max()) < 1e-6 and float(np.abs(g[mode + '|grad|' + k]).max()) < 1e-6
            else:
                assert _close(grads[k], g[mode + '|grad|' + k]), k
    seq, slp = R.sample(opt, params, vid)
    ok = g['sample|margin'] > 1e-4
    assert ok.mean() >= 0.9 and np.array_equal(seq.numpy()[ok], g['sample|seq'][ok])
    assert U.relerr(slp.numpy()[ok], g['sample|logp'][ok]) < TOL


@pytest.mark.parametrize('name', VARIANTS)
def test_sat_ref_reproduces_the_summaries(name):
    g = U.gold('case_sat.npz')
    pre = name + '|'
    opt, params, vid = _case(name, g, pre)
    for mode in ('eval', 'train'):
        pred, loss, grads, g_tap = R.run(opt, params, vid, mode == 'train')
        key = pre + mode
        assert abs(loss - float(g[key + '|loss'])) < TOL * abs(loss)
        s = SM.summarize_logp(pred)
        assert U.relerr(s['slice'], g[key + '|logp|slice']) < TOL and np.array_equal(s['argmax'], g[key + '|logp|argmax'])
        dead = [k for k in grads if any(a in k for a in ATT)]
        if 'C' not in opt.CG_input_feats_type:
            assert dead and all(grads[k] is None for k in dead)
        grads = dict(grads, tap=g_tap)
        for k, v in SM.summarize_grads(grads).items():
            ref = g[key + ('|gtap|' + k.split('|', 1)[1] if k.startswith('tap|') else '|grad|' + k)]
            if k.split('|')[0] in R.NOISE_ONLY:
                assert float(np.abs(v).max()) < 1e-6 and float(np.abs(ref).max()) < 1e-6
                continue
            scale = max(float(g[key + ('|gtap|linf' if k.startswith('tap|') else '|grad|' + k.split('|')[0] + '|linf')]), U.GRAD_FLOOR)
            if k.endswith('|l2'):
                assert abs(v - ref) <= TOL * max(float(ref), U.GRAD_FLOOR), k
            else:
                assert float(np.abs(np.asarray(v, np.float64) - ref).max()) <= TOL * scale, k
    seq, slp = R.sample(opt, params, vid)
    ok = g[pre + 'sample|margin'] > 1e-4
    assert ok.mean() >= 0.9 and np.array_equal(seq.numpy()[ok], g[pre + 'sample|seq'][ok])
    assert U.relerr(slp.numpy()[ok], g[pre + 'sample|logp'][ok]) < TOL


def test_sat_ref_float32_gap():
    """What float32 costs the reference arithmetic itself (the floor of every GPU comparison against it)."""
    opt, params, vid = synth.make_sat_case('sat_vec_init')
    worst = 0.0
    for mode in (False, True):
        p32, l32, g32, t32 = R.run(opt, params, vid, mode)
        p64, l64, g64, t64 = R.run(opt, params, vid, mode, dtype=torch.float64)
        gap = max([U.relerr(p32, p64), abs(l32 - l64) / abs(l64), U.relerr(t32, t64, U.GRAD_FLOOR)] +
                  [U.relerr(g32[k], g64[k], U.GRAD_FLOOR) for k in g64 if g64[k] is not None and k not in R.NOISE_ONLY])
        print('float32 vs float64, train=%s: %.2e' % (mode, gap))
        worst = max(worst, gap)
    assert worst < 2e-5


# ---- the liveness matrix --------------------------------------------------------------------------------------------------------------
def _opt(**over):
    return synth.default_opt(vocab_size=30, seq_length=5, caption_model='show_attend_tell', **dict(dict(CG_num_layers=1, CG_input_feats_type='VEC'), **over))


def _call(m, mode='train', **kw):
    """forward() on CPU tensors of a 2-event video."""
    T = 6
    return m(torch.zeros(T, m.opt.hidden_dim), torch.zeros(T, m.opt.video_dim), torch.zeros(m.opt.lda_dim), torch.zeros(2, 4, dtype=torch.long),
             [1, 4], [[0, 2], [2, 5]], mode=mode, **kw)


LIVE = [dict(), dict(CG_input_feats_type='C'), dict(CG_input_feats_type='E'), dict(CG_input_feats_type='VE'), dict(CG_input_feats_type='V'),
        dict(CG_init_feats_type='VEC'), dict(CG_init_feats_type='C'), dict(video_context_type='VC'), dict(video_context_type='VLVCVH'),
        dict(event_context_type='ER1'), dict(event_context_type='ER2'), dict(event_context_type='EC'), dict(event_context_type='EH')]


@pytest.mark.parametrize('over', LIVE, ids=lambda o: ','.join('%s=%s' % kv for kv in o.items()) or 'default')
def test_live_options_reach_the_device_check(over):
    """A live configuration gets as far as the GPU-only message on CPU tensors (before this decoder ran, the container raised
    NotImplementedError here)."""
    m = echr_amd.CaptionGenerator(_opt(**over))
    for mode in ('train', 'eval'):
        with pytest.raises(L.EchrHipError) as e:
            _call(m, mode)
        assert 'GPU' in str(e.value)
    lm = m.lm_model
    with pytest.raises(L.EchrHipError):          # the module's own entries too: the first device pointer taken from a CPU tensor
        lm(torch.zeros(m.opt.video_context_dim), torch.zeros(2, m.opt.event_context_dim), torch.zeros(2, 3, m.opt.clip_context_dim), torch.ones(2, 3),
           torch.zeros(2, 4, dtype=torch.long))
    h, c = echr_amd.CaptionGenerator(_opt(**dict(over, CG_init_feats_type=''))).lm_model.init_hidden(None, torch.zeros(2, m.opt.event_context_dim), None)
    assert tuple(h.shape) == tuple(c.shape) == (1, 2, m.opt.CG_rnn_size) and float(h.abs().max()) == 0.0


REFUSED_CONFIG = [(dict(CG_num_layers=3), 'CG_num_layers'), (dict(CG_num_layers=2), 'CG_num_layers'), (dict(CG_rnn_type='gru'), 'CG_rnn_type'),
                  (dict(CG_rnn_type='rnn'), 'CG_rnn_type'), (dict(CG_att_hid_size=0), 'CG_att_hid_size'),
                  (dict(CG_input_feats_type=''), 'CG_input_feats_type'), (dict(clip_context_type='CH'), 'CH'), (dict(clip_context_type='CC+CH'), 'CH')]


@pytest.mark.parametrize('over,word', REFUSED_CONFIG, ids=[w + str(i) for i, (_, w) in enumerate(REFUSED_CONFIG)])
def test_refused_configurations_construct_and_say_so_at_call_time(over, word):
    m = echr_amd.CaptionGenerator(_opt(**over))          # never at construction
    m.load_state_dict(m.state_dict())
    for mode in ('train', 'eval'):
        with pytest.raises(NotImplementedError) as e:
            _call(m, mode)
        assert 'show_attend_tell' in str(e.value) and word in str(e.value)
    if 'clip_context_type' not in over:          # the module's own entries check before they touch an argument
        for fn in (m.lm_model.forward, m.lm_model.sample, m.lm_model.get_logprobs_state, m.lm_model.init_hidden):
            with pytest.raises(NotImplementedError) as e:
                fn()
            assert 'show_attend_tell' in str(e.value) and word in str(e.value)
    if 'CG_input_feats_type' in over:
        assert 'reference fails' in str(e.value)


def test_refused_calls_of_a_live_model():
    m = echr_amd.CaptionGenerator(_opt())
    lm = m.lm_model
    calls = [(lambda: _call(m, 'train_rl'), 'train_rl'), (lambda: _call(m, 'eval', beam_size=3), 'beam_size'),
             (lambda: lm.sample(None, None, None, None, {'beam_size': 2}), 'beam_size'), (lambda: lm.sample(None, None, None, None, {'sample_max': 0}), 'sample_max'),
             (lambda: lm.prepare(None, None, None, None), 'prepare'), (lambda: lm.sample_train(None, None, None, None, None), 'train_rl'),
             (lambda: lm.sequence_logprobs(None, None, None, None, None), 'train_rl'),
             (lambda: m.forward_batch(None), 'batch'), (lambda: m.beam_batch(None, 2), 'beam'), (lambda: m.train_rl_batch(None), 'train_rl_batch'),
             (lambda: m._batch_contexts(None, None), 'batch')]
    for call, word in calls:
        with pytest.raises(NotImplementedError) as e:
            call()
        assert 'show_attend_tell' in str(e.value) and word in str(e.value), word
    lm.train()
    lm.ss_prob = 0.25
    with pytest.raises(NotImplementedError) as e:
        _call(m, 'train')
    assert 'show_attend_tell' in str(e.value) and 'ss_prob' in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        lm(None, None, torch.zeros(2, 3, m.opt.clip_context_dim), torch.ones(2, 3), torch.zeros(2, 4, dtype=torch.long))
    assert 'ss_prob' in str(e.value)


def test_fused_steps_refuse_the_one_stream_decoder():
    from echr_amd import fused
    from echr_amd.optim import ClampAdam

    class _Arena(object):
        pass
    m = echr_amd.CaptionGenerator(_opt())
    opt = ClampAdam.__new__(ClampAdam)
    opt.arena = _Arena()
    with pytest.raises(NotImplementedError) as e:
        fused.FusedTrainStep(m, opt)
    assert 'show_attend_tell' in str(e.value) and 'FusedTrainStep' in str(e.value)


def test_three_stream_behaviour_is_unchanged():
    m = echr_amd.CaptionGenerator(synth.default_opt(vocab_size=30, seq_length=5))
    assert not m.one_stream() and tuple(m.lm_model.logit.weight.shape) == (31, 3 * 512)
    assert len(m.lm_model.native_params()) == 21
    st = m.lm_model.next_drop_state()
    assert (st.p_h, st.p_out) == (0.5, 0.5)


# ---- state dict -----------------------------------------------------------------------------------------------------------------------
def test_state_dict_names_and_shapes():
    opt = _opt()
    m = echr_amd.CaptionGenerator(opt)
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    H, E = opt.CG_rnn_size, opt.CG_input_encoding_size
    assert sd == {k: tuple(v) for k, v in synth.sat_state_dict_shapes(opt).items()}
    assert sd['lm_model.core.rnn.weight_ih_l0'] == (4 * H, E + opt.lda_dim + opt.d_o + opt.video_dim)
    assert sd['lm_model.core.rnn.weight_hh_l0'] == (4 * H, H) and sd['lm_model.logit.weight'] == (31, H)
    assert not any('bias' in k for k in sd if '.core.rnn.' in k)
    assert tuple(echr_amd.CaptionGenerator(_opt(CG_init_feats_type='VE')).state_dict()['lm_model.init_linear.weight'].shape) == (H, opt.lda_dim + opt.d_o)
    assert len(m.lm_model.native_params()) == 11 and feats_bits('VEC') == 7 and feats_bits('CE') == 6 and feats_bits('') == 0


def test_state_dict_loads_into_the_reference_shaped_dict():
    g = U.gold('case_sat_tiny.npz')
    ref = {k[len('state_dict|'):]: tuple(int(x) for x in v) for k, v in g.items() if k.startswith('state_dict|')}
    opt, params, _ = _case('sat_tiny', g, '')
    m = echr_amd.CaptionGenerator(copy.copy(opt))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == ref
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    shaped = {k: torch.zeros(s) for k, s in ref.items()}
    torch.nn.Module.load_state_dict(echr_amd.CaptionGenerator(copy.copy(opt)), shaped, strict=True)
    assert all(np.array_equal(m.state_dict()[k].numpy(), params[k]) for k in params)


def test_existing_cases_keep_their_parameter_draws():
    """synth's additions are additive: the encoder cases' names and draws did not move."""
    opt, params, _ = synth.make_case('tiny')
    assert set(params) == set(synth.state_dict_shapes(opt)) and len(params) == 37
    p2 = synth.make_sat_params(synth.make_sat_case('sat_tiny')[0])
    assert 'lm_model.core.rnn.weight_ih_l0' in p2 and 'lm_model.core.layer0.weight_ih' not in p2


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
SAT_SYMBOLS = {'echr_sat_ws_floats': (L.i64, [C.POINTER(L.SatArgs)]), 'echr_sat_ws_bwd_floats': (L.i64, [C.POINTER(L.SatArgs)]),
               'echr_sat_fwd': (L.i32, [C.POINTER(L.SatArgs), C.POINTER(L.Dropout), C.c_void_p]),
               'echr_sat_bwd': (L.i32, [C.POINTER(L.SatArgs), C.POINTER(L.SatGrads), C.POINTER(L.Dropout), C.c_void_p]),
               'echr_sat_step': (L.i32, [C.POINTER(L.SatArgs), L.c_f, L.c_f, L.c_f, L.c_f, C.POINTER(L.Dropout), C.c_void_p]),
               'echr_sat_sampler_ws_floats': (L.i64, [C.POINTER(L.SatArgs)]),
               'echr_sat_sample': (L.i32, [C.POINTER(L.SatSampleArgs), C.c_void_p])}


def test_c_symbols_and_struct_layouts():
    lib = L.load()
    table = {n: (r, a) for n, r, a in L.SYMBOLS}
    for name, (res, args) in SAT_SYMBOLS.items():
        assert table[name] == (res, args), name
        assert getattr(lib, name).restype is res
    header = open(L.os.path.join(L.os.path.dirname(L._HERE), 'include', 'echr_hip.h')).read()
    for name in SAT_SYMBOLS:
        assert name + '(' in header, name
    for cname, cls in (('echr_sat_args', L.SatArgs), ('echr_sat_grads', L.SatGrads), ('echr_sat_sample_args', L.SatSampleArgs)):
        assert lib.echr_abi_sizeof(cname.encode()) == C.sizeof(cls), cname
    assert lib.echr_version() == 3


def _shape_args(N, A, Tv, D, H, E, Ha, De, Dv, V1, S, feats):
    a = L.SatArgs()
    a.N, a.A, a.Tv, a.D, a.H, a.E, a.Ha, a.De, a.Dv, a.V1, a.S, a.feats = N, A, Tv, D, H, E, Ha, De, Dv, V1, S, feats
    return a


def test_workspace_sizes_are_positive_and_grow_with_the_steps():
    lib = L.load()
    tiny = dict(N=3, A=7, Tv=15, D=20, H=32, E=16, Ha=24, De=32, Dv=12, V1=31, feats=7)
    echr = dict(N=64, A=128, Tv=8192, D=500, H=512, E=512, Ha=512, De=512, Dv=100, V1=5001, feats=7)
    for shp in (tiny, echr):
        sizes = []
        for S in (1, 6):
            a = _shape_args(S=S, **shp)
            f, b, s = lib.echr_sat_ws_floats(C.byref(a)), lib.echr_sat_ws_bwd_floats(C.byref(a)), lib.echr_sat_sampler_ws_floats(C.byref(a))
            assert f > 0 and b > 0 and s >= shp['N'] * shp['V1']
            sizes.append((f, b))
        assert sizes[1][0] > sizes[0][0] and sizes[1][1] > sizes[0][1]
        # what every step keeps: gates, two states, the dropped output, q, scores, weights, the attended rows
        per_step = shp['N'] * (4 * shp['H'] + 3 * shp['H'] + shp['Ha'] + 2 * shp['A'] + shp['D'] + shp['E'])
        assert sizes[1][0] >= 6 * per_step
    assert lib.echr_sat_ws_floats(None) == -1 and lib.echr_sat_ws_bwd_floats(None) == -1 and lib.echr_sat_sampler_ws_floats(None) == -1


def test_entries_check_their_arguments_before_the_device():
    """NULL stream, NULL buffers: the argument checks return -EINVAL and name what is missing; nothing reaches the device."""
    lib = L.load()
    a = _shape_args(3, 7, 15, 20, 32, 16, 24, 32, 12, 31, 6, 0)
    d = L.Dropout()
    assert lib.echr_sat_fwd(C.byref(a), C.byref(d), None) == -22
    assert b'feats' in lib.echr_last_error() and b'reference fails' in lib.echr_last_error()
    a.feats = 7
    a.H = 30
    assert lib.echr_sat_fwd(C.byref(a), C.byref(d), None) == -22 and b'H%4' in lib.echr_last_error()
    a.H = 32
    assert lib.echr_sat_fwd(C.byref(a), C.byref(d), None) == -22          # 'V' without a video pointer
    assert lib.echr_sat_sample(None, None) == -22

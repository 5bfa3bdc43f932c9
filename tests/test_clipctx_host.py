"""Frame-level contexts 'CH' / 'CC+CH' on the host: construction, widths and state_dict against the reference's list (tests/golden/case_ch.npz,
case_cch.npz from tools/make_golden_clipctx.py), the cases that raise, the CPU oracle (tests/clipctx_ref.py) against the reference's
fixtures, and the new library entry points / structs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from echr_amd import synth
from oracle import summary as SM
from tests import clipctx_ref as R
from tests import util as U

CASES = [('case_ch.npz', 'ch'), ('case_cch.npz', 'cch')]


def _model(opt):
    import echr_amd
    return echr_amd.CaptionGenerator(opt)


@pytest.mark.parametrize('fixture,case', CASES)
def test_widths_and_state_dict_match_reference(fixture, case):
    g = U.gold(fixture)
    opt, params, _ = synth.make_case(case)
    m = _model(opt)
    want = {'ch': opt.hidden_dim, 'cch': opt.video_dim + opt.hidden_dim}[case]
    assert opt.clip_context_dim == want
    assert m.lm_model.core.attention.ctx2att.weight.shape[1] == want
    assert m.lm_model.core.layer1.weight_ih.shape[1] == opt.CG_input_encoding_size + want
    sd = m.state_dict()
    keys = [str(k) for k in g['state_dict|keys']]
    assert list(sd.keys()) == keys
    for k, shp in zip(keys, g['state_dict|shapes']):
        assert tuple(sd[k].shape) == tuple(int(x) for x in shp if x >= 0), k
    assert {k: tuple(v.shape) for k, v in params.items()} == {k: tuple(v.shape) for k, v in sd.items()}


def test_clip_context_spellings():
    opt, _, _ = synth.make_case('cch')
    assert _model(opt).clip_parts() == 3
    opt.clip_context_type = 'CCCH'          # the reference tests with `in`
    m = _model(opt)
    assert m.clip_parts() == 3 and opt.clip_context_dim == opt.video_dim + opt.hidden_dim
    opt, _, _ = synth.make_case('ch')
    assert _model(opt).clip_parts() == 2


def test_unsupported_clip_contexts_raise():
    opt, _, _ = synth.make_case('ch', )
    opt.CG_init_feats_type = 'C'
    with pytest.raises(NotImplementedError):
        _model(opt)
    opt, _, _ = synth.make_case('cch')
    opt.CG_init_feats_type = 'VC'
    with pytest.raises(NotImplementedError):
        _model(opt)
    opt, _, _ = synth.make_case('ch')
    opt.clip_context_type = 'CX'
    with pytest.raises(NotImplementedError):
        _model(opt)


@pytest.mark.parametrize('fixture,case', CASES)
@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_oracle_reproduces_reference(fixture, case, mode):
    g = U.gold(fixture)
    opt, params, vid = synth.make_case(case)
    logp, loss, grads, g_tap = R.run(opt, params, vid, mode == 'train')
    assert abs(loss - float(g[mode + '|loss'])) < 1e-5 * abs(float(g[mode + '|loss']))
    for k, v in SM.summarize_logp(logp).items():
        assert np.abs(np.asarray(v, np.float64) - g[mode + '|logp|' + k]).max() <= 2e-5 * max(1.0, np.abs(g[mode + '|logp|' + k]).max()), k
    for k, v in SM.summarize_grads(grads).items():
        ref = g[mode + '|grad|' + k]
        scale = max(float(np.abs(g[mode + '|grad|' + k.rsplit('|', 1)[0] + '|linf']).max()), 1e-5)
        assert np.abs(np.asarray(v, np.float64) - ref).max() <= 1e-4 * scale * (np.sqrt(np.asarray(ref).size) if k.endswith('|l2') else 1), k
    if mode == 'train':
        ref = g['train|g_tap']
        assert g_tap.shape == ref.shape == (vid['T_v'], opt.hidden_dim)
        assert U.relerr(g_tap, ref) < 1e-4
    else:
        assert abs(float(np.sqrt((g_tap.astype(np.float64) ** 2).sum())) - float(g['eval|g_tap|l2'])) < 1e-4 * float(g['eval|g_tap|l2'])


@pytest.mark.parametrize('fixture,case', CASES)
def test_oracle_greedy_matches_reference(fixture, case):
    g = U.gold(fixture)
    opt, params, vid = synth.make_case(case)
    seq, logp = R.sample(opt, params, vid)
    assert np.array_equal(seq.numpy(), g['sample|seq'])
    assert np.abs(logp.numpy() - g['sample|logp']).max() < 1e-4


def test_row_gradient_entry_points_are_bound():
    from echr_amd import _lib as L
    lib = L.load()
    names = {n for n, _, _ in L.SYMBOLS}
    for n in ('echr_decoder_row_grad', 'echr_decoder_row_grad_ws_floats', 'echr_clip_rows', 'echr_train_step_clip', 'echr_train_step_clip_ws_floats'):
        assert n in names and hasattr(lib, n), n
    for cname, cls in (('echr_row_grad_args', L.RowGradArgs), ('echr_clip_step_args', L.ClipStepArgs)):
        assert L.ABI_STRUCTS[cname] is cls
        assert lib.echr_abi_sizeof(cname.encode()) == C.sizeof(cls), cname
    assert lib.echr_version() == L.ABI_VERSION == 3
    # the workspace query: d att rows [S*N, ncols] + the live-row flags, each padded to 64 floats
    a = L.DecArgs()
    a.N, a.S, a.A = 12, 8, 40
    assert lib.echr_decoder_row_grad_ws_floats(C.byref(a), 512) == 96 * 512 + 128
    assert lib.echr_decoder_row_grad_ws_floats(C.byref(a), 0) == -1

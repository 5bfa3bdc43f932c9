"""CPU: the event contexts without the event encoder, 'EC' and 'EH' (CaptionGenerator.py:106-137) -- the module's constructor and state
dict, the oracle composition (tests/plain_event_ref.py) against the fixtures the reference itself produced (tools/make_golden.py ->
tests/golden/case_ec.npz / case_eh.npz), the argument contract of echr_train_step_args.event_direct on the six one-call entries (NULL
stream: nothing reaches the device), and the arena / optimiser / hand-over ranges of a model without fusion_model parameters."""
import ctypes as C

import numpy as np
import pytest
import torch

import echr_amd
from echr_amd import _lib as L
from echr_amd import synth
from oracle import summary as SM
from tests import plain_event_ref as R
from tests import test_step_contract_host as SC
from tests import util as U

WIDTH = {'ec': ('EC', 500), 'eh': ('EH', 512)}


@pytest.mark.parametrize('case', ['ec', 'eh'])
def test_module_constructs_without_a_fusion_model(case):
    opt, params, _ = synth.make_case(case)
    et, width = WIDTH[case]
    assert opt.event_context_type == et
    m = echr_amd.CaptionGenerator(opt)
    assert not hasattr(m, 'fusion_model') and m.event_direct() == {'EC': 1, 'EH': 2}[et]
    assert opt.event_context_dim == width
    sd = m.state_dict()
    shapes = synth.state_dict_shapes(opt)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v) for k, v in shapes.items()}
    assert all(k.startswith('lm_model.') for k in sd)
    assert shapes['lm_model.core.layer0.weight_ih'] == (4 * opt.CG_rnn_size, opt.CG_input_encoding_size + width)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    assert all(np.array_equal(m.state_dict()[k].numpy(), params[k]) for k in params)
    m2 = echr_amd.CaptionGenerator(synth.make_case(case)[0])
    m2.load_state_dict(m.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))


def test_init_linear_takes_the_direct_event_width():
    for et, width in WIDTH.values():
        opt = synth.default_opt(event_context_type=et, CG_init_feats_type='VE', vocab_size=30, seq_length=5)
        m = echr_amd.CaptionGenerator(opt)
        assert tuple(m.lm_model.init_linear.weight.shape) == (3 * opt.CG_rnn_size, opt.lda_dim + width)
        assert synth.state_dict_shapes(opt)['lm_model.init_linear.weight'] == (3 * opt.CG_rnn_size, opt.lda_dim + width)


def test_existing_cases_keep_their_parameter_draws():
    """The name sets of the encoder cases did not change, so the sorted-name draw order (synth.make_params) did not move: 'er1' against the
    reference-made fixture is covered by tests/test_oracle_golden.py; here the names."""
    opt = synth.default_opt()
    names = set(synth.state_dict_shapes(opt))
    assert sum(k.startswith('fusion_model.') for k in names) == 14 and len(names) == 37


@pytest.mark.parametrize('et', ['ECEH', 'EC+EH', '', 'EX'])
def test_other_event_contexts_are_refused(et):
    with pytest.raises(NotImplementedError) as e:
        echr_amd.CaptionGenerator(synth.default_opt(event_context_type=et))
    assert 'CaptionGenerator.py:132' in str(e.value) and 'torch.cat' in str(e.value)


@pytest.mark.parametrize('case', ['ec', 'eh'])
def test_oracle_composition_reproduces_the_reference(case):
    """The limits tests/test_oracle_golden.py applies to case_er1 (test_config_summaries, test_greedy_sample)."""
    opt, params, vid = synth.make_case(case)
    g = U.gold('case_%s.npz' % case)
    for mode in ('eval', 'train'):
        pred, loss, grads, g_tap, ev = R.run(opt, params, vid, mode == 'train')
        assert abs(loss - float(g[mode + '|loss'])) < 1e-5
        s = SM.summarize_logp(pred)
        assert np.abs(s['slice'] - g[mode + '|logp|slice']).max() < 1e-5
        assert np.array_equal(s['argmax'], g[mode + '|logp|argmax'])
        assert sorted(k for k, v in grads.items() if v is None) == ['lm_model.core.fusion_layer.bias', 'lm_model.core.fusion_layer.weight']
        for key, v in SM.summarize_grads(grads).items():
            ref = g[mode + '|grad|' + key]
            assert np.allclose(v, ref, rtol=1e-4, atol=1e-7 * (1 + np.abs(ref).max())), key
        # 'VL' + 'CC': tap_feats is reached through the anchors only ('EH'), or not at all ('EC')
        rows = np.flatnonzero(np.abs(g_tap).max(1) > 0)
        assert (len(rows) == 0) if case == 'ec' else set(rows) <= set(int(i) for i in vid['ind'])
    assert np.abs(ev - g['event_context']).max() < 1e-6 and ev.shape == (len(vid['soi']), WIDTH[case][1])
    seq, lp = R.sample(opt, params, vid)
    assert np.array_equal(seq.numpy(), g['sample|seq'])
    assert np.abs(lp.numpy() - g['sample|logp']).max() < 1e-5


# ---- echr_train_step_args.event_direct: the argument contract of the six entries --------------------------------------------------------
def _direct_call(entry, direct, **kw):
    """tests/test_step_contract_host.Call with a direct event context: tsrm / tsrm_g zeroed, dec.De the width the value names."""
    c = SC.Call(entry, **kw)
    a = c.a
    a.tsrm, a.tsrm_g, a.event_parts = L.TsrmArgs(), L.TsrmGrads(), 0
    a.event_direct = direct
    a.dec.De = SC.SHAPES[0][6] if direct == 1 else a.Ht          # Dc / Ht
    return c


@pytest.mark.parametrize('entry', SC.ENTRIES)
def test_direct_arguments_are_accepted_up_to_the_optimiser_state(entry):
    lib = L.load()
    for direct in (1, 2):
        rc, msg = _direct_call(entry, direct).run(lib)
        assert rc == -22 and msg == 'train_step: optimiser state missing', (entry, direct, rc, msg)
    # the same argument sets through the encoder are refused for their zeroed encoder description: the field is what is read
    c = _direct_call(entry, 1)
    c.a.event_direct = 0
    rc, msg = c.run(lib)
    assert rc == -22 and 'shapes disagree' in msg, (entry, rc, msg)


@pytest.mark.parametrize('entry', SC.ENTRIES)
def test_direct_refusals(entry):
    lib = L.load()
    c = _direct_call(entry, 1)
    c.a.event_direct = 3
    rc, msg = c.run(lib)
    assert rc == -22 and msg.startswith('train_step: event_direct = 3'), (entry, rc, msg)
    for direct in (1, 2):
        c = _direct_call(entry, direct)
        c.a.dec.De += 1
        rc, msg = c.run(lib)
        assert rc == -22 and msg.startswith('train_step: event_direct = %d: dec.De = %d is not the width' % (direct, c.a.dec.De)), (entry, rc, msg)
    c = _direct_call(entry, 2)
    c.a.tap = None
    rc, msg = c.run(lib)
    assert rc == -22, (entry, rc, msg)
    if 'clip' in entry:          # (the clip entries' own rule on their row source reports first)
        assert 'c3d / tap missing' in msg, (entry, msg)
    elif entry == '_batch_tap':          # (its own rule: g_tap needs tap)
        assert 'g_tap / tap missing' in msg, (entry, msg)
    else:
        assert msg.startswith("train_step: event_direct = 2 ('EH')") and 'tap' in msg, (entry, msg)
    # 'EC' reads no tap row
    c = _direct_call('', 1)
    c.a.tap = None
    rc, msg = c.run(lib)
    assert rc == -22 and msg == 'train_step: optimiser state missing', (rc, msg)
    # prepared = 1 is refused with a direct context (include/echr_hip.h), by the entry that takes it otherwise and by the prepare half
    c = _direct_call('', 1)
    c.a.prepared = 1
    rc, msg = c.run(lib)
    assert rc == -22 and 'event_direct = 1' in msg and 'prepared must be 0' in msg, (rc, msg)
    rc = lib.echr_train_step_prepare(C.byref(c.a), None)
    assert rc == -22 and 'event_direct' in (lib.echr_last_error() or b'').decode()


@pytest.mark.parametrize('shape', SC.SHAPES)
def test_direct_workspace_is_strictly_smaller(shape):
    lib = L.load()
    for cp, wi, V in ((1, False, 1), (1, True, 3), (2, False, 3), (3, True, 1)):
        sizes = {}
        for direct in (0, 1):
            a, x, bx = SC._args(shape, cp, wi), SC._x(shape, cp), SC._bx(V)
            a.event_direct = direct
            ra, rx, rb = C.byref(a), C.byref(x), C.byref(bx)
            if cp == 1:
                sizes[direct] = [lib.echr_train_step_ws_floats(ra), lib.echr_train_step_rw_ws_floats(ra), lib.echr_train_step_batch_ws_floats(ra, rb),
                                 lib.echr_train_step_batch_tap_ws_floats(ra, rb)]
            else:
                sizes[direct] = [lib.echr_train_step_clip_ws_floats(ra, rx), lib.echr_train_step_batch_clip_ws_floats(ra, rx, rb)]
        assert all(0 < d < e for d, e in zip(sizes[1], sizes[0])), (shape, cp, wi, V, sizes)
        # what is gone is exactly the four encoder regions (64-float aligned): its input rows and their gradient, its two workspaces
        N, _, _, H, _, De, Dc = shape
        up = lambda n: (n + 63) // 64 * 64
        enc = 2 * up(N * (Dc + H)) + up(lib.echr_tsrm_ws_floats(N, Dc + H, De, De, 4)) + up(lib.echr_tsrm_ws_bwd_floats(N, Dc + H, De, De, 4))
        assert all(e - d == enc for d, e in zip(sizes[1], sizes[0])), (shape, sizes, enc)


def test_abi_carries_the_field_last():
    lib = L.load()
    assert lib.echr_abi_sizeof(b'echr_train_step_args') == C.sizeof(L.TrainStepArgs)
    assert L.TrainStepArgs._fields_[-1][0] == 'event_direct'
    assert L.TrainStepArgs.event_direct.offset > L.TrainStepArgs.mid_user.offset


def test_arena_optimiser_and_handover_ranges_without_fusion_parameters():
    """ParamArena / ClampAdam over an 'EC' model, and the ranges the data-parallel exchange hands to the collectives (the logit layer, the
    LSTM layers, then parallel.StagedExchange.reduce_rest's remainder): they partition the arena, and every parameter that receives a
    gradient lies in exactly one of them.  The never-used core.fusion_layer lies in the remainder and stays zero."""
    from echr_amd.arena import ParamArena
    from echr_amd.optim import ClampAdam
    from echr_amd.parallel import StagedExchange
    opt, params, _ = synth.make_case('ec')
    m = echr_amd.CaptionGenerator(opt)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    ar = m.build_arena()
    assert isinstance(ar, ParamArena) and ar.params_in_arena() and len(ar.params) == len(params)
    assert m.lm_model._echr_arena_ref is ar
    o = ClampAdam(m.parameters(), lr=1e-3, arena=ar)
    assert {id(p) for p in o.param_groups[0]['params']} == {id(p) for p in ar.params}
    assert all(np.array_equal(p.detach().numpy(), params[k]) for k, p in m.named_parameters())
    lm = m.lm_model
    lstm = [p for k in range(3) for p in getattr(lm.core, 'layer%d' % k).parameters()]
    ex = StagedExchange()
    ex._queue = lambda flat, lo, hi, early: ex.ranges.append(dict(lo=lo, hi=hi, early=early))          # (no process group: record only)
    for group in ([lm.logit.weight, lm.logit.bias], lstm):
        slots = sorted(ar.slot(p) for p in group)
        assert slots == list(range(slots[0], slots[-1] + 1))
        ex.reduce_early(ar.flat_g, *ar.span(slots))
    ex.reduce_rest(ar.flat_g)
    ranges = sorted((r['lo'], r['hi']) for r in ex.ranges)
    assert ranges[0][0] == 0 and ranges[-1][1] == ar.total and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    unused = {id(p) for p in lm.core.fusion_layer.parameters()}
    live = [p for p in ar.params if id(p) not in unused]
    assert len(live) == len(ar.params) - 2
    for p in ar.params:
        lo = ar.offsets[ar.slot(p)]
        inside = [r for r in ranges if r[0] <= lo and lo + p.numel() <= r[1]]
        assert len(inside) == 1, p.shape

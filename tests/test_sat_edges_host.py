"""The inputs of tests/test_gpu_sat_edges.py are where their names say -- measured on tests/sat_ref.py alone, on the CPU, never on the HIP path: every
edge shape has the tile property it is in the table for; the scaled variants reach the gate and state ranges they are named for on the float64 run;
the float64 greedy decodes are resolvable; and the float32 run's own error (e_ref) is what the GPU file's table says."""
import numpy as np
import pytest
import torch

from tests import sat_ref as R
from tests import sat_regime_ref as G
from tests import test_gpu_sat as T
from tests import test_gpu_sat_edges as E
from tests import util as U


# ---- 1. tile edges -----------------------------------------------------------------------------------------------------------------------------
def test_kernel_constants_are_the_ones_the_table_was_laid_out_for():
    """SKC and SUNITS as csrc/sat.hip declares them: a change there has to come with a new table (every `want` below would name another tile)."""
    assert G.kernel_constants() == (64, 16)


@pytest.mark.parametrize('name', list(G.EDGES))
def test_edge_case_has_the_tile_property_it_is_there_for(name):
    p = G.check_edge(name)
    opt, params, vid = G.edge_case(name)
    assert vid['labels'].shape == (p['N'], 7) and int(max(vid['soi'][:, 1] - vid['soi'][:, 0])) == 7 and opt.CG_vocab_size == 30
    assert p['S'] == (1 if name == 's1' else 6)
    if p['Dc'] == 0:
        assert 'C' not in opt.CG_input_feats_type and p['K'] == p['H']


def test_the_table_covers_what_the_existing_cases_left_out():
    P = {n: G.tile_props(*G.edge_case(n)) for n in G.EDGES}
    assert {4, 12} <= {p['H'] for p in P.values()}                                            # H below one unit tile
    assert any(p['h_rem'] and p['unit_blocks'] > 1 for p in P.values())                       # a partial unit block behind a full one
    assert any(p['K'] == 64 for p in P.values()) and any(p['k_chunks'] == 2 and p['live4'] == 1 for p in P.values())
    assert {1, 2, 3} <= {p['col_blocks'] for p in P.values()} and {1, 2, 3} <= {p['row_tiles'] for p in P.values()}
    assert any(p['Dc'] and 0 < p['split_datt'] and p['split_block'] >= 1 for p in P.values())  # d att and d h columns in a block that is not the first
    assert any(p['vec_ic'] == 0 and p['Dc'] and p['h_rem'] for p in P.values())
    assert any(p['S'] == 1 for p in P.values()) and any(p['init'] and p['h_rem'] for p in P.values())
    assert {p['boundary'] // 4 for p in P.values() if p['Dc']} == set(range(16))                # the att | h boundary at every float4 of a chunk


@pytest.mark.parametrize('name', E.MAIN)
def test_edge_case_float32_noise_and_greedy_margin(name):
    """The float32 run of the reference arithmetic against its float64 run on the edge shapes (train mode): a quarter of the imported gates and
    less, so the gates hold room for the device's summation order.  The float64 greedy decode: EVERY pick resolvable, margin above 3e-4, not empty."""
    opt, params, vid = G.edge_case(name)
    with G.one_thread():
        a = R.run(opt, params, vid, True, dtype=torch.float32)
    b = R.run(opt, params, vid, True, dtype=torch.float64)
    e = G.errors(dict(logp=a[0], loss=a[1], grads=a[2], gtap=a[3]), dict(logp=b[0], loss=b[1], grads=b[2], gtap=b[3]))
    e_logp = U.relerr(a[0], b[0])
    print('[%s] float32 vs float64: logp %.2e loss %.2e grad %.2e (%s)' % (name, e_logp, e[1], e[2][0], e[2][1]))
    assert 4 * e_logp < T.TOL_LOGP and 4 * e[1] < T.TOL_LOSS and 4 * e[2][0] < T.TOL_GRAD
    seq, lp, mar, live = G.greedy64_of(opt, params, vid)
    assert seq.shape[1] >= 3 and live.all() and float(mar.min()) > 3e-4, (seq.shape, live.mean(), mar.min())          # (the seeds were picked for it)


# ---- 2. trained-weight scales ------------------------------------------------------------------------------------------------------------------
def _gate(pre, j):
    H = pre.shape[-1] // 4
    return pre[..., j * H:(j + 1) * H]


@pytest.mark.parametrize('name', ['gates_sat_vec', 'gates_sat_c', 'gates_sat70', 'neg_far'])
def test_gates_sat_variants_saturate_the_gates(name):
    """At least 15 % of the pre-activations beyond +-8, the largest beyond 17 (there the float32 sigmoid is exactly 1).  Measured: gates_sat_vec
    22.7 % / 34.0, gates_sat_c 21.0 % / 31.9, gates_sat70 21.6 % / 33.5, neg_far 67.0 % / 157."""
    pre, c, h0 = G.probe(name)
    a = np.abs(pre)
    print(name, 'share beyond 8: %.3f, largest %.1f, max |c| %.1f' % ((a > 8).mean(), a.max(), np.abs(c).max()))
    assert float((a > 8).mean()) >= 0.15 and float(a.max()) > 17.0
    assert pre.shape[1] == (70 if name == 'gates_sat70' else 12) and pre.shape[0] == 8
    if name != 'gates_sat_c':
        assert float(np.abs(h0).max()) > 0.0          # a non-zero initial state
    else:
        assert G.case(name)[0].CG_input_feats_type == 'C' and not np.any(h0)
    assert np.float32(1) / (np.float32(1) + np.exp(np.float32(-17.5))) == np.float32(1)


def test_gates_sat70_has_two_row_tiles():
    opt, params, vid = G.case('gates_sat70')
    assert -(-len(vid['soi']) // G.ROWS) == 2


def test_neg_far_reaches_below_minus_90_in_every_sigmoid_gate():
    """i, f and o each hold a pre-activation below -90 (-130 / -120 / -139 measured): exp(90) overflows float32, so 1 / (1 + exp(-x)) goes through
    +inf and has to come out as exactly 0."""
    pre, _, _ = G.probe('neg_far')
    lows = [float(_gate(pre, j).min()) for j in (0, 1, 3)]
    assert all(x < -90.0 for x in lows), lows
    with np.errstate(over='ignore'):
        assert np.isinf(np.exp(np.float32(90.0))) and np.float32(1) / (np.float32(1) + np.exp(np.float32(90.0))) == 0


def test_state_far_starts_and_steps_from_a_large_state():
    pre, c, h0 = G.probe('state_far')
    assert float(np.abs(h0).max()) >= 9.0 and float(np.abs(c).max()) >= 9.0          # (12.0 by construction; max |c(0)| 9.1)
    assert np.float32(1) - np.tanh(np.float32(10.0)) ** 2 == 0                        # 1 - tanh^2 is 0 in float32 there
    it, (h, cc), logp, (h2, c2), _ = G.far_state()
    a = np.abs(cc.numpy())
    assert 0.2 <= float((a >= 9).mean()) <= 0.3 and float(a.max()) <= 20.0 and int((a == 0).sum()) >= 16
    assert tuple(h.shape) == tuple(cc.shape) == (1, 12, 512) and np.isfinite(logp).all()
    # h is the pass's own: |h| < 1 behind a step
    assert float(h.abs().max()) < 1.0


@pytest.mark.parametrize('name', list(G.REGIME))
def test_float64_greedy_decode_is_resolvable(name):
    """At least 90 % of the picks have a top-1 / top-2 margin above 1e-4, they and every earlier pick of their row (measured: 100 % but gates_sat70's
    97.6 %); the decode is not empty."""
    seq, lp, mar, live = G.greedy64(name)
    print(name, seq.shape, 'resolvable %.3f, smallest margin %.2e' % (live.mean(), mar.min()))
    assert seq.shape[1] >= 4 and float(live.mean()) >= 0.9


@pytest.mark.parametrize('name', list(G.REGIME))
def test_e_ref_is_what_the_table_says_and_the_gates_stay_inside_the_contract(name):
    assert set(E.E_REF) == set(G.REGIME)
    e = G.e_ref(name)
    print(name, 'e_ref: logp %.2e loss %.2e grad %.2e gate slice %.2e' % e)
    for stored, measured in zip(E.E_REF[name], e):
        assert measured / 2 <= stored <= measured * 2, (name, E.E_REF[name], e)
    g = E.gates(name)
    assert g[0] <= E.CONTRACT and g[1] <= E.CONTRACT and 4 * E.E_REF[name][0] <= E.CONTRACT
    assert g == (max(T.TOL_LOGP, 4 * E.E_REF[name][0]), max(T.TOL_LOSS, 4 * E.E_REF[name][1]), max(T.TOL_GRAD, 4 * E.E_REF[name][2]),
                 max(T.TOL_GRAD, 4 * E.E_REF[name][3]))


def test_far_step_e_ref_is_what_the_table_says():
    e = G.far_step_e_ref()
    print('far step e_ref: logp %.2e h %.2e c %.2e' % e)
    for stored, measured in zip(E.E_REF_STEP, e):
        assert measured / 2 <= stored <= measured * 2, (E.E_REF_STEP, e)
    assert E.step_gates()[0] <= E.CONTRACT

"""The conditions tests/test_gpu_decoder_widths.py rests on, measured on the CPU oracles alone (tests/width_ref.py), never on the HIP path:
the case table reaches every width dispatch and every chunk edge it names; the float32 oracle's own error (e_ref) leaves every gate inside
the 1e-4 contract and, as the table says, below the existing gates; a last float4 that contributes nothing moves the float64 oracle far past
those gates; and the slices the GPU file judges hold live values."""
import numpy as np
import pytest

from tests import util as U
from tests import width_ref as W


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- 1. coverage of the table -------------------------------------------------------------------------------------------------------------
def test_group_a_reaches_every_width_dispatch():
    """All 16 (R, RD) pairs of att_bwd (so all four R of att_score / att_post), every listed Ha and D, D on both sides of att_context's
    128-column chunk, and the widths at which every clamped address is 0."""
    cs = [W.CASES[k] for k in W.GROUP['A']]
    assert {W.dispatch(c) for c in cs} == {(r, rd) for r in range(1, 5) for rd in range(1, 5)}
    assert {c['Ha'] for c in cs} == set(W.HA_VALUES) and {c['D'] for c in cs} == set(W.D_VALUES)
    assert len(cs) <= 20
    for vals in (W.HA_VALUES, W.D_VALUES):
        assert all(4 <= v <= 1024 and v % 4 == 0 for v in vals)
        for edge in (256, 512, 768):          # both sides of every 256-wide chunk boundary
            assert any(v <= edge for v in vals) and any(edge < v <= edge + 8 for v in vals), edge
        assert min(vals) == 4 and max(vals) == 1024
    assert any(c['D'] < W.CTX_CHUNK for c in cs if c['D'] > 4) and any(W.CTX_CHUNK < c['D'] < 2 * W.CTX_CHUNK for c in cs)
    assert all(c['H'] == 32 and c['E'] == 16 and c['lens'] == W.LENS for c in cs)


def test_group_b_straddles_every_slot_chunk_in_both_layouts():
    """The planted lengths against the 4 * SLOTS chunk of att_score / att_bwd / dq_fold for all three slot counts, the 8-slot chunk of att_post
    and the 32-row step of att_context: a length below, on and above an edge of each; one layout shares rows, one does not."""
    cs = {k: W.CASES[k] for k in W.GROUP['B']}
    assert {(c['D'], c['Ha']) for c in cs.values()} == {(20, 24), (516, 260)}
    assert W.SLOTS == (2, 4, 8)
    lens = set(W.SLOT_LENS)
    for chunk in [4 * s for s in W.SLOTS] + [8, 32]:
        assert any(l % chunk == 0 for l in lens) and any(l % chunk == 1 for l in lens) and any(l % chunk == chunk - 1 for l in lens), chunk
        assert len({_cdiv(l, chunk) for l in lens}) >= 3, chunk          # one chunk, a few, many
    assert 1 in lens and max(lens) == 65
    for k, c in cs.items():
        opt, params, vid = W.case(k)
        got = sorted(int(e - s) for s, e in vid['soi'])
        assert got == sorted(W.SLOT_LENS), k          # every planted length is there
        assert W.rows_shared(vid) == (c['layout'] == 'shared'), k
        assert np.array_equal(vid['ind'], vid['soi'][:, 1] - 1)


def test_group_c_straddles_the_recurrence_tiles():
    """4H against the 64-wide Nout tile of rec_gemm_kernel (below one tile, partial last tiles, many tiles) and K = H against its 128-wide k
    slice (a last slice of 4)."""
    cs = [W.CASES[k] for k in W.GROUP['C']]
    assert {(c['H'], c['E']) for c in cs} == set(W.HE_VALUES) | set(W.HE_EXTRA)
    assert sorted(4 * h for h, _ in W.HE_VALUES) == [16, 144, 240, 528, 1040]
    assert sorted(4 * h for h, _ in W.HE_EXTRA) == [32, 48]          # K = 4H of the d XT products: one k tile of 32, two
    assert any(4 * c['H'] < W.REC_TILE for c in cs) and sum((4 * c['H']) % W.REC_TILE != 0 for c in cs) >= 4
    assert sorted(c['H'] % W.REC_KSLICE for c in cs if c['H'] > W.REC_KSLICE) == [4, 4]
    assert all(c['D'] == 20 and c['Ha'] == 24 for c in cs)


def test_group_d_reaches_every_padding_group_of_the_persistent_kernels():
    """H = Ha = 512 and the ten D values: the smallest, one group of 8 columns, a partial group (D % 8 == 4), both sides of the 16-group wave
    boundaries at 128 and 256, and no padding at all; the BIG cases have an event past 129 slots."""
    cs = {k: W.CASES[k] for k in W.GROUP['D']}
    assert all(c['H'] == W.PH and c['Ha'] == W.PH and 8 <= c['D'] <= W.PH and c['D'] % 4 == 0 for c in cs.values())
    assert {c['D'] for k, c in cs.items() if c['lens'] == W.LENS and c['E'] == 16} == set(W.PERSIST_D)
    ds = set(W.PERSIST_D)
    assert 8 in ds and 512 in ds and any(d % 8 == 4 for d in ds) and any(d % 8 == 0 for d in ds)
    for wave_edge in (128, 256):          # 16 groups of 8 columns per wave
        assert wave_edge in ds and wave_edge + 4 in ds, wave_edge
    assert 124 in ds and 508 in ds          # a partial last group just below a wave boundary
    assert {(d >> 3) >> 4 for d in (x - 1 for x in ds)} == {0, 1, 2, 3}          # the last column's wave
    assert cs['d_d512_e512']['E'] == 512 and cs['d_d512_e512']['D'] == 512
    for k in W.PERSIST_BIG:
        assert cs[k]['lens'] == W.BIG_LENS and max(cs[k]['lens']) == 130 and cs[k]['D'] in (12, 512)
    assert len(W.BIG_LENS) == 3 and all(len(c['lens']) == 3 for c in cs.values())


def test_every_case_plants_its_lengths_and_keeps_the_small_shapes():
    for k, c in W.CASES.items():
        opt, params, vid = W.case(k)
        assert [int(e - s) for s, e in vid['soi']] == list(c['lens']), k
        assert vid['labels'].shape == (len(c['lens']), W.L) and opt.CG_vocab_size + 1 == W.V1
        assert (opt.d_feats, opt.d_o, opt.n_head, opt.hidden_dim, opt.lda_dim) == (32, 32, 4, 24, 12)
        assert (opt.video_dim, opt.CG_att_hid_size, opt.CG_rnn_size, opt.CG_input_encoding_size) == (c['D'], c['Ha'], c['H'], c['E'])
        assert vid['c3d'].shape == (vid['T_v'], c['D']) and 16 <= vid['T_v'] <= 186
    assert set(W.ONE_CALL) <= set(W.CASES) and [W.CASES[k]['group'] for k in W.ONE_CALL] == ['A', 'C', 'D']
    assert (W.CASES['a_ha772_d516']['D'], W.CASES['a_ha772_d516']['Ha']) == (516, 772) and W.CASES['d_d12']['D'] == 12
    assert {(W.CASES[k]['D'], W.CASES[k]['Ha']) for k in W.GROUP['F'] if W.is_sat(k)} == {(260, 252), (772, 516)}
    c = W.CASES['f_dec_d260_ha252']
    assert (c['D'], c['Ha'], c['H'], c['E']) == (260, 252, 36, 20)


# ---- 2. the float32 oracle's own error ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(W.CASES))
def test_e_ref_leaves_the_plain_gates_standing(name):
    """e_ref = float32 oracle against float64 oracle, train mode, per judged quantity (log-probs, loss, worst gradient tensor, worst width
    slice).  4 e_ref stays inside the 1e-4 contract, and -- what the table of tests/width_ref.py says -- below the existing gate of every
    quantity, so gates(name) are the plain gates.  The largest error of a float32 pass follows the host's summation order (BLAS kernels, thread
    count), so the re-measurement is held to the table loosely: within 4x of its entry, or below a quarter of the existing gate, where the
    plain gate stands whatever the entry says."""
    assert set(W.E_REF) == set(W.CASES)
    e = W.e_ref(name)
    e = (e[0], e[1], e[2], e[4])
    print(name, 'e_ref: logp %.2e loss %.2e grad %.2e slice %.2e' % e)
    assert 4 * e[0] <= W.CONTRACT and 4 * e[1] <= W.CONTRACT
    assert all(a <= max(4 * b, g / 4) for a, b, g in zip(e, W.E_REF[name], W.PLAIN)), (e, W.E_REF[name])
    assert all(4 * b <= g for b, g in zip(W.E_REF[name], W.PLAIN)), name          # the plain gate applies ...
    assert W.gates(name) == W.PLAIN                                               # ... and is what the GPU file uses


# ---- 3. the mutants -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['alpha', 'c3d'])
@pytest.mark.parametrize('name', W.MUTATED)
def test_a_dead_last_float4_moves_the_oracle_far_past_the_gates(name, which):
    """alpha_net.weight[:, -4:] = 0 (the last float4 of Ha contributes nothing) and c3d[:, -4:] = 0 (the last float4 of a clip row): the float64
    oracle's log-probs move by at least 10x their gate and its worst gradient tensor by at least 100x its gate at every case of A, B and D
    (smallest measured: 4.9e-4 on the log-probs of a_ha1020_d4, 0.29 of a tensor's max-norm at d_d512_big) -- a kernel that dropped that float4
    could not pass."""
    tl, _, tg, _ = W.gates(name)
    m = W.errors(W.mutant(name, which), W.oracle(name), W.case(name)[0])
    print(name, which, 'logp %.2e grad %.2e (%s)' % (m[0], m[2], m[3]))
    assert m[0] >= 10 * tl and m[2] >= 100 * tg, m


# ---- 4. the slices hold live values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [k for k in W.CASES if not W.is_sat(k)])
def test_last_float4_of_d_alpha_is_live(name):
    """The last float4 of d alpha_net.weight is at least 0.1 of the tensor's max-norm (0.21 .. 1.0 measured), so the slice measure judges values
    of the tensor's own size, not its rounding noise."""
    g = W.oracle(name)['grads']['lm_model.core.attention.alpha_net.weight']
    r = float(np.abs(g[:, -4:]).max() / np.abs(g).max())
    print(name, 'last float4 of d alpha / max-norm: %.2f' % r)
    assert r >= 0.1, r


def test_slices_are_the_last_float4_and_the_last_partial_chunk():
    """width_slices cuts what its labels say, on the axis that varies."""
    opt = W.case('a_ha516_d260')[0]
    g = W.oracle('a_ha516_d260')['grads']
    att = 'lm_model.core.attention.'
    s = dict(W.width_slices(att + 'ctx2att.weight', g[att + 'ctx2att.weight'], opt))
    assert [v.shape for v in s.values()] == [(4, 260), (4, 260), (516, 4), (516, 4)]          # Ha 516: chunk [512, 516); D 260: [256, 260)
    s = dict(W.width_slices(att + 'alpha_net.weight', g[att + 'alpha_net.weight'], opt))
    assert [v.shape for v in s.values()] == [(1, 4), (1, 4)]
    opt = W.case('a_ha508_d768')[0]
    g = W.oracle('a_ha508_d768')['grads']
    s = W.width_slices(att + 'h2att.bias', g[att + 'h2att.bias'], opt)
    assert [v.shape for _, v in s] == [(4,), (252,)]
    k = 'lm_model.core.layer1.weight_ih'
    s = W.width_slices(k, g[k], opt)
    assert [v.shape for _, v in s] == [(128, 4), (128, 256)] and np.array_equal(s[0][1], g[k][:, 16 + 764:16 + 768])
    assert not W.width_slices('lm_model.logit.weight', g['lm_model.logit.weight'], opt)
    sat = W.case('f_sat_d260_ha252')[0]
    assert W.context_col0(sat) == 16 + 12 + 32
    assert W.oracle('f_sat_d260_ha252')['grads']['lm_model.core.rnn.weight_ih_l0'].shape[1] == 16 + 12 + 32 + 260


def test_decoding_case_has_picks_outside_the_margin():
    """The float64 greedy decode of the decoding case: some pick is gated by the margin rule (exact comparison there)."""
    from tests import decoder_regime_ref as D
    seq, slp, margin, live = D.greedy64_of(*W.case('f_dec_d260_ha252'))
    assert seq.shape[1] >= 1 and int((margin[live] >= W.MARGIN).sum()) >= 1

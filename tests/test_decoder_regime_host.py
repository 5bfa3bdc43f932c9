"""The inputs of tests/test_gpu_decoder_regime.py (synth.make_decsat) are where their names say -- measured on the float64 oracle alone, on the
CPU, never on the HIP path: the gates saturate, the cell state drifts, the per-event bound on |C3D| spans 14 binades with the planted events in
place; the float32 oracle's own error (e_ref) is what the GPU file's table says and leaves its gates inside the 1e-4 contract; the float64 greedy
decode of every decoded variant has one right answer.  Thresholds: about two thirds of the measured figure, which stands beside each."""
import numpy as np
import pytest

from echr_amd import synth
from tests import decoder_regime_ref as D
from tests import test_gpu_decoder_regime as G


@pytest.mark.parametrize('name', ['gates_sat', 'gates_sat70', 'gates_sat_vb'])
def test_gates_sat_saturates_the_gates_of_every_stream(name):
    r = D.probe(name)
    # measured share of |pre| > 8 / max |pre| per stream: gates_sat 0.159 0.197 0.157 / 27.0 29.2 25.8; gates_sat70 0.156 0.198 0.155 / 27.3 35.9 30.9;
    # gates_sat_vb 0.160 0.218 0.155 / 26.5 32.3 26.2
    for k, share_min in enumerate((0.10, 0.12, 0.10)):
        pre = np.abs(r['pre'][k])
        assert float((pre > 8).mean()) >= share_min, (k, float((pre > 8).mean()))
        assert float(pre.max()) >= 17.0, (k, float(pre.max()))          # 17: beyond it the float32 sigmoid is exactly 1
    assert np.float32(1) / (np.float32(1) + np.exp(np.float32(-17.5))) == np.float32(1)


def test_drift_walks_the_cell_state_far_past_one():
    r = D.probe('drift')
    assert r['c'][0].shape[0] == 20          # 20 steps
    # measured max |c| 18.95 19.49 18.83, share of |c| > 9: 0.049 0.079 0.050 for streams 0, 1, 2
    for k, share_min in enumerate((0.033, 0.052, 0.033)):
        c = np.abs(r['c'][k])
        assert float(c.max()) >= 12.5, (k, float(c.max()))
        assert float((c > 9).mean()) >= share_min, (k, float((c > 9).mean()))
    assert np.float32(1) - np.tanh(np.float32(10.0)) ** 2 == 0          # 1 - tanh^2 is 0 in float32 there


def _lens(vid):
    return (vid['soi'][:, 1] - vid['soi'][:, 0]).tolist()


def _is_pow2(x):
    m, _ = np.frexp(x)
    return m == 0.5


def test_feat_wide_spreads_the_context_bound_and_carries_its_planted_events():
    opt, params, vid = D.case('feat_wide')
    c3d = vid['c3d']
    assert float(np.abs(c3d).max()) >= 143.0          # (215.7 measured; 3.9 in every other case of the suite)
    assert float(np.abs(D.probe('feat_wide')['pre'][1]).max()) >= 90.0          # stream 1 is fed the attended context (142 measured)
    # every event but the zero one: |context| < 2^8 (N(0, 1) rows give 2^2 or 2^3 everywhere), and its rows' own maxima span 9 or more binades below
    # that -- a bound taken from the wrong row is off by binades
    for n, (s, e) in enumerate(vid['soi'][1:], 1):
        rows = np.abs(c3d[s:e]).max(1)
        assert np.frexp(rows.max())[1] in (8, 9) and (n == 2 or np.frexp(rows.max())[1] - np.frexp(rows[rows > 0].min())[1] >= 9), (n, s, e)
    # event 0: every row zero -- a context bound of 0
    s, e = vid['soi'][0]
    assert e - s == 3 and not np.any(c3d[s:e]) and synth.decsat_event_max(vid, 0)[0] == 0.0
    # event 1: its largest |element| is exactly a power of two and exceeds every other element of the event
    s, e = vid['soi'][1]
    a = np.sort(np.abs(c3d[s:e]).reshape(-1))
    assert _is_pow2(a[-1]) and a[-1] > a[-2] and a[-1] < 2 * a[-2], (a[-1], a[-2])
    # event 2: ONE row, the one with the video's largest |element| before event 1 was planted -- its context is that row.  Under the factor of
    # the usual bound (|context| < 2^3) it overflows fp16 at every step, under its own bound it stays below 2^12
    s, e = vid['soi'][2]
    ctx = np.abs(D.probe_context('feat_wide')[:, 2])
    assert e - s == 1 and float(np.abs(c3d[s]).max()) >= 143.0 and np.allclose(ctx.max(1), np.abs(c3d[s]).max())
    assert D.pair_scaled(ctx.max(1), 4.0).min() >= D.FP16_INF and D.pair_scaled(ctx.max(), np.abs(c3d[s]).max()) < 4096.0
    assert np.array_equal(vid['ind'], vid['soi'][:, 1] - 1)


def test_feat_wide_big_plants_each_maximum_where_the_second_slot_set_can_miss_it():
    opt, params, vid = D.case('feat_wide_big')
    lens = _lens(vid)
    assert tuple(lens[:4]) == synth.DECSAT_BIG_LENS == (130, 258, 100, 173) and max(lens) == 258 and min(lens) <= 129
    c3d, soi = vid['c3d'], vid['soi']
    top = float(synth.DECSAT_BIG_TOP)
    mx = [synth.decsat_event_max(vid, n) for n in range(4)]
    assert mx[0] == (top, 129)          # the 130-long event: slot 129, the first slot of the second set and its only one
    assert mx[1] == (top, 257)          # the 258-long event: its last slot
    assert mx[3] == (top, 129)          # the 173-long event: slot 129
    ctx = np.abs(D.probe_context('feat_wide_big'))
    for n in (0, 1, 3):
        # without that slot the event's bound is below 0.5 (0.26 .. 0.28 measured), while the near-uniform attention leaves |context| = 15.9 .. 31.5
        # in the planted column at every step: under the factor of a maximum that misses the slot the context overflows fp16 -- at EVERY step --, under
        # the right one it stays below 2^12
        s, e = soi[n]
        rest = float(np.abs(np.delete(c3d[s:e], mx[n][1], axis=0)).max())
        assert rest < 0.5, (n, rest)
        assert D.pair_scaled(ctx[:, n].max(1), rest).min() >= D.FP16_INF, (n, ctx[:, n].max(1), rest)
        assert D.pair_scaled(ctx[:, n].max(), top) < 4096.0
    # event 2 (100 rows: no second slot set): the row just past its end holds 16384, more than 60 times the event's own maximum; it belongs to none
    # of the four planted events (others may hold it)
    e2 = int(soi[2, 1])
    assert float(np.abs(c3d[e2]).max()) == 4 * top and mx[2][0] < 256.0 and all(not (soi[n, 0] <= e2 < soi[n, 1]) for n in range(4))
    assert np.array_equal(vid['ind'], vid['soi'][:, 1] - 1)


def test_the_recurrent_input_comes_within_a_sixteenth_of_the_activation_scales_range():
    """csrc/persist.hip converts h to an fp16 pair at the fixed scale 2^12 (|h| < 16 keeps hi finite).  In train mode h = go tanh(c) * 2 comes
    as close to 2 as float64 shows (1.99984 in gates_sat_vb, at a step whose h IS fed to the next one): 2^15 would already overflow there."""
    opt, params, vids = D.case('gates_sat_vb')
    fed = D.max_fed_h('gates_sat_vb')
    assert 65520.0 / 32768.0 <= fed <= 2.0, fed


def test_batch_variant_is_a_three_video_batch_of_at_most_16_events():
    opt, params, vids = D.case('gates_sat_vb')
    assert len(vids) == 3 and sum(len(v['soi']) for v in vids) <= 16 and len({v['labels'].shape[1] for v in vids}) >= 2
    assert synth.make_decsat('gates_sat70')[2]['soi'].shape[0] == 70


@pytest.mark.parametrize('name', D.DECODED)
def test_float64_greedy_decode_has_one_right_answer(name):
    """Top-1 / top-2 margin of the float64 oracle's own greedy decode (seq_length 19) above 1e-4 at every step of every unfinished row, no row
    exempt: gates_sat 8.3e-4, drift 1.2e-4, feat_wide 5.9e-4, feat_wide_big 4.5e-4, gates_sat70 1.6e-4 (the seeds: synth.DECSAT)."""
    seq, slp, margin, live = D.greedy64(name)
    assert D.case(name)[0].CG_seq_length == 19 and seq.shape[1] >= 15
    assert live[:, 0].all() and float(margin[live].min()) > D.MARGIN, float(margin[live].min())
    if name.startswith('gates_sat'):
        assert len(set((seq > 0).sum(1).tolist())) >= 2          # rows finish at different steps


@pytest.mark.parametrize('name', list(synth.DECSAT))
def test_e_ref_is_what_the_table_says_and_the_gates_stay_inside_the_contract(name):
    """The table of the GPU file: max(existing gate, 4 e_ref) <= 1e-4 for log-probs and loss of every variant.  e_ref is re-measured here, but held
    to the table loosely: the largest error of a float32 pass follows the host's summation order (BLAS kernels, thread count) -- on a second host
    the same construction gave up to 2.6x the table's entry (gates_sat gradients 2.3e-5 for 8.8e-6, log-probs 3.1e-5 for 1.9e-5) -- so the gates
    come from the table, the smaller of the two, and the re-measurement only has to stay within 4x of it."""
    assert set(G.E_REF) == set(synth.DECSAT)
    e = [max(D.e_ref(name, False)[i], D.e_ref(name, True)[i]) for i in (0, 1, 2, 4)]
    print(name, 'e_ref: logp %.2e loss %.2e grad %.2e gate slice %.2e' % tuple(e))
    assert all(a <= 4 * b for a, b in zip(e, G.E_REF[name])), (e, G.E_REF[name])
    g = G.gates(name)
    assert g[0] <= G.CONTRACT and g[1] <= G.CONTRACT
    assert g[1] == max(G.TOL_LOSS, 4 * G.E_REF[name][1]) and 4 * G.E_REF[name][1] <= G.CONTRACT
    if name == 'gates_sat70':
        # the float32 reference itself costs 3.1e-5 over 70 saturated events in train mode (4 e_ref = 1.3e-4): the gate is the contract, 3.2 e_ref
        assert G.CONTRACT / 4 < G.E_REF[name][0] <= G.CONTRACT / 3 and g[0] == G.CONTRACT
    else:
        assert 4 * G.E_REF[name][0] <= G.CONTRACT and g[0] == max(G.TOL_LOGP, 4 * G.E_REF[name][0])


def test_gate_slices_show_what_the_tensor_norm_hides_in_drift():
    """In drift the gate slices of one LSTM tensor differ in max-norm by more than a decade (forget +8 saturates f: g f (1 - f) is small), so an
    error confined to the small slice would pass the per-tensor gate; the per-slice measure of the float32 oracle is above its per-tensor one."""
    ref = D.oracle('drift', True)['grads']
    ratios = []
    for k, g in ref.items():
        if D.is_lstm(k) and 'weight' in k:
            n = [float(np.abs(s).max()) for _, s in D.gate_slices(k, g)]
            ratios.append(max(n) / min(n))
    assert max(ratios) >= 10.0, ratios
    e = D.e_ref('drift', True)
    assert e[4] >= e[2] or not D.is_lstm(e[3])


def test_drift_state_is_taken_where_the_cell_is_largest():
    t, it, (h, c), logp, _ = D.drift_state()
    assert t >= 10 and float(c.abs().max()) >= 12.5          # (step 19, 18.5 measured)
    e = D.drift_step_e_ref()
    assert all(a <= 4 * b for a, b in zip(e, G.E_REF_STEP)) and 4 * G.E_REF_STEP[0] <= G.CONTRACT, e

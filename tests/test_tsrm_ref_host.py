"""The reference side of the event-encoder route tests (tests/tsrm_ref.py) checked on its own, without a GPU: against the fixtures made
from the reference project, its batched form against its plain form, the numpy transcription of the device's sin / cos helper against
float64, the dropout thresholds, and -- on the float64 reference alone -- the conditions every case of tests/test_gpu_tsrm_routes.py states.

sincos_f64arg_np against np.sin / np.cos in float64 over 1e-1 .. 2e6 rad, both signs (400 002 arguments), measured: 8.3e-8 maximum error
(MEASURED_SINCOS_ERR), well inside the 1e-6 gate the direct embedding test holds the kernel to."""
import numpy as np
import pytest
import torch

from echr_amd import philox, synth
from oracle import echr_ref_cpu as O
from tests import tsrm_ref as R, util as U

MEASURED_SINCOS_ERR = 8.3e-8
POSEMB_GATE = 1e-6          # tests/test_gpu_tsrm_routes.py::test_position_embedding_alone


@pytest.mark.parametrize('case', ['tiny', 'c1'])
def test_run_float32_reproduces_the_reference_fixture(case):
    """run(dtype = float32) is the arithmetic the fixtures were made with: event_context of tests/golden/case_<case>.npz to 1e-6 relative."""
    opt, params, vid = synth.make_case(case)
    ech = torch.cat((O.event_pool(torch.from_numpy(vid['c3d']), vid['soi']), torch.from_numpy(vid['tap'])[torch.as_tensor(np.asarray(vid['ind']), dtype=torch.long)]), 1).numpy()
    out, _, _ = R.run(params, ech, vid['soi'], opt.n_head, 0, None, dtype=torch.float32)
    gold = U.gold('case_%s.npz' % case)['event_context']
    assert out.shape == gold.shape
    assert R.rel(out, gold) < 1e-6


def _inputs(counts, width='S', mode=0, seed=5):
    Df, Do, G = R.WIDTHS[width]
    N = sum(counts)
    params = R.make_params(R.DIN, Df, Do, G, seed)
    soi = np.concatenate([R.make_events(n, R.T_V, R.MAX_LEN, seed + v) for v, n in enumerate(counts)], 0)
    return params, R.make_ech(N, R.DIN, seed + 1), soi, np.repeat(np.arange(len(counts)), counts), R.drop_mask(N, G), G


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_one_video_batch_equals_the_plain_form_bitwise(dtype):
    params, ech, soi, vid, dm, G = _inputs((7,))
    a = R.run(params, ech, soi, G, 0, dm, None, dtype)
    b = R.run(params, ech, soi, G, 0, dm, vid, dtype)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in R.NAMES:
        assert np.array_equal(a[2][k], b[2][k]), k


def test_three_video_batch_rows_equal_each_videos_own_call():
    """Rows of video v (out and d ech) equal the single call on that video with the mask block [rows_v][:, :, rows_v] and w's rows."""
    counts = (4, 1, 6)
    params, ech, soi, vid, dm, G = _inputs(counts, mode=0)
    out, dech, grads = R.run(params, ech, soi, G, 0, dm, vid)
    N, Do = out.shape
    w = R.out_weight(N, Do).astype(np.float64)
    total = {k: 0.0 for k in R.NAMES}
    for v in range(len(counts)):
        rows = np.nonzero(vid == v)[0]
        P = {k: torch.from_numpy(params[k]).double().requires_grad_(True) for k in R.NAMES}
        x = torch.from_numpy(ech[rows]).double().requires_grad_(True)
        o = O.tsrm_forward(P, x, soi[rows], G, torch.from_numpy(dm[rows][:, :, rows]).double())
        (o * torch.from_numpy(w[rows])).sum().backward()
        assert np.array_equal(o.detach().numpy(), out[rows]), v
        assert np.array_equal(x.grad.numpy(), dech[rows]), v
        for k in R.NAMES:
            total[k] = total[k] + P[k].grad.numpy()
    for k in R.NAMES:          # parameter gradients: the sum over the videos (another order of the same float64 additions)
        assert R.rel(grads[k], total[k]) < 1e-13, k


def test_make_events_edges():
    for N in (1, 2, 5, 130):
        soi = R.make_events(N, R.T_V, R.MAX_LEN, 3 + N)
        ln = soi[:, 1] - soi[:, 0]
        assert soi.dtype == np.int64 and soi.shape == (N, 2) and ln.min() == 1 and ln.max() <= R.MAX_LEN and soi.min() >= 0 and soi[:, 1].max() <= R.T_V
        c2 = soi[:, 0] + soi[:, 1]
        if N > 1:
            assert c2[0] == c2[1] and ln[0] != ln[1]
            assert O.position_matrix(soi)[0, 1, 0] == 1e-3          # the floor of dc between two distinct events


def test_posemb_is_the_oracles_formula_with_the_documented_dl():
    """tsrm_ref.posemb differs from oracle.position_embedding(position_matrix) only through dl: numpy's float32 log against the correctly rounded
    one (at most an ulp or two of dl, times the largest frequency scale 100)."""
    soi = np.array([[0, 1], [8191, 8192], [100, 300], [199, 201], [5, 6], [7, 20], [8191, 8391], [3, 4], [50, 61]])
    for Df in (32, 48, 80, 512):
        a, b = R.posemb(soi, Df), O.position_embedding(O.position_matrix(soi), Df)
        F4 = Df // 4
        assert a.shape == b.shape == (9, 9, Df)
        assert np.array_equal(a[:, :, :2 * F4], b[:, :, :2 * F4])
        assert np.abs(a - b).max() <= 100.0 * np.log(200.0) * 2.0 ** -22


def test_sincos_transcription_against_float64():
    x = np.logspace(-1, np.log10(2e6), 200000)
    x = np.concatenate([x, -x, [0.0, 1.6e6]])
    s, c = R.sincos_f64arg_np(x)
    err = max(float(np.abs(s - np.sin(x)).max()), float(np.abs(c - np.cos(x)).max()))
    print('sincos_f64arg_np: max error %.3e over %d arguments' % (err, x.size))
    assert err < POSEMB_GATE
    assert err <= MEASURED_SINCOS_ERR * 1.0001          # the figure recorded above


@pytest.mark.parametrize('p, want', [(0.1, 429496736), (0.3, 1288490240), (0.5, 2147483648), (0.7, 3006477056)])
def test_drop_threshold_is_the_float32_probabilitys(p, want):
    """The device floors float32(p) * 2**32 (csrc/decoder.hip, drop_thresh(float)): float32(0.1) = 13421773 * 2**-27, float32(0.3) = 10066330 * 2**-25,
    float32(0.7) = 11744051 * 2**-24, so the thresholds are those integers times 32, 128 and 256."""
    assert philox.drop_threshold(p) == want
    assert philox.drop_threshold(np.float32(p)) == want
    assert want == int(np.floor(float(np.float32(p)) * 4294967296.0))
    assert philox.drop_threshold(1.0) == 0xFFFFFFFF


def test_float32_threshold_changes_no_mask_of_the_fixture_stream():
    """Only p = 0.3 (the encoder's site) has another threshold as a float32; an element changes when its word lies in [1288490188, 1288490240):
    52 / 2**32 per element.  No [N, 16, N] mask of the fixtures' dropout stream (util.SEED / OFFSET, step 0) up to N = 200 holds such a word."""
    lo, hi = int(np.floor(0.3 * 4294967296.0)), philox.drop_threshold(0.3)
    assert (lo, hi) == (1288490188, 1288490240)
    e = np.arange(200 * 16 * 200, dtype=np.uint64)
    words = np.stack(philox.philox4x32_10(e >> np.uint64(2), 0, philox.SITE_TSRM, U.OFFSET, U.SEED & 0xFFFFFFFF, (U.SEED >> 32) & 0xFFFFFFFF), axis=-1)
    sel = words[np.arange(e.size), (e & np.uint64(3)).astype(np.int64)].astype(np.int64)
    assert not np.any((sel >= lo) & (sel < hi))
    assert np.array_equal(sel >= hi, philox.keep_mask(e.size, 0.3, U.SEED, U.OFFSET, philox.SITE_TSRM, 0))


# ---- the conditions of the GPU cases, on the float64 reference alone -------------------------------------------------------------------
def _median_top(spec, scale=None):
    spec = dict(spec, qk_scale=spec['qk_scale'] if scale is None else scale)
    params, ech, soi, _, _ = R.case_inputs(spec)
    _, w = R.probe(params, ech, soi, R.WIDTHS[spec['width']][2], spec['mode'])
    assert np.allclose(w.sum(2), 1.0, atol=1e-12)
    return float(np.median(w.max(axis=2)))


PEAKED = [n for n, s in R.CASES.items() if s['peaked'] and s['train']]          # (eval and train share their inputs)


@pytest.mark.parametrize('name', PEAKED)
def test_peaked_cases_are_peaked_at_the_smallest_qualifying_scale(name):
    """Median over (row, head) of the largest softmax weight >= 0.9, and the scale is the first of PEAK_SCALES that achieves it."""
    spec = R.CASES[name]
    assert spec['qk_scale'] in R.PEAK_SCALES
    med = _median_top(spec)
    print('%s: qk_scale %g, median top weight %.3f' % (name, spec['qk_scale'], med))
    assert med >= R.PEAK_MEDIAN
    below = [s for s in R.PEAK_SCALES if s < spec['qk_scale']]
    if below:
        assert _median_top(spec, below[-1]) < R.PEAK_MEDIAN
    assert R.CASES[name.replace('-train', '-eval')]['qk_scale'] == spec['qk_scale']


def test_unscaled_cases_are_near_uniform():
    """What the peaked cases add: the same shapes at qk_scale = 1 have a median top weight close to 1 / N."""
    for name in ('route-S-33', 'route-S-130'):
        assert _median_top(R.CASES[name]) < 3.0 / R.CASES[name]['N']


@pytest.mark.parametrize('name', [n for n, s in R.CASES.items() if s['mode'] == 2])
def test_fst2_cases_keep_their_gates_out_of_the_amplifying_band(name):
    spec = R.CASES[name]
    params, ech, soi, vid, _ = R.case_inputs(spec)
    vid = np.zeros(len(soi), np.int64) if vid is None else vid
    G = R.WIDTHS[spec['width']][2]
    clamped = live = 0
    for v in np.unique(vid):
        rows = np.nonzero(vid == v)[0]
        gate, _ = R.probe(params, ech[rows], soi[rows], G, 2)
        assert not np.any((gate > R.FST2_BAND[0]) & (gate < R.FST2_BAND[1])), (name, v)
        clamped += int((gate <= R.FST2_BAND[0]).sum())
        live += int((gate >= R.FST2_BAND[1]).sum())
    assert clamped > 0 and live > 0          # both sides of clamp(min = 1e-6) occur


@pytest.mark.parametrize('name', [n for n, s in R.CASES.items() if s['inference']])
def test_table_cases_meet_the_table_rule(name):
    """pair_table_rows (csrc/tsrm.hip): N^2 >= 16384 and 2 ((max_span + 1)(max_len + 1) + (max_len + 1)^2) <= N^2."""
    spec = R.CASES[name]
    soi = R.case_inputs(spec)[2]
    max_len, max_span = R.bounds(soi)
    N = spec['N']
    assert N * N >= 16384 and N * N % 16 == 4          # the last tile of 16 pairs holds 4
    assert 2 * ((max_span + 1) * (max_len + 1) + (max_len + 1) ** 2) <= N * N
    assert R.WIDTHS[spec['width']][0] in (256, 512) and R.WIDTHS[spec['width']][2] <= 16


def test_case_table_is_the_one_the_issue_lists():
    kinds = {}
    for n in R.CASES:
        kinds[n.split('-')[0]] = kinds.get(n.split('-')[0], 0) + 1
    assert kinds == {'route': 21, 'fst0': 3, 'fst1': 3, 'fst2': 3, 'fst3': 3, 'fst4': 3, 'peak': 14, 'batch': 6, 'tables': 2}
    for s in R.CASES.values():
        Df, Do, G = R.WIDTHS[s['width']]
        assert Df % G == 0 and Do % G == 0 and Df % 4 == 0

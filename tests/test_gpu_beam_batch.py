"""Beam search over a multi-video batch on the GPU (echr_decoder_beam_batch through CaptionGenerator.beam_batch and
eval_utils.caption_videos_beam) against the host beam search over the CPU oracle per video (tests/beam_ref.py, tests/beam_batch_ref.py)
and against the single-video calls on the GPU.

The gates are those of tests/test_gpu_beam.py: index outputs (seq, words, widths) are compared only for events whose ORACLE margin is
>= 1e-4 -- a condition on the inputs, measured with the CPU oracle alone and asserted as a minimum count -- log-probs within 1e-4, scores
within 1e-4 relative; sentence_confidence within 1e-3 and grouped against ungrouped log-probs within 2e-5 as in tests/test_gpu_eval_batch.py.
A video's width is compared when an event of the oracle's widest is gated."""
import numpy as np
import pytest
import torch

from echr_amd import functional as EF
from echr_amd.batch import VideoBatch
from tests import beam_batch_ref as R
from tests import beam_ref
from tests import util as U

pytestmark = pytest.mark.gpu

MARGIN = 1e-4
TOL_LOGP = 1e-4
TOL_SCORE = 1e-4       # relative
TOL_CONF = 1e-3
TOL_GROUPED = 2e-5
f2t = lambda s, e, n, d: [round(float(s) / n * d, 3), round(float(e) / n * d, 3)]


# ---- shared, read-only state ------------------------------------------------------------------------------------------------------
_MODELS, _BATCHES, _RUNS = {}, {}, {}


def model(eos_bias=0.0):
    if eos_bias not in _MODELS:
        opt, params = R.make_opt()
        _MODELS[eos_bias] = U.build_gpu_model(opt, R.biased(params, eos_bias), False)
    return _MODELS[eos_bias]


def to_dev(videos):
    dev = torch.device('cuda')
    return [dict(v, c3d=torch.from_numpy(v['c3d']).to(dev), lda=torch.from_numpy(v['lda']).to(dev), tap=torch.from_numpy(v['tap']).to(dev))
            for v in videos]


def batch_of(case):
    """The case's videos as one VideoBatch, every video with its own 'tap' (no tap_model)."""
    if case not in _BATCHES:
        _BATCHES[case] = VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi')} for v in to_dev(R.videos(case))])
    return _BATCHES[case]


def as_numpy(out, N):
    seq, lp, score, vw = out
    if len(seq) == 0:
        return np.zeros((N, 0), np.int64), np.zeros((N, 0), np.float32), score.cpu().numpy(), np.asarray(vw)
    return seq.cpu().numpy(), lp.cpu().numpy(), score.cpu().numpy(), np.asarray(vw)


def run(case, eos_bias, B, **kw):
    """beam_batch on the case (numpy results), computed once per argument set."""
    key = (case, eos_bias, B) + tuple(sorted(kw.items()))
    if key not in _RUNS:
        b = batch_of(case)
        _RUNS[key] = as_numpy(model(eos_bias).beam_batch(b, B, **kw), b.n_events)
    return _RUNS[key]


def fit(x, w):
    """x [N, T] zero-padded or cut to w columns."""
    out = np.zeros((x.shape[0], w), x.dtype)
    k = min(w, x.shape[1])
    out[:, :k] = x[:, :k]
    return out


def widest_gated(ref, g):
    return bool(g.any()) and int(ref['words'][g].max()) == int(ref['words'].max())


def check_against_oracle(case, eos_bias, B, out):
    seq, lp, score, vw = out
    b, refs = batch_of(case), R.oracle(case, eos_bias, B)
    gates = R.gated(case, eos_bias, B, MARGIN)
    n_gated = sum(int(g.sum()) for g in gates)
    print('gated %d of %d (minimum %d)' % (n_gated, b.n_events, R.MIN_GATED[(case, eos_bias, B)]))
    assert n_gated >= R.MIN_GATED[(case, eos_bias, B)]
    assert vw.shape == (b.n_videos,) and vw.dtype == np.int64 and seq.shape[1] == lp.shape[1] == int(vw.max()) and score.shape == (b.n_events,)
    for v, (s, ref, g) in enumerate(zip(b.event_slices, refs, gates)):
        w = int(vw[v])
        if widest_gated(ref, g):
            assert w == int(ref['words'][g].max()), (v, w, ref['words'].tolist())
        assert not seq[s, w:].any()                                    # a video's rows are zero from its own width on
        assert np.all(ref['words'][g] <= w)
        assert np.array_equal(seq[s, :w][g], fit(ref['seq'], w)[g]), v
        rs = ref['score'][g]
        err = np.abs(score[s][g] - rs) / np.maximum(np.abs(rs), 1.0)
        print('video %d: width %d, score rel err %.2e' % (v, w, err.max(initial=0.0)))
        assert np.all(err <= TOL_SCORE)
        for n in np.nonzero(g)[0]:
            m = min(int(ref['words'][n]) + 1, w, ref['logp'].shape[1])
            assert np.abs(lp[s][n, :m] - ref['logp'][n, :m]).max(initial=0.0) < TOL_LOGP
            assert not lp[s][n, m:w].any()


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eos_bias', [0.0, 0.25])
@pytest.mark.parametrize('B', [2, 3, 5])
def test_beam_batch_vs_oracle_few_rows(B, eos_bias):
    """27 events of 6 videos, at most 135 rows: the few-rows form of the chain.  With the <eos> bias videos 0, 1, 2 and 5 are empty and
    videos 3 and 4 mix a 9-word caption with empty ones."""
    out = run('small', eos_bias, B)
    check_against_oracle('small', eos_bias, B, out)
    if eos_bias:
        gates, refs = R.gated('small', eos_bias, B, MARGIN), R.oracle('small', eos_bias, B)
        empty = [v for v in range(6) if gates[v].all() and not refs[v]['words'].any()]
        assert len(empty) >= 3 and not out[3][empty].any() and out[3].max() == 9


@pytest.mark.parametrize('gemm_h2', [1, 0])
@pytest.mark.parametrize('B', [3, 5])
def test_beam_batch_vs_oracle_many_rows(B, gemm_h2):
    """65 events of 7 videos: 195 / 325 rows, across SAMP_SLAB_ROWS = 192 -- every product an h2 GEMM over the rows; with gemm_h2 = 0 the
    exact-fp32 form."""
    from echr_amd import _lib
    lib = _lib.load()
    try:
        lib.echr_config_set(b'gemm_h2', gemm_h2)
        b = batch_of('slab')
        out = as_numpy(model().beam_batch(b, B), b.n_events)
    finally:
        lib.echr_config_set(b'gemm_h2', 1)
    check_against_oracle('slab', 0.0, B, out)


# ---- 2. against the single-video call ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,eos_bias,B', [('small', 0.0, 2), ('small', 0.25, 3), ('small', 0.0, 5), ('slab', 0.0, 3)])
def test_beam_batch_vs_single_video_calls(case, eos_bias, B):
    seq, lp, score, vw = run(case, eos_bias, B)
    b, cg = batch_of(case), model(eos_bias)
    refs, gates = R.oracle(case, eos_bias, B), R.gated(case, eos_bias, B, MARGIN)
    assert sum(int(g.sum()) for g in gates) >= R.MIN_GATED[(case, eos_bias, B)]
    for v, (s, g) in enumerate(zip(b.event_slices, gates)):
        d, w = b.video(v), int(vw[v])
        with torch.no_grad():
            sv, lv, scv = cg(d['tap'], d['c3d'], d['lda'], [], d['ind'], d['soi'], mode='eval', beam_size=B, return_score=True)
        n = s.stop - s.start
        sv = sv.cpu().numpy() if len(sv) else np.zeros((n, 0), np.int64)
        lv = lv.cpu().numpy() if len(lv) else np.zeros((n, 0), np.float32)
        scv = scv.cpu().numpy()
        if widest_gated(refs[v], g):
            assert sv.shape[1] == w, (v, sv.shape, w)
        assert not seq[s, w:].any()
        assert np.array_equal(seq[s, :w][g], fit(sv, w)[g])
        assert np.abs(lp[s, :w][g] - fit(lv, w)[g]).max(initial=0.0) < TOL_LOGP
        assert np.all(np.abs(score[s][g] - scv[g]) <= TOL_SCORE * np.maximum(np.abs(scv[g]), 1.0))


# ---- 3. empty results --------------------------------------------------------------------------------------------------------------
def test_whole_batch_empty_returns_nothing():
    """<eos> dominant (logit bias + 40): every result is the empty caption -- T == 0, seq and logp are [], the scores are still there."""
    b = batch_of('small')
    seq, lp, score, vw = model(40.0).beam_batch(b, 3, max_rows=40)
    assert seq == [] and lp == [] and vw.tolist() == [0] * 6
    assert score.shape == (b.n_events,) and bool(torch.isfinite(score).all()) and float(score.max()) <= 0.0
    _MODELS.pop(40.0)


# ---- 4. max_rows -------------------------------------------------------------------------------------------------------------------
def test_max_rows_runs_equal_one_decode(monkeypatch):
    """B = 3 on the 27-event case: max_rows = 40 -> runs [0,2) | the 36-row video alone | [3,6); max_rows = 1 -> every video alone.  Against
    one decode over the batch: gated seq identical, log-probs within the project's gate for grouped against ungrouped evaluation."""
    b, cg = batch_of('small'), model()
    assert b.beam_groups(3, 40) == [(0, 2, 0, 7), (2, 3, 7, 19), (3, 6, 19, 27)]
    assert b.beam_groups(3, 1) == [(v, v + 1, s.start, s.stop) for v, s in enumerate(b.event_slices)]
    assert b.beam_groups(3, None) == [(0, 6, 0, 27)]
    calls = []
    real = EF.beam_search_batch

    def counted(video, event, *a, **k):
        calls.append((video.shape[0], event.shape[0]))
        return real(video, event, *a, **k)
    monkeypatch.setattr(EF, 'beam_search_batch', counted)
    g = np.concatenate(R.gated('small', 0.0, 3, MARGIN))
    assert int(g.sum()) >= R.MIN_GATED[('small', 0.0, 3)]
    seq0, lp0, sc0, vw0 = as_numpy(cg.beam_batch(b, 3, max_rows=None), b.n_events)
    assert calls == [(6, 27)]
    for max_rows, want in ((40, [(2, 7), (1, 12), (3, 8)]), (1, [(1, 3), (1, 4), (1, 12), (1, 3), (1, 4), (1, 1)])):
        del calls[:]
        seq1, lp1, sc1, vw1 = as_numpy(cg.beam_batch(b, 3, max_rows=max_rows), b.n_events)
        assert calls == want
        assert seq1.shape == seq0.shape and np.array_equal(seq1[g], seq0[g])
        assert np.abs(lp1[g] - lp0[g]).max() < TOL_GROUPED
        assert np.all(np.abs(sc1[g] - sc0[g]) <= TOL_SCORE * np.maximum(np.abs(sc0[g]), 1.0))
        refs, gates = R.oracle('small', 0.0, 3), R.gated('small', 0.0, 3, MARGIN)
        for v in range(6):
            if widest_gated(refs[v], gates[v]):
                assert vw1[v] == vw0[v]
    # with empty videos inside the runs (one run is empty as a whole)
    a = run('small', 0.25, 3)
    c = as_numpy(model(0.25).beam_batch(b, 3, max_rows=40), b.n_events)
    g = np.concatenate(R.gated('small', 0.25, 3, MARGIN))
    assert np.array_equal(a[3], c[3]) and np.array_equal(a[0][g], c[0][g]) and np.abs(a[1][g] - c[1][g]).max() < TOL_GROUPED


# ---- 5. reproducibility ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,B', [('small', 3), ('slab', 3)])
def test_decode_is_bitwise_reproducible(case, B):
    """Two identical decodes (functional.beam_search_batch on the same contexts, as tests/test_gpu_beam.py repeats functional.beam_search:
    the event encoder in front runs split-K sums that are not bitwise repeatable) agree bit for bit, video_words included."""
    b, cg = batch_of(case), model()
    with torch.no_grad():
        video, event, ev_start, ev_len, A, vid, _ = cg._batch_contexts(b, None)
        lm = cg.lm_model
        outs = [as_numpy(EF.beam_search_batch(video, event, b.c3d, ev_start, ev_len, vid, A, lm.seq_length, lm.native_params(), B), b.n_events)
                for _ in range(2)]
    for x, y in zip(*outs):
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # and the module call gives the same captions
    seq = run(case, 0.0, B)[0]
    g = np.concatenate(R.gated(case, 0.0, B, MARGIN))
    assert np.array_equal(fit(seq, 9)[g], fit(outs[0][0], 9)[g])


# ---- 6. beam_size = 1 --------------------------------------------------------------------------------------------------------------
def test_beam1_is_the_greedy_batch_decode():
    b, cg = batch_of('small'), model()
    g = np.concatenate(R.gated('small', 0.0, 1, MARGIN))
    assert int(g.sum()) >= R.MIN_GATED[('small', 0.0, 1)]
    seq, lp, score, vw = run('small', 0.0, 1)
    with torch.no_grad():
        gs, gl = cg.forward_batch(b, mode='eval')
    gs, gl = gs.cpu().numpy(), gl.cpu().numpy()
    L = cg.lm_model.seq_length
    # (the greedy decode zeroes a row behind its first <eos> already)
    assert np.array_equal(fit(seq, L)[g], fit(gs, L)[g])
    for n in np.nonzero(g)[0]:
        row = fit(gs, L)[n]
        k = min((int(np.argmax(row == 0)) if (row == 0).any() else L) + 1, seq.shape[1], gs.shape[1])
        assert np.abs(lp[n, :k] - gl[n, :k]).max(initial=0.0) < TOL_LOGP


# ---- 7. caption_videos_beam --------------------------------------------------------------------------------------------------------
def _tap_model(opt):
    from tests import test_gpu_eval_batch as TE
    return TE.make_tap(opt).cuda()


@pytest.mark.parametrize('eos_bias,min_gated', [(0.0, 20), (0.25, 22)])
def test_caption_videos_beam_given_events_vs_oracle(eos_bias, min_gated):
    """flag_eval_what='cg' on the 27-event videos at B = 3, the oracle fed the device's encoder states.  Gated events measured with the
    oracle's own encoder in front: 22 (bias 0) / 24 (0.25) of 27; the minimum leaves two for states that differ by the encoder's 2e-5.
    With the bias whole videos are empty: they return nothing while the batch decodes on."""
    from echr_amd import eval_utils as EU
    opt, params = R.make_opt()
    params = R.biased(params, eos_bias)
    cg, tap = model(eos_bias), _tap_model(opt)
    videos = R.videos('small')
    dv = [{k: v[k] for k in ('c3d', 'lda', 'duration', 'ind', 'soi', 'timestamps')} for v in to_dev(videos)]
    infos, ex = EU.caption_videos_beam(tap, cg, dv, f2t, 3, flag_eval_what='cg', max_rows=40)
    assert ex['kept'] == list(range(6)) and ex['selection'] is None and cg.training is False
    vw, ro, taps = ex['video_words'], ex['row_offset'], ex['tap_feats'].cpu().numpy()
    assert len(vw) == 6 and tuple(ex['score'].shape) == (27,)
    n_gated, n_empty = 0, 0
    for v, vid in enumerate(videos):
        ref = beam_ref.oracle_beam(opt, params, dict(vid, tap=taps[ro[v]:ro[v + 1]]), 3, vid['soi'], vid['ind'])
        g = ref['margin'] >= MARGIN
        n_gated += int(g.sum())
        pv = ex['per_video'][v]
        if g.all() and not ref['words'].any():
            n_empty += 1
            assert infos[v] == [] and pv['seq'] is None and pv['cg_prob'] is None and vw[v] == 0
            continue
        if widest_gated(ref, g):
            assert vw[v] == ref['words'].max()
        if vw[v] == 0:
            assert infos[v] == [] and pv['seq'] is None
            continue
        assert tuple(pv['seq'].shape) == (len(vid['ind']), vw[v]) == tuple(pv['cg_prob'].shape)
        assert len(infos[v]) == len(vid['ind'])
        for i in np.nonzero(g)[0]:
            rec = infos[v][i]
            assert rec['sentence'] == [int(t) for t in ref['seq'][i] if t > 0]
            assert rec['timestamp'] == vid['timestamps'][i] and rec['num'] == [i, len(vid['ind'])] and rec['proposal_score'] == 1.0
            assert abs(rec['sentence_confidence'] - ref['score'][i]) < TOL_CONF
            assert abs(rec['re_score'] - (10.0 + rec['sentence_confidence'])) < 1e-9
    print('gated %d of 27, empty videos %d' % (n_gated, n_empty))
    assert n_gated >= min_gated
    assert n_empty >= (2 if eos_bias else 0) and any(infos)          # (oracle: all four empty videos, videos 0 and 5 with every event gated)


def test_caption_videos_beam_nms_vs_caption_video():
    """One NMS run on the four videos of tests/test_gpu_eval_batch.py (24, 1, 9 and 40 rows; the one-row video has no candidate and is
    dropped from the batch) at B = 3 against caption_video(beam_size=3) per video on the GPU.  The oracle margin comes from the device's
    encoder states; measured with the oracle's own encoder in front every one of the 36 events is gated (smallest margin 1.3e-4)."""
    from echr_amd import eval_utils as EU
    from tests import test_gpu_eval_batch as TE
    opt, params = R.make_opt()
    cg, tap = model(), _tap_model(opt)
    videos = TE.make_inputs(opt)
    dv = TE.to_dev(videos)
    infos, ex = EU.caption_videos_beam(tap, cg, dv, f2t, 3, topN=TE.TOPN, nms_threshold=0.6)
    assert ex['kept'] == [0, 2, 3] and infos[1] == [] and ex['batch'].n_videos == 3 and len(ex['video_words']) == 3
    ro, taps = ex['row_offset'], ex['tap_feats'].cpu().numpy()
    n_gated = 0
    for v, vid in enumerate(dv):
        one, ex1 = EU.caption_video(tap, cg, vid['c3d'], vid['lda'], vid['duration'], f2t, topN=TE.TOPN, nms_threshold=0.6, beam_size=3)
        pv = ex['per_video'][v]
        assert [int(i) for i in pv['ind_select_list']] == [int(i) for i in ex1['ind_select_list']]
        assert np.array_equal(np.asarray(pv['soi_select_list']).reshape(-1, 2), np.asarray(ex1['soi_select_list']).reshape(-1, 2))
        if v == 1:
            assert one == [] and pv['seq'] is None
            continue
        soi, ind = np.asarray(pv['soi_select_list'], np.int64), np.asarray(pv['ind_select_list'], np.int64)
        ref = beam_ref.oracle_beam(opt, params, dict(tap=taps[ro[v]:ro[v + 1]], c3d=videos[v]['c3d'], lda=videos[v]['lda']), 3, soi, ind)
        g = ref['margin'] >= MARGIN
        n_gated += int(g.sum())
        assert len(infos[v]) == len(one) == len(ind)
        if widest_gated(ref, g):
            assert tuple(pv['seq'].shape) == tuple(ex1['seq'].shape)
        for i in np.nonzero(g)[0]:
            a, b = infos[v][i], one[i]
            assert a['sentence'] == b['sentence'] and a['timestamp'] == b['timestamp'] and a['num'] == b['num'] and set(a) == set(b)
            assert abs(a['proposal_score'] - b['proposal_score']) < 1e-6
            assert abs(a['sentence_confidence'] - b['sentence_confidence']) < TOL_CONF
            assert abs(a['re_score'] - (10 * a['proposal_score'] + a['sentence_confidence'])) < 1e-9
    print('gated %d of 36' % n_gated)
    assert n_gated >= 34

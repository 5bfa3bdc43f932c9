"""Beam search on the GPU (echr_decoder_beam through functional.beam_search / OldModel.sample opt beam_size) against the reference's
greedy captions (B = 1) and the host beam search over the CPU oracle (tests/beam_ref.py).

Index outputs are compared only for events whose oracle margin (the smallest gap between a kept and a dropped candidate, or between the
result and the runner-up finished hypothesis) is at least MARGIN: below it a float32 decode may legitimately choose differently.  Every
event's score must equal the oracle's re-score of the GPU's own hypothesis."""
import numpy as np
import pytest
import torch

from echr_amd import functional as EF, synth
from tests import beam_ref, util as U

pytestmark = pytest.mark.gpu

MARGIN = 1e-4          # ~2e-6 per step of log-prob noise (test_gpu_parity.TOL_LOGP's measurement) summed over 19 steps stays below
TOL_LOGP = 1e-4
TOL_SCORE = 1e-4       # relative


def _case(name):
    """(opt, params, vid, soi, ind, reference greedy seq, logp) of a fixture."""
    if name.startswith('eosmix_'):
        k = name[-1]
        opt, params, vid = synth.make_eosmix(k)
        g = U.gold('case_eosmix.npz')
        return opt, params, vid, g[k + '|soi'], g[k + '|ind'], g[k + '|seq'], g[k + '|logp']
    opt, params, vid = synth.make_case(name)
    g = U.gold('case_%s.npz' % name)
    return opt, params, vid, vid['soi'], vid['ind'], g['sample|seq'], g['sample|logp']


def _inputs(vid):
    dev = torch.device('cuda')
    return tuple(torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))


def _contexts(m, vid, soi, ind):
    """The decoder inputs CaptionGenerator.forward(mode='eval') hands to OldModel.sample (video, event, clip, clip_mask)."""
    got = {}

    def grab(video, event, clip, clip_mask, opt={}):
        got.update(video=video, event=event, clip=clip, clip_mask=clip_mask)
        return [], []
    m.lm_model.sample = grab
    try:
        with torch.no_grad():
            m(*_inputs(vid), [], ind, soi, mode='eval')
    finally:
        del m.lm_model.sample
    return got


def _beam(m, ctx, B):
    lm = m.lm_model
    cv = lm._clip_view(ctx['clip'], ctx['clip_mask'])
    with torch.no_grad():
        seq, lp, score = EF.beam_search(ctx['video'], ctx['event'], cv.feats, cv.ev_start, cv.ev_len, cv.max_len, lm.seq_length,
                                        lm.native_params(), B, h0=lm._initial_state(ctx['video'], ctx['event'], cv))
    n = ctx['event'].shape[0]
    if len(seq) == 0:
        return np.zeros((n, 0), np.int64), np.zeros((n, 0), np.float32), score.cpu().numpy()
    return seq.cpu().numpy(), lp.cpu().numpy(), score.cpu().numpy()


def _words(seq):
    T = seq.shape[1]
    return np.array([int(np.argmax(r == 0)) if (r == 0).any() else T for r in seq], np.int64)


def _pad(seq, L):
    out = np.zeros((seq.shape[0], L), np.int64)
    out[:, :seq.shape[1]] = seq
    return out


def _check_against_oracle(opt, params, vid, soi, ind, seq, lp, score, B, min_gated):
    L = opt.CG_seq_length
    ref = beam_ref.oracle_beam(opt, params, vid, B, soi, ind)
    gated = ref['margin'] >= MARGIN
    assert int(gated.sum()) >= min_gated, (int(gated.sum()), min_gated)
    assert np.array_equal(_pad(seq, L)[gated], _pad(ref['seq'], L)[gated])
    # the GPU's own hypotheses, re-scored by the oracle: every event
    resc, words = beam_ref.oracle_rescore(opt, params, vid, seq, soi, ind)
    assert np.all(np.abs(score - resc) <= TOL_SCORE * np.maximum(np.abs(resc), 1.0)), np.abs(score - resc).max()
    # log-probs: the gated events' against the oracle's, <eos> included where it is inside the output
    T = seq.shape[1]
    for n in np.nonzero(gated)[0]:
        m = min(int(words[n]) + 1, T)
        assert np.abs(lp[n, :m] - ref['logp'][n, :m]).max(initial=0.0) < TOL_LOGP
        assert not lp[n, m:].any()
    return ref


@pytest.mark.parametrize('case', ['tiny', 'c1', 'c3bench', 'init', 'initc', 'vctx', 'er1', 'eosmix_a', 'eosmix_b', 'eosmix_c'])
def test_beam1_is_reference_greedy(case):
    """B = 1 is the greedy decode up to each row's first <eos>: the reference's seq (and width T) bit for bit, its log-probs up to <eos>,
    zeros after (where the greedy decode keeps the raw arg-max log-probs), score = the sum of the log-probs."""
    opt, params, vid, soi, ind, rseq, rlp = _case(case)
    m = U.build_gpu_model(opt, params, False)
    seq, lp, score = _beam(m, _contexts(m, vid, soi, ind), 1)
    assert seq.shape == rseq.shape and np.array_equal(seq, rseq)
    T, L = seq.shape[1], opt.CG_seq_length
    w = _words(seq)
    for n in range(seq.shape[0]):
        k = min(int(w[n]) + 1, T)
        assert np.abs(lp[n, :k] - rlp[n, :k]).max(initial=0.0) < TOL_LOGP
        assert not lp[n, k:].any()
        if w[n] < T or w[n] == L:          # every term of the score is inside the output
            ref = float(rlp[n, :k].astype(np.float64).sum())
            assert abs(score[n] - ref) <= TOL_SCORE * max(abs(ref), 1.0), (n, score[n], ref)


# (case, B, minimum number of events the margin gates; measured on the CPU oracle: c1 2/2/1, init 10/12/11, eosmix_a 62/55/58,
# eosmix_b 136/138/128, c3bench@3 38)
ORACLE_CASES = [('c1', 2, 1), ('c1', 3, 1), ('c1', 5, 1), ('init', 2, 8), ('init', 3, 10), ('init', 5, 9),
                ('eosmix_a', 2, 55), ('eosmix_a', 3, 48), ('eosmix_a', 5, 50), ('eosmix_b', 2, 120), ('eosmix_b', 5, 110),
                ('c3bench', 3, 30)]


@pytest.mark.parametrize('case,B,min_gated', ORACLE_CASES)
def test_beam_vs_host_reference(case, B, min_gated):
    opt, params, vid, soi, ind, _, _ = _case(case)
    m = U.build_gpu_model(opt, params, False)
    seq, lp, score = _beam(m, _contexts(m, vid, soi, ind), B)
    _check_against_oracle(opt, params, vid, soi, ind, seq, lp, score, B, min_gated)


@pytest.mark.parametrize('gemm_h2', [1, 0])
def test_beam_both_chain_forms(gemm_h2):
    """eosmix b (150 events) at B = 3: 450 rows -- the many-rows h2 form of the chain; with gemm_h2 = 0 the exact-fp32 one."""
    from echr_amd import _lib
    lib = _lib.load()
    opt, params, vid, soi, ind, _, _ = _case('eosmix_b')
    m = U.build_gpu_model(opt, params, False)
    ctx = _contexts(m, vid, soi, ind)
    try:
        lib.echr_config_set(b'gemm_h2', gemm_h2)
        seq, lp, score = _beam(m, ctx, 3)
    finally:
        lib.echr_config_set(b'gemm_h2', 1)
    ref = _check_against_oracle(opt, params, vid, soi, ind, seq, lp, score, 3, 120)
    assert len(set(ref['words'].tolist())) >= 5                  # results of many lengths: slots finish at different steps


def test_beam_is_bitwise_reproducible():
    opt, params, vid, soi, ind, _, _ = _case('eosmix_a')
    m = U.build_gpu_model(opt, params, False)
    ctx = _contexts(m, vid, soi, ind)
    a, b = _beam(m, ctx, 3), _beam(m, ctx, 3)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_beam_eos_dominant_returns_empty():
    """A logit bias that makes <eos> dominant: every result is the empty caption, sample returns ([], []), the score is the <eos> log-prob
    of the first step."""
    opt, params, vid, soi, ind, _, _ = _case('vctx')
    params = dict(params)
    params['lm_model.logit.bias'] = params['lm_model.logit.bias'].copy()
    params['lm_model.logit.bias'][0] += np.float32(40.0)
    m = U.build_gpu_model(opt, params, False)
    ctx = _contexts(m, vid, soi, ind)
    seq, lp, score = _beam(m, ctx, 3)
    assert seq.shape[1] == 0
    with torch.no_grad():
        out = m(*_inputs(vid), [], ind, soi, mode='eval', beam_size=3)
    assert out == ([], [])
    P, video, event, clip, mask, state0 = beam_ref.oracle_contexts(opt, params, vid)
    from oracle import echr_ref_cpu as O
    with torch.no_grad():
        lp0, _ = O.logprobs_state(P, torch.zeros(event.shape[0], dtype=torch.long), video, event, clip, mask, state0)
    eos = lp0[:, 0].double().numpy()
    assert np.all(np.abs(score - eos) <= TOL_SCORE * np.maximum(np.abs(eos), 1.0)), np.abs(score - eos).max()


def test_beam_public_api():
    opt, params, vid, soi, ind, rseq, _ = _case('eosmix_a')
    m = U.build_gpu_model(opt, params, False)
    ctx = _contexts(m, vid, soi, ind)
    x = _inputs(vid)
    with torch.no_grad():
        s_cg, l_cg = m(*x, [], ind, soi, mode='eval', beam_size=3)
        s_lm, l_lm = m.lm_model.sample(ctx['video'], ctx['event'], ctx['clip'], ctx['clip_mask'], {'beam_size': 3})
        s3, l3, sc3 = m(*x, [], ind, soi, mode='eval', beam_size=3, return_score=True)
        g_def, gl_def = m(*x, [], ind, soi, mode='eval')
        g_b1, gl_b1 = m(*x, [], ind, soi, mode='eval', beam_size=1)
    # (the event encoder in front of the decoder runs again per call: its split-K sums are not bitwise repeatable, the captions are)
    assert torch.equal(s_cg, s_lm) and torch.equal(s_cg, s3)
    assert float((l_cg - l_lm).abs().max()) < 1e-5 and float((l_cg - l3).abs().max()) < 1e-5
    assert sc3.shape == (s3.shape[0],) and sc3.dtype == torch.float32
    # the default stays today's greedy decode
    assert np.array_equal(g_def.cpu().numpy(), rseq) and torch.equal(g_def, g_b1)
    assert float((gl_def - gl_b1).abs().max()) < 1e-5
    with pytest.raises(ValueError):
        m.lm_model.sample(ctx['video'], ctx['event'], ctx['clip'], ctx['clip_mask'], {'beam_size': 3, 'sample_max': 0})
    for bad in (0, 17):
        with pytest.raises(ValueError):
            m.lm_model.sample(ctx['video'], ctx['event'], ctx['clip'], ctx['clip_mask'], {'beam_size': bad})
    m.train()
    try:
        with pytest.raises(ValueError):
            m.lm_model.sample(ctx['video'], ctx['event'], ctx['clip'], ctx['clip_mask'], {'beam_size': 3})
    finally:
        m.eval()
    with pytest.raises(ValueError):
        m(*x, [], ind, soi, mode='train', beam_size=3)


def test_caption_video_with_beam():
    """eval_utils.caption_video(beam_size=3) end to end: the captions of the beam decode and sentence_confidence = its score."""
    from echr_amd import eval_utils as EU, models as EM
    opt, params, vid = synth.make_case('c1')
    opt.K = 8
    cg = U.build_gpu_model(opt, params, False)
    torch.manual_seed(3)
    tap = EM.setup_tap(opt).cuda()
    tap.eval()
    dev = torch.device('cuda')
    rs = np.random.RandomState(11)
    T = 24
    c3d = torch.from_numpy(rs.standard_normal((T, opt.video_dim)).astype(np.float32)).to(dev)
    lda = torch.from_numpy(rs.standard_normal(opt.video_context_dim).astype(np.float32)).to(dev)
    f2t = lambda s, e, n, d: [round(float(s) / n * d, 3), round(float(e) / n * d, 3)]
    info, ex = EU.caption_video(tap, cg, c3d, lda, 60.0, f2t, topN=12, beam_size=3)
    assert len(info) == len(ex["ind_select_list"]) >= 1
    with torch.no_grad():
        seq, lp, score = cg(ex['tap_feats'], c3d, lda, [], ex['ind_select_list'], ex['soi_select_list'], mode='eval', beam_size=3,
                            return_score=True)
    assert torch.equal(ex['seq'], seq)
    sc = score.cpu().numpy()
    for i, rec in enumerate(info):
        assert abs(rec['sentence_confidence'] - float(sc[i])) < 1e-5
        assert abs(rec['re_score'] - (10 * rec['proposal_score'] + float(sc[i]))) < 1e-4
        assert rec['sentence'] == [int(t) for t in seq[i].cpu().numpy() if t > 0]

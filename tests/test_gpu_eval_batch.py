"""eval_utils.caption_videos (one SST call, one selection launch, one caption pass for V videos) and forward_batch(event_group_rows=)
against the host chain built from the oracle's pieces, video by video (tests/props_batch_ref.py), with the project's existing gates:
proposal scores / encoder states 2e-5 absolute, proposals identical integers, sequences bit-exact after the per-video trim,
proposal_score 1e-6, sentence_confidence 1e-3, timestamp and num exact, eval log-probs 2e-5.

The oracle is fed the DEVICE's scores and encoder states (selection is discontinuous in them).  Bit-exact sequences need a resolvable
arg-max: every comparison asserts that the ORACLE's smallest top-1 / top-2 log-prob margin over all rows and decoded steps is >= 1e-4 -- a
condition on the inputs, chosen on the CPU with the oracle alone (the oracle's own encoder in front), not a measurement of the code under
test.  Smallest margins measured there: input seed 19 / encoder seed 3: 2.7e-4 with threshold selection, 5.5e-4 with NMS; given-event videos,
seed 950: 5.6e-4 (3.7e-4 with the <eos> bias of 0.25 that ends two of the five videos at the first step); grouping videos, seed 1070: 3.3e-4."""
import numpy as np
import pytest
import torch

from echr_amd import synth
from tests import props_batch_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

LENGTHS = (24, 1, 9, 40)
TOPN, DURATION, MARGIN = 12, 60.0, 1e-4
INPUT_SEED, TAP_SEED, GIVEN_SEED, GROUP_SEED = 19, 3, 950, 1070
f2t = lambda s, e, n, d: [round(float(s) / n * d, 3), round(float(e) / n * d, 3)]


def make_opt():
    opt, params, _ = synth.make_case('c1')
    opt.K = 8
    return opt, params


def make_inputs(opt, seed=INPUT_SEED):
    rs = np.random.RandomState(seed)
    return [dict(c3d=rs.standard_normal((T, opt.video_dim)).astype(np.float32), lda=rs.standard_normal(opt.lda_dim).astype(np.float32),
                 duration=DURATION) for T in LENGTHS]


def make_tap(opt, seed=TAP_SEED):
    from echr_amd import models as EM
    torch.manual_seed(seed)
    tap = EM.setup_tap(opt)
    tap.eval()
    return tap


def given_videos(opt, counts, seed=GIVEN_SEED):
    """Videos with ground-truth events (flag_eval_what='cg'): `counts` events each, 8..16 rows long."""
    out = []
    for i, n in enumerate(counts):
        v = synth.make_video(n, 16, 11, opt.CG_vocab_size + 1, seed=seed + i, T_v=20 + 3 * i, min_len=8, video_dim=opt.video_dim,
                             hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
        out.append(dict(c3d=v['c3d'], lda=v['lda'], duration=DURATION, ind=v['ind'], soi=v['soi'],
                        timestamps=[[float(s), float(e)] for s, e in np.asarray(v['soi']).tolist()]))
    return out


def to_dev(videos):
    dev = torch.device('cuda')
    return [dict(v, c3d=torch.from_numpy(v['c3d']).to(dev), lda=torch.from_numpy(v['lda']).to(dev)) for v in videos]


def host_chain(opt, params, videos, scores, taps, ro, **kw):
    """tests/props_batch_ref.caption_flow per video on the given (device) scores / encoder states."""
    P = {k: torch.from_numpy(v) for k, v in params.items()}
    out = []
    for v, vid in enumerate(videos):
        a, b = int(ro[v]), int(ro[v + 1])
        given = (vid['ind'], vid['soi'], vid['timestamps']) if kw.get('flag_eval_what') == 'cg' else None
        out.append(R.caption_flow(opt, P, scores[a:b], taps[a:b], vid['c3d'], vid['lda'], vid['duration'], f2t, TOPN, given=given, **kw))
    return out


@pytest.fixture(scope='module')
def models():
    opt, params = make_opt()
    return opt, params, make_tap(opt).cuda(), U.build_gpu_model(opt, params, False)


@pytest.fixture(scope='module')
def runs(models):
    """caption_videos on the four videos for nms in {0, 0.6}, each with its host chain -- computed once, read by several tests."""
    from echr_amd import eval_utils as EU
    opt, params, tap, cg = models
    videos = make_inputs(opt)
    out = {}
    for nms in (0.0, 0.6):
        infos, ex = EU.caption_videos(tap, cg, to_dev(videos), f2t, topN=TOPN, nms_threshold=nms)
        sc, tp = ex['pred_proposals'].cpu().numpy(), ex['tap_feats'].cpu().numpy()
        out[nms] = (infos, ex, host_chain(opt, params, videos, sc, tp, ex['row_offset'], nms_threshold=nms), videos)
    return out


def check_video(info, pv, want, T):
    """One video's records and tensors against its host chain."""
    assert [list(map(int, x)) for x in pv['soi_select_list']] == want['soi'] and [int(i) for i in pv['ind_select_list']] == want['ind']
    assert len(info) == len(want['info'])
    if not want['info']:
        return
    print('oracle margin %.3e' % want['margin'])
    assert want['margin'] >= MARGIN
    assert np.array_equal(pv['seq'].cpu().numpy(), want['seq'])                      # bit-exact after the per-video trim
    assert np.abs(pv['cg_prob'].cpu().numpy() - want['logp']).max() < 1e-3
    for i, (rec, ref) in enumerate(zip(info, want['info'])):
        assert rec['timestamp'] == ref['timestamp'] == f2t(want['soi'][i][0], want['soi'][i][1], T, DURATION) and rec['num'] == ref['num'] == [i, len(info)]
        assert abs(rec['proposal_score'] - ref['proposal_score']) < 1e-6
        assert abs(rec['sentence_confidence'] - ref['sentence_confidence']) < 1e-3
        assert abs(rec['re_score'] - (10 * rec['proposal_score'] + rec['sentence_confidence'])) < 1e-9
        assert rec['sentence'] == ref['sentence'] and set(rec) == set(ref)


@pytest.mark.parametrize('nms', [0.0, 0.6])
def test_caption_videos_vs_host_chain(models, runs, nms):
    from oracle import echr_ref_cpu as O
    opt, params, tap, cg = models
    infos, ex, want, videos = runs[nms]
    ro = ex['row_offset']
    assert ro.tolist() == [0, 24, 25, 34, 74] and len(infos) == 4
    P_tap = {k: v.detach().cpu() for k, v in tap.state_dict().items()}
    for v, vid in enumerate(videos):
        tap_o, sc_o = O.sst_forward(P_tap, torch.from_numpy(vid['c3d']))
        assert np.abs(ex['pred_proposals'][ro[v]:ro[v + 1]].cpu().numpy() - sc_o.numpy()).max() < 2e-5
        assert np.abs(ex['tap_feats'][ro[v]:ro[v + 1]].cpu().numpy() - tap_o.numpy()).max() < 2e-5
        check_video(infos[v], ex['per_video'][v], want[v], LENGTHS[v])
    counts = [len(w['ind']) for w in want]
    assert ex['selection']['count'].cpu().numpy()[:5].tolist() == counts + [sum(counts)]
    if nms:
        assert counts[1] == 0 and infos[1] == [] and ex['kept'] == [0, 2, 3]         # the one-row video has no NMS candidate: dropped from the batch
    else:
        assert counts == [12, 1, 12, 12] and ex['kept'] == [0, 1, 2, 3]
    b = ex['batch']
    assert b.n_videos == len(ex['kept']) and b.n_events == sum(counts) and len(ex['seq']) == sum(counts)
    assert max(len(i) for i in infos) > 0
    assert cg.training is False


def test_a_video_emptied_by_the_threshold_returns_nothing_and_leaves_the_others(models, runs):
    """val_score_thres above every score of video 2 but below the other videos' topN-th scores: video 2 gets [], the rest is unchanged."""
    from echr_amd import eval_utils as EU
    opt, params, tap, cg = models
    infos, ex, want, videos = runs[0.0]
    ro, sc = ex['row_offset'], ex['pred_proposals'].cpu().numpy()
    conf = [np.array(w['conf']) for w in want]
    # the video whose best pick is lowest is emptied; the threshold stays below every other video's weakest pick
    v_empty = int(np.argmin([c.max() for c in conf]))
    thres = float(conf[v_empty].max()) + 1e-6
    others_min = min(float(c.min()) for v, c in enumerate(conf) if v != v_empty)
    if others_min <= thres:
        pytest.fail('inputs: no threshold separates one video from the others (%.6f vs %.6f)' % (thres, others_min))
    infos2, ex2 = EU.caption_videos(tap, cg, to_dev(videos), f2t, topN=TOPN, val_score_thres=thres)
    assert np.abs(ex2['pred_proposals'].cpu().numpy() - sc).max() < 2e-5          # (the encoder's own run-to-run rounding)
    assert infos2[v_empty] == [] and ex2['kept'] == [v for v in range(4) if v != v_empty]
    assert int(ex2['selection']['count'][v_empty]) == 0
    for v in ex2['kept']:
        assert len(infos2[v]) == len(infos[v]) > 0
        for a, b in zip(infos2[v], infos[v]):
            assert a['sentence'] == b['sentence'] and a['timestamp'] == b['timestamp'] and a['num'] == b['num'] and abs(a['proposal_score'] - b['proposal_score']) < 1e-6
            assert abs(a['sentence_confidence'] - b['sentence_confidence']) < 1e-3
        assert np.array_equal(ex2['per_video'][v]['seq'].cpu().numpy(), ex['per_video'][v]['seq'].cpu().numpy())
    # nobody selected: all-empty lists, the decoder is never called
    infos3, ex3 = EU.caption_videos(tap, cg, to_dev(videos), f2t, topN=TOPN, val_score_thres=2.0)
    assert infos3 == [[], [], [], []] and ex3['batch'] is None and ex3['seq'] is None and ex3['kept'] == []


def test_flag_tap_skips_the_caption_pass(models, runs, monkeypatch):
    from echr_amd import eval_utils as EU
    opt, params, tap, cg = models
    infos, ex, want, videos = runs[0.6]

    def no_decoder(*a, **k):
        raise AssertionError("flag_eval_what='tap' must not run the caption pass")
    monkeypatch.setattr(cg, 'forward_batch', no_decoder)
    infos_t, ex_t = EU.caption_videos(tap, cg, to_dev(videos), f2t, topN=TOPN, nms_threshold=0.6, flag_eval_what='tap')
    assert ex_t['seq'] is None and infos_t[1] == []
    for v in (0, 2, 3):
        assert len(infos_t[v]) == len(want[v]['ind']) > 0
        for i, rec in enumerate(infos_t[v]):
            assert rec['sentence'] == 0 and rec['sentence_confidence'] == 0 and rec['num'] == [i, len(infos_t[v])]
            assert rec['timestamp'] == infos[v][i]['timestamp'] and abs(rec['proposal_score'] - infos[v][i]['proposal_score']) < 1e-6
            assert rec['re_score'] == 10 * rec['proposal_score']


@pytest.mark.parametrize('eos_bias', [0.0, 0.25])
def test_given_events_equal_single_video_calls_and_the_oracle(models, eos_bias):
    """flag_eval_what='cg', V = 5 with 3-4 events each: the records equal single-video mode='eval' calls (caption_video's caption half) on the
    same encoder states, and the host chain.  eos_bias 0.25 (added to the <eos> logit bias): every row of videos 1 and 2 emits <eos> first
    -- they get [] while the batch decodes on -- and the other videos keep finished rows beside unfinished ones."""
    from echr_amd import eval_utils as EU
    opt, params, tap, cg = models
    if eos_bias:
        params = dict(params)
        params['lm_model.logit.bias'] = params['lm_model.logit.bias'].copy()
        params['lm_model.logit.bias'][0] += np.float32(eos_bias)
        cg = U.build_gpu_model(opt, params, False)
    videos = given_videos(opt, (3, 4, 3, 4, 3))
    dv = to_dev(videos)
    infos, ex = EU.caption_videos(tap, cg, dv, f2t, flag_eval_what='cg')
    ro = ex['row_offset']
    assert ex['selection'] is None and ex['kept'] == [0, 1, 2, 3, 4]
    want = host_chain(opt, params, videos, ex['pred_proposals'].cpu().numpy(), ex['tap_feats'].cpu().numpy(), ro, flag_eval_what='cg')
    for v, vid in enumerate(videos):
        assert want[v]['margin'] >= MARGIN
        with torch.no_grad():
            seq, lp = cg(ex['tap_feats'][ro[v]:ro[v + 1]], dv[v]['c3d'], dv[v]['lda'], [], vid['ind'], vid['soi'], mode='eval')
        if len(seq) == 0:                                  # every row emitted <eos> first (reference eval_utils.py:131-132)
            assert len(want[v]['seq']) == 0 and infos[v] == [] and ex['per_video'][v]['seq'] is None and eos_bias
            continue
        assert np.array_equal(ex['per_video'][v]['seq'].cpu().numpy(), seq.cpu().numpy()) and np.array_equal(seq.cpu().numpy(), want[v]['seq'])
        assert np.abs(ex['per_video'][v]['cg_prob'].cpu().numpy() - lp.cpu().numpy()).max() < 2e-5
        score = lp.sum(1).cpu().numpy().astype('float')
        assert len(infos[v]) == len(vid['ind'])
        for i, rec in enumerate(infos[v]):
            assert rec['sentence'] == [int(t) for t in seq[i].cpu().numpy() if t > 0] == want[v]['info'][i]['sentence']
            assert rec['timestamp'] == vid['timestamps'][i] and rec['proposal_score'] == 1.0 and rec['num'] == [i, len(vid['ind'])]
            assert abs(rec['sentence_confidence'] - score[i]) < 1e-3 and abs(rec['sentence_confidence'] - want[v]['info'][i]['sentence_confidence']) < 1e-3
            assert abs(rec['re_score'] - (10.0 + rec['sentence_confidence'])) < 1e-9
    assert [len(i) > 0 for i in infos] == ([True, False, False, True, True] if eos_bias else [True] * 5)


def test_grouped_event_encoder_equals_the_block_diagonal_call(models):
    """forward_batch(mode='eval', event_group_rows=8) on videos with (3, 4, 12, 3, 4, 1) events: runs [0,2) | [2,3) | [3,6) -- a multi-video run whose
    first vid is not 0 and a 12-event video on the single-video route -- against event_group_rows=None on the same VideoBatch (seq identical,
    logp within 2e-5) and against per-video forward(mode='eval')."""
    from echr_amd.batch import VideoBatch
    opt, params, tap, cg = models
    videos = given_videos(opt, (3, 4, 12, 3, 4, 1), GROUP_SEED)
    with torch.no_grad():
        batch = VideoBatch.from_videos([dict(c3d=v['c3d'], lda=v['lda'], ind=v['ind'], soi=v['soi']) for v in to_dev(videos)], tap_model=tap)
        assert batch.event_groups(8) == [(0, 2, 0, 7), (2, 3, 7, 19), (3, 6, 19, 27)]
        seq0, lp0 = cg.forward_batch(batch, mode='eval')
        for G in (8, 1, 1000):
            seq1, lp1 = cg.forward_batch(batch, mode='eval', event_group_rows=G)
            assert np.array_equal(seq1.cpu().numpy(), seq0.cpu().numpy())
            assert np.abs(lp1.cpu().numpy() - lp0.cpu().numpy()).max() < 2e-5
        seq1, lp1 = cg.forward_batch(batch, mode='eval', event_group_rows=8)
        want = host_chain(opt, params, videos, np.zeros((batch.c3d.shape[0], 1), np.float32), batch.tap.cpu().numpy(), batch.row_offset, flag_eval_what='cg')
        for v in range(batch.n_videos):
            assert want[v]['margin'] >= MARGIN
            w = want[v]['seq'].shape[1]
            assert np.array_equal(seq1[batch.event_slices[v], :w].cpu().numpy(), want[v]['seq'])
        for v in range(batch.n_videos):
            d, s = batch.video(v), batch.event_slices[v]
            sv, lv = cg(d['tap'], d['c3d'], d['lda'], [], d['ind'], d['soi'], mode='eval')
            w = sv.shape[1]
            assert np.array_equal(seq1[s, :w].cpu().numpy(), sv.cpu().numpy()) and not seq1[s, w:].any()
            assert np.abs(lp1[s, :w].cpu().numpy() - lv.cpu().numpy()).max() < 2e-5

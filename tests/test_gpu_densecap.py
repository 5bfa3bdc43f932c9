"""Dense-caption scoring on the GPU (-m gpu): echr_amd.densecap.evaluate and eval_utils.dense_scores against the plain-Python oracle
tests/densecap_ref.py.

Required: the pair lists and every per-pair integer equal; Precision / Recall equal bit for bit (integer counts divided in fp64 on both
sides, IoU in one written order without a multiply next to an add); Bleu_n and ROUGE_L within 1e-12 relative (fp64 on both sides from
identical integers: what differs is a handful of log / exp / pow roundings and one possible contraction, ~1e-16 each); CIDErD within
tests/test_gpu_ciderd.py's 1e-5 absolute, its per-pair values being echr_ciderd_score's fp32 outputs."""
import functools
import math

import numpy as np
import pytest
import torch

from echr_amd import densecap as D
from echr_amd import reward as RW
from echr_amd import synth
from tests import ciderd_ref as CR
from tests import densecap_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

REL, CIDER_TOL = 1e-12, 1e-5
TIOUS = (0.3, 0.5, 0.7, 0.9)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _make(seed, P, G, L, top, full=False):
    """V = len(P) videos with P[v] predictions and G[v] ground truths.  A video of 7 ground truths has them crowded around one interval,
    and most predictions are jittered copies of a ground truth: many partners per prediction at 0.3, few at 0.9.  Captions are random
    words, references with a token replaced, or references with their first bigram repeated in front (clipping)."""
    rs = np.random.RandomState(seed)
    vids, pst, caps, p_off = [], [], [], [0]
    for pv, gv in zip(P, G):
        base = rs.uniform(5.0, 40.0)
        ts = np.stack([base + rs.uniform(-4.0, 4.0, gv), base + 30.0 + rs.uniform(-4.0, 4.0, gv)], 1)
        lo = L if full else 1
        sents = [rs.randint(1, top + 1, size=rs.randint(lo, L + 1)).tolist() for _ in range(gv)]
        vids.append(dict(timestamps=ts, sentences=sents))
        for i in range(pv):
            g = rs.randint(gv)
            kind = i % 4
            if kind == 0:
                s = rs.uniform(0.0, 80.0)
                pst.append([s, s + rs.uniform(1.0, 40.0)])
            else:
                w = (0.5, 3.0, 12.0)[kind - 1]
                pst.append([ts[g, 0] + rs.uniform(-w, w), ts[g, 1] + rs.uniform(-w, w)])
            ref = list(sents[g])
            if full:
                row = rs.randint(1, top + 1, size=L).tolist() if kind == 0 else ref
                if kind == 1:
                    row = list(ref)
                    row[rs.randint(L)] = int(rs.randint(1, top + 1))
            elif kind == 0:
                row = rs.randint(1, top + 1, size=rs.randint(0, L + 1)).tolist()
            elif kind == 1:
                row = list(ref)
                row[rs.randint(len(row))] = int(rs.randint(1, top + 1))
            elif kind == 2:
                row = (ref[:2] + ref)[:L]
            else:
                row = ref
            caps.append((row + [0] * L)[:L])
        p_off.append(len(pst))
    gt = D.pack_ground_truth(vids, L, top)
    sc = RW.CiderD.from_corpus([[s] for v in vids for s in v['sentences']], L, top)
    return dict(gt=gt, sc=sc, pst=np.asarray(pst, np.float64).reshape(-1, 2), caps=np.asarray(caps, np.int64).reshape(-1, L), p_off=np.asarray(p_off, np.int32),
                L=L, top=top, vids=vids)


def _oracle(c, tious=TIOUS, rows=None):
    """The oracle on the case (or on the videos `rows` of it, in that order)."""
    g_off = c['gt'].offset.numpy()
    vs = list(range(len(g_off) - 1)) if rows is None else list(rows)
    pi = [i for v in vs for i in range(c['p_off'][v], c['p_off'][v + 1])]
    gi = [j for v in vs for j in range(g_off[v], g_off[v + 1])]
    p_off = np.concatenate([[0], np.cumsum([c['p_off'][v + 1] - c['p_off'][v] for v in vs])])
    go = np.concatenate([[0], np.cumsum([g_off[v + 1] - g_off[v] for v in vs])])
    refs = c['gt'].refs.numpy()[gi]
    df, n = CR.document_frequency([[CR.sequence(r, c['L'])] for r in c['gt'].refs.numpy()])
    memo = {}

    def fn(p, g):          # a pair recurs at every threshold it reaches
        if (p, g) not in memo:
            memo[p, g] = CR.score(CR.sequence(c['caps'][pi[p]], c['L']), [CR.sequence(refs[g], c['L'])], df, n)
        return memo[p, g]
    return R.evaluate(c['pst'][pi], p_off, c['caps'][pi], c['gt'].stamps.numpy()[gi], go, refs, tious, fn)


def _device(c, tious=TIOUS, seq=None, scorer=True, captions=True):
    seq = torch.from_numpy(c['caps']).cuda() if seq is None else seq
    return D.evaluate(torch.from_numpy(c['pst']).cuda(), c['p_off'], seq if captions else None, c['gt'].cuda(), tious,
                      scorer=c['sc'] if scorer and captions else None)


@functools.lru_cache(maxsize=None)
def _main():
    """V = 6, P_v in {0, 1, 5, 64, 65, 300}, G_v in {1, 7}, L = 20 over 30 words."""
    c = _make(5, (0, 1, 5, 64, 65, 300), (7, 1, 7, 1, 7, 7), 20, 30)
    return c, _oracle(c), _device(c)


def _check(res, o, tious=TIOUS, cider=True, language=True):
    nt = len(tious)
    # the pair lists and the per-pair integers
    want_pairs = [pg for k in range(nt) for pg in o['pairs'][k]]
    if res.pairs is None:
        assert not want_pairs
    else:
        got = list(zip(res.pairs['pair_pred'].cpu().tolist(), res.pairs['pair_gt'].cpu().tolist()))
        assert got == want_pairs
        assert res.pairs['totals'] == [0] + np.cumsum([len(o['pairs'][k]) for k in range(nt)]).tolist()
        if language:
            want_stats = [s for k in range(nt) for s in o['stats'][k]]
            assert [tuple(s) for s in res.pairs['stats'].cpu().tolist()] == want_stats
    assert np.array_equal(res.n_pairs, np.asarray(o['n_pairs'])) and np.array_equal(res.n_unmatched, np.asarray(o['n_unmatched']))
    # detection: bit for bit
    pv = res.per_video
    for name in ('Recall', 'Precision'):
        assert np.array_equal(getattr(res, name), np.asarray(o[name])), name
        assert np.array_equal(pv[name], np.asarray(o['video'][name])), name
    assert np.array_equal(res.f1(), np.asarray(o['f1']))
    if not language:
        assert all(getattr(res, n) is None and pv[n] is None for n in D.LANGUAGE)
        return
    for name in ('Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L'):
        for got, want in ((getattr(res, name), np.asarray(o[name])), (pv[name], np.asarray(o['video'][name]))):
            assert got.shape == want.shape and np.isfinite(got).all()
            err = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
            print('%s max relative error %.3e (max value %.3e)' % (name, err.max(), want.max()))
            assert (np.abs(got - want) <= REL * np.abs(want)).all(), (name, err.max())
    if cider:
        for got, want in ((res.CIDErD, np.asarray(o['CIDErD'])), (pv['CIDErD'], np.asarray(o['video']['CIDErD']))):
            print('CIDErD max |gpu - oracle| = %.3e (max value %.3e)' % (np.abs(got - want).max(), want.max()))
            assert np.abs(got - want).max() < CIDER_TOL
    else:
        assert res.CIDErD is None and pv['CIDErD'] is None


# ---- the main case ----------------------------------------------------------------------------------------------------------------
def test_main_case_meets_its_conditions_and_matches_the_oracle():
    c, o, res = _main()
    n_pairs = np.asarray(o['n_pairs'])
    stats = np.asarray([s for k in range(4) for s in o['stats'][k]])
    print('pairs per (tau, video):\n%s\nunmatched:\n%s' % (n_pairs, np.asarray(o['n_unmatched'])))
    # conditions on the inputs, from the oracle alone
    assert n_pairs.max() > 1024 and ((n_pairs > 256) & (n_pairs <= 1024)).any()
    assert (n_pairs[:, 0] == 0).all() and np.asarray(o['n_unmatched'])[3].sum() > 0 and (np.asarray(o['n_unmatched'])[0] < n_pairs[0]).any()
    clipped = sum(1 for k in range(4) for (p, g), s in zip(o['pairs'][k], o['stats'][k])
                  if g >= 0 and s[0] < min(s[4], s[5]) and len(set(R.words(c['caps'][p]))) < s[4])
    assert clipped > 0 and (stats[:, 6] > 0).any() and (stats[:, 3] > 0).any() and (stats[:, 4] == 0).any()
    assert all(0 < x < 1 for x in o['Precision'] + o['Recall']) and len(set(o['Precision'])) == 4
    assert all(x > 1e-3 for x in o['Bleu_4']) and all(x > 0.05 for x in o['ROUGE_L']) and all(x > 0.1 for x in o['CIDErD'])
    assert res.video.dtype == torch.float64 and res.video.is_cuda and tuple(res.video.shape) == (4, 6, D.VIDEO_COLS)
    _check(res, o)


def test_seq_length_63_with_full_length_captions_and_references():
    c = _make(8, (9, 3), (2, 3), 63, 30, full=True)
    assert (c['caps'] != 0).all() and (c['gt'].refs != 0).all()
    o = _oracle(c)
    st = np.asarray([s for k in range(4) for s in o['stats'][k]])
    m = st[st[:, 5] > 1]                                                                     # the matched pairs
    assert (st[:, 4] == 63).all() and (m[:, 5] == 63).all() and m[:, 6].max() == 63 and 0 < m[:, 6].min() < 63 and len(m) < len(st)
    _check(_device(c), o)


def test_int32_and_strided_captions_are_bitwise_the_contiguous_int64_result():
    c, o, res = _main()
    rows = torch.from_numpy(c['caps']).cuda()
    wide = torch.full((rows.shape[0], 40), 7, dtype=torch.int64, device='cuda')
    wide[:, ::2] = rows
    tr = rows.t().contiguous().t()
    assert not wide[:, ::2].is_contiguous() and tr.stride() == (1, rows.shape[0])
    for seq in (rows.to(torch.int32), wide[:, ::2], tr, tr.to(torch.int32)):
        r2 = _device(c, seq=seq)
        assert torch.equal(r2.video, res.video) and torch.equal(r2.mean, res.mean)
        assert torch.equal(r2.pairs['stats'], res.pairs['stats'])
    narrow = _make(5, (0, 1, 5, 64, 65, 300), (7, 1, 7, 1, 7, 7), 20, 30)          # the same captions cut at 12 columns
    narrow['caps'] = np.ascontiguousarray(c['caps'][:, :12])
    _check(D.evaluate(torch.from_numpy(c['pst']).cuda(), c['p_off'], torch.from_numpy(narrow['caps']).cuda(), c['gt'].cuda(), TIOUS, scorer=c['sc']),
           _oracle(narrow))


def test_a_threshold_equal_to_an_iou_pairs_without_a_hit():
    c = _make(13, (3,), (1,), 20, 30)
    gs, ge = c['gt'].stamps[0].tolist()
    c['pst'][0] = [gs - 7.0, ge - 11.0]
    tau = R.iou(c['pst'][0][0], c['pst'][0][1], gs, ge)
    others = [R.iou(s, e, gs, ge) for s, e in c['pst'][1:]]
    assert 0.2 < tau < 0.9 and all(abs(x - tau) > 1e-3 for x in others)
    tious = (tau, math.nextafter(tau, 0.0), math.nextafter(tau, 1.0))
    o = _oracle(c, tious)
    assert (0, 0) in o['pairs'][0] and (0, 0) in o['pairs'][1] and (0, 0) not in o['pairs'][2]
    below = sum(x > tau for x in others)
    assert o['video']['Precision'][0][0] == below / 3 and o['video']['Precision'][1][0] == (below + 1) / 3
    _check(_device(c, tious), o, tious)


def test_detection_only_and_no_scorer():
    c, o, _ = _main()
    _check(_device(c, captions=False), o, language=False)
    _check(_device(c, scorer=False), o, cider=False)


# ---- independence -----------------------------------------------------------------------------------------------------------------
def _sub(c, rows):
    g_off, p_off = c['gt'].offset.numpy(), c['p_off']
    pi = np.concatenate([np.arange(p_off[v], p_off[v + 1]) for v in rows]).astype(np.int64)
    out = dict(c, gt=D.pack_ground_truth([c['vids'][v] for v in rows], c['L'], c['top']), pst=c['pst'][pi], caps=c['caps'][pi],
               p_off=np.concatenate([[0], np.cumsum([p_off[v + 1] - p_off[v] for v in rows])]).astype(np.int32))
    assert out['gt'].stamps.shape[0] == sum(g_off[v + 1] - g_off[v] for v in rows)
    return out


def test_a_videos_numbers_do_not_depend_on_the_call():
    c, o, res = _main()
    again = _device(c)
    assert torch.equal(again.video, res.video) and torch.equal(again.mean, res.mean)          # two identical calls
    for k in ('pair_pred', 'pair_gt', 'stats', 'rouge', 'cider'):
        assert torch.equal(again.pairs[k], res.pairs[k])
    for v in (0, 3, 5):                                                                        # a video alone (0: without predictions)
        one = _device(_sub(c, [v]))
        assert torch.equal(one.video[:, 0], res.video[:, v]), v
    order = [5, 4, 3, 2, 1, 0]
    rev = _device(_sub(c, order))
    assert torch.equal(rev.video, res.video[:, order])
    _check(rev, _oracle(c, rows=order))


def test_a_call_without_any_prediction():
    c = _make(3, (0, 0), (2, 1), 20, 30)
    res = _device(c)
    assert res.pairs is None and not res.video.any() and not res.mean.any()
    _check(res, _oracle(c))


# ---- end to end -------------------------------------------------------------------------------------------------------------------
LENGTHS, DURATION = (24, 1, 9, 40), 60.0
f2t = lambda s, e, n, d: [round(float(s) / n * d, 3), round(float(e) / n * d, 3)]


@functools.lru_cache(maxsize=None)
def _models():
    from echr_amd import models as EM
    opt, params, _ = synth.make_case('c1')
    opt.K = 8
    torch.manual_seed(3)
    tap = EM.setup_tap(opt)
    tap.eval()
    rs = np.random.RandomState(19)
    videos = [dict(c3d=torch.from_numpy(rs.standard_normal((T, opt.video_dim)).astype(np.float32)).cuda(),
                   lda=torch.from_numpy(rs.standard_normal(opt.lda_dim).astype(np.float32)).cuda(), duration=DURATION) for T in LENGTHS]
    L, top = opt.CG_seq_length, opt.CG_vocab_size
    tap, cg = tap.cuda(), U.build_gpu_model(opt, params, False)
    # ground truth that the model's own output can meet: per video, events next to its first and last record whose sentences are those
    # records' with one word replaced -- a random model's captions share next to nothing with random sentences
    from echr_amd import eval_utils as EU
    infos, _ = EU.caption_videos(tap, cg, videos, f2t, topN=8)
    gts = []
    for info in infos:
        ts, ss = [[0.0, 30.0]], [rs.randint(1, top + 1, size=rs.randint(1, L + 1)).tolist()]
        for r in ([info[0], info[-1]] if info else []):
            words = list(r['sentence']) or [int(rs.randint(1, top + 1))]
            words[rs.randint(len(words))] = int(rs.randint(1, top + 1))
            ts.append([r['timestamp'][0], r['timestamp'][1] + 0.7])
            ss.append(words)
        gts.append(dict(timestamps=ts, sentences=ss))
    gt = D.pack_ground_truth(gts, L, top)
    sc = RW.CiderD.from_corpus([[s] for v in gts for s in v['sentences']], L, top)
    return opt, tap, cg, videos, gt, sc


def _records_oracle(infos, gt, L, cider_scorer=None, captions=True, corpus=None):
    pst = [r['timestamp'] for info in infos for r in info]
    p_off = np.concatenate([[0], np.cumsum([len(i) for i in infos])])
    caps = [(list(r['sentence']) + [0] * L)[:L] for info in infos for r in info] if captions else None
    fn = None
    if cider_scorer is not None:
        refs = gt.refs.numpy()
        df, n = CR.document_frequency([[CR.sequence(r, L)] for r in (gt if corpus is None else corpus).refs.numpy()])
        fn = lambda p, g: CR.score(CR.sequence(caps[p], L), [CR.sequence(refs[g], L)], df, n)
    return R.evaluate(pst, p_off, caps, gt.stamps.numpy(), gt.offset.numpy(), gt.refs.numpy(), TIOUS, fn)


def test_dense_scores_of_a_caption_videos_result():
    from echr_amd import eval_utils as EU
    opt, tap, cg, videos, gt, sc = _models()
    infos, ex = EU.caption_videos(tap, cg, videos, f2t, topN=8)
    assert sum(len(i) for i in infos) > 8 and any(len(r['sentence']) for i in infos for r in i)
    res = EU.dense_scores(infos, ex, gt.cuda(), scorer=sc)
    o = _records_oracle(infos, gt, opt.CG_seq_length, sc)
    print('end to end: Recall %s ROUGE_L %s CIDErD %s' % (o['Recall'], o['ROUGE_L'], o['CIDErD']))
    assert max(o['Recall']) > 0 and np.asarray(o['n_pairs']).sum() > np.asarray(o['n_unmatched']).sum()
    assert min(o['ROUGE_L']) > 0.01 and min(o['Bleu_1']) > 0.01 and min(o['CIDErD']) > 0.01          # the language scores are exercised
    _check(res, o)


def test_dense_scores_of_a_tap_result_is_detection_only():
    from echr_amd import eval_utils as EU
    opt, tap, cg, videos, gt, sc = _models()
    infos, ex = EU.caption_videos(tap, cg, videos, f2t, topN=8, flag_eval_what='tap')
    assert ex['seq'] is None and sum(len(i) for i in infos) > 8
    res = EU.dense_scores(infos, ex, gt.cuda())
    _check(res, _records_oracle(infos, gt, opt.CG_seq_length, captions=False), language=False)
    assert res.Bleu_4 is None and res.f1().shape == (4,)


def test_dense_scores_of_a_single_video_result():
    from echr_amd import eval_utils as EU
    opt, tap, cg, videos, gt, sc = _models()
    v = 3
    info, ex = EU.caption_video(tap, cg, videos[v]['c3d'], videos[v]['lda'], DURATION, f2t, topN=8)
    g0, g1 = gt.offset[v].item(), gt.offset[v + 1].item()
    one = D.GroundTruth(gt.stamps[g0:g1], torch.tensor([0, g1 - g0], dtype=torch.int32), gt.refs[g0:g1], gt.ref_len[g0:g1])
    assert len(info) > 1 and 'per_video' not in ex
    res = EU.dense_scores(info, ex, one.cuda(), scorer=sc)
    o = _records_oracle([info], one, opt.CG_seq_length, sc, corpus=gt)
    assert max(o['ROUGE_L']) > 0.01 and max(o['CIDErD']) > 0.01
    _check(res, o)


def test_cpu_tensors_raise():
    from echr_amd._lib import EchrHipError
    c, _, _ = _main()
    pst, seq = torch.from_numpy(c['pst']), torch.from_numpy(c['caps'])
    with pytest.raises(EchrHipError):
        D.evaluate(pst, c['p_off'], seq.cuda(), c['gt'].cuda())
    with pytest.raises(EchrHipError):
        D.evaluate(pst.cuda(), c['p_off'], seq, c['gt'].cuda())
    with pytest.raises(EchrHipError):
        D.evaluate(pst.cuda(), c['p_off'], seq.cuda(), c['gt'])

"""The one-stream decoder (caption_model='show_attend_tell') over multi-video batches on the GPU (-m gpu): forward_batch in training and
greedy evaluation against the reference's own batch fixture (tests/golden/case_sat_batch.npz, tools/make_golden_sat_batch.py), against
tests/sat_batch_ref.py carried in float64 on edge batches, and against the single-video entries it must equal.

Gates: those of tests/test_gpu_sat.py (log-probs / losses 3e-6 relative, gradients and d tap 5e-5 of the tensor's max-norm: ten times the
noise measured there; the project's bounds are 1e-4 / 1e-4 / 1e-3); two HIP results against each other 2 x TOL_LOGP; greedy indices exact
at the positions whose float64 margin resolves at 1e-4 -- at least 90 % of every greedy case, asserted on the CPU by
tests/test_sat_batch_host.py.  Every test prints its figures ahead of its assertions."""
import functools

import numpy as np
import pytest
import torch

from tests import sat_batch_ref as B
from tests import sat_ref as R
from tests import util as U
from tests.test_gpu_sat import MARGIN, TOL_GRAD, TOL_LOGP, TOL_LOSS

pytestmark = pytest.mark.gpu

SAT = 'show_attend_tell'


def _dev():
    return torch.device('cuda')


def _batch(opt, videos, labels=True, tap_grad=False):
    from echr_amd.batch import VideoBatch
    keys = ('c3d', 'tap', 'lda', 'ind', 'soi') + (('labels', 'masks') if labels else ())
    b = VideoBatch.from_videos([{k: v[k] for k in keys} for v in videos], device=_dev(), caption_model=SAT,
                               CG_init_feats_type=opt.CG_init_feats_type)
    b.tap.requires_grad_(tap_grad)
    return b


def _run(opt, params, videos, train_mode, m=None):
    """forward_batch(mode='train') + batch.criterion + backward: dict like sat_batch_ref.run's, plus the module."""
    from echr_amd.misc.utils import LanguageModelCriterion
    m = m if m is not None else U.build_gpu_model(opt, params, train_mode)
    b = _batch(opt, videos, tap_grad=True)
    logp = m.forward_batch(b, mode='train')
    loss, per = b.criterion(LanguageModelCriterion(), logp)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}
    g_tap = b.tap.grad.cpu().numpy() if b.tap.grad is not None else np.zeros(tuple(b.tap.shape), np.float32)
    ro, lp = b.row_offset, logp.detach().cpu().numpy()
    assert lp.shape[:2] == (b.n_events, b.S)
    return dict(logp=[lp[s, :b.steps[v]] for v, s in enumerate(b.event_slices)], loss=float(loss.detach()), losses=per.detach().cpu().numpy(),
                grads=grads, g_tap=[g_tap[ro[v]:ro[v + 1]] for v in range(b.n_videos)], m=m, full=lp)


def _check(tag, got, ref, opt):
    e_logp = max(U.relerr(a, b) for a, b in zip(got['logp'], ref['logp']))
    e_loss = max(abs(got['loss'] - ref['loss']) / abs(ref['loss']), float(np.abs(got['losses'] - ref['losses']).max() / np.abs(ref['losses']).max()))
    errs = {}
    for k, g in ref['grads'].items():
        if g is None:
            assert got['grads'][k] is None or not np.any(got['grads'][k]), k
        elif k in R.NOISE_ONLY:
            assert float(np.abs(got['grads'][k]).max()) < 1e-6 and float(np.abs(g).max()) < 1e-6, k
        else:
            errs[k] = U.relerr(got['grads'][k], g, U.GRAD_FLOOR)
    e_tap = max(U.relerr(a, b, U.GRAD_FLOOR) for a, b in zip(got['g_tap'], ref['g_tap']))
    worst = max(errs, key=errs.get)
    print('[%s] logp %.2e  loss %.2e  worst gradient %.2e (%s)  d tap %.2e' % (tag, e_logp, e_loss, errs[worst], worst, e_tap))
    assert all(a.shape == b.shape for a, b in zip(got['logp'], ref['logp']))
    assert e_logp < TOL_LOGP and e_loss < TOL_LOSS
    assert errs[worst] < TOL_GRAD and e_tap < TOL_GRAD


# ---- 1. the reference's fixture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('train_mode', [False, True], ids=['eval', 'train'])
def test_fixture_full_tensors(train_mode):
    g = U.gold('case_sat_batch.npz')
    opt, params, videos = B.make_case('fixture')
    key = 'fixture|' + ('train' if train_mode else 'eval')
    V = len(videos)
    ref = dict(logp=[g['%s|logp|%d' % (key, v)] for v in range(V)], loss=float(g[key + '|loss']), losses=g[key + '|losses'],
               grads={k: g.get(key + '|grad|' + k) for k in params}, g_tap=[g['%s|gtap|%d' % (key, v)] for v in range(V)])
    got = _run(opt, params, videos, train_mode)
    _check(key, got, ref, opt)
    assert any(np.any(t) for t in got['g_tap'])          # (d batch.tap: 'ER3' reads the anchors' states)


# ---- 2. edge batches against float64 -----------------------------------------------------------------------------------------------------
EDGES = [(c, f, ()) for c in ('edge3', 'tile65', 'widths') for f in ('VEC', 'V', 'VE', 'C')] + [
    ('edge3', 'V', (('lda_dim', 10),)), ('edge3', 'VEC', (('lda_dim', 10),)),
    ('edge3', 'VEC', (('event_context_type', 'EH'), ('video_context_type', 'VLVCVH'))),
    ('edge3', 'VEC', (('CG_init_feats_type', 'VEC'),)), ('edge3', 'VEC', (('CG_init_feats_type', 'C'),)),
]


@functools.lru_cache(maxsize=None)
def _ref64(case, feats, over, train_mode):
    opt, params, videos = B.make_case(case, feats, **dict(over))
    return B.run(opt, params, videos, train_mode, dtype=torch.float64)


@pytest.mark.parametrize('train_mode', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('case,feats,over', EDGES, ids=['%s-%s%s' % (c, f, ''.join('-' + str(v) for _, v in o)) for c, f, o in EDGES])
def test_edge_batches_against_float64(case, feats, over, train_mode):
    opt, params, videos = B.make_case(case, feats, **dict(over))
    counts = [len(v['soi']) for v in videos]
    if case == 'edge3':          # (conditions on the inputs)
        steps = [R.O.n_decoder_steps(v['labels']) for v in videos]
        assert counts == [1, 3, 2] and [v['T_v'] for v in videos] == [9, 14, 11] and steps[2] == 3 < max(steps) == 6
        assert 1 in (videos[1]['soi'][:, 1] - videos[1]['soi'][:, 0]) and max(int((v['soi'][:, 1] - v['soi'][:, 0]).max()) for v in videos) == 7
        assert len({int((v['soi'][:, 1] - v['soi'][:, 0]).max()) for v in videos}) == 3          # different padded clip lengths
    if case == 'tile65':
        assert sum(counts) == 65 and counts[0] == 13
    if case == 'widths':
        assert opt.CG_rnn_size == 512 and opt.video_dim == 500 and counts == [2, 1]
    got = _run(opt, params, videos, train_mode)
    _check('%s/%s/%s/%s' % (case, feats, dict(over), 'train' if train_mode else 'eval'), got, _ref64(case, feats, over, train_mode), opt)
    if dict(over).get('event_context_type') == 'EH':
        assert all(np.any(t) for t in got['g_tap'])          # through 'EH' (the anchors) and 'VH' (every row)


# ---- 3. a batch against V sequential calls -------------------------------------------------------------------------------------------------
def _single(m, vid, mode='train'):
    tap, c3d, lda = (torch.from_numpy(np.ascontiguousarray(vid[k])).to(_dev()) for k in ('tap', 'c3d', 'lda'))
    with torch.no_grad():
        return m(tap, c3d, lda, torch.from_numpy(vid['labels']) if mode == 'train' else [], vid['ind'], vid['soi'], mode=mode)


@pytest.mark.parametrize('case,feats', [('edge3', 'VEC'), ('tile65', 'VE'), ('fixture', 'V')])
def test_eval_batch_equals_sequential_forward_calls(case, feats):
    opt, params, videos = B.make_case(case, feats)
    m = U.build_gpu_model(opt, params, False)
    b = _batch(opt, videos)
    with torch.no_grad():
        logp = m.forward_batch(b, mode='train')
    worst = 0.0
    for v, s in enumerate(b.event_slices):
        one = _single(m, videos[v])
        assert one.shape[1] == b.steps[v]
        worst = max(worst, U.relerr(logp[s, :b.steps[v]].cpu().numpy(), one.cpu().numpy()))
    print('[batch vs sequential/%s/%s] logp %.2e' % (case, feats, worst))
    assert worst < 2 * TOL_LOGP


# ---- 4. a one-video batch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('feats', ['VEC', 'V', 'VE', 'C'])
@pytest.mark.parametrize('init', ['', 'VEC'])
def test_one_video_batch_is_the_single_video_call_bit_for_bit(feats, init):
    """Eval mode, 'EH' (no event encoder in front: whole calls are compared): the scene part arrives as a per-row addend where the
    single-video entry adds one row -- the same add at the same place."""
    opt, params, videos = B.make_case('fixture', feats, event_context_type='EH', CG_init_feats_type=init)
    vid = videos[1]
    m = U.build_gpu_model(opt, params, False)
    b = _batch(opt, [vid])
    with torch.no_grad():
        logp = m.forward_batch(b, mode='train')
        seq, lp = m.forward_batch(b, mode='eval')
    one = _single(m, vid)
    seq1, lp1 = _single(m, vid, 'eval')
    assert torch.equal(logp, one)
    assert torch.equal(seq, seq1) and torch.equal(lp, lp1)


# ---- 5. greedy decode of a batch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['fixture', 'eos'])
def test_greedy_decode_of_a_batch(case):
    opt, params, videos = B.make_case(case)
    per = B.sample(opt, params, videos, torch.float64)
    rseq, _, widths = B.stack_sample(per, videos)
    ok = B.resolvable(per, MARGIN)
    if case == 'eos':
        assert len(set(widths.tolist())) > 1 and widths.min() > 0          # (condition on the inputs: captions end at different steps)
    m = U.build_gpu_model(opt, params, False)
    b = _batch(opt, videos, labels=False)
    seq, lp = m.forward_batch(b, mode='eval')
    seq_h, lp_h = seq.cpu().numpy(), lp.cpu().numpy()
    assert seq.dtype == torch.int64 and seq_h.shape == rseq.shape
    g = U.gold('case_sat_batch.npz')
    worst = 0.0
    for v, s in enumerate(b.event_slices):
        w = int(widths[v])
        assert int((seq_h[s] > 0).any(0).sum()) == w and not seq_h[s, w:].any()          # zero-padded behind the video's own width
        assert np.array_equal(seq_h[s, :w][ok[v]], per[v][0][ok[v]])
        worst = max(worst, U.relerr(lp_h[s, :w][ok[v]], per[v][1][ok[v]]))
        seq1, lp1 = _single(m, videos[v], 'eval')
        assert tuple(seq1.shape) == (s.stop - s.start, w)
        assert np.array_equal(seq1.cpu().numpy()[ok[v]], seq_h[s, :w][ok[v]])
        worst = max(worst, U.relerr(lp_h[s, :w][ok[v]], lp1.cpu().numpy()[ok[v]]) / 2)
        if case == 'fixture':
            fok = np.logical_and.accumulate(g['fixture|sample|margin|%d' % v] > MARGIN, axis=1)
            assert np.array_equal(seq_h[s, :w][fok], g['fixture|sample|seq|%d' % v][fok])
            worst = max(worst, U.relerr(lp_h[s, :w][fok], g['fixture|sample|logp|%d' % v][fok]))
    print('[greedy/%s] %s widths %s logp %.2e' % (case, seq_h.shape, widths.tolist(), worst))
    assert worst < TOL_LOGP


# ---- 6. cross-video isolation ----------------------------------------------------------------------------------------------------------------
def test_scaling_one_video_leaves_the_others_bit_identical():
    import echr_amd
    opt, params, videos = B.make_case('edge3', 'VEC', video_context_type='VLVCVH', CG_init_feats_type='VEC')
    hot = 1
    scaled = [dict(v) for v in videos]
    for k in ('c3d', 'tap', 'lda'):
        scaled[hot][k] = (videos[hot][k] * np.float32(10.0)).astype(np.float32)
    m = U.build_gpu_model(opt, params, False)
    echr_amd.set_deterministic(True)
    try:
        with torch.no_grad():
            b0, b1 = _batch(opt, videos), _batch(opt, scaled)
            a = m.forward_batch(b0, mode='train').cpu().numpy()
            c = m.forward_batch(b1, mode='train').cpu().numpy()
    finally:
        echr_amd.set_deterministic(False)
    for v, s in enumerate(b0.event_slices):
        if v == hot:
            assert not np.array_equal(a[s], c[s])
        else:
            assert np.array_equal(a[s], c[s]), v


# ---- 7. fixed-order mode ---------------------------------------------------------------------------------------------------------------------
def test_deterministic_batched_iterations_agree_bit_for_bit():
    import echr_amd
    from echr_amd.misc.utils import LanguageModelCriterion, clip_gradient
    from echr_amd.optim import ClampAdam
    opt, params, videos = B.make_case('edge3', 'VEC', video_context_type='VLVCVH', CG_init_feats_type='VEC')
    runs = []
    echr_amd.set_deterministic(True)
    try:
        for _ in range(2):
            m = U.build_gpu_model(opt, params, True)
            o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
            b = _batch(opt, videos, tap_grad=True)
            o.zero_grad()
            loss, per = b.criterion(LanguageModelCriterion(), m.forward_batch(b, mode='train'))
            loss.backward()
            grads = m._echr_arena.flat_g.clone()
            clip_gradient(o, 0.05)
            o.step()
            torch.cuda.synchronize()
            runs.append((float(loss), per.detach().cpu().numpy(), grads.cpu().numpy(), b.tap.grad.cpu().numpy(),
                         {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}))
    finally:
        echr_amd.set_deterministic(False)
    (la, pa, ga, ta, sa), (lb, pb, gb, tb, sb) = runs
    assert la == lb and np.array_equal(pa, pb) and np.array_equal(ga, gb) and np.array_equal(ta, tb) and np.any(ga)
    moved = 0
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
        moved += int(not np.array_equal(sa[k], params[k]))
    assert moved > 10


# ---- 8. the evaluation pass ----------------------------------------------------------------------------------------------------------------
F2T = lambda s, e, n, d: [round(float(s) / n * d, 3), round(float(e) / n * d, 3)]


def _tap_model(opt):
    from echr_amd import models as EM
    opt.K = 8
    torch.manual_seed(3)
    tap = EM.setup_tap(opt).cuda()
    tap.eval()
    return tap


def _same_records(got, want):
    assert len(got) == len(want) > 0
    for a, b in zip(got, want):
        assert a['sentence'] == b['sentence'] and a['timestamp'] == b['timestamp'] and a['num'] == b['num'] and set(a) == set(b)
        assert abs(a['proposal_score'] - b['proposal_score']) < 1e-6 and abs(a['sentence_confidence'] - b['sentence_confidence']) < 1e-3


def test_caption_videos_given_events():
    from echr_amd import eval_utils as EU
    opt, params, videos = B.make_case('eos')
    tap, cg = _tap_model(opt), U.build_gpu_model(opt, params, False)
    dev_v = [dict(c3d=torch.from_numpy(v['c3d']).to(_dev()), lda=torch.from_numpy(v['lda']).to(_dev()), duration=60.0, ind=v['ind'], soi=v['soi'],
                  timestamps=[[float(s), float(e)] for s, e in v['soi'].tolist()]) for v in videos]
    infos, ex = EU.caption_videos(tap, cg, dev_v, F2T, flag_eval_what='cg')
    assert ex['batch'].one_stream and len(infos) == 3
    for v, d in enumerate(dev_v):
        with torch.no_grad():
            tf, _ = tap(d['c3d'])
            seq, lp = cg(tf, d['c3d'], d['lda'], [], d['ind'], d['soi'], mode='eval')
        assert torch.equal(ex['per_video'][v]['seq'], seq)
        conf = lp.sum(1).cpu().numpy().astype('float')
        want = [dict(sentence=row[row > 0].tolist(), timestamp=d['timestamps'][i], sentence_confidence=conf[i], proposal_score=1.0,
                     re_score=10.0 + conf[i], num=[i, len(seq)]) for i, row in enumerate(seq.cpu().numpy())]
        _same_records(infos[v], want)


def test_caption_videos_nms_proposals():
    from echr_amd import eval_utils as EU
    opt, params, videos = B.make_case('eos')
    tap, cg = _tap_model(opt), U.build_gpu_model(opt, params, False)
    dev_v = [dict(c3d=torch.from_numpy(v['c3d']).to(_dev()), lda=torch.from_numpy(v['lda']).to(_dev()), duration=60.0) for v in videos]
    infos, ex = EU.caption_videos(tap, cg, dev_v, F2T, topN=8, nms_threshold=0.6)
    assert ex['batch'].one_stream and len(ex['kept']) >= 2          # (a video without an NMS candidate is dropped from the batch)
    for v, d in enumerate(dev_v):
        want, ex1 = EU.caption_video(tap, cg, d['c3d'], d['lda'], 60.0, F2T, topN=8, nms_threshold=0.6)
        assert [list(map(int, x)) for x in ex['per_video'][v]['soi_select_list']] == [list(map(int, x)) for x in ex1['soi_select_list']]
        if v in ex['kept']:
            _same_records(infos[v], want)
        else:
            assert infos[v] == [] and want == []


# ---- 9. the example driver -------------------------------------------------------------------------------------------------------------------
def test_example_driver_trains_over_batches():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import train_synthetic
    history, cg_model, _ = train_synthetic.main(['--caption_model', SAT, '--CG_input_feats_type', 'VEC', '--m_batch', '3', '--iters', '2',
                                                 '--events', '6', '--segments', '12', '--vocab', '60', '--quiet'])
    print('[example] mean cg_loss per batched iteration: %s' % ' '.join('%.4f' % x for x in history))
    assert cg_model.one_stream() and len(history) == 2 and all(np.isfinite(history))
    assert history[1] < history[0]

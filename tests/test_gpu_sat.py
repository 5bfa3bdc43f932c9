"""The one-stream decoder (caption_model='show_attend_tell', one LSTM layer: csrc/sat.hip, echr_amd/sat.py) on the GPU (-m gpu): training
and greedy evaluation of one video per call against the reference's own fixtures (tests/golden/case_sat_tiny.npz, case_sat.npz, written by
tools/make_golden_sat.py) and, on edge shapes, against tests/sat_ref.py carried in float64.

Gates.  The project's bounds (tests/test_gpu_parity.py header): log-probs and losses within 1e-4 relative of the reference, every gradient
within 1e-3 of its tensor's max-norm, indices exact -- greedy indices at the positions whose reference margin exceeds 1e-4 (at least 90 % of
a fixture's positions, asserted from the fixture: a condition on the inputs).  The gates below are ten times the noise measured on an
MI355X, as the three-stream gates were set, and never looser than those bounds.  Measured over every case of this file (two runs; every test
prints its figures ahead of its assertions) and by tools/parity_report.py --sat per variant: log-probs at most 2.7e-7 relative, losses
2.5e-7, the worst gradient tensor 4.4e-6 of its max-norm (the event encoder's pair_pos_fc1.weight; the decoder's own tensors stay below
2.2e-6), d tap_feats 1.2e-6; the float32 reference arithmetic itself sits at 1e-7 / 1.4e-7 / 1.4e-6 / 4.8e-7 against float64.
d alpha_net.bias is exactly zero in real arithmetic (tests/sat_ref.NOISE_ONLY): rounding noise on every side, held below 1e-6."""
import functools

import numpy as np
import pytest
import torch

from echr_amd import synth
from oracle import summary as SM
from tests import sat_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

TOL_LOGP, TOL_LOSS, TOL_GRAD = 3e-6, 3e-6, 5e-5          # 10 x (2.7e-7, 2.5e-7, 4.4e-6); the project's bounds are 1e-4, 1e-4, 1e-3
MARGIN = 1e-4
VARIANTS = ('sat_c', 'sat_e', 'sat_ve', 'sat_vec_init', 'sat_vec_eh')
ATT = ('ctx2att', 'h2att', 'alpha_net')
TINY = synth.SAT_CASES['sat_tiny']['opt']


def _dev():
    return torch.device('cuda')


def _feats(vid, tap_grad=False):
    tap, c3d, lda = (torch.from_numpy(np.ascontiguousarray(vid[k])).to(_dev()) for k in ('tap', 'c3d', 'lda'))
    return tap.requires_grad_(tap_grad), c3d, lda


def _run(opt, params, vid, train_mode, m=None):
    """forward(mode='train') + LanguageModelCriterion + backward: (log-probs, loss, parameter gradients, d tap_feats, module)."""
    from echr_amd.misc.utils import LanguageModelCriterion
    m = m if m is not None else U.build_gpu_model(opt, params, train_mode)
    tap, c3d, lda = _feats(vid, True)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    loss = LanguageModelCriterion()(pred, labels[:, 1:].to(_dev()), masks[:, 1:].to(_dev()))
    loss.backward()
    grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}
    g_tap = tap.grad.cpu().numpy() if tap.grad is not None else np.zeros(tuple(tap.shape), np.float32)
    torch.cuda.synchronize()
    return pred.detach().cpu().numpy(), float(loss.detach()), grads, g_tap, m


def _dead(opt):
    return 'C' not in opt.CG_input_feats_type


def _check_dead_attention(opt, grads):
    """Without 'C' the reference computes the attention and never reads it: no gradient there, exact zeros (or none) here."""
    for k, g in grads.items():
        if k.startswith('lm_model.core.') and any(a in k for a in ATT):
            assert g is None or not np.any(g), k


def _grad_err(name, got, ref):
    if name in R.NOISE_ONLY:
        assert float(np.abs(got).max()) < 1e-6 and float(np.abs(ref).max()) < 1e-6, name
        return 0.0
    return U.relerr(got, ref, U.GRAD_FLOOR)


def _check_against(tag, got, ref, opt):
    """Full tensors: (log-probs, loss, gradients, d tap) of the device against a reference run."""
    pred, loss, grads, g_tap = got[:4]
    rpred, rloss, rgrads, rg_tap = ref
    e_logp, e_loss = U.relerr(pred, rpred), abs(loss - rloss) / abs(rloss)
    errs = {}
    for k, g in rgrads.items():
        if g is None:
            assert grads[k] is None or not np.any(grads[k]), k
        else:
            errs[k] = _grad_err(k, grads[k], g)
    e_tap = U.relerr(g_tap, rg_tap, U.GRAD_FLOOR)
    worst = max(errs, key=errs.get)
    print('[%s] logp %.2e  loss %.2e  worst gradient %.2e (%s)  d tap %.2e' % (tag, e_logp, e_loss, errs[worst], worst, e_tap))
    if _dead(opt):
        _check_dead_attention(opt, grads)
    assert pred.shape == rpred.shape and e_logp < TOL_LOGP and e_loss < TOL_LOSS
    assert errs[worst] < TOL_GRAD and e_tap < TOL_GRAD


# ---- 1. the reference's fixtures --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('train_mode', [False, True], ids=['eval', 'train'])
def test_tiny_fixture_full_tensors(train_mode):
    g = U.gold('case_sat_tiny.npz')
    opt, params, vid = synth.make_sat_case('sat_tiny', video_seed=int(g['seed']))
    mode = 'train' if train_mode else 'eval'
    got = _run(opt, params, vid, train_mode)
    rgrads = {k: g.get(mode + '|grad|' + k) for k in params}
    _check_against('sat_tiny/' + mode, got, (g[mode + '|logp'], float(g[mode + '|loss']), rgrads, g[mode + '|gtap']), opt)
    assert np.abs(np.exp(got[0].astype(np.float64)).sum(2) - 1).max() < 1e-5


@pytest.mark.parametrize('name', VARIANTS)
@pytest.mark.parametrize('train_mode', [False, True], ids=['eval', 'train'])
def test_variant_summaries(name, train_mode):
    """log-probs (64 columns, top-1, arg-max), loss, every parameter gradient -- the event encoder's included -- and d tap_feats against the
    summaries of the reference's run."""
    g = U.gold('case_sat.npz')
    pre, mode = name + '|', 'train' if train_mode else 'eval'
    opt, params, vid = synth.make_sat_case(name, video_seed=int(g[pre + 'seed']))
    pred, loss, grads, g_tap, m = _run(opt, params, vid, train_mode)
    key = pre + mode
    s = SM.summarize_logp(pred)
    e_logp = max(U.relerr(s['slice'], g[key + '|logp|slice']), U.relerr(s['top1'], g[key + '|logp|top1']))
    e_loss = abs(loss - float(g[key + '|loss'])) / abs(float(g[key + '|loss']))
    safe = g[key + '|logp|margin'] > MARGIN
    errs = {}
    for k, v in SM.summarize_grads(dict(grads, tap=g_tap)).items():
        pname, part = k.split('|')
        base = key + ('|gtap|' if pname == 'tap' else '|grad|' + pname + '|')
        if base + part not in g:
            assert pname != 'tap' and not np.any(grads[pname]), k          # no gradient in the reference: none, or exact zeros, here
            continue
        ref = g[base + part]
        if pname in R.NOISE_ONLY:
            assert float(np.abs(v).max()) < 1e-6 and float(np.abs(ref).max()) < 1e-6, k
            continue
        scale = max(float(g[base + 'linf']), U.GRAD_FLOOR)
        errs[k] = float(np.abs(np.asarray(v, np.float64) - ref).max()) / (max(abs(float(ref)), U.GRAD_FLOOR) if part in ('l2', 'linf') else scale)
    missing = [k for k in g if k.startswith(key + '|grad|') and k.split('|')[3] not in grads]
    worst = max(errs, key=errs.get)
    print('[%s/%s] logp %.2e  loss %.2e  worst gradient summary %.2e (%s)' % (name, mode, e_logp, e_loss, errs[worst], worst))
    assert not missing, missing
    if _dead(opt):
        _check_dead_attention(opt, grads)
    assert e_logp < TOL_LOGP and e_loss < TOL_LOSS and errs[worst] < TOL_GRAD
    assert np.array_equal(s['argmax'][safe], g[key + '|logp|argmax'][safe])


@pytest.mark.parametrize('name', ('sat_tiny',) + VARIANTS)
def test_greedy_decode_matches_reference(name):
    g = U.gold('case_sat_tiny.npz' if name == 'sat_tiny' else 'case_sat.npz')
    pre = '' if name == 'sat_tiny' else name + '|'
    opt, params, vid = synth.make_sat_case(name, video_seed=int(g[pre + 'seed']))
    m = U.build_gpu_model(opt, params, False)
    tap, c3d, lda = _feats(vid)
    with torch.no_grad():
        seq, lp = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
    ok = g[pre + 'sample|margin'] > MARGIN
    assert ok.mean() >= 0.9          # (the generator's condition on the inputs)
    assert seq.dtype == torch.int64 and tuple(seq.shape) == g[pre + 'sample|seq'].shape
    e = U.relerr(lp.cpu().numpy()[ok], g[pre + 'sample|logp'][ok])
    print('[%s/sample] %s, resolvable %.3f, logp %.2e' % (name, tuple(seq.shape), ok.mean(), e))
    assert np.array_equal(seq.cpu().numpy()[ok], g[pre + 'sample|seq'][ok]) and e < TOL_LOGP


# ---- 2. edge shapes against the float64 reference arithmetic -------------------------------------------------------------------------------
def _edge_case(feats, N=3, A=7, L=7, seed=301, vocab=30, widths=TINY, lens=None, disjoint=False, cap=None, opt_over=None, T_v=None):
    o = dict(widths, CG_input_feats_type=feats, CG_vocab_size=vocab, CG_seq_length=L - 2)
    o.update(opt_over or {})
    opt = synth.default_opt(**o)
    vid = synth.make_video(N=N, A=A, L=L, V1=vocab + 1, seed=seed, video_dim=opt.video_dim, hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim,
                           disjoint=disjoint, T_v=T_v, min_len=min(4, A))
    if lens is not None:          # the first events get these lengths
        ln = np.asarray(lens, np.int64)
        soi = vid['soi']
        soi[:len(ln), 0] = np.minimum(soi[:len(ln), 0], vid['T_v'] - ln)
        soi[:len(ln), 1] = soi[:len(ln), 0] + ln
        vid['ind'] = (soi[:, 1] - 1).astype(np.int64)
    if cap is not None:           # no caption longer than `cap` words: the label columns behind are all zero
        vid['labels'][:, 1 + cap:] = 0
        vid['masks'][:] = 0
        for i, row in enumerate(vid['labels']):
            vid['masks'][i, :int((row != 0).sum()) + 2] = 1.0
    return opt, synth.make_sat_params(opt, 0), vid


ECHR_WIDTHS = dict(caption_model='show_attend_tell', CG_num_layers=1)          # default_opt's: H = E = Ha = 512, D = 500 (K = 1012)
EDGES = {
    'n1': dict(N=1),
    'n65': dict(N=65, seed=302),
    'lens_a7': dict(N=6, A=7, lens=(1, 2, 7, 1), seed=303),
    'lens_a129': dict(N=5, A=129, lens=(1, 2, 129), seed=304),
    'disjoint': dict(N=4, A=5, disjoint=True, seed=305),
    'echr_widths': dict(N=3, A=9, L=5, widths=ECHR_WIDTHS, seed=306),
    'v5001': dict(N=2, A=7, L=5, vocab=5000, seed=307),
    'early_stop': dict(N=5, A=7, L=9, cap=2, seed=308),
    # lda_dim = 10: with 'VEC' the event and attended-clip columns of W_ih start at E + 10 and E + 42 and its rows are 78 floats apart -- the
    # cell kernels' scalar panel loads and the unaligned operands / outputs of the products and the scene-row product around them
    'unaligned': dict(N=5, A=7, seed=310, opt_over=dict(lda_dim=10)),
    'init_c': dict(N=4, A=7, seed=309, opt_over=dict(CG_init_feats_type='C', video_context_type='VC', event_context_type='EC')),
}


@pytest.mark.parametrize('feats', ['VEC', 'C'])
@pytest.mark.parametrize('edge', sorted(EDGES))
def test_edge_shapes_against_float64(edge, feats):
    opt, params, vid = _edge_case(feats, **EDGES[edge])
    if edge == 'early_stop':
        assert R.O.n_decoder_steps(vid['labels']) == 3 < vid['labels'].shape[1] - 1
    if edge.startswith('lens'):
        ln = vid['soi'][:, 1] - vid['soi'][:, 0]
        assert {1, 2, EDGES[edge]['A']} <= set(ln.tolist())
    from echr_amd import functional as EF
    assert EF.rows_disjoint(vid['soi']) == (edge in ('disjoint', 'n1'))          # every other case has events that share rows (rows_disjoint = 0)
    for train_mode in (False, True):
        ref = R.run(opt, params, vid, train_mode, dtype=torch.float64)
        _check_against('%s/%s/%s' % (edge, feats, 'train' if train_mode else 'eval'), _run(opt, params, vid, train_mode), ref, opt)


@pytest.mark.parametrize('feats,seed', [('VEC', 222), ('C', 221)])
def test_greedy_captions_that_end_at_different_steps(feats, seed):
    """A token-driven model (embedding x 10, the <eos> row of the logit layer x 2.5) whose rows finish at three or more different steps, one
    of them at its first word: seq is zero behind a row's end, the log-probs keep the raw arg-max values, the width is the reference's."""
    opt, params, vid = _edge_case(feats, N=8, A=7, L=8, seed=seed)
    params['lm_model.embed.weight'] = params['lm_model.embed.weight'] * np.float32(10.0)
    params['lm_model.logit.weight'][0] *= np.float32(2.5)
    margins = []
    rseq, rlp = R.sample(opt, params, vid, torch.float64, margins)
    rseq, rlp = rseq.numpy(), rlp.numpy()
    lens = {int((r != 0).sum()) for r in rseq}
    assert len(lens) >= 3 and 0 in lens and float(np.min(np.stack(margins))) > 1e-3          # (conditions on the inputs)
    m = U.build_gpu_model(opt, params, False)
    tap, c3d, lda = _feats(vid)
    with torch.no_grad():
        seq, lp = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
    e = U.relerr(lp.cpu().numpy(), rlp)
    print('[eos/%s] %s lengths %s logp %.2e' % (feats, tuple(seq.shape), sorted(lens), e))
    assert np.array_equal(seq.cpu().numpy(), rseq) and e < TOL_LOGP


# ---- 3. one step at a time ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['sat_tiny', 'sat_vec_init'])
def test_get_logprobs_state_chain_reproduces_forward(name):
    """get_logprobs_state over the S steps of the teacher-forced tokens in eval mode: forward's log-probs, and the UNDROPPED (h, c) of the
    reference arithmetic at every step."""
    opt, params, vid = synth.make_sat_case(name)
    m = U.build_gpu_model(opt, params, False)
    tap, c3d, lda = _feats(vid)
    labels = torch.from_numpy(vid['labels'])
    states = []
    P, rtap, rc3d, rlda = R.leaves(params, vid, torch.float64, False)
    with torch.no_grad():
        video, event, clip, mask = R.contexts(opt, P, rtap, rc3d, rlda, vid['ind'], vid['soi'])
        rpred = R.decoder_forward(P, video, event, clip, mask, labels, opt.CG_input_feats_type, None, opt.CG_init_feats_type, states).numpy()
        pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
        ev = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'])
        vd = m.get_video_context(tap, c3d, lda, vid['ind'], vid['soi'])
        cl, cm = m.get_clip_context(tap, c3d, lda, vid['ind'], vid['soi'])
        lm = m.lm_model
        state = lm.init_hidden(vd, ev, cl, cm)
        assert tuple(state[0].shape) == (1, len(vid['soi']), opt.CG_rnn_size)
        worst = 0.0
        for t in range(pred.shape[1]):
            lp, state = lm.get_logprobs_state(labels[:, t].to(_dev()), vd, ev, cl, cm, state)
            assert torch.equal(lp, pred[:, t]) or U.relerr(lp.cpu().numpy(), pred[:, t].cpu().numpy()) < 1e-6
            worst = max(worst, U.relerr(lp.cpu().numpy(), rpred[:, t]), U.relerr(state[0].cpu().numpy(), states[t][0].numpy()),
                        U.relerr(state[1].cpu().numpy(), states[t][1].numpy()))
    print('[step chain/%s] worst of logp, h, c against float64: %.2e' % (name, worst))
    assert worst < 2e-5          # ten times the measured 1.5e-6 (the states h, c relative to their max-norm carry it; the log-probs stay at 2e-7)


def test_get_logprobs_state_in_training_mode_draws_one_stream_per_call():
    """Training mode: call i draws the output mask of step 0 under the call's own counter (offset OFFSET + i); the states stay undropped.
    Against the reference arithmetic in float64 fed those masks."""
    from echr_amd import philox
    opt, params, vid = synth.make_sat_case('sat_tiny')
    m = U.build_gpu_model(opt, params, True)          # (set_dropout_state(SEED, OFFSET))
    tap, c3d, lda = _feats(vid)
    labels = torch.from_numpy(vid['labels'])
    N, H = len(vid['soi']), opt.CG_rnn_size
    P, rtap, rc3d, rlda = R.leaves(params, vid, torch.float64, False)
    with torch.no_grad():
        m.eval()          # the contexts without the event encoder's dropout, on both sides
        ev = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'])
        vd = m.get_video_context(tap, c3d, lda, vid['ind'], vid['soi'])
        cl, cm = m.get_clip_context(tap, c3d, lda, vid['ind'], vid['soi'])
        m.train()
        video, event, clip, mask = R.contexts(opt, P, rtap, rc3d, rlda, vid['ind'], vid['soi'])
        lm = m.lm_model
        state, rstate = lm.init_hidden(vd, ev, cl, cm), R.init_hidden(P, video, event, clip, opt.CG_init_feats_type)
        worst, dropped = 0.0, 0
        for i in range(4):
            lp, state = lm.get_logprobs_state(labels[:, i].to(_dev()), vd, ev, cl, cm, state)
            dm = torch.from_numpy(philox.scale_mask((N, H), opt.CG_drop_prob, U.SEED, U.OFFSET + i, philox.SITE_OUT, 0)).double()
            dropped += int((dm == 0).sum())
            rlp, rstate = R.logprobs_state(P, labels[:, i], video, event, clip, mask, rstate, opt.CG_input_feats_type, dm)
            worst = max(worst, U.relerr(lp.cpu().numpy(), rlp.numpy()), U.relerr(state[0].cpu().numpy(), rstate[0].numpy()),
                        U.relerr(state[1].cpu().numpy(), rstate[1].numpy()))
    print('[step chain/train] worst of logp, h, c against float64: %.2e (%d of %d outputs dropped)' % (worst, dropped, 4 * N * H))
    assert 0 < dropped < 4 * N * H and worst < 2e-5          # (the eval chain's gate)


def test_example_driver_trains_the_one_stream_model():
    """examples/train_synthetic.py --caption_model show_attend_tell --CG_input_feats_type VEC: the plain autograd path, then a greedy decode."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import train_synthetic
    history, cg_model, _ = train_synthetic.main(['--caption_model', 'show_attend_tell', '--CG_input_feats_type', 'VEC', '--iters', '4', '--events', '6',
                                                 '--segments', '12', '--vocab', '60', '--quiet'])
    print('[example] cg_loss per iteration: %s' % ' '.join('%.3f' % x for x in history))
    assert cg_model.one_stream() and len(history) == 4 and all(np.isfinite(history))
    # the freshly initialised model is near uniform over the 61 words: logit weights within 0.1 on |h| < 1 keep its first loss within 0.5 of
    # log(61) (that the updates are right is test_two_iterations_with_arena_and_clamp_adam's; captions of random words cannot be learnt
    # across the driver's different videos, so no fall of the loss is asked for)
    assert abs(history[0] - np.log(61.0)) < 0.5
    torch.manual_seed(0)          # the driver's seed and construction order: these models hold its initial parameters
    import echr_amd
    echr_amd.models.setup_tap(cg_model.opt)
    fresh = echr_amd.CaptionGenerator(cg_model.opt).state_dict()
    moved = [k for k, v in cg_model.state_dict().items() if not torch.equal(v.cpu(), fresh[k])]
    assert 'fusion_model.h2a_layer.weight' not in moved          # (never used: no gradient, no update -- and the rebuilt model matches)
    assert 'lm_model.core.rnn.weight_hh_l0' in moved and 'lm_model.logit.weight' in moved and 'lm_model.embed.weight' in moved


# ---- 4. repeatability -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['sat_vec_init', 'sat_vec_eh'])
def test_eval_forward_and_greedy_decode_are_bitwise_repeatable(name):
    """Two eval forwards and two greedy decodes of the decoder on IDENTICAL inputs agree bit for bit (initial state included).  Through
    CaptionGenerator the event encoder runs again per call, and its split-K sums move the event context by an ulp (the note in
    tests/test_gpu_parity.py's greedy test): the whole call is compared bit for bit where there is no encoder ('EH'), and under the
    deterministic switch elsewhere (below)."""
    opt, params, vid = synth.make_sat_case(name)
    m = U.build_gpu_model(opt, params, False)
    tap, c3d, lda = _feats(vid)
    labels = torch.from_numpy(vid['labels'])
    with torch.no_grad():
        ev = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'])
        vd = m.get_video_context(tap, c3d, lda, vid['ind'], vid['soi'])
        cl, cm = m.get_clip_context(tap, c3d, lda, vid['ind'], vid['soi'])
        a, b = (m.lm_model(vd, ev, cl, cm, labels) for _ in range(2))
        (s1, l1), (s2, l2) = (m.lm_model.sample(vd, ev, cl, cm) for _ in range(2))
        assert torch.equal(a, b) and torch.equal(s1, s2) and torch.equal(l1, l2)
        if name == 'sat_vec_eh':
            a, b = (m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train') for _ in range(2))
            (s1, l1), (s2, l2) = (m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval') for _ in range(2))
            assert torch.equal(a, b) and torch.equal(s1, s2) and torch.equal(l1, l2)


@pytest.mark.parametrize('name', ['sat_vec_init', 'sat_c'])
def test_deterministic_training_iterations_agree_bit_for_bit(name):
    import echr_amd
    opt, params, vid = synth.make_sat_case(name)
    echr_amd.set_deterministic(True)
    try:
        runs = [_run(opt, params, vid, True) for _ in range(2)]
    finally:
        echr_amd.set_deterministic(False)
    (p1, l1, g1, t1, _), (p2, l2, g2, t2, _) = runs
    assert np.array_equal(p1, p2) and l1 == l2 and np.array_equal(t1, t2)
    for k in g1:
        assert (g1[k] is None and g2[k] is None) or np.array_equal(g1[k], g2[k]), k
    _check_against(name + '/deterministic', runs[0], R.run(opt, params, vid, True, dtype=torch.float64), opt)


# ---- 5. the arena and the fused optimiser -----------------------------------------------------------------------------------------------------
def test_two_iterations_with_arena_and_clamp_adam():
    """build_arena() + echr_amd.optim.ClampAdam over the one-stream model: the loss of the SECOND iteration against the reference arithmetic
    run with torch.optim.Adam and the same clamp (each iteration draws its own dropout stream: offsets OFFSET, OFFSET + 1)."""
    from echr_amd import philox
    from echr_amd.misc.utils import LanguageModelCriterion, clip_gradient
    from echr_amd.optim import ClampAdam
    opt, params, vid = synth.make_sat_case('sat_vec_eh')
    lr, clip = 1e-3, 0.05
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=lr, arena=m.build_arena())
    tap, c3d, lda = _feats(vid)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    losses = []
    for _ in range(2):
        o.zero_grad()
        loss = LanguageModelCriterion()(m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train'), labels[:, 1:].to(_dev()), masks[:, 1:].to(_dev()))
        loss.backward()
        clip_gradient(o, clip)
        o.step()
        losses.append(float(loss))
    # the reference arithmetic, float64, torch.optim.Adam
    P, rtap, rc3d, rlda = R.leaves(params, vid, torch.float64, True)
    rtap.requires_grad_(False)
    ro = torch.optim.Adam(list(P.values()), lr=lr, betas=(opt.optim_alpha, opt.optim_beta), eps=opt.optim_epsilon)
    rl = []
    for it in range(2):
        def drop(site, step, shape, it=it):
            s, p = dict(tsrm=(philox.SITE_TSRM, 0.3), out=(philox.SITE_OUT, opt.CG_drop_prob))[site]
            return torch.from_numpy(philox.scale_mask(tuple(shape), p, U.SEED, U.OFFSET + it, s, step))
        ro.zero_grad()
        video, event, clip_, mask = R.contexts(opt, P, rtap, rc3d, rlda, vid['ind'], vid['soi'], drop)
        logp = R.decoder_forward(P, video, event, clip_, mask, labels, opt.CG_input_feats_type, drop, opt.CG_init_feats_type)
        loss = R.O.lm_criterion(logp, labels[:, 1:], masks[:, 1:].double())
        loss.backward()
        for p in P.values():
            if p.grad is not None:
                p.grad.clamp_(-clip, clip)
        ro.step()
        rl.append(float(loss))
    e = [abs(a - b) / abs(b) for a, b in zip(losses, rl)]
    print('[arena + ClampAdam] losses %s against %s: %.2e, %.2e' % (losses, rl, e[0], e[1]))
    assert rl[1] < rl[0] and e[0] < TOL_LOSS and e[1] < TOL_LOSS

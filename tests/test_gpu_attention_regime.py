"""The decoder's additive attention at TRAINED-WEIGHT scales of alpha, p and q (-m gpu): every form of the chain against a FLOAT64 oracle.

Every other parity test feeds the attention freshly initialised weights (|p|, |q| ~ 1, sum|alpha| ~ 11, slot soft-max near uniform).  The
variants of synth.make_attsat move alpha_net, ctx2att, h2att to where the kernels behave differently:
  below / above      sum|alpha| = 39 / 41: both sides of the ALPHA_SAFE = 40 switch of the split soft-max (no shift / max exchange between the
                     three workgroups of an event), otherwise identical inputs; 'above64' is 'above' at the benchmarked shape
  alpha_big          sum|alpha| = 150 with ctx2att.bias = 2 sign(alpha): every score sits at +138..+142, exp() of an unshifted score overflows -- only an
                     exact shift gives finite weights ('alpha_big150': 150 events; 150, not more: 4 * e_ref must stay inside 1e-4)
  pq_wide            max|p| = 34, max|q| = 28, half of the large pairs of opposite sign: the factored tanh inside its domain at its worst conditioning
  pq_cross           p ~ +-60, q ~ -+50 on eight columns: OUTSIDE the domain of the factored tanh (|p|, |q| <= 43).  The library must say so (-EDOM through
                     the asynchronous check, naming the tensor) instead of returning tanh(10) = 0; the launch-per-phase forward is exact there
  short / short_big  'above' with events of 1, 2, 43, 44, 86, 87, 129 (130, 172, 173, 258) segments: thirds of an event that publish -inf

Gates.  For every variant e_ref = the error of the float32 oracle (the reference's arithmetic) against the float64 oracle on the same inputs,
measured on the CPU (tools/parity_report.py --attsat prints it); the gate of the HIP path against float64 is max(existing gate, 4 * e_ref), and
never above the 1e-4 contract for log-probs and loss.  4x: the HIP path rounds in the same precision but sums in another, partly atomic order
and uses the 1-ulp hardware exp / rcp.  e_ref, the larger of eval and train mode (log-probs absolute, loss relative, worst gradient tensor
relative to its max-norm):

  variant        logp      loss      grad    |  HIP path measured (persistent / launch-per-phase, worst of eval and train)
  below         7.9e-7    8.8e-9    1.0e-6   |  1.3e-6 / 1.3e-6   8.9e-8   1.1e-6
  above         8.3e-7    1.1e-7    8.5e-7   |  1.5e-6 / 1.4e-6   1.1e-7   9.6e-7
  above64       1.4e-6    1.4e-7    7.9e-7   |  2.4e-6 / 2.2e-6   8.8e-8   6.7e-7
  alpha_big     1.1e-5    1.7e-8    7.6e-6   |  5.7e-6 / 6.8e-6   6.6e-8   4.9e-6
  alpha_big150  1.3e-5    1.3e-7    6.2e-6   |  5.8e-6 (launch)   5.5e-8   3.8e-6
  pq_wide       7.7e-7    1.0e-7    2.3e-6   |  1.4e-6 / 1.3e-6   1.8e-8   2.0e-6
  short         1.0e-6    2.0e-8    1.1e-6   |  1.5e-6 / 1.4e-6   1.6e-7   1.0e-6
  short_big     1.3e-6    4.8e-8    1.0e-6   |  1.3e-6 / 1.2e-6   3.6e-8   1.7e-6

So 4 * e_ref stays at or below the existing gates (2e-5 / 1e-5 / 1e-5) everywhere except alpha_big / alpha_big150, whose scores of ~140 cost the
float32 reference itself 1e-5 (gates there: log-probs 4.4e-5 / 5.2e-5, gradients 3.0e-5 / 2.5e-5), and the
factored tanh costs nothing measurable at max|p| = 34: the HIP path sits within 2x of the reference's own rounding in every variant.

Sensitivity (scratch builds, arithmetic altered only): with the shift of the max-exchange branch replaced by 0 the persistent alpha_big cases fail (NaN);
with the domain report switched off -- the clamp as it was -- all four pq_cross cases fail."""
import functools

import numpy as np
import pytest
import torch

from echr_amd import synth
from tests import beam_ref, clipctx_ref as R, util as U

pytestmark = pytest.mark.gpu

TOL_LOGP, TOL_LOSS, TOL_GRAD = 2e-5, 1e-5, 1e-5          # the existing gates (tests/test_gpu_parity.py)
CONTRACT = 1e-4
# e_ref (logp absolute, loss relative, gradient relative to the tensor's max-norm): float32 oracle vs float64 oracle, CPU
E_REF = {
    'below': (7.9e-7, 8.8e-9, 1.0e-6), 'above': (8.3e-7, 1.1e-7, 8.5e-7), 'above64': (1.4e-6, 1.4e-7, 7.9e-7),
    'alpha_big': (1.1e-5, 1.7e-8, 7.6e-6), 'alpha_big150': (1.3e-5, 1.3e-7, 6.2e-6), 'pq_wide': (7.7e-7, 1.0e-7, 2.3e-6),
    'pq_cross': (6.2e-7, 6.3e-8, 7.8e-7), 'short': (1.0e-6, 2.0e-8, 1.1e-6), 'short_big': (1.3e-6, 4.8e-8, 1.0e-6),
}
IN_DOMAIN = ['below', 'above', 'above64', 'alpha_big', 'alpha_big150', 'pq_wide', 'short', 'short_big']


def gates(name):
    e = E_REF[name]
    g = (max(TOL_LOGP, 4 * e[0]), max(TOL_LOSS, 4 * e[1]), max(TOL_GRAD, 4 * e[2]))
    assert g[0] <= CONTRACT and g[1] <= CONTRACT
    return g


def _lib():
    from echr_amd import _lib as L
    return L, L.load()


def _config(pairs):
    L, lib = _lib()
    for k, v in pairs:
        L.check(lib.echr_config_set(k.encode(), int(v)), 'config_set')


@functools.lru_cache(maxsize=None)
def _oracle64(name, train_mode, clip='CC'):
    """(log-probs, loss, parameter gradients, d tap_feats) of the float64 oracle (tests/clipctx_ref.py composes the 'CC' clip too)."""
    opt, params, vid = synth.make_attsat(name, clip)
    return R.run(opt, params, vid, train_mode, dtype=torch.float64)


def _check(name, got, ref, what=''):
    tl, ts, tg = gates(name)
    pred, loss, grads = got[:3]
    rp, rl, rg = ref[:3]
    assert pred.shape == rp.shape and np.isfinite(pred).all(), what
    e = float(np.abs(pred - rp).max())
    print('%s %s: max|d logp| %.3e (gate %.2e)  loss rel %.3e (gate %.2e)' % (name, what, e, tl, abs(loss - rl) / abs(rl), ts))
    worst = max((U.relerr(grads[k], g, U.GRAD_FLOOR), k) for k, g in rg.items() if g is not None and k not in U.NOISE_ONLY)
    print('%s %s: worst gradient %.3e of its max-norm (%s, gate %.2e)' % (name, what, worst[0], worst[1], tg))
    assert e < tl, (what, e)
    assert abs(loss - rl) < ts * abs(rl), (what, loss, rl)
    for k, g in rg.items():
        if g is None:
            assert grads[k] is None or not np.any(grads[k]), k
        else:
            assert U.grad_close(k, grads[k], g, tg), (what, k, U.relerr(grads[k], g))


def _drain():
    """Leave no asynchronous report behind for the next test."""
    _, lib = _lib()
    torch.cuda.synchronize()
    while lib.echr_check_async() != 0:
        pass


@pytest.mark.parametrize('persist', [1, 0])
@pytest.mark.parametrize('train_mode', [False, True])
@pytest.mark.parametrize('name', IN_DOMAIN)
def test_module_path_vs_float64_oracle(name, train_mode, persist):
    """CaptionGenerator(mode='train') + criterion + backward, eval and train mode (the oracle gets the same dropout masks): every log-prob, the loss,
    every gradient element against float64 -- persistent recurrences and launch-per-phase."""
    _, lib = _lib()
    opt, params, vid = synth.make_attsat(name)
    try:
        _config([('persist', persist), ('persist_bwd', persist)])
        got = U.run_gpu(opt, params, vid, train_mode)
    finally:
        _config([('persist', 1), ('persist_bwd', 1)])
    assert lib.echr_check_async() == 0, lib.echr_last_error()
    _check(name, got, _oracle64(name, train_mode), 'module path persist=%d train=%d' % (persist, train_mode))


@pytest.mark.parametrize('train_mode', [False, True])
@pytest.mark.parametrize('name', ['above', 'pq_wide'])
def test_module_path_vs_reference_fixture(name, train_mode):
    """The same against what the reference's own CPU code produced (tests/golden/case_attsat.npz, tools/make_golden.py do_attsat): float32
    summaries, therefore held to the existing gates plus nothing."""
    from oracle import summary as SM
    g = U.gold('case_attsat.npz')
    tag = name + ('|train' if train_mode else '|eval')
    opt, params, vid = synth.make_attsat(name)
    pred, loss, grads, _ = U.run_gpu(opt, params, vid, train_mode)
    tl, ts, tg = gates(name)
    assert abs(loss - float(g[tag + '|loss'])) < ts * abs(float(g[tag + '|loss']))
    s = SM.summarize_logp(pred)
    assert np.abs(s['slice'] - g[tag + '|logp|slice']).max() < tl and np.abs(s['top1'] - g[tag + '|logp|top1']).max() < tl
    safe = g[tag + '|logp|margin'] > 1e-4
    assert np.array_equal(s['argmax'][safe], g[tag + '|logp|argmax'][safe])
    for key, v in SM.summarize_grads(grads).items():
        ref = g[tag + '|grad|' + key]
        pname = key.split('|')[0]
        if pname in U.NOISE_ONLY:
            assert np.abs(np.asarray(v)).max() < 1e-6 and np.abs(np.asarray(ref)).max() < 1e-6, key
            continue
        scale = max(float(g[tag + '|grad|' + pname + '|linf']), U.GRAD_FLOOR)
        if key.endswith('|l2') or key.endswith('|linf'):
            assert abs(float(v) - float(ref)) < tg * max(abs(float(ref)), U.GRAD_FLOOR), (key, float(v), float(ref))
        else:
            assert np.abs(v - ref).max() < tg * scale, (key, np.abs(v - ref).max() / scale)


def _forward_branch(name):
    L, lib = _lib()
    opt, params, vid = synth.make_attsat(name)
    with torch.no_grad():
        pred = U.run_gpu(opt, params, vid, False, backward=False)[0]
    assert lib.echr_check_async() == 0
    return pred, lib.echr_persist_softmax_branch()


def test_below_and_above_take_different_softmax_branches():
    """The two cases differ by the scale of alpha_net alone; the library reports which soft-max branch the persistent forward launch took
    (echr_persist_softmax_branch: 1 no shift, 2 max exchange).  Also the decoding kernel's copy of the switch."""
    _, lib = _lib()
    pb, bb = _forward_branch('below')
    pa, ba = _forward_branch('above')
    assert (bb, ba) == (1, 2), (bb, ba)
    assert _forward_branch('alpha_big')[1] == 2 and _forward_branch('pq_wide')[1] == 1
    for name, want in (('below', 1), ('above', 2)):
        opt, params, vid = synth.make_attsat(name)
        m = U.build_gpu_model(opt, params, False)
        dev = torch.device('cuda')
        with torch.no_grad():
            m(*(torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda')), [], vid['ind'], vid['soi'], mode='eval')
        torch.cuda.synchronize()
        assert lib.echr_persist_softmax_branch() == want, name


@pytest.mark.parametrize('name', ['below', 'above'])
def test_cooperative_launch_vs_float64_oracle(name):
    _, lib = _lib()
    opt, params, vid = synth.make_attsat(name)
    try:
        _config([('persist_coop', 1)])
        got = U.run_gpu(opt, params, vid, True)
    finally:
        _config([('persist_coop', 0)])
    assert lib.echr_check_async() == 0
    _check(name, got, _oracle64(name, True), 'persist_coop')


@pytest.mark.parametrize('name', ['above', 'alpha_big', 'pq_wide'])
def test_one_call_path_vs_float64_oracle(name):
    """fused.FusedTrainStep (echr_train_step) with step=False: loss and every gradient, train mode."""
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    opt, params, vid = synth.make_attsat(name)
    rp, rl, rg, _ = _oracle64(name, True)
    dev = torch.device('cuda')
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
    f = FusedTrainStep(m, o, grad_clip=None)
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    loss = float(f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], step=False))
    torch.cuda.synchronize()
    assert _lib()[1].echr_check_async() == 0
    _, ts, tg = gates(name)
    print('%s one-call: loss rel %.3e' % (name, abs(loss - rl) / abs(rl)))
    assert abs(loss - rl) < ts * abs(rl), (loss, rl)
    grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}
    for k, g in rg.items():
        if g is None:
            assert grads[k] is None or not np.any(grads[k]), k
        else:
            assert U.grad_close(k, grads[k], g, tg), (k, U.relerr(grads[k], g))


def test_deterministic_mode_on_above():
    """Fixed-order mode: two runs bit-identical, and inside the gates of the default mode."""
    import echr_amd
    opt, params, vid = synth.make_attsat('above')
    echr_amd.set_deterministic(True)
    try:
        a = U.run_gpu(opt, params, vid, True)
        b = U.run_gpu(opt, params, vid, True)
    finally:
        echr_amd.set_deterministic(False)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    for k, v in a[2].items():
        assert (v is None and b[2][k] is None) or np.array_equal(v, b[2][k]), k
    _check('above', a, _oracle64('above', True), 'deterministic')


# ---- decoding --------------------------------------------------------------------------------------------------------------------------
MAX_EXCLUDED = 0.02          # share of positions a case may leave uncompared because the float64 oracle itself cannot resolve them


def _contexts64(opt, params, vid):
    P = {k: torch.from_numpy(v.copy()).double() for k, v in params.items()}
    tap, c3d, lda = (torch.from_numpy(vid[k]).double() for k in ('tap', 'c3d', 'lda'))
    with torch.no_grad():
        return (P,) + tuple(R.contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi']))


def _greedy64(opt, params, vid):
    """oracle.decoder_sample in float64, with the top-1 margin of every emitted position."""
    from oracle import echr_ref_cpu as O
    P, video, event, cl, mask = _contexts64(opt, params, vid)
    N = event.shape[0]
    state = O.init_hidden(P, video, event, cl, opt.CG_init_feats_type)
    seq, slp, mar = [], [], []
    logprobs = unfinished = None
    with torch.no_grad():
        for t in range(opt.CG_seq_length + 1):
            if t == 0:
                it = torch.zeros(N, dtype=torch.long)
            else:
                top = logprobs.topk(2, dim=1)
                sample_lp, it, margin = top.values[:, 0], top.indices[:, 0], top.values[:, 0] - top.values[:, 1]
            logprobs, state = O.logprobs_state(P, it, video, event, cl, mask, state)
            if t >= 1:
                unfinished = (it > 0) if t == 1 else unfinished & (it > 0)
                if int(unfinished.sum()) == 0:
                    break
                seq.append(it * unfinished.type_as(it)); slp.append(sample_lp); mar.append(margin)
    return torch.stack(seq, 1).numpy(), torch.stack(slp, 1).numpy(), torch.stack(mar, 1).numpy()


@pytest.mark.parametrize('persist_sample', [1, 0])
@pytest.mark.parametrize('name', ['above', 'pq_wide', 'alpha_big150'])
def test_greedy_decoding_vs_float64_oracle(name, persist_sample):
    """mode='eval': the sequence equals the float64 oracle's up to each row's first position whose top-1 margin is below the log-prob gate (from
    there on the row may legitimately differ and is not compared); log-probs of the compared positions within the gate."""
    opt, params, vid = synth.make_attsat(name)
    rseq, rlp, margin = _greedy64(opt, params, vid)
    tl = gates(name)[0]
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    try:
        _config([('persist_sample', persist_sample)])
        with torch.no_grad():
            seq, lp = m(*(torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda')), [], vid['ind'], vid['soi'], mode='eval')
    finally:
        _config([('persist_sample', 1)])
    seq, lp = seq.cpu().numpy(), lp.cpu().numpy()
    safe = np.logical_and.accumulate(margin > tl, axis=1)          # a row is compared up to its first unresolvable position
    excluded = 1.0 - safe.mean()
    print('%s greedy persist_sample=%d: %.2f%% of %d positions excluded, min margin %.2e' % (name, persist_sample, 100 * excluded, safe.size, margin.min()))
    assert excluded <= MAX_EXCLUDED
    if safe.all():
        assert seq.shape == rseq.shape
    T = min(seq.shape[1], rseq.shape[1])
    assert T >= 1
    assert np.array_equal(seq[:, :T][safe[:, :T]], rseq[:, :T][safe[:, :T]])
    assert np.abs(lp[:, :T][safe[:, :T]] - rlp[:, :T][safe[:, :T]]).max() < tl


@pytest.mark.parametrize('gemm_h2', [1, 0])
@pytest.mark.parametrize('name', ['above', 'pq_wide'])
def test_beam_decoding_vs_float64_oracle(name, gemm_h2):
    """beam_size = 3 against the host beam search (tests/beam_ref.py) over the float64 oracle.  An event is compared when its oracle margin (smallest gap
    between a kept and a dropped candidate, or between the result and the runner-up) exceeds the log-prob gate (the float32 oracle agrees with the
    float64 one on every such event of both cases, with nothing excluded: checked on the CPU); a hypothesis score is a sum of up to seq_length
    log-probs, each within the gate."""
    opt, params, vid = synth.make_attsat(name)
    B, L = 3, opt.CG_seq_length
    tl = gates(name)[0]
    from oracle import echr_ref_cpu as O
    P, video, event, cl, mask = _contexts64(opt, params, vid)
    state0 = O.init_hidden(P, video, event, cl, opt.CG_init_feats_type)
    step, rep_state = beam_ref.oracle_step(P, video, event, cl, mask, B)
    ref = beam_ref.beam_search(step, rep_state(state0), event.shape[0], B, L)
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    try:
        _config([('gemm_h2', gemm_h2)])
        with torch.no_grad():
            seq, lp, score = m(*(torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda')), [], vid['ind'], vid['soi'], mode='eval', beam_size=B, return_score=True)
    finally:
        _config([('gemm_h2', 1)])
    seq, lp, score = seq.cpu().numpy(), lp.cpu().numpy(), score.cpu().numpy()
    gated = ref['margin'] > tl
    words = ref['words']
    excluded = float(((~gated) * np.minimum(words + 1, L)).sum()) / float(np.minimum(words + 1, L).sum())
    print('%s beam gemm_h2=%d: %.2f%% of positions excluded, min margin %.2e' % (name, gemm_h2, 100 * excluded, ref['margin'].min()))
    assert excluded <= MAX_EXCLUDED
    pad = lambda x: np.concatenate([x, np.zeros((x.shape[0], L - x.shape[1]), x.dtype)], 1)
    assert np.array_equal(pad(seq)[gated], pad(ref['seq'])[gated])
    Tm = min(ref['seq'].shape[1], seq.shape[1])
    for n in np.nonzero(gated)[0]:
        k = min(int(words[n]) + 1, Tm)
        assert np.abs(lp[n, :k] - ref['logp'][n, :k]).max(initial=0.0) < tl, n
        assert abs(float(score[n]) - float(ref['score'][n])) < L * tl, n


@pytest.mark.parametrize('name', ['above', 'pq_wide'])
def test_single_steps_vs_float64_oracle(name):
    """lm_model.get_logprobs_state, three consecutive steps from the zero state: log-probs and both halves of the returned state (stream 1 is the
    LSTM fed by the attended context: the closest view of the slot weights the public API gives) against float64."""
    from oracle import echr_ref_cpu as O
    opt, params, vid = synth.make_attsat(name)
    P, video_r, event_r, cl_r, mask_r = _contexts64(opt, params, vid)
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels = torch.from_numpy(vid['labels'])
    tl = gates(name)[0]
    with torch.no_grad():
        video = m.get_video_context(tap, c3d, lda, vid['ind'], vid['soi'])
        event = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'])
        clip, cmask = m.get_clip_context(tap, c3d, lda, vid['ind'], vid['soi'])
        state = m.lm_model.init_hidden(video, event, clip)
        N, H = event.shape[0], opt.CG_rnn_size
        rstate = (torch.zeros(3, N, H, dtype=torch.float64), torch.zeros(3, N, H, dtype=torch.float64))
        for t in range(3):
            it = labels[:, t]
            logp, state = m.lm_model.get_logprobs_state(it.to(dev), video, event, clip, cmask, state)
            rlogp, rstate = O.logprobs_state(P, it, video_r, event_r, cl_r, mask_r, rstate)
            eh, ec = float((state[0].cpu().double() - rstate[0]).abs().max()), float((state[1].cpu().double() - rstate[1]).abs().max())
            print('%s step %d: logp %.3e  h %.3e  c %.3e  (stream 1: h %.3e)' % (name, t, float((logp.cpu().double() - rlogp).abs().max()), eh, ec,
                                                                            float((state[0][1].cpu().double() - rstate[0][1]).abs().max())))
            assert float((logp.cpu().double() - rlogp).abs().max()) < tl, t
            assert eh < 1e-5 and ec < 1e-5, t          # the gate test_get_logprobs_state_single_step_vs_oracle holds the state to


@pytest.mark.parametrize('clip', ['CH', 'CC+CH'])
@pytest.mark.parametrize('train_mode', [False, True])
def test_clip_contexts_on_above(clip, train_mode):
    """'CH' (D = 512: the persistent kernels, same body) and 'CC+CH' (D = 1012: launch-per-phase) with sum|alpha| = 41, incl. d tap_feats."""
    from echr_amd.misc.utils import LanguageModelCriterion
    _, lib = _lib()
    opt, params, vid = synth.make_attsat('above', clip)
    m = U.build_gpu_model(opt, params, train_mode)
    dev = torch.device('cuda')
    tap = torch.from_numpy(vid['tap']).to(dev).requires_grad_(True)
    c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('c3d', 'lda'))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    loss = LanguageModelCriterion()(pred, labels[:, 1:].cuda(), masks[:, 1:].cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert lib.echr_check_async() == 0
    if clip == 'CH':
        assert lib.echr_persist_softmax_branch() == 2
    grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}
    ref = _oracle64('above', train_mode, clip)
    _check('above', (pred.detach().cpu().numpy(), float(loss.detach()), grads), ref, clip)
    assert U.relerr(tap.grad.cpu().numpy(), ref[3]) < gates('above')[2]


# ---- outside the domain of the factored tanh -----------------------------------------------------------------------------------------------
def _expect_domain_report(lib, run):
    """`run` queues work that meets the out-of-domain arguments.  The report arrives once: either a later library call of `run` itself has
    already seen it (EchrHipError), or the check behind a synchronisation point returns it."""
    from echr_amd._lib import EchrHipError
    try:
        run()
        torch.cuda.synchronize()
        assert lib.echr_check_async() == -33
        msg = lib.echr_last_error().decode()
    except EchrHipError as e:
        msg = str(e)
        assert 'rc=-33' in msg, msg
    assert 'domain of the factored tanh' in msg and 'P_all' in msg and 'h2att' in msg, msg
    assert '|p| = 6' in msg and '|q| = 50' in msg, msg          # the magnitudes reached: p ~ 60..62, q ~ 50
    torch.cuda.synchronize()
    assert lib.echr_check_async() == 0                           # reported once


@pytest.mark.parametrize('form', ['persist_fwd', 'launch_fwd_persist_bwd', 'launch', 'greedy'])
def test_pq_cross_is_reported_not_hidden(form):
    """p ~ +-60 and q ~ -+50 on eight attention columns (p + q = +-10).  The factored form would give tanh = 0 there where tanh(+-10) = +-1, and
    1 - tanh^2 = 1 where it is 8e-9 (measured before the report existed: d ctx2att.weight off by 1.1x its max-norm, on every form, the
    log-probs untouched because the score error is the same for every slot of an event).  Every kernel that uses the form reports the argument
    (-EDOM, once, naming tensor and magnitude; the launch runs to its end); the launch-per-phase forward evaluates tanh(p + q) directly and is
    held to the float64 oracle here."""
    L, lib = _lib()
    opt, params, vid = synth.make_attsat('pq_cross')
    dev = torch.device('cuda')
    try:
        if form == 'persist_fwd':
            def run():
                with torch.no_grad():
                    U.run_gpu(opt, params, vid, False, backward=False)
            _expect_domain_report(lib, run)
            assert lib.echr_persist_softmax_branch() == 1
        elif form == 'greedy':
            m = U.build_gpu_model(opt, params, False)
            with pytest.raises(L.EchrHipError, match='domain of the factored tanh'):
                with torch.no_grad():
                    m(*(torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda')), [], vid['ind'], vid['soi'], mode='eval')
            assert lib.echr_check_async() == 0
        else:
            _config([('persist', 0), ('persist_bwd', 1 if form == 'launch_fwd_persist_bwd' else 0)])
            with torch.no_grad():
                pred = U.run_gpu(opt, params, vid, True, backward=False)[0]
            assert lib.echr_check_async() == 0                       # the exact forward has no such limit ...
            rp = _oracle64('pq_cross', True)[0]
            assert np.abs(pred - rp).max() < gates('pq_cross')[0]    # ... and is right
            _expect_domain_report(lib, lambda: U.run_gpu(opt, params, vid, True))          # its backward uses the factored form (reverse recurrence, d P_all pass)
    finally:
        _config([('persist', 1), ('persist_bwd', 1)])
        _drain()
    # the library is usable and clean afterwards
    opt, params, vid = synth.make_attsat('below')
    got = U.run_gpu(opt, params, vid, False)
    assert lib.echr_check_async() == 0
    _check('below', got, _oracle64('below', False), 'after the report')

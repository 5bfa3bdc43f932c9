"""Self-critical training on the GPU (-m gpu): CaptionGenerator.forward(mode='train_rl') + RewardCriterion and the one-call
SelfCriticalStep against the reference's own train_rl fixtures (tools/make_golden_scst.py), the training-mode sampled decode against
its teacher-forced recompute, and bitwise determinism with and without stage-ahead."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from echr_amd import synth
from tests import util as U

pytestmark = pytest.mark.gpu

TOL_LOSS = 1e-5     # relative (the train-mode fixture gates of tests/test_gpu_parity.py)
TOL_GRAD = 1e-5     # relative to the tensor's max-norm
TOL_LOGP = 1e-5
CASES = [('case_scst.npz', 'tiny'), ('case_scst_eos.npz', 'tiny_eos')]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_rl_mask = U.rl_mask


def _check_grads(named, ref):
    worst = 0.0
    for k, p in named:
        g = ref.get('grad|' + k)
        if g is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        if k.endswith('alpha_net.bias'):          # exactly zero in real arithmetic (softmax shift invariance): both sides are rounding noise
            assert float(p.grad.abs().max()) < 1e-6
            continue
        err = float(np.abs(p.grad.detach().cpu().numpy() - g).max() / max(float(np.abs(g).max()), 1e-5))
        worst = max(worst, err)
        assert err < TOL_GRAD, (k, err)
    return worst


def _inputs(vid):
    return tuple(torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))


@pytest.mark.parametrize('fixture,case', CASES)
def test_train_rl_module_path_matches_reference(fixture, case):
    from echr_amd.misc.utils import RewardCriterion
    ref = U.gold(fixture)
    opt, params, vid = synth.make_case(case)
    m = U.build_gpu_model(opt, params, True)
    tap, c3d, lda = _inputs(vid)
    gen, slp, greedy = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='train_rl', gen_result=torch.from_numpy(ref['gen_result']))
    assert gen.dtype == torch.int64 and slp.dtype == torch.float32 and tuple(slp.shape) == ref['gen_result'].shape
    assert torch.equal(gen.cpu(), torch.from_numpy(ref['gen_result']))
    if ref['greedy_res'].shape[1] == 0:
        assert isinstance(greedy, list) and greedy == []
    else:
        assert torch.equal(greedy.cpu(), torch.from_numpy(ref['greedy_res']))          # bit-exact
    mask = _rl_mask(ref['gen_result'])
    assert np.abs(slp.detach().cpu().numpy() - ref['sample_logprobs'])[mask].max() < TOL_LOGP
    loss = RewardCriterion()(slp, gen, torch.from_numpy(ref['reward']).cuda())
    assert abs(float(loss.detach()) - float(ref['loss'])) < TOL_LOSS * abs(float(ref['loss']))
    loss.backward()
    _check_grads(m.named_parameters(), ref)


@pytest.mark.parametrize('fixture,case', CASES)
def test_self_critical_step_matches_reference(fixture, case):
    from echr_amd.fused import FusedTrainStep, SelfCriticalStep
    from echr_amd.optim import ClampAdam
    ref = U.gold(fixture)
    opt, params, vid = synth.make_case(case)
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
    sc = SelfCriticalStep(FusedTrainStep(m, o))
    tap, c3d, lda = _inputs(vid)
    loss, gen, greedy, reward = sc(tap, c3d, lda, vid['ind'], vid['soi'], gen_result=ref['gen_result'], reward=ref['reward'], step=False)
    assert torch.equal(gen, torch.from_numpy(ref['gen_result']))
    assert tuple(greedy.shape) == ref['greedy_res'].shape and np.array_equal(greedy.numpy(), ref['greedy_res'])
    assert abs(float(loss) - float(ref['loss'])) < TOL_LOSS * abs(float(ref['loss']))
    _check_grads(m.named_parameters(), ref)


def test_module_path_and_one_call_path_agree_after_one_adam_step():
    from echr_amd.fused import FusedTrainStep, SelfCriticalStep
    from echr_amd.misc.utils import RewardCriterion, clip_gradient
    from echr_amd.optim import ClampAdam
    ref = U.gold('case_scst_eos.npz')
    opt, params, vid = synth.make_case('tiny_eos')
    tap, c3d, lda = _inputs(vid)
    lr = 1e-3
    ma = U.build_gpu_model(opt, params, True)
    oa = ClampAdam(ma.parameters(), lr=lr, arena=ma.build_arena())
    gen, slp, _ = ma(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='train_rl', gen_result=torch.from_numpy(ref['gen_result']))
    oa.zero_grad()
    la = RewardCriterion()(slp, gen, torch.from_numpy(ref['reward']).cuda())
    la.backward()
    clip_gradient(oa, 0.1)
    oa.step()
    mb = U.build_gpu_model(opt, params, True)
    ob = ClampAdam(mb.parameters(), lr=lr, arena=mb.build_arena())
    lb, _, _, _ = SelfCriticalStep(FusedTrainStep(mb, ob, grad_clip=0.1))(tap, c3d, lda, vid['ind'], vid['soi'], gen_result=ref['gen_result'],
                                                                         reward=ref['reward'])
    # the two losses sum the same signed terms in different orders (gathered [N,T] reduction vs fused per-row terms + fixed-order sum)
    assert abs(float(la.detach()) - float(lb)) < TOL_LOSS * abs(float(la.detach()))
    assert ob._flat['step'] == 1 and oa._flat['step'] == 1
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        if k.endswith('alpha_net.bias'):
            continue          # its gradient is exactly zero in real arithmetic: both updates are +-lr coin flips on rounding noise
        d = (pa.detach() - pb.detach()).abs()
        # Adam's first update is lr * g / (|g| + eps): equal where |g| is resolvable, a coin flip of +-lr where the gradient is rounding
        # noise -- a handful of elements at most, counted, not a fraction (small tensors)
        assert float(d.max()) <= 2.0 * lr * 1.001, k
        assert int((d > 1e-6).sum()) <= max(2, d.numel() // 100), (k, int((d > 1e-6).sum()), d.numel())


def _big_case():
    """Over SAMP_SLAB_ROWS (192) events: the sampler's per-step chain takes step_fwd_big (h2 products over the N rows)."""
    opt = synth.default_opt(vocab_size=5000, seq_length=9)
    params = synth.make_params(opt, 0)
    vid = synth.make_video(200, 24, 11, 5001, seed=17, T_v=512, video_dim=opt.video_dim, hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
    return opt, params, vid


@pytest.mark.parametrize('case', ['tiny_eos', 'c1', 'big'])
def test_sampled_decode_equals_teacher_forced_recompute(case):
    """The training-mode multinomial decode's emitted log-probs equal the teacher-forced pass under the same dropout state gathered at its own
    tokens (the dropout keying agrees step for step); a fixed seed reproduces the draws bit for bit.  'big' (200 events) runs the chain's
    many-event form (step_fwd_big)."""
    opt, params, vid = _big_case() if case == 'big' else synth.make_case(case)
    m = U.build_gpu_model(opt, params, True)
    tap, c3d, lda = _inputs(vid)
    lm = m.lm_model
    from echr_amd import functional as EF
    with torch.no_grad():
        ev = EF.event_index_tensors(vid['soi'], vid['ind'], c3d.device, min(c3d.shape[0], tap.shape[0]))
        drop = lm.next_drop_state(m.fusion_model.enc_attn.dropout.p)
        drop.training = True
        video = m.get_video_context(tap, c3d, lda, vid['ind'], vid['soi'])
        clip, cm = m.get_clip_context(tap, c3d, lda, vid['ind'], vid['soi'], _ev=ev)
        event = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'], _ev=ev, _drop=drop)
        gen, slp = lm.sample_train(video, event, clip, cm, drop, seed=1234)
        gen2, slp2 = lm.sample_train(video, event, clip, cm, drop, seed=1234)
        off = EF.DropState(drop.seed, drop.offset, False, drop.p_tsrm, drop.p_h, drop.p_out)
        gen_eval, _ = lm.sample_train(video, event, clip, cm, off, seed=1234)
        tf = lm.sequence_logprobs(video, event, clip, cm, gen, drop=drop)
    assert isinstance(gen, torch.Tensor) and gen.shape[1] > 0
    assert torch.equal(gen, gen2) and torch.equal(slp, slp2)
    mask = _rl_mask(gen.cpu().numpy())
    err = np.abs(slp.cpu().numpy() - tf.cpu().numpy())[mask].max()
    assert err < TOL_LOGP, err
    # dropout really is active in the draws: the same seed without it gives other log-probs
    if isinstance(gen_eval, torch.Tensor) and gen_eval.shape == gen.shape and torch.equal(gen_eval, gen):
        tf_eval = lm.sequence_logprobs(video, event, clip, cm, gen, drop=off)
        assert np.abs(tf_eval.detach().cpu().numpy() - tf.detach().cpu().numpy())[mask].max() > 1e-4


def test_deterministic_self_critical_steps_bitwise_with_and_without_stage_ahead(tmp_path):
    outs = {}
    for sa in ('1', '0'):
        out = str(tmp_path / ('sa%s.npz' % sa))
        env = dict(os.environ, ECHR_STAGE_AHEAD=sa)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'scst_worker.py'), out], env=env, cwd=ROOT, timeout=600,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[sa] = dict(np.load(out))
    a, b = outs['1'], outs['0']
    assert int(a['step']) == int(b['step']) == 3
    for k in ('gen', 'loss', 'p', 'm', 'v'):
        assert np.array_equal(a[k], b[k]), k


def _step_event_context(f):
    """The event context echr_train_step_rw recomputed, read from its workspace: the leading regions of csrc/step.hip's carve_step
    (index vectors incl. the weights | event-encoder input rows | event-encoder workspace | event context), each rounded up to 64 floats."""
    a, lib = f.a, f.lib
    up = lambda n: (n + 63) // 64 * 64
    N, S, t = a.dec.N, a.dec.S, a.tsrm
    off = up((3 + 5 * S) * N) + up(N * t.Din) + up(lib.echr_tsrm_ws_floats(t.N, t.Din, t.Df, t.Do, t.G))
    return f.ws[off:off + N * t.Do].view(N, t.Do)


@pytest.mark.parametrize('det', [False, True])
def test_step_recomputes_the_sampling_event_context(det):
    """The encoder inside echr_train_step_rw (same inputs, same dropout state) gives the event context the decodes read: within fp32 rounding,
    bitwise under set_deterministic(True)."""
    import echr_amd
    from echr_amd.fused import FusedTrainStep, SelfCriticalStep
    from echr_amd.optim import ClampAdam
    ref = U.gold('case_scst_eos.npz')
    opt, params, vid = synth.make_case('tiny_eos')
    tap, c3d, lda = _inputs(vid)
    echr_amd.set_deterministic(det)
    try:
        m = U.build_gpu_model(opt, params, True)
        o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
        sc = SelfCriticalStep(FusedTrainStep(m, o))
        sc(tap, c3d, lda, vid['ind'], vid['soi'], gen_result=ref['gen_result'], reward=ref['reward'], step=False)
        torch.cuda.synchronize()
        ev_sample, ev_step = sc.last_event, _step_event_context(sc.fused)
        if det:
            assert torch.equal(ev_sample, ev_step)
        else:
            assert float((ev_sample - ev_step).abs().max()) <= 1e-6 * float(ev_sample.abs().max())
    finally:
        echr_amd.set_deterministic(False)


def test_reward_weighted_step_takes_device_weights():
    """echr_train_step_rw with the criterion on the device (host_nll = 0, `weight` [N,S] in device memory) equals the host form; host_nll = 1
    together with a device `weight` is refused."""
    import ctypes as C
    from echr_amd import _lib as L
    from echr_amd.fused import FusedTrainStep, SelfCriticalStep
    from echr_amd.optim import ClampAdam
    ref = U.gold('case_scst_eos.npz')
    opt, params, vid = synth.make_case('tiny_eos')
    tap, c3d, lda = _inputs(vid)
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
    m.set_dropout_state(U.SEED, U.OFFSET)
    sc = SelfCriticalStep(FusedTrainStep(m, o))
    lh = float(sc(tap, c3d, lda, vid['ind'], vid['soi'], gen_result=ref['gen_result'], reward=ref['reward'], step=False)[0])
    f = sc.fused
    g_host = f.arena.flat_g.clone()
    a, lib = f.a, f.lib
    N, S = a.dec.N, a.dec.S
    gen = ref['gen_result']
    T = gen.shape[1]
    tgt = np.zeros((N, S), dtype=np.int32)
    tgt[:, :T] = gen
    mask = np.zeros((N, S), dtype=np.float32)
    mask[:, 0] = 1.0
    mask[:, 1:T] = gen[:, :T - 1] > 0
    w = np.zeros((N, S), dtype=np.float32)
    w[:, :T] = ref['reward'] * mask[:, :T]
    tgt_d, mask_d, w_d = (torch.from_numpy(x).cuda() for x in (tgt, mask, w))
    assert lib.echr_train_step_rw(C.byref(a), w_d.data_ptr(), L.stream_ptr()) != 0          # host_nll = 1 plus a device weight: refused
    a.host_nll, a.n_active = 0, 0
    a.nll_target, a.nll_target_i64, a.nll_mask = tgt_d.data_ptr(), 0, mask_d.data_ptr()
    L.check(lib.echr_train_step_rw(C.byref(a), w_d.data_ptr(), L.stream_ptr()), 'train_step_rw')
    torch.cuda.synchronize()
    ld = float(f.loss_ring[(f.calls - 1) % f.LOSS_SLOTS][0])
    assert abs(ld - lh) < TOL_LOSS * abs(lh) and abs(lh - float(ref['loss'])) < TOL_LOSS * abs(float(ref['loss']))
    g_dev = f.arena.flat_g
    for i, p in enumerate(f.arena.params):
        lo, n = f.arena.offsets[i], p.numel()
        gh, gd = g_host[lo:lo + n], g_dev[lo:lo + n]
        assert float((gh - gd).abs().max()) <= TOL_GRAD * max(float(gh.abs().max()), 1e-5) or float(gh.abs().max()) < 1e-6, i

"""Self-critical training over a multi-video batch on the GPU (-m gpu): CaptionGenerator.train_rl_batch + VideoBatch.reward_criterion and
the one-call SelfCriticalBatchStep against the reference's own per-video train_rl fixture (tools/make_golden_scst_batch.py), the batched
training-mode sampled decode against the single-video entry (bit for bit on a one-video batch: the one-launch multinomial step against
the slab-sum + draw pair) and against its teacher-forced recompute, the device's video_words, and the batch step against V single-video
SelfCriticalStep calls.

Gates: those of tests/test_gpu_scst.py -- 1e-5 relative on losses, 1e-5 on log-probs, 1e-5 of the tensor's max-norm on gradients, index
outputs bit-exact."""
import functools

import numpy as np
import pytest
import torch

from echr_amd import synth
from tests import scst_batch_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

TOL_LOSS = 1e-5
TOL_GRAD = 1e-5
TOL_LOGP = 1e-5
CASE = 'vbscst'


@functools.lru_cache(maxsize=None)
def _fixture():
    opt, params, videos = synth.make_vbatch(CASE)
    g = U.gold('case_scst_batch.npz')
    gens, slps, greedys, rewards, losses = R.load_fixture(g, len(videos))
    return dict(opt=opt, params=params, videos=videos, g=g, gens=gens, slps=slps, greedys=greedys, rewards=rewards, losses=losses,
                gen=R.stack(gens, videos, np.int64), reward=R.stack(rewards, videos, np.float32), widths=[x.shape[1] for x in gens])


def _batch(videos):
    from echr_amd.batch import VideoBatch
    return VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi')} for v in videos], device=torch.device('cuda'))


_rl_mask = U.rl_mask


def _check_grads(named, ref, tol=TOL_GRAD):
    for k, p in named:
        g = ref.get('grad|' + k)
        if g is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        if k.endswith('alpha_net.bias'):          # exactly zero in real arithmetic (softmax shift invariance): both sides are rounding noise
            assert float(p.grad.abs().max()) < 1e-6
            continue
        err = float(np.abs(p.grad.detach().cpu().numpy() - g).max() / max(float(np.abs(g).max()), 1e-5))
        assert err < tol, (k, err)


def _check_greedy(b, greedy, greedys):
    greedy = greedy.cpu().numpy() if isinstance(greedy, torch.Tensor) else np.zeros((b.n_events, 0), np.int64)
    for s, want in zip(b.event_slices, greedys):
        assert np.array_equal(greedy[s, :want.shape[1]], want) and not greedy[s, want.shape[1]:].any()          # bit-exact


def _fused(opt, params, lr=1e-3, clip=None):
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=lr, arena=m.build_arena())
    return m, o, FusedTrainStep(m, o, grad_clip=clip)


def _no_dropout(m):
    m.fusion_model.enc_attn.dropout.p = 0.0
    c = m.lm_model.core
    c.dropout0.p = c.dropout1.p = c.dropout2.p = 0.0
    m.lm_model.dropout.p = 0.0


# ---- the reference's fixture ------------------------------------------------------------------------------------------------------
def test_train_rl_batch_module_path_matches_reference():
    from echr_amd.misc.utils import RewardCriterion
    f = _fixture()
    m = U.build_gpu_model(f['opt'], f['params'], True)
    b = _batch(f['videos'])
    gen, slp, greedy, vw = m.train_rl_batch(b, gen_result=torch.from_numpy(f['gen']))
    assert gen.dtype == torch.int64 and slp.dtype == torch.float32 and tuple(slp.shape) == f['gen'].shape
    assert torch.equal(gen.cpu(), torch.from_numpy(f['gen']))
    assert vw.dtype == np.int64 and vw.tolist() == f['widths']
    _check_greedy(b, greedy, f['greedys'])
    got = slp.detach().cpu().numpy()
    for s, want, g in zip(b.event_slices, f['slps'], f['gens']):
        assert np.abs(got[s, :g.shape[1]] - want)[_rl_mask(g)].max() < TOL_LOGP
    total, per = b.reward_criterion(RewardCriterion(), slp, gen, f['reward'], vw)
    assert np.abs(per.detach().cpu().numpy() - f['losses']).max() < TOL_LOSS * np.abs(f['losses']).max()
    assert abs(float(total.detach()) - float(f['g']['loss'])) < TOL_LOSS * abs(float(f['g']['loss']))
    total.backward()
    _check_grads(m.named_parameters(), f['g'])


def test_self_critical_batch_step_matches_reference():
    from echr_amd.fused import SelfCriticalBatchStep
    f = _fixture()
    m, o, fs = _fused(f['opt'], f['params'])
    b = _batch(f['videos'])
    sc = SelfCriticalBatchStep(fs)
    loss, gen, greedy, reward, vw = sc(b, gen_result=f['gen'], reward=f['reward'], step=False)
    assert torch.equal(gen, torch.from_numpy(f['gen'])) and vw.tolist() == f['widths']
    assert tuple(reward.shape) == f['gen'].shape
    _check_greedy(b, greedy, f['greedys'])
    assert abs(float(loss) - float(f['g']['loss'])) < TOL_LOSS * abs(float(f['g']['loss']))
    per = sc.last_video_losses.cpu().numpy()
    assert np.abs(per - f['losses']).max() < TOL_LOSS * np.abs(f['losses']).max()
    assert fs.last_video_losses is sc.last_video_losses
    _check_grads(m.named_parameters(), f['g'])


def test_module_path_and_one_call_path_agree_after_one_adam_step():
    from echr_amd.fused import FusedTrainStep, SelfCriticalBatchStep
    from echr_amd.misc.utils import RewardCriterion, clip_gradient
    from echr_amd.optim import ClampAdam
    f = _fixture()
    lr = 1e-3
    b = _batch(f['videos'])
    ma = U.build_gpu_model(f['opt'], f['params'], True)
    oa = ClampAdam(ma.parameters(), lr=lr, arena=ma.build_arena())
    gen, slp, _, vw = ma.train_rl_batch(b, gen_result=torch.from_numpy(f['gen']))
    oa.zero_grad()
    la, _ = b.reward_criterion(RewardCriterion(), slp, gen, f['reward'], vw)
    la.backward()
    clip_gradient(oa, 0.1)
    oa.step()
    mb = U.build_gpu_model(f['opt'], f['params'], True)
    ob = ClampAdam(mb.parameters(), lr=lr, arena=mb.build_arena())
    lb = SelfCriticalBatchStep(FusedTrainStep(mb, ob, grad_clip=0.1))(b, gen_result=f['gen'], reward=f['reward'])[0]
    assert abs(float(la.detach()) - float(lb)) < TOL_LOSS * abs(float(la.detach()))
    assert ob._flat['step'] == 1 and oa._flat['step'] == 1
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        if k.endswith('alpha_net.bias'):
            continue          # its gradient is exactly zero in real arithmetic: both updates are +-lr coin flips on rounding noise
        d = (pa.detach() - pb.detach()).abs()
        # Adam's first update is lr * g / (|g| + eps): equal where |g| is resolvable, a coin flip of +-lr where the gradient is rounding
        # noise -- a handful of elements at most, counted, not a fraction (the rule of tests/test_gpu_scst.py)
        assert float(d.max()) <= 2.0 * lr * 1.001, k
        assert int((d > 1e-6).sum()) <= max(2, d.numel() // 100), (k, int((d > 1e-6).sum()), d.numel())


# ---- the batched sampled decode ---------------------------------------------------------------------------------------------------
def _one_video_case(name):
    if name in ('tiny_eos', 'c1'):
        return synth.make_case(name)
    V1, N, L = {'v301': (301, 12, 7), 'v12288': (12288, 3, 3), 'v12289': (12289, 3, 3)}[name]
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=L)
    vid = synth.make_video(N, 16, L + 2, V1, seed=77, T_v=64, video_dim=opt.video_dim, hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
    return opt, synth.make_params(opt, 0), vid


@pytest.mark.parametrize('case', ['tiny_eos', 'v301', 'c1', 'v12288', 'v12289'])
def test_one_video_batch_equals_the_single_video_decode_bitwise(case):
    """V1 = 31 / 301 / 5001 (the row in 8 / 8 / 20 registers per thread + LDS), 12 288 (48 per thread: the last on-chip vocabulary) and
    12 289 (streamed): tokens and emitted log-probs of echr_decoder_sample_train_batch on a one-video batch equal
    echr_decoder_sample_train's -- the one-launch multinomial step against the slab-sum + draw pair on the same logits."""
    from echr_amd import functional as EF
    opt, params, vid = _one_video_case(case)
    m = U.build_gpu_model(opt, params, True)
    tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
    lm = m.lm_model
    with torch.no_grad():
        ev = EF.event_index_tensors(vid['soi'], vid['ind'], c3d.device, min(c3d.shape[0], tap.shape[0]))
        drop = lm.next_drop_state(m.fusion_model.enc_attn.dropout.p)
        drop.training = True
        video = m.get_video_context(tap, c3d, lda, vid['ind'], vid['soi'])
        clip, cm = m.get_clip_context(tap, c3d, lda, vid['ind'], vid['soi'], _ev=ev)
        event = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'], _ev=ev, _drop=drop)
        gen, slp = lm.sample_train(video, event, clip, cm, drop, seed=1234)
        zero = torch.zeros(event.shape[0], dtype=torch.int32, device=event.device)
        gen_b, slp_b, vw = EF.sample_train_batch(video.reshape(1, -1), event, c3d, ev[0], ev[1], zero, ev[3], lm.seq_length, lm.native_params(),
                                                 drop, seed=1234)
    assert isinstance(gen, torch.Tensor) and gen.shape[1] > 0
    assert torch.equal(gen, gen_b) and torch.equal(slp, slp_b)
    assert vw.tolist() == [gen.shape[1]]


def _decode_case(name):
    if name == 'rows196':          # 49 videos x 4 events: at SAMP_SLAB_ROWS (192) and above the chain runs step_fwd_big on h2 operands
        opt = synth.default_opt(vocab_size=300, seq_length=7)
        vids = synth.make_vbatch_videos(49, (4, 4), (3, 30), (30, 80), (6, 9), 301, 1500, max_events=196, video_dim=opt.video_dim,
                                        hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
        return opt, synth.make_params(opt, 0), vids
    return synth.make_vbatch(name)


@pytest.mark.parametrize('case', ['vbctx', 'rows196', 'vb33'])
def test_batched_sampled_decode_equals_teacher_forced_recompute(case):
    """Dropout on: the log-probs the batched decode emits equal DecoderBatchFunction under the same drop state at the decode's own tokens,
    under the per-video masks; the same seed reproduces the draws bit for bit; video_words from the device are the host's widths.
    'vbctx': 5 videos incl. a one-event video, 'VLVCVH' scene vectors; 'rows196': step_fwd_big; 'vb33' (132 rows): the slab form."""
    from echr_amd import functional as EF
    opt, params, vids = _decode_case(case)
    m = U.build_gpu_model(opt, params, True)
    b = _batch(vids)
    lm = m.lm_model
    with torch.no_grad():
        video, event, ev_start, ev_len, A, vid, drop = m._batch_contexts(b, None)
        args = (video, event, b.c3d, ev_start, ev_len, vid, A, lm.seq_length, lm.native_params(), drop)
        gen, slp, vw = EF.sample_train_batch(*args, seed=1234)
        gen2, slp2, vw2 = EF.sample_train_batch(*args, seed=1234)
        assert isinstance(gen, torch.Tensor) and gen.shape[1] > 0
        N, T = gen.shape
        labels = torch.zeros(N, T + 2, dtype=torch.int64, device=gen.device)
        labels[:, 1:T + 1] = gen
        logp = EF.DecoderFunction.apply(video, event, b.c3d, ev_start, ev_len, lm._tokens(labels, b.device), A, EF.rows_disjoint(b.soi), drop,
                                        None, None, None, None, 0, vid, *lm.native_params())
        tf = EF.GatherTokens.apply(logp, gen)
    assert torch.equal(gen, gen2) and torch.equal(slp, slp2) and np.array_equal(vw, vw2)
    g = gen.cpu().numpy()
    assert np.array_equal(vw, b.caption_widths(g)) and T == int(vw.max())
    mask = _rl_mask(g, vw, b.vid)
    assert mask.any()
    err = np.abs(slp.cpu().numpy() - tf.cpu().numpy())[mask].max()
    assert err < TOL_LOGP, err


# ---- the batch step against V single-video steps ----------------------------------------------------------------------------------
def _single_video_sum(f, skip=()):
    """V single-video SelfCriticalStep(step=False) calls without dropout: (sum of losses, sum of flat gradients, per-video losses)."""
    from echr_amd.fused import SelfCriticalStep
    m, o, fs = _fused(f['opt'], f['params'])
    _no_dropout(m)
    sc = SelfCriticalStep(fs)
    total, flat, per = 0.0, torch.zeros_like(fs.arena.flat_g), []
    for v, vid in enumerate(f['videos']):
        if v in skip or f['gens'][v].shape[1] == 0:
            per.append(0.0)
            continue
        tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
        loss = sc(tap, c3d, lda, vid['ind'], vid['soi'], gen_result=f['gens'][v], reward=f['rewards'][v], step=False)[0]
        per.append(float(loss))
        total += float(loss)
        flat += fs.arena.flat_g
    return total, flat, np.asarray(per), fs.arena


def _check_flat(arena, got, want):
    for i, p in enumerate(arena.params):
        lo, n = arena.offsets[i], p.numel()
        a, r = got[lo:lo + n], want[lo:lo + n]
        scale = float(r.abs().max())
        assert float((a - r).abs().max()) <= TOL_GRAD * max(scale, 1e-5) or scale < 1e-6, (i, float((a - r).abs().max()), scale)


def test_batch_step_equals_the_sum_of_single_video_steps_without_dropout():
    from echr_amd.fused import SelfCriticalBatchStep
    f = _fixture()
    want_loss, want_flat, want_per, _ = _single_video_sum(f)
    m, o, fs = _fused(f['opt'], f['params'])
    _no_dropout(m)
    sc = SelfCriticalBatchStep(fs)
    loss = sc(_batch(f['videos']), gen_result=f['gen'], reward=f['reward'], step=False)[0]
    assert abs(float(loss) - want_loss) < TOL_LOSS * abs(want_loss)
    assert np.abs(sc.last_video_losses.cpu().numpy() - want_per).max() < TOL_LOSS * np.abs(want_per).max()
    _check_flat(fs.arena, fs.arena.flat_g, want_flat)


def test_width_zero_video_contributes_nothing():
    from echr_amd.fused import SelfCriticalBatchStep
    f = _fixture()
    dead = 2
    b = _batch(f['videos'])
    gen = f['gen'].copy()
    gen[b.event_slices[dead]] = 0
    m, o, fs = _fused(f['opt'], f['params'])
    _no_dropout(m)
    sc = SelfCriticalBatchStep(fs)
    loss, _, _, _, vw = sc(b, gen_result=gen, reward=f['reward'], step=False)
    assert vw[dead] == 0
    per = sc.last_video_losses.cpu().numpy()
    assert per[dead] == 0.0
    got = fs.arena.flat_g.clone()
    # the batch without that video (no dropout: the masks' batch-global keys do not matter)
    keep = [v for v in range(len(f['videos'])) if v != dead]
    b2 = _batch([f['videos'][v] for v in keep])
    m2, o2, fs2 = _fused(f['opt'], f['params'])
    _no_dropout(m2)
    sc2 = SelfCriticalBatchStep(fs2)
    rows = np.concatenate([np.arange(s.start, s.stop) for v, s in enumerate(b.event_slices) if v != dead])
    loss2 = sc2(b2, gen_result=gen[rows], reward=f['reward'][rows], step=False)[0]
    assert abs(float(loss) - float(loss2)) < TOL_LOSS * abs(float(loss2))
    assert np.abs(per[keep] - sc2.last_video_losses.cpu().numpy()).max() < TOL_LOSS * np.abs(per).max()
    _check_flat(fs.arena, got, fs2.arena.flat_g)
    # and against the single-video calls of the remaining videos
    want_loss, want_flat, _, _ = _single_video_sum(f, skip=(dead,))
    assert abs(float(loss) - want_loss) < TOL_LOSS * abs(want_loss)
    _check_flat(fs.arena, got, want_flat)
    with pytest.raises(ValueError):
        sc(b, gen_result=np.zeros_like(gen), reward=f['reward'], step=False)


def test_reward_fn_gets_each_video_at_its_own_widths():
    from echr_amd.fused import SelfCriticalBatchStep
    f = _fixture()
    b = _batch(f['videos'])
    gen = f['gen'].copy()
    gen[b.event_slices[3]] = 0
    seen = []

    def reward_fn(gen_v, greedy_v):
        seen.append((tuple(gen_v.shape), tuple(greedy_v.shape), gen_v.clone()))
        return np.full(gen_v.shape[0], 0.5, np.float32)
    m, o, fs = _fused(f['opt'], f['params'])
    loss, gen_h, greedy_h, reward, vw = SelfCriticalBatchStep(fs, reward_fn)(b, gen_result=gen, step=False)
    assert [s[0] for s in seen] == [(len(f['videos'][v]['soi']), f['widths'][v]) for v in range(3)]          # video 3 (width 0): not called
    assert [s[1] for s in seen] == [tuple(x.shape) for x in f['greedys'][:3]]
    for v in range(3):
        assert np.array_equal(seen[v][2].numpy(), f['gens'][v])
    r = reward.numpy()
    assert not r[b.event_slices[3]].any() and not r[b.event_slices[1], f['widths'][1]:].any() and (r[b.event_slices[0]] == 0.5).all()


def test_deterministic_batch_steps_are_bitwise():
    import echr_amd
    from echr_amd.fused import SelfCriticalBatchStep
    f = _fixture()
    echr_amd.set_deterministic(True)
    try:
        outs = []
        for _ in range(2):
            m, o, fs = _fused(f['opt'], f['params'], clip=0.1)
            sc = SelfCriticalBatchStep(fs, lambda gen_v, greedy_v: ((gen_v > 0).sum(1) - (greedy_v > 0).sum(1)).float() * 0.1 + 0.05)
            b = _batch(f['videos'])
            l1, g1 = sc(b)[:2]
            l2, g2 = sc(b)[:2]
            torch.cuda.synchronize()
            assert o._flat['step'] == 2
            outs.append((float(l1), float(l2), g1, g2, fs.arena.flat_p.clone(), o._flat['m'].clone(), o._flat['v'].clone()))
        a, c = outs
        assert a[0] == c[0] and a[1] == c[1] and torch.equal(a[2], c[2]) and torch.equal(a[3], c[3])
        for x, y in zip(a[4:], c[4:]):
            assert torch.equal(x, y)
    finally:
        echr_amd.set_deterministic(False)

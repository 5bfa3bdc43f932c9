"""Frame-level contexts 'CH' / 'CC+CH' on the GPU (-m gpu): the module path's log-probs, parameter gradients and d tap_feats against the CPU
oracle (tests/clipctx_ref.py) and the reference's fixtures, the persistent kernels at D = 512, fixed-order determinism on overlapping
events, greedy / beam decoding, caption_video, and the one-call steps (FusedTrainStep, JointTrainStep, SelfCriticalStep)."""
import numpy as np
import pytest
import torch

from echr_amd import synth
from tests import clipctx_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

TOL_LOGP = 2e-5
TOL_LOSS = 1e-5
TOL_GRAD = 1e-5
CASES = [('case_ch.npz', 'ch'), ('case_cch.npz', 'cch')]


def _inputs(vid, tap_grad=True):
    dev = torch.device('cuda')
    tap = torch.from_numpy(vid['tap']).to(dev).requires_grad_(tap_grad)
    c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('c3d', 'lda'))
    return tap, c3d, lda


def _module_pass(opt, params, vid, train_mode, arena=False):
    """CaptionGenerator.forward(mode='train') + LanguageModelCriterion + backward with tap_feats as a leaf."""
    from echr_amd.misc.utils import LanguageModelCriterion
    m = U.build_gpu_model(opt, params, train_mode)
    if arena:
        m.build_arena()
    tap, c3d, lda = _inputs(vid)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    loss = LanguageModelCriterion()(pred, labels[:, 1:].cuda(), masks[:, 1:].cuda())
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}
    return pred.detach().cpu().numpy(), float(loss.detach()), grads, tap.grad.detach().cpu().numpy(), m


def _check_vs_oracle(opt, params, vid, train_mode, got, ltol=TOL_LOSS):
    logp, loss, grads, g_tap = got[:4]
    rlogp, rloss, rgrads, rg_tap = R.run(opt, params, vid, train_mode)
    assert np.abs(logp - rlogp).max() < TOL_LOGP
    assert abs(loss - rloss) < ltol * abs(rloss), (loss, rloss)
    for k, g in rgrads.items():
        if g is None:
            assert grads[k] is None or not np.any(grads[k]), k
            continue
        assert U.grad_close(k, grads[k], g, TOL_GRAD), (k, U.relerr(grads[k], g))
    assert U.relerr(g_tap, rg_tap) < TOL_GRAD, U.relerr(g_tap, rg_tap)
    return rg_tap


@pytest.mark.parametrize('fixture,case', CASES)
@pytest.mark.parametrize('train_mode', [False, True])
@pytest.mark.parametrize('arena', [False, True])
def test_module_path_matches_oracle_and_reference(fixture, case, train_mode, arena):
    g = U.gold(fixture)
    opt, params, vid = synth.make_case(case)
    got = _module_pass(opt, params, vid, train_mode, arena)
    _check_vs_oracle(opt, params, vid, train_mode, got)
    mode = 'train' if train_mode else 'eval'
    assert abs(got[1] - float(g[mode + '|loss'])) < TOL_LOSS * abs(float(g[mode + '|loss']))
    for k, v in got[2].items():
        if v is not None and k not in U.NOISE_ONLY and (mode + '|grad|' + k + '|linf') in g:
            ref = float(g[mode + '|grad|' + k + '|linf'])
            assert abs(float(np.abs(v).max()) - ref) <= TOL_GRAD * max(ref, 1e-5) + 1e-9, k
    if train_mode:
        assert U.relerr(got[3], g['train|g_tap']) < TOL_GRAD
    else:
        assert abs(float(np.sqrt((got[3].astype(np.float64) ** 2).sum())) - float(g['eval|g_tap|l2'])) < TOL_GRAD * float(g['eval|g_tap|l2'])


def _config(pairs):
    from echr_amd import _lib as L
    lib = L.load()
    for k, v in pairs:
        L.check(lib.echr_config_set(k.encode(), int(v)), 'config_set')


def test_persistent_kernels_at_d512_agree_and_match_oracle():
    """The ECHR-width 'CH' case (64 ragged, overlapping events): D = 512 sits exactly at the persistent recurrences' and greedy decoder's
    limit.  Runs with them on and off agree with each other and with the oracle."""
    opt, params, vid = synth.make_case('ch64')
    runs = []
    try:
        for on in (1, 0):
            _config([('persist', on), ('persist_bwd', on), ('persist_sample', on)])
            got = _module_pass(opt, params, vid, True)
            m = got[4]
            m.eval()
            tap, c3d, lda = _inputs(vid, False)
            with torch.no_grad():
                seq, _ = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
            runs.append((got, seq.cpu()))
    finally:
        _config([('persist', 1), ('persist_bwd', 1), ('persist_sample', 1)])
    (a, sa), (b, sb) = runs
    assert abs(a[1] - b[1]) < 1e-5 * abs(b[1])
    assert U.relerr(a[3], b[3]) < 1e-5
    _check_vs_oracle(opt, params, vid, True, a)
    oseq, _ = R.sample(opt, params, vid)
    assert torch.equal(sa, sb)
    assert sa.shape == oseq.shape and float((sa == oseq).float().mean()) > 0.99


def test_fixed_order_mode_is_bitwise_reproducible():
    import echr_amd
    opt, params, vid = synth.make_case('ch')
    assert not echr_amd.functional.rows_disjoint(vid['soi'])          # overlapping events: the slab-and-fold form
    echr_amd.set_deterministic(True)
    try:
        a = _module_pass(opt, params, vid, True, True)
        b = _module_pass(opt, params, vid, True, True)
    finally:
        echr_amd.set_deterministic(False)
    assert a[1] == b[1]
    assert np.array_equal(a[3], b[3])
    for k, v in a[2].items():
        assert (v is None and b[2][k] is None) or np.array_equal(v, b[2][k]), k


@pytest.mark.parametrize('fixture,case', CASES)
def test_greedy_and_beam_decoding(fixture, case):
    g = U.gold(fixture)
    opt, params, vid = synth.make_case(case)
    m = U.build_gpu_model(opt, params, False)
    tap, c3d, lda = _inputs(vid, False)
    with torch.no_grad():
        seq, logp = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
        bseq, blogp, bscore = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval', beam_size=3, return_score=True)
    assert np.array_equal(seq.cpu().numpy(), g['sample|seq'])
    assert np.abs(logp.cpu().numpy() - g['sample|logp']).max() < 1e-4
    ref = R.beam(opt, params, vid, 3)
    rseq = ref['seq']
    for n in range(rseq.shape[0]):
        if ref['margin'][n] < 1e-4:          # a near-tie between hypotheses: either order is within rounding
            continue
        T = min(bseq.shape[1], rseq.shape[1])
        assert np.array_equal(bseq[n, :T].cpu().numpy(), rseq[n, :T]), n
        assert abs(float(bscore[n]) - float(ref['score'][n])) < 1e-4 * max(1.0, abs(float(ref['score'][n]))), n


def test_caption_video_with_ch():
    """eval_utils.caption_video end to end with 'CH': the captions it reports are the greedy decode over the proposal encoder's states."""
    from echr_amd import eval_utils as EU, models as EM
    opt, params, vid = synth.make_case('ch')
    opt.K = 8
    cg = U.build_gpu_model(opt, params, False)
    torch.manual_seed(3)
    tap = EM.setup_tap(opt).cuda()
    tap.eval()
    dev = torch.device('cuda')
    rs = np.random.RandomState(11)
    c3d = torch.from_numpy(rs.standard_normal((24, opt.video_dim)).astype(np.float32)).to(dev)
    lda = torch.from_numpy(rs.standard_normal(opt.video_context_dim).astype(np.float32)).to(dev)
    f2t = lambda s, e, n, d: [round(float(s) / n * d, 3), round(float(e) / n * d, 3)]
    info, ex = EU.caption_video(tap, cg, c3d, lda, 60.0, f2t, topN=12)
    assert len(info) == len(ex['ind_select_list']) >= 1
    with torch.no_grad():
        seq, _ = cg(ex['tap_feats'], c3d, lda, [], ex['ind_select_list'], ex['soi_select_list'], mode='eval')
    for i, rec in enumerate(info):
        assert rec['sentence'] == [int(t) for t in seq[i].cpu().numpy() if t > 0]


def _fused(opt, params, train_mode=True):
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    m = U.build_gpu_model(opt, params, train_mode)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
    return m, o, FusedTrainStep(m, o, grad_clip=100.0)


@pytest.mark.parametrize('case', ['ch', 'cch'])
def test_fused_step_matches_oracle(case):
    opt, params, vid = synth.make_case(case)
    m, o, f = _fused(opt, params)
    tap, c3d, lda = _inputs(vid, False)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    g_tap = torch.zeros_like(tap)
    loss = float(f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], step=False, tap_grad=g_tap))
    torch.cuda.synchronize()
    _, rloss, rgrads, rg_tap = R.run(opt, params, vid, True)
    assert abs(loss - rloss) < TOL_LOSS * abs(rloss)
    for k, p in m.named_parameters():
        if rgrads[k] is None:
            continue
        assert U.grad_close(k, p.grad.detach().cpu().numpy(), rgrads[k], TOL_GRAD), k
    assert U.relerr(g_tap.cpu().numpy(), rg_tap) < TOL_GRAD
    with pytest.raises(NotImplementedError):
        f.prepare(c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:])


def test_joint_step_without_early_prepare_matches_autograd():
    """JointTrainStep(early_prepare=False) under 'CH' (tap_grad + defer_update: the library runs the plain form) against the autograd joint
    iteration on a twin: proposal encoder forward -> caption loss through the module path -> backward into the SST."""
    from echr_amd import models as EM
    from echr_amd.fused import JointTrainStep
    from echr_amd.misc.utils import LanguageModelCriterion, TAPModelCriterion
    from echr_amd.optim import ClampAdam
    opt, params, vid = synth.make_case('ch')
    sst = synth.make_sst_params(opt)
    dev = torch.device('cuda')
    T = vid['c3d'].shape[0]
    rs = np.random.RandomState(5)
    tl = torch.from_numpy((rs.uniform(size=(T, opt.K)) > 0.9).astype(np.float32)).to(dev)
    tm = torch.from_numpy((np.arange(T)[:, None] >= np.arange(opt.K)[None, :]).astype(np.float32)).to(dev)
    w1 = torch.from_numpy(rs.uniform(0.05, 0.3, size=(opt.K,)).astype(np.float32)).to(dev)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('c3d', 'lda'))

    def tap_model():
        t = EM.setup_tap(opt)
        t.load_state_dict({k: torch.from_numpy(v) for k, v in sst.items()})
        t = t.to(dev)
        t.eval()                              # (SST.eval switches the inter-layer dropout only and returns None, like the reference's)
        return t

    m, o, f = _fused(opt, params)
    tpa = tap_model()
    tap_o = ClampAdam(tpa.parameters(), lr=1e-9, arena=tpa.build_arena())
    j = JointTrainStep(f, tpa, tap_o, lambda1=0.01, early_prepare=False)
    with pytest.raises(NotImplementedError):
        JointTrainStep(f, tpa, tap_o, lambda1=0.01, early_prepare=True)(c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], tm, tl, w1)
    j(c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], tm, tl, w1)
    f.join()
    torch.cuda.synchronize()
    cg = float(j.cg_loss)
    sst_g = {k: tpa._echr_arena.grad_view(i).detach().cpu().numpy() for i, (k, _) in enumerate(tpa.named_parameters())}

    mb = U.build_gpu_model(opt, params, True)
    tpb = tap_model()
    tap, scores = tpb(c3d)
    tap_loss = TAPModelCriterion()(scores, tm, tl, w1)
    pred = mb(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    loss = LanguageModelCriterion()(pred, labels[:, 1:].to(dev), masks[:, 1:].to(dev))
    (0.01 * tap_loss + loss).backward()          # train.py:322-329, lambda2 = 1
    torch.cuda.synchronize()
    assert abs(cg - float(loss)) < TOL_LOSS * abs(float(loss))
    for k, p in tpb.named_parameters():
        assert U.relerr(sst_g[k], p.grad.detach().cpu().numpy()) < 1e-4, (k, U.relerr(sst_g[k], p.grad.detach().cpu().numpy()))


def test_self_critical_step_matches_module_path():
    from echr_amd.fused import SelfCriticalStep
    from echr_amd.misc.utils import RewardCriterion
    opt, params, vid = synth.make_case('ch')
    m, o, f = _fused(opt, params)
    tap, c3d, lda = _inputs(vid, False)
    sc = SelfCriticalStep(f)
    rs = np.random.RandomState(3)
    gen = torch.from_numpy(rs.randint(1, opt.CG_vocab_size + 1, size=(len(vid['soi']), 4)).astype(np.int64))
    reward = torch.from_numpy(rs.uniform(-1, 1, size=gen.shape).astype(np.float32))
    m.set_dropout_state(U.SEED, U.OFFSET)
    loss, _, _, _ = sc(tap, c3d, lda, vid['ind'], vid['soi'], gen_result=gen, reward=reward, step=False)
    torch.cuda.synchronize()
    loss = float(loss)
    gf = {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}

    mb = U.build_gpu_model(opt, params, True)
    tapb = tap.detach().clone()
    g2, slp, _ = mb(tapb, c3d, lda, [], vid['ind'], vid['soi'], mode='train_rl', gen_result=gen)
    lb = RewardCriterion()(slp, g2, reward.cuda())
    lb.backward()
    torch.cuda.synchronize()
    assert abs(loss - float(lb)) < 1e-5 * abs(float(lb)), (loss, float(lb))
    for k, p in mb.named_parameters():
        if p.grad is not None and k in gf:
            assert U.grad_close(k, gf[k], p.grad.detach().cpu().numpy(), 1e-4), k

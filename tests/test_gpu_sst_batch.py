"""The proposal encoder over a multi-video batch on the GPU (-m gpu): models.SST.forward_batch against the CPU reference of the contract
(tests/sst_batch_ref.py: oracle/echr_ref_cpu.sst_forward once per video, gradients summed, each video fed its slice of the batch's
dropout mask), the persistent form against the launch-per-step wavefront, the unchanged single-video call, and the reference's fixture.

Shapes are small on purpose: the recurrence goes wrong at video boundaries and where a video ends, not at size.  Gates are the project's own:
2e-5 absolute on tap / scores, U.grad_close(..., TOL_GRAD) on every parameter gradient (tests/test_gpu_parity.py::test_sst_native_vs_oracle).
"""
import functools

import numpy as np
import pytest
import torch

from tests import sst_batch_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

TOL_OUT = 2e-5
TOL_GRAD = 1e-5     # relative to the tensor's max-norm


@functools.lru_cache(maxsize=None)
def _case(lengths, D, H, K, train, seed=11):
    """(params, inputs, oracle result) of a batch; computed once and shared (read-only)."""
    rs = np.random.RandomState(seed + sum(lengths) + K)
    params = R.make_params(rs, D, H, K)
    x, wt, ws, ro = R.make_inputs(rs, lengths, D, H, K)
    return params, (x, wt, ws, ro), R.run(params, x, wt, ws, ro, train)


def _check(got, ref, tol_out=TOL_OUT):
    assert np.isfinite(got['tap']).all() and np.isfinite(got['scores']).all()
    print('tap %.3g scores %.3g' % (np.abs(got['tap'] - ref['tap']).max(), np.abs(got['scores'] - ref['scores']).max()))
    assert np.abs(got['tap'] - ref['tap']).max() < tol_out
    assert np.abs(got['scores'] - ref['scores']).max() < tol_out
    for k, g in ref['grads'].items():
        print(k, U.relerr(got['grads'][k], g))
        assert U.grad_close(k, got['grads'][k], g, TOL_GRAD), (k, U.relerr(got['grads'][k], g))


def _config(name, value):
    from echr_amd import _lib
    assert _lib.load().echr_config_set(name, value) == 0


@pytest.mark.parametrize('train', [True, False])
def test_mixed_lengths_vs_oracle_persistent(train):
    """A one-step video, two of equal length, the longest not first; inter-layer dropout 0.5 keyed by the batch-global row."""
    D, H, K = 500, 512, 16
    params, (x, wt, ws, ro), ref = _case((1, 2, 5, 37, 5), D, H, K, train)
    _check(R.gpu_pass(R.module(params, D, H, K, train), x, wt, ws, ro), ref)


@pytest.mark.parametrize('D,H,K,train', [(20, 24, 8, True), (20, 24, 8, False), (500, 512, 16, True), (500, 512, 16, False)])
def test_mixed_lengths_vs_oracle_wavefront(D, H, K, train):
    """The same batch through the launch-per-step wavefront (video axis on the grid): a small-H model, and H = 512 with sst_persist = 0."""
    params, (x, wt, ws, ro), ref = _case((1, 2, 5, 37, 5), D, H, K, train)
    try:
        _config(b'sst_persist', 0)
        got = R.gpu_pass(R.module(params, D, H, K, train), x, wt, ws, ro)
    finally:
        _config(b'sst_persist', 1)
    _check(got, ref)


def test_persistent_equals_wavefront_on_the_same_batch():
    from echr_amd import _lib
    D, H, K = 500, 512, 16
    params, (x, wt, ws, ro), _ = _case((3, 40, 17), D, H, K, True)
    out = {}
    try:
        for persist in (1, 0):
            _config(b'sst_persist', persist)
            out[persist] = R.gpu_pass(R.module(params, D, H, K, True), x, wt, ws, ro)
    finally:
        _config(b'sst_persist', 1)
    assert _lib.load().echr_check_async() == 0
    assert np.isfinite(out[1]['tap']).all()
    assert np.abs(out[1]['tap'] - out[0]['tap']).max() < 1e-5 and np.abs(out[1]['scores'] - out[0]['scores']).max() < 1e-5
    for k, g in out[0]['grads'].items():
        assert U.grad_close(k, out[1]['grads'][k], g, TOL_GRAD), (k, U.relerr(out[1]['grads'][k], g))


def test_more_videos_than_one_launch_carries():
    """V = echr_sst_batch_group() + 1: the library splits the batch into two persistent launches."""
    from echr_amd import _lib
    D, H, K = 500, 512, 16
    V = _lib.load().echr_sst_batch_group() + 1
    lengths = tuple(1 + v % 6 for v in range(V))
    params, (x, wt, ws, ro), ref = _case(lengths, D, H, K, True)
    _check(R.gpu_pass(R.module(params, D, H, K, True), x, wt, ws, ro), ref)


@pytest.mark.parametrize('D,H,K,persist', [(500, 512, 16, 1), (500, 512, 16, 0), (20, 24, 8, 1)])
def test_one_video_batch_equals_forward_bit_for_bit(D, H, K, persist):
    """V = 1 takes today's keys: outputs and gradients of forward_batch equal SST.forward on that video exactly.  Run in the fixed-order mode:
    by default the split-K products of a short video add with atomics, so two runs of SST.forward itself differ in the last bit.
    On the persistent route, with sst_persist = 0 and on the small-H model: the wavefront kernels serve one video and a batch alike."""
    import echr_amd
    params, (x, wt, ws, ro), _ = _case((9,), D, H, K, True)
    dev = torch.device('cuda')
    try:
        _config(b'sst_persist', persist)
        echr_amd.set_deterministic(True)
        got = R.gpu_pass(R.module(params, D, H, K, True), x, wt, ws, ro)
        m = R.module(params, D, H, K, True)
        tap, sc = m(torch.from_numpy(x).to(dev))
        ((tap * torch.from_numpy(wt).to(dev)).sum() + (sc * torch.from_numpy(ws).to(dev)).sum()).backward()
        # and a list of videos is the concatenated matrix plus offsets
        t2, s2 = R.module(params, D, H, K, True).forward_batch([torch.from_numpy(x).to(dev)])
        # the library's own batch entries with V = 1 (the module hands a one-video batch to forward())
        from echr_amd import functional as EF
        m3 = R.module(params, D, H, K, True)
        ro3 = EF.sst_row_offsets(ro, x.shape[0])
        t3, s3 = EF.SSTFunction.apply(torch.from_numpy(x).to(dev), ro3, torch.from_numpy(ro3).to(dev), 0.5, EF.DropState(U.SEED, U.OFFSET, True), None,
                                      *m3.native_params())
        ((t3 * torch.from_numpy(wt).to(dev)).sum() + (s3 * torch.from_numpy(ws).to(dev)).sum()).backward()
        torch.cuda.synchronize()
    finally:
        echr_amd.set_deterministic(False)
        _config(b'sst_persist', 1)
    assert torch.equal(tap.detach().cpu(), torch.from_numpy(got['tap'])) and torch.equal(sc.detach().cpu(), torch.from_numpy(got['scores']))
    for k, p in m.named_parameters():
        assert np.array_equal(p.grad.cpu().numpy(), got['grads'][k]), k
    assert torch.equal(t2.detach().cpu(), torch.from_numpy(got['tap'])) and torch.equal(s2.detach().cpu(), torch.from_numpy(got['scores']))
    assert torch.equal(t3.detach().cpu(), torch.from_numpy(got['tap'])) and torch.equal(s3.detach().cpu(), torch.from_numpy(got['scores']))
    for k, p in m3.named_parameters():
        assert np.array_equal(p.grad.cpu().numpy(), got['grads'][k]), k


@pytest.mark.parametrize('persist', [1, 0])
def test_recurrent_weight_gradient_excludes_the_boundary_pair(persist):
    """dW_hh pairs dG(t) with h(t-1) INSIDE a video only: the batch's gradient is the sum of the two single-video gradients, and it is not
    the gradient of the two videos run as one sequence (whose first row of video 1 meets the last state of video 0)."""
    D, H, K = 500, 512, 16
    params, (x, wt, ws, ro), _ = _case((6, 4), D, H, K, False)
    try:
        _config(b'sst_persist', persist)
        got = R.gpu_pass(R.module(params, D, H, K, False), x, wt, ws, ro)
        single = None
        for a, b in zip(ro[:-1], ro[1:]):
            g = R.gpu_pass(R.module(params, D, H, K, False), x[a:b], wt[a:b], ws[a:b], [0, b - a])['grads']
            single = g if single is None else {k: single[k] + g[k] for k in g}
        joined = R.gpu_pass(R.module(params, D, H, K, False), x, wt, ws, [0, ro[-1]])['grads']
    finally:
        _config(b'sst_persist', 1)
    for k in ('rnn.weight_hh_l0', 'rnn.weight_hh_l1'):
        assert U.grad_close(k, got['grads'][k], single[k], TOL_GRAD), (k, U.relerr(got['grads'][k], single[k]))
        assert not U.grad_close(k, got['grads'][k], joined[k], 100 * TOL_GRAD), k


def test_video_zero_of_a_batch_matches_the_reference_fixture():
    """[the reference fixture's video, a second random one] in eval mode: rows of video 0 against the reference's own tap / scores."""
    from echr_amd import models, synth
    g = U.gold('sst.npz')
    params = {k[len('param|'):]: v for k, v in g.items() if k.startswith('param|')}
    m = models.setup_tap(synth.default_opt(**dict(synth.CASES['tiny']['opt'], K=8)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.cuda()
    m.eval()
    x0 = g['x']
    x1 = np.random.RandomState(4).standard_normal((x0.shape[0] + 3, x0.shape[1])).astype(np.float32)
    dev = torch.device('cuda')
    tap, sc = m.forward_batch([torch.from_numpy(x0).to(dev), torch.from_numpy(x1).to(dev)])
    T0 = x0.shape[0]
    assert tap.shape[0] == 2 * T0 + 3
    assert np.abs(tap[:T0].detach().cpu().numpy() - g['tap']).max() < 1e-5 and np.abs(sc[:T0].detach().cpu().numpy() - g['scores']).max() < 1e-5
    # and the other order: the fixture's video behind the random one
    tap, sc = m.forward_batch([torch.from_numpy(x1).to(dev), torch.from_numpy(x0).to(dev)])
    assert np.abs(tap[T0 + 3:].detach().cpu().numpy() - g['tap']).max() < 1e-5 and np.abs(sc[T0 + 3:].detach().cpu().numpy() - g['scores']).max() < 1e-5


def test_arena_step_equals_the_step_on_the_summed_single_video_gradients():
    """SST.build_arena() + ClampAdam: ONE batched backward into the zero-filled flat gradient buffer + one step, against V single-video
    backward passes accumulating into per-tensor gradients + one step.  Parameters within 1e-6 of the tensor's max-norm after the update.
    Adam's first step is lr * g / (|g| + eps): with the default eps = 1e-8 it is lr * sign(g), discontinuous at g = 0, and two fp32 summation
    orders of the same gradient may differ in the sign of an element that is zero to rounding; eps = 1 keeps the update Lipschitz in g
    (slope <= lr), so a gradient difference inside TOL_GRAD moves a parameter by at most lr * 1e-5 * max|g|."""
    from echr_amd.misc.utils import clip_gradient
    from echr_amd.optim import ClampAdam
    D, H, K = 500, 512, 16
    params, (x, wt, ws, ro), _ = _case((4, 9, 2), D, H, K, False)
    dev = torch.device('cuda')
    X, WT, WS = (torch.from_numpy(a).to(dev) for a in (x, wt, ws))
    scale = 1.0 / ro[-1]
    ma, mb = R.module(params, D, H, K, False), R.module(params, D, H, K, False)
    arena = ma.build_arena()
    oa = ClampAdam(ma.parameters(), lr=1e-3, eps=1.0, arena=arena)
    ob = ClampAdam(mb.parameters(), lr=1e-3, eps=1.0)
    oa.zero_grad(); ob.zero_grad()
    tap, sc = ma.forward_batch(X, ro)
    (((tap * WT).sum() + (sc * WS).sum()) * scale).backward()
    assert arena.grads_in_arena()
    for a, b in zip(ro[:-1], ro[1:]):
        tap, sc = mb(X[a:b])
        (((tap * WT[a:b]).sum() + (sc * WS[a:b]).sum()) * scale).backward()
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert U.grad_close(k, pa.grad.cpu().numpy(), pb.grad.cpu().numpy(), TOL_GRAD), (k, U.relerr(pa.grad.cpu().numpy(), pb.grad.cpu().numpy()))
    clip_gradient(oa, 100.0); clip_gradient(ob, 100.0)
    oa.step(); ob.step()
    torch.cuda.synchronize()
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        a, b = pa.detach().cpu().numpy(), pb.detach().cpu().numpy()
        assert not np.array_equal(b, params[k]), k
        print(k, np.abs(a - b).max() / np.abs(b).max())
        assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max(), (k, np.abs(a - b).max() / np.abs(b).max())


def test_from_videos_with_tap_model_feeds_the_caption_batch():
    """VideoBatch.from_videos(..., tap_model=sst) -> forward_batch(mode='train') -> batch.criterion -> backward(): the encoder's parameter
    gradients (through 'ER3', which reads batch.tap) equal those of the same batch built from V separate sst(c3d_v) calls."""
    from echr_amd import models, synth
    from echr_amd.batch import VideoBatch
    from echr_amd.misc.utils import LanguageModelCriterion
    opt, params, vids = synth.make_vbatch('vbctx')
    assert 'ER3' in opt.event_context_type
    dev = torch.device('cuda')
    keys = ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')
    sst_params = R.make_params(np.random.RandomState(2), opt.video_dim, opt.hidden_dim, opt.K)

    def run(batched):
        sst = models.setup_tap(opt)
        sst.load_state_dict({k: torch.from_numpy(v) for k, v in sst_params.items()})
        sst = sst.cuda()
        sst.eval()
        cg = U.build_gpu_model(opt, params, False)
        if batched:
            b = VideoBatch.from_videos([{k: v[k] for k in keys} for v in vids], tap_model=sst)
        else:
            b = VideoBatch.from_videos([dict({k: v[k] for k in keys}, tap=sst(torch.from_numpy(v['c3d']).to(dev))[0]) for v in vids], device=dev)
        assert b.tap.requires_grad and b.tap.is_cuda
        total, _ = b.criterion(LanguageModelCriterion(), cg.forward_batch(b, mode='train'))
        total.backward()
        torch.cuda.synchronize()
        return float(total.detach()), b.tap.detach().cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in sst.named_parameters() if p.grad is not None}
    la, ta, ga = run(True)
    lb, tb, gb = run(False)
    assert np.abs(ta - tb).max() < TOL_OUT and abs(la - lb) < 1e-5 * abs(lb)
    assert set(ga) == set(gb) and 'rnn.weight_hh_l0' in ga
    for k in gb:
        assert U.grad_close(k, ga[k], gb[k], TOL_GRAD), (k, U.relerr(ga[k], gb[k]))


def test_deterministic_mode_is_bitwise():
    """echr_amd.set_deterministic(True): two runs of the batched forward + backward agree bit for bit."""
    import echr_amd
    D, H, K = 500, 512, 16
    params, (x, wt, ws, ro), _ = _case((3, 40, 17), D, H, K, True)
    try:
        echr_amd.set_deterministic(True)
        a = R.gpu_pass(R.module(params, D, H, K, True), x, wt, ws, ro)
        b = R.gpu_pass(R.module(params, D, H, K, True), x, wt, ws, ro)
    finally:
        echr_amd.set_deterministic(False)
    assert np.array_equal(a['tap'], b['tap']) and np.array_equal(a['scores'], b['scores'])
    for k in a['grads']:
        assert np.array_equal(a['grads'][k], b['grads'][k]), k


def test_pre_tap_mode_of_the_example_trains_the_encoder_over_batches():
    """examples/train_synthetic.py --pre_tap: m_batch videos per forward_batch call, tap_criterion_batch, one clamp + step; the loss goes down."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('train_synthetic', os.path.join(os.path.dirname(U.GOLD), '..', 'examples', 'train_synthetic.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist, _, tap = mod.main(['--pre_tap', '--iters', '16', '--m_batch', '3', '--quiet', '--lr', '2e-3'])
    assert len(hist) == 16 and np.isfinite(hist).all()
    assert np.mean(hist[-4:]) < np.mean(hist[:4]), hist
    assert all(p.grad is not None for p in tap.parameters())

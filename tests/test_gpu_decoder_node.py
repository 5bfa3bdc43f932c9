"""Which input each gradient of the decoder node and the initial-state node lands on (-m gpu), through the module API only:
CaptionGenerator.forward_batch(mode='train') / forward(mode='train'), the criterion, backward().

Case 'vbinitch' of synth.VBATCH: an initial decoder state ('VE' through init_linear), 'CH' clip rows (d tap comes back from the decoder's
backward) and five videos, so h0, tap and vid are all live inputs of the decoder node.  Three forms -- the batch, a one-video batch of its
video 0, and video 0 through the single-video forward -- each run in the four combinations of {init_linear's parameters require grad or
not} x {the tap leaves require grad or not}, without and with the flat gradient arena, under echr_amd.set_deterministic(True) from the
same dropout state:

  * tap.grad and init_linear.*.grad exist exactly when requested, every other parameter's gradient exists in all four or in none;
  * a gradient that exists in two combinations is the same tensor in both, bit for bit (the same kernels in the same order on the same
    inputs: what is not requested is computed or not, never summed differently);
  * with everything requested the one-video batch and the single-video form agree in log-probs, loss and every gradient.  NOT bit for bit:
    the two forms run different kernels in front of the decoder (segmented scene means, the block-diagonal event encoder), and on the commit
    before the two decoder Functions became one their log-probs already differ by 9.5e-7 in deterministic mode.  The gates are the project's
    own for this case (tests/test_gpu_init_batch.py): log-probs TOL_LOGP, loss TOL_LOSS relative, each gradient tol_grad(case) of its max-norm.

A gradient returned in the wrong slot shows as a missing or a misattached .grad (a shape error from autograd, or a None), or as a tensor
that changes with what else was requested.
"""
import functools

import numpy as np
import pytest
import torch

from echr_amd import synth
from tests import util as U
from tests.test_gpu_init_batch import TOL_LOGP, TOL_LOSS, tol_grad

pytestmark = pytest.mark.gpu

CASE = 'vbinitch'
FORMS = ('batch', 'one_video_batch', 'single')
COMBOS = [(True, True), (True, False), (False, True), (False, False)]          # (init_linear requires grad, tap requires grad)
INIT = ('lm_model.init_linear.weight', 'lm_model.init_linear.bias')


def _pass(m, opt, vids, form, init_req, tap_req):
    from echr_amd.batch import VideoBatch
    from echr_amd.misc.utils import LanguageModelCriterion
    dev = torch.device('cuda')
    for p in m.parameters():
        p.grad = None
    m.set_dropout_state(U.SEED, U.OFFSET)
    for k, p in m.named_parameters():
        if k in INIT:
            p.requires_grad_(init_req)
    crit = LanguageModelCriterion()
    vs = vids if form == 'batch' else vids[:1]
    taps = [torch.from_numpy(v['tap']).to(dev).requires_grad_(tap_req) for v in vs]
    if form == 'single':
        v = vs[0]
        labels, masks = torch.from_numpy(v['labels']), torch.from_numpy(v['masks'])
        logp = m(taps[0], torch.from_numpy(v['c3d']).to(dev), torch.from_numpy(v['lda']).to(dev), labels, v['ind'], v['soi'], mode='train')
        loss = crit(logp, labels[:, 1:].to(dev), masks[:, 1:].to(dev))
    else:
        b = VideoBatch.from_videos([dict({k: v[k] for k in ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')}, tap=t) for v, t in zip(vs, taps)],
                                   device=dev, CG_init_feats_type=opt.CG_init_feats_type, clip_context_type=opt.clip_context_type)
        logp = m.forward_batch(b, mode='train')
        loss, _ = b.criterion(crit, logp)
    loss.backward()
    torch.cuda.synchronize()
    return dict(logp=logp.detach().cpu().numpy(), loss=float(loss.detach()),
                tap=[None if t.grad is None else t.grad.cpu().numpy() for t in taps],
                grads={k: (None if p.grad is None else p.grad.detach().cpu().numpy().copy()) for k, p in m.named_parameters()})


@functools.lru_cache(maxsize=None)
def _results(arena):
    """Every form in every combination on ONE model (gradients cleared and the dropout stream rewound in front of each pass)."""
    import echr_amd
    opt, params, vids = synth.make_vbatch(CASE)
    assert opt.CG_init_feats_type == 'VE' and opt.clip_context_type == 'CH' and len(vids) > 1
    echr_amd.set_deterministic(True)
    try:
        m = U.build_gpu_model(opt, params, True)
        if arena:
            m.build_arena()
        return {(form,) + c: _pass(m, opt, vids, form, *c) for form in FORMS for c in COMBOS}
    finally:
        echr_amd.set_deterministic(False)


def _same(what, a, b):
    d = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    print('%-60s max |diff| %.2e of %.2e' % (what, d, float(np.abs(b).max())))
    assert a.shape == b.shape and np.array_equal(a, b), (what, d)


@pytest.mark.parametrize('arena', [False, True], ids=['private', 'arena'])
@pytest.mark.parametrize('form', FORMS)
def test_gradients_exist_exactly_when_requested(form, arena):
    res = _results(arena)
    others = None
    for init_req, tap_req in COMBOS:
        r = res[form, init_req, tap_req]
        assert all((g is not None) == tap_req for g in r['tap']), (init_req, tap_req)
        assert all(g is None or np.any(g) for g in r['tap'])
        for k in INIT:
            assert (r['grads'][k] is not None) == init_req, (k, init_req, tap_req)
            assert r['grads'][k] is None or np.any(r['grads'][k]), k
        have = {k for k, g in r['grads'].items() if g is not None and k not in INIT}
        assert 'lm_model.embed.weight' in have and 'lm_model.core.layer2.weight_ih' in have and 'fusion_model.event_emb.weight' in have
        assert others is None or have == others, (init_req, tap_req, have ^ others)
        others = have


@pytest.mark.parametrize('arena', [False, True], ids=['private', 'arena'])
@pytest.mark.parametrize('form', FORMS)
def test_a_gradient_is_the_same_in_every_combination_that_has_it(form, arena):
    res = _results(arena)
    base = res[(form,) + COMBOS[0]]          # everything requested
    for c in COMBOS[1:]:
        r = res[(form,) + c]
        _same('%s %s logp' % (form, c), r['logp'], base['logp'])
        assert r['loss'] == base['loss']
        for v, g in enumerate(r['tap']):
            if g is not None:
                _same('%s %s d tap video %d' % (form, c, v), g, base['tap'][v])
        for k, g in r['grads'].items():
            if g is not None:
                _same('%s %s %s' % (form, c, k), g, base['grads'][k])


@pytest.mark.parametrize('arena', [False, True], ids=['private', 'arena'])
def test_one_video_batch_equals_the_single_video_form(arena):
    res = _results(arena)
    bat, one = res[('one_video_batch',) + COMBOS[0]], res[('single',) + COMBOS[0]]
    tol = tol_grad(CASE)
    d = float(np.abs(bat['logp'] - one['logp']).max())
    print('logp: max |diff| %.2e   loss %.9g vs %.9g' % (d, bat['loss'], one['loss']))
    assert bat['logp'].shape == one['logp'].shape and d < TOL_LOGP, d
    assert abs(bat['loss'] - one['loss']) < TOL_LOSS * abs(one['loss'])
    a, r = bat['tap'][0], one['tap'][0]
    print('d tap: rel err %.2e' % U.relerr(a, r, U.GRAD_FLOOR))
    assert a.shape == r.shape and np.abs(a - r).max() <= tol * max(float(np.abs(r).max()), U.GRAD_FLOOR) + 1e-9
    assert set(k for k, g in bat['grads'].items() if g is not None) == set(k for k, g in one['grads'].items() if g is not None)
    bad = []
    for k, g in bat['grads'].items():
        if g is not None:
            print('%-55s rel err %.2e' % (k, U.relerr(g, one['grads'][k], U.GRAD_FLOOR)))
            if g.shape != one['grads'][k].shape or not U.grad_close(k, g, one['grads'][k], tol):
                bad.append((k, U.relerr(g, one['grads'][k])))
    assert not bad, bad

"""The joint 'tap_cg' iteration over a multi-video batch, the part that needs no GPU: the new library symbols, fused.JointBatchStep's
validation and refusals, the refusals that stay, and the CPU reference of the contract (tests/joint_batch_ref.py) against the reference's
own numbers (tests/golden/case_joint_batch.npz, made by tools/make_golden_joint_batch.py)."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from echr_amd import synth
from echr_amd.batch import VideoBatch
from oracle import summary as SM
from tests import joint_batch_ref as J
from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_LOSS = 1e-5


def test_new_symbols_are_declared_bound_and_exported():
    from echr_amd import _lib
    lib = _lib.load()
    new = ['echr_tap_bce_fwd_batch', 'echr_tap_bce_bwd_batch', 'echr_train_step_batch_tap', 'echr_train_step_batch_tap_ws_floats']
    bound = {s[0] for s in _lib.SYMBOLS}
    hdr = open(os.path.join(ROOT, 'include', 'echr_hip.h')).read()
    for name in new:
        assert name in bound and hasattr(lib, name) and re.search(r'\b%s\s*\(' % name, hdr), name
    # no struct changed: the ABI version and every restated layout stand
    assert lib.echr_version() == _lib.ABI_VERSION == 3
    for cname, cls in _lib.ABI_STRUCTS.items():
        assert lib.echr_abi_sizeof(cname.encode()) == C.sizeof(cls), cname


def test_library_entries_refuse_bad_arguments_without_a_launch():
    from echr_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(64)          # never dereferenced: every call below is refused by the argument check
    assert lib.echr_tap_bce_fwd_batch(p, p, p, p, 3, p, 2, 16, p, p, p, None) != 0          # w1_ld must be 0 or K
    assert lib.echr_tap_bce_fwd_batch(p, p, p, p, 0, None, 2, 16, p, p, p, None) != 0       # row_offset missing
    assert lib.echr_tap_bce_bwd_batch(p, p, p, p, 0, p, 0, 16, 10, p, p, None) != 0         # V = 0
    assert lib.echr_tap_bce_bwd_batch(p, p, p, p, 0, p, 4, 16, 3, p, p, None) != 0          # fewer rows than videos
    a, x = _lib.TrainStepArgs(), _lib.BatchExt(2, None, 64, None, None)
    a.dec.N = 4
    a.host_nll, a.vh_offset = 1, -1
    assert lib.echr_train_step_batch_tap(C.byref(a), C.byref(x), None, None, None, None) != 0    # g_tap missing
    assert b'g_tap' in lib.echr_last_error()
    a.g_tap, a.tap, a.Ht, a.defer_update = 64, 64, 512, 1
    assert lib.echr_train_step_batch_tap(C.byref(a), C.byref(x), None, None, None, None) != 0    # defer_update stays refused
    assert b'defer_update' in lib.echr_last_error()
    a.defer_update, a.vh_offset = 0, 0
    assert lib.echr_train_step_batch_tap(C.byref(a), C.byref(x), None, None, None, None) != 0    # 'VH' without row_offset
    assert b'row_offset' in lib.echr_last_error()
    assert lib.echr_train_step_batch_tap_ws_floats(None, None) == -1


def _videos():
    return synth.make_vbatch('vbctx')


def test_joint_batch_step_constructor_validation():
    import echr_amd
    from echr_amd import models
    from echr_amd.fused import FusedTrainStep, JointBatchStep
    from echr_amd.optim import ClampAdam
    opt, _, _ = _videos()
    opt.K = 8
    sst = models.setup_tap(opt)
    with pytest.raises(TypeError):
        JointBatchStep(echr_amd.CaptionGenerator(opt), sst, None)
    f = object.__new__(FusedTrainStep)
    with pytest.raises(ValueError):          # no arena
        JointBatchStep(f, sst, ClampAdam(sst.parameters(), lr=1e-3))
    with pytest.raises(ValueError):          # not a ClampAdam
        JointBatchStep(f, sst, torch.optim.SGD(sst.parameters(), lr=1e-3))
    sig = inspect.signature(JointBatchStep.__init__).parameters
    assert [sig[k].default for k in ('lambda1', 'lambda2', 'tap_grad_clip')] == [1.0, 1.0, None]


def test_joint_batch_step_refuses_what_batches_refuse():
    import echr_amd
    from echr_amd.fused import FusedTrainStep, JointBatchStep
    opt, params, vids = _videos()
    b = VideoBatch.from_videos(vids)

    def step(**over):
        o = synth.make_vbatch('vbctx')[0]
        for k, v in over.items():
            setattr(o, k, v)
        s, f = object.__new__(JointBatchStep), object.__new__(FusedTrainStep)
        f.model = echr_amd.CaptionGenerator(o)
        s.fused, s.lib, s.tap_model = f, None, None
        return s
    for over in (dict(CG_init_feats_type='V'), dict(clip_context_type='CH'), dict(clip_context_type='CC+CH')):
        with pytest.raises(NotImplementedError):
            step(**over)(b, None, None, None)
    s = step()
    s.fused.model._echr_arena = SimpleNamespace(early_grad_hook=lambda *a, **k: None, early_reducer=None)
    with pytest.raises(NotImplementedError):
        s(b, None, None, None)
    s = step()
    s.fused._prepared = True
    with pytest.raises(NotImplementedError):
        s(b, None, None, None)


def test_pinned_refusals_still_raise_and_name_the_batch_step():
    from echr_amd.fused import DataParallelStep, FusedTrainStep, JointTrainStep, SelfCriticalStep
    opt, params, vids = _videos()
    b = VideoBatch.from_videos(vids)
    for cls in (SelfCriticalStep, JointTrainStep, DataParallelStep):
        with pytest.raises(NotImplementedError):
            object.__new__(cls).batch(b)
    with pytest.raises(NotImplementedError, match='JointBatchStep'):
        object.__new__(JointTrainStep).batch(b)
    with pytest.raises(NotImplementedError):
        object.__new__(FusedTrainStep).batch(b, tap_grad=torch.zeros(1))


def test_joint_train_step_takes_lambda2():
    from echr_amd import models
    from echr_amd.fused import FusedTrainStep, JointTrainStep
    from echr_amd.optim import ClampAdam
    sig = inspect.signature(JointTrainStep.__init__).parameters
    assert sig['lambda2'].default == 1.0
    # every earlier positional argument keeps its place
    assert list(sig)[:8] == ['self', 'fused', 'tap_model', 'tap_optim', 'lambda1', 'tap_grad_clip', 'early_prepare', 'order']
    opt, _, _ = _videos()
    opt.K = 8
    sst = models.setup_tap(opt)
    with pytest.raises(ValueError):          # the keyword is accepted: the call gets as far as the arena validation
        JointTrainStep(object.__new__(FusedTrainStep), sst, ClampAdam(sst.parameters(), lr=1e-3), lambda1=0.01, lambda2=0.5)


def test_from_videos_takes_a_tap_producer():
    opt, params, vids = _videos()
    seen = {}

    def tap_fn(c3d, rows):
        seen['rows'] = list(rows)
        return torch.zeros(c3d.shape[0], 7)
    b = VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')} for v in vids], tap_fn=tap_fn)
    assert seen['rows'] == J.row_offsets(vids) and tuple(b.tap.shape) == (seen['rows'][-1], 7)
    with pytest.raises(ValueError):
        VideoBatch.from_videos(vids, tap_fn=tap_fn, tap_model=object())


def test_joint_batch_ref_matches_the_reference_fixture():
    """Both per-video loss vectors and the ACCUMULATED gradients of both models: the reference's own numbers (eval mode)."""
    g = U.gold('case_joint_batch.npz')
    opt, params, sst_params, vids, tap_in = J.setup('vbctx')
    lam1, lam2 = (float(x) for x in g['lambda'])
    assert (lam1, lam2) == (J.LAMBDA1, 1.0)
    ref = J.run(opt, params, sst_params, vids, tap_in, False, lam1, lam2)
    for name in ('tap_losses', 'cg_losses'):
        assert g['eval|' + name].shape == (len(vids),)
        assert np.abs(ref[name] - g['eval|' + name]).max() < TOL_LOSS * np.abs(g['eval|' + name]).max(), name
    for tag, grads in (('eval|grad|', ref['grads']), ('eval|sstgrad|', ref['sst_grads'])):
        n = 0
        for k, gr in grads.items():
            if gr is None or k in U.NOISE_ONLY:
                continue
            linf = float(g[tag + k + '|linf'])
            assert abs(float(np.abs(gr).max()) - linf) <= 1e-4 * max(linf, U.GRAD_FLOOR) + 1e-9, k
            head, strided = SM.grad_slices(gr)
            for got, want in ((head, g[tag + k + '|head']), (strided, g[tag + k + '|strided'])):
                assert np.abs(got - want).max() <= 1e-4 * max(linf, U.GRAD_FLOOR) + 1e-9, k          # (the oracle-vs-reference bar of tools/make_golden*.py)
            n += 1
        assert n >= 10
    assert os.path.getsize(os.path.join(U.GOLD, 'case_joint_batch.npz')) <= os.path.getsize(os.path.join(U.GOLD, 'case_vbatch.npz'))


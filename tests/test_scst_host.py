"""Self-critical training, host side: RewardCriterion's formula, the 'train_rl' mode's availability and the new C ABI entry points."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_formula(inp, seq, reward):
    mask = (seq > 0).float()
    mask = torch.cat([torch.ones(seq.shape[0], 1), mask[:, :-1]], 1)
    return float((-inp * reward * mask).sum() / mask.sum())


def test_reward_criterion_matches_the_formula_on_host_tensors():
    from echr_amd.misc.utils import RewardCriterion
    rs = np.random.RandomState(3)
    seq = torch.tensor([[0, 0, 0, 0], [5, 2, 0, 0], [7, 1, 3, 9], [4, 0, 0, 0]])          # row 0 finishes at the first step: mask [1, 0, 0, 0]
    inp = torch.from_numpy(-rs.uniform(0.1, 5.0, size=(4, 4)).astype(np.float32)).requires_grad_(True)
    reward = torch.from_numpy(rs.uniform(-2.0, 2.0, size=(4, 4)).astype(np.float32))    # signed
    loss = RewardCriterion()(inp, seq, reward)
    assert abs(float(loss.detach()) - _reference_formula(inp.detach(), seq, reward)) < 1e-6
    loss.backward()
    mask = torch.tensor([[1, 0, 0, 0], [1, 1, 1, 0], [1, 1, 1, 1], [1, 1, 0, 0]], dtype=torch.float32)
    assert torch.allclose(inp.grad, -reward * mask / mask.sum(), atol=1e-7)
    # a per-caption reward [N] is broadcast over the steps
    r1 = torch.tensor([1.0, -0.5, 2.0, -1.0])
    assert abs(float(RewardCriterion()(inp.detach(), seq, r1)) - _reference_formula(inp.detach(), seq, r1[:, None].expand(4, 4))) < 1e-6


def test_train_rl_mode_is_live():
    """mode='train_rl' no longer raises NotImplementedError; without a GPU the call fails on the inputs' device like every other mode."""
    import echr_amd
    from echr_amd import synth
    opt, params, vid = synth.make_case('tiny')
    m = echr_amd.CaptionGenerator(opt)
    tap, c3d, lda = (torch.from_numpy(vid[k]) for k in ('tap', 'c3d', 'lda'))
    with pytest.raises(echr_amd.functional.L.EchrHipError):
        m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='train_rl')
    with pytest.raises(NotImplementedError):
        m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='1stage')
    assert hasattr(m.lm_model, 'sequence_logprobs') and hasattr(m.lm_model, 'sample_train')


def test_self_critical_entry_points_are_declared_bound_and_exported():
    from echr_amd import _lib
    new = {'echr_decoder_sample_train', 'echr_train_step_rw', 'echr_train_step_rw_ws_floats', 'echr_gather_tokens_fwd',
           'echr_gather_tokens_bwd', 'echr_reward_loss_fwd', 'echr_reward_loss_bwd'}
    hdr = open(os.path.join(ROOT, 'include', 'echr_hip.h')).read()
    declared = set(re.findall(r'\b(echr_[a-z0-9_]+)\s*\(', hdr))
    assert new <= declared
    assert new <= {s[0] for s in _lib.SYMBOLS}
    lib = _lib.load()
    for name in new:
        assert hasattr(lib, name), name
    # no argument struct changed: every ctypes mirror still has the library's size
    for name, cls in _lib.ABI_STRUCTS.items():
        assert lib.echr_abi_sizeof(name.encode()) == __import__('ctypes').sizeof(cls), name


def test_reward_weighted_step_workspace_holds_the_weights():
    """echr_train_step_rw's workspace carries the [N,S] weights in its index region: never smaller than the plain step's."""
    import ctypes
    from echr_amd import _lib
    lib = _lib.load()
    a = _lib.TrainStepArgs()
    a.tsrm.N, a.tsrm.Din, a.tsrm.Df, a.tsrm.Do, a.tsrm.G = 4, 24, 32, 32, 4
    d = a.dec
    d.N, d.A, d.Tv, d.D, d.H, d.E, d.Ha, d.De, d.Dv, d.V1, d.S = 4, 7, 30, 20, 32, 16, 24, 32, 12, 31, 6
    plain, rw = lib.echr_train_step_ws_floats(ctypes.byref(a)), lib.echr_train_step_rw_ws_floats(ctypes.byref(a))
    assert plain > 0 and rw >= plain + d.N * d.S - 64

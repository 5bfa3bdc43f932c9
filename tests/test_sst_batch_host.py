"""Host-side contract of the batched proposal encoder (no GPU): the five exports and the ctypes restatement of echr_sst_batch, the input
validation of SST.forward_batch / VideoBatch.from_videos(tap_model=...), and misc.utils.tap_criterion_batch against its per-video sum."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from echr_amd import _lib, models, synth
from echr_amd.batch import VideoBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ('echr_sst_batch_ws_floats', 'echr_sst_batch_ws_bwd_floats', 'echr_sst_fwd_batch', 'echr_sst_bwd_batch', 'echr_sst_batch_group')


def test_header_declares_and_library_exports_the_five_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'echr_hip.h')).read()
    declared = {n for n, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in EXPORTS:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in declared, name
        assert getattr(lib, name) is not None
    assert 'echr_sst_batch;' in hdr and lib.echr_version() == 3
    assert 1 <= lib.echr_sst_batch_group() <= 16


def test_ctypes_struct_size_matches_the_library():
    lib = _lib.load()
    assert 'echr_sst_batch' in _lib.ABI_STRUCTS
    assert lib.echr_abi_sizeof(b'echr_sst_batch') == C.sizeof(_lib.SstBatch) > 0
    # the batch's workspaces hold at least the single-video ones over the same rows
    assert lib.echr_sst_batch_ws_floats(40, 500, 512, 16, 3) >= lib.echr_sst_ws_floats(40, 500, 512, 16)
    assert lib.echr_sst_batch_ws_bwd_floats(40, 500, 512, 16, 3) >= lib.echr_sst_ws_bwd_floats(40, 500, 512, 16) + 2 * 40 * 512


def _video(T=12, with_tap=True):
    v = synth.make_video(2, 8, 6, 301, seed=3, T_v=T, video_dim=20, hidden_dim=24, lda_dim=10)
    d = {k: v[k] for k in ('c3d', 'lda', 'ind', 'soi')}
    if with_tap:
        d['tap'] = v['tap']
    return d


def test_from_videos_without_tap_and_without_tap_model_keeps_its_message():
    with pytest.raises(ValueError) as e:
        VideoBatch.from_videos([_video(), _video(with_tap=False)])
    assert str(e.value) == "video 1 lacks ['tap']"
    b = VideoBatch.from_videos([_video(), _video()])           # unchanged without tap_model
    assert b.tap.shape[0] == b.c3d.shape[0] == int(b.row_offset[-1])


def _sst(D=20, H=24, K=8):
    return models.setup_tap(synth.default_opt(video_dim=D, hidden_dim=H, K=K))


def test_forward_batch_on_cpu_tensors_raises():
    m = _sst()
    x = torch.zeros(7, 20)
    with pytest.raises(_lib.EchrHipError):
        m.forward_batch(x, [0, 3, 7])
    with pytest.raises(_lib.EchrHipError):
        m.forward_batch([x[:3], x[3:]])
    with pytest.raises(_lib.EchrHipError):
        VideoBatch.from_videos([_video(with_tap=False)], device='cpu', tap_model=m)


@pytest.mark.parametrize('ro', [[1, 3, 7], [0, 3, 3, 7], [0, 3, 6], [0, 3, 9], [0], [0, 5, 3, 7]])
def test_malformed_offsets_raise_value_error(ro):
    from echr_amd import functional as EF
    with pytest.raises(ValueError):
        EF.sst_row_offsets(ro, 7)
    assert EF.sst_row_offsets([0, 3, 7], 7).dtype == np.int32
    with pytest.raises(ValueError):          # the offsets are checked before anything touches a device
        _sst().forward_batch(torch.zeros(7, 20), ro)
    with pytest.raises(ValueError):
        _sst().forward_batch([torch.zeros(3, 20), torch.zeros(0, 20)])


def test_tap_criterion_batch_equals_the_per_video_sum():
    from echr_amd.misc import utils

    def crit(scores, masks, labels, w1):          # TAPModelCriterion's arithmetic (misc/utils.py:78-99) on host tensors
        y, p = labels * masks, scores * masks
        w = y * (1 - w1) + (1 - y) * w1
        bce = -(y * torch.log(p).clamp(min=-100) + (1 - y) * torch.log(1 - p).clamp(min=-100))
        return (w * bce).mean() * scores.shape[1]
    rs = np.random.RandomState(0)
    ro, K = [0, 4, 5, 12], 6
    scores = torch.from_numpy(rs.uniform(0.05, 0.95, size=(12, K)).astype(np.float32)).requires_grad_(True)
    masks = torch.from_numpy(rs.uniform(0.5, 1.0, size=(12, K)).astype(np.float32))          # positive: the host restatement keeps log() finite
    labels = torch.from_numpy((rs.uniform(size=(12, K)) > 0.7).astype(np.float32))
    w1 = torch.from_numpy(rs.uniform(0.05, 0.3, size=(K,)).astype(np.float32))
    total, per = utils.tap_criterion_batch(crit, scores, masks, labels, w1, ro)
    want = [crit(scores[a:b], masks[a:b], labels[a:b], w1) for a, b in zip(ro[:-1], ro[1:])]
    assert per.shape == (3,) and all(float(per[i].detach()) == float(want[i].detach()) for i in range(3))
    assert abs(float(total.detach()) - sum(float(w.detach()) for w in want)) < 1e-6 * abs(float(total.detach()))
    assert abs(float(total.detach()) - float(crit(scores, masks, labels, w1).detach())) > 1e-3          # NOT the mean over the concatenated rows
    total.backward()
    assert scores.grad is not None and torch.isfinite(scores.grad).all() and float(scores.grad.abs().sum()) > 0
    w1s = [w1, w1 * 2, w1]                                                            # one weight vector per video
    _, per2 = utils.tap_criterion_batch(crit, scores, masks, labels, w1s, np.asarray(ro))
    assert float(per2[0].detach()) == float(want[0].detach()) and float(per2[1].detach()) != float(want[1].detach())
    with pytest.raises(ValueError):
        utils.tap_criterion_batch(crit, scores, masks, labels, w1, [0, 4, 11])

"""Self-critical training over a multi-video batch on the host (no GPU): the CPU reference of the contract (tests/scst_batch_ref.py)
against the reference's own fixture, VideoBatch.reward_weights against VideoBatch.reward_criterion, the fixture's promised coverage, the
library symbol, and the entry points / refusals."""
import os
import re

import numpy as np
import pytest
import torch

from echr_amd import synth
from echr_amd.batch import VideoBatch
from echr_amd.misc.utils import RewardCriterion
from tests import scst_batch_ref as R
from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = 'vbscst'


@pytest.fixture(scope='module')
def case():
    opt, params, videos = synth.make_vbatch(CASE)
    g = U.gold('case_scst_batch.npz')
    return opt, params, videos, g, R.load_fixture(g, len(videos))


def _batch(videos):
    return VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi')} for v in videos])


def _rl_mask(gen):
    mask = np.zeros(gen.shape, dtype=bool)
    if gen.shape[1]:
        mask[:, 0] = True
        mask[:, 1:] = gen[:, :-1] > 0
    return mask


def test_case_shape_and_fixture_coverage(case):
    opt, params, videos, g, (gens, slps, greedys, rewards, losses) = case
    assert opt.CG_vocab_size + 1 == 31 and opt.CG_seq_length == 6 and len(videos) == 4
    assert all(3 <= len(v['soi']) <= 6 for v in videos)
    widths = [x.shape[1] for x in gens]
    words = [(x != 0).sum(1) for x in gens]
    T = max(widths)
    assert len(set(widths)) >= 2                                                         # two different video widths
    assert any(0 < w < T and int(r.max()) == w for w, r in zip(widths, words))           # a narrower video whose widest row has no <eos> inside
    assert any(w > 0 and int(r.min()) == 0 for w, r in zip(widths, words))               # a row that draws <eos> first
    assert abs(float(g['loss']) - float(np.sum(losses))) < 1e-12


def test_cpu_reference_reproduces_the_fixture(case):
    """The oracle once per video with sliced masks on [0 | gen_v | 0], gather, RewardCriterion, summed gradients -- at the
    oracle-vs-fixture tolerances of tests/test_oracle_golden.py."""
    opt, params, videos, g, (gens, slps, greedys, rewards, losses) = case
    ref = R.run(opt, params, videos, gens, rewards)
    for a, b, gen in zip(ref['slp'], slps, gens):
        if gen.shape[1]:
            assert np.abs(a - b)[_rl_mask(gen)].max() < 1e-5
    for a, b in zip(ref['greedy'], greedys):
        assert np.array_equal(a, b)
    assert np.abs(ref['losses'] - losses).max() < 1e-5 and abs(ref['loss'] - float(g['loss'])) < 1e-5
    for k, v in ref['grads'].items():
        gk = g.get('grad|' + k)
        if gk is None:
            assert v is None or float(np.abs(v).max()) == 0.0, k
        elif k in U.NOISE_ONLY:
            assert float(np.abs(v).max()) < 1e-6
        else:
            assert U.relerr(v, gk) < 1e-5, k


def _check_weights_against_criterion(b, gen, reward, seed):
    vw = b.caption_widths(gen)
    N, T = gen.shape[0], int(vw.max())
    labels, mask, w = b.reward_weights(gen, reward, vw)
    assert labels.shape == (N, T + 2) and labels.dtype == np.int64 and mask.shape == w.shape == (N, T + 1)
    assert np.array_equal(labels[:, 1:T + 1], gen[:, :T]) and not labels[:, 0].any() and not labels[:, -1].any()
    cols = np.arange(T + 1)[None, :]
    beyond = cols >= vw[b.vid][:, None]
    assert not mask[beyond].any() and not w[beyond].any()          # zero from the row's video's own width on
    slp = torch.from_numpy(np.random.RandomState(seed).uniform(-6.0, -0.1, size=(N, T))).to(torch.float64)
    total, per = b.reward_criterion(RewardCriterion(), slp, torch.from_numpy(gen), reward, vw)
    terms = -slp.numpy() * w[:, :T].astype(np.float64)
    # w is the float32 rounding of reward * mask / sum(mask): two roundings per term, 2^-23 relative each
    tol = 4 * 2.0 ** -23 * np.abs(terms).sum() + 1e-12
    assert abs(terms.sum() - float(total)) < tol
    for s, p in zip(b.event_slices, per):
        assert abs(terms[s].sum() - float(p)) < tol
    return vw, mask, per


def test_reward_weights_equal_reward_criterion_on_the_fixture(case):
    opt, params, videos, g, (gens, slps, greedys, rewards, losses) = case
    b = _batch(videos)
    gen, reward = R.stack(gens, videos, np.int64), R.stack(rewards, videos, np.float32)
    vw, mask, _ = _check_weights_against_criterion(b, gen, reward, 1)
    assert vw.tolist() == [x.shape[1] for x in gens]
    # the narrower video's widest row: non-zero at its last own column, and still no criterion position behind it
    v = int(np.argmin(vw))
    s = b.event_slices[v]
    n = s.start + int(np.argmax((gen[s] != 0).sum(1)))
    assert gen[n, vw[v] - 1] > 0 and vw[v] < gen.shape[1] and mask[n, vw[v]] == 0.0
    # per-caption rewards [N_tot] broadcast over the steps
    _check_weights_against_criterion(b, gen, np.random.RandomState(2).uniform(-1, 1, size=gen.shape[0]).astype(np.float32), 3)
    # with the fixture's own log-probs the per-video criterion is the fixture's per-video loss
    slp = torch.from_numpy(R.stack(slps, videos, np.float32))
    total, per = b.reward_criterion(RewardCriterion(), slp, torch.from_numpy(gen), reward, vw)
    assert np.abs(per.numpy() - losses).max() < 1e-6 and abs(float(total) - float(g['loss'])) < 1e-6


def test_reward_weights_with_a_width_zero_video(case):
    opt, params, videos, g, (gens, slps, greedys, rewards, losses) = case
    b = _batch(videos)
    gen = R.stack(gens, videos, np.int64)
    gen[b.event_slices[2]] = 0
    reward = np.random.RandomState(5).uniform(-1, 1, size=gen.shape).astype(np.float32)
    vw, mask, per = _check_weights_against_criterion(b, gen, reward, 7)
    assert vw[2] == 0 and float(per[2]) == 0.0 and not mask[b.event_slices[2]].any()
    with pytest.raises(ValueError):
        b.reward_weights(gen, reward, vw[:-1])
    with pytest.raises(ValueError):
        b.reward_criterion(RewardCriterion(), torch.zeros(gen.shape), gen, reward[:3], vw)


def test_symbol_is_declared_bound_and_exported():
    from echr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'echr_hip.h')).read()
    assert re.search(r'int echr_decoder_sample_train_batch\(const echr_sample_args\* \w+, const echr_dropout\* \w+, const echr_batch_ext\* \w+,\s*'
                     r'int32_t\* video_words,\s*void\* stream\);', hdr)
    assert 'echr_decoder_sample_train_batch' in [s[0] for s in _lib.SYMBOLS]
    fn = _lib.load().echr_decoder_sample_train_batch
    assert len(fn.argtypes) == 5 and fn.restype is _lib.i32
    # the existing entries keep their prototypes
    assert re.search(r'int echr_decoder_sample_batch\(const echr_sample_args\* \w+, const echr_batch_ext\* \w+, void\* stream\);', hdr)
    assert re.search(r'int echr_decoder_sample_train\(const echr_sample_args\* \w+, const echr_dropout\* \w+, void\* stream\);', hdr)


def test_entry_points_exist_and_old_refusals_name_them(case):
    import inspect
    import echr_amd
    from echr_amd import functional as EF
    from echr_amd.fused import FusedTrainStep, SelfCriticalBatchStep, SelfCriticalStep
    opt, params, videos = case[:3]
    assert list(inspect.signature(echr_amd.CaptionGenerator.train_rl_batch).parameters) == ['self', 'batch', 'gen_result', 'seed']
    assert list(inspect.signature(SelfCriticalBatchStep.__call__).parameters) == ['self', 'batch', 'gen_result', 'reward', 'step']
    assert list(inspect.signature(SelfCriticalBatchStep.__init__).parameters) == ['self', 'fused', 'reward_fn']
    assert callable(EF.sample_train_batch) and callable(VideoBatch.reward_criterion) and callable(VideoBatch.reward_weights)
    with pytest.raises(TypeError):
        SelfCriticalBatchStep(object())
    b = _batch(videos)
    m = echr_amd.CaptionGenerator(opt)
    with pytest.raises(NotImplementedError, match='train_rl_batch'):
        m.forward_batch(b, mode='train_rl')
    with pytest.raises(NotImplementedError, match='SelfCriticalBatchStep'):
        object.__new__(SelfCriticalStep).batch(b)
    # on CPU tensors the new module entry fails like every other mode, and the batch options stay refused
    with pytest.raises(EF.L.EchrHipError):
        m.train_rl_batch(b)
    opt2, _, _ = synth.make_vbatch(CASE)
    opt2.clip_context_type = 'CH'
    with pytest.raises(NotImplementedError):
        echr_amd.CaptionGenerator(opt2).train_rl_batch(b)
    opt3, _, _ = synth.make_vbatch(CASE)
    opt3.CG_init_feats_type = 'V'
    with pytest.raises(NotImplementedError):
        echr_amd.CaptionGenerator(opt3).train_rl_batch(b)
    s = SelfCriticalBatchStep(object.__new__(FusedTrainStep))
    s.fused.model = echr_amd.CaptionGenerator(opt3)
    s.fused.lib = EF.L.load()
    with pytest.raises(NotImplementedError):
        s(b)

"""CPU: echr_amd.batch.sampled_criterion (labels [0 | gen | 0], RewardCriterion's mask, reward * mask), VideoBatch.reward_weights on top
of it and the label helper -- bit for bit against the formulas the two self-critical steps carried before they shared it
(tests/sampled_criterion_ref.py), and against an independent float64 statement of RewardCriterion with both normalisations: the
single-video step passes reward * mask and divides by sum(mask) inside the step, the batch passes reward * mask / sum(mask of the video).

Shapes: the smallest that reach every place the function can go wrong -- T = 1, a row whose first token is 0, a row that never ends, a
video of width 0 between two live ones, a video narrower than the batch whose longest row would gain its <eos> column at the batch's
width, the reward as [N] and as [N, T' > T], a pinned single-video gen with a trailing all-zero column."""
import numpy as np
import pytest
import torch

from echr_amd.batch import VideoBatch, caption_labels, reward_matrix, sampled_criterion
from tests import sampled_criterion_ref as R
from tests import util as U

# video 0: width 2 < 4, its longest row has no <eos> inside its width, its other row draws <eos> first; video 1: width 0; video 2: a row
# that never ends
GEN = np.array([[5, 7, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 2, 3, 4], [3, 0, 0, 0], [2, 9, 0, 0]], np.int64)
ROWS, WIDTHS = [2, 2, 3], [2, 0, 4]
PINNED = np.array([[4, 2, 0], [0, 0, 0], [6, 0, 0]], np.int64)          # one video, given with a trailing all-zero column


def _batch(rows):
    b = object.__new__(VideoBatch)          # (reward_weights reads the event offsets only)
    b.event_offset, b.n_videos = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64), len(rows)
    return b


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _rewards(N, T, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(-2, 2, size=N).astype(np.float32), rs.uniform(-2, 2, size=(N, T)).astype(np.float32)


@pytest.mark.parametrize('gen,rows,widths', [(GEN, ROWS, WIDTHS), (np.array([[3], [0], [4]], np.int64), [1, 1, 1], [1, 0, 1]),
                                             (np.array([[0], [2]], np.int64), [2], [1])])
def test_batch_arrays_are_the_earlier_ones_and_the_criterion(gen, rows, widths):
    b = _batch(rows)
    N, T = gen.shape[0], max(widths)
    assert b.caption_widths(gen).tolist() == widths
    r1, r2 = _rewards(N, T + 2, 1)
    logp = np.random.RandomState(2).uniform(-6.0, -0.1, size=(N, T))
    for reward in (r1, r2[:, :T], r2):          # [N], [N, T], [N, T' > T]
        want = R.batch_step_arrays(gen, reward, widths, b.event_slices)
        _same(b.reward_weights(gen, reward, np.asarray(widths)), want)
        labels, mask, w = want
        # undivided, as the function itself returns it
        l0, m0, w0 = sampled_criterion(gen, reward, widths, b.event_slices)
        assert np.array_equal(l0, labels) and np.array_equal(m0, mask)
        assert np.array_equal(labels, np.pad(gen[:, :T], ((0, 0), (1, 1)))) and labels.dtype == np.int64
        rm = np.repeat(reward[:, None], T, 1) if reward.ndim == 1 else reward[:, :T]
        for v, (s, wv) in enumerate(zip(b.event_slices, widths)):
            assert not mask[s, wv:].any() and not w[s, wv:].any() and not w0[s, wv:].any()          # zero from the video's own width on
            assert np.array_equal(mask[s, :wv].astype(bool), U.rl_mask(gen[s, :wv])) if wv else True
            assert np.array_equal(w0[s, :wv], rm[s, :wv] * mask[s, :wv])
            if wv:
                loss, m64 = R.reward_criterion(logp[s, :wv], gen[s, :wv], rm[s, :wv])
                assert np.array_equal(m64, mask[s, :wv])
                terms = -logp[s, :wv] * w[s, :wv].astype(np.float64)
                assert abs(terms.sum() - loss) < 4 * 2.0 ** -23 * np.abs(terms).sum() + 1e-12          # two fp32 roundings per term


def test_narrower_video_keeps_its_eos_column_out():
    b = _batch(ROWS)
    _, mask, _ = b.reward_weights(GEN, np.ones(7, np.float32), np.asarray(WIDTHS))
    assert GEN[0, 1] > 0 and mask[0, 1] == 1.0 and mask[0, 2] == 0.0          # at the batch's width RewardCriterion would count column 2
    assert U.rl_mask(GEN)[0, 2] and not U.rl_mask(GEN, WIDTHS, np.repeat(np.arange(3), ROWS))[0, 2]


@pytest.mark.parametrize('gen', [PINNED, PINNED[:, :2], np.array([[7], [0]], np.int64), GEN[4:]])
def test_single_video_arrays_are_the_earlier_ones_and_the_criterion(gen):
    """One group at the width of the tensor it was given, a trailing all-zero column included."""
    N, T = gen.shape
    r1, r2 = _rewards(N, T, 3)
    logp = np.random.RandomState(4).uniform(-6.0, -0.1, size=(N, T))
    for reward in (r1, r2, torch.from_numpy(r1), torch.from_numpy(r2)):
        labels, mask, w, r = R.single_step_arrays(gen, np.asarray(reward))
        got = sampled_criterion(torch.from_numpy(gen), reward, [T], [slice(0, N)], 'single')
        _same(got, (labels, mask, w))
        assert np.array_equal(reward_matrix(reward, N, T, 'single'), r)
        assert np.array_equal(mask[:, :T].astype(bool), U.rl_mask(gen)) and not mask[:, T].any() and not w[:, T].any()
        loss, _ = R.reward_criterion(logp, gen, r)
        terms = -logp * w[:, :T].astype(np.float64)          # the step divides by sum(mask) itself
        assert abs(terms.sum() / mask.sum(dtype=np.float64) - loss) < 4 * 2.0 ** -23 * np.abs(terms).sum() + 1e-12


def test_reward_shapes_that_are_refused():
    b = _batch(ROWS)
    N, T = 7, 4
    for bad in (np.zeros(N + 1, np.float32), np.zeros((N, T - 1), np.float32), np.zeros((N + 1, T), np.float32)):
        with pytest.raises(ValueError, match=r'reward must be \[N_tot, T\] or \[N_tot\] \(got .* for gen_result \(7, 4\)\)'):
            b.reward_weights(GEN, bad, np.asarray(WIDTHS))
        with pytest.raises(ValueError, match=r'reward must be \[N, T\] or \[N\] \(got .* for gen_result \(7, 4\)\)'):
            sampled_criterion(GEN, bad, [T], [slice(0, N)], 'single')
    with pytest.raises(ValueError, match=r'reward must be \[N, T\] or \[N\]'):          # the single-video form takes no wider reward
        reward_matrix(np.zeros((N, T + 1), np.float32), N, T, 'single')
    assert reward_matrix(np.zeros((N, T + 1), np.float32), N, T).shape == (N, T)
    with pytest.raises(ValueError, match=r'reward_fn must return \[N_v, T_v\] or \[N_v\] \(got \(2, 3\) for a video of \(2, 2\)\)'):
        reward_matrix(np.zeros((2, 3)), 2, 2, 'video')
    # a pinned single-video gen_result with a row more than the reward: the refusal names the tensor's own rows (a reward with the tensor's
    # rows passes here; FusedTrainStep._setup then refuses the labels' row count: tests/test_gpu_scst_unify.py)
    with pytest.raises(ValueError, match=r'reward must be \[N, T\] or \[N\] \(got \(3, 3\) for gen_result \(4, 3\)\)'):
        reward_matrix(np.zeros(3, np.float32), 4, 3, 'single')
    assert sampled_criterion(np.ones((4, 3), np.int64), np.zeros(4, np.float32), [3], [slice(0, 4)], 'single')[0].shape == (4, 5)
    with pytest.raises(ValueError, match='gen_result must be .7 events, T. and video_words .3.'):
        b.reward_weights(GEN[:-1], np.zeros(6, np.float32), np.asarray(WIDTHS))
    with pytest.raises(ValueError, match='gen_result must be'):
        b.reward_weights(GEN, np.zeros(7, np.float32), np.asarray(WIDTHS[:-1]))
    with pytest.raises(ValueError, match=r'video_words \[2, 0, 5\] exceed gen_result \(7, 4\)'):
        b.reward_weights(GEN, np.zeros(7, np.float32), np.asarray([2, 0, 5]))


def test_caption_labels_on_numpy_and_torch():
    want = np.pad(PINNED, ((0, 0), (1, 1)))
    got = caption_labels(PINNED)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)
    for t in (torch.from_numpy(PINNED), torch.from_numpy(PINNED.astype(np.int32)), torch.from_numpy(PINNED).to('meta')):
        got = caption_labels(t)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and got.device == t.device and tuple(got.shape) == (3, 5)
        if t.device.type == 'cpu':
            assert np.array_equal(got.numpy(), want)
    assert caption_labels(np.zeros((2, 0), np.int64)).shape == (2, 2)

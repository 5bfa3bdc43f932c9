"""The token-selection references (tests/select_ref.py) checked on the host, without a GPU: the conditions on the inputs of every
multinomial case tests/test_gpu_select.py runs, the checker against a float32 emulation of the device arithmetic, the checker's power
(five planted mistakes are rejected), the Philox sampling site, and the tie designs against the host beam search."""
import functools

import numpy as np
import pytest

from echr_amd import philox
from tests import select_ref as R

L = R.SEQ_LEN
# the distinct (kind, V1, N) behind the GPU cases (the entry does not change the inputs; rows are keyed batch-globally)
INPUTS = sorted({(kind, V1, N) for _, N, V1, kind in R.MULTINOMIAL_PARAMS})


@functools.lru_cache(maxsize=None)
def _design(V1, kind):
    return R.bias_design(V1, kind, V1)


def test_sample_u24_is_the_philox_word_of_the_sampling_site():
    """word >> 8 of element = row at site 6, offset 0, both key words used; rows 4 k .. 4 k + 3 are the four words of one counter."""
    assert philox.SITE_SAMPLE == 6
    seed = 0x5EED0123456789
    u = philox.sample_u24(9, 3, seed)
    assert u.shape == (9, 3) and u.dtype == np.int64 and u.min() >= 0 and u.max() < 1 << 24
    for t in range(3):
        for c0 in range(3):
            w = philox.philox4x32_10(np.array([c0]), t, 6, 0, seed & 0xFFFFFFFF, seed >> 32)
            for k in range(4):
                if 4 * c0 + k < 9:
                    assert u[4 * c0 + k, t] == int(w[k][0]) >> 8
    assert not np.array_equal(u, philox.sample_u24(9, 3, seed & 0xFFFFFFFF))          # the high key word matters
    assert np.array_equal(philox.sample_u24(5, 2, seed), u[:5, :2])                    # counter-based: a prefix is a prefix


@pytest.mark.parametrize('kind,V1,N', INPUTS)
def test_input_conditions_and_checker_accepts_the_emulation(kind, V1, N):
    """For every (design, V1, temperature, seed) of the GPU cases: near-boundary share <= 5 %, observable share, marked-token share (the
    float64 replay alone), and check_draws accepts the float32 emulation of the device arithmetic."""
    bias, marked = _design(V1, kind)
    for T in R.TEMPERATURES + ((0.0,) if (kind, V1, N) == ('edges', 2049, 64) else ()):
        for seed in R.SEEDS:
            ref = R.replay_multinomial(bias, T, seed, N, L)
            R.input_conditions(ref, marked, kind)
            got = R.emitted(R.draw_f32(bias, T, philox.sample_u24(N, L, seed)))
            c = R.check_draws(got, ref)
            assert c['bad_a'] == 0 and c['bad_b'] == 0, (T, seed, c)
            assert c['worst'] < R.DELTA and c['differ'] <= c['near']
            assert np.array_equal(got[~ref['near'] & ref['observable']], ref['seq'][~ref['near'] & ref['observable']])


def test_replay_bookkeeping():
    """seq / observable / n_unfinished / T_out / video_words of the replay on a decode whose rows end at different steps."""
    bias, _ = _design(2049, 'eos')
    vid = np.repeat([0, 1, 2], [20, 1, 43])
    ref = R.replay_multinomial(bias, 1.0, 11, 64, L, vid=vid)
    tok, seq = ref['tok'], ref['seq']
    for n in range(64):
        z = np.nonzero(tok[n] == 0)[0]
        end = int(z[0]) if len(z) else L
        assert np.array_equal(seq[n, :end], tok[n, :end]) and not seq[n, end:].any()
        assert ref['observable'][n].tolist() == [t <= end for t in range(L)]
    words = (seq != 0).sum(1)
    assert ref['n_unfinished'][1:].tolist() == [(words > t).sum() for t in range(L)]
    assert ref['T_out'] == words.max() < L
    assert ref['video_words'].tolist() == [words[:20].max(), words[20], words[21:].max(), words.max()]
    x = bias.astype(np.float64)
    assert np.allclose(ref['logp'], (x - np.log(np.exp(x).sum()))[tok], atol=1e-12)
    assert R.inv_temperature(0.0) == 1.0 and R.inv_temperature(-1.0) == 1.0 and R.inv_temperature(0.7) == float(np.float32(1) / np.float32(0.7))


def test_sparse_design_leaves_whole_chunks_without_mass():
    for V1 in (2049, 12289):
        bias, live = _design(V1, 'sparse')
        CH, _ = R.chunking(V1)
        assert 10 <= len(live) <= 14 and bias[0] == np.float32(R.ZERO_MASS)
        mass = np.zeros(256)
        np.add.at(mass, np.arange(V1) // CH, np.exp(bias.astype(np.float64) * 1.0))
        assert (mass[201:] == 0).all() and (mass == 0).sum() > 240 and (np.array(live) % CH == CH // 2).any()
        assert np.exp(np.float32((np.float32(R.ZERO_MASS) - bias.max()) * np.float32(1 / 0.7))) == 0.0


MUT = dict(V1=2049, T=0.7, seed=11, N=64)


@pytest.mark.parametrize('mutation', ['pick_plus_one', 'ch_floor', 'strided', 'no_temp_walk', 'row_plus_one'])
def test_checker_rejects_a_planted_mistake(mutation):
    """One mistake planted in the emulation -- pick + 1, CH = V1 // 256, strided chunk ownership, the temperature left out of the walk, the
    Philox word of element row + 1 -- and check_draws reports violations (V1 = 2049, T = 0.7: the sizes at which each of them matters)."""
    bias, _ = _design(MUT['V1'], 'edges')
    ref = R.replay_multinomial(bias, MUT['T'], MUT['seed'], MUT['N'], L)
    if mutation == 'row_plus_one':
        picks = R.draw_f32(bias, MUT['T'], philox.sample_u24(MUT['N'] + 1, L, MUT['seed'])[1:])
    else:
        picks = R.draw_f32(bias, MUT['T'], philox.sample_u24(MUT['N'], L, MUT['seed']), mutate=mutation)
    c = R.check_draws(R.emitted(picks), ref)
    assert c['bad_a'] + c['bad_b'] > 0, c
    assert c['bad_a'] > 0.05 * c['observable'], c          # not a marginal rejection: rule (a) alone fails on a visible share of the draws


def test_checker_rejects_an_out_of_range_token():
    bias, _ = _design(257, 'edges')
    ref = R.replay_multinomial(bias, 1.0, 11, 64, L)
    got = ref['seq'].copy()
    got[0, 0] = 257
    assert R.check_draws(got, ref)['bad_a'] == 1
    assert R.check_draws(ref['seq'], ref) == dict(observable=int(ref['observable'].sum()), near=int((ref['near'] & ref['observable']).sum()),
                                                  differ=0, bad_a=0, bad_b=0, worst=0.0)


@pytest.mark.parametrize('V1', [2048, 2049, 5001, 5121, 10241, 12289])
def test_greedy_tie_designs(V1):
    for kind in ('ties', 'ties_high', 'ties_far', 'negative', 'eos_tie'):
        b, want, tied = R.greedy_ties_design(V1, kind)
        assert b.dtype == np.float32 and b.shape == (V1,)
        assert want == int(np.argmax(b)) == tied[0]          # numpy's arg-max takes the first maximum too
        assert (b == b.max()).sum() == len(tied) >= 1 and np.isfinite(b).all()
        if kind in ('ties', 'negative'):
            assert want == 79 and 80 in tied and 159 in tied and V1 - 1 in tied and (5199 in tied) == (V1 > 5199)
        if kind == 'negative':
            assert b.max() == -50.0 and b.min() >= -60.0 and np.sort(b)[-len(tied) - 1] <= -51.0
        if kind == 'ties_high':
            assert want == 159
        if kind == 'ties_far':
            assert want >= 256 and want == (5199 if V1 > 5199 else V1 - 1)
        if kind == 'eos_tie':
            assert want == 0


@pytest.mark.parametrize('V1', [512, 513, 2049, 5121])
@pytest.mark.parametrize('B', [1, 3, 16])
def test_beam_designs_are_decided_by_the_tie_rules(V1, B):
    """The reference search on the class designs: every step's winners are the smallest alive slot's children, tokens ascending, so the
    result is X's smallest token at every position; the margin between the last kept and the first dropped candidate is exactly 0."""
    N = 2
    b, Ls = R.beam_class_design(V1, B, 'one')
    X = np.nonzero(b == b.max())[0]
    assert len(X) == 2 * B + 3 and V1 - 1 in X and 0 not in X and np.sort(b)[-len(X) - 1] <= b.max() - 30
    r = R.beam_reference(b, N, B, Ls)
    assert r['words'].tolist() == [Ls] * N and (r['seq'] == X[0]).all()
    assert (r['margin'] == 0).all()          # the B-th kept and the best dropped candidate tie at every step: only the rule decides
    b, Ls = R.beam_class_design(V1, B, 'one_eos')
    X = np.nonzero(b == b.max())[0]
    assert len(X) == 2 * B + 3 and X[0] == 0 and V1 - 1 in X
    r = R.beam_reference(b, N, B, Ls)
    assert r['words'].tolist() == [0] * N and r['seq'].shape == (N, 0)
    if B > 1:
        b, Ls = R.beam_class_design(V1, B, 'two')
        X, Y = np.nonzero(b == b.max())[0], np.nonzero(b == b.max() - np.float32(1.5))[0]
        assert Ls == 2 and len(X) == 2 and len(Y) == 2 * B
        r = R.beam_reference(b, N, B, Ls)
        assert r['words'].tolist() == [2] * N and (r['seq'] == X[0]).all()
        if B > 2:
            assert (r['margin'] == 0).all()

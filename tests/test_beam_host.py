"""Beam search on the host side: the host reference (tests/beam_ref.py) on a hand-built log-prob table, the new ABI entry points, and the
argument checks that run before any GPU work."""
import ctypes as C

import numpy as np
import pytest
import torch

import echr_amd
from echr_amd import synth
from tests import beam_ref

# log-prob rows by (step, token fed); token 0 is <bos> / <eos>.  Dyadic values: float64 sums are exact.
TABLE = {
    (0, 0): [-3.0, -1.0, -1.0, -2.0],          # a tie between tokens 1 and 2
    (1, 1): [-0.5, -4.0, -3.0, -2.0],          # the slot on token 1 ends early (<eos> at step 1)
    (1, 2): [-4.0, -3.0, -4.0, -0.25],
    (2, 3): [-1.0, -0.125, -2.0, -2.0],        # ... and is overtaken at the last step
}


def _table_step(it, state):
    (tt,) = state                                              # [1, rows, 1]: the step, carried like a decoder state
    t = int(tt[0, 0, 0])
    rows = [TABLE.get((t, int(v)), [-5.0, -6.0, -7.0, -8.0]) for v in it]
    return torch.tensor(rows, dtype=torch.float64), (tt + 1,)


def _run(B, N=1, L=3):
    return beam_ref.beam_search(_table_step, (torch.zeros(1, N * B, 1),), N, B, L)


def test_beam_ref_known_answer():
    r = _run(2)
    # t0: tie -> slot 0 = token 1, slot 1 = token 2 (-1 each).  t1: -1.25 (slot 1, token 3) and -1.5 (slot 0, <eos>: finished, 1 word).
    # t2 (last): -1.375 (token 1) beats -1.5 and replaces the result; -2.25 (<eos>) does not.
    assert r['seq'].tolist() == [[2, 3, 1]]
    assert r['words'].tolist() == [3]
    assert r['score'].tolist() == [-1.375]
    assert r['logp'].tolist() == [[-1.0, -0.25, -0.125]]
    assert r['margin'].tolist() == [0.125]                       # result -1.375 against the runner-up finished hypothesis -1.5


def test_beam_ref_early_finisher_keeps_eos_logp_and_zeros():
    global TABLE
    saved = dict(TABLE)
    try:
        TABLE[(2, 3)] = [-1.0, -0.5, -2.0, -2.0]                # now nothing at the last step beats the early finisher (-1.75 < -1.5)
        r = _run(2)
        assert r['seq'].tolist() == [[1]] and r['words'].tolist() == [1]
        assert r['score'].tolist() == [-1.5]
        assert r['logp'].tolist() == [[-1.0]]                  # <eos> sits at position w = 1 = T: outside the output
    finally:
        TABLE = saved


def test_beam_ref_b1_is_greedy():
    r = _run(1, N=3)
    # greedy: arg-max with the lowest index on ties -> token 1, then <eos>
    assert r['seq'].tolist() == [[1]] * 3
    assert r['score'].tolist() == [-1.5] * 3
    assert r['words'].tolist() == [1] * 3


def test_beam_ref_matches_greedy_oracle_on_fixture():
    """B = 1 over the CPU oracle decodes the reference's greedy captions of the fixture (tests/golden/case_vctx.npz)."""
    from tests import util as U
    opt, params, vid = synth.make_case('vctx')
    g = U.gold('case_vctx.npz')
    r = beam_ref.oracle_beam(opt, params, vid, 1)
    assert np.array_equal(r['seq'], g['sample|seq'])
    T = r['seq'].shape[1]
    for n in range(r['seq'].shape[0]):
        w = r['words'][n]
        m = min(w + 1, T)
        assert np.abs(r['logp'][n, :m] - g['sample|logp'][n, :m]).max() < 1e-4
    resc, words = beam_ref.oracle_rescore(opt, params, vid, r['seq'])
    assert np.allclose(resc, r['score'], rtol=1e-9, atol=1e-9)


def test_library_exports_beam_entry_points():
    from echr_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, 'echr_decoder_beam') and hasattr(lib, 'echr_beam_ws_floats')
    assert lib.echr_abi_sizeof(b'echr_beam_args') == C.sizeof(_lib.BeamArgs) > C.sizeof(_lib.DecArgs)
    bad = _lib.BeamArgs()
    bad.beam_size, bad.seq_len = 3, 5
    bad.dec.N = 7                                              # not events * beam_size
    assert lib.echr_beam_ws_floats(C.byref(bad)) == -1
    assert lib.echr_decoder_beam(C.byref(bad), None) != 0      # refused before any device work


def test_sample_rejects_bad_beam_options():
    opt = synth.default_opt(vocab_size=30, seq_length=5)
    m = echr_amd.CaptionGenerator(opt)
    lm = m.lm_model
    for o in ({'beam_size': 17}, {'beam_size': 0}, {'beam_size': 3, 'sample_max': 0}):
        with pytest.raises(ValueError):
            lm.eval().sample(None, None, None, None, o)
    with pytest.raises(ValueError):
        lm.train().sample(None, None, None, None, {'beam_size': 3})
    small = echr_amd.CaptionGenerator(synth.default_opt(vocab_size=3, seq_length=5)).lm_model.eval()
    with pytest.raises(ValueError):
        small.sample(None, None, None, None, {'beam_size': 5})          # B > V1 = 4
    for mode in ('train', 'train_rl'):
        with pytest.raises(ValueError):
            m(None, None, None, None, None, None, mode=mode, beam_size=3)

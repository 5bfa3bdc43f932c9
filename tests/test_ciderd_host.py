"""CIDEr-D on the host side (no GPU): the oracle's closed-form anchors, echr_amd.reward's corpus table and reference packing against the
oracle, the refusals, and the new ABI surface."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from echr_amd import reward as RW
from tests import ciderd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle against closed forms ----------------------------------------------------------------------------------------------
def _two_docs():
    docs = [[R.sequence([5, 0], 4)], [R.sequence([6, 0], 4)]]
    assert docs[0] == [(5, 0)]
    return docs, R.document_frequency(docs)


def test_anchor_repeated_unigram():
    docs, (df, n) = _two_docs()
    want = 10.0 * (0.5 + 1.0 / math.sqrt(2.0)) / 4.0 * math.exp(-1.0 / 72.0)
    assert abs(want - 2.9761432457) < 1e-9
    assert abs(R.score((5, 5, 0), docs[0], df, n) - want) < 1e-12


def test_anchor_equal_to_reference_with_two_orders():
    docs, (df, n) = _two_docs()
    assert abs(R.score((5, 0), docs[0], df, n) - 5.0) < 1e-12          # orders 1 and 2 exist, 3 and 4 do not


def test_anchor_nothing_shared():
    docs, (df, n) = _two_docs()
    assert R.sequence([7, 7, 7, 7], 4) == (7, 7, 7, 7)                   # l = L: no end token
    assert R.score((7, 7, 7, 7), docs[0], df, n) == 0.0


def test_anchor_single_document_corpus_scores_zero():
    docs = [[(5, 6, 7, 0), (5, 5, 0)]]
    df, n = R.document_frequency(docs)
    for cand in [(5, 6, 7, 0), (5, 0), (9, 9, 9, 9), (0,)]:
        s = R.score(cand, docs[0], df, n)
        assert s == 0.0 and not math.isnan(s)


def test_anchor_candidate_equal_to_its_reference_scores_ten():
    docs = [[(5, 6, 7, 0)], [(8, 9, 3, 0)]]
    df, n = R.document_frequency(docs)
    assert abs(R.score((5, 6, 7, 0), docs[0], df, n) - 10.0) < 1e-12


# ---- the table --------------------------------------------------------------------------------------------------------------------
def _random_docs(rs, n_docs, L, top, label_rows):
    docs = []
    for _ in range(n_docs):
        doc = []
        for _ in range(rs.randint(1, 4)):
            words = rs.randint(1, top + 1, size=rs.randint(0, L + 1)).tolist()
            doc.append([0] + words + [0] * rs.randint(0, 3) if label_rows else words + [0] if len(words) < L and rs.rand() < 0.5 else words)
        docs.append(doc)
    return docs


@pytest.mark.parametrize('label_rows', [True, False])
def test_table_equals_the_oracles_document_frequency(label_rows):
    rs = np.random.RandomState(3)
    L, top = 6, 9
    docs = _random_docs(rs, 40, L, top, label_rows)
    seqs = [[R.label_sequence(r, L) if label_rows else R.sequence(r, L) for r in doc] for doc in docs]
    df, n = R.document_frequency(seqs)
    sc = RW.CiderD.from_corpus(docs, L, top)
    assert sc.n_docs == n == 40 and sc.keys.dtype == np.uint64
    assert (sc.keys[1:] > sc.keys[:-1]).all()
    got = {RW.unpack_key(k): int(d) for k, d in zip(sc.keys, sc.df)}
    assert len(got) == len(sc.keys)                      # every key decodes to its own tuple
    assert got == dict(df)
    for k in sc.keys:                                    # and packs back to itself
        t = RW.unpack_key(k)
        assert RW.pack_keys(t, len(t)).tolist() == [int(k)]
    want = np.asarray([math.log(n) - math.log(max(1, df[RW.unpack_key(k)])) for k in sc.keys])
    assert np.array_equal(sc.idf(), want) or np.abs(sc.idf() - want).max() < 1e-15


def test_key_order_with_the_top_bit_set():
    """token ids >= 32767 in the fourth field set bit 63: the order must be the unsigned one."""
    L, top = 5, 39999
    docs = [[[39999, 39998, 39997, 39996, 3]], [[1, 2, 3, 32767]], [[1, 2, 3, 32766, 0]], [[40, 0]]]
    sc = RW.CiderD.from_corpus(docs, L, top)
    assert int(sc.keys.max()) >> 63 == 1
    assert (sc.keys[1:] > sc.keys[:-1]).all()
    as_int = [int(k) for k in sc.keys]
    assert as_int == sorted(as_int)                      # python ints: the unsigned order
    assert not (sc.keys.view(np.int64)[1:] > sc.keys.view(np.int64)[:-1]).all()          # the signed order differs: this case can tell
    df, n = R.document_frequency([[R.sequence(r, L) for r in d] for d in docs])
    assert {RW.unpack_key(k): int(d) for k, d in zip(sc.keys, sc.df)} == dict(df)
    sd = sc.state_dict()
    assert sd['keys'].dtype == torch.int64
    back = RW.CiderD.from_state_dict(sd)
    assert np.array_equal(back.keys, sc.keys) and back.keys.dtype == np.uint64


def test_state_dict_round_trip():
    rs = np.random.RandomState(5)
    sc = RW.CiderD.from_corpus(_random_docs(rs, 12, 6, 9, True), 6, 9)
    sd = sc.state_dict()
    assert set(sd) == {'keys', 'df', 'n_docs', 'seq_length', 'vocab_size'}
    other = RW.CiderD.from_corpus([[[1, 0]]], 3, 4).load_state_dict(sd)
    for a in (other, RW.CiderD.from_state_dict(sd)):
        assert np.array_equal(a.keys, sc.keys) and np.array_equal(a.df, sc.df)
        assert (a.n_docs, a.seq_length, a.vocab_size) == (sc.n_docs, 6, 9)


# ---- pack_refs against the sequence rule ------------------------------------------------------------------------------------------
def test_pack_refs_follows_the_sequence_rule():
    L = 4
    sets = [[[0, 5, 6, 7, 8]],                            # l = L: no end token
            [[0, 0, 0, 0]],                               # l = 0: [0]
            [[0, 5, 6, 0, 0, 0, 0, 0], [0, 5, 6]],        # the same caption cut wide and cut narrower than the batch
            [[0, 9, 0], [0, 9, 8, 0], [0, 9, 8, 7, 0]]]
    p = RW.pack_refs(sets, L)
    assert p.refs.dtype == p.ref_len.dtype == p.ref_offset.dtype == torch.int32
    assert p.ref_offset.tolist() == [0, 1, 2, 4, 7]
    flat = [r for s in sets for r in s]
    for row, n, lab in zip(p.refs.tolist(), p.ref_len.tolist(), flat):
        want = R.label_sequence(lab, L)
        assert tuple(row[:n]) == want and not any(row[n:])
    assert p.refs[0].tolist() == [5, 6, 7, 8] and p.ref_len[0] == 4
    assert p.refs[1].tolist() == [0, 0, 0, 0] and p.ref_len[1] == 1
    assert p.refs[2].tolist() == p.refs[3].tolist() == [5, 6, 0, 0] and p.ref_len[2] == p.ref_len[3] == 3


def test_candidate_sequence_is_independent_of_the_cut():
    L = 6
    for row in ([3, 4, 0, 0, 0, 0], [3, 4, 0], [3, 4]):          # <eos> inside, at the cut's edge, and cut away with the all-zero column
        assert R.sequence(row, L) == (3, 4, 0)
    assert R.sequence([1, 2, 3, 4, 5, 6], L) == (1, 2, 3, 4, 5, 6)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    with pytest.raises(ValueError):
        RW.CiderD.from_corpus([[[1, 0]]], 4, 65535)           # V1 = 65536
    RW.CiderD.from_corpus([[[1, 0]]], 4, 65534)               # V1 = 65535 fits
    with pytest.raises(ValueError):
        RW.CiderD.from_corpus([[[1, 0]]], 64, 10)
    RW.CiderD.from_corpus([[[1, 0]]], 63, 10)
    with pytest.raises(ValueError):
        RW.CiderD.from_corpus([[[1, 0]], []], 4, 10)          # a document without a reference
    with pytest.raises(ValueError):
        RW.pack_refs([[[0, 1, 0]], []], 4)                    # an event without a reference
    with pytest.raises(ValueError):
        RW.pack_refs([[[0, 11, 0]]], 4, vocab_size=10)        # a token outside the vocabulary
    with pytest.raises(ValueError):
        RW.pack_refs([[[0, -1, 0]]], 4)
    with pytest.raises(ValueError):
        RW.pack_refs([[[0, 65535, 0]]], 4)
    with pytest.raises(ValueError):
        RW.CiderD([2, 1], [1, 1], 2, 4, 10)                   # keys out of order
    with pytest.raises(TypeError):
        RW.CiderDReward(lambda a, b: 0)


def test_cpu_captions_are_refused():
    from echr_amd._lib import EchrHipError
    sc = RW.CiderD.from_corpus([[[1, 0]], [[2, 0]]], 4, 10)
    refs = sc.pack_refs([[[0, 1, 0]]])
    with pytest.raises(EchrHipError):
        sc.score(torch.tensor([[1, 0]]), refs)
    with pytest.raises(EchrHipError):
        sc.reward(torch.tensor([[1, 0]]), torch.tensor([[2, 0]]), refs)


def test_the_steps_refs_rules():
    sc = RW.CiderD.from_corpus([[[1, 0]], [[2, 0]]], 4, 10)
    rw = RW.CiderDReward(sc, weight=0.5)
    refs = sc.pack_refs([[[0, 1, 0]]])
    with pytest.raises(TypeError):
        RW.check_reward_refs(lambda gen, greedy: 0.0, refs)           # refs with a plain callable
    with pytest.raises(TypeError):
        RW.check_reward_refs(None, refs)
    with pytest.raises(ValueError):
        RW.check_reward_refs(rw, None)                                 # CiderDReward without refs
    assert RW.check_reward_refs(rw, refs) is True
    assert RW.check_reward_refs(rw, None, reward=np.zeros(1)) is False          # reward= pins the reward: today's path
    assert RW.check_reward_refs(lambda gen, greedy: 0.0, None) is False
    # the step objects apply the rules before they touch the device
    import inspect
    from echr_amd import fused
    assert inspect.signature(fused.SelfCriticalStep.__call__).parameters['refs'].default is None
    assert inspect.signature(fused.SelfCriticalBatchStep.handover).parameters['refs'].default is None
    # the batch step's call keeps its parameter list (tests/test_scst_batch_host.py pins it): the references travel as VideoBatch.refs
    from echr_amd.batch import VideoBatch
    assert 'refs' not in inspect.signature(fused.SelfCriticalBatchStep.__call__).parameters
    assert 'refs' in VideoBatch.__doc__


# ---- ABI --------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    from echr_amd import _lib, build
    assert 'reward.hip' in build.SOURCES
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'echr_hip.h')).read()
    declared = set(re.findall(r'\b(echr_[a-z0-9_]+)\s*\(', hdr))
    bound = {s[0] for s in _lib.SYMBOLS}
    assert 'echr_ciderd_score' in declared and 'echr_ciderd_score' in bound and hasattr(lib, 'echr_ciderd_score')
    assert 'echr_ciderd_args' in hdr and _lib.ABI_STRUCTS['echr_ciderd_args'] is _lib.CiderdArgs
    assert lib.echr_abi_sizeof(b'echr_ciderd_args') == C.sizeof(_lib.CiderdArgs) > 0
    assert lib.echr_version() == _lib.ABI_VERSION == 3


def test_entry_point_validates_before_any_launch():
    """The argument checks run on the host ahead of the launch: they need no GPU."""
    from echr_amd import _lib
    lib = _lib.load()
    a = _lib.CiderdArgs()
    a.N, a.L = 1, 64
    assert lib.echr_ciderd_score(C.byref(a), None) == -22 and b'seq_length' in lib.echr_last_error()
    a.L, a.T = 8, 9
    assert lib.echr_ciderd_score(C.byref(a), None) == -22 and b'width' in lib.echr_last_error()
    a.T, a.n_keys = 8, 3
    assert lib.echr_ciderd_score(C.byref(a), None) == -22 and b'table' in lib.echr_last_error()
    a.n_keys, a.N = 0, 0
    assert lib.echr_ciderd_score(C.byref(a), None) == 0          # no rows: nothing to launch

"""Dense-caption scoring on the host side (no GPU): hand anchors on the oracle tests/densecap_ref.py, the ground-truth packer and its
refusals, and the new ABI surface with its argument checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import densecap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(pred, caps, gts, refs, tious=(0.5,)):
    return R.evaluate(pred, [0, len(pred)], caps, gts, [0, len(gts)], refs, tious)


# ---- the oracle against hand values -----------------------------------------------------------------------------------------------
def test_anchor_prediction_equal_to_its_ground_truth():
    cap = [4, 5, 6, 7, 8, 0, 0]
    o = _one([[1.0, 9.0]], [cap], [[1.0, 9.0]], [cap])
    assert o['pairs'] == [[(0, 0)]]
    m1, m2, m3, m4, lc, lr, l = o['stats'][0][0]
    assert (lc, lr, l) == (5, 5, 5)
    assert [m1, m2, m3, m4] == [5, 4, 3, 2]                      # match_n = guess_n
    assert o['ROUGE_L'][0] == 1.0
    for n in R.ORDERS:
        assert abs(o['Bleu_%d' % n][0] - 1.0) < 1e-9
    assert o['Precision'] == [1.0] and o['Recall'] == [1.0] and o['f1'] == [1.0]


def test_anchor_clipping_and_lcs():
    assert R.pair_stats([5, 5, 5, 5], [5, 5])[0] == 2            # tf 4 clipped to the reference's 2
    assert R.pair_stats([5, 5, 5, 5], [5, 5])[1] == 1            # (5, 5): tf 3 against 1
    assert R.pair_stats([1, 2, 3, 4], [1, 3, 4, 2])[6] == 3
    assert R.lcs([], [1]) == 0 and R.lcs([1, 2], [2, 1]) == 1
    assert R.words([3, 4, 0, 9]) == [3, 4] and R.words([3, 4]) == [3, 4] and R.words([0, 3]) == []
    assert R.key((1, 2)) == 2 | (3 << 16) and R.key((0,)) == 1


@pytest.mark.parametrize('n', [0, 1, 2, 3])
def test_anchor_short_candidates_miss_orders(n):
    cand = [7, 8, 9][:n]
    o = _one([[0.0, 10.0]], [cand + [0]], [[0.0, 10.0]], [[7, 8, 9, 3]])
    st = o['stats'][0][0]
    assert st[:4] == tuple(max(n - k + 1, 0) for k in R.ORDERS) and st[4:] == (n, 4, n)
    # an order without an n-gram has guess 0: p = 1e-15 / 1e-9
    c, r = n, 4
    bp = math.exp(1.0 - 1.0 / ((c + 1e-15) / (r + 1e-9)))
    prod = 1.0
    for k in R.ORDERS:
        g = max(n - k + 1, 0)
        prod *= (g + 1e-15) / (g + 1e-9)
        want = prod ** (1.0 / k) * bp
        assert o['Bleu_%d' % k][0] == want
        if k > n:
            assert o['Bleu_%d' % k][0] < 0.05
    if n == 0:
        assert o['Bleu_1'][0] == 0.0 and o['ROUGE_L'][0] == 0.0
    else:
        P, Rc = 1.0, n / 4.0
        assert abs(o['ROUGE_L'][0] - (1 + 1.44) * P * Rc / (Rc + 1.44 * P)) < 1e-12


def test_anchor_video_without_prediction_scores_zero():
    o = R.evaluate([[0.0, 4.0]], [0, 0, 1], [[3, 4, 0]], [[0.0, 5.0], [0.0, 4.0]], [0, 1, 2], [[3, 0], [3, 4, 0]], (0.3, 0.9))
    for name in R.SCORES:
        assert [row[0] for row in o['video'][name]] == [0.0, 0.0], name
    assert [row[0] for row in o['n_pairs']] == [0, 0]
    assert o['video']['ROUGE_L'][0][1] == 1.0 and o['ROUGE_L'][0] == 0.5          # the mean runs over both videos
    assert o['Recall'] == [0.5, 0.5] and o['Precision'] == [0.5, 0.5]


def test_anchor_nothing_matches_at_the_high_threshold():
    pred = [[0.0, 5.0], [2.0, 8.0], [20.0, 30.0]]
    gts = [[0.0, 10.0], [5.0, 10.0]]
    o = _one(pred, [[3, 4, 5, 0], [3, 0, 0, 0], [6, 7, 0, 0]], gts, [[3, 4, 5, 6], [3, 4, 0, 0]], (0.9,))
    assert o['pairs'][0] == [(0, -1), (1, -1), (2, -1)] and o['n_unmatched'] == [[3]]
    assert all(s[:4] == (0, 0, 0, 0) and s[5] == 1 and s[6] == 0 for s in o['stats'][0])
    assert o['ROUGE_L'] == [0.0] and o['Precision'] == [0.0] and o['Recall'] == [0.0] and o['f1'] == [0.0]
    # c = 3 + 1 + 2 = 6 words against r = 3 (one per unmatched pair): no brevity penalty, p_1 = 1e-15 / (6 + 1e-9)
    assert o['Bleu_1'] == [1e-15 / (6 + 1e-9)]
    short = _one(pred, [[0], [3, 0], [0]], gts, [[3, 4, 5, 6], [3, 4, 0, 0]], (0.9,))          # c = 1 < r = 3
    assert short['Bleu_1'] == [(1e-15 / (1 + 1e-9)) * math.exp(1.0 - 1.0 / ((1 + 1e-15) / (3 + 1e-9)))]


def test_anchor_tie_is_a_pair_and_not_a_hit():
    tau = R.iou(0.0, 6.0, 3.0, 9.0)
    assert 0.3 < tau < 0.34
    o = _one([[0.0, 6.0]], [[3, 0]], [[3.0, 9.0]], [[3, 0]], (tau, math.nextafter(tau, 0.0)))
    assert o['pairs'] == [[(0, 0)], [(0, 0)]] and o['n_unmatched'] == [[0], [0]]
    assert o['Precision'] == [0.0, 1.0] and o['Recall'] == [0.0, 1.0]


# ---- the packer -------------------------------------------------------------------------------------------------------------------
def test_pack_ground_truth():
    from echr_amd import densecap as D
    vids = [dict(timestamps=[[0.0, 5.5], [2.0, 9.0]], sentences=[[0, 3, 4, 0, 0], [5, 6, 7]]),
            ([[1.0, 2.0]], [[0, 9, 9, 9, 9]])]
    gt = D.pack_ground_truth(vids, 4, 10)
    assert gt.stamps.dtype == torch.float64 and tuple(gt.stamps.shape) == (3, 2) and gt.stamps[1].tolist() == [2.0, 9.0]
    assert gt.offset.dtype == torch.int32 and gt.offset.tolist() == [0, 2, 3]
    assert gt.refs.dtype == torch.int32 and gt.refs.tolist() == [[3, 4, 0, 0], [5, 6, 7, 0], [9, 9, 9, 9]]
    assert gt.ref_len.tolist() == [3, 4, 4]                       # section 4s's lengths: the end token counts where there is room
    assert [R.words(r) for r in gt.refs.tolist()] == [[3, 4], [5, 6, 7], [9, 9, 9, 9]]


def test_packer_refusals():
    from echr_amd import densecap as D
    ok = dict(timestamps=[[0.0, 1.0]], sentences=[[3, 0]])
    D.pack_ground_truth([ok], 63, 65534)
    for bad in ([dict(timestamps=[], sentences=[])],                                     # a video without an event
                [ok, dict(timestamps=np.zeros((0, 2)), sentences=[])],
                [dict(timestamps=[[0.0, 1.0], [1.0, 2.0]], sentences=[[3, 0]])],         # count mismatch
                [dict(timestamps=[[0.0, 1.0, 2.0]], sentences=[[3, 0]])],
                [dict(timestamps=[[0.0, float('nan')]], sentences=[[3, 0]])],
                [dict(timestamps=[[0.0, 1.0]], sentences=[[3, 4, 5, 6, 7]])],            # longer than seq_length
                [dict(timestamps=[[0.0, 1.0]], sentences=[[11, 0]])],                    # outside the vocabulary
                []):
        with pytest.raises(ValueError):
            D.pack_ground_truth(bad, 4, 10)
    with pytest.raises(ValueError):
        D.pack_ground_truth([ok], 64, 10)
    with pytest.raises(ValueError):
        D.pack_ground_truth([ok], 4, 65535)


def test_cpu_tensors_are_refused_before_the_device_is_touched():
    from echr_amd import densecap as D
    from echr_amd._lib import EchrHipError
    gt = D.pack_ground_truth([dict(timestamps=[[0.0, 1.0]], sentences=[[3, 0]])], 4, 10)
    with pytest.raises(EchrHipError):
        D.evaluate(torch.zeros(1, 2, dtype=torch.float64), [0, 1], torch.zeros(1, 4, dtype=torch.int64), gt)
    with pytest.raises(TypeError):
        D.evaluate(torch.zeros(1, 2, dtype=torch.float64), [0, 1], None, (gt.stamps, gt.offset))
    assert 'once per file' in D.__doc__                          # the one-ground-truth-set restriction is documented


# ---- ABI --------------------------------------------------------------------------------------------------------------------------
ENTRIES = ('echr_densecap_match', 'echr_densecap_fill', 'echr_densecap_pair_stats', 'echr_densecap_reduce')


def test_new_symbols_are_declared_bound_and_exported():
    from echr_amd import _lib, build
    assert 'densecap.hip' in build.SOURCES
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'echr_hip.h')).read()
    declared = set(re.findall(r'\b(echr_[a-z0-9_]+)\s*\(', hdr))
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in ENTRIES:
        assert name in declared and name in bound and hasattr(lib, name), name
    assert 'echr_densecap_args' in hdr and _lib.ABI_STRUCTS['echr_densecap_args'] is _lib.DensecapArgs
    assert lib.echr_abi_sizeof(b'echr_densecap_args') == C.sizeof(_lib.DensecapArgs) > 0
    assert lib.echr_version() == _lib.ABI_VERSION == 3
    from echr_amd import densecap as D
    for macro, value in (('MAX_TAU', D.MAX_TIOUS), ('VIDEO_COLS', D.VIDEO_COLS), ('MEAN_COLS', D.MEAN_COLS), ('STATS', D.STATS)):
        assert int(re.search(r'#define ECHR_DENSECAP_%s (\d+)' % macro, hdr).group(1)) == value


def test_entry_points_validate_before_any_launch():
    """The argument checks run on the host ahead of the launches: they need no GPU."""
    from echr_amd import _lib
    lib = _lib.load()
    fns = [getattr(lib, n) for n in ENTRIES]
    for fn, name in zip(fns, ENTRIES):
        assert fn(None, None) == -22 and name.encode() in lib.echr_last_error()
        a = _lib.DensecapArgs()
        a.L = 8
        assert fn(C.byref(a), None) == -22 and b'thresholds' in lib.echr_last_error()          # n_tau = 0
        a.n_tau = 9
        assert fn(C.byref(a), None) == -22 and b'thresholds' in lib.echr_last_error()
        a.n_tau, a.N_tot = 4, -1
        assert fn(C.byref(a), None) == -22 and b'negative' in lib.echr_last_error()
        a.N_tot = 0
        assert fn(C.byref(a), None) == 0                          # no video, no pair: nothing to launch
    match, fill, stats, reduce_ = fns
    a = _lib.DensecapArgs()
    a.V, a.n_tau, a.N_tot, a.G_tot, a.L = 1, 4, 3, 2, 8
    assert match(C.byref(a), None) == -22 and b'pred_offset' in lib.echr_last_error()
    a.P_tot = 1 << 31
    for fn in (fill, stats, reduce_):
        assert fn(C.byref(a), None) == -22 and b'pairs' in lib.echr_last_error()
    a.P_tot = 5
    assert fill(C.byref(a), None) == -22 and b'pred_offset' in lib.echr_last_error()
    assert reduce_(C.byref(a), None) == -22 and b'pred_offset' in lib.echr_last_error()
    a.L = 64
    assert stats(C.byref(a), None) == -22 and b'seq_length' in lib.echr_last_error()
    a.L, a.T = 63, 64
    assert stats(C.byref(a), None) == -22 and b'width' in lib.echr_last_error()
    a.T = 20
    assert stats(C.byref(a), None) == -22 and b'pair_pred' in lib.echr_last_error()
    a.P_tot = 0
    assert fill(C.byref(a), None) == 0 and stats(C.byref(a), None) == 0          # no pair

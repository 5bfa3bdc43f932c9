"""CPU: the float64 statements of tests/context_ref.py against plain float64 torch autograd (x.mean(0), index_add_, torch.cat) on two random
shapes each, the fixed-order float32 statement of the anchor scatter inside its own bound, and the conditioning of the attended-row
gradient cases the device test runs (tests/test_gpu_context_edges.py, section B): the float32 oracle resolves every row of d tap_feats to a
quarter of the device gate, rows outside every event are exactly zero in float64, and every case contains the lengths it claims."""
import numpy as np
import pytest
import torch

from tests import context_ref as CR
from tests import plain_event_ref as R

ORACLE_ROW_TOL = 2.5e-6          # a quarter of the device gate (1e-5 per row)


def _events(rs, N, T):
    ln = rs.randint(1, T + 1, size=N)
    st = np.array([rs.randint(0, T - l + 1) for l in ln])
    return st, ln, rs.randint(0, T, size=N)


@pytest.mark.parametrize('T,D,Ht,N,seed', [(9, 5, 3, 4, 0), (40, 66, 17, 7, 1)])
def test_event_pool_and_its_backward_match_autograd(T, D, Ht, N, seed):
    rs = np.random.RandomState(seed)
    c3d = rs.standard_normal((T, D)).astype(np.float32)
    tap = rs.standard_normal((T, Ht)).astype(np.float32)
    st, ln, ind = _events(rs, N, T)
    ind[1] = ind[0]          # a shared anchor
    for parts in (1, 2, 3):
        ref, bound, Dp = CR.event_pool(c3d, tap, st, ln, ind, parts)
        c, t = torch.from_numpy(c3d).double(), torch.from_numpy(tap).double().requires_grad_(True)
        cols = []
        if parts & 1:
            cols.append(torch.stack([c[s:s + l].mean(0) for s, l in zip(st, ln)]))
        if parts & 2:
            cols.append(t[torch.from_numpy(ind)])
        want = torch.cat(cols, 1)
        assert Dp == (D if parts & 1 else 0) and ref.shape == tuple(want.shape) and bound.shape == (N, Dp)
        assert np.abs(ref - want.detach().numpy()).max() < 1e-14
        if parts & 2:
            assert np.array_equal(ref[:, Dp:].astype(np.float32), tap[ind])          # copies
        if parts & 1:          # the bound scales as (len + 2) u mean|x| and the float32 mean of numpy lies inside it
            got = np.stack([c3d[s:s + l].mean(0, dtype=np.float32) for s, l in zip(st, ln)])
            assert np.all(np.abs(got - ref[:, :D]) <= bound) and np.all(bound > 0)
        if parts & 2:          # backward: index_add_ of the gathered columns' gradient onto a known base
            d_ech = rs.standard_normal((N, Dp + Ht)).astype(np.float32)
            base = rs.standard_normal((T, Ht)).astype(np.float32)
            gref, fixed, gbound, sharers = CR.event_gather_bwd(d_ech, ind, T, Dp, Ht, base)
            want.backward(torch.from_numpy(d_ech).double())
            assert np.abs(gref - (base.astype(np.float64) + t.grad.numpy())).max() < 1e-14
            iadd = torch.from_numpy(base).double().index_add_(0, torch.from_numpy(ind), torch.from_numpy(d_ech[:, Dp:]).double())
            assert np.abs(gref - iadd.numpy()).max() < 1e-14
            assert sharers.sum() == N and sharers[ind[0]] >= 2
            # the fixed-order float32 value lies within its own bound of the float64 one; rows that are no anchor are base, bit for bit
            assert fixed.dtype == np.float32 and np.all(np.abs(fixed - gref) <= gbound)
            off = sharers == 0
            assert off.any() and np.array_equal(fixed[off], base[off]) and not np.any(gbound[off]) and np.all(gbound[~off] > 0)


def test_fixed_order_scatter_is_the_owner_sum_in_event_order():
    """Three events on one anchor, the owner not event 0: base + ((0 + d1) + d3) + d4 in float32, a value the other orders do not all give."""
    ind = [2, 0, 1, 0, 0]
    d = np.asarray([[1.0], [1.0], [7.0], [2.0 ** -24], [2.0 ** -24]], np.float32)
    base = np.zeros((3, 1), np.float32)
    ref, fixed, bound, sharers = CR.event_gather_bwd(d, ind, 3, 0, 1, base)
    assert list(sharers) == [3, 1, 1]
    assert fixed[0, 0] == np.float32(1.0)                      # (1 + 2^-24) rounds to 1 twice; 2^-24 + 2^-24 first would give 1 + 2^-23
    assert ref[0, 0] == 1.0 + 2.0 ** -23 and abs(fixed[0, 0] - ref[0, 0]) <= bound[0, 0]
    assert fixed[1, 0] == 7.0 and fixed[2, 0] == 1.0


@pytest.mark.parametrize('rows,cols,seed', [(5, 7, 0), (129, 65, 1)])
def test_col_mean_and_its_backward_match_autograd(rows, cols, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((rows, cols)).astype(np.float32)
    g = rs.standard_normal(cols).astype(np.float32)
    base = rs.standard_normal((rows, cols)).astype(np.float32)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    m = xt.mean(0)
    m.backward(torch.from_numpy(g).double())
    ref, bound = CR.col_mean(x)
    assert np.abs(ref - m.detach().numpy()).max() < 1e-14
    assert np.all(np.abs(x.mean(0, dtype=np.float32) - ref) <= bound)
    assert np.allclose(bound, (rows + 3) * CR.U32 * np.abs(x.astype(np.float64)).mean(0), rtol=1e-12)
    gref, gbound = CR.col_mean_bwd(g, rows, base)
    assert np.abs(gref - (base.astype(np.float64) + xt.grad.numpy())).max() < 1e-14
    got = (base + g[None, :] * np.float32(1.0 / rows)).astype(np.float32)          # the kernel's own three roundings
    assert np.all(np.abs(got - gref) <= gbound)


@pytest.mark.parametrize('segs,cols,seed', [((0, 3, 0, 5, 0), 7, 0), ((9, 1, 0, 4), 65, 1)])
def test_seg_col_mean_and_its_backward_match_autograd(segs, cols, seed):
    rs = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(segs)]).astype(np.int32)
    T = int(off[-1]) + 2          # two rows behind the last segment belong to none
    x = rs.standard_normal((T, cols)).astype(np.float32)
    g = rs.standard_normal((len(segs), cols)).astype(np.float32)
    base = rs.standard_normal((T, cols)).astype(np.float32)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    means = torch.stack([xt[a:b].mean(0) if b > a else torch.zeros(cols, dtype=torch.float64) for a, b in zip(off[:-1], off[1:])])
    means.backward(torch.from_numpy(g).double())
    ref, bound = CR.seg_col_mean(x, off)
    assert np.abs(ref - means.detach().numpy()).max() < 1e-14
    empty = np.asarray(segs) == 0
    assert not np.any(ref[empty]) and not np.any(bound[empty]) and np.all(bound[~empty] > 0)
    gref, gbound = CR.seg_col_mean_bwd(g, off, base)
    assert np.abs(gref - (base.astype(np.float64) + xt.grad.numpy())).max() < 1e-14
    assert np.array_equal(gref[off[-1]:], base[off[-1]:].astype(np.float64)) and not np.any(gbound[off[-1]:])
    # one segment over all rows is col_mean
    one, ob = CR.seg_col_mean(x, [0, T])
    cm, cb = CR.col_mean(x)
    assert np.array_equal(one[0], cm) and np.array_equal(ob[0], cb)


@pytest.mark.parametrize('Tc,Tt,Dc,Ht', [(5, 5, 3, 2), (7, 4, 20, 24)])
def test_clip_rows_is_torch_cat(Tc, Tt, Dc, Ht):
    rs = np.random.RandomState(Tc)
    c3d, tap = rs.standard_normal((Tc, Dc)).astype(np.float32), rs.standard_normal((Tt, Ht)).astype(np.float32)
    T = min(Tc, Tt)
    want = torch.cat([torch.from_numpy(c3d)[:T], torch.from_numpy(tap)[:T]], 1).numpy()
    got = CR.clip_rows(c3d, tap)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))


def test_per_row_relerr():
    ref = np.asarray([[1.0, -2.0], [0.0, 0.0], [1e-3, 0.0], [0.5, 0.5]])
    got = ref + np.asarray([[1e-6, 0.0], [1e-6, 0.0], [0.0, 1e-6], [0.0, 0.0]])
    err, zero = CR.per_row_relerr(got, ref)
    assert list(zero) == [False, True, False, False]
    # row 0 on its own maximum; the zero row and the small row on the floor 1e-2 * 2.0
    assert np.allclose(err, [1e-6 / 2.0, 1e-6 / 2e-2, 1e-6 / 2e-2, 0.0], rtol=1e-9)
    err, _ = CR.per_row_relerr(got, ref, floor_frac=1e-4)
    assert np.allclose(err[2], 1e-6 / 1e-3, rtol=1e-9)


# ---- the attended-row gradient cases ------------------------------------------------------------------------------------------------------
def _lens(vid):
    return [int(e - s) for s, e in vid['soi']]


@pytest.mark.parametrize('name', sorted(CR.ROW_GRAD_CASES))
def test_row_grad_cases_are_well_conditioned(name):
    from echr_amd import functional as EF
    c = CR.ROW_GRAD_CASES[name]
    opt, params, vid = CR.make_row_grad_case(name)
    T, lens = vid['tap'].shape[0], _lens(vid)
    # the case contains what it claims
    assert opt.event_context_type == 'EC' and opt.video_context_type == 'VL' and opt.clip_context_type == c['clip']
    assert len(lens) == c['N'] and max(lens) == c['A'] and vid['labels'].shape[1] == CR.ROW_GRAD_L
    assert vid['tap'].shape[1] == opt.hidden_dim and vid['c3d'].shape[1] == opt.video_dim
    if 'lens' in c:
        assert tuple(lens[:len(c['lens'])]) == tuple(c['lens'])
    assert EF.rows_disjoint(vid['soi']) == bool(c.get('disjoint'))
    if name.startswith('slots'):
        assert {l % 8 for l in lens} >= {1, 7, 0} and min(lens) == 1 and sum(l <= 8 for l in lens) >= 3          # tails; chunks past len
        assert opt.hidden_dim == 24 and (opt.video_dim == 20)
    if name == 'nc260':
        assert opt.hidden_dim == 260
    if name == 'a3':
        assert max(lens) < 8
    if name == 'odd_dc':
        assert (opt.video_dim + opt.hidden_dim) % 4 == 1 and opt.video_dim % 4 != 0
    cov = CR.covered_rows(vid['soi'], T)
    assert cov.all() == bool(c.get('disjoint'))          # every other case has rows outside every event
    for train_mode in (False, True):
        r64 = R.run(opt, params, vid, train_mode, dtype=torch.float64)
        r32 = R.run(opt, params, vid, train_mode, dtype=torch.float32)
        g64, g32 = r64[3], r32[3]
        assert g64.dtype == np.float64 and g64.shape == vid['tap'].shape
        err, zero = CR.per_row_relerr(g32, g64)
        assert np.array_equal(zero, ~cov)                    # rows of no event: exactly zero; every covered row: a gradient
        assert not np.any(g32[~cov])
        assert err.max() <= ORACLE_ROW_TOL, (name, train_mode, err.max())
        assert np.abs(g64).max(1)[cov].min() > 1e-7          # no covered row is numerically dead

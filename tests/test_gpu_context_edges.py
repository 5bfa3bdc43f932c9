"""The kernels that build the decoder's contexts, called directly at their tile edges (-m gpu), against the float64 statements and derived
bounds of tests/context_ref.py:

  A. echr_event_pool_gather_fwd / _bwd, echr_col_mean_fwd / _bwd, echr_seg_col_mean_fwd / _bwd and echr_clip_rows through echr_amd._lib,
     so that a pre-filled output, ld > cols and a pointer that is only 4-byte aligned are reachable: 64-column chunks, the 16 row groups,
     the float4 / scalar load split, the 128-row chunks of the column sum (plain store up to 128 rows, zero-fill plus atomics above), the
     fixed-order forms.  Every output and all padding is pre-filled with a NaN bit pattern (known values for the kernels that accumulate)
     and what a kernel does not own is compared bit for bit afterwards.
  B. the attended-row gradient alone (echr_decoder_row_grad): with event_context_type 'EC' and video_context_type 'VL' tap_feats reaches
     the loss only through the attended rows, so d tap_feats of the module path IS that kernel chain's output.  Judged per row
     (context_ref.per_row_relerr) against tests/plain_event_ref.run in float64 at the cases of context_ref.ROW_GRAD_CASES, whose conditioning
     tests/test_context_ref_host.py asserts (the float32 oracle resolves every row to 2.5e-6).  Measured on an MI355X, worst per-row error
     of the device | of the float32 CPU oracle: slots_ch 3.4e-7 | 4.1e-7, slots_cch 3.8e-7 | 2.9e-7, nc260 2.7e-7 | 2.2e-7, disjoint
     3.3e-7 | 4.2e-7, a3 2.8e-7 | 3.1e-7, fixed-order slots_ch 3.4e-7; with gemm_h2 = 0, gemm_bf16x3 = 0 the device stays below 4.7e-7 and
     within 3.5e-7 of its default configuration in every row.  The gate is the project's TOL_GRAD = 1e-5, applied per row.
     'odd_dc' (video_dim = 21, D = 45) is refused by the decoder's width rule and kept as a refusal test.

The default-mode anchor scatter adds its terms onto the buffer one atomic at a time: a row with two sharers holds (base + t1) + t2 in one of
the two orders, which is the fixed-order value base + (t1 + t2) bit for bit only where base is zero.  One two-sharer anchor here has a zero
base and is compared with the fixed-order value; the other has a non-zero base and is compared with the two possible orders.
"""
import numpy as np
import pytest
import torch

from tests import context_ref as CR
from tests import plain_event_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

TOL_LOGP = 2e-5          # tests/test_gpu_clipctx.py
TOL_GRAD = 1e-5
ROW_TOL = 1e-5           # TOL_GRAD per row, with the floor of context_ref.per_row_relerr
GUARD = 8                # floats in front of and behind every buffer (keeps 16-byte alignment)
POISON = np.uint32(0x7FC12345)          # a quiet NaN with a recognisable payload


def _lib():
    from echr_amd import _lib as L
    return L, L.load()


def _poison(n):
    return np.full(n, POISON, np.uint32).view(np.float32)


class Buf(object):
    """A device buffer of `n` floats between two poisoned guards; `init` (n floats) or poison inside."""

    def __init__(self, n, init=None):
        host = _poison(n + 2 * GUARD).copy()
        if init is not None:
            host[GUARD:GUARD + n] = np.asarray(init, np.float32).reshape(-1)
        self.n, self.host = n, host
        self.t = torch.from_numpy(host.copy()).cuda()
        assert self.t.data_ptr() % 16 == 0

    def ptr(self, offset=0):
        return self.t.data_ptr() + 4 * (GUARD + offset)

    def get(self):
        """The n floats inside; asserts that both guards are untouched."""
        a = self.t.cpu().numpy()
        assert np.array_equal(a[:GUARD].view(np.uint32), self.host[:GUARD].view(np.uint32)), 'write in front of the buffer'
        assert np.array_equal(a[GUARD + self.n:].view(np.uint32), self.host[GUARD + self.n:].view(np.uint32)), 'write behind the buffer'
        return a[GUARD:GUARD + self.n].copy()


def _ints(a):
    return torch.from_numpy(np.asarray(a, np.int32)).cuda()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _padded(x, ld):
    """[rows, ld] float32: x in the first columns, poison in the padding."""
    out = _poison(x.shape[0] * ld).copy().reshape(x.shape[0], ld)
    out[:, :x.shape[1]] = x
    return out


def _deterministic(on):
    import echr_amd
    echr_amd.set_deterministic(on)


# ---- A. pool and gather, forward -------------------------------------------------------------------------------------------------------------
T_POOL = 40
POOL_LENS = (1, 15, 16, 17, 33, 40)          # around the 16 row groups; one, two and three rounds of them
POOL_STARTS = (38, 20, 3, 10, 7, 0)          # overlapping
POOL_IND = (39, 34, 0, 26, 39, 17)           # anchors anywhere on the video, one shared


def _pool_inputs(D, Ht, seed):
    rs = np.random.RandomState(seed)
    c3d = rs.standard_normal((T_POOL, max(D, 1))).astype(np.float32)
    tap = rs.standard_normal((T_POOL, max(Ht, 1))).astype(np.float32)
    assert all(s + l <= T_POOL for s, l in zip(POOL_STARTS, POOL_LENS))
    return c3d, tap


def _pool_fwd(c3d, tap, D, Ht, c3d_offset=0):
    """echr_event_pool_gather_fwd on [N, D + Ht] between guards; c3d_offset: the C3D rows start that many floats into their buffer."""
    L, lib = _lib()
    N = len(POOL_LENS)
    cb = Buf(c3d_offset + c3d.size, np.concatenate([_poison(c3d_offset), c3d.reshape(-1)]))
    tb = Buf(tap.size, tap)
    out = Buf(N * (D + Ht))
    st, ln, ind = _ints(POOL_STARTS), _ints(POOL_LENS), _ints(POOL_IND)
    L.check(lib.echr_event_pool_gather_fwd(cb.ptr(c3d_offset) if D else None, tb.ptr() if Ht else None, st.data_ptr(), ln.data_ptr(), ind.data_ptr(),
                                           out.ptr(), N, D, Ht, L.stream_ptr()), 'event_pool_gather_fwd')
    torch.cuda.synchronize()
    return out.get().reshape(N, D + Ht)


def _check_pool(got, c3d, tap, D, Ht):
    parts = (1 if D else 0) | (2 if Ht else 0)
    ref, bound, Dp = CR.event_pool(c3d[:, :max(D, 1)], tap[:, :max(Ht, 1)], POOL_STARTS, POOL_LENS, POOL_IND, parts)
    assert Dp == D and ref.shape == got.shape
    if D:
        err = np.abs(got[:, :D].astype(np.float64) - ref[:, :D])
        assert np.all(err <= bound), (D, Ht, float((err / np.maximum(bound, 1e-300)).max()))
    if Ht:
        assert _same_bits(got[:, D:], tap[list(POOL_IND)][:, :Ht])


# D: scalar path {1, 2, 3, 5, 63, 65, 66}, float4 path {4, 64, 68, 500}; the gather beside it 20 wide (parts 3)
@pytest.mark.parametrize('D', [1, 2, 3, 5, 63, 65, 66, 4, 64, 68, 500])
def test_pool_widths_on_both_load_paths(D):
    c3d, tap = _pool_inputs(D, 20, D)
    _check_pool(_pool_fwd(c3d, tap, D, 20), c3d, tap, D, 20)


# Ht against D = 500 (8 column chunks: Ht = 1 and 3 leave chunks without a gather share), against D = 4 (one chunk: the strided loop), and alone
@pytest.mark.parametrize('D', [500, 4, 0])
@pytest.mark.parametrize('Ht', [1, 3, 20, 257, 600])
def test_gather_widths_against_the_column_chunks(D, Ht):
    c3d, tap = _pool_inputs(D, Ht, 100 + Ht)
    _check_pool(_pool_fwd(c3d, tap, D, Ht), c3d, tap, D, Ht)


@pytest.mark.parametrize('D', [5, 64, 500])
def test_pool_alone(D):
    """parts = 1 (Ht = 0, tap NULL): the pooled rows only."""
    c3d, tap = _pool_inputs(D, 0, 200 + D)
    _check_pool(_pool_fwd(c3d, tap, D, 0), c3d, tap, D, 0)


def test_pool_from_a_pointer_that_is_only_4_byte_aligned():
    """D = 64 qualifies for float4 loads by its width; one float into a larger buffer the rows do not, and the scalar path must give the
    aligned call's values bit for bit (both add the rows of a row group in the same order)."""
    c3d, tap = _pool_inputs(64, 20, 7)
    a = _pool_fwd(c3d, tap, 64, 20)
    b = _pool_fwd(c3d, tap, 64, 20, c3d_offset=1)
    _check_pool(a, c3d, tap, 64, 20)
    assert _same_bits(a, b)


# ---- A. gather, backward ---------------------------------------------------------------------------------------------------------------------
# 14 events on 12 rows: row 3 is the anchor of events 1, 3, 6, 8, 10 (five sharers, none adjacent, the owner is not event 0), row 9 of events
# 2 and 5, row 0 of events 11 and 13; rows 7, 5, 2, 11, 6 have one event each; rows 1, 4, 8, 10 are no anchor.
GB_IND = (7, 3, 9, 3, 5, 9, 3, 2, 3, 11, 3, 0, 6, 0)
GB_T = 12
GB_ZERO_BASE_ROW = 9


def _gather_bwd(d_ech, base, D, Ht):
    L, lib = _lib()
    N = len(GB_IND)
    db, out = Buf(d_ech.size, d_ech), Buf(base.size, base)
    ind = _ints(GB_IND)
    L.check(lib.echr_event_pool_gather_bwd(db.ptr(), ind.data_ptr(), out.ptr(), N, D, Ht, L.stream_ptr()), 'event_pool_gather_bwd')
    torch.cuda.synchronize()
    return out.get().reshape(GB_T, Ht)


@pytest.mark.parametrize('D,Ht', [(5, 1), (5, 255), (5, 256), (5, 257), (5, 600), (0, 257), (500, 257)])
def test_gather_backward_adds_onto_the_buffer_in_both_modes(D, Ht):
    rs = np.random.RandomState(1000 + D + Ht)
    N = len(GB_IND)
    d_ech = rs.standard_normal((N, D + Ht)).astype(np.float32)
    base = rs.standard_normal((GB_T, Ht)).astype(np.float32)
    base[GB_ZERO_BASE_ROW] = 0.0
    ref, fixed, bound, sharers = CR.event_gather_bwd(d_ech, GB_IND, GB_T, D, Ht, base)
    assert sorted(set(sharers)) == [0, 1, 2, 5] and sharers[3] == 5 and sharers[9] == 2 and sharers[0] == 2 and GB_IND[0] != 3
    try:
        _deterministic(True)
        a, b = _gather_bwd(d_ech, base, D, Ht), _gather_bwd(d_ech, base, D, Ht)
    finally:
        _deterministic(False)
    assert _same_bits(a, fixed) and _same_bits(a, b)          # (rows that are no anchor included: base, bit for bit)
    got = _gather_bwd(d_ech, base, D, Ht)
    off = sharers == 0
    assert _same_bits(got[off], base[off])
    assert _same_bits(got[sharers == 1], fixed[sharers == 1])
    assert _same_bits(got[GB_ZERO_BASE_ROW], fixed[GB_ZERO_BASE_ROW])          # 0 + t1 + t2 in either order
    t1, t2 = d_ech[11, D:], d_ech[13, D:]                                         # row 0, a base that is not zero: one of the two orders
    o12, o21 = (base[0] + t1) + t2, (base[0] + t2) + t1
    assert o12.dtype == np.float32 and np.all((got[0] == o12) | (got[0] == o21))
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err <= bound), float((err[~off] / bound[~off]).max())           # the five-sharer row: 5 u (|base| + sum|terms|)
    assert np.abs(ref - base).max(1)[~off].min() > 0                              # every anchor row really received something


# ---- A. col_mean -----------------------------------------------------------------------------------------------------------------------------
COL_ROWS = [1, 3, 4, 13, 16, 17, 127, 128, 129, 257]
COL_COLS = [1, 63, 64, 65, 500]
COL_SHAPES = [(r, 65, 3) for r in COL_ROWS] + [(129, c, 3) for c in COL_COLS if c != 65] + [(129, 64, 0), (128, 64, 0)]


def _col_mean_fwd(xp, rows, cols, ld):
    L, lib = _lib()
    xb, out = Buf(xp.size, xp), Buf(cols)
    L.check(lib.echr_col_mean_fwd(xb.ptr(), rows, cols, ld, out.ptr(), L.stream_ptr()), 'col_mean_fwd')
    torch.cuda.synchronize()
    return out.get()


@pytest.mark.parametrize('fixed', [False, True], ids=['default', 'fixed'])
@pytest.mark.parametrize('rows,cols,pad', COL_SHAPES)
def test_col_mean_forward(rows, cols, pad, fixed):
    """out is poisoned: up to 128 rows the kernel overwrites it, above it must zero-fill before its chunks add (a NaN would survive)."""
    rs = np.random.RandomState(rows * 1000 + cols)
    x = rs.standard_normal((rows, cols)).astype(np.float32)
    ld = cols + pad
    xp = _padded(x, ld)
    ref, bound = CR.col_mean(x)
    try:
        _deterministic(fixed)
        runs = [_col_mean_fwd(xp, rows, cols, ld) for _ in range(2)]
    finally:
        _deterministic(False)
    for got in runs:
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - ref)
        assert np.all(err <= bound), float((err / bound).max())
    if fixed or rows <= 128:          # one writer per element, one order
        assert _same_bits(runs[0], runs[1])


@pytest.mark.parametrize('rows,cols,pad', COL_SHAPES)
def test_col_mean_backward_adds_onto_the_buffer(rows, cols, pad):
    L, lib = _lib()
    rs = np.random.RandomState(rows * 1000 + cols + 1)
    g = rs.standard_normal(cols).astype(np.float32)
    base = rs.standard_normal((rows, cols)).astype(np.float32)
    ld = cols + pad
    ref, bound = CR.col_mean_bwd(g, rows, base)
    gb, out = Buf(cols, g), Buf(rows * ld, _padded(base, ld))
    L.check(lib.echr_col_mean_bwd(gb.ptr(), rows, cols, ld, out.ptr(), L.stream_ptr()), 'col_mean_bwd')
    torch.cuda.synchronize()
    got = out.get().reshape(rows, ld)
    assert _same_bits(got[:, cols:], _padded(base, ld)[:, cols:])
    err = np.abs(got[:, :cols].astype(np.float64) - ref)
    assert np.all(err <= bound), float((err / bound).max())
    assert np.abs(ref - base).max() > 1e-2 / rows          # the added term is there to be got wrong


# ---- A. seg_col_mean -------------------------------------------------------------------------------------------------------------------------
SEGS = (0, 1, 3, 0, 4, 5, 9, 0)          # an empty segment first, in the middle and last; 1, 3, 4, 5, 9 rows around the four row lanes
SEG_TAIL = 2                             # rows behind the last segment that belong to none


def _seg_fwd(xp, off, cols, ld, ld_out):
    L, lib = _lib()
    V = len(off) - 1
    xb, out = Buf(xp.size, xp), Buf(V * ld_out)
    o = _ints(off)
    L.check(lib.echr_seg_col_mean_fwd(xb.ptr(), o.data_ptr(), V, cols, ld, out.ptr(), ld_out, L.stream_ptr()), 'seg_col_mean_fwd')
    torch.cuda.synchronize()
    return out.get().reshape(V, ld_out)


@pytest.mark.parametrize('cols', [63, 64, 65, 130])
def test_seg_col_mean_forward(cols):
    rs = np.random.RandomState(cols)
    off = np.concatenate([[0], np.cumsum(SEGS)]).astype(np.int32)
    T = int(off[-1]) + SEG_TAIL
    x = rs.standard_normal((T, cols)).astype(np.float32)
    ld, ld_out = cols + 3, cols + 5
    ref, bound = CR.seg_col_mean(x, off)
    a, b = (_seg_fwd(_padded(x, ld), off, cols, ld, ld_out) for _ in range(2))
    assert _same_bits(a, b)
    assert np.array_equal(a[:, cols:].view(np.uint32), np.full((len(SEGS), 5), POISON))
    empty = np.asarray(SEGS) == 0
    assert _same_bits(a[empty][:, :cols], np.zeros((int(empty.sum()), cols), np.float32))          # exactly +0.0
    err = np.abs(a[:, :cols].astype(np.float64) - ref)
    assert np.all(err <= bound), float((err[~empty] / bound[~empty]).max())


@pytest.mark.parametrize('cols', [63, 64, 65, 130])
def test_seg_col_mean_backward_adds_onto_the_buffer(cols):
    """g of the empty segments and all padding is poison: an empty segment reads nothing and leaves its (no) rows and everyone else's alone."""
    L, lib = _lib()
    rs = np.random.RandomState(cols + 1)
    off = np.concatenate([[0], np.cumsum(SEGS)]).astype(np.int32)
    V, T = len(SEGS), int(off[-1]) + SEG_TAIL
    g = rs.standard_normal((V, cols)).astype(np.float32)
    base = rs.standard_normal((T, cols)).astype(np.float32)
    ld, ld_g = cols + 3, cols + 2
    ref, bound = CR.seg_col_mean_bwd(g, off, base)
    gp = _padded(g, ld_g)
    gp[np.asarray(SEGS) == 0] = _poison(ld_g)
    runs = []
    for _ in range(2):
        gb, out, o = Buf(gp.size, gp), Buf(T * ld, _padded(base, ld)), _ints(off)
        L.check(lib.echr_seg_col_mean_bwd(gb.ptr(), ld_g, o.data_ptr(), V, cols, ld, out.ptr(), L.stream_ptr()), 'seg_col_mean_bwd')
        torch.cuda.synchronize()
        runs.append(out.get().reshape(T, ld))
    got = runs[0]
    assert _same_bits(got, runs[1])
    assert _same_bits(got[:, cols:], _padded(base, ld)[:, cols:])
    assert _same_bits(got[off[-1]:, :cols], base[off[-1]:])
    err = np.abs(got[:, :cols].astype(np.float64) - ref)
    assert np.all(err <= bound), float((err[:off[-1]] / bound[:off[-1]]).max())
    assert np.abs(ref - base)[:off[-1]].max(1).min() > 1e-3


@pytest.mark.parametrize('rows,cols', [(9, 65), (129, 130)])
def test_one_segment_agrees_with_col_mean(rows, cols):
    """The two kernels add in different orders: each within its own bound of the float64 mean, and of each other within the sum."""
    rs = np.random.RandomState(rows + cols)
    x = rs.standard_normal((rows, cols)).astype(np.float32)
    ref, bound = CR.col_mean(x)
    sref, sbound = CR.seg_col_mean(x, [0, rows])
    seg = _seg_fwd(x, np.asarray([0, rows], np.int32), cols, cols, cols)[0]
    col = _col_mean_fwd(x, rows, cols, cols)
    assert np.all(np.abs(seg.astype(np.float64) - sref[0]) <= sbound[0]) and np.all(np.abs(col.astype(np.float64) - ref) <= bound)
    assert np.all(np.abs(seg.astype(np.float64) - col.astype(np.float64)) <= bound + sbound[0])


# ---- A. clip_rows ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Tv', [1, 40])
@pytest.mark.parametrize('Dc,Ht', [(1, 1), (500, 512), (20, 24), (300, 3)])          # (300, 3): the second pass of the 256-thread loop crosses from c3d to tap
def test_clip_rows_is_bit_exact(Dc, Ht, Tv):
    L, lib = _lib()
    rs = np.random.RandomState(Dc + Ht + Tv)
    c3d = rs.standard_normal((Tv + 3, Dc)).astype(np.float32)          # the C3D matrix is longer: T = min(rows)
    tap = rs.standard_normal((Tv, Ht)).astype(np.float32)
    want = CR.clip_rows(c3d, tap)
    assert want.shape == (Tv, Dc + Ht)
    cb, tb, out = Buf(c3d.size, c3d), Buf(tap.size, tap), Buf(Tv * (Dc + Ht))
    L.check(lib.echr_clip_rows(cb.ptr(), Dc, tb.ptr(), Ht, out.ptr(), Tv, L.stream_ptr()), 'clip_rows')
    torch.cuda.synchronize()
    assert _same_bits(out.get().reshape(Tv, Dc + Ht), want)


# ---- B. the attended-row gradient alone ------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(name):
    """tests/plain_event_ref.run in float64 (train mode: the device's own dropout masks), once per case."""
    if name not in _REF:
        opt, params, vid = CR.make_row_grad_case(name)
        _REF[name] = (opt, params, vid, R.run(opt, params, vid, True, dtype=torch.float64))
    return _REF[name]


def _device(name):
    from tests.test_gpu_clipctx import _module_pass
    opt, params, vid, _ = _reference(name)
    return _module_pass(opt, params, vid, True)


def _check_row_grad(name, got):
    opt, params, vid, (rlogp, rloss, rgrads, rg_tap, _) = _reference(name)
    logp, loss, grads, g_tap = got[:4]
    cov = CR.covered_rows(vid['soi'], vid['tap'].shape[0])
    err, zero = CR.per_row_relerr(g_tap, rg_tap)
    print('%s: d tap_feats per-row error worst %.3e (row %d), median %.3e; d logp %.3e' % (name, err.max(), int(err.argmax()), float(np.median(err[cov])),
                                                                                        float(np.abs(logp - rlogp).max())))
    assert np.array_equal(zero, ~cov)
    assert not np.any(g_tap[~cov]), 'a row outside every event received a gradient'
    assert err.max() <= ROW_TOL, (name, float(err.max()), int(err.argmax()))
    assert np.abs(logp - rlogp).max() < TOL_LOGP
    for k, g in rgrads.items():
        if g is None:
            assert grads[k] is None or not np.any(grads[k]), k
            continue
        assert U.grad_close(k, grads[k], g, TOL_GRAD), (k, U.relerr(grads[k], g))


@pytest.mark.parametrize('name', ['slots_ch', 'slots_cch', 'nc260', 'disjoint', 'a3'])
def test_row_grad_per_row_against_float64(name):
    _check_row_grad(name, _device(name))


def test_row_grad_fixed_order_form():
    """'slots_ch' under set_deterministic(True): per-(event, slot) slabs folded per row in event order -- two runs bit-equal, and the gate."""
    try:
        _deterministic(True)
        a, b = _device('slots_ch'), _device('slots_ch')
    finally:
        _deterministic(False)
    assert a[1] == b[1] and _same_bits(a[3], b[3])
    for k, v in a[2].items():
        assert (v is None and b[2][k] is None) or np.array_equal(v, b[2][k]), k
    _check_row_grad('slots_ch', a)


def test_row_grad_odd_width_is_refused():
    """video_dim = 21 under 'CC+CH': D = 45.  The decoder takes row sources whose width is a multiple of 4 only and says so; the 'EC' pooling
    at D = 21 (scalar path) and the 45-wide row source are built before it refuses."""
    from echr_amd._lib import EchrHipError
    with pytest.raises(EchrHipError) as e:
        _device('odd_dc')
    assert 'D%4==0' in str(e.value) and 'D=45' in str(e.value), str(e.value)

"""Every GEMM kernel family of csrc/gemm.hip against the echr_gemm_desc contract of include/echr_hip.h (-m gpu):

    C[b][rowmap(i)][j] = act(alpha * sum_k A B + beta * C_old + bias + bias2 + addend[i % add_mod])

evaluated literally in float64 by tests/gemm_ref.py.  The 64 x 64 exact-fp32 tile (four layouts), the bf16x3 split kernel (BN = 64 / 128), the
two h2 kernels and the h2 pack (bit-exact against the format model), the grouped launch and the skinny streaming kernel are each driven
through the C ABI with the epilogue, layout, batching and split-K features production relies on, at the smallest shapes that reach the
mechanism (tile tails, every arm of the two-register-set k loop, padded XCD rectangles, scale-segment boundaries).

Harness: operands live in larger buffers whose surroundings are NaN; C is a [rows + 2, ldc] buffer of a sentinel (or random base values
where the call accumulates).  A case passes when |C - ref| <= tol * bound (+ 2e-6 where act = TANH) componentwise, every cell outside the
written region is bit-identical to what it held, and the output is finite.  bound = |alpha| |A| |B| + |beta| |C_old| + |bias| + |bias2| +
|addend|; tol is what tests/test_gpu_parity.py already enforces against float64 per family: 1e-6 fp32 (and skinny), 4e-7 bf16x3, 6e-7 h2
(all K <= 2048).  The family that ran is asserted from the profiler's launch counts (echr_prof_read kinds 0 = fp32, 6 = bf16x3, 7 = h2,
8 = pack): exactly one launch of the expected kind, none of the others.

Worst observed err / (tol * bound) per family on an MI355X (every case prints its own figure; run with -s):
    fp32 64 x 64 tile 0.27 (NN, K = 65), grouped fp32 0.25; bf16x3 0.56 (batch 2); h2 0.70 (9 x 2 tile grid, beta = 1), grouped h2 0.54;
    skinny 0.25 (K = 256), 0.31 in the grid-stride case.  The h2 pack is bit-exact in every case.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests import gemm_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENT = np.float32(-77.25)                      # what every C cell holds that no call may touch
TOL = {'f32': 1e-6, 'bf16x3': 4e-7, 'h2': 6e-7, 'skinny': 1e-6}
KINDS = {'f32': 0, 'bf16x3': 6, 'h2': 7, 'pack': 8}
PTRS = ('A', 'B', 'C', 'bias', 'bias2', 'addend', 'aux', 'row_index')
SCALARS = ('M', 'N', 'K', 'sam', 'sak', 'sbk', 'sbn', 'ldc', 'batch', 'bsa', 'bsb', 'bsc', 'alpha', 'beta', 'bs_bias', 'add_mod', 'ld_add', 'act',
           'ld_aux', 'rowmap_mod', 'rowmap_mul', 'split_k', 'algo', 'row_index_max')


def _libs():
    from echr_amd import _lib as L
    return L, L.load()


def _counts(fn):
    """(fn's result, {kind: launches the library's profiler counted while fn ran})."""
    L, lib = _libs()
    L.check(lib.echr_prof_enable(1), 'prof_enable')
    try:
        out = fn()
        torch.cuda.synchronize()
        n = {}
        for kind in KINDS.values():
            ms, fl, by, cnt = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
            L.check(lib.echr_prof_read(kind, C.byref(ms), C.byref(fl), C.byref(by), C.byref(cnt)), 'prof_read')
            n[kind] = cnt.value
    finally:
        L.check(lib.echr_prof_enable(0), 'prof_enable')
    return out, n


def _only(family, launches=1):
    return {k: (launches if k == KINDS[family] else 0) for k in KINDS.values()}


def _embed(x, pad, extra_rows=1):
    """x inside a [rows + extra_rows, cols + pad] buffer of NaN: the leading dimension is cols + pad."""
    x = np.asarray(x, dtype=np.float32)
    buf = np.full((x.shape[0] + extra_rows, x.shape[1] + pad), np.nan, dtype=np.float32)
    buf[:x.shape[0], :x.shape[1]] = x
    return buf


def _cbuf(rows, N, ldc, base=None):
    """[rows + 2, ldc] of the sentinel; base ([rows, N]): the values the call accumulates onto."""
    c = np.full((rows + 2, ldc), SENT, dtype=np.float32)
    if base is not None:
        c[:rows, :N] = base
    return c


def _upload(d):
    """Device copies of a host descriptor's buffers and the echr_gemm_desc over them.  d['_off'] = {name: elements}: the pointer is advanced by
    that many elements (the host references then see the same view)."""
    L, _ = _libs()
    t, desc = {}, L.GemmDesc()
    off = d.get('_off', {})
    for name in PTRS:
        if d.get(name) is not None:
            t[name] = torch.from_numpy(np.ascontiguousarray(d[name]).reshape(-1)).to(DEV)
            setattr(desc, name, t[name].data_ptr() + t[name].element_size() * off.get(name, 0))
    for name in SCALARS:
        if name in d:
            setattr(desc, name, d[name])
    for name, v in (('batch', 1), ('alpha', 1.0), ('split_k', 1)):
        if name not in d:
            setattr(desc, name, v)
    return t, desc


def _host(d):
    """The descriptor as tests/gemm_ref.py reads it: flat buffers, pointer offsets applied."""
    h = {k: v for k, v in d.items() if not k.startswith('_')}
    for name in PTRS:
        if h.get(name) is not None:
            h[name] = np.ascontiguousarray(h[name]).reshape(-1)[d.get('_off', {}).get(name, 0):]
    return h


def _ratio(out, ref, bnd, mask, tol, tanh):
    """max err / (tol * bound (+ 2e-6)) over the written cells; cells of bound 0 must be exact."""
    err = np.abs(out[mask].astype(np.float64) - ref[mask])
    lim = tol * bnd[mask] + (2e-6 if tanh else 0.0)
    assert np.all(err[lim == 0] == 0), 'a cell whose bound is zero is not exact'
    return float(np.max(err[lim > 0] / lim[lim > 0])) if np.any(lim > 0) else 0.0


def _verify(d, out, family, what, ref=None, bnd=None):
    h = _host(d)
    c0 = h['C']
    ref = R.desc_ref(h) if ref is None else ref
    bnd = R.bound(h) if bnd is None else bnd
    mask = R.written_mask(h)
    assert np.all(np.isfinite(out)), what
    assert np.array_equal(out[~mask].view(np.uint32), c0[~mask].view(np.uint32)), '%s: a cell outside the written region changed' % (what,)
    r = _ratio(out, ref, bnd, mask, TOL[family], h.get('act', 0) == R.ACT_TANH)
    print('RATIO %s %.4f %s' % (family, r, what))
    assert r <= 1.0, (what, r)
    return r


def _run(d, family, what, dev_ab=None):
    """One echr_gemm_f32 call on the descriptor; dev_ab: packed h2 images that replace the A / B pointers on the device."""
    L, lib = _libs()
    t, desc = _upload(d)
    if dev_ab is not None:
        desc.A, desc.B = dev_ab[0].data_ptr(), dev_ab[1].data_ptr()
    _, n = _counts(lambda: L.check(lib.echr_gemm_f32(C.byref(desc), L.stream_ptr()), what))
    assert n == _only(family), (what, n)
    out = t['C'].cpu().numpy()
    _verify(d, out, family, what)
    return out


def _rejected(d, what):
    """The call must fail with a message, launch nothing and leave C as it was."""
    L, lib = _libs()
    t, desc = _upload(d)
    rc, n = _counts(lambda: lib.echr_gemm_f32(C.byref(desc), L.stream_ptr()))
    assert rc != 0, what
    assert lib.echr_last_error(), what
    assert n == {k: 0 for k in KINDS.values()}, (what, n)
    assert np.array_equal(t['C'].cpu().numpy().view(np.uint32), np.ascontiguousarray(d['C']).reshape(-1).view(np.uint32)), what


def _rs(*seed):
    return np.random.RandomState(zlib.crc32(repr(seed).encode()) & 0x7FFFFFFF)


def _randn(rs, *shape):
    return rs.standard_normal(shape).astype(np.float32)


# ---- a. the 64 x 64 exact-fp32 tile ----------------------------------------------------------------------------------------------------
# (every shape has fewer than 200 128-tiles and K < 1024: the 128 x 128 tile is never chosen)

def _f32_desc(rs, layout, M, N, K, pad, ldc_pad=0, **kw):
    """layout: NT (A [M,K], B [N,K]), NN (B [K,N]), TN (A [K,M], B [K,N]), TT (A [K,M], B [N,K]); leading dimensions padded by `pad`."""
    a, b = _randn(rs, M, K), _randn(rs, N, K)
    d = dict(M=M, N=N, K=K, ldc=N + ldc_pad, algo=0)
    if layout[0] == 'N':
        d.update(A=_embed(a, pad), sam=K + pad, sak=1)
    else:
        d.update(A=_embed(a.T, pad), sam=1, sak=M + pad)
    if layout[1] == 'T':
        d.update(B=_embed(b, pad), sbk=1, sbn=K + pad)
    else:
        d.update(B=_embed(b.T, pad), sbk=N + pad, sbn=1)
    d['C'] = _cbuf(M, N, N + ldc_pad)
    d.update(kw)
    return d


@pytest.mark.parametrize('pad', [0, 3])
@pytest.mark.parametrize('layout', ['NT', 'NN', 'TN', 'TT'])
def test_f32_tile_layouts(layout, pad):
    """All four <AKC, BKC> instantiations, float4 staging (pad 0) and scalar staging on misaligned rows (pad 3): one tile with tails in every
    direction, one exact tile, tails of 1 past the tile in M, N (two tiles) and K, several workgroups."""
    for (M, N, K) in [(5, 7, 3), (64, 64, 32), (65, 129, 33), (130, 70, 100)]:
        _run(_f32_desc(_rs('lay', layout, pad, M), layout, M, N, K, pad), 'f32', 'f32 %s pad %d %s' % (layout, pad, (M, N, K)))


@pytest.mark.parametrize('layout', ['NT', 'NN', 'TN', 'TT'])
def test_f32_tile_k_sweep(layout):
    """k-tile counts 1 .. 6 with and without a k tail: every arm of the two-register-set loop (odd and even counts, the last prefetch)."""
    for K in (31, 32, 33, 64, 65, 96, 97, 128, 161):
        _run(_f32_desc(_rs('ks', layout, K), layout, 70, 66, K, 0), 'f32', 'f32 %s K=%d' % (layout, K))


def _epilogue_parts(rs, M, N, mod=10):
    return dict(bias=_randn(rs, N + 5), bias2=_randn(rs, N + 5), addend=_embed(_randn(rs, mod, N), 2), aux=_embed(np.tanh(_randn(rs, M, N)), 1))


def test_f32_tile_epilogues():
    """(130, 70, 100) NT, ldc = N + 3: each epilogue feature alone, then all that combine."""
    M, N, K, mod, mul = 130, 70, 100, 10, 13
    rs = _rs('epi')
    p = _epilogue_parts(rs, M, N, mod)
    base = _randn(rs, M, N)
    add = dict(addend=p['addend'], add_mod=mod, ld_add=N + 2)
    cases = {
        'alpha': dict(alpha=0.5),
        'beta': dict(beta=-0.75, C=_cbuf(M, N, N + 3, base)),
        'bias': dict(bias=p['bias']),
        'bias2': dict(bias2=p['bias2']),
        'addend': add,
        'tanh': dict(act=R.ACT_TANH),
        'rowmap': dict(rowmap_mod=mod, rowmap_mul=mul),
        'all': dict(alpha=0.5, beta=-0.75, C=_cbuf(M, N, N + 3, base), bias=p['bias'], bias2=p['bias2'], act=R.ACT_TANH, rowmap_mod=mod, rowmap_mul=mul, **add),
    }
    for name, kw in cases.items():
        _run(_f32_desc(_rs('epi', 1), 'NT', M, N, K, 0, 3, **kw), 'f32', 'f32 epilogue ' + name)
    # (1 - aux^2) gradient form on the NN layout, as the TSRM backward issues it
    _run(_f32_desc(_rs('epi', 2), 'NN', M, N, K, 0, 3, act=R.ACT_MUL_DTANH, aux=p['aux'], ld_aux=N + 1, alpha=0.5), 'f32', 'f32 epilogue mul_dtanh NN')
    # row_index: a hot row, indices beyond both ends (clamped), accumulate onto random base values
    Rr = 40
    idx = rs.randint(0, Rr, M).astype(np.int32)
    idx[:30], idx[30], idx[31] = 0, Rr + 5, -3
    _run(_f32_desc(_rs('epi', 3), 'NT', M, N, K, 0, 3, beta=1.0, split_k=-1, row_index=idx, row_index_max=Rr - 1, bias=p['bias'],
                   C=_cbuf(Rr, N, N + 3, _randn(rs, Rr, N))), 'f32', 'f32 epilogue row_index')


def test_f32_tile_batches():
    M, N, K, nb = 130, 70, 100, 3
    rs = _rs('batch')
    A, B = _randn(rs, nb * M, K), _randn(rs, nb * N, K)
    bias = _randn(rs, nb * N)
    d = dict(A=_embed(A, 0), B=_embed(B, 0), C=_cbuf(nb * M, N, N + 3), M=M, N=N, K=K, sam=K, sak=1, sbk=1, sbn=K, ldc=N + 3, batch=nb, bsa=M * K,
             bsb=N * K, bsc=M * (N + 3), bias=bias, algo=0)
    _run(dict(d, bs_bias=N), 'f32', 'f32 batch, a bias per batch')
    _run(dict(d, bs_bias=0, alpha=0.5), 'f32', 'f32 batch, one bias (the TSRM heads: batch + alpha)')
    # the sampler's K slabs: batch b contracts columns [b K, (b + 1) K) of ONE operand pair (bsa = bsb = K, row strides unchanged)
    for Ks in (32, 34):
        A, B = _randn(rs, M, 3 * Ks), _randn(rs, N, 3 * Ks)
        _run(dict(A=_embed(A, 0), B=_embed(B, 0), C=_cbuf(nb * M, N, N + 3), M=M, N=N, K=Ks, sam=3 * Ks, sak=1, sbk=1, sbn=3 * Ks, ldc=N + 3, batch=nb,
                  bsa=Ks, bsb=Ks, bsc=M * (N + 3), algo=0), 'f32', 'f32 K slabs of %d' % Ks)


def test_f32_tile_split_k():
    M, N = 130, 70
    rs = _rs('split')
    p = _epilogue_parts(rs, M, N)
    base = _randn(rs, M, N)
    # explicit: C holds its base value, beta is ignored, bias and addend land once
    _run(_f32_desc(_rs('split', 1), 'NT', M, N, 100, 0, 3, split_k=3, beta=0.0, bias=p['bias'], addend=p['addend'], add_mod=10, ld_add=N + 2,
                   C=_cbuf(M, N, N + 3, base)), 'f32', 'f32 explicit split_k = 3')
    # auto at K = 512 (16 k tiles on 6 workgroups: 4 slices): beta = 0 -> the library's own zero fill must respect ldc; beta = 1 accumulates
    _run(_f32_desc(_rs('split', 2), 'NT', M, N, 512, 0, 3, split_k=-1, beta=0.0, bias=p['bias']), 'f32', 'f32 auto split beta 0')
    _run(_f32_desc(_rs('split', 3), 'NT', M, N, 512, 0, 3, split_k=-1, beta=1.0, bias=p['bias'], C=_cbuf(M, N, N + 3, base)), 'f32', 'f32 auto split beta 1')
    A, B = _randn(rs, 2 * M, 512), _randn(rs, 2 * N, 512)
    for beta in (0.0, 1.0):
        c = _cbuf(2 * M, N, N + 3, _randn(rs, 2 * M, N) if beta else None)
        _run(dict(A=_embed(A, 0), B=_embed(B, 0), C=c, M=M, N=N, K=512, sam=512, sak=1, sbk=1, sbn=512, ldc=N + 3, batch=2, bsa=M * 512, bsb=N * 512,
                  bsc=M * (N + 3), split_k=-1, beta=beta, algo=0), 'f32', 'f32 auto split, batch 2, beta %g' % beta)


def test_f32_rejections():
    M, N, K = 130, 70, 100
    rs = _rs('rej')
    p = _epilogue_parts(rs, M, N)
    mk = lambda **kw: _f32_desc(_rs('rej', 1), 'NT', M, N, K, 0, 3, **kw)
    _rejected(mk(act=R.ACT_TANH, split_k=3), 'activation with split_k = 3')
    _rejected(mk(addend=p['addend'], add_mod=0, ld_add=N + 2), 'addend without add_mod')
    _rejected(mk(row_index=np.zeros(M, np.int32), row_index_max=5, beta=0.0), 'row_index with beta = 0')
    _rejected(mk(sam=K, sak=2), 'both strides of A != 1')


# ---- b. bf16x3 ---------------------------------------------------------------------------------------------------------------------------

def _wide(rs, rows, K, span=6):
    return (rs.standard_normal((rows, K)) * np.exp(rs.uniform(-span, span, (rows, 1)))).astype(np.float32)


def _bf_desc(rs, M, N, K, ldc_pad=0, span=6, **kw):
    d = dict(A=_embed(_wide(rs, M, K, span), 0), B=_embed(_wide(rs, N, K, span), 0), C=_cbuf(M, N, N + ldc_pad), M=M, N=N, K=K, sam=K, sak=1, sbk=1, sbn=K,
             ldc=N + ldc_pad, algo=1)
    d.update(kw)
    return d


@pytest.mark.parametrize('M,N,K', [(130, 257, 36), (300, 130, 100), (1409, 897, 68)])
def test_bf16x3_shapes(M, N, K):
    """BN = 64 form (fewer than 96 tiles) and BN = 128 form (12 x 8 = 96 tiles), ragged M / N, k tails, wide dynamic range."""
    _run(_bf_desc(_rs('bf', M), M, N, K), 'bf16x3', 'bf16x3 %s' % ((M, N, K),))


def test_bf16x3_epilogues_batch_split():
    M, N, K = 130, 257, 100
    rs = _rs('bfe')
    p = _epilogue_parts(rs, M, N)
    base = _randn(rs, M, N)
    cases = {
        'bias + rowmap (the logits form)': dict(bias=p['bias'], rowmap_mod=10, rowmap_mul=13),
        'alpha + beta': dict(alpha=0.5, beta=-0.75, C=_cbuf(M, N, N + 3, base)),
        # (narrow data and a small alpha: most pre-activations sit where tanh is not saturated)
        'bias + bias2 + addend + tanh': dict(bias=p['bias'], bias2=p['bias2'], addend=p['addend'], add_mod=10, ld_add=N + 2, act=R.ACT_TANH, alpha=0.05, span=0.5),
        'explicit split_k = 2': dict(split_k=2, bias=p['bias'], C=_cbuf(M, N, N + 3, base)),
    }
    for name, kw in cases.items():
        _run(_bf_desc(_rs('bfe', 1), M, N, K, 3, **kw), 'bf16x3', 'bf16x3 ' + name)
    # auto split at K = 256: 8 k tiles on 6 workgroups -> 2 slices
    _run(_bf_desc(_rs('bfe', 2), M, N, 256, 3, split_k=-1, beta=0.0), 'bf16x3', 'bf16x3 auto split beta 0')
    _run(_bf_desc(_rs('bfe', 3), M, N, 256, 3, split_k=-1, beta=1.0, C=_cbuf(M, N, N + 3, base)), 'bf16x3', 'bf16x3 auto split beta 1')
    A, B = _wide(rs, 2 * M, K), _wide(rs, 2 * N, K)
    _run(dict(A=_embed(A, 0), B=_embed(B, 0), C=_cbuf(2 * M, N, N + 3), M=M, N=N, K=K, sam=K, sak=1, sbk=1, sbn=K, ldc=N + 3, batch=2, bsa=M * K, bsb=N * K,
              bsc=M * (N + 3), bias=_randn(rs, 2 * N), bs_bias=N, algo=1), 'bf16x3', 'bf16x3 batch 2')


def test_bf16x3_silent_fallbacks_run_the_fp32_tile():
    """K % 4 != 0, an A pointer that is not 16-byte aligned, and M N < 128^2: right results, counted as fp32 launches."""
    _run(_bf_desc(_rs('bff', 1), 130, 257, 38), 'f32', 'bf16x3 fallback K = 38')
    d = _bf_desc(_rs('bff', 2), 130, 257, 36)
    d['A'] = np.concatenate([np.full(1, np.nan, np.float32), d['A'].reshape(-1)])
    d['_off'] = {'A': 1}
    _run(d, 'f32', 'bf16x3 fallback misaligned A')
    _run(_bf_desc(_rs('bff', 3), 100, 100, 36), 'f32', 'bf16x3 fallback M N < 128^2')


# ---- c. h2 -------------------------------------------------------------------------------------------------------------------------------

def _h2_operands(rs, M, N, K):
    """The dynamic range of test_gemm_h2_packed_is_fp32_accurate, with an all-zero row M // 2."""
    a = (rs.standard_normal((M, K)) * np.exp(rs.uniform(-12, 12, (M, 1))) * np.exp2(rs.randint(-8, 8, (M, K)))).astype(np.float32)
    b = _wide(rs, N, K, 12)
    a[rs.uniform(size=a.shape) < 0.05] = 0.0
    a[M // 2] = 0.0
    return a, b


def _pack(x, s_row=None, s_col=1, rows=None, cols=None, gather=None, fill=0xAB):
    """echr_h2_pack (echr_h2_pack_gather) of the device tensor x into an image pre-filled with a byte pattern."""
    L, lib = _libs()
    rows = x.shape[0] if rows is None else rows
    cols = x.shape[1] if cols is None else cols
    img = torch.full((int(lib.echr_h2_bytes(rows, cols)),), fill, dtype=torch.uint8, device=DEV)
    s_row = x.stride(0) if s_row is None else s_row
    if gather is None:
        L.check(lib.echr_h2_pack(x.data_ptr(), rows, cols, s_row, s_col, img.data_ptr(), L.stream_ptr()), 'h2_pack')
    else:
        L.check(lib.echr_h2_pack_gather(x.data_ptr(), rows, cols, s_row, s_col, gather.data_ptr(), img.data_ptr(), L.stream_ptr()), 'h2_pack_gather')
    return img


def _h2_desc(a, b, ldc_pad=0, **kw):
    M, K = a.shape
    N = b.shape[0]
    d = dict(A=a, B=b, C=_cbuf(M, N, N + ldc_pad), M=M, N=N, K=K, sam=K, sak=1, sbk=1, sbn=K, ldc=N + ldc_pad, algo=2)
    d.update(kw)
    return d


def _h2_images(a, b):
    return _pack(torch.from_numpy(a).to(DEV)), _pack(torch.from_numpy(b).to(DEV))


@pytest.mark.parametrize('tm,tn', [(1, 1), (3, 5), (9, 2), (2, 9), (17, 1)])
def test_h2_tile_grids(tm, tn):
    """tiles_m x tiles_n grids whose XCD rectangles are padded (3 x 5 -> 2 x 4 rectangles of 2 x 2 = 16 slots for 15 tiles, 17 x 1 -> 24 slots, ...):
    the spare workgroups must retire, every cell is written (beta = 0, sentinel C) exactly once (beta = 1, random C)."""
    M, N, K = 128 * tm - 5, 128 * tn - 3, 72
    rs = _rs('h2g', tm, tn)
    a, b = _h2_operands(rs, M, N, K)
    imgs = _h2_images(a, b)
    _run(_h2_desc(a, b), 'h2', 'h2 grid %dx%d beta 0' % (tm, tn), imgs)
    _run(_h2_desc(a, b, beta=1.0, C=_cbuf(M, N, N, _randn(rs, M, N))), 'h2', 'h2 grid %dx%d beta 1' % (tm, tn), imgs)


@pytest.mark.parametrize('K', [24, 32, 40, 256, 264, 761])
def test_h2_k_blocks_and_both_kernels(K):
    """One k block, a k tail, the 256-wide scale-segment boundary and a partial last segment.  The dispatch is `split < 8`: split_k = 1 and an
    explicit split_k = 3 run gemm_h2m16_kernel, split_k = 8 at K = 761 (24 k blocks, 3 per slice: slices cross the segments at non-multiples
    of 8) runs gemm_h2_kernel<128, 32, 2>."""
    M, N = 130, 131
    rs = _rs('h2k', K)
    a, b = _h2_operands(rs, M, N, K)
    imgs = _h2_images(a, b)
    _run(_h2_desc(a, b), 'h2', 'h2 K=%d unsplit' % K, imgs)
    base = _randn(rs, M, N)
    _run(_h2_desc(a, b, split_k=3, C=_cbuf(M, N, N, base)), 'h2', 'h2 K=%d split_k 3' % K, imgs)
    if K == 761:
        _run(_h2_desc(a, b, split_k=8, C=_cbuf(M, N, N, base), bias=_randn(rs, N)), 'h2', 'h2 K=761 split_k 8', imgs)


def test_h2_epilogues():
    M, N, K = 130, 257, 100
    rs = _rs('h2e')
    a, b = _h2_operands(rs, M, N, K)
    imgs = _h2_images(a, b)
    p = _epilogue_parts(rs, M, N)
    Rr = 40
    idx = rs.randint(0, Rr, M).astype(np.int32)
    idx[:30], idx[30], idx[31] = 0, Rr + 5, -3
    cases = {
        'bias + rowmap (the logits form)': dict(bias=p['bias'], rowmap_mod=10, rowmap_mul=13),
        'bias + bias2 + addend': dict(bias=p['bias'], bias2=p['bias2'], addend=p['addend'], add_mod=10, ld_add=N + 2),
        'alpha': dict(alpha=0.5),
        'row_index': dict(beta=1.0, split_k=-1, row_index=idx, row_index_max=Rr - 1, C=_cbuf(Rr, N, N + 3, _randn(rs, Rr, N))),
    }
    for name, kw in cases.items():
        out = _run(_h2_desc(a, b, 3, **kw), 'h2', 'h2 ' + name, imgs)
        if name == 'alpha':
            assert np.all(out.reshape(-1, N + 3)[M // 2, :N] == 0.0)          # the all-zero row (scale 1) gives exact zeros


# ---- d. the h2 pack, bit-exact against the format model -------------------------------------------------------------------------------

def _canon(img, rows, cols):
    """NaN payloads are not part of the format (inf - inf): every fp16 NaN of the planes becomes one pattern."""
    img = np.array(img, dtype=np.uint8, copy=True)
    nplane = -(-rows // 128) * -(-cols // 32) * R.H2_CHUNK
    h = img[:nplane].view(np.uint16)
    h[(h & 0x7FFF) > 0x7C00] = 0x7E00
    return torch.from_numpy(img)


def _pack_case(x, what, transposed=False, ld=None, gather=None, src=None):
    """Pack the logical [rows, cols] operand x from a NaN-surrounded source (k-contiguous with row stride ld, or transposed: element (r, k) at
    src[k * ld + r]); the whole image -- planes, padding and scales -- must equal h2_pack_ref(x), in exactly one pack launch."""
    rows, cols = x.shape
    if src is None:
        src = _embed(x.T if transposed else x, (ld or (rows if transposed else cols)) - (rows if transposed else cols))
    dev = torch.from_numpy(src).to(DEV)
    g = None if gather is None else torch.from_numpy(np.asarray(gather, dtype=np.int32)).to(DEV)
    s_row, s_col = (1, src.shape[1]) if transposed else (src.shape[1], 1)
    img, n = _counts(lambda: _pack(dev, s_row, s_col, rows, cols, g))
    assert n == _only('pack'), (what, n)
    assert torch.equal(_canon(img.cpu().numpy(), rows, cols), _canon(R.h2_pack_ref(x), rows, cols)), what


def test_h2_pack_k_contiguous_sources():
    rs = _rs('pk')
    for (Rw, K, ld) in [(16, 64, 64), (130, 100, 100), (130, 100, 104), (257, 264, 264), (130, 101, 101), (33, 61, 63), (128, 5, 5)]:
        # ld % 4 == 0: float4 loads; otherwise the dword-aligned F4U path; K % 8 != 0: the scalar tail
        _pack_case(_wide(rs, Rw, K, 12), 'pack rows %s' % ((Rw, K, ld),), ld=ld)


def test_h2_pack_transposing_sources():
    rs = _rs('pt')
    for (Rw, K, ld) in [(128, 100, 128), (192, 264, 196), (130, 100, 130), (128, 72, 131), (64, 40, 64), (200, 33, 200)]:
        # vector form: the 64-row half inside the operand and ld % 4 == 0; scalar form otherwise (R = 130 and 200 mix both per row block)
        _pack_case(_wide(rs, Rw, K, 12), 'pack cols %s' % ((Rw, K, ld),), transposed=True, ld=ld)


@pytest.mark.parametrize('K', [20, 256, 264, 530])
def test_h2_pack_k_block_counts(K):
    """KT = 1, 8, 9, 17 k blocks: one partial segment, exactly one, one and a block, two and a block -- every form of the pack."""
    rs = _rs('pkt', K)
    _pack_case(_wide(rs, 16, K, 12), 'rows K=%d' % K)
    _pack_case(_wide(rs, 64, K, 12), 'cols vec K=%d' % K, transposed=True)
    _pack_case(_wide(rs, 70, K, 12), 'cols scalar K=%d' % K, transposed=True, ld=71)


def _special_rows():
    K = 300
    x = np.zeros((8, K), np.float32)
    rs = _rs('sp')
    x[1] = rs.standard_normal(K) * 1e-40                          # subnormal row: scale 1
    x[2] = rs.standard_normal(K); x[2, 7] = np.inf                # an inf: scale 1 in its segment
    x[3] = rs.uniform(-1, 1, K) * 30; x[3, 3] = x[3, 299] = 32.0  # maximum exactly at a power of two
    x[4] = rs.uniform(1, 1.9, K) * 2.0 ** -120                    # below the exponent floor
    x[5, :256] = rs.uniform(-1, 1, 256) * 3.0
    x[5, 256:] = rs.uniform(-1, 1, 44) * 1e6                      # segments scale independently
    return x


def test_h2_pack_special_rows():
    x = _special_rows()
    _pack_case(x, 'special rows, k-contiguous')
    _pack_case(x, 'special rows, transposing', transposed=True, ld=8)
    _pack_case(x, 'special rows, transposing, misaligned', transposed=True, ld=9)


def test_h2_pack_gather():
    rs = _rs('pg')
    src = _wide(rs, 40, 100, 12)
    g = np.array([3, 3, 0, 39, 7, 38, 3, 21, 20, 19, 5, 39, 0, 12, 30, 31, 33, 2, 2, 9], dtype=np.int32)      # repeats 3, 0, 39, 2; skips most rows
    _pack_case(src[g], 'gathered row pack', src=_embed(src, 4), gather=g)
    # transposing pack with a gathered k axis: element (r, k) = src[gather[k]][r]
    for (Rw, ld) in [(128, 128), (130, 131)]:
        src = _wide(rs, 50, Rw, 12)
        g = rs.randint(0, 50, 70).astype(np.int32)
        g[:4] = [49, 49, 0, 0]
        _pack_case(np.ascontiguousarray(src[g].T), 'gathered transposing pack R=%d' % Rw, transposed=True, src=_embed(src, ld - Rw), gather=g)


# ---- e. the grouped launch -------------------------------------------------------------------------------------------------------------

def _grouped(ds, family, what, launches=1, imgs=None, chain=False):
    """echr_gemm_grouped on the host descriptors ds (chain: they share ds[0]'s C buffer and accumulate one after the other in the reference)."""
    L, lib = _libs()
    ups = [_upload(d) for d in ds]
    arr = (L.GemmDesc * len(ds))(*[u[1] for u in ups])
    for i in range(len(ds)):
        if imgs is not None:
            arr[i].A, arr[i].B = imgs[i][0].data_ptr(), imgs[i][1].data_ptr()
        if chain:
            arr[i].C = ups[0][1].C
    _, n = _counts(lambda: L.check(lib.echr_gemm_grouped(arr, len(ds), L.stream_ptr()), what))
    assert n == _only(family, launches), (what, n)
    if not chain:
        return [_verify(d, u[0]['C'].cpu().numpy(), family, '%s [%d]' % (what, i)) for i, (d, u) in enumerate(zip(ds, ups))]
    out = ups[0][0]['C'].cpu().numpy()
    ref, bnd = _host(ds[0])['C'].astype(np.float64), np.abs(_host(ds[0])['C'].astype(np.float64)) * R.written_mask(_host(ds[0]))
    for d in ds:
        ref, bnd = R.desc_ref(dict(_host(d), C=ref)), R.bound(dict(_host(d), C=bnd))
    _verify(ds[0], out, family, what, ref, bnd)
    return out


def _f32_group(beta, shared):
    M, N, K = 70, 66, 200
    ds = []
    for g in range(3):
        rs = _rs('grp', g)
        p = _epilogue_parts(rs, M, N)
        kw = [dict(addend=p['addend']), dict(bias=p['bias'], bias2=p['bias2']), dict(bias=p['bias'])][g]          # the decoder's token-side products
        ds.append(_f32_desc(rs, 'NT', M, N, K, 0, 3, split_k=-1, beta=beta, add_mod=10, ld_add=N + 2,
                            C=_cbuf(M, N, N + 3, _randn(_rs('grp', 'c', 0 if shared else g), M, N) if beta else None), **kw))
    return ds


def test_grouped_f32_distinct_outputs():
    for beta in (0.0, 1.0):
        _grouped(_f32_group(beta, False), 'f32', 'grouped f32 beta %g' % beta)


def test_grouped_f32_shared_output_accumulates():
    """Three problems into ONE C in accumulate mode: two forced k slices that add atomically; under 'deterministic' one launch per problem, in
    order, bit-identical run to run."""
    _, lib = _libs()
    _grouped(_f32_group(1.0, True), 'f32', 'grouped f32 shared C', chain=True)
    try:
        assert lib.echr_config_set(b'deterministic', 1) == 0
        o1 = _grouped(_f32_group(1.0, True), 'f32', 'grouped f32 shared C, deterministic', launches=3, chain=True)
        o2 = _grouped(_f32_group(1.0, True), 'f32', 'grouped f32 shared C, deterministic again', launches=3, chain=True)
        assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32))
    finally:
        lib.echr_config_set(b'deterministic', 0)


@pytest.mark.parametrize('beta', [0.0, 1.0])
def test_grouped_h2_eight_problems_of_different_shapes(beta):
    """The weight-gradient launch of the decoder's backward, scaled down: seven problems with M = 200 and N of 1 or 3 column chunks, one with
    M = 60 -- the grid is sized for 2 x 3 tiles, so most problems own spare workgroups that must retire without touching anything, and no
    needed tile may retire."""
    K = 136
    ds, imgs = [], []
    for g, (M, N) in enumerate([(200, 70), (200, 70), (200, 70), (200, 100), (200, 100), (200, 100), (200, 300), (60, 70)]):
        rs = _rs('g8', g)
        a, b = _h2_operands(rs, M, N, K)
        imgs.append(_h2_images(a, b))
        ds.append(_h2_desc(a, b, 3, split_k=-1, beta=beta, C=_cbuf(M, N, N + 3, _randn(rs, M, N) if beta else None)))
    _grouped(ds, 'h2', 'grouped h2 x8 beta %g' % beta, imgs=imgs)


def test_grouped_rejections():
    L, lib = _libs()
    M, N, K = 70, 66, 200

    def rej(ds, what, share=False):
        ups = [_upload(d) for d in ds]
        arr = (L.GemmDesc * len(ds))(*[u[1] for u in ups])
        if share:
            for i in range(len(ds)):
                arr[i].C = ups[0][1].C
        rc, n = _counts(lambda: lib.echr_gemm_grouped(arr, len(ds), L.stream_ptr()))
        assert rc != 0 and lib.echr_last_error(), what
        assert n == {k: 0 for k in KINDS.values()}, (what, n)
        for d, u in zip(ds, ups):
            assert np.array_equal(u[0]['C'].cpu().numpy().view(np.uint32), d['C'].reshape(-1).view(np.uint32)), what

    mk = lambda m, n, k, **kw: _f32_desc(_rs('grej', m, n, k), 'NT', m, n, k, 0, 3, **kw)
    rej([mk(M, N, K), mk(M, N, K + 32)], 'problems of different K')
    rej([mk(M, N, K), mk(M, N + 4, K)], 'different N on fp32')
    rej([mk(M, N, K), mk(M + 2, N, K)], 'different M on fp32')
    rej([mk(M, N, K, beta=1.0), mk(M, N, K, beta=1.0)], 'shared C with split_k = 1', share=True)
    assert lib.echr_gemm_grouped(None, 2, L.stream_ptr()) != 0


# ---- f. the skinny streaming kernel ----------------------------------------------------------------------------------------------------

def _skinny(A, lda, W, ldw, bias, Cc, ldc, M, Nc, K):
    L, lib = _libs()
    return lib.echr_gemm_skinny_nt(A.data_ptr(), lda, W.data_ptr(), ldw, None if bias is None else bias.data_ptr(), Cc.data_ptr(), ldc, M, Nc, K,
                                   L.stream_ptr())


@pytest.mark.parametrize('K', [256, 512])
def test_skinny_shapes(K):
    """M at and just past the 4096 minimum and past a 16-row tile boundary (4097: one row in the last tile, 4111: fifteen), 1 / 5 / 16 columns,
    padded leading dimensions with NaN padding, bias present and null."""
    L, lib = _libs()
    rs = _rs('sk', K)
    Mmax = 4111
    a, w, bias = _randn(rs, Mmax, K), _randn(rs, 16, K), _randn(rs, 16)
    A, W, bv = torch.from_numpy(_embed(a, 4)).to(DEV), torch.from_numpy(_embed(w, 4)).to(DEV), torch.from_numpy(bias).to(DEV)
    prod = a.astype(np.float64) @ w.astype(np.float64).T
    bprod = np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T
    for M in (4096, 4097, 4111):
        for Nc in (1, 5, 16):
            for with_bias in (True, False):
                what = 'skinny M=%d Nc=%d K=%d bias=%s' % (M, Nc, K, with_bias)
                c0 = _cbuf(M, Nc, Nc + 3)
                Cc = torch.from_numpy(c0).to(DEV)
                _, n = _counts(lambda: L.check(_skinny(A, K + 4, W, K + 4, bv if with_bias else None, Cc, Nc + 3, M, Nc, K), what))
                assert n == _only('f32'), (what, n)
                out = Cc.cpu().numpy()
                ref = prod[:M, :Nc] + (bias[:Nc].astype(np.float64) if with_bias else 0.0)
                bnd = bprod[:M, :Nc] + (np.abs(bias[:Nc]).astype(np.float64) if with_bias else 0.0)
                mask = np.zeros(c0.shape, bool)
                mask[:M, :Nc] = True
                assert np.all(np.isfinite(out)), what
                assert np.array_equal(out[~mask].view(np.uint32), c0[~mask].view(np.uint32)), what
                r = _ratio(out, _place(ref, c0.shape), _place(bnd, c0.shape), mask, TOL['skinny'], False)
                print('RATIO skinny %.4f %s' % (r, what))
                assert r <= 1.0, (what, r)


def _place(x, shape):
    out = np.zeros(shape, np.float64)
    out[:x.shape[0], :x.shape[1]] = x
    return out


def test_skinny_grid_stride():
    """More than 8192 row tiles: the 2048-workgroup grid loops over them.  The float64 reference of this one case is built on the device."""
    L, lib = _libs()
    M, Nc, K = 131072 + 21, 16, 256
    g = torch.Generator(device='cpu').manual_seed(11)
    A = torch.full((M + 1, K + 4), float('nan'), device=DEV)
    A[:M, :K] = torch.randn(M, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(12))
    w = torch.randn(Nc, K, generator=g)
    W = torch.full((Nc + 1, K + 4), float('nan'), device=DEV)
    W[:Nc, :K] = w.to(DEV)
    bias = torch.randn(Nc, generator=g).to(DEV)
    Cc = torch.full((M + 2, Nc + 3), float(SENT), device=DEV)
    _, n = _counts(lambda: L.check(_skinny(A, K + 4, W, K + 4, bias, Cc, Nc + 3, M, Nc, K), 'skinny grid stride'))
    assert n == _only('f32'), n
    a64, w64 = A[:M, :K].double(), W[:Nc, :K].double()
    ref = a64 @ w64.t() + bias.double()
    lim = TOL['skinny'] * (a64.abs() @ w64.abs().t() + bias.double().abs())
    r = float(((Cc[:M, :Nc].double() - ref).abs() / lim).max())
    print('RATIO skinny %.4f grid stride' % r)
    assert r <= 1.0, r
    assert bool(torch.isfinite(Cc).all())
    assert bool((Cc[M:] == float(SENT)).all()) and bool((Cc[:, Nc:] == float(SENT)).all())


def test_skinny_rejections():
    L, lib = _libs()
    A = torch.zeros(4200, 520, device=DEV)
    W = torch.zeros(17, 520, device=DEV)
    for what, (M, Nc, K, lda) in {'M = 4095': (4095, 16, 512, 516), 'Nc = 17': (4096, 17, 512, 516), 'K = 500': (4096, 16, 500, 516),
                                  'lda % 4 != 0': (4096, 16, 512, 517)}.items():
        Cc = torch.full((4200, 20), float(SENT), device=DEV)
        rc, n = _counts(lambda: _skinny(A, lda, W, 516, None, Cc, 20, M, Nc, K))
        assert rc != 0 and lib.echr_last_error(), what
        assert n == {k: 0 for k in KINDS.values()}, (what, n)
        assert bool((Cc == float(SENT)).all()), what
    Cc = torch.full((4200, 20), float(SENT), device=DEV)
    assert lib.echr_gemm_skinny_nt(None, 516, W.data_ptr(), 516, None, Cc.data_ptr(), 20, 4096, 16, 512, L.stream_ptr()) != 0

"""CPU tests of tests/gemm_ref.py, the float64 references that tests/test_gpu_gemm_contract.py holds every GEMM kernel family to: desc_ref
against plain torch float64 expressions, one echr_gemm_desc feature at a time, and the h2 format model against the properties that
csrc/gemm.hip and include/echr_hip.h document (image size, round trip within the derived bound, the special rows)."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as R


def _rs(seed):
    return np.random.RandomState(seed)


def _f32(rs, *shape):
    return rs.standard_normal(shape).astype(np.float32)


def _t(x):
    return torch.from_numpy(np.asarray(x)).double()


def _nt(rs, M, N, K, **kw):
    """An NT descriptor on contiguous operands with ldc = N and a random C."""
    d = dict(A=_f32(rs, M, K), B=_f32(rs, N, K), C=_f32(rs, M, N), M=M, N=N, K=K, sam=K, sak=1, sbk=1, sbn=K, ldc=N)
    d.update(kw)
    return d


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape
    assert np.max(np.abs(a - b)) <= 1e-12 * max(1.0, np.max(np.abs(b)))


def test_desc_ref_plain_product_and_layouts():
    rs = _rs(1)
    M, N, K = 7, 5, 11
    d = _nt(rs, M, N, K)
    prod = _t(d['A']) @ _t(d['B']).t()
    _close(R.desc_ref(d), prod)
    # NN: B stored [K, N]; TN: A stored [K, M]; both with padded leading dimensions whose padding is NaN
    Bp = np.full((K, N + 3), np.nan, np.float32); Bp[:, :N] = d['B'].T
    Ap = np.full((K, M + 2), np.nan, np.float32); Ap[:, :M] = d['A'].T
    _close(R.desc_ref(dict(d, B=Bp, sbk=N + 3, sbn=1)), prod)
    _close(R.desc_ref(dict(d, A=Ap, sam=1, sak=M + 2, B=Bp, sbk=N + 3, sbn=1)), prod)


def test_desc_ref_alpha_beta_bias_is_addmm():
    rs = _rs(2)
    d = _nt(rs, 6, 4, 9, alpha=0.5, beta=-0.75, bias=_f32(rs, 4), bias2=_f32(rs, 4))
    ref = torch.addmm(_t(d['C']), _t(d['A']), _t(d['B']).t(), beta=-0.75, alpha=0.5) + _t(d['bias']) + _t(d['bias2'])
    _close(R.desc_ref(d), ref)
    b = R.bound(d)
    expect = 0.5 * (_t(d['A']).abs() @ _t(d['B']).abs().t()) + 0.75 * _t(d['C']).abs() + _t(d['bias']).abs() + _t(d['bias2']).abs()
    _close(b, expect)


def test_desc_ref_addend_and_activations():
    rs = _rs(3)
    M, N, K, mod = 12, 5, 8, 4
    add = np.full((mod, N + 2), np.nan, np.float32); add[:, :N] = _f32(rs, mod, N)
    aux = np.full((M, N + 1), np.nan, np.float32); aux[:, :N] = np.tanh(_f32(rs, M, N))
    d = _nt(rs, M, N, K, addend=add, add_mod=mod, ld_add=N + 2)
    pre = _t(d['A']) @ _t(d['B']).t() + _t(add[:, :N])[torch.arange(M) % mod]
    _close(R.desc_ref(d), pre)
    _close(R.desc_ref(dict(d, act=R.ACT_TANH)), torch.tanh(pre))
    _close(R.desc_ref(dict(d, act=R.ACT_MUL_DTANH, aux=aux, ld_aux=N + 1)), pre * (1 - _t(aux[:, :N]) ** 2))
    _close(R.bound(dict(d, act=R.ACT_TANH)), _t(d['A']).abs() @ _t(d['B']).abs().t() + _t(add[:, :N]).abs()[torch.arange(M) % mod])


def test_desc_ref_batch_is_bmm():
    rs = _rs(4)
    nb, M, N, K = 3, 5, 4, 6
    A, B, bias = _f32(rs, nb, M, K), _f32(rs, nb, N, K), _f32(rs, nb, N)
    d = dict(A=A, B=B, C=np.zeros((nb, M, N), np.float32), M=M, N=N, K=K, sam=K, sak=1, sbk=1, sbn=K, ldc=N, batch=nb, bsa=M * K, bsb=N * K,
             bsc=M * N, bias=bias, bs_bias=N)
    _close(R.desc_ref(d), torch.bmm(_t(A), _t(B).transpose(1, 2)) + _t(bias)[:, None, :])
    _close(R.desc_ref(dict(d, bs_bias=0)), torch.bmm(_t(A), _t(B).transpose(1, 2)) + _t(bias)[0])
    # K slabs: batch b contracts columns [b K/3, (b+1) K/3) of ONE pair of operands (bsa = bsb = K/3, row strides unchanged)
    A2, B2 = _f32(rs, M, 3 * K), _f32(rs, N, 3 * K)
    d2 = dict(A=A2, B=B2, C=np.zeros((3, M, N), np.float32), M=M, N=N, K=K, sam=3 * K, sak=1, sbk=1, sbn=3 * K, ldc=N, batch=3, bsa=K, bsb=K, bsc=M * N)
    ref = torch.stack([_t(A2[:, b * K:(b + 1) * K]) @ _t(B2[:, b * K:(b + 1) * K]).t() for b in range(3)])
    _close(R.desc_ref(d2), ref)


def test_desc_ref_rowmap_is_a_permutation_and_ldc_keeps_padding():
    rs = _rs(5)
    M, N, K, mod, mul = 12, 3, 4, 4, 3
    d = _nt(rs, M, N, K, rowmap_mod=mod, rowmap_mul=mul, ldc=N + 2)
    C0 = _f32(rs, M + 2, N + 2)
    d['C'] = C0
    rows = torch.arange(M)
    perm = (rows % mod) * mul + rows // mod
    assert sorted(perm.tolist()) == list(range(M))
    ref = _t(C0).clone()
    ref[perm, :N] = _t(d['A']) @ _t(d['B']).t()
    _close(R.desc_ref(d), ref)
    m = R.written_mask(d).reshape(M + 2, N + 2)
    assert m[:M, :N].all() and not m[M:].any() and not m[:, N:].any()
    assert np.all(R.bound(d).reshape(M + 2, N + 2)[~m] == 0)


def test_desc_ref_row_index_is_index_add_with_clamping():
    rs = _rs(6)
    M, N, K, Rr = 20, 4, 5, 6
    idx = rs.randint(0, Rr, M).astype(np.int32)
    idx[:7] = 2                                                   # a hot row
    idx[7], idx[8] = Rr + 3, -4                                   # clamped to Rr - 1 and 0
    d = _nt(rs, M, N, K, beta=1.0, split_k=-1, row_index=idx, row_index_max=Rr - 1, bias=_f32(rs, N))
    d['C'] = _f32(rs, Rr, N)
    ref = _t(d['C']).clone()
    ref.index_add_(0, torch.from_numpy(np.clip(idx, 0, Rr - 1).astype(np.int64)), _t(d['A']) @ _t(d['B']).t() + _t(d['bias']))
    _close(R.desc_ref(d), ref)


def test_desc_ref_explicit_split_adds_once_and_ignores_beta():
    rs = _rs(7)
    d = _nt(rs, 6, 5, 40, split_k=3, beta=0.0, bias=_f32(rs, 5), addend=_f32(rs, 2, 5), add_mod=2, ld_add=5)
    ref = _t(d['C']) + _t(d['A']) @ _t(d['B']).t() + _t(d['bias']) + _t(d['addend'])[torch.arange(6) % 2]
    _close(R.desc_ref(d), ref)
    # auto split follows the formula: beta = 0 overwrites, beta = 1 accumulates
    _close(R.desc_ref(dict(d, split_k=-1, beta=0.0)), ref - _t(d['C']))
    _close(R.desc_ref(dict(d, split_k=-1, beta=1.0)), ref)


# ---- the h2 format model ---------------------------------------------------------------------------------------------------------------

def _h2_data(rs, Rw, K):
    """The dynamic range of test_gemm_h2_packed_is_fp32_accurate: per-row scales e^+-12, per-element 2^-8 .. 2^7, 5 % zeros."""
    x = (rs.standard_normal((Rw, K)) * np.exp(rs.uniform(-12, 12, (Rw, 1))) * np.exp2(rs.randint(-8, 8, (Rw, K)))).astype(np.float32)
    x[rs.uniform(size=x.shape) < 0.05] = 0.0
    return x


@pytest.mark.parametrize('Rw,K', [(1, 1), (16, 64), (128, 32), (129, 33), (130, 100), (257, 264), (5, 761)])
def test_h2_image_size_is_the_echr_h2_bytes_formula(Rw, K):
    x = _f32(_rs(Rw + K), Rw, K)
    img = R.h2_pack_ref(x)
    assert img.dtype == np.uint8 and img.size == -(-Rw // 128) * -(-K // 32) * (16384 + 512) == R.h2_bytes(Rw, K)


@pytest.mark.parametrize('Rw,K', [(16, 64), (130, 100), (257, 264), (40, 761)])
def test_h2_round_trip_within_the_derived_bound(Rw, K):
    """|xs - h1 - h2| <= max(2^-22 |xs|, 2^-25) in the segment's scaled units: two roundings to 11 significant bits leave 2^-22 relative while
    h2 is a normal fp16, and half the fp16 subnormal spacing (2^-24 / 2) below that."""
    x = _h2_data(_rs(Rw * 3 + K), Rw, K)
    back = R.h2_unpack_ref(R.h2_pack_ref(x), Rw, K)
    e, _ = R.h2_exponents(x)
    sc = np.repeat(np.exp2(14.0 - e), 256, axis=1)[:Rw, :K]      # scaled units of every element
    xs = x.astype(np.float64) * sc
    err = np.abs(back * sc - xs)
    lim = np.maximum(2.0 ** -22 * np.abs(xs), 2.0 ** -25)
    assert np.all(err <= lim), float((err / lim).max())
    assert np.abs(xs).max() < 2.0 ** 15 and np.all(np.abs(xs).reshape(-1)[np.abs(xs).argmax()] >= 2.0 ** 14)


def _planes_and_scales(img, Rw, K):
    RB, KT = -(-Rw // 128), -(-K // 32)
    return img[:RB * KT * 16384].view(np.float16).reshape(RB, KT, 2, 128, 32), img[RB * KT * 16384:].view(np.float32).reshape(RB, KT, 128)


def test_h2_layout_swizzle_and_zero_padding():
    """One non-zero element at (r, k): it must sit in chunk (r / 128, k / 32), plane 0, row r % 128, at 16-byte slot (k % 32) / 8 ^ {0,2,3,1}[(r >> 2) & 3]."""
    Rw, K = 130, 70
    for (r, k) in [(0, 0), (5, 9), (9, 17), (14, 31), (129, 69), (127, 40)]:
        x = np.zeros((Rw, K), np.float32)
        x[r, k] = 1.0                                             # xs = 2^14: exactly representable, h2 = 0
        img = R.h2_pack_ref(x)
        planes, inv = _planes_and_scales(img, Rw, K)
        nz = np.argwhere(planes != 0)
        slot = ((k % 32) // 8) ^ [0, 2, 3, 1][((r % 128) >> 2) & 3]
        assert nz.tolist() == [[r // 128, k // 32, 0, r % 128, slot * 8 + k % 8]], (r, k, nz)
        assert planes[tuple(nz[0])] == np.float16(2.0 ** 14)
        seg = (k // 32) // 8
        expect = np.ones_like(inv)
        expect[r // 128, seg * 8:(seg + 1) * 8, r % 128] = 2.0 ** -14      # every block of the segment carries the scale
        assert np.array_equal(inv, expect)


def test_h2_special_rows():
    K = 300                                                       # two segments: 256 + 44
    x = np.zeros((8, K), np.float32)
    rs = _rs(9)
    x[1] = rs.standard_normal(K) * 1e-40                          # subnormal row: scale 1
    x[2] = rs.standard_normal(K); x[2, 7] = np.inf                # an inf in the first segment: scale 1 there
    x[3] = rs.uniform(-1, 1, K) * 30; x[3, 3] = x[3, 299] = 32.0  # maximum exactly at a power of two: e = 5
    x[4] = rs.uniform(1, 1.9, K) * 2.0 ** -120                    # below the exponent floor: e = 14 - 126
    x[5, :256] = rs.uniform(-1, 1, 256) * 3.0; x[5, 0] = 3.0      # segments are scaled independently: e = 1 ...
    x[5, 256:] = rs.uniform(-1, 1, 44) * 1e6; x[5, 256] = 1e6     # ... and e = 19
    e, _ = R.h2_exponents(x)
    assert e[0].tolist() == [14, 14] and e[1].tolist() == [14, 14]
    assert e[2, 0] == 14 and e[3].tolist() == [5, 5] and e[4].tolist() == [-112, -112] and e[5].tolist() == [1, 19]
    assert e[8:].tolist() == [[14, 14]] * 120                     # padded rows: scale 1
    img = R.h2_pack_ref(x)
    planes, inv = _planes_and_scales(img, 8, K)
    assert np.all(inv[0, :, 0] == 1.0) and np.all(inv[0, :, 1] == 1.0) and np.all(inv[0, :, 8:] == 1.0)
    assert np.all(inv[0, :, 3] == 2.0 ** -9) and np.all(inv[0, :, 4] == 2.0 ** -126)
    assert np.all(inv[0, :8, 5] == 2.0 ** -13) and np.all(inv[0, 8:, 5] == 2.0 ** 5)
    assert np.all(planes[0, :, :, 0] == 0) and np.all(planes[0, :, :, 8:] == 0)          # zero row and padding
    assert np.all(planes[0, :, :, 1] == 0)                        # a subnormal row at scale 1 is below fp16's range
    back = R.h2_unpack_ref(img, 8, K)
    assert np.isinf(planes[0, 0, 0, 2]).sum() == 1 and np.isnan(back[2, 7])      # h1 = inf, h2 = inf - inf
    fin = np.ones(K, bool); fin[7] = False
    assert np.all(np.abs(back[2, fin] - x[2, fin]) <= 2.0 ** -22 * np.abs(x[2, fin]) + 2.0 ** -25)   # the rest of that row at scale 1
    sc = np.repeat(np.exp2(14.0 - e), 256, axis=1)[:8, :K]
    for r in (3, 4, 5):
        assert np.all(np.abs(back[r] - x[r]) * sc[r] <= np.maximum(2.0 ** -22 * np.abs(x[r].astype(np.float64)) * sc[r], 2.0 ** -25)), r
    assert back[3, 3] == 32.0 and np.abs(planes[0, 0, 0, 3]).max() == np.float16(2.0 ** 14)

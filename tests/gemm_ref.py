"""Host references (NumPy, float64) for the dense products of csrc/gemm.hip: the echr_gemm_desc formula of include/echr_hip.h evaluated
literally, its componentwise error scale, and a model of the h2 packed-operand format.  No GPU, no library: tests/test_gemm_ref_host.py checks
these against plain torch float64 expressions, tests/test_gpu_gemm_contract.py checks every kernel family against them.

A descriptor is a dict with the field names of echr_gemm_desc; A, B, C, bias, bias2, addend, aux and row_index are FLAT host arrays (the
whole buffers, padding included) that the strides index exactly as the device pointers would be indexed.  Missing fields take the values of
a zeroed struct, except alpha = 1, batch = 1, split_k = 1."""
import numpy as np

ACT_NONE, ACT_TANH, ACT_MUL_DTANH = 0, 1, 2

_DEFAULTS = dict(batch=1, bsa=0, bsb=0, bsc=0, alpha=1.0, beta=0.0, bias=None, bs_bias=0, bias2=None, addend=None, add_mod=0, ld_add=0,
                 act=ACT_NONE, aux=None, ld_aux=0, rowmap_mod=0, rowmap_mul=0, split_k=1, row_index=None, row_index_max=0)


def _full(d):
    f = dict(_DEFAULTS)
    f.update(d)
    return f


def _flat(x):
    return None if x is None else np.ascontiguousarray(x).reshape(-1)


def out_rows(d):
    """Output row of every logical row i: the row_index scatter (clamped), else the rowmap permutation, else i."""
    d = _full(d)
    i = np.arange(d['M'])
    if d['row_index'] is not None:
        return np.clip(_flat(d['row_index'])[:d['M']].astype(np.int64), 0, d['row_index_max'])
    if d['rowmap_mod'] > 0:
        return (i % d['rowmap_mod']) * d['rowmap_mul'] + i // d['rowmap_mod']
    return i


def _accumulates(d):
    # split_k > 1: "C must already hold its base value, beta is ignored"; row_index: rows are ADDED into C
    return d['split_k'] > 1 or d['row_index'] is not None


def _terms(d, absolute):
    """Per batch b: (pre-activation contribution of everything but C_old, as [M, N] float64).  absolute: every factor by its magnitude."""
    d = _full(d)
    f = (lambda x: np.abs(x)) if absolute else (lambda x: x)
    M, N, K = d['M'], d['N'], d['K']
    A, B = _flat(d['A']), _flat(d['B'])
    i, j, k = np.arange(M, dtype=np.int64), np.arange(N, dtype=np.int64), np.arange(K, dtype=np.int64)
    out = []
    for b in range(d['batch']):
        a = f(A[b * d['bsa'] + i[:, None] * d['sam'] + k[None, :] * d['sak']].astype(np.float64))
        w = f(B[b * d['bsb'] + k[:, None] * d['sbk'] + j[None, :] * d['sbn']].astype(np.float64))
        v = f(np.float64(np.float32(d['alpha']))) * (a @ w)
        if d['bias'] is not None:
            v = v + f(_flat(d['bias'])[b * d['bs_bias'] + j].astype(np.float64))[None, :]
        if d['bias2'] is not None:
            v = v + f(_flat(d['bias2'])[j].astype(np.float64))[None, :]
        if d['addend'] is not None:
            v = v + f(_flat(d['addend'])[(i % d['add_mod'])[:, None] * d['ld_add'] + j[None, :]].astype(np.float64))
        out.append(v)
    return out


def _scatter(d, C, old, terms, absolute):
    """Write (or, in the accumulate forms, add) the per-batch terms into the flat buffer C; `old` is what beta multiplies."""
    d = _full(d)
    M, N = d['M'], d['N']
    i, j = np.arange(M, dtype=np.int64), np.arange(N, dtype=np.int64)
    orow = out_rows(d)
    beta = np.float64(np.float32(d['beta']))
    for b, v in enumerate(terms):
        idx = b * d['bsc'] + orow[:, None] * d['ldc'] + j[None, :]
        if _accumulates(d):
            np.add.at(C, idx, v)                                   # duplicates of a row_index target all land
            continue
        if beta != 0.0:
            v = v + (abs(beta) if absolute else beta) * old[idx]
        if not absolute:
            if d['act'] == ACT_TANH:
                v = np.tanh(v)
            elif d['act'] == ACT_MUL_DTANH:
                t = _flat(d['aux'])[i[:, None] * d['ld_aux'] + j[None, :]].astype(np.float64)
                v = v * (1.0 - t * t)
        C[idx] = v
    return C


def desc_ref(d):
    """The whole C buffer (float64, flat, padding included) after echr_gemm_f32(d), from d['C'] as C_old:
        C[b][rowmap(i)][j] = act(alpha * sum_k A[b](i,k) B[b](k,j) + beta * C_old + bias[b*bs_bias + j] + bias2[j] + addend[i % add_mod][j])
    split_k == 1 and split_k < 0 (auto; beta in {0, 1}) follow the formula; an explicit split_k > 1 and a row_index scatter ADD the product,
    the biases and the addend -- each exactly once -- to what C holds and ignore beta.  aux and addend are indexed by the logical row i."""
    old = _flat(d['C']).astype(np.float64)
    return _scatter(d, old.copy(), old, _terms(d, False), False)


def bound(d):
    """Componentwise scale |alpha| (|A| |B|) + |beta| |C_old| + |bias| + |bias2| + |addend| of the PRE-activation value, laid out like the C
    buffer (cells the product does not write hold 0).  tanh is 1-Lipschitz and |1 - aux^2| <= 1, so an error of tol * bound before the
    activation is at most tol * bound after it; in the accumulate forms C_old counts with coefficient 1."""
    old = np.abs(_flat(d['C']).astype(np.float64))
    C = old * written_mask(d) if _accumulates(_full(d)) else np.zeros_like(old)
    return _scatter(d, C, old, _terms(d, True), True)


def written_mask(d):
    """Boolean mask over the flat C buffer: the cells the call may write."""
    dd = _full(d)
    m = np.zeros(_flat(d['C']).shape, dtype=bool)
    j = np.arange(dd['N'], dtype=np.int64)
    orow = out_rows(d)
    for b in range(dd['batch']):
        m[b * dd['bsc'] + orow[:, None] * dd['ldc'] + j[None, :]] = True
    return m


# ---- the h2 packed-operand format (csrc/gemm.hip, "h2 operands"; include/echr_hip.h echr_h2_pack) ----------------------------------------
H2_ROWS, H2_BK, H2_SEG = 128, 32, 8
H2_PLANE = H2_ROWS * H2_BK * 2          # bytes of one fp16 plane of a chunk
H2_CHUNK = 2 * H2_PLANE
H2_SCALES = H2_ROWS * 4
_SWZ = np.array([0, 2, 3, 1])


def h2_bytes(R, K):
    return -(-R // H2_ROWS) * -(-K // H2_BK) * (H2_CHUNK + H2_SCALES)


def h2_exponents(x):
    """Block exponent e per (row, 256-wide k segment) of the zero-padded operand: floor(log2 max|x|), 14 (scale 1) for zero, subnormal and
    non-finite maxima, floored at 14 - 126 so that 2^(14 - e) stays a normal fp32.  NaN elements do not take part in the maximum (fmaxf)."""
    R, K = x.shape
    RB, KT = -(-R // H2_ROWS), -(-K // H2_BK)
    KS = -(-KT // H2_SEG)
    xp = np.zeros((RB * H2_ROWS, KS * H2_SEG * H2_BK), dtype=np.float32)
    xp[:R, :K] = x
    mx = np.fmax.reduce(np.abs(xp).reshape(RB * H2_ROWS, KS, H2_SEG * H2_BK), axis=2, initial=np.float32(0))
    ex = ((mx.astype(np.float32).view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    e = np.where((ex == 0) | (ex == 255), 14, ex - 127)
    return np.maximum(e, 14 - 126), xp


def h2_pack_ref(x):
    """The full packed image (uint8 array of h2_bytes(R, K) bytes) of the logical [R, K] fp32 operand x, k = the contraction axis:
    chunks [ceil(R/128)][ceil(K/32)] of two 128 x 32 fp16 planes (h1 = fp16(xs), h2 = fp16(xs - h1), xs = x * 2^(14 - e)), 16-byte slot s of
    row r at physical slot s ^ {0,2,3,1}[(r >> 2) & 3], zero padding; then the inverse scales 2^(e - 14) as [ceil(R/128)][ceil(K/32)][128] fp32."""
    x = np.asarray(x, dtype=np.float32)
    R, K = x.shape
    RB, KT = -(-R // H2_ROWS), -(-K // H2_BK)
    e, xp = h2_exponents(x)
    e_blk = np.repeat(e, H2_SEG, axis=1)[:, :KT]                                        # [rows, KT]
    with np.errstate(invalid='ignore', over='ignore'):
        xs = (xp[:, :KT * H2_BK].reshape(RB * H2_ROWS, KT, H2_BK) * np.ldexp(np.float32(1), 14 - e_blk)[:, :, None].astype(np.float32)).astype(np.float32)
        h1 = xs.astype(np.float16)
        h2 = (xs - h1.astype(np.float32)).astype(np.float16)
    r = np.arange(H2_ROWS)
    phys = (np.arange(4)[None, :] ^ _SWZ[(r >> 2) & 3][:, None])                        # [row, logical slot] -> physical slot
    planes = np.zeros((RB, KT, 2, H2_ROWS, 4, 8), dtype=np.uint16)
    for p, h in enumerate((h1, h2)):
        v = h.view(np.uint16).reshape(RB, H2_ROWS, KT, 4, 8).transpose(0, 2, 1, 3, 4)  # [RB, KT, row, logical slot, 8]
        planes[:, :, p, r[:, None], phys, :] = v
    inv = np.ldexp(np.float32(1), e_blk - 14).astype(np.float32).reshape(RB, H2_ROWS, KT).transpose(0, 2, 1)
    return np.concatenate([planes.reshape(-1).view(np.uint8), np.ascontiguousarray(inv).reshape(-1).view(np.uint8)])


def h2_unpack_ref(img, R, K):
    """Inverse of h2_pack_ref: the float64 [R, K] operand (h1 + h2) * inverse scale an image stands for."""
    img = np.asarray(img, dtype=np.uint8)
    RB, KT = -(-R // H2_ROWS), -(-K // H2_BK)
    assert img.size == h2_bytes(R, K)
    planes = img[:RB * KT * H2_CHUNK].view(np.float16).reshape(RB, KT, 2, H2_ROWS, 4, 8)
    inv = img[RB * KT * H2_CHUNK:].view(np.float32).reshape(RB, KT, H2_ROWS)
    r = np.arange(H2_ROWS)
    phys = (np.arange(4)[None, :] ^ _SWZ[(r >> 2) & 3][:, None])
    with np.errstate(invalid='ignore'):
        v = planes[:, :, :, r[:, None], phys, :].astype(np.float64).sum(axis=2)         # [RB, KT, row, logical slot, 8]
        v = v * inv.astype(np.float64)[:, :, :, None, None]
    return v.transpose(0, 2, 1, 3, 4).reshape(RB * H2_ROWS, KT * H2_BK)[:R, :K]

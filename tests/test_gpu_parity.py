"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on the same seeded
inputs and against the golden fixtures generated from the reference (tests/golden, tools/make_golden.py).

Tolerances (north_star): log-probs / losses within 1e-4 relative of the reference's PyTorch-CPU path; index
outputs bit-exact.  Gradients: 1e-3 of each tensor's max-norm (fp32 atomics reorder sums; measured ~1e-6)."""
import os

import numpy as np
import pytest
import torch

from echr_amd import synth
from oracle import summary as SM
from tests import util as U

pytestmark = pytest.mark.gpu

# measured noise of the HIP path against the oracle at the benchmarked size (tools/parity_report.py): max |d logp| 1.9e-6, loss 1.1e-7
# relative, worst gradient entry 1.2e-6 of its tensor's max-norm.  The gates sit 10x above that -- two orders inside north_star's 1e-4.
TOL_LOGP = 2e-5     # absolute on log-probs of magnitude ~8.5 => ~2e-6 relative
TOL_LOSS = 1e-5     # relative
TOL_GRAD = 1e-5     # relative to the tensor's max-norm


def test_library_loaded_on_gpu():
    from echr_amd import _lib
    lib = _lib.load()
    assert lib.echr_version() == _lib.ABI_VERSION == 3


@pytest.mark.parametrize('M,N,K,trans_b', [(64, 64, 32, True), (130, 70, 100, True), (1280, 513, 1536, True),
                                           (64, 2048, 512, True), (200, 96, 500, False), (5, 7, 3, True),
                                           (257, 5001, 64, True), (64, 500, 2048, False),
                                           # large NT shapes: the 128 x 128 double-buffered kernel (ragged M / N, K tail, K = 500)
                                           (1280, 5001, 1536, True), (1300, 1537, 500, True), (4100, 1536, 1284, True), (8192, 512, 500, True)])
def test_gemm_f32(M, N, K, trans_b):
    from echr_amd import functional as EF
    rs = np.random.RandomState(M * 7 + N)
    A = rs.standard_normal((M, K)).astype(np.float32)
    B = rs.standard_normal((N, K) if trans_b else (K, N)).astype(np.float32)
    bias = rs.standard_normal(N).astype(np.float32)
    ref = A.astype(np.float64) @ (B.T if trans_b else B).astype(np.float64) + bias
    out = EF.gemm(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), trans_b, torch.from_numpy(bias).cuda()).cpu().numpy()
    scale = np.abs(A).astype(np.float64) @ np.abs(B.T if trans_b else B).astype(np.float64) + 1.0
    assert np.max(np.abs(out - ref) / scale) < 1e-6, np.max(np.abs(out - ref) / scale)


@pytest.mark.parametrize('M,N,K', [(128, 128, 32), (1280, 5001, 1536), (300, 700, 500), (4096, 512, 512), (130, 257, 36)])
def test_gemm_bf16x3_split_is_fp32_accurate(M, N, K):
    """The three-plane bf16 split product must be as accurate as the exact fp32 MFMA path (both against float64)."""
    from echr_amd import functional as EF
    rs = np.random.RandomState(M + N + K)
    A = (rs.standard_normal((M, K)) * np.exp(rs.uniform(-6, 6, (M, 1)))).astype(np.float32)      # wide dynamic range
    B = (rs.standard_normal((N, K)) * np.exp(rs.uniform(-6, 6, (N, 1)))).astype(np.float32)
    ref = A.astype(np.float64) @ B.T.astype(np.float64)
    scale = np.abs(A).astype(np.float64) @ np.abs(B.T).astype(np.float64) + 1e-30
    At, Bt = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    e32 = np.max(np.abs(EF.gemm(At, Bt, True, None, 0).cpu().numpy() - ref) / scale)
    esp = np.max(np.abs(EF.gemm(At, Bt, True, None, 1).cpu().numpy() - ref) / scale)
    assert esp < 4e-7 and esp < 4 * e32 + 1e-7, (esp, e32)


@pytest.mark.parametrize('M,N,K', [(128, 128, 32), (1280, 5001, 1536), (300, 700, 500), (4096, 512, 512), (130, 257, 36), (77, 3, 8200)])
def test_gemm_h2_packed_is_fp32_accurate(M, N, K):
    """Two block-scaled fp16 planes + three fp16 MFMA products must be as accurate as the exact fp32 MFMA path (both against
    float64, componentwise bound), over a wide dynamic range, and a transposing pack must give the identical image."""
    from echr_amd import functional as EF
    rs = np.random.RandomState(M + N + K)
    A = (rs.standard_normal((M, K)) * np.exp(rs.uniform(-12, 12, (M, 1))) * np.exp2(rs.randint(-8, 8, (M, K)))).astype(np.float32)
    B = (rs.standard_normal((N, K)) * np.exp(rs.uniform(-12, 12, (N, 1)))).astype(np.float32)
    A[rs.uniform(size=A.shape) < 0.05] = 0.0
    A[M // 2] = 0.0                                                      # an all-zero row: scale stays 1
    bias = rs.standard_normal(N).astype(np.float32)
    ref = A.astype(np.float64) @ B.T.astype(np.float64)
    scale = np.abs(A).astype(np.float64) @ np.abs(B.T).astype(np.float64) + 1e-300
    At, Bt = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    pa, pb = EF.h2_pack(At), EF.h2_pack(Bt)
    pbt = EF.h2_pack(Bt.t().contiguous(), transposed=True)
    assert torch.equal(pb[0], pbt[0])
    out = EF.gemm_h2(pa, pb).cpu().numpy()
    e32 = np.max(np.abs(EF.gemm(At, Bt, True, None, 0).cpu().numpy() - ref) / scale)
    eh2 = np.max(np.abs(out - ref) / scale)
    assert eh2 < 6e-7 and eh2 < 2 * e32 + 5e-8, (eh2, e32)
    assert np.all(out[M // 2] == 0.0)
    outb = EF.gemm_h2(pa, pb, torch.from_numpy(bias).cuda()).cpu().numpy()
    assert np.max(np.abs(outb - (out.astype(np.float64) + bias)) / (scale + np.abs(bias))) < 1e-6     # split-K sums are order-dependent


def test_gemm_h2_adversarial_segment_outlier():
    """The documented bound of the h2 format: one element 2^20 above the rest of its 256-wide k segment sets the
    segment's scale, so the small elements keep 2^-39 of that maximum as absolute error -- the product's error stays below
    2^-38 * sum_segments(segmax_a * sum|b|), and the signal carried by the small elements survives to ~2^-18 relative."""
    from echr_amd import functional as EF
    rs = np.random.RandomState(7)
    M, N, K = 128, 128, 512
    A = rs.standard_normal((M, K)).astype(np.float32)
    B = rs.standard_normal((N, K)).astype(np.float32)
    A[:, 5] = np.float32(2.0 ** 20) * np.sign(A[:, 5])          # one outlier per row in the first segment
    B[:, 5] = 0.0                                                # ... that the product never sees: the signal is in the small elements
    ref = A.astype(np.float64) @ B.T.astype(np.float64)
    out = EF.gemm_h2(EF.h2_pack(torch.from_numpy(A).cuda()), EF.h2_pack(torch.from_numpy(B).cuda())).cpu().numpy()
    seg = np.abs(A).reshape(M, K // 256, 256).max(axis=2)                           # [M, segments]
    babs = np.abs(B).reshape(N, K // 256, 256).sum(axis=2)                          # [N, segments]
    bound = 2.0 ** -38 * (seg.astype(np.float64) @ babs.T.astype(np.float64)) + 1e-6 * (np.abs(A).astype(np.float64) @ np.abs(B.T).astype(np.float64))
    err = np.abs(out - ref)
    assert np.all(err <= bound), float((err / bound).max())
    assert err.max() / np.abs(ref).max() < 2.0 ** -16                               # the small-element signal is still there


def test_persistent_abort_path():
    """Failure path of the persistent recurrences, once and deterministically: a diagnostic switch makes ONE hand-off wait (the q edge of
    timestep 3) never complete.  The grid must drain through its bounded spins; while the abort is unacknowledged the fused optimiser
    kernel must NOT touch its buffers; the next check must return -ETIME naming the wait (once); the next forward (persistent kernels on)
    must be right again."""
    from echr_amd import _lib
    from echr_amd import functional as EF
    lib = _lib.load()
    opt, params, vid = synth.make_case('c2')
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels = torch.from_numpy(vid['labels'])
    m = U.build_gpu_model(opt, params, True)
    p = torch.ones(4096, device=dev)
    g = torch.full((4096,), 0.5, device=dev)
    mom, var = torch.zeros_like(p), torch.zeros_like(p)
    try:
        assert lib.echr_config_set(b'persist_spin_limit', 20000) == 0          # tens of milliseconds instead of seconds
        assert lib.echr_config_set(b'persist_inject_timeout', 200000 + 3) == 0
        with torch.no_grad():
            m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')     # ONE library call that launches the forward pair
        torch.cuda.synchronize()                                               # the grid drained: nothing hangs
        EF.clamp_adam_(p, g, mom, var, 1, 1e-2)                                # enqueued behind an unacknowledged abort: skipped on device
        EF.clamp_(g, 0.1)
        torch.cuda.synchronize()
        assert bool((p == 1).all()) and bool((mom == 0).all()) and bool((g == 0.5).all())
        assert lib.echr_check_async() == -62
        msg = lib.echr_last_error().decode()
        assert 'code 200003' in msg and 'timestep 3' in msg, msg
        assert lib.echr_check_async() == 0                                     # reported once, abort word cleared
        EF.clamp_adam_(p, g, mom, var, 1, 1e-2)
        torch.cuda.synchronize()
        assert bool((p < 1).all())                                             # ... and the optimiser kernel works again
    finally:
        lib.echr_config_set(b'persist_inject_timeout', 0)
        lib.echr_config_set(b'persist_spin_limit', 0)
    # the following forward (persistent kernels on) is correct again: same log-probs as the launch-per-phase path
    with torch.no_grad():
        m.set_dropout_state(U.SEED, U.OFFSET)
        good = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
        try:
            lib.echr_config_set(b'persist', 0)
            m.set_dropout_state(U.SEED, U.OFFSET)
            ref = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
        finally:
            lib.echr_config_set(b'persist', 1)
    torch.cuda.synchronize()
    assert lib.echr_check_async() == 0
    assert float((good - ref).abs().max()) < TOL_LOGP


def test_cooperative_persistent_launch_equals_plain_launch():
    """persist_coop = 1 (what data-parallel runs use: the grid starts only when all 256 workgroups can be resident): same results."""
    from echr_amd import _lib
    lib = _lib.load()
    opt, params, vid = synth.make_case('c2full')
    outs = {}
    try:
        for coop in (0, 1):
            assert lib.echr_config_set(b'persist_coop', coop) == 0
            pred, loss, grads, _ = U.run_gpu(opt, params, vid, True)
            outs[coop] = (pred, loss, grads)
    finally:
        lib.echr_config_set(b'persist_coop', 0)
    assert np.abs(outs[0][0] - outs[1][0]).max() < 1e-5
    for k, g in outs[0][2].items():
        if g is not None:
            assert U.grad_close(k, outs[1][2][k], g, TOL_GRAD), k


@pytest.mark.parametrize('layout', ['NT', 'NN', 'TN'])
@pytest.mark.parametrize('M,N,K,pad', [(128, 128, 64, 0), (762, 1536, 1001, 0), (762, 1536, 1001, 3), (130, 257, 100, 0), (513, 502, 1000, 1), (300, 131, 67, 2)])
def test_gemm_f32_t128_every_layout(layout, M, N, K, pad):
    """gemm_f32_t128_kernel (the exact-fp32 128 x 128 tile, round 6) forced on every layout the path issues -- NT (nn.Linear forward), NN (data
    gradients), TN (weight gradients) -- with aligned, ragged and unaligned (pad: leading dimensions that are not multiples of 4, i.e. the
    scalar staging path) operands, unsplit and with the automatic k split: against float64.  One fp32 fma chain over K terms: ~sqrt(K) ulp."""
    import ctypes as C
    from echr_amd import _lib as L
    lib = L.load()
    dev = torch.device('cuda')
    g = torch.Generator(device='cpu').manual_seed(M * 7 + N * 3 + K)
    if layout == 'NT':
        A = torch.randn(M, K + pad, generator=g).to(dev)[:, :K]; B = torch.randn(N, K + pad, generator=g).to(dev)[:, :K]
        st = (K + pad, 1, 1, K + pad); ref = A.double() @ B.double().t()
    elif layout == 'NN':
        A = torch.randn(M, K + pad, generator=g).to(dev)[:, :K]; B = torch.randn(K, N + pad, generator=g).to(dev)[:, :N]
        st = (K + pad, 1, N + pad, 1); ref = A.double() @ B.double()
    else:
        A = torch.randn(K, M + pad, generator=g).to(dev)[:, :M]; B = torch.randn(K, N + pad, generator=g).to(dev)[:, :N]
        st = (1, M + pad, N + pad, 1); ref = A.double().t() @ B.double()
    try:
        assert lib.echr_config_set(b'gemm_tile', ord('t')) == 0
        for split in (-1, 1):
            Cc = torch.full((M, N), 7.0, device=dev)
            d = L.GemmDesc()
            d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), Cc.data_ptr()
            d.M, d.N, d.K = M, N, K
            d.sam, d.sak, d.sbk, d.sbn = st
            d.ldc, d.batch, d.alpha, d.beta, d.split_k, d.algo = N, 1, 1.0, 0.0, split, 0
            L.check(lib.echr_gemm_f32(C.byref(d), L.stream_ptr()), 'gemm')
            torch.cuda.synchronize()
            err = float((Cc.double() - ref).abs().max() / ref.abs().max())
            assert err < 1e-5, (layout, M, N, K, pad, split, err)
    finally:
        lib.echr_config_set(b'gemm_tile', 0)


def test_gemm_f32_t128_k_split_rule_and_wave_forms():
    """The library's OWN choice (no tile override) for the exact-fp32 products it sends to the 128 x 128 tile: the 240-tile logits shape
    (eight-wave form of the kernel: launches of at most one workgroup per CU; unsplit, with bias), the K-heavy 72-tile d OUTD shape (eight-wave
    form on 3 k slices, accumulating into a pre-filled C as the backward pass calls it) and a 480-tile shape (four-wave form, two workgroups per
    CU) -- against float64."""
    import ctypes as C
    from echr_amd import _lib as L
    lib = L.load()
    dev = torch.device('cuda')
    lib.echr_config_set(b'gemm_h2', 0); lib.echr_config_set(b'gemm_bf16x3', 0)
    try:
        for (M, N, K, beta, bias) in [(762, 5001, 1536, 0.0, True), (762, 1536, 5004, 1.0, False), (5001, 1536, 764, 0.0, False)]:
            g = torch.Generator(device='cpu').manual_seed(M + N + K)
            A, B = torch.randn(M, K, generator=g).to(dev), torch.randn(N, K, generator=g).to(dev)
            C0 = torch.randn(M, N, generator=g).to(dev) if beta else torch.zeros(M, N, device=dev)
            bv = torch.randn(N, generator=g).to(dev) if bias else None
            Cc = C0.clone()
            d = L.GemmDesc()
            d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), Cc.data_ptr()
            d.M, d.N, d.K = M, N, K
            d.sam, d.sak, d.sbk, d.sbn = K, 1, 1, K
            d.ldc, d.batch, d.alpha, d.beta, d.split_k, d.algo = N, 1, 1.0, beta, -1, 0
            if bias:
                d.bias = bv.data_ptr()
            L.check(lib.echr_gemm_f32(C.byref(d), L.stream_ptr()), 'gemm')
            torch.cuda.synchronize()
            ref = A.double() @ B.double().t() + (C0.double() if beta else 0.0) + (bv.double() if bias else 0.0)
            err = float((Cc.double() - ref).abs().max() / ref.abs().max())
            assert err < 1e-5, (M, N, K, err)
    finally:
        lib.echr_config_set(b'gemm_h2', 1); lib.echr_config_set(b'gemm_bf16x3', 1)


@pytest.mark.parametrize('shape', [(300, 260, 96), (2100, 2100, 96)])          # 9 tiles: the eight-wave form; 289 tiles: the four-wave form
def test_gemm_f32_t128_epilogues(shape):
    """Every epilogue mode of echr_gemm_f32 through the 128 x 128 tile (tile override 't'; NT operands; small launch = eight waves of 64 x 32,
    large launch = four waves of 64 x 64): bias + bias2 + tanh, the broadcast addend, the output row remap, accumulate (beta = 1) and the
    (1 - aux^2) gradient form -- against float64."""
    import ctypes as C
    from echr_amd import _lib as L
    lib = L.load()
    dev = torch.device('cuda')
    M, N, K = shape
    g = torch.Generator(device='cpu').manual_seed(M + 3 * N + K)
    A, B = (0.3 * torch.randn(M, K, generator=g)).to(dev), (0.3 * torch.randn(N, K, generator=g)).to(dev)
    b1, b2 = torch.randn(N, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
    add_mod = 20 if M % 20 == 0 else 1
    addend = torch.randn(add_mod, N, generator=g).to(dev)
    aux = torch.tanh(torch.randn(M, N, generator=g)).to(dev)
    C0 = torch.randn(M, N, generator=g).to(dev)
    prod = A.double() @ B.double().t()
    rows = torch.arange(M)
    cases = {
        'bias+bias2+tanh': (dict(bias=b1, bias2=b2, act=1), torch.tanh(prod + b1.double() + b2.double())),
        'addend': (dict(addend=addend, add_mod=add_mod, ld_add=N), prod + addend.double()[rows % add_mod]),
        'accumulate': (dict(beta=1.0), prod + C0.double()),
        'mul_dtanh': (dict(act=2, aux=aux, ld_aux=N), prod * (1.0 - aux.double() ** 2)),
    }
    if M % 20 == 0:
        mod, mul = 20, M // 20
        perm = (rows % mod) * mul + rows // mod
        ref = torch.empty_like(prod)
        ref[perm.to(dev)] = prod
        cases['rowmap'] = (dict(rowmap_mod=mod, rowmap_mul=mul), ref)
    try:
        assert lib.echr_config_set(b'gemm_tile', ord('t')) == 0
        for name, (kw, ref) in cases.items():
            Cc = C0.clone() if kw.get('beta') else torch.full((M, N), 3.0, device=dev)
            d = L.GemmDesc()
            d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), Cc.data_ptr()
            d.M, d.N, d.K = M, N, K
            d.sam, d.sak, d.sbk, d.sbn = K, 1, 1, K
            d.ldc, d.batch, d.alpha, d.beta, d.split_k, d.algo = N, 1, 1.0, kw.get('beta', 0.0), 1, 0
            for k in ('bias', 'bias2', 'addend', 'aux'):
                if k in kw:
                    setattr(d, k, kw[k].data_ptr())
            for k in ('add_mod', 'ld_add', 'act', 'ld_aux', 'rowmap_mod', 'rowmap_mul'):
                if k in kw:
                    setattr(d, k, kw[k])
            L.check(lib.echr_gemm_f32(C.byref(d), L.stream_ptr()), 'gemm ' + name)
            torch.cuda.synchronize()
            err = float((Cc.double() - ref).abs().max() / ref.abs().max())
            assert err < 1e-5, (name, shape, err)
    finally:
        lib.echr_config_set(b'gemm_tile', 0)


def test_gemm_row_index_scatter():
    """echr_gemm_desc.row_index: row i of A . B^T is ADDED into C[row_index[i]] (duplicates allowed, out-of-range indices clamped)."""
    import ctypes as C
    from echr_amd import _lib as L
    lib = L.load()
    rs = np.random.RandomState(3)
    M, N, K, R = 300, 96, 64, 40
    A = torch.from_numpy(rs.standard_normal((M, K)).astype(np.float32)).cuda()
    B = torch.from_numpy(rs.standard_normal((N, K)).astype(np.float32)).cuda()
    idx = rs.randint(0, R, size=M).astype(np.int32)
    idx[:30] = 0                                                    # a hot row
    idx[30] = R + 5                                                 # clamped to R - 1
    out = torch.ones(R, N, device='cuda')
    d = L.GemmDesc()
    d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), out.data_ptr()
    d.M, d.N, d.K = M, N, K
    d.sam, d.sak, d.sbk, d.sbn, d.ldc = K, 1, 1, K, N
    d.batch, d.alpha, d.beta, d.split_k, d.algo = 1, 1.0, 1.0, -1, 0
    it = torch.from_numpy(idx).cuda()
    d.row_index, d.row_index_max = it.data_ptr(), R - 1
    L.check(lib.echr_gemm_f32(C.byref(d), L.stream_ptr()), 'gemm_f32')
    ref = np.ones((R, N))
    prod = A.cpu().numpy().astype(np.float64) @ B.cpu().numpy().astype(np.float64).T
    for i in range(M):
        ref[min(idx[i], R - 1)] += prod[i]
    assert np.abs(out.cpu().numpy() - ref).max() < 1e-3


def test_position_embedding_matches_reference_numpy():
    from echr_amd import functional as EF
    g = U.gold('position.npz')
    for k in ('a', 'b'):
        soi = g[k + '|soi']
        st = torch.from_numpy(soi[:, 0].astype(np.int32)).cuda()
        ln = torch.from_numpy((soi[:, 1] - soi[:, 0]).astype(np.int32)).cuda()
        for d, key in ((512, '|pos_emb_f32'), (32, '|pos_emb32_f32')):
            pos = EF.position_embedding(st, ln, d).cpu().numpy()
            err = np.abs(pos - g[k + key]).max()
            # float64 math on device.  log(l_j/l_i) is float32 in the reference (numpy's SIMD logf, <= 1 ulp); the device
            # rounds the float64 log to float32 (correctly rounded), so the two can differ by one float32 ulp of a value
            # <= ~5, i.e. <= 4.8e-7 * 100 in the sin/cos argument.
            assert err < 5e-5, (k, d, err)


def test_event_pool_gather():
    from echr_amd import functional as EF
    from oracle import echr_ref_cpu as O
    opt, params, vid = synth.make_case('c2')
    c3d, tap = torch.from_numpy(vid['c3d']), torch.from_numpy(vid['tap'])
    ev = EF.event_index_tensors(vid['soi'], vid['ind'], torch.device('cuda'))
    ech = EF.EventPoolGather.apply(c3d.cuda(), tap.cuda(), ev[0], ev[1], ev[2]).cpu()
    ref = torch.cat((O.event_pool(c3d, vid['soi']), tap[torch.from_numpy(vid['ind'])]), 1)
    assert float((ech - ref).abs().max()) < 1e-5


@pytest.mark.parametrize('case', ['tiny', 'c1', 'c2'])
@pytest.mark.parametrize('train_mode', [False, True])
def test_event_context_tsrm(case, train_mode):
    """fusion_model (TSRM) forward + backward against the oracle, eval and train (dropout) mode."""
    from echr_amd import functional as EF
    from oracle import echr_ref_cpu as O
    opt, params, vid = synth.make_case(case)
    m = U.build_gpu_model(opt, params, train_mode)
    dev = torch.device('cuda')
    N = len(vid['soi'])
    P = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in params.items()}
    dm = U.oracle_drop(opt)('tsrm', 0, (N, opt.n_head, N)) if train_mode else None
    ref = O.event_context(P, torch.from_numpy(vid['tap']), torch.from_numpy(vid['c3d']), vid['ind'], vid['soi'], opt.n_head, dm)
    ev = EF.event_index_tensors(vid['soi'], vid['ind'], dev)
    drop = EF.DropState(U.SEED, U.OFFSET, train_mode)
    out = m.get_event_context(torch.from_numpy(vid['tap']).to(dev), torch.from_numpy(vid['c3d']).to(dev), None, vid['ind'], vid['soi'],
                              _ev=ev, _drop=drop)
    assert U.relerr(out.detach().cpu().numpy(), ref.detach().numpy()) < 1e-5
    if not train_mode:
        gold = U.gold('case_%s.npz' % case)['event_context']
        assert U.relerr(out.detach().cpu().numpy(), gold) < 1e-5
    w = torch.from_numpy(np.random.RandomState(1).standard_normal(tuple(ref.shape)).astype(np.float32))
    (ref * w).sum().backward()
    (out * w.to(dev)).sum().backward()
    for k, p in m.named_parameters():
        if not k.startswith('fusion_model.') or P[k].grad is None:
            continue
        assert U.relerr(p.grad.cpu().numpy(), P[k].grad.numpy()) < TOL_GRAD, k


def test_event_context_many_events_vs_oracle():
    """More than 64 events (evaluation-style batches: N * N >= 4096 pairs): the pair MLP's fc2 runs on the streaming 16-row-tile kernel and
    the position embedding is written packed for the fc1 product (and as fp32 for the backward pass); forward + backward against the oracle, and against the general kernels."""
    from echr_amd import functional as EF
    from echr_amd import _lib
    from oracle import echr_ref_cpu as O
    lib = _lib.load()
    opt = synth.default_opt(vocab_size=300, seq_length=6)
    params = synth.make_params(opt, 5)
    vid = synth.make_video(80, 24, 8, 301, seed=9, T_v=200)
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    P = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in params.items()}
    ref = O.event_context(P, torch.from_numpy(vid['tap']), torch.from_numpy(vid['c3d']), vid['ind'], vid['soi'], opt.n_head, None)
    ev = EF.event_index_tensors(vid['soi'], vid['ind'], dev)
    tap, c3d = torch.from_numpy(vid['tap']).to(dev), torch.from_numpy(vid['c3d']).to(dev)
    outs = []
    try:
        for flag in (1, 0):
            for key in (b'gemm_skinny', b'posemb_rows', b'posemb_packed'):
                lib.echr_config_set(key, flag)
            out = m.get_event_context(tap, c3d, None, vid['ind'], vid['soi'], _ev=ev, _drop=EF.DropState(U.SEED, U.OFFSET, False))
            outs.append(out)
    finally:
        for key in (b'gemm_skinny', b'posemb_rows', b'posemb_packed'):
            lib.echr_config_set(key, 1)
    with torch.no_grad():          # inference: the fp32 position embedding is never materialised (echr_tsrm_args.inference)
        out_ng = m.get_event_context(tap, c3d, None, vid['ind'], vid['soi'], _ev=ev, _drop=EF.DropState(U.SEED, U.OFFSET, False))
    assert U.relerr(outs[0].detach().cpu().numpy(), ref.detach().numpy()) < 1e-5
    assert U.relerr(outs[0].detach().cpu().numpy(), outs[1].detach().cpu().numpy()) < 2e-6
    assert U.relerr(out_ng.cpu().numpy(), outs[0].detach().cpu().numpy()) < 2e-6
    w = torch.from_numpy(np.random.RandomState(1).standard_normal(tuple(ref.shape)).astype(np.float32))
    (ref * w).sum().backward()
    (outs[0] * w.to(dev)).sum().backward()
    for k, p in m.named_parameters():
        if not k.startswith('fusion_model.') or P[k].grad is None:
            continue
        assert U.relerr(p.grad.cpu().numpy(), P[k].grad.numpy()) < TOL_GRAD, k


def test_event_context_inference_tables_vs_oracle():
    """Inference over >= 16384 event pairs (evaluation batches): fc1 of the pair MLP is tabulated over the distinct integer keys
    (|2 dc|, l_i) and (l_i, l_j) and the gates are formed from two gathered table rows per pair (echr_tsrm_args.inference + max_len / max_span).
    Against the oracle, against the dense path (grad mode / pair_tables = 0), and with bounds the host did not supply (dense fallback)."""
    from echr_amd import functional as EF
    from echr_amd import _lib
    from oracle import echr_ref_cpu as O
    lib = _lib.load()
    opt = synth.default_opt(vocab_size=300, seq_length=6)
    params = synth.make_params(opt, 7)
    vid = synth.make_video(200, 24, 8, 301, seed=13, T_v=200, min_len=1)
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    P = {k: torch.from_numpy(v) for k, v in params.items()}
    with torch.no_grad():
        ref = O.event_context(P, torch.from_numpy(vid['tap']), torch.from_numpy(vid['c3d']), vid['ind'], vid['soi'], opt.n_head, None).numpy()
    ev = EF.event_index_tensors(vid['soi'], vid['ind'], dev)
    assert ev[1].echr_bounds[0] == 24 and ev[1].echr_bounds[1] > 0
    tap, c3d = torch.from_numpy(vid['tap']).to(dev), torch.from_numpy(vid['c3d']).to(dev)

    def run():
        return m.get_event_context(tap, c3d, None, vid['ind'], vid['soi'], _ev=ev, _drop=EF.DropState(U.SEED, U.OFFSET, False))
    with torch.no_grad():
        tab = run().cpu().numpy()                      # tables
        lib.echr_config_set(b'pair_tables', 0)
        try:
            dense_ng = run().cpu().numpy()             # dense, inference
        finally:
            lib.echr_config_set(b'pair_tables', 1)
        ev2 = EF.event_index_tensors(vid['soi'], vid['ind'], dev)
        del ev2[1].echr_bounds                         # a caller that does not know the bounds
        nob = m.get_event_context(tap, c3d, None, vid['ind'], vid['soi'], _ev=ev2, _drop=EF.DropState(U.SEED, U.OFFSET, False)).cpu().numpy()
    dense = run().detach().cpu().numpy()               # grad mode: dense, activations kept
    assert U.relerr(tab, ref) < 1e-5
    assert U.relerr(tab, dense) < 2e-6 and U.relerr(tab, dense_ng) < 2e-6 and U.relerr(nob, dense) < 2e-6


@pytest.mark.parametrize('case', ['tiny', 'c1', 'c2', 'c2full', 'c3bench', 'vctx', 'er1', 'er2', 'init', 'initc'])
@pytest.mark.parametrize('train_mode', [False, True])
def test_full_path_vs_oracle(case, train_mode):
    """CaptionGenerator forward + criterion + backward against the oracle run on the host with identical dropout masks: EVERY log-prob
    and EVERY gradient element, also at the benchmarked size (c2full / c3bench: N64 x A128 x S20, V1 = 5001)."""
    opt, params, vid = synth.make_case(case)
    pred, loss, grads, _ = U.run_gpu(opt, params, vid, train_mode)
    rpred, rloss, rgrads = U.run_oracle(opt, params, vid, train_mode)
    assert pred.shape == rpred.shape
    assert np.abs(pred - rpred).max() < TOL_LOGP, np.abs(pred - rpred).max()
    assert abs(loss - rloss) < TOL_LOSS * abs(rloss)
    for k, g in rgrads.items():
        if g is None:
            assert grads[k] is None, k
        else:
            assert U.grad_close(k, grads[k], g, TOL_GRAD), (k, U.relerr(grads[k], g))


@pytest.mark.parametrize('case', ['tiny', 'c1', 'c2', 'c2full', 'c3bench', 'vctx', 'er1', 'er2', 'init', 'initc'])
@pytest.mark.parametrize('train_mode', [False, True])
def test_full_path_vs_reference_golden(case, train_mode):
    """Same, against the fixtures the reference itself produced (full tensors for 'tiny', summaries otherwise)."""
    opt, params, vid = synth.make_case(case)
    g = U.gold('case_%s.npz' % case)
    mode = 'train' if train_mode else 'eval'
    pred, loss, grads, _ = U.run_gpu(opt, params, vid, train_mode)
    assert abs(loss - float(g[mode + '|loss'])) < TOL_LOSS * abs(float(g[mode + '|loss']))
    if case == 'tiny':
        assert np.abs(pred - g[mode + '|logp']).max() < TOL_LOGP
        for k, v in grads.items():
            key = mode + '|grad|' + k
            if v is None:
                assert key not in g
            else:
                assert U.grad_close(k, v, g[key], TOL_GRAD), (k, U.relerr(v, g[key]))
        return
    s = SM.summarize_logp(pred)
    assert np.abs(s['slice'] - g[mode + '|logp|slice']).max() < TOL_LOGP
    assert np.abs(s['top1'] - g[mode + '|logp|top1']).max() < TOL_LOGP
    assert np.abs(s['prob_sum'] - 1.0).max() < 1e-4
    safe = g[mode + '|logp|margin'] > 1e-4                # arg-max must agree wherever the reference's own margin is resolvable
    assert np.array_equal(s['argmax'][safe], g[mode + '|logp|argmax'][safe])
    gs = SM.summarize_grads(grads)
    for key, v in gs.items():
        ref = g[mode + '|grad|' + key]
        name = key.split('|')[0]
        if name in U.NOISE_ONLY:          # true gradient is exactly zero: both sides are rounding noise (order-dependent atomics)
            assert np.abs(np.asarray(v)).max() < 1e-6 and np.abs(np.asarray(ref)).max() < 1e-6, (key, v, ref)
            continue
        scale = max(float(g[mode + '|grad|' + name + '|linf']), U.GRAD_FLOOR)
        if key.endswith('|l2') or key.endswith('|linf'):
            assert abs(float(v) - float(ref)) < TOL_GRAD * max(abs(float(ref)), U.GRAD_FLOOR), (key, float(v), float(ref))
        else:
            assert np.abs(v - ref).max() < TOL_GRAD * scale, (key, np.abs(v - ref).max() / scale)


def _check_summaries(g, mode, pred, loss, grads, loss_key='|loss', grad_tag='|grad|'):
    assert abs(loss - float(g[mode + loss_key])) < TOL_LOSS * abs(float(g[mode + loss_key]))
    s = SM.summarize_logp(pred)
    assert np.abs(s['slice'] - g[mode + '|logp|slice']).max() < TOL_LOGP
    assert np.abs(s['top1'] - g[mode + '|logp|top1']).max() < TOL_LOGP
    safe = g[mode + '|logp|margin'] > 1e-4
    assert np.array_equal(s['argmax'][safe], g[mode + '|logp|argmax'][safe])
    for key, v in SM.summarize_grads(grads).items():
        ref = g[mode + grad_tag + key]
        name = key.split('|')[0]
        if name in U.NOISE_ONLY:
            assert np.abs(np.asarray(v)).max() < 1e-6 and np.abs(np.asarray(ref)).max() < 1e-6, (key, v, ref)
            continue
        scale = max(float(g[mode + grad_tag + name + '|linf']), U.GRAD_FLOOR)
        if key.endswith('|l2') or key.endswith('|linf'):
            assert abs(float(v) - float(ref)) < TOL_GRAD * max(abs(float(ref)), U.GRAD_FLOOR), (key, float(v), float(ref))
        else:
            assert np.abs(v - ref).max() < TOL_GRAD * scale, (key, np.abs(v - ref).max() / scale)


@pytest.mark.parametrize('persist', [1, 0])
def test_bench_layout_with_arena_vs_reference_golden(persist):
    """The EXACT configuration bench.py times -- N64 x A128 disjoint events on T_v = 8192 (rows_disjoint = 1: plain-store branch of the
    d P_all pass), train mode, flat parameter/gradient arena (zeroed = 1 accumulate paths), fused clamp+Adam afterwards -- against the
    reference's own outputs on the same inputs (case_c3bench.npz); with the persistent recurrence and with the launch-per-phase one."""
    from echr_amd import _lib
    from echr_amd.misc.utils import LanguageModelCriterion
    lib = _lib.load()
    opt, params, vid = synth.make_case('c3bench')
    assert vid['T_v'] == 8192
    g = U.gold('case_c3bench.npz')
    try:
        assert lib.echr_config_set(b'persist', persist) == 0
        m = U.build_gpu_model(opt, params, True)
        arena = m.build_arena()
        dev = torch.device('cuda')
        tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
        labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
        pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
        loss = LanguageModelCriterion()(pred, labels[:, 1:].to(dev), masks[:, 1:].to(dev))
        loss.backward()
        assert arena.grads_in_arena()
        grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}
        _check_summaries(g, 'train', pred.detach().cpu().numpy(), float(loss), grads)
    finally:
        lib.echr_config_set(b'persist', 1)


@pytest.mark.parametrize('train_mode', [False, True])
def test_c5_sst_plus_decoder_vs_reference_golden(train_mode):
    """BASELINE config 5 as ONE unit: native SST over a 256-segment video -> tap_feats -> caption path on 64 proposals of 4..256
    segments -> lambda1 * tap_loss + lambda2 * cg_loss -> gradients into both models (train.py:322-329), against the reference's
    own summaries (case_c5.npz: reference SST in eval mode, caption model eval / train with the injected dropout masks)."""
    from echr_amd import models as EM
    from echr_amd.misc.utils import LanguageModelCriterion, TAPModelCriterion
    opt, params, sst_params, vid = synth.make_c5()
    g = U.gold('case_c5.npz')
    mode = 'train' if train_mode else 'eval'
    m = U.build_gpu_model(opt, params, train_mode)
    dev = torch.device('cuda')
    tapm = EM.setup_tap(opt)
    tapm.load_state_dict({k: torch.from_numpy(v) for k, v in sst_params.items()})
    tapm = tapm.to(dev)
    tapm.eval()                                          # the fixture's SST runs without inter-layer dropout
    c3d, lda = torch.from_numpy(vid['c3d']).to(dev), torch.from_numpy(vid['lda']).to(dev)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    tap_feats, props = tapm(c3d)
    pred = m(tap_feats, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    tap_loss = TAPModelCriterion()(props, torch.from_numpy(vid['tap_masks']), torch.from_numpy(vid['tap_labels']), torch.from_numpy(vid['w1']))
    cg_loss = LanguageModelCriterion()(pred, labels[:, 1:].to(dev), masks[:, 1:].to(dev))
    (opt.lambda1 * tap_loss + opt.lambda2 * cg_loss).backward()
    assert abs(float(tap_loss) - float(g[mode + '|tap_loss'])) < TOL_LOSS * abs(float(g[mode + '|tap_loss']))
    grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}
    _check_summaries(g, mode, pred.detach().cpu().numpy(), float(cg_loss), grads, loss_key='|cg_loss')
    assert np.abs(tap_feats.detach().cpu().numpy()[::8, ::16] - g['tap_feats|slice']).max() < 1e-5
    assert np.abs(props.detach().cpu().numpy()[::8, ::16] - g['props|slice']).max() < 1e-5
    sg = SM.summarize_grads({k: p.grad.detach().cpu().numpy() for k, p in tapm.named_parameters()})
    for key, v in sg.items():
        ref = g[mode + '|sstgrad|' + key]
        scale = max(float(g[mode + '|sstgrad|' + key.split('|')[0] + '|linf']), U.GRAD_FLOOR)
        if key.endswith('|l2') or key.endswith('|linf'):
            assert abs(float(v) - float(ref)) < TOL_GRAD * max(abs(float(ref)), U.GRAD_FLOOR), (key, float(v), float(ref))
        else:
            assert np.abs(v - ref).max() < TOL_GRAD * scale, (key, np.abs(v - ref).max() / scale)


@pytest.mark.parametrize('train_mode', [False, True])
def test_c5_full_path_vs_oracle(train_mode):
    """BASELINE config 5 element by element: native SST over the 256-segment video -> tap_feats -> caption path on 64 proposals of 4..256
    segments (persistent recurrences, BIG instantiations: second slot set) -> lambda1 * tap + lambda2 * cg -> backward into BOTH models,
    EVERY log-prob and EVERY gradient element of both models against the oracle on the same inputs (the oracle itself is pinned to the
    reference on this case by tools/make_golden.py do_c5 / case_c5.npz)."""
    from echr_amd import models as EM
    from echr_amd.misc.utils import LanguageModelCriterion, TAPModelCriterion
    from oracle import echr_ref_cpu as O
    opt, params, sst_params, vid = synth.make_c5()
    m = U.build_gpu_model(opt, params, train_mode)
    dev = torch.device('cuda')
    tapm = EM.setup_tap(opt)
    tapm.load_state_dict({k: torch.from_numpy(v) for k, v in sst_params.items()})
    tapm = tapm.to(dev)
    tapm.eval()
    c3d, lda = torch.from_numpy(vid['c3d']).to(dev), torch.from_numpy(vid['lda']).to(dev)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    tl, tm, tw = (torch.from_numpy(vid[k]) for k in ('tap_labels', 'tap_masks', 'w1'))
    tap_feats, props = tapm(c3d)
    pred = m(tap_feats, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    tap_loss = TAPModelCriterion()(props, tm, tl, tw)
    cg_loss = LanguageModelCriterion()(pred, labels[:, 1:].to(dev), masks[:, 1:].to(dev))
    (opt.lambda1 * tap_loss + opt.lambda2 * cg_loss).backward()
    torch.cuda.synchronize()
    # the oracle on the same joint path
    P = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in params.items()}
    SP = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in sst_params.items()}
    otap, oprops = O.sst_forward(SP, torch.from_numpy(vid['c3d']))
    opred = O.caption_forward(P, otap, torch.from_numpy(vid['c3d']), torch.from_numpy(vid['lda']), labels, vid['ind'], vid['soi'], 'train',
                              U.oracle_drop(opt) if train_mode else None, opt.n_head)
    otl, ocl = O.tap_criterion(oprops, tm, tl, tw), O.lm_criterion(opred, labels[:, 1:], masks[:, 1:])
    (opt.lambda1 * otl + opt.lambda2 * ocl).backward()
    assert np.abs(tap_feats.detach().cpu().numpy() - otap.detach().numpy()).max() < 1e-5
    assert np.abs(props.detach().cpu().numpy() - oprops.detach().numpy()).max() < 1e-5
    assert pred.shape == opred.shape
    assert np.abs(pred.detach().cpu().numpy() - opred.detach().numpy()).max() < TOL_LOGP
    assert abs(float(cg_loss) - float(ocl)) < TOL_LOSS * abs(float(ocl)) and abs(float(tap_loss) - float(otl)) < TOL_LOSS * abs(float(otl))
    for k, p in m.named_parameters():
        if P[k].grad is None:
            assert p.grad is None, k
        else:
            assert U.grad_close(k, p.grad.cpu().numpy(), P[k].grad.numpy(), TOL_GRAD), (k, U.relerr(p.grad.cpu().numpy(), P[k].grad.numpy()))
    for k, p in tapm.named_parameters():
        assert U.grad_close(k, p.grad.cpu().numpy(), SP[k].grad.numpy(), TOL_GRAD), (k, U.relerr(p.grad.cpu().numpy(), SP[k].grad.numpy()))


@pytest.mark.parametrize('N,A,min_len', [(64, 130, 4), (33, 200, 120), (64, 258, 100), (20, 256, 1)])
def test_long_events_vs_oracle(N, A, min_len):
    """Events of 130..258 segments -- the persistent recurrences' second slot set (`BIG` instantiations: CaptionGenerator.py:142-151 pads to
    the longest event; config 5's 256-segment proposals, long ground-truth events) -- directly against the oracle at the full-path gates:
    every log-prob and every gradient element, train mode (dropout), ECHR widths."""
    opt = synth.default_opt(vocab_size=300, seq_length=5)
    params = synth.make_params(opt, seed=5)
    vid = synth.make_video(N, A, 7, 301, seed=177 + N + A, min_len=min_len)
    pred, loss, grads, _ = U.run_gpu(opt, params, vid, True)
    rpred, rloss, rgrads = U.run_oracle(opt, params, vid, True)
    assert pred.shape == rpred.shape
    assert np.abs(pred - rpred).max() < TOL_LOGP, np.abs(pred - rpred).max()
    assert abs(loss - rloss) < TOL_LOSS * abs(rloss)
    for k, g in rgrads.items():
        if g is None:
            assert grads[k] is None, k
        else:
            assert U.grad_close(k, grads[k], g, TOL_GRAD), (k, U.relerr(grads[k], g))


@pytest.mark.parametrize('case', ['tiny', 'c1', 'c2', 'c2full', 'c3bench', 'vctx', 'er1', 'er2', 'init', 'initc'])
def test_greedy_sample_bit_exact(case):
    """mode='eval': the index output must equal the reference's greedy sequence exactly; log-probs within 1e-4."""
    opt, params, vid = synth.make_case(case)
    g = U.gold('case_%s.npz' % case)
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    with torch.no_grad():
        seq, lp = m(torch.from_numpy(vid['tap']).to(dev), torch.from_numpy(vid['c3d']).to(dev), torch.from_numpy(vid['lda']).to(dev),
                    [], vid['ind'], vid['soi'], mode='eval')
    assert seq.dtype == torch.int64
    assert tuple(seq.shape) == tuple(g['sample|seq'].shape)
    assert np.array_equal(seq.cpu().numpy(), g['sample|seq'])
    assert np.abs(lp.cpu().numpy() - g['sample|logp']).max() < TOL_LOGP


@pytest.mark.parametrize('persist_sample', [1, 0])
@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_greedy_sample_mixed_finish_vs_reference(name, persist_sample):
    """Greedy decoding where events emit <eos> at DIFFERENT steps (OldModel_NEW.py:171-183: per-row `unfinished`, emitted token masked, the
    network keeps consuming the raw arg-max, raw max log-prob appended for finished rows too, break when nobody is unfinished) against the
    REFERENCE's own seq / seqLogprobs (tests/golden/case_eosmix.npz).  'a': 64 events, 11 distinct finishing steps, 50 never finish;
    'b': 150 events = three 64-event groups of the persistent decoder, the first group is done after step 8 while the others run to the end;
    'c': 48 events that all finish -- the batch stops after 4 columns.  Both decoder forms."""
    from echr_amd import _lib
    lib = _lib.load()
    opt, params, vid = synth.make_eosmix(name)
    g = U.gold('case_eosmix.npz')
    soi, ind = g[name + '|soi'], g[name + '|ind']
    ref_seq, ref_lp = g[name + '|seq'], g[name + '|logp']
    assert (ref_seq == 0).any() and len(set(int((r == 0).argmax()) if (r == 0).any() else -1 for r in ref_seq)) >= 3
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    try:
        lib.echr_config_set(b'persist_sample', persist_sample)
        with torch.no_grad():
            seq, lp = m(tap, c3d, lda, [], ind, soi, mode='eval')
    finally:
        lib.echr_config_set(b'persist_sample', 1)
    assert seq.dtype == torch.int64 and tuple(seq.shape) == tuple(ref_seq.shape)          # trimmed width included
    assert np.array_equal(seq.cpu().numpy(), ref_seq)                                     # zeros of finished rows included
    assert np.abs(lp.cpu().numpy() - ref_lp).max() < TOL_LOGP                             # finished rows' raw log-probs included


@pytest.mark.parametrize('case', ['c2', 'c2full', 'c3bench'])
def test_persistent_sampler_equals_launch_per_step_sampler(case):
    """Greedy decoding as ONE persistent launch (logits role + arg-max keys inside the recurrence kernels) against the launch-per-step
    form: same sequences, log-probs to rounding."""
    from echr_amd import _lib
    lib = _lib.load()
    opt, params, vid = synth.make_case(case)
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    outs = []
    try:
        for flag in (1, 0):
            lib.echr_config_set(b'persist_sample', flag)
            with torch.no_grad():
                seq, lp = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
            outs.append((seq.cpu().numpy(), lp.cpu().numpy()))
    finally:
        lib.echr_config_set(b'persist_sample', 1)
    assert outs[0][0].shape == outs[1][0].shape and outs[0][0].shape[1] > 1
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.abs(outs[0][1] - outs[1][1]).max() < TOL_LOGP


@pytest.mark.parametrize('N,A,V1,min_len', [(1, 7, 301, 7), (5, 40, 301, 4), (33, 129, 1201, 1), (12, 200, 301, 60), (64, 258, 5001, 100), (150, 130, 301, 4), (7, 60, 9001, 10)])
def test_persistent_sampler_edge_shapes_vs_launch_per_step(N, A, V1, min_len):
    """The persistent greedy decoder at the edges of its shapes: one event, a second half machine with a single row, events past 129 segments
    (second slot set, BIG instantiation), the largest A, a vocabulary that leaves most logits workgroups without a column, more than 64 events
    (three launches, the last one partly filled), a vocabulary of two column chunks -- same sequences as the launch-per-step form, log-probs to rounding; and against the oracle for
    the smallest case."""
    from echr_amd import _lib
    lib = _lib.load()
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=7)
    params = synth.make_params(opt, seed=3)
    vid = synth.make_video(N, A, 9, V1, seed=31 + N + A, min_len=min_len, T_v=max(A + 40, 300))
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    outs = []
    try:
        for flag in (1, 0):
            lib.echr_config_set(b'persist_sample', flag)
            with torch.no_grad():
                seq, lp = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
            outs.append((seq.cpu().numpy(), lp.cpu().numpy()))
    finally:
        lib.echr_config_set(b'persist_sample', 1)
    assert outs[0][0].shape == outs[1][0].shape == (N, outs[0][0].shape[1])
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.isfinite(outs[0][1]).all() and np.abs(outs[0][1] - outs[1][1]).max() < TOL_LOGP
    if N <= 5:
        from oracle import echr_ref_cpu as O
        P = {k: torch.from_numpy(v) for k, v in params.items()}
        with torch.no_grad():
            seq_o, lp_o = O.caption_forward(P, torch.from_numpy(vid['tap']), torch.from_numpy(vid['c3d']), torch.from_numpy(vid['lda']), None, vid['ind'],
                                            vid['soi'], mode='eval', seq_length=opt.CG_seq_length)
        assert np.array_equal(outs[0][0], seq_o.numpy())
        assert np.abs(outs[0][1] - lp_o.numpy()).max() < TOL_LOGP


def test_many_event_decode_batched_form_vs_oracle_and_persistent():
    """Greedy decoding of MORE than `persist_sample_max` (default 512; 256 here) events -- evaluation over hundreds of proposals -- takes one batched launch chain
    per step whose recurrent, context and logits products are h2 GEMMs over the N rows (fixed-order k loops: bitwise reproducible).  Same `seq`
    as the oracle and as the persistent form (one launch per 64 events), log-probs to rounding."""
    from echr_amd import _lib
    from oracle import echr_ref_cpu as O
    lib = _lib.load()
    opt = synth.default_opt(vocab_size=1200, seq_length=9)
    params = synth.make_params(opt, seed=4)
    N = 300
    vid = synth.make_video(N, 20, 11, 1201, seed=91, T_v=90)
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))

    def decode(mx):
        try:
            lib.echr_config_set(b'persist_sample_max', mx)
            with torch.no_grad():
                seq, lp = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
            return seq.cpu().numpy(), lp.cpu().numpy()
        finally:
            lib.echr_config_set(b'persist_sample_max', 512)

    sb, lb = decode(256)          # batched form (300 > 256)
    sb2, lb2 = decode(256)
    sp, lpp = decode(0)           # persistent form
    assert sb.shape == (N, sb.shape[1]) and sb.shape[1] > 1
    assert np.array_equal(sb, sb2) and np.abs(lb - lb2).max() < 2e-6          # (the event encoder's split-K sums in front of the decoder are not bitwise repeatable)
    assert np.array_equal(sb, sp) and np.abs(lb - lpp).max() < TOL_LOGP
    P = {k: torch.from_numpy(v) for k, v in params.items()}
    with torch.no_grad():
        so, lo = O.caption_forward(P, torch.from_numpy(vid['tap']), torch.from_numpy(vid['c3d']), torch.from_numpy(vid['lda']), None, vid['ind'], vid['soi'],
                                   mode='eval', seq_length=opt.CG_seq_length)
    assert np.array_equal(sb, so.numpy()) and np.abs(lb - lo.numpy()).max() < TOL_LOGP


@pytest.mark.parametrize('N', [3, 64, 100])
def test_persistent_sampler_stops_when_every_event_has_finished(N):
    """OldModel.sample breaks out of its loop once no event is unfinished (models/OldModel_NEW.py:171-180); the persistent decoder then stops
    its launch (its workgroups leave through their wait loops).  The synthetic initialisation never ends a caption between the first and the
    last step (checked with the oracle: the <eos> margin is smallest at step 1), so the diagnostic `persist_sample_force_eos` = k lets <eos>
    win from step k - 1 on: the decode must return exactly the first k - 1 columns of the free-running decode, report the early stop, raise
    no error, and leave the next decode undisturbed.  A model whose <eos> bias ends every caption at once gives ([], []) on both forms."""
    from echr_amd import _lib
    from echr_amd import functional as EF
    from echr_amd.models.OldModel_NEW import ClipView
    lib = _lib.load()
    opt, params, _ = synth.make_case('c2')
    V1 = params['lm_model.logit.bias'].shape[0]
    vid = synth.make_video(N, 40, 21, V1, seed=5, T_v=120)
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    with torch.no_grad():
        ev = EF.event_index_tensors(vid['soi'], vid['ind'], dev)
        event = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'], _ev=ev, _drop=m.lm_model.next_drop_state())

        def decode():
            dbg = {}
            out = EF.greedy_sample(lda, event, c3d, ev[0], ev[1], ev[3], m.lm_model.seq_length, m.lm_model.native_params(), debug=dbg)
            return out, dbg
        (free_seq, free_lp), dbg = decode()
        assert free_seq.shape == (N, opt.CG_seq_length) and dbg['stopped_early'] == 0
        for k in (2, 7):
            lib.echr_config_set(b'persist_sample_force_eos', k)
            try:
                (seq, lp), dbg = decode()
            finally:
                lib.echr_config_set(b'persist_sample_force_eos', 0)
            assert lib.echr_check_async() == 0
            assert dbg['stopped_early'] == (1 if N <= 64 else 0)      # several groups: every group runs every step, the host trims (OldModel_NEW.py:179-183)
            assert tuple(seq.shape) == (N, k - 1)
            assert torch.equal(seq, free_seq[:, :k - 1]) and torch.equal(lp, free_lp[:, :k - 1])
        (again, again_lp), dbg = decode()
        assert torch.equal(again, free_seq) and torch.equal(again_lp, free_lp) and dbg['stopped_early'] == 0
        # every caption ends at its first token: nothing is generated, on both forms
        m.lm_model.logit.bias.data[0] += 500.0
        for flag in (1, 0):
            lib.echr_config_set(b'persist_sample', flag)
            try:
                out = m.lm_model.sample(lda, event, ClipView(c3d, ev[0], ev[1], ev[3], False), None)
            finally:
                lib.echr_config_set(b'persist_sample', 1)
            assert len(out[0]) == 0 and len(out[1]) == 0


def test_persistent_sampler_table_cache_follows_parameter_updates():
    """The persistent decoder caches its parameter-only operands (token-side gate tables, logit image) on the model.  A second decode must
    reuse them (bitwise the same output); an in-place parameter update (torch version counter) and a library optimiser step (raw-pointer
    write: functional.PARAM_EPOCH) must each invalidate them -- checked against the launch-per-step form on the updated model."""
    from echr_amd import _lib
    from echr_amd import functional as EF
    from echr_amd.optim import ClampAdam
    lib = _lib.load()
    opt, params, vid = synth.make_case('c2')
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))

    def decode(flag=1):
        lib.echr_config_set(b'persist_sample', flag)
        try:
            with torch.no_grad():
                seq, lp = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
            return seq.cpu().numpy(), lp.cpu().numpy()
        finally:
            lib.echr_config_set(b'persist_sample', 1)

    s1, l1 = decode()
    cache = m.lm_model._sample_tables
    assert cache.get('key') is not None and cache['tables'].numel() > 0
    key1 = cache['key']
    s2, l2 = decode()
    assert cache['key'] == key1 and np.array_equal(s1, s2) and np.abs(l1 - l2).max() < 2e-6      # (the event encoder's split-K sums are not bitwise repeatable)
    with torch.no_grad():
        m.lm_model.embed.weight.mul_(-1.0)            # in-place update through torch: version counter
    s3, l3 = decode()
    assert cache['key'] != key1
    r3, rl3 = decode(0)
    assert np.array_equal(s3, r3) and np.abs(l3 - rl3).max() < TOL_LOGP
    assert not np.array_equal(s3, s1)
    key3 = cache['key']
    optim = ClampAdam(m.parameters(), lr=2e-3)        # raw-pointer update by the library's fused kernel
    for p_ in m.parameters():
        p_.grad = torch.ones_like(p_)
    optim.step()
    s4, l4 = decode()
    assert cache['key'] != key3
    r4, rl4 = decode(0)
    assert np.array_equal(s4, r4) and np.abs(l4 - rl4).max() < TOL_LOGP * max(1.0, float(np.abs(rl4).max()))
    assert not np.array_equal(s4, s3)


@pytest.mark.parametrize('V1', [9001, 13001])
def test_greedy_sample_large_vocabulary_vs_oracle(V1):
    """Vocabularies beyond the benchmark's 5001 (ActivityNet Captions has ~10 k words): the persistent decoder's second / third column chunk per
    logits workgroup (and, with persist_sample = 0, the arg-max kernel's long-row instantiations) must decode the oracle's sequence."""
    from oracle import echr_ref_cpu as O
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=6)
    params = synth.make_params(opt, 11)
    vid = synth.make_video(5, 20, 8, V1, seed=3, T_v=40)
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    with torch.no_grad():
        seq1, lp1 = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
        seq2, lp2 = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
    P = {k: torch.from_numpy(v) for k, v in params.items()}
    with torch.no_grad():
        seq_o, lp_o = O.caption_forward(P, torch.from_numpy(vid['tap']), torch.from_numpy(vid['c3d']), torch.from_numpy(vid['lda']), None, vid['ind'],
                                        vid['soi'], mode='eval', seq_length=opt.CG_seq_length)
    # (bitwise repeatability on IDENTICAL decoder inputs is test_greedy_sampler_is_bitwise_reproducible's; here the event encoder runs again,
    # and its split-K sums move the event context by an ulp)
    assert torch.equal(seq1, seq2) and float((lp1 - lp2).abs().max()) < 2e-6
    assert np.array_equal(seq1.cpu().numpy(), seq_o.numpy())
    assert np.abs(lp1.cpu().numpy() - lp_o.numpy()).max() < TOL_LOGP


@pytest.mark.parametrize('persistent', [1, 0])
def test_greedy_sampler_is_bitwise_reproducible(persistent):
    """`seq` is an index output: two decodes of the same inputs must agree bit for bit -- sequence, log-probs AND (launch-per-step form) the
    raw logits of the last step: no fp32-atomic split-K anywhere on the sampler path, the persistent form folds its arg-max through an
    order-independent 64-bit atomic max and adds the context partials in slot order; OldModel_NEW.py:158 takes the lowest index on ties."""
    from echr_amd import functional as EF
    from echr_amd import _lib
    lib = _lib.load()
    lib.echr_config_set(b'persist_sample', persistent)
    try:
        _reproducible(EF, persistent)
    finally:
        lib.echr_config_set(b'persist_sample', 1)


def _reproducible(EF, persistent):
    opt, params, vid = synth.make_case('c2full')
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    runs = []
    with torch.no_grad():
        ev = EF.event_index_tensors(vid['soi'], vid['ind'], dev)
        event = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'], _ev=ev, _drop=m.lm_model.next_drop_state())
        for rep in range(3):
            if rep == 1:        # disturb the allocator / caches between the runs
                junk = torch.randn(1 << 22, device=dev).sum().item()
                assert junk == junk
            dbg = {}
            EF.greedy_sample(lda, event, c3d, ev[0], ev[1], ev[3], m.lm_model.seq_length, m.lm_model.native_params(), debug=dbg)
            runs.append(dbg)
    for r in runs[1:]:
        assert torch.equal(r['seq_full'], runs[0]['seq_full'])
        assert torch.equal(r['logp_full'], runs[0]['logp_full'])
        if not persistent:
            assert torch.equal(r['last_logits'], runs[0]['last_logits'])
    if not persistent:
        assert torch.isfinite(runs[0]['last_logits']).all()
    assert torch.isfinite(runs[0]['logp_full']).all()


def test_sampler_at_eval_size_is_per_event_and_matches_small_batch():
    """Eval-size property test (1000 proposals): the decoder is independent per event given its contexts, so a
    batch of 1000 events made of 125 copies of 8 distinct events must decode every copy to the SAME token sequence as the 8-event batch, with log-probs
    equal to rounding (5e-6)."""
    from echr_amd.models.OldModel_NEW import ClipView
    opt, params, vid = synth.make_case('c1')
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    rs = np.random.RandomState(5)
    base, reps, T_v, D = 8, 125, 160, opt.video_dim
    c3d = torch.from_numpy(rs.standard_normal((T_v, D)).astype(np.float32)).to(dev)
    start = rs.randint(0, T_v - 128, size=base)
    length = rs.randint(1, 129, size=base)
    video = torch.from_numpy(rs.standard_normal(opt.video_context_dim).astype(np.float32)).to(dev)
    event = torch.from_numpy(rs.standard_normal((base, opt.event_context_dim)).astype(np.float32)).to(dev)

    def decode(n_rep):
        st = torch.from_numpy(np.tile(start, n_rep).astype(np.int32)).to(dev)
        ln = torch.from_numpy(np.tile(length, n_rep).astype(np.int32)).to(dev)
        cv = ClipView(c3d, st, ln, int(length.max()), False)
        with torch.no_grad():
            seq, lp = m.lm_model.sample(video, event.repeat(n_rep, 1), cv, None)
        return seq.cpu().numpy(), lp.cpu().numpy()

    s1, l1 = decode(1)
    sN, lN = decode(reps)
    assert sN.shape[0] == base * reps
    assert np.array_equal(sN, np.tile(s1, (reps, 1)))
    assert np.abs(lN - np.tile(l1, (reps, 1))).max() < 5e-6          # the per-step logit GEMM picks a different split-K at M = 8 and M = 1000
    assert (s1 != 0).any()


def test_clamp_adam_matches_torch_adam():
    from echr_amd import functional as EF
    g = U.gold('adam.npz')
    p = torch.from_numpy(g['p0'].copy()).cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for i in range(4):
        EF.clamp_adam_(p, torch.from_numpy(g['g%d' % i]).cuda(), m, v, i + 1, 5e-5, 0.9, 0.999, 1e-8, 100.0)
        assert np.abs(p.cpu().numpy() - g['p%d' % (i + 1)]).max() < 2e-7, i
    assert U.relerr(m.cpu().numpy(), g['exp_avg']) < 1e-6
    assert U.relerr(v.cpu().numpy(), g['exp_avg_sq']) < 1e-6


def test_optimizer_step_on_model():
    """clip_gradient + ClampAdam.step() == reference's clip_gradient + torch.optim.Adam on the same gradients."""
    from echr_amd.misc.utils import clip_gradient
    from echr_amd.optim import ClampAdam
    opt, params, vid = synth.make_case('tiny')
    _, _, grads, m = U.run_gpu(opt, params, vid, False)
    ref_p = {k: torch.nn.Parameter(torch.from_numpy(v.copy())) for k, v in params.items()}
    for k, p in ref_p.items():
        p.grad = torch.from_numpy(grads[k].copy()) if grads[k] is not None else None
    ropt = torch.optim.Adam(list(ref_p.values()), lr=1e-3)
    for p in ref_p.values():
        if p.grad is not None:
            p.grad.clamp_(-0.01, 0.01)
    ropt.step()
    o = ClampAdam(m.parameters(), lr=1e-3)
    clip_gradient(o, 0.01)
    o.step()
    for k, p in m.named_parameters():
        assert np.abs(p.detach().cpu().numpy() - ref_p[k].detach().numpy()).max() < 1e-6, k


def test_padded_clip_tensor_api():
    """lm_model accepts the reference-style padded clip tensor + mask (external callers of lm_model.forward)."""
    from echr_amd import functional as EF
    opt, params, vid = synth.make_case('tiny')
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels = torch.from_numpy(vid['labels'])
    a = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    clip, mask = m.get_clip_context(tap, c3d, lda, vid['ind'], vid['soi'])
    from oracle import echr_ref_cpu as O
    rc, rm = O.clip_context(torch.from_numpy(vid['c3d']), vid['soi'])
    assert torch.equal(clip.cpu(), rc) and torch.equal(mask.cpu(), rm)
    ev = EF.event_index_tensors(vid['soi'], vid['ind'], dev)
    event = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'], _ev=ev, _drop=EF.DropState())
    b = m.lm_model(lda, event, clip, mask, labels)
    assert float((a - b).abs().max()) < 1e-5


def test_cpu_tensors_fail_loudly():
    import echr_amd
    from echr_amd._lib import EchrHipError
    opt, params, vid = synth.make_case('tiny')
    m = echr_amd.CaptionGenerator(opt)
    with pytest.raises(EchrHipError):
        m(torch.from_numpy(vid['tap']), torch.from_numpy(vid['c3d']), torch.from_numpy(vid['lda']), torch.from_numpy(vid['labels']),
          vid['ind'], vid['soi'], mode='train')


def test_abandoned_prepare_is_cancelled_and_next_forward_is_unaffected():
    """The decoder precompute runs on the library's second stream; when the event encoder fails in between (here: a proposal tensor of
    the wrong width), forward() must cancel it (echr_decoder_fwd_prepare_cancel) and the next, valid call must give the usual result."""
    from echr_amd import functional as EF
    opt, params, vid = synth.make_case('c1')
    m = U.build_gpu_model(opt, params, True)
    m.set_dropout_state(5)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels = torch.from_numpy(vid['labels'])
    ref = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train').detach().clone()
    m.set_dropout_state(5)
    with pytest.raises(Exception):
        m(tap[:, :-3].contiguous(), c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    EF.decoder_prepare_cancel()          # a second cancel is a no-op
    m.set_dropout_state(5)
    out = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    assert float((out.detach() - ref).abs().max()) < 1e-5          # same dropout stream; the split-K sums are not bitwise repeatable


def test_staged_decoder_backward_equals_single_call():
    """echr_dec_grads.phase: late-fusion stage (1), reverse recurrence + LSTM-layer gradients (3), the rest (4) on the same scratch
    must equal the one-call backward (0); the data-parallel early reducer hooks in after stages 1 and 3 and must see the FINAL
    gradients of logit.* and of the twelve core.layer* tensors (it starts summing them over ranks right there)."""
    from echr_amd.misc.utils import LanguageModelCriterion
    opt, params, vid = synth.make_case('c1')
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels = torch.from_numpy(vid['labels'])
    tgt, msk = labels[:, 1:].to(dev), torch.from_numpy(vid['masks'])[:, 1:].to(dev)
    grads, seen = [], []
    for hooked in (False, True):
        m = U.build_gpu_model(opt, params, True)
        arena = m.build_arena()
        names = {id(p): k for k, p in m.named_parameters()}
        if hooked:
            def hook(ps, arena=arena, names=names):
                torch.cuda.synchronize()
                seen.append({names[id(p_)]: arena.grad_view(arena.slot(p_)).clone().cpu().numpy() for p_ in ps})
            arena.early_grad_hook = hook
        m.set_dropout_state(U.SEED, U.OFFSET)
        LanguageModelCriterion()(m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train'), tgt, msk).backward()
        grads.append({k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()})
    assert len(seen) == 2
    assert sorted(seen[0]) == ['lm_model.logit.bias', 'lm_model.logit.weight']
    assert len(seen[1]) == 12 and all(k.startswith('lm_model.core.layer') for k in seen[1])
    for k in grads[0]:
        if grads[0][k] is not None:
            assert U.grad_close(k, grads[1][k], grads[0][k], 1e-5), k
    for call in seen:                          # what the hook saw between the stages is what ends up in .grad
        for k, v in call.items():
            assert np.array_equal(v, grads[1][k]), k


@pytest.mark.parametrize('case', ['tiny', 'c1'])
def test_flat_arena_path_matches_per_tensor_path(case):
    """build_arena(): gradients land in the flat buffer (adopted as .grad without copies) and equal the per-tensor path's;
    the single-launch fused optimiser step equals the per-tensor one on identical gradients; a second backward without
    zero_grad accumulates instead of aliasing."""
    from echr_amd.misc.utils import LanguageModelCriterion, clip_gradient
    from echr_amd.optim import ClampAdam
    opt, params, vid = synth.make_case(case)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels = torch.from_numpy(vid['labels'])
    tgt, msk = labels[:, 1:].to(dev), torch.from_numpy(vid['masks'])[:, 1:].to(dev)

    def backward(m, off):
        m.set_dropout_state(U.SEED, off)
        LanguageModelCriterion()(m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train'), tgt, msk).backward()

    ma, mb = U.build_gpu_model(opt, params, True), U.build_gpu_model(opt, params, True)
    arena = ma.build_arena()
    for k, v in ma.state_dict().items():
        assert torch.equal(v.cpu(), torch.from_numpy(params[k])), k          # packing kept every value
    oa = ClampAdam(ma.parameters(), lr=1e-3, arena=arena)
    ob = ClampAdam(mb.parameters(), lr=1e-3)
    for it in range(2):
        oa.zero_grad(); ob.zero_grad()
        backward(ma, U.OFFSET + it); backward(mb, U.OFFSET + it)
        assert arena.grads_in_arena()
        for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
            assert (pa.grad is None) == (pb.grad is None), k
            if pa.grad is not None:
                assert U.grad_close(k, pa.grad.cpu().numpy(), pb.grad.cpu().numpy(), 1e-4), k
                pb.grad.copy_(pa.grad)                                       # identical inputs for the optimiser comparison
        clip_gradient(oa, 0.05); clip_gradient(ob, 0.05)
        oa.step(); ob.step()
        for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
            assert float((pa.detach() - pb.detach()).abs().max()) < 1e-7, k
    assert oa._flat is not None and oa._flat['step'] == 2 and ob._flat is None and ob.state[mb.lm_model.embed.weight]['step'] == 2
    # gradient accumulation: two backward passes without zero_grad == twice the single gradient
    oa.zero_grad()
    backward(ma, U.OFFSET + 9)
    g1 = {k: p.grad.detach().clone() for k, p in ma.named_parameters() if p.grad is not None}
    backward(ma, U.OFFSET + 9)
    for k, p in ma.named_parameters():
        if p.grad is not None:
            assert U.grad_close(k, p.grad.cpu().numpy(), 2 * g1[k].cpu().numpy(), 1e-4), k


def _fused_train_step_vs_autograd_path(case, ltol, fixed):
    """echr_train_step (one library call per iteration: zero_grad, forward, criterion, backward, clip_gradient, Adam -- train.py:281-317)
    against the autograd path on a twin model: same losses, same parameters and Adam moments after three iterations (train mode, same
    dropout stream), same gradients with step=False, same validation loss with forward_only; then both paths mixed on one model."""
    from echr_amd.fused import FusedTrainStep
    from echr_amd.misc.utils import LanguageModelCriterion, clip_gradient
    from echr_amd.optim import ClampAdam
    opt, params, vid = synth.make_case(case)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    tgt, msk = labels[:, 1:].to(dev), masks[:, 1:].to(dev)
    crit = LanguageModelCriterion()

    def make():
        m = U.build_gpu_model(opt, params, True)
        o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
        return m, o

    def autograd_iteration(m, o, step=True, mask=None):
        o.zero_grad()
        loss = crit(m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train'), tgt, msk if mask is None else mask)
        loss.backward()
        clip_gradient(o, 0.05)
        if step:
            o.step()
        return float(loss)

    ma, oa = make()
    mb, ob = make()
    fb = FusedTrainStep(mb, ob, grad_clip=0.05)
    lr = 1e-3
    # ONE step from identical states.  Split-K / scatter sums use fp32 atomics, so two evaluations of the same gradient differ in the last
    # bits (~1e-7 of the tensor's max-norm) whichever path runs, and Adam's first update is lr * g / (|g| + eps): insensitive to that noise
    # where |g| is resolvable, a coin flip of +-lr where the gradient itself is rounding noise
    la = autograd_iteration(ma, oa)
    lb = float(fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:]))      # host targets / masks: uploaded inside
    assert abs(la - lb) < 1e-6 * abs(la), (la, lb)
    assert 0 < fb.last_active_rows < labels.shape[0] * (labels.shape[1] - 1)          # host masks: the late-fusion stage ran on the active rows only
    assert ob._flat['step'] == 1 and oa._flat['step'] == 1
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        dp = (pa.detach() - pb.detach()).abs()
        assert float(dp.max()) <= 2.01 * lr, k
        if pa.grad is not None and k not in U.NOISE_ONLY:          # (alpha_net.bias: the true gradient is exactly zero, both sides hold noise)
            g = pa.grad.abs()
            solid = g > 1e-4 * g.max()
            if bool(solid.any()):
                assert float(dp[solid].max()) < 0.02 * lr, (k, float(dp[solid].max()))
    # the trajectories stay together (noise is amplified by Adam from step to step, so the gate widens)
    for it in range(3):
        la = autograd_iteration(ma, oa)
        lb = float(fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], tgt, msk))
        assert abs(la - lb) < 1e-3 * abs(la), (it, la, lb)
    assert ob._flat['step'] == 4 and oa._flat['step'] == 4
    # from here on the twins are re-synchronised before every comparison
    def sync():
        with torch.no_grad():
            mb._echr_arena.flat_p.copy_(ma._echr_arena.flat_p)
            ob._flat['m'].copy_(oa._flat['m']); ob._flat['v'].copy_(oa._flat['v'])
        ma.set_dropout_state(U.SEED, 40); mb.set_dropout_state(U.SEED, 40)
    sync()
    # gradients only (data-parallel protocol: reduce, then clip + step by the caller)
    autograd_iteration(ma, oa, step=False)
    lb = fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], tgt, msk, step=False)
    assert fb.last_active_rows == 0                                                 # device tensors: all rows
    assert mb._echr_arena.grads_in_arena()
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert (pa.grad is None) == (pb.grad is None), k
        if pa.grad is not None:
            assert U.grad_close(k, pb.grad.cpu().numpy(), pa.grad.cpu().numpy(), 2e-5), (k, U.relerr(pb.grad.cpu().numpy(), pa.grad.cpu().numpy()))
    clip_gradient(ob, 0.05)
    ob.step()
    oa.step()
    sync()
    # the same gradient comparison with the criterion inputs on the host (active rows only)
    autograd_iteration(ma, oa, step=False)
    fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:].numpy(), masks[:, 1:].numpy(), step=False)
    assert fb.last_active_rows > 0
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        if pa.grad is not None:
            assert U.grad_close(k, pb.grad.cpu().numpy(), pa.grad.cpu().numpy(), 2e-5), (k, U.relerr(pb.grad.cpu().numpy(), pa.grad.cpu().numpy()))
    # ... and with holes in the mask (a zero INSIDE a caption: its position still receives gradient through the recurrence from the later
    # steps, so it stays on the active list -- the list runs up to each caption's last non-zero entry)
    holed = masks[:, 1:].clone()
    holed[:, 1] = 0
    holed[::2, 0] = 0
    sync()
    autograd_iteration(ma, oa, step=False, mask=holed.to(dev))
    fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:].numpy(), holed.numpy(), step=False)
    last = np.where(holed.numpy().any(1), holed.shape[1] - np.argmax(holed.numpy()[:, ::-1] != 0, 1), 0)
    assert fb.last_active_rows == int(last.sum()) > int((holed != 0).sum())
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        if pa.grad is not None:
            assert U.grad_close(k, pb.grad.cpu().numpy(), pa.grad.cpu().numpy(), 2e-5), (k, U.relerr(pb.grad.cpu().numpy(), pa.grad.cpu().numpy()))
    clip_gradient(ob, 0.05)
    ob.step()
    oa.step()
    sync()
    # validation loss (eval mode, no backward): forward_only
    ma.eval(); mb.eval()
    with torch.no_grad():
        va = float(crit(ma(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train'), tgt, msk))
    vb = float(fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], tgt, msk, forward_only=True))
    assert abs(va - vb) < 1e-5 * abs(va)
    # the two paths interleaved on ONE model: an autograd iteration after a fused one (stale .grad views, arena bookkeeping) and back
    ma.train(); mb.train()
    sync()
    la = autograd_iteration(ma, oa)
    lb = autograd_iteration(mb, ob)
    assert abs(la - lb) < ltol * abs(la)          # (two models several Adam steps apart on split-K atomics: the loss, 0.02 here, moves in quanta of ~2e-6 relative between runs)
    assert not fixed or la == lb                  # fixed-order accumulation: the SAME path on twins in the same state gives the same bits
    sync()
    la = autograd_iteration(ma, oa)
    lb = float(fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], tgt, msk))
    assert abs(la - lb) < ltol * abs(la)
    assert oa._flat['step'] == ob._flat['step']
    # the joint 'tap_cg' iteration (train.py:300-313): d loss / d tap_feats comes back through `tap_grad` for the proposal encoder
    sync()
    tap_leaf = tap.clone().requires_grad_(True)
    oa.zero_grad()
    crit(ma(tap_leaf, c3d, lda, labels, vid['ind'], vid['soi'], mode='train'), tgt, msk).backward()
    g_tap = torch.zeros_like(tap)
    fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], step=False, tap_grad=g_tap)
    assert float(tap_leaf.grad.abs().max()) > 0
    assert U.grad_close('tap_feats', g_tap.cpu().numpy(), tap_leaf.grad.cpu().numpy(), 2e-5), U.relerr(g_tap.cpu().numpy(), tap_leaf.grad.cpu().numpy())
    with pytest.raises(ValueError):
        fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], tgt, msk, step=False, tap_grad=torch.zeros(3, device=dev))
    # ... and with the deferred update: tap_grad and the loss are final on return, the parameter gradients and Adam finish on the helper
    # streams (joined by join() / the next call); same update as the autograd iteration from the same state
    sync()
    la = autograd_iteration(ma, oa)
    g_ref = torch.zeros_like(tap)
    fb2_tap = torch.zeros_like(tap)
    lb = float(fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], tap_grad=fb2_tap, defer_update=True))
    assert abs(la - lb) < ltol * abs(la)
    assert U.grad_close('tap_feats', fb2_tap.cpu().numpy(), g_tap.cpu().numpy(), 1e-3)          # (same state up to one Adam step of noise-level drift)
    fb.join()
    assert oa._flat['step'] == ob._flat['step']
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        dp = (pa.detach() - pb.detach()).abs()
        if k not in U.NOISE_ONLY:          # (a noise-only gradient against several steps of Adam history: |m^ / sqrt(v^)| is not bounded by 1)
            assert float(dp.max()) <= 2.01 * lr, k
        if pa.grad is not None and k not in U.NOISE_ONLY:
            gg = pa.grad.abs()
            solid = gg > 1e-4 * gg.max()
            if bool(solid.any()):
                assert float(dp[solid].max()) < 0.02 * lr, (k, float(dp[solid].max()))
    # two deferred iterations back to back (the second call joins the first by itself), then an ordinary one
    for _ in range(2):
        fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], tap_grad=torch.zeros_like(tap), defer_update=True)
    lb = float(fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], tgt, msk))
    assert np.isfinite(lb)
    # the two-call form: prepare() (everything that does not read tap_feats, started before the proposal encoder's forward) + prepared=True
    sync()
    la = autograd_iteration(ma, oa)
    fb.prepare(c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:])
    filler = (torch.randn(256, 256, device=dev) @ torch.randn(256, 256, device=dev)).sum()          # (the caller's own work in between)
    with pytest.raises(RuntimeError):
        fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], tgt, msk)                                  # prepare() must be followed by prepared=True
    lb = float(fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], tap_grad=torch.zeros_like(tap), defer_update=True,
                  prepared=True))
    fb.join()
    assert abs(la - lb) < ltol * abs(la) and bool(torch.isfinite(filler))
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert k in U.NOISE_ONLY or float((pa.detach() - pb.detach()).abs().max()) <= 2.01 * lr, k
    with pytest.raises(RuntimeError):
        fb(tap, c3d, lda, labels, vid['ind'], vid['soi'], tgt, msk, prepared=True)                   # no prepare() before


@pytest.mark.parametrize('fixed', [False, True], ids=['atomic', 'fixed_order'])
@pytest.mark.parametrize('case', ['c1', 'c2'])
def test_fused_train_step_equals_autograd_path(case, fixed):
    """The comparison above with the default (atomic split-K, persistent recurrences) and with `echr_config_set("deterministic", 1)`: under
    fixed-order accumulation the loss gates between the two paths tighten from 5e-6 to 2e-6 relative (what is left is the two paths' different
    association of the same sums, not run-to-run noise)."""
    import echr_amd
    echr_amd.set_deterministic(fixed)
    try:
        _fused_train_step_vs_autograd_path(case, 2e-6 if fixed else 5e-6, fixed)
    finally:
        echr_amd.set_deterministic(False)


def test_deferred_update_survives_changing_shapes():
    """Joint-mode iterations (defer_update: parameter gradients + Adam finish on the helper streams after the call returns) alternating between
    two workloads of different sizes on ONE model: the workspace is re-allocated while a deferred update may still be running (the step joins
    first), the index ring is restaged -- the losses must equal those of the same sequence run with the update joined inside the call."""
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    dev = torch.device('cuda')
    cases = [synth.make_case(c) for c in ('c2', 'c1', 'c2full', 'c1', 'c2')]
    opt, params, _ = cases[0]

    def run(defer):
        m = U.build_gpu_model(opt, params, True)
        m.set_dropout_state(U.SEED, 7)
        o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
        f = FusedTrainStep(m, o, grad_clip=0.05)
        losses, taps = [], []
        for _, _, vid in cases * 2:
            tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
            labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
            g = torch.zeros_like(tap)
            losses.append(f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], tap_grad=g, defer_update=defer))
            taps.append(g)
        f.join()
        torch.cuda.synchronize()
        return [float(x) for x in losses], [float(t.abs().sum()) for t in taps], m

    la, ta, ma = run(False)
    lb, tb, mb = run(True)
    for i, (x, y) in enumerate(zip(la, lb)):
        assert abs(x - y) <= 2e-4 * abs(x), (i, x, y)          # (same trajectory up to atomic-order noise amplified by Adam over ten steps)
    for x, y in zip(ta, tb):
        assert abs(x - y) <= 2e-3 * abs(x) + 1e-12
    assert la[-1] < la[0]


def test_backward_pass_that_raises_does_not_poison_the_next_one():
    """The decoder's backward zero-fills the whole gradient arena once per pass and tells the later Functions of THAT pass so.  When a later
    node raises, autograd's end-of-pass callbacks do not run; the next pass must still zero-fill (the flag is tied to the graph task it was
    set in) -- otherwise it would accumulate into the failed pass's partial gradients."""
    from echr_amd.misc.utils import LanguageModelCriterion

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, g):
            raise RuntimeError('injected failure in a later backward node')

    opt, params, vid = synth.make_case('c1')
    dev = torch.device('cuda')
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])

    def backward(m, boom):
        m.set_dropout_state(U.SEED, U.OFFSET)
        tap = torch.from_numpy(vid['tap']).to(dev).requires_grad_(True)
        c3d, lda = torch.from_numpy(vid['c3d']).to(dev), torch.from_numpy(vid['lda']).to(dev)
        pred = m(Boom.apply(tap) if boom else tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
        LanguageModelCriterion()(pred, labels[:, 1:].to(dev), masks[:, 1:].to(dev)).backward()

    m = U.build_gpu_model(opt, params, True)
    arena = m.build_arena()
    with pytest.raises(RuntimeError, match='injected failure'):
        backward(m, True)
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=True)
    backward(m, False)
    assert arena.grads_in_arena()
    ref = U.build_gpu_model(opt, params, True)
    ref.build_arena()
    backward(ref, False)
    torch.cuda.synchronize()
    for (k, pa), (_, pb) in zip(m.named_parameters(), ref.named_parameters()):
        assert (pa.grad is None) == (pb.grad is None), k
        if pa.grad is not None:
            assert U.grad_close(k, pa.grad.cpu().numpy(), pb.grad.cpu().numpy(), 1e-5), (k, U.relerr(pa.grad.cpu().numpy(), pb.grad.cpu().numpy()))


@pytest.mark.parametrize('N,A,T_v,L,V1', [(1, 5, 9, 4, 57), (100, 37, 160, 7, 301), (70, 200, 256, 6, 129), (3, 1, 4, 3, 11),
                                           (6, 24, 60, 5, 9001)])          # a vocabulary in the row kernels' widest register form (<40>: 5121 .. 10240 columns)
def test_odd_shapes_vs_oracle(N, A, T_v, L, V1):
    """Shapes off the tuned path: N not a multiple of the 64-row MFMA block (N=1, 70, 100), A > 128 (config-5-like 256-segment
    videos), single-slot events, tiny vocabularies -- forward, loss and every gradient against the oracle (train mode)."""
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=L - 2)
    params = synth.make_params(opt, 3)
    vid = synth.make_video(N, A, L, V1, seed=N * 7 + A, T_v=T_v, min_len=1)
    pred, loss, grads, _ = U.run_gpu(opt, params, vid, True)
    rpred, rloss, rgrads = U.run_oracle(opt, params, vid, True)
    assert pred.shape == rpred.shape
    assert np.abs(pred - rpred).max() < TOL_LOGP, np.abs(pred - rpred).max()
    assert abs(loss - rloss) < TOL_LOSS * abs(rloss)
    for k, g in rgrads.items():
        if g is None:
            assert grads[k] is None, k
        else:
            assert U.grad_close(k, grads[k], g, TOL_GRAD), (k, U.relerr(grads[k], g))


@pytest.mark.parametrize('N,A,T_v,L,V1', [(1, 5, 9, 4, 57), (3, 1, 4, 3, 11), (70, 200, 256, 6, 129), (6, 24, 60, 5, 9001), (64, 129, 200, 12, 301),
                                           (33, 130, 260, 9, 2049)])
def test_fused_step_odd_shapes_vs_oracle(N, A, T_v, L, V1):
    """The one-call iteration (echr_train_step: active rows, fused criterion, three-stream tail) on shapes off the tuned path -- a single
    event, single-slot events, N > 64 (launch-per-step recurrences), a vocabulary beyond the register-resident criterion kernel, the
    129 / 130-segment boundary of the BIG instantiations: loss, every parameter gradient and d tap_feats against the oracle (train mode)."""
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=L - 2)
    params = synth.make_params(opt, 3)
    vid = synth.make_video(N, A, L, V1, seed=N * 7 + A, T_v=T_v, min_len=1)
    rpred, rloss, rgrads = U.run_oracle(opt, params, vid, True)
    dev = torch.device('cuda')
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
    f = FusedTrainStep(m, o, grad_clip=None)
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    g_tap = torch.zeros_like(tap)
    loss = float(f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], step=False, tap_grad=g_tap))
    assert abs(loss - rloss) < TOL_LOSS * abs(rloss), (loss, rloss)
    grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}
    for k, g in rgrads.items():
        if g is None:
            assert grads[k] is None, k
        else:
            assert U.grad_close(k, grads[k], g, TOL_GRAD), (k, U.relerr(grads[k], g))
    assert bool(torch.isfinite(g_tap).all()) and float(g_tap.abs().max()) > 0


def test_gemm_path_switches_do_not_change_results_beyond_tolerance():
    """echr_config_set('gemm_h2' / 'gemm_bf16x3'): the packed fp16-pair products, the bf16-plane split products and the native
    fp32 MFMA products agree to ~1e-6 on the whole forward/backward path."""
    from echr_amd import _lib
    lib = _lib.load()
    opt, params, vid = synth.make_case('c1')
    runs = {}
    try:
        for name, h2, x3 in (('f32', 0, 0), ('bf16x3', 0, 1), ('h2', 1, 1)):
            assert lib.echr_config_set(b'gemm_h2', h2) == 0 and lib.echr_config_set(b'gemm_bf16x3', x3) == 0
            runs[name] = U.run_gpu(opt, params, vid, False)
    finally:
        lib.echr_config_set(b'gemm_bf16x3', 1)
        lib.echr_config_set(b'gemm_h2', 1)
    p0, l0, g0, _ = runs['f32']
    for name in ('bf16x3', 'h2'):
        p1, l1, g1, _ = runs[name]
        assert np.abs(p0 - p1).max() < 2e-5 and abs(l0 - l1) < 1e-5 * abs(l0), name
        for k in g0:
            if g0[k] is not None:
                assert U.grad_close(k, g1[k], g0[k], 1e-4), (name, k)
    assert lib.echr_config_set(b'no_such_key', 1) != 0


@pytest.mark.parametrize('case', ['c1', 'c2', 'c2full'])
def test_persistent_recurrence_equals_launch_path(case):
    """echr_config_set('persist' / 'persist_bwd'): the persistent weights-stationary recurrences (csrc/persist.hip: forward and reverse)
    against the launch-per-phase recurrences on the same inputs, train mode (dropout), twice in a row (re-launch state: counters,
    exchange buffers), and each direction on its own."""
    from echr_amd import _lib
    lib = _lib.load()
    opt, params, vid = synth.make_case(case)
    runs = {}
    try:
        # (name, persist, persist_bwd, persist_h2): the default is everything on = each direction ONE launch of 256 workgroups
        for name, v, vb, h2 in (('launch', 0, 0, 1), ('persist', 1, 1, 1), ('persist2', 1, 1, 1), ('fwd_only', 1, 0, 1),
                                ('bwd_only', 0, 1, 1), ('f32_products', 1, 1, 0)):
            assert lib.echr_config_set(b'persist', v) == 0 and lib.echr_config_set(b'persist_bwd', vb) == 0
            assert lib.echr_config_set(b'persist_h2', h2) == 0
            runs[name] = U.run_gpu(opt, params, vid, True)
    finally:
        for key in (b'persist', b'persist_bwd', b'persist_h2'):
            lib.echr_config_set(key, 1)
    p0, l0, g0, _ = runs['launch']
    for name in ('persist', 'persist2', 'fwd_only', 'bwd_only', 'f32_products'):
        p1, l1, g1, _ = runs[name]
        assert np.isfinite(p1).all(), name
        assert np.abs(p0 - p1).max() < 2e-5 and abs(l0 - l1) < 1e-5 * abs(l0), (name, np.abs(p0 - p1).max())
        for k in g0:
            if g0[k] is not None:
                assert U.grad_close(k, g1[k], g0[k], 1e-4), (name, k, U.relerr(g1[k], g0[k]))


def _train_steps(m, o, vid, n, first=0):
    """n optimiser steps of the reference protocol on one video (clip_gradient + step); returns the parameters afterwards."""
    from echr_amd.misc.utils import LanguageModelCriterion, clip_gradient
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    for i in range(first, first + n):
        o.zero_grad()
        pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
        LanguageModelCriterion()(pred, labels[:, 1:].to(dev), masks[:, 1:].to(dev)).backward()
        clip_gradient(o, 0.05)
        o.step()
    torch.cuda.synchronize()
    return {k: p.detach().cpu().numpy().copy() for k, p in m.named_parameters()}


@pytest.mark.parametrize('arena', [True, False])
def test_optimizer_state_dict_resumes_and_matches_torch_adam_layout(arena):
    """train.py:214-216,456-461 save / restore `cg_optimizer.state_dict()`: after 3 steps save model + optimiser, load both into a
    FRESH model + optimiser, step 4 must equal the uninterrupted run (to the run-to-run noise of the fp32-atomic gradient sums, 1e-6
    of a 1e-3 update; a resume WITHOUT the optimiser state is off by 1e-3); the saved blob has torch.optim.Adam's layout (it loads
    into torch.optim.Adam and a torch.optim.Adam blob loads back)."""
    from echr_amd.optim import ClampAdam
    import io
    opt, params, vid = synth.make_case('tiny')

    def fresh(state=None):
        m = U.build_gpu_model(opt, params, True)           # pins the dropout stream (seed, offset)
        if state is not None:
            m.load_state_dict(state)
        ar = m.build_arena() if arena else None
        return m, ClampAdam(m.parameters(), lr=1e-3, arena=ar)

    m, o = fresh()
    _train_steps(m, o, vid, 3)
    buf = io.BytesIO()
    torch.save({'cg_model': m.state_dict(), 'cg_optimizer': o.state_dict(), 'drop_calls': m.lm_model._drop_calls}, buf)
    ref4 = _train_steps(m, o, vid, 1, first=3)
    ck = torch.load(io.BytesIO(buf.getvalue()), map_location='cuda')
    sd = ck['cg_optimizer']
    live = [k for k, p in m.named_parameters() if p.grad is not None]
    assert len(sd['state']) == len(live) and len(sd['state']) > 0
    for st in sd['state'].values():
        assert set(st) == {'step', 'exp_avg', 'exp_avg_sq'} and int(float(st['step'])) == 3
    m2, o2 = fresh(ck['cg_model'])
    o2.load_state_dict(sd)
    m2.set_dropout_state(U.SEED, ck['drop_calls'])
    got4 = _train_steps(m2, o2, vid, 1, first=3)
    for k in list(ref4):
        if k in U.NOISE_ONLY:          # true gradient exactly zero: Adam normalises pure rounding noise there (+-lr either way)
            del ref4[k]
    for k in ref4:
        assert np.abs(ref4[k] - got4[k]).max() < 1e-5, (k, np.abs(ref4[k] - got4[k]).max())
    m5, o5 = fresh(ck['cg_model'])                        # control: moments and step count lost -> visibly different step
    m5.set_dropout_state(U.SEED, ck['drop_calls'])
    lost4 = _train_steps(m5, o5, vid, 1, first=3)
    assert max(np.abs(ref4[k] - lost4[k]).max() for k in ref4) > 1e-4
    if arena:
        assert o2._flat is not None and not o2.state      # the resumed run stays on the single-launch path
    # layout interop with torch.optim.Adam (what the reference saves)
    # (torch's load_state_dict adopts the blob's tensors without copying and the step kernel updates moments in place: read the
    #  checkpoint again, as a real resume does)
    ck = torch.load(io.BytesIO(buf.getvalue()), map_location='cuda')
    m3, _ = fresh(ck['cg_model'])
    ta = torch.optim.Adam(m3.parameters(), lr=1e-3)
    ta.load_state_dict(ck['cg_optimizer'])
    m4, o4 = fresh(ck['cg_model'])
    o4.load_state_dict(ta.state_dict())
    m4.set_dropout_state(U.SEED, ck['drop_calls'])
    back4 = _train_steps(m4, o4, vid, 1, first=3)
    for k in ref4:
        assert np.abs(ref4[k] - back4[k]).max() < 1e-5, k


@pytest.mark.parametrize('arena,defer', [(True, True), (True, False), (False, True)])
def test_clip_gradient_with_accumulation_matches_reference_protocol(arena, defer):
    """m_batch = 2 (train.py:281-283,313-317): the reference clamps the RUNNING gradient after every backward, i.e.
    clamp(clamp(g1) + g2), then steps -- with |g| well above the clip value, so that clamp(g1 + g2) would differ.  ClampAdam follows that
    trajectory with its default settings (flat arena: the clamp deferred to the step kernel is applied before the second backward
    accumulates) and with defer_clamp = False (in-place clamp at every clip_gradient; .grad then holds clamped values too)."""
    from echr_amd.misc.utils import LanguageModelCriterion, clip_gradient
    from echr_amd.optim import ClampAdam
    opt, params, vid = synth.make_case('tiny')
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    clip = 0.002
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena() if arena else None)
    assert o.defer_clamp is True            # the default
    o.defer_clamp = defer
    mr = U.build_gpu_model(opt, params, True)
    ro = torch.optim.Adam(mr.parameters(), lr=1e-3)
    n_over = 0
    for mm, oo, ref in ((m, o, False), (mr, ro, True)):
        oo.zero_grad()
        for b in range(2):
            pred = mm(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
            LanguageModelCriterion()(pred, labels[:, 1:].to(dev), masks[:, 1:].to(dev)).backward()
            if ref:
                for p in mr.parameters():
                    if p.grad is not None:
                        if b == 0:
                            n_over += int((p.grad.abs() > clip).sum())
                        p.grad.data.clamp_(-clip, clip)
            else:
                clip_gradient(oo, clip)
        oo.step()
    assert n_over > 100                     # the first backward's gradient really exceeds the clip value in many entries
    for (k, p), (_, q) in zip(m.named_parameters(), mr.named_parameters()):
        if k in U.NOISE_ONLY:
            continue
        if q.grad is not None and not (arena and defer):
            assert float(p.grad.abs().max()) <= clip * (1 + 1e-6), k
            assert float((p.grad - q.grad).abs().max()) <= 1e-6 * clip + 1e-4 * float(q.grad.abs().max()), k
        assert float((p.detach() - q.detach()).abs().max()) < 2e-6, k


def test_two_criteria_on_one_decoder_output():
    """Two LanguageModelCriterion calls consuming the same log-probs (two target sets): both gradients must arrive (the fused sparse
    hand-over keeps a LIST of pending criteria and falls back to the dense form when there is more than one)."""
    from echr_amd import functional as EF
    from echr_amd.misc.utils import LanguageModelCriterion
    opt, params, vid = synth.make_case('c1')
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    tgt1 = labels[:, 1:].to(dev)
    tgt2 = ((labels[:, 1:] * 7 + 3) % (opt.CG_vocab_size + 1)).to(dev)
    msk = masks[:, 1:].to(dev)
    out = {}
    try:
        for fused in (True, False):
            EF.FUSED_NLL[0] = fused
            m = U.build_gpu_model(opt, params, True)
            pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
            loss = LanguageModelCriterion()(pred, tgt1, msk) + 0.5 * LanguageModelCriterion()(pred, tgt2, msk)
            loss.backward()
            torch.cuda.synchronize()
            out[fused] = {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}
    finally:
        EF.FUSED_NLL[0] = True
    for k, g0 in out[False].items():
        assert U.grad_close(k, out[True][k], g0, 2e-5), (k, U.relerr(out[True][k], g0))


def test_clamp_propagates_nan_like_torch():
    from echr_amd import functional as EF
    g = torch.tensor([1.0, float('nan'), -500.0, 7.0, float('inf'), 0.5, 3.0], device='cuda')
    out = EF.clamp_(g.clone(), 100.0).cpu()
    ref = g.cpu().clamp(-100.0, 100.0)
    assert torch.isnan(out[1]) and torch.equal(torch.nan_to_num(out, nan=-1.0), torch.nan_to_num(ref, nan=-1.0))
    p = torch.ones(7, device='cuda')
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    EF.clamp_adam_(p, g, m, v, 1, 1e-3, 0.9, 0.999, 1e-8, 100.0)
    assert torch.isnan(p[1]) and torch.isfinite(p[[0, 2, 3, 4, 5, 6]]).all()


@pytest.mark.parametrize('case', ['tiny', 'c1'])
def test_get_logprobs_state_single_step_vs_oracle(case):
    """OldModel.get_logprobs_state (OldModel_NEW.py:133-137): one timestep with state in / state out, three consecutive steps from the
    zero state, against oracle.logprobs_state; also equals the teacher-forced forward()'s log-probs of those steps."""
    from echr_amd import functional as EF
    from oracle import echr_ref_cpu as O
    opt, params, vid = synth.make_case(case)
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]) for k in ('tap', 'c3d', 'lda'))
    labels = torch.from_numpy(vid['labels'])
    P = {k: torch.from_numpy(v) for k, v in params.items()}
    with torch.no_grad():
        event_ref = O.event_context(P, tap, c3d, vid['ind'], vid['soi'], opt.n_head)
        clip_ref, mask_ref = O.clip_context(c3d, vid['soi'])
        video = m.get_video_context(tap.to(dev), c3d.to(dev), lda.to(dev), vid['ind'], vid['soi'])
        event = m.get_event_context(tap.to(dev), c3d.to(dev), lda.to(dev), vid['ind'], vid['soi'])
        clip, cmask = m.get_clip_context(tap.to(dev), c3d.to(dev), lda.to(dev), vid['ind'], vid['soi'])     # padded [N,A,D] + mask (reference form)
        full = m(tap.to(dev), c3d.to(dev), lda.to(dev), labels, vid['ind'], vid['soi'], mode='train').cpu()
        state = m.lm_model.init_hidden(video, event, clip)
        N, H = event.shape[0], opt.CG_rnn_size
        rstate = (torch.zeros(3, N, H), torch.zeros(3, N, H))
        for t in range(min(3, full.shape[1])):
            it = labels[:, t]
            logp, state = m.lm_model.get_logprobs_state(it.to(dev), video, event, clip, cmask, state)
            rlogp, rstate = O.logprobs_state(P, it, lda, event_ref, clip_ref, mask_ref, rstate)
            assert float((logp.cpu() - rlogp).abs().max()) < TOL_LOGP, t
            assert float((state[0].cpu() - rstate[0]).abs().max()) < 1e-5 and float((state[1].cpu() - rstate[1]).abs().max()) < 1e-5, t
            assert float((logp.cpu() - full[:, t]).abs().max()) < 2e-5, t


def test_attention_module_multi_head_forward_vs_oracle():
    """fusion_model.enc_attn(roi_feat, position_embedding) on its own (MA_attention_8_NEW.py:101-177) == the oracle's TSRM on the same
    embedded events; and MA_Attention8.forward == enc_attn(event_emb(feats), pos)."""
    from echr_amd import functional as EF
    from oracle import echr_ref_cpu as O
    opt, params, vid = synth.make_case('c1')
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d = torch.from_numpy(vid['tap']), torch.from_numpy(vid['c3d'])
    P = {k: torch.from_numpy(v) for k, v in params.items()}
    with torch.no_grad():
        ech = torch.cat((O.event_pool(c3d, vid['soi']), tap[torch.from_numpy(vid['ind'])]), 1)
        ref = O.tsrm_forward(P, ech, vid['soi'], opt.n_head)
        fm = m.fusion_model
        pm = fm.extract_position_matrix(np.asarray(vid['soi']), len(vid['soi']))
        pos = torch.from_numpy(fm.extract_position_embedding(pm, opt.d_feats).astype(np.float32)).to(dev)
        x = torch.nn.functional.linear(ech, P['fusion_model.event_emb.weight'], P['fusion_model.event_emb.bias']).to(dev)
        out = fm.enc_attn(x, pos, True)
        whole = fm(ech.to(dev), vid['soi'])
    assert float((out.cpu() - ref).abs().max()) < 1e-5
    assert float((out - whole).abs().max()) < 1e-5


def test_reference_checkpoint_reproduces_reference_output():
    """Weights initialised and saved by the reference itself -> loaded as is -> the reference's own eval-mode log-probs."""
    import echr_amd
    import os
    opt, _, vid = synth.make_case('tiny')
    ck = torch.load(os.path.join(U.GOLD, 'ref_tiny_checkpoint.pth'), map_location='cpu')
    m = echr_amd.CaptionGenerator(opt)
    m.load_state_dict(ck['cg_model'])
    m = m.cuda().eval()
    dev = torch.device('cuda')
    pred = m(torch.from_numpy(vid['tap']).to(dev), torch.from_numpy(vid['c3d']).to(dev), torch.from_numpy(vid['lda']).to(dev),
             torch.from_numpy(vid['labels']), vid['ind'], vid['soi'], mode='train')
    ref = U.gold('ref_tiny_checkpoint_out.npz')['logp']
    assert np.abs(pred.detach().cpu().numpy() - ref).max() < TOL_LOGP


@pytest.mark.parametrize('joint,m_batch', [(False, 1), (True, 2)])
def test_reference_shaped_driver_trains_and_checkpoints(tmp_path, joint, m_batch):
    """examples/train_synthetic.py: train.py's call protocol (m_batch accumulation, clip, two optimisers, joint tap_cg mode
    with gradients through tap_feats into the SST), loss goes down, checkpoint in the reference's dict layout round-trips."""
    import importlib.util
    import os
    import echr_amd
    spec = importlib.util.spec_from_file_location('train_synthetic', os.path.join(os.path.dirname(U.GOLD), '..', 'examples', 'train_synthetic.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = str(tmp_path / 'ckpt.pth')
    argv = ['--iters', '24', '--m_batch', str(m_batch), '--save', path, '--quiet', '--lr', '2e-3'] + (['--joint'] if joint else [])
    hist, cg, tap = mod.main(argv)
    assert np.mean(hist[-4:]) < np.mean(hist[:4]) - 0.1, hist
    ck = torch.load(path, map_location='cpu')
    assert set(ck) == {'iteration', 'cg_model', 'tap_model', 'cg_optimizer', 'tap_optimizer'}
    assert len(ck['cg_optimizer']['state']) > 0 and all('exp_avg' in st for st in ck['cg_optimizer']['state'].values())
    hist2, _, _ = mod.main(['--iters', '4', '--m_batch', str(m_batch), '--resume', path, '--quiet', '--lr', '2e-3'] + (['--joint'] if joint else []))
    assert np.mean(hist2) < np.mean(hist[:4]) - 0.1, (hist2, hist[:4])        # picks up where the first run stopped (not from scratch)
    fresh = echr_amd.CaptionGenerator(cg.opt)
    fresh.load_state_dict(ck['cg_model'])
    for (k, a), (_, b) in zip(cg.state_dict().items(), fresh.state_dict().items()):
        assert torch.equal(a.cpu(), b), k
    if joint:
        assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in tap.parameters())


def _sst_module(params, opt_over, train):
    from echr_amd import models
    opt = synth.default_opt(**opt_over)
    m = models.setup_tap(opt)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.cuda()
    m.train() if train else m.eval()
    return m, opt


def test_sst_native_matches_reference_fixture():
    """models.setup_tap(opt) on the GPU (echr_sst_fwd/bwd, echr_tap_bce_*) against the reference's nn.LSTM-based SST +
    TAPModelCriterion outputs and gradients (eval mode: no dropout)."""
    from echr_amd.misc.utils import TAPModelCriterion
    g = U.gold('sst.npz')
    params = {k[len('param|'):]: v for k, v in g.items() if k.startswith('param|')}
    m, _ = _sst_module(params, dict(synth.CASES['tiny']['opt'], K=8), False)
    dev = torch.device('cuda')
    tap, sc = m(torch.from_numpy(g['x']).to(dev))
    assert np.abs(tap.detach().cpu().numpy() - g['tap']).max() < 1e-5 and np.abs(sc.detach().cpu().numpy() - g['scores']).max() < 1e-5
    loss = TAPModelCriterion()(sc, torch.from_numpy(g['masks']), torch.from_numpy(g['labels']), torch.from_numpy(g['w1'])) + 0.1 * (tap * tap).sum()
    assert abs(float(loss.detach()) - float(g['loss'])) < 1e-4 * abs(float(g['loss']))
    loss.backward()
    for k, p in m.named_parameters():
        assert U.grad_close(k, p.grad.cpu().numpy(), g['grad|' + k], TOL_GRAD), (k, U.relerr(p.grad.cpu().numpy(), g['grad|' + k]))


@pytest.mark.parametrize('T,D,H,K,train', [(37, 500, 512, 256, True), (5, 20, 24, 8, True), (64, 500, 512, 32, False), (1, 500, 512, 16, True),
                                           (2, 500, 512, 16, True), (256, 500, 512, 256, True)])
def test_sst_native_vs_oracle(T, D, H, K, train):
    """ECHR-sized SST (500 -> 512, K anchors) incl. the inter-layer dropout with injected Philox masks, forward and backward."""
    from echr_amd import philox
    from oracle import echr_ref_cpu as O
    rs = np.random.RandomState(T + K)
    shapes = {'rnn.weight_ih_l0': (4 * H, D), 'rnn.weight_hh_l0': (4 * H, H), 'rnn.bias_ih_l0': (4 * H,), 'rnn.bias_hh_l0': (4 * H,),
              'rnn.weight_ih_l1': (4 * H, H), 'rnn.weight_hh_l1': (4 * H, H), 'rnn.bias_ih_l1': (4 * H,), 'rnn.bias_hh_l1': (4 * H,),
              'scores.weight': (K, H), 'scores.bias': (K,)}
    params = {k: (rs.uniform(-1, 1, size=s) / np.sqrt(H)).astype(np.float32) for k, s in shapes.items()}
    m, opt = _sst_module(params, dict(video_dim=D, hidden_dim=H, K=K, rnn_dropout=0.5), train)
    m.set_dropout_state(U.SEED, U.OFFSET)
    x = rs.standard_normal((T, D)).astype(np.float32)
    wt = rs.standard_normal((T, H)).astype(np.float32)
    ws = rs.standard_normal((T, K)).astype(np.float32)
    dev = torch.device('cuda')
    tap, sc = m(torch.from_numpy(x).to(dev))
    ((tap * torch.from_numpy(wt).to(dev)).sum() + (sc * torch.from_numpy(ws).to(dev)).sum()).backward()
    P = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in params.items()}
    mask = torch.from_numpy(philox.scale_mask((T, H), 0.5, U.SEED, U.OFFSET, philox.SITE_SST, 0)) if train else None
    otap, osc = O.sst_forward(P, torch.from_numpy(x), mask)
    ((otap * torch.from_numpy(wt)).sum() + (osc * torch.from_numpy(ws)).sum()).backward()
    assert np.abs(tap.detach().cpu().numpy() - otap.detach().numpy()).max() < 2e-5
    assert np.abs(sc.detach().cpu().numpy() - osc.detach().numpy()).max() < 2e-5
    for k, p in m.named_parameters():
        assert U.grad_close(k, p.grad.cpu().numpy(), P[k].grad.numpy(), TOL_GRAD), (k, U.relerr(p.grad.cpu().numpy(), P[k].grad.numpy()))


def test_sst_persistent_equals_wavefront_launches():
    """The one-launch persistent form of the proposal encoder's recurrence (registers hold the recurrent matrices, sentinel-polled rows)
    against the T+1-launch wavefront form it replaces: outputs and gradients agree to fp32 summation-order noise."""
    from echr_amd import _lib
    lib = _lib.load()
    rs = np.random.RandomState(5)
    T, D, H, K = 96, 500, 512, 64
    shapes = {'rnn.weight_ih_l0': (4 * H, D), 'rnn.weight_hh_l0': (4 * H, H), 'rnn.bias_ih_l0': (4 * H,), 'rnn.bias_hh_l0': (4 * H,),
              'rnn.weight_ih_l1': (4 * H, H), 'rnn.weight_hh_l1': (4 * H, H), 'rnn.bias_ih_l1': (4 * H,), 'rnn.bias_hh_l1': (4 * H,),
              'scores.weight': (K, H), 'scores.bias': (K,)}
    params = {k: (rs.uniform(-1, 1, size=s) / np.sqrt(H)).astype(np.float32) for k, s in shapes.items()}
    x = torch.from_numpy(rs.standard_normal((T, D)).astype(np.float32)).cuda()
    wt = torch.from_numpy(rs.standard_normal((T, H)).astype(np.float32)).cuda()
    out = {}
    try:
        for persist in (1, 0):
            assert lib.echr_config_set(b'sst_persist', persist) == 0
            m, _ = _sst_module(params, dict(video_dim=D, hidden_dim=H, K=K, rnn_dropout=0.5), True)
            m.set_dropout_state(U.SEED, U.OFFSET)
            tap, sc = m(x)
            ((tap * wt).sum() + sc.sum()).backward()
            torch.cuda.synchronize()
            out[persist] = (tap.detach().cpu().numpy(), sc.detach().cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in m.named_parameters()})
    finally:
        lib.echr_config_set(b'sst_persist', 1)
    assert lib.echr_check_async() == 0
    assert np.isfinite(out[1][0]).all() and np.abs(out[1][0] - out[0][0]).max() < 1e-5 and np.abs(out[1][1] - out[0][1]).max() < 1e-5
    for k, g in out[0][2].items():
        assert U.grad_close(k, out[1][2][k], g, TOL_GRAD), (k, U.relerr(out[1][2][k], g))


def test_top_proposals_bit_exact_vs_reference():
    """echr_amd.eval_utils.gettop1000 (one HIP kernel) against the reference's gettop1000 index outputs (fixtures) incl. ties."""
    from echr_amd import eval_utils as EU
    g = U.gold('proposals.npz')
    for i in range(3):
        scores, mask, topN = g['g%d|scores' % i], g['g%d|mask' % i], int(g['g%d|topN' % i])
        ind, feat, _, ts, conf = EU.gettop1000(torch.from_numpy(scores).cuda(), mask, [], 100.0, lambda s, e, n, d: [s, e], topN=topN)
        assert ind == g['g%d|ind' % i].tolist() and feat == g['g%d|feat' % i].reshape(-1, 2).tolist() and ts == feat
        assert np.allclose(conf, (scores * mask)[np.array(ind), np.array(ind) - np.array(feat)[:, 0]])
    # heavy ties + a threshold above the topN-th value
    rs = np.random.RandomState(0)
    scores = np.round(rs.uniform(0, 1, size=(50, 20)), 1).astype(np.float32)
    mask = (np.arange(50)[:, None] >= np.arange(20)[None, :]).astype(np.float32)
    from oracle import echr_ref_cpu as O
    for topN, thr in ((30, 0.0), (100, 0.75), (5000, 0.0)):
        oi, of, oc = O.top_proposals(scores, mask, topN, thr)
        ind, feat, _, _, conf = EU.gettop1000(torch.from_numpy(scores).cuda(), mask, [], 1.0, lambda s, e, n, d: 0, val_score_thres=thr, topN=topN)
        assert ind == oi and feat == of and np.allclose(conf, oc)


def test_nms_proposals_bit_exact_vs_reference():
    """echr_amd.eval_utils.gettop1000_nms (one HIP kernel) against the reference's gettop1000_nms outputs (fixtures) and, on a grid
    with many tied scores, against the oracle's stable-sort reading of it."""
    from echr_amd import eval_utils as EU
    from oracle import echr_ref_cpu as O
    g = U.gold('proposals.npz')
    for i in range(3):
        scores, topN, ov = g['n%d|scores' % i], int(g['n%d|topN' % i]), float(g['n%d|overlap' % i])
        ind, props, gts, ts, conf = EU.gettop1000_nms(torch.from_numpy(scores).cuda(), None, [], 100.0, lambda s, e, n, d: [s, e], overlap=ov, topN=topN)
        assert np.array_equal(props, g['n%d|props' % i]) and np.array_equal(conf, g['n%d|conf' % i])
        assert np.array_equal(ind, props[:, 1] - 1) and ts == [[int(s), int(e)] for s, e in props]
    rs = np.random.RandomState(3)
    scores = np.round(rs.uniform(0, 1, size=(70, 24)), 1).astype(np.float32)
    for ov, topN in ((0.5, 40), (0.95, 2000)):
        _, oprops, oconf = O.top_proposals_nms(scores, ov, topN)
        _, props, _, _, conf = EU.gettop1000_nms(torch.from_numpy(scores).cuda(), None, [], 1.0, lambda s, e, n, d: 0, overlap=ov, topN=topN)
        assert np.array_equal(props, oprops) and np.array_equal(conf, oconf)


@pytest.mark.parametrize('nms', [0.0, 0.6])
def test_eval_flow_sst_to_captions_vs_oracle(nms):
    """eval_utils.caption_video (SST -> proposal selection -> greedy captions, eval_utils.py:51-167) against the same chain built from
    the oracle's pieces on the host: identical proposals (integers), identical token sequences, scores within 1e-4."""
    from echr_amd import eval_utils as EU, models as EM
    from oracle import echr_ref_cpu as O
    opt, params, vid = synth.make_case('c1')
    opt.K = 8
    cg = U.build_gpu_model(opt, params, False)
    torch.manual_seed(3)
    tap = EM.setup_tap(opt).cuda()
    tap.eval()                                   # the reference's SST.eval() returns None (sst_model.py:25-29)
    dev = torch.device('cuda')
    rs = np.random.RandomState(11)
    T = 24
    c3d = rs.standard_normal((T, opt.video_dim)).astype(np.float32)
    lda = rs.standard_normal(opt.video_context_dim).astype(np.float32)
    f2t = lambda s, e, n, d: [round(float(s) / n * d, 3), round(float(e) / n * d, 3)]
    info, ex = EU.caption_video(tap, cg, torch.from_numpy(c3d).to(dev), torch.from_numpy(lda).to(dev), 60.0, f2t, topN=12,
                                nms_threshold=nms)
    # host chain from the oracle's pieces
    P_tap = {k: v.detach().cpu() for k, v in tap.state_dict().items()}
    tap_o, sc_o = O.sst_forward(P_tap, torch.from_numpy(c3d))
    assert np.abs(ex['pred_proposals'].cpu().numpy() - sc_o.numpy()).max() < 1e-5
    sc_dev = ex['pred_proposals'].cpu().numpy()                        # selection is discontinuous in the scores: feed both the same ones
    masks = (np.arange(T)[:, None] >= np.arange(opt.K)[None, :]).astype(np.float32)
    if nms:
        _, props, conf = O.top_proposals_nms(sc_dev, nms, 12)
        ind, soi = (props[:, 1] - 1).tolist(), props.tolist()
    else:
        ind, soi, conf = O.top_proposals(sc_dev, masks, 12, 0.0)
    assert [list(map(int, x)) for x in ex['soi_select_list']] == [list(map(int, x)) for x in soi] and len(info) == len(ind)
    P = {k: torch.from_numpy(v) for k, v in params.items()}
    assert np.abs(ex['tap_feats'].cpu().numpy() - tap_o.numpy()).max() < 1e-5
    seq_o, lp_o = O.caption_forward(P, ex['tap_feats'].cpu(), torch.from_numpy(c3d), torch.from_numpy(lda), None, ind, soi, mode='eval',
                                    seq_length=opt.CG_seq_length)
    assert np.array_equal(ex['seq'].cpu().numpy(), seq_o.numpy())
    for i, rec in enumerate(info):
        assert rec['timestamp'] == f2t(soi[i][0], soi[i][1], T, 60.0) and rec['num'] == [i, len(info)]
        assert abs(rec['proposal_score'] - float(conf[i])) < 1e-6
        assert abs(rec['sentence_confidence'] - float(lp_o[i].sum())) < 1e-3
        assert rec['sentence'] == [int(t) for t in seq_o[i].numpy() if t > 0]


@pytest.mark.parametrize('overlap', [False, True, 'staged', 'fused', 'fused_coop', 'fused1'])
def test_two_rank_data_parallel_on_one_gpu(tmp_path, overlap):
    """Two data-parallel ranks (separate processes, gloo transport, both on cuda:0) run two optimiser steps on different videos:
    both ranks must end with IDENTICAL parameters, equal to one process that accumulates the two videos' gradients before each
    step (the reference's m_batch = 2, train.py:281-283,313-317) -- with the staged early all-reduce on and off."""
    import socket
    import subprocess
    import sys as _sys
    from echr_amd.misc.utils import LanguageModelCriterion, clip_gradient
    from echr_amd.optim import ClampAdam
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = str(s.getsockname()[1]); s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = [str(tmp_path / ('rank%d.npz' % r)) for r in range(2)]
    # overlap=False: launch-per-phase recurrences; overlap=True: persistent recurrences launched cooperatively by both processes (the form
    # real data-parallel runs use) -- two plain 256-workgroup persistent grids must never share a device
    # 'staged': the three-stage decoder backward (ECHR_DP_STAGED=1: logit- and LSTM-layer ranges early); True: the one-call backward with the
    # LSTM-layer range reduced early (the default form)
    # 'fused' / 'fused_coop': the ONE host path of bench.py for every world size -- echr_train_step(step=False, handover) per rank, the logit- and
    # LSTM-layer ranges handed to the collective stream from the library's hand-over events while the backward tail still runs, then the
    # remainder, clip + step (fused.DataParallelStep); launch-per-phase recurrences / cooperative persistent ones.  'fused1': one collective
    mode = {False: '0', True: '1', 'staged': '1', 'fused': 'fused', 'fused_coop': 'fused', 'fused1': 'fused1'}[overlap]
    env = dict(os.environ, ECHR_DP_WORKER_COOP='1' if overlap in (True, 'fused_coop') else '0', ECHR_DP_STAGED='1' if overlap == 'staged' else '0')
    procs = [subprocess.Popen([_sys.executable, os.path.join(root, 'tests', 'dp_worker.py'), str(r), '2', port, outs[r], mode],
                              cwd=root, env=env) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    r0, r1 = np.load(outs[0]), np.load(outs[1])
    assert int(r0['n_collectives']) == {False: 1, True: 3, 'staged': 4, 'fused': 4, 'fused_coop': 4, 'fused1': 1}[overlap]
    if overlap in ('fused', 'fused_coop'):
        assert int(r0['n_early']) == 2          # both hand-over points were recorded and used
    for k in synth.state_dict_shapes(synth.make_case('c1')[0]):
        assert np.array_equal(r0[k], r1[k]), k                               # replicas stay bitwise identical after two steps
    # one process accumulating the two videos' gradients of step 0 (same initial parameters)
    dev = torch.device('cuda')
    opt, params, _ = synth.make_case('c1')
    model = U.build_gpu_model(opt, params, True)
    crit = LanguageModelCriterion()
    for rank in range(2):
        vid = synth.make_video(2, 16, 11, opt.CG_vocab_size + 1, seed=500 + rank, T_v=40, video_dim=opt.video_dim,
                               hidden_dim=opt.hidden_dim, lda_dim=opt.video_context_dim)
        tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
        labels = torch.from_numpy(vid['labels'])
        model.set_dropout_state(U.SEED, U.OFFSET + rank)
        crit(model(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train'), labels[:, 1:].to(dev),
             torch.from_numpy(vid['masks'])[:, 1:].to(dev)).backward()
    for k, p in model.named_parameters():
        if p.grad is None:
            assert 'grad|' + k not in r0.files, k
        else:
            assert np.array_equal(r0['grad|' + k], r1['grad|' + k]), k
            assert U.grad_close(k, r0['grad|' + k], p.grad.detach().cpu().numpy(), 1e-5), k     # SUM over ranks == accumulation, no 1/R


@pytest.mark.parametrize('mode,algo,via', [('fused', 'allreduce', 'callback'), ('fused', 'rs_ag', 'callback'), ('fused', 'rs_ag', 'event'), ('fused1', 'rs_ag', 'callback')])
def test_single_rank_rccl_one_call_path(tmp_path, mode, algo, via):
    """The collectives of the data-parallel paths on RCCL itself (backend 'nccl'; the gloo rehearsals above never touch it): ONE rank on cuda:0
    -- RCCL wants a device per rank -- with persistent recurrences launched cooperatively, as bench.py does for N > 1.  A sum over one rank
    is the identity, so the first step's gradients must equal the same worker's over gloo to the run-to-run noise of the split-K atomics
    (1e-5 of the tensor's maximum) and the parameters after two Adam steps to 2 x 2 x lr: this pins the nccl-only branches (asynchronous
    reduce-scatter + all-gather on the collective stream, Work.wait() stream semantics, hand-over waits) as far as ONE rank can: it proves
    that they run and leave the values alone.  It cannot show a premature hand-over -- over one rank every collective is the identity, in
    place -- so WHERE the hand-over points sit is pinned separately (test_handover_points_see_final_ranges: a snapshot queued at each point
    must equal the final range); that RCCL orders its stream behind the library stream made current in the callback, and that waiting for
    the last collective waits for all (fused.DataParallelStep._in_order), is torch.distributed's documented contract and stays UNVERIFIED
    on hardware until a run on two or more GPUs exists."""
    import socket
    import subprocess
    import sys as _sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for backend in ('nccl', 'gloo'):
        s = socket.socket(); s.bind(('127.0.0.1', 0)); port = str(s.getsockname()[1]); s.close()
        out = str(tmp_path / (backend + '.npz'))
        # via: how an early range reaches the collective stream -- 'callback' (default): queued from inside echr_train_step at the hand-over point
        # with the library's stream current; 'event': a side stream per range waits for the hand-over event
        env = dict(os.environ, ECHR_DP_WORKER_COOP='1', ECHR_DP_WORKER_BACKEND=backend, ECHR_DP_WORKER_ALGO=algo, ECHR_DP_STAGED='0', ECHR_DP_VIA=via)
        p = subprocess.Popen([_sys.executable, os.path.join(root, 'tests', 'dp_worker.py'), '0', '1', port, out, mode], cwd=root, env=env)
        assert p.wait(timeout=600) == 0, backend
        res[backend] = np.load(out)
    a, b = res['nccl'], res['gloo']
    assert int(a['n_collectives']) == int(b['n_collectives']) and int(a['n_collectives']) >= 1
    if mode == 'fused':
        assert int(a['n_early']) == 2
    assert set(a.files) == set(b.files)
    for k in a.files:
        if k.startswith('grad|'):
            assert U.grad_close(k[5:], a[k], b[k], 1e-5), (k, U.relerr(a[k], b[k]))
        elif a[k].dtype.kind == 'f':
            assert np.abs(a[k] - b[k]).max() <= 4.1e-3, k          # (lr = 1e-3: Adam's first steps move a parameter by <= lr, whatever the gradient's size)
            if k not in U.NOISE_ONLY:                              # (a true gradient of exactly zero: the update is a coin flip of +-lr)
                assert np.mean(np.abs(a[k] - b[k]) > 1e-4) < 0.02, k   # ... and only elements whose gradient is at the noise floor differ at all


@pytest.mark.parametrize('case', ['c2', 'c3bench'])
def test_handover_points_see_final_ranges(case):
    """echr_train_step_args.handover_cb (the data-parallel path's early collectives): what is queued on the stream the callback receives must
    see the FINAL gradients of its range.  The 'collective' here is a snapshot copy queued exactly where fused.DataParallelStep queues
    reduce_sum_ (library stream made current); a hand-over point in front of the last launch that writes the range -- or in front of a
    split-K slice still adding into it -- would leave the snapshot short of the final values.  train.py:281-283,313-317."""
    from echr_amd.fused import DataParallelStep, FusedTrainStep
    from echr_amd.optim import ClampAdam
    opt, params, vid = synth.make_case(case)
    dev = torch.device('cuda')
    m = U.build_gpu_model(opt, params, True)
    ar = m.build_arena()
    f = FusedTrainStep(m, ClampAdam(m.parameters(), lr=1e-3, arena=ar))
    ranges = DataParallelStep(f)._range
    assert set(ranges) == {0, 1}
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels = torch.from_numpy(vid['labels'])
    for rep in range(3):          # (the first call also builds workspaces; later calls run with every stream warm)
        snaps, ext = {}, {}

        def cb(which, stream_ptr):
            lo, hi = ranges[which]
            st = ext.setdefault(stream_ptr, torch.cuda.ExternalStream(stream_ptr, device=dev))
            with torch.cuda.stream(st):
                snaps[which] = ar.flat_g[lo:hi].clone()
        f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:].numpy(), vid['masks'][:, 1:], step=False, handover=True, handover_cb=cb)
        torch.cuda.synchronize()
        assert set(snaps) == {0, 1}, snaps.keys()
        for which, (lo, hi) in ranges.items():
            final = ar.flat_g[lo:hi]
            assert float(final.abs().max()) > 0
            assert torch.equal(snaps[which], final), (rep, which, float((snaps[which] - final).abs().max()))


@pytest.mark.parametrize('fused', ['auto', 'off'])
def test_bench_two_rank_rehearsal_on_one_gpu(fused):
    """(fused = 'auto': every rank's iteration as one echr_train_step call up to the backward pass with the early range collectives started
    from its hand-over events, then clip + step -- the same host path as the single-rank line; 'off': the autograd path + EarlyReducer.)
    The WHOLE multi-rank bench path on the one-GPU box: `python bench.py --gpus 2` launches its own two ranks (gloo transport, both on
    cuda:0, launch-per-phase recurrences), runs warm-up + timed steps with the staged early reducer, takes the MAX over ranks and prints
    ONE JSON line whose value is the whole-job rate."""
    import json
    import subprocess
    import sys as _sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ECHR_BENCH_BACKEND='gloo', ECHR_BENCH_ONE_GPU='1')
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([_sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '4', '--warmup', '2', '--full', '--no-cpu',
                        '--no-native', '--no-roofline', '--fused', fused], env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out['config']['host_path'].startswith('echr_train_step + early range collectives' if fused == 'auto' else 'autograd')
    assert out['config']['dp_overlap'] is True
    assert out['config']['dp_algo'] == 'allreduce' and out['config']['persist_coop'] == 1      # two ranks: one link; a shared device: cooperative launches
    if fused == 'auto':          # the exchange pass: exposed wait per step, the ranges and which of them started inside the backward tail
        ex = out['config']['exchange']
        assert out['config']['exchange_exposed_ms'] == ex['exposed_ms_median'] and ex['exposed_ms_median'] >= 0 and ex['steps'] >= 3
        assert sorted(r['name'] for r in ex['ranges'] if r['early']) == ['LSTM layers', 'logit layer'] and ex['n_early'] == 2
        assert sum(r['bytes'] for r in ex['ranges']) == 4 * 21712392 or sum(r['bytes'] for r in ex['ranges']) % 256 == 0
    assert out['n_gpus'] == 2 and out['steps'] == 4 and out['scaling'] == 'weak' and out['config']['global_events'] == 128
    assert out['value'] > 0 and abs(out['value'] - 4 * 20 * 2 / (out['ms_per_step'] * 4 / 1e3)) < 0.01 * out['value']
    assert np.isfinite(out['config']['final_loss'])


@pytest.mark.gpu
@pytest.mark.parametrize('extra_consumer', [False, True])
def test_fused_criterion_gradient_equals_dense_path(extra_consumer):
    """LanguageModelCriterion on the native decoder's output leaves its gradient with the decoder node in sparse form (targets, mask,
    upstream scalar: echr_dec_grads.nll_*) instead of a dense [N,S,V+1] tensor.  Same gradients as the dense route (ECHR_FUSED_NLL=0),
    also when the log-probs have a second consumer (then the placeholder is accumulated away and the dense form is added back) and
    under an upstream factor (lambda2 * loss, train.py:322-329)."""
    from echr_amd import functional as EF
    from echr_amd.misc.utils import LanguageModelCriterion
    opt, params, vid = synth.make_case('c1')
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    out = {}
    try:
        for fused in (True, False):
            EF.FUSED_NLL[0] = fused
            m = U.build_gpu_model(opt, params, True)
            pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
            loss = 0.7 * LanguageModelCriterion()(pred, labels[:, 1:].to(dev), masks[:, 1:].to(dev))
            if extra_consumer:
                wgt = torch.linspace(-1.0, 1.0, pred.numel(), device=dev).view_as(pred) * 1e-4
                loss = loss + (pred * wgt).sum()
            loss.backward()
            torch.cuda.synchronize()
            out[fused] = (float(loss.detach()), {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None})
    finally:
        EF.FUSED_NLL[0] = True
    assert abs(out[True][0] - out[False][0]) <= 1e-6 * abs(out[False][0])
    for k, g0 in out[False][1].items():
        assert U.grad_close(k, out[True][1][k], g0, 2e-5), (k, U.relerr(out[True][1][k], g0))


@pytest.mark.gpu
@pytest.mark.parametrize('N,A,L,min_len,video_dim', [(1, 1, 3, 1, 500), (31, 43, 4, 1, 500), (33, 44, 6, 2, 500), (64, 129, 5, 100, 500),
                                                      (32, 5, 9, 1, 512), (17, 87, 3, 50, 8), (64, 2, 21, 1, 500),
                                                      # events longer than 129 segments: the second slot set of the BIG instantiations
                                                      (64, 258, 5, 1, 500), (33, 130, 4, 120, 500), (20, 200, 6, 4, 500), (64, 256, 21, 4, 500),
                                                      (7, 173, 3, 172, 8)])
def test_persistent_recurrence_edge_shapes(N, A, L, min_len, video_dim):
    """The persistent recurrences at the edges of their eligibility (csrc/persist.hip: N <= 64 events split 32 + 32 over two half-chip
    machines, A <= 129 slots split 43 + 43 + 43 over three workgroups, D <= 512, any S): one event, a half machine with a single row, slot
    counts around the 43-slot thirds, the largest A, the smallest and the largest feature width, one and two decoder steps -- against the
    launch-per-phase path on the same seeded inputs, train mode."""
    from echr_amd import _lib
    lib = _lib.load()
    opt = synth.default_opt(vocab_size=300, seq_length=L - 2, video_dim=video_dim)
    params = synth.make_params(opt, seed=5)
    vid = synth.make_video(N, A, L, opt.CG_vocab_size + 1, seed=77 + N + A, min_len=min_len, video_dim=video_dim)
    runs = {}
    try:
        for name, v in (('launch', 0), ('persist', 1)):
            assert lib.echr_config_set(b'persist', v) == 0 and lib.echr_config_set(b'persist_bwd', v) == 0
            runs[name] = U.run_gpu(opt, params, vid, True)
    finally:
        lib.echr_config_set(b'persist', 1)
        lib.echr_config_set(b'persist_bwd', 1)
    p0, l0, g0, _ = runs['launch']
    p1, l1, g1, _ = runs['persist']
    assert np.isfinite(p1).all()
    assert np.abs(p0 - p1).max() < 2e-5 and abs(l0 - l1) < 1e-5 * abs(l0), np.abs(p0 - p1).max()
    for k in g0:
        if g0[k] is not None:
            if A == 1 and '.attention.' in k:
                # single-slot events: the attention weights are identically 1, the true gradients of ctx2att / h2att / alpha_net are
                # exactly zero and both paths only hold rounding noise of their (different) summation orders
                assert np.abs(g1[k]).max() < 1e-6 and np.abs(g0[k]).max() < 1e-6, k
            else:
                assert U.relerr(g1[k], g0[k], 1e-4) < 1e-4, (k, U.relerr(g1[k], g0[k], 1e-4))


@pytest.mark.gpu
def test_multinomial_sampling_distribution_and_reproducibility():
    """OldModel.sample with sample_max = 0 (OldModel_NEW.py:160-168): every step draws a token from softmax(logp / temperature).
    The random stream is the library's Philox, not torch.multinomial's, so the check is distributional: over 3000 seeds the first
    sampled token of each event follows the softmax of the <bos> step's log-probs (chi-square on the tokens with expected count >= 5,
    the rest pooled; 5-sigma bound), also at temperature 0.7; a fixed seed reproduces the whole decode bit for bit; a very low
    temperature reduces to the greedy decode; the emitted log-probs are the un-tempered log-softmax values of the sampled tokens."""
    opt, params, vid = synth.make_case('tiny')
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    lm = m.lm_model
    with torch.no_grad():
        video = m.get_video_context(tap, c3d, lda, vid['ind'], vid['soi'])
        event = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'])
        clip, cmask = m.get_clip_context(tap, c3d, lda, vid['ind'], vid['soi'])
        N = event.shape[0]
        logp0, _ = lm.get_logprobs_state(torch.zeros(N, dtype=torch.int64, device=dev), video, event, clip, cmask,
                                         lm.init_hidden(video, event, clip))
        logp0 = logp0.double().cpu().numpy()
        V1 = logp0.shape[1]
        greedy_seq, _ = lm.sample(video, event, clip, cmask, {'sample_max': 1})
        for temp in (1.0, 0.7):
            counts = np.zeros((N, V1))
            draws = 3000
            for s in range(draws):
                m.set_dropout_state(1000 + s)
                lm._sample_calls = 0
                seq, slp = lm.sample(video, event, clip, cmask, {'sample_max': 0, 'temperature': temp})
                first = seq[:, 0].cpu().numpy() if len(seq) else np.zeros(N, np.int64)
                # a draw of token 0 ends the caption at once: the sampler then returns nothing for rows that all finished
                counts[np.arange(N), first] += 1
                if s == 0 and len(seq):
                    tok = seq[:, 0].cpu().numpy()
                    assert np.abs(slp[:, 0].cpu().numpy() - logp0[np.arange(N), tok]).max() < 1e-4
            p = np.exp(logp0 / temp)
            p /= p.sum(1, keepdims=True)
            for n in range(N):
                exp_c = p[n] * draws
                big = exp_c >= 5
                chi = ((counts[n, big] - exp_c[big]) ** 2 / exp_c[big]).sum()
                dof = int(big.sum())
                if (~big).any():
                    e_rest, c_rest = exp_c[~big].sum(), counts[n, ~big].sum()
                    if e_rest > 0:
                        chi += (c_rest - e_rest) ** 2 / e_rest
                        dof += 1
                assert chi < dof + 5.0 * np.sqrt(2.0 * dof), (temp, n, chi, dof)
        m.set_dropout_state(77)
        lm._sample_calls = 0
        a_seq, a_lp = lm.sample(video, event, clip, cmask, {'sample_max': 0})
        m.set_dropout_state(77)
        lm._sample_calls = 0
        b_seq, b_lp = lm.sample(video, event, clip, cmask, {'sample_max': 0})
        assert torch.equal(a_seq, b_seq) and torch.equal(a_lp, b_lp)
        c_seq, _ = lm.sample(video, event, clip, cmask, {'sample_max': 0, 'temperature': 1e-3})
        assert torch.equal(c_seq, greedy_seq)


@pytest.mark.gpu
def test_sst_flat_arena_update_equals_per_tensor_update():
    """SST.build_arena(): gradients land in the flat arena (views adopted by autograd) and ClampAdam updates the whole proposal encoder
    in one launch; two optimiser steps equal the per-tensor path bit for bit (same kernels element-wise, no atomics in the SST)."""
    from echr_amd.optim import ClampAdam
    from echr_amd.misc.utils import clip_gradient
    g = U.gold('sst.npz')
    params = {k[len('param|'):]: v for k, v in g.items() if k.startswith('param|')}
    dev = torch.device('cuda')
    x = torch.from_numpy(g['x']).to(dev)
    out = {}
    for arena_on in (False, True):
        m, _ = _sst_module(params, dict(synth.CASES['tiny']['opt'], K=8), False)
        arena = m.build_arena() if arena_on else None
        o = ClampAdam(m.parameters(), lr=1e-3, arena=arena)
        for _ in range(2):
            o.zero_grad()
            tap, sc = m(x)
            ((tap * tap).sum() + sc.sum()).backward()
            if arena_on:
                assert arena.grads_in_arena()
            clip_gradient(o, 0.05)
            o.step()
        torch.cuda.synchronize()
        out[arena_on] = {k: p.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
    for k in out[False]:
        assert np.array_equal(out[False][k], out[True][k]), k

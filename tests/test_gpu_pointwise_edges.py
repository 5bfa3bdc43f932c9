"""The optimiser kernel and the small criterion ops of csrc/core.hip called directly (-m gpu), at the sizes where their index arithmetic
changes: the float4 body / scalar tail split and the second grid-stride pass of clamp_adam_kernel (the grid is capped at 4096 blocks of
256 threads), the four-rows-per-round loop of nll_loss_kernel, one-block reductions over N*T around 256 and 1024, tokens / targets in
column 0 and column V1 - 1.  Every reference is a few lines of float64 torch (or oracle.echr_ref_cpu.clamp_adam_step in float64) on the
same float32 inputs, computed on the CPU at run time.
"""
import numpy as np
import pytest
import torch

from tests import util as U

pytestmark = pytest.mark.gpu

TOL_LOSS = 1e-5     # relative (tests/test_gpu_parity.py)
CLIP = 100.0
BIG = 4 * 256 * 4096 + 4 * 1027 + 3          # float4 body: one full pass of the capped grid + 1027 quads of a second pass; scalar tail of 3
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1025, BIG]
NAN = float('nan')
# the head of every gradient buffer (cut to n): far above +clip, far below -clip, exactly +-clip, a zero gradient (on zero moments), a NaN
HEAD = [1.0e4, -1.0e4, CLIP, -CLIP, 0.0, NAN, 37.5]
I_ZERO, I_NAN = 4, 5


def _grad(n, rs, scale=80.0):
    """N(0, 80^2): about one element in five lies beyond +-100."""
    g = (scale * rs.standard_normal(n)).astype(np.float32)
    k = min(n, len(HEAD))
    g[:k] = np.asarray(HEAD[:k], np.float32)
    return g


def _adam_reference(p, gs, m, v, first_step, lr):
    """oracle.echr_ref_cpu.clamp_adam_step in float64 on the float32 inputs."""
    from oracle import echr_ref_cpu as O
    p, m, v = (torch.from_numpy(x).double() for x in (p, m, v))
    for i, g in enumerate(gs):
        O.clamp_adam_step(p, torch.from_numpy(g).double(), m, v, first_step + i, lr, clip=CLIP)
    return p.numpy(), m.numpy(), v.numpy()


def _check_adam(n, got, ref, p0):
    (p, m, v), (rp, rm, rv) = got, ref
    nan = np.zeros(n, bool)
    if n > I_NAN:
        nan[I_NAN] = True
    for a, r in ((p, rp), (m, rm), (v, rv)):
        assert np.array_equal(np.isnan(a), nan) and np.array_equal(np.isnan(r), nan)          # the NaN gradient poisons ITS element only
    ok = ~nan
    if n > I_ZERO:          # zero gradient on zero moments: 0 / (0 + eps) -- no update at all
        assert p[I_ZERO] == p0[I_ZERO] and m[I_ZERO] == 0.0 and v[I_ZERO] == 0.0
    if ok.any():
        assert np.abs(p[ok] - rp[ok]).max() < 2e-7, np.abs(p[ok] - rp[ok]).max()
        assert U.relerr(m[ok], rm[ok]) < 1e-6, U.relerr(m[ok], rm[ok])
        assert U.relerr(v[ok], rv[ok]) < 1e-6, U.relerr(v[ok], rv[ok])


@pytest.mark.parametrize('n', SIZES)
def test_clamp_adam_sizes_with_a_live_clamp(n):
    """Four steps from zero moments at lr 5e-5 (the gates of test_clamp_adam_matches_torch_adam: |dp| < 2e-7, moments 1e-6 of their max-norm),
    parameters in the model's own initialisation range (+-0.1, where one float32 rounding of p is 3.7e-9); `applied` counts the calls."""
    from echr_amd import functional as EF
    rs = np.random.RandomState(n % 9973)
    p0 = rs.uniform(-0.1, 0.1, n).astype(np.float32)
    gs = [_grad(n, rs) for _ in range(4)]
    if n >= 1023:
        share = float(np.mean(np.abs(np.stack(gs)[:, len(HEAD):]) > CLIP))
        assert 0.15 < share < 0.30, share          # the clamp is live on a sizeable share of the random elements
    p = torch.from_numpy(p0.copy()).cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    applied = torch.zeros(1, dtype=torch.int32, device='cuda')
    for i, g in enumerate(gs):
        EF.clamp_adam_(p, torch.from_numpy(g).cuda(), m, v, i + 1, 5e-5, 0.9, 0.999, 1e-8, CLIP, applied=applied)
    torch.cuda.synchronize()
    assert int(applied[0]) == 4
    ref = _adam_reference(p0.copy(), gs, np.zeros(n, np.float32), np.zeros(n, np.float32), 1, 5e-5)
    _check_adam(n, (p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()), ref, p0)
    if n > 3:          # the clamped elements really moved as a gradient of +-clip moves them: m = +-clip * (1 - 0.9^4)
        assert abs(ref[1][0] - CLIP * (1 - 0.9 ** 4)) < 1e-9 and abs(ref[1][1] + CLIP * (1 - 0.9 ** 4)) < 1e-9
        assert np.array_equal(m.cpu().numpy()[0:2], m.cpu().numpy()[2:4])          # far beyond the clip == exactly on it


def test_clamp_adam_late_step_from_nonzero_moments():
    """step = 100000: both bias corrections are 1 to float precision (lr / bc1 and 1 / sqrt(bc2) pass through unchanged)."""
    from echr_amd import functional as EF
    n = 1025
    rs = np.random.RandomState(5)
    p0 = rs.uniform(-0.1, 0.1, n).astype(np.float32)
    m0 = (20.0 * rs.standard_normal(n)).astype(np.float32)
    v0 = (400.0 * rs.uniform(0.1, 2.0, n)).astype(np.float32)
    g = _grad(n, rs)
    g[I_ZERO], g[I_NAN] = 12.5, -250.0          # (the zero-moment / NaN elements belong to the test above)
    p, m, v = (torch.from_numpy(x.copy()).cuda() for x in (p0, m0, v0))
    EF.clamp_adam_(p, torch.from_numpy(g).cuda(), m, v, 100000, 5e-5, 0.9, 0.999, 1e-8, CLIP)
    torch.cuda.synchronize()
    rp, rm, rv = _adam_reference(p0.copy(), [g], m0.copy(), v0.copy(), 100000, 5e-5)
    assert np.abs(p.cpu().numpy() - rp).max() < 2e-7
    assert U.relerr(m.cpu().numpy(), rm) < 1e-6 and U.relerr(v.cpu().numpy(), rv) < 1e-6
    assert np.abs(rp - p0).max() > 1e-5          # the update is there to be got wrong


@pytest.mark.parametrize('n', SIZES)
def test_clamp_is_bit_exact(n):
    """functional.clamp_ == torch.clamp on the CPU, bit for bit: NaN stays NaN, +-inf and everything beyond the clip land exactly on it, +-clip
    and -0.0 pass through."""
    from echr_amd import functional as EF
    rs = np.random.RandomState(n % 9973 + 1)
    x = (80.0 * rs.standard_normal(n)).astype(np.float32)
    head = np.asarray([NAN, np.inf, -np.inf, CLIP, -CLIP, -0.0, np.nextafter(np.float32(CLIP), np.float32(np.inf))], np.float32)
    k = min(n, len(head))
    x[:k] = head[:k]
    if n > 16:
        x[-3:] = np.asarray([-np.inf, NAN, 1.0e30], np.float32)          # the last elements of the last grid-stride pass
    want = torch.clamp(torch.from_numpy(x.copy()), -CLIP, CLIP).numpy()
    got = EF.clamp_(torch.from_numpy(x.copy()).cuda(), CLIP).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(x)) and np.array_equal(np.isnan(want), np.isnan(x))
    ok = ~np.isnan(x)
    assert np.array_equal(got[ok].view(np.int32), want[ok].view(np.int32))
    if n >= 1023:
        assert 0.15 < float(np.mean(np.abs(x[ok]) > CLIP)) < 0.30


# ---- MaskedNLL ---------------------------------------------------------------------------------------------------------------------

NLL_SHAPES = [(1, 1), (5, 51), (16, 16), (257, 1), (33, 31), (32, 32), (41, 25), (7, 293)]          # N*S = 1, 255, 256, 257, 1023, 1024, 1025, 2051
NLL_WIDTHS = [1, 3, 301, 2049]


def _nll_case(N, S, V1, seed, zero_mask=False):
    rs = np.random.RandomState(seed)
    logp = torch.log_softmax(torch.from_numpy(rs.standard_normal((N, S, V1))), 2).float()
    tgt = rs.randint(0, V1, size=(N, S)).astype(np.int64)
    msk = (rs.uniform(size=(N, S)) < 0.7).astype(np.float32)
    tgt.flat[0], tgt.flat[-1] = 0, V1 - 1                    # targets reach column 0 and column V1 - 1 (a single row: the last column) ...
    msk.flat[0], msk.flat[-1] = 1.0, 1.0                     # ... on rows that count
    if N * S > 2:
        msk.flat[1] = 0.0
        tgt.flat[1] = V1 - 1
    if zero_mask:
        msk[:] = 0.0
    return logp, torch.from_numpy(tgt), torch.from_numpy(msk)


def _nll_reference(logp, tgt, msk, g):
    x = logp.double().requires_grad_(True)
    loss = -(x.gather(2, tgt[:, :, None])[:, :, 0] * msk.double()).sum() / (msk.double().sum() + 1e-6)
    (loss * g).backward()
    return float(loss.detach()), x.grad.numpy()


def _nll_device(logp, tgt, msk, g, dtype):
    from echr_amd import functional as EF
    x = logp.cuda().requires_grad_(True)
    loss = EF.MaskedNLL.apply(x, tgt.to(dtype).cuda(), msk.cuda())
    (loss * g).backward()          # node = None: the backward is MaskedNLL.dense_grad
    torch.cuda.synchronize()
    return float(loss.detach()), x.grad.cpu().numpy()


def _check_nll(got, ref):
    (loss, grad), (rloss, rgrad) = got, ref
    assert abs(loss - rloss) <= TOL_LOSS * abs(rloss), (loss, rloss)
    zero = rgrad == 0
    assert not np.any(grad[zero])                                    # exact zeros off the targets and on masked rows
    assert np.all(np.abs(grad[~zero] - rgrad[~zero]) <= 1e-6 * np.abs(rgrad[~zero]))


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64], ids=['i32', 'i64'])
@pytest.mark.parametrize('N,S', NLL_SHAPES)
def test_masked_nll_forward_and_dense_grad(N, S, dtype):
    for V1 in NLL_WIDTHS:
        logp, tgt, msk = _nll_case(N, S, V1, seed=N * 1000 + S + V1)
        assert tgt.max() == V1 - 1 and (N * S == 1 or tgt.min() == 0) and (N * S <= 2 or (msk == 0).any())
        _check_nll(_nll_device(logp, tgt, msk, 0.75, dtype), _nll_reference(logp, tgt, msk, 0.75))


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64], ids=['i32', 'i64'])
def test_masked_nll_all_zero_mask(dtype):
    """0 / (0 + 1e-6): loss and gradient are zeros, not NaN."""
    logp, tgt, msk = _nll_case(33, 31, 301, seed=9, zero_mask=True)
    loss, grad = _nll_device(logp, tgt, msk, 0.75, dtype)
    rloss, rgrad = _nll_reference(logp, tgt, msk, 0.75)
    assert rloss == 0.0 and not np.any(rgrad)
    assert loss == 0.0 and np.isfinite(grad).all() and not np.any(grad)


# ---- GatherTokens ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,S,T,V1', [(1, 1, 1, 1), (51, 7, 5, 301), (16, 16, 16, 7), (257, 3, 1, 3), (5, 6, 6, 2049), (43, 9, 6, 300)])
def test_gather_tokens_is_pure_data_movement(N, S, T, V1):
    """Forward == torch.gather, backward == its scatter with the rows t >= T written as zeros -- bit for bit (N*T = 1, 255, 256, 257, 30, 258;
    T < S and T = S; tokens 0 and V1 - 1)."""
    from echr_amd import functional as EF
    rs = np.random.RandomState(N * 100 + T)
    logp = torch.from_numpy(rs.standard_normal((N, S, V1)).astype(np.float32))
    seq = torch.from_numpy(rs.randint(0, V1, size=(N, T)).astype(np.int64))
    seq.view(-1)[0], seq.view(-1)[-1] = V1 - 1, 0
    if N * T > 2:
        seq.view(-1)[1], seq.view(-1)[-2] = 0, V1 - 1
    g = torch.from_numpy(rs.standard_normal((N, T)).astype(np.float32))
    want = logp[:, :T].gather(2, seq[:, :, None])[:, :, 0]
    want_g = torch.zeros(N, S, V1)
    want_g[:, :T].scatter_(2, seq[:, :, None], g[:, :, None])
    x = logp.cuda().requires_grad_(True)
    out = EF.GatherTokens.apply(x, seq.cuda())
    # (the wrapper allocates d logp itself; a NaN-filled block of that size returned to the allocator just before makes it likely, not
    # certain, that the kernel's zeros land on NaNs -- the returned tensor is compared as a whole either way)
    junk = torch.full((N, S, V1), NAN, device='cuda')
    del junk
    out.backward(g.cuda())
    torch.cuda.synchronize()
    assert np.array_equal(out.detach().cpu().numpy().view(np.int32), want.numpy().view(np.int32))
    assert np.array_equal(x.grad.cpu().numpy().view(np.int32), want_g.numpy().view(np.int32))


# ---- RewardLoss --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,T', [(1, 1), (5, 51), (257, 1), (41, 25)])          # N*T = 1, 255, 257, 1025
def test_reward_loss_forward_and_backward(N, T):
    """sum(-input * reward * mask) / sum(mask), mask = [1 | seq > 0][:, :-1] (RewardLoss's docstring) in float64.  Sequences contain zeros
    (holes in the shifted mask), row 0 is zero from the start (only its first position counts), rewards have both signs.

    Forward gate: the terms are signed, so the error is measured against sum|term| / sum(mask): 17 float32 roundings deep (two products,
    at most 5 sequential adds per thread at N*T = 1025, 9 levels of the block sum, the division) -> 17 * 2^-24 = 1.0e-6.
    Backward: three roundings per element -> 1e-6 relative; exact zeros where the mask is zero."""
    from echr_amd import functional as EF
    rs = np.random.RandomState(N + T)
    x0 = (-3.0 * rs.uniform(0.1, 1.0, size=(N, T))).astype(np.float32)
    seq = rs.randint(0, 4, size=(N, T)).astype(np.int64)          # a quarter of the tokens are zeros
    seq[0, :] = 0
    reward = rs.uniform(-1.0, 1.0, size=(N, T)).astype(np.float32)
    mask = np.ones((N, T))
    mask[:, 1:] = seq[:, :-1] > 0
    assert mask[0].sum() == 1 and (T == 1 or ((mask == 0).any() and (mask[1:, 1:] == 1).any()))
    assert N * T == 1 or ((reward > 0).any() and (reward < 0).any())
    xr = torch.from_numpy(x0).double().requires_grad_(True)
    terms = -xr * torch.from_numpy(reward).double() * torch.from_numpy(mask)
    ref = terms.sum() / mask.sum()
    (ref * 0.75).backward()
    rg = xr.grad.numpy()
    x = torch.from_numpy(x0).cuda().requires_grad_(True)
    loss = EF.RewardLoss.apply(x, torch.from_numpy(seq).cuda(), torch.from_numpy(reward).cuda())
    (loss * 0.75).backward()
    torch.cuda.synchronize()
    scale = float(terms.detach().abs().sum() / mask.sum())
    assert abs(float(loss.detach()) - float(ref.detach())) <= 17 * 2.0 ** -24 * scale, (float(loss.detach()), float(ref.detach()))
    g = x.grad.cpu().numpy()
    assert not np.any(g[mask == 0])
    live = mask != 0
    assert np.all(np.abs(g[live] - rg[live]) <= 1e-6 * np.abs(rg[live]))

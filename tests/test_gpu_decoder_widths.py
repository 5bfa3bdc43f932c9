"""The decoders at every width their dimension rules admit (-m gpu): each width dispatch of the attention kernels, the slot counts, the
launch-per-phase recurrence tiles and the persistent kernels' zero padding against a FLOAT64 oracle (tests/width_ref.py; the conditions it
rests on are asserted on the CPU by tests/test_width_ref_host.py).

check_dims / att_check_dims admit every Ha, D in [4, 1024] and every H, E that are multiples of 4; persist_shape_ok admits every D in [8, 512]
at H = Ha = 512.  Every other test runs the widths of 'tiny' (D 20, Ha 24, H 32, E 16) or of ECHR (D 500 / 512 / 1012, Ha = H = E = 512).  The
cases here keep the event encoder, the vocabulary (V1 = 31) and the label width (L = 5) tiny and vary the decoder's widths alone, N = 3 events
of 1, 5 and 9 slots unless said, train mode with the injected dropout masks.

Route table (R = ceil(Ha / 256), RD = ceil(D / 256): att_score_kernel<R, SLOTS>, att_post_kernel<R>, att_bwd_kernel<R, RD, SLOTS>):

  A  launch-per-phase, H 32, E 16, att_slots 2        (Ha, D) -> (R, RD)
     (4, 4) (1,1)        (252, 260) (1,2)     (256, 516) (1,3)     (256, 772) (1,4)      (4, 1024) (1,4)
     (260, 124) (2,1)    (260, 500) (2,2)     (508, 768) (2,3)     (508, 1024) (2,4)
     (516, 132) (3,1)    (516, 260) (3,2)     (768, 516) (3,3)     (516, 772) (3,4)
     (772, 256) (4,1)    (1020, 500) (4,2)    (772, 516) (4,3)     (1024, 1024) (4,4)    (1020, 4) (4,1)
     D 124 / 132: one / two 128-column chunks of att_context_kernel; D = 4, Ha = 4: every clamped address is 0
  B  att_slots 2 / 4 / 8 x atomic / fixed order, D/Ha 20/24 (1,1) and 516/260 (2,3), 8 events of 1, 7, 8, 9, 31, 32, 33, 65 slots: the 8- /
     16- / 32-slot chunk of att_score / att_bwd / dq_fold, the 8-slot chunk of att_post, the 32-row step and A32 padding of att_context;
     'shared': 186 slots on 80 rows (atomic adds; dpall_fold under fixed order), 'disjoint': back to back (the plain-store form)
  C  rec_gemm_kernel / lstm_pointwise_*, D 20, Ha 24: (H, E) = (4, 4) (36, 20) (60, 16) (132, 132) (260, 4) -- 4H = 16, 144, 240, 528, 1040
     against the 64-wide tile, K = H against the 128-wide slice (a last slice of 4 at 132 and 260)
  D  H = Ha = 512, D = 8, 12, 124, 128, 132, 256, 260, 388, 508, 512 (E 16), D = 512 with E = 512, D = 12 and 512 with events of 130, 1, 44
     slots (BIG): persistent recurrences (launches counted: >= 2), launch-per-phase (persist = persist_bwd = 0: none counted), gemm_h2 = 0;
     the persistent sampler against the launch-per-step sampler and the float64 greedy decode
  E  the one-call step (FusedTrainStep, step=False, tap_grad=) on a_ha772_d516, c_h132_e132, d_d12
  F  the one-stream decoder (csrc/sat.hip, the same attention launches) at D/Ha 260/252 (1,2) and 772/516 (3,4); greedy decode and beam
     search (B = 3) at D/Ha/H/E 260/252/36/20 against the float64 greedy decode and the float64 host beam search
  G  refusals: Ha = 1028, D = 1028, D = 6, H = 34, E = 18

Gates: per judged quantity max(existing gate, 4 e_ref), e_ref = float32 oracle against float64 oracle (CPU, tools/parity_report.py --widths).
Over all 43 cases e_ref is at most 6.4e-7 on log-probs, 1.8e-7 on loss (relative), 2.3e-6 on the worst gradient tensor and 1.7e-6 on the worst
width slice, so 4 e_ref stays below every existing gate and the plain gates stand: 2e-5 absolute on log-probs, 1e-5 relative on loss, 1e-5 of
the max-norm on every gradient tensor (util.grad_close) and on every width slice -- the last float4 and the last, possibly partial, 256-wide
chunk of the Ha axis of d ctx2att / d h2att / d alpha_net and of the D axis of d ctx2att.weight and of the context columns of the input
weight that reads them, each relative to the slice's own max-norm.  Index outputs are exact where the float64 margin is at least 1e-4.
A last float4 that contributes nothing moves the float64 oracle by 4.9e-4 or more on log-probs and 0.29 or more of a tensor's max-norm
(tests/test_width_ref_host.py).

The gradient figure is width_ref.grad_err, the quantity util.grad_close judges: max |error| less its 1e-9 absolute allowance, over the tensor's
(slice's) max-norm.  The allowance matters for d h2att.weight of the H = 512 cases: with three events its max-norm is 2.5e-6 .. 2.9e-5, and a
plain max-norm ratio of that tensor runs to 2e-5 on every route (6e-5 on its last float4) while its absolute error stays below 1e-9.

Measured: e_ref on the CPU | the HIP path on an MI355X, worst of the routes of the case (their number in brackets): log-probs absolute, loss
relative, worst gradient tensor, worst width slice.

  case                    e_ref: logp    loss    grad   slice  |  HIP:  logp    loss    grad   slice
  a_ha4_d4               2.4e-07 1.7e-08 3.1e-07 3.1e-07  |  4.4e-07 5.3e-08 2.9e-07 1.4e-07  (1)
  a_ha252_d260           2.9e-07 1.1e-07 3.3e-07 3.3e-07  |  5.6e-07 2.3e-08 4.2e-07 8.9e-07  (1)
  a_ha256_d516           3.3e-07 4.4e-08 4.5e-07 4.5e-07  |  6.0e-07 9.4e-08 6.5e-07 6.1e-07  (1)
  a_ha256_d772           3.3e-07 7.7e-08 6.7e-07 1.1e-06  |  5.3e-07 8.2e-09 5.7e-07 8.5e-07  (1)
  a_ha260_d124           2.8e-07 8.8e-08 3.3e-07 2.1e-07  |  6.5e-07 2.0e-08 8.7e-07 6.9e-07  (1)
  a_ha260_d500           3.3e-07 4.3e-08 1.3e-06 1.3e-06  |  5.2e-07 2.6e-08 6.4e-07 6.1e-07  (1)
  a_ha508_d768           2.9e-07 5.1e-08 4.5e-07 4.7e-07  |  6.6e-07 8.7e-08 6.3e-07 1.0e-06  (1)
  a_ha508_d1024          3.8e-07 1.1e-08 5.2e-07 5.5e-07  |  8.3e-07 8.0e-08 5.4e-07 6.2e-07  (1)
  a_ha516_d132           3.2e-07 3.7e-09 3.2e-07 3.2e-07  |  6.0e-07 3.7e-09 3.7e-07 5.5e-07  (1)
  a_ha516_d260           3.5e-07 4.9e-08 4.3e-07 2.1e-07  |  7.3e-07 2.1e-08 4.4e-07 3.3e-07  (1)
  a_ha768_d516           3.1e-07 1.1e-08 3.6e-07 4.6e-07  |  6.1e-07 1.1e-08 1.0e-06 8.9e-07  (1)
  a_ha516_d772           3.0e-07 3.3e-08 3.2e-07 1.2e-06  |  7.5e-07 1.1e-07 6.3e-07 1.5e-06  (1)
  a_ha772_d256           2.6e-07 1.8e-07 4.9e-07 2.3e-07  |  5.3e-07 4.0e-08 4.2e-07 4.2e-07  (1)
  a_ha1020_d500          2.7e-07 8.5e-08 5.3e-07 4.8e-07  |  5.8e-07 5.4e-08 6.9e-07 5.3e-07  (1)
  a_ha772_d516           2.9e-07 5.2e-08 5.4e-07 5.2e-07  |  5.6e-07 5.2e-08 5.7e-07 4.1e-07  (2: module path, one-call)
  a_ha1024_d1024         3.7e-07 6.0e-08 6.6e-07 7.3e-07  |  5.4e-07 6.0e-08 1.1e-06 1.2e-06  (1)
  a_ha1020_d4            2.7e-07 4.7e-08 2.1e-07 8.9e-08  |  4.1e-07 9.2e-08 2.4e-07 1.2e-07  (1)
  a_ha4_d1024            2.8e-07 7.1e-08 1.1e-06 1.4e-06  |  5.7e-07 6.1e-08 2.8e-06 2.8e-06  (1)
  b_d20_ha24_shared      2.8e-07 7.0e-08 1.3e-07 1.3e-07  |  5.9e-07 8.5e-10 1.9e-07 2.1e-07  (6: att_slots x accumulation mode)
  b_d20_ha24_disjoint    3.1e-07 8.2e-08 1.7e-07 1.7e-07  |  5.8e-07 1.5e-07 1.9e-07 1.2e-07  (6)
  b_d516_ha260_shared    3.5e-07 1.7e-08 6.0e-07 2.8e-07  |  6.1e-07 1.2e-07 5.1e-07 4.4e-07  (6)
  b_d516_ha260_disjoint  6.1e-07 3.0e-08 1.2e-06 1.2e-06  |  6.9e-07 1.0e-07 1.0e-06 9.7e-07  (6)
  c_h4_e4                2.7e-07 9.5e-08 1.7e-07 6.0e-08  |  7.3e-07 1.1e-07 4.6e-07 4.6e-07  (1)
  c_h8_e8                2.6e-07 2.6e-08 1.9e-07 1.5e-07  |  5.6e-07 9.5e-08 2.7e-07 2.3e-07  (1)
  c_h12_e12              2.5e-07 4.6e-08 1.9e-07 4.0e-07  |  6.3e-07 9.3e-08 3.6e-07 1.0e-06  (1)
  c_h36_e20              2.6e-07 4.9e-09 1.9e-07 1.9e-07  |  6.1e-07 6.4e-08 4.0e-07 2.7e-07  (1)
  c_h60_e16              2.4e-07 3.6e-08 2.5e-07 1.4e-07  |  5.6e-07 1.0e-07 2.1e-07 2.8e-07  (1)
  c_h132_e132            2.5e-07 1.1e-07 4.9e-07 4.7e-07  |  5.3e-07 1.1e-07 4.2e-07 4.2e-07  (2: module path, one-call)
  c_h260_e4              2.4e-07 1.7e-08 1.9e-07 2.1e-07  |  5.0e-07 1.8e-08 3.3e-07 1.7e-07  (1)
  d_d8                   2.5e-07 8.7e-09 2.6e-07 1.5e-07  |  7.5e-07 8.7e-09 8.7e-07 1.9e-07  (3: persistent, launch, gemm_h2 = 0)
  d_d12                  2.6e-07 6.6e-08 4.5e-07 4.5e-07  |  7.1e-07 7.5e-08 1.9e-06 4.4e-07  (4: those and one-call)
  d_d124                 2.8e-07 2.5e-08 5.4e-07 5.4e-07  |  8.8e-07 4.4e-08 9.8e-07 4.2e-07  (3)
  d_d128                 3.1e-07 7.0e-08 3.5e-07 5.8e-07  |  8.0e-07 1.4e-07 1.0e-06 5.1e-07  (3)
  d_d132                 4.1e-07 1.3e-08 3.9e-07 3.9e-07  |  8.3e-07 8.3e-08 1.0e-06 5.3e-07  (3)
  d_d256                 3.8e-07 2.9e-08 3.7e-07 5.2e-07  |  8.2e-07 1.1e-07 1.2e-06 4.7e-07  (3)
  d_d260                 3.9e-07 1.0e-07 5.4e-07 2.9e-07  |  7.4e-07 1.1e-07 6.0e-07 4.5e-07  (3)
  d_d388                 5.0e-07 1.7e-09 3.3e-07 3.7e-07  |  9.9e-07 7.0e-08 1.6e-06 6.6e-07  (3)
  d_d508                 5.0e-07 2.6e-08 4.2e-07 5.0e-07  |  8.6e-07 2.6e-08 1.5e-06 5.7e-07  (3)
  d_d512                 3.8e-07 4.1e-08 4.6e-07 4.3e-07  |  8.9e-07 4.1e-08 1.0e-06 6.8e-07  (3)
  d_d512_e512            4.3e-07 5.5e-08 4.0e-07 4.0e-07  |  8.5e-07 8.3e-08 1.1e-06 9.4e-07  (3)
  d_d12_big              2.4e-07 2.1e-08 3.1e-07 3.4e-07  |  6.7e-07 1.2e-07 1.7e-06 1.2e-06  (3)
  d_d512_big             6.4e-07 2.2e-08 4.0e-07 3.7e-07  |  1.9e-06 2.2e-08 1.2e-06 5.9e-07  (3)
  f_sat_d260_ha252       2.7e-07 2.5e-08 5.4e-07 5.4e-07  |  5.1e-07 4.5e-08 4.7e-07 4.7e-07  (1)
  f_sat_d772_ha516       3.1e-07 6.1e-08 4.5e-07 5.0e-07  |  5.1e-07 8.0e-08 8.2e-07 4.8e-07  (1)
  f_dec_d260_ha252       2.6e-07 8.2e-08 5.5e-07 5.5e-07  |  decoding only: 9 of 9 greedy picks and 3 of 3 beam events inside the margin rule, all equal

The HIP path stays within 6x of the float32 oracle's own rounding of the same case at every width (largest figure: 2.8e-6 on the last float4
of the D axis of d ctx2att.weight at Ha = 4, D = 1024, where e_ref is 1.4e-6) and a factor of 3.5 or more inside every gate.  The persistent route counts 2 persistent launches at every
D, the launch route none.  The persistent sampler equals the launch-per-step sampler on all 13 cases; 5 to 9 of the 9 picks of a case lie inside
the margin rule and equal the float64 decode.

One defect found: H = 4 and H = 8 passed check_dims and failed in echr_decoder_bwd with "gemm_grouped: problems sharing C need auto split-K
(accumulate mode) and K > 32" -- the three d XT products share their output and contract over K = 4H, one k tile of 32 there.  bwd now runs
them one behind the other at 4H <= 32 (csrc/decoder.hip), and c_h4_e4 / c_h8_e8 / c_h12_e12 stand on both sides of that switch.

Sensitivity (scratch builds, arithmetic altered only, memory accesses unchanged; 113 cases).
 1. att_score_kernel without the zeroing of alpha on the duplicated lanes (a doubled last float4): every case whose Ha is no multiple of 256 on
    a launch-per-phase forward fails -- 14 of A (a_ha256_d516, a_ha256_d772, a_ha768_d516, a_ha1024_d1024 pass), all of B, C, E, F and the
    refusal follow-ups; Ha = 512 (group D) passes.
 2. The training forward of the persistent kernel adding the context columns d < D - 4 only (a dropped last float4 of D): all 26 persistent
    and gemm_h2 = 0 cases of D and the one-call d_d12 fail; the 13 launch cases and the 13 sampler cases pass.
 3. att_bwd_kernel forming clip . d ATT over j + 4 < D only: all of A, B, C, the 13 launch cases of D, the two non-persistent one-call cases and
    both one-stream cases fail on gradients alone; the persistent routes and the decoding tests pass.
 4. The persistent sampler storing the context columns d < D - 4 only: all 13 sampler cases fail, nothing else.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util as U
from tests import width_ref as W

pytestmark = pytest.mark.gpu

DEFAULTS = (('persist', 1), ('persist_bwd', 1), ('persist_sample', 1), ('gemm_h2', 1), ('att_slots', 2), ('deterministic', 0))
ROUTES_D = {
    'persistent': (),
    'launch': (('persist', 0), ('persist_bwd', 0)),
    'fp32gemm': (('gemm_h2', 0),),
}


def _lib():
    from echr_amd import _lib as L
    return L, L.load()


def _config(pairs):
    L, lib = _lib()
    for k, v in pairs:
        L.check(lib.echr_config_set(k.encode(), int(v)), 'config_set')


def _drain():
    _, lib = _lib()
    torch.cuda.synchronize()
    while lib.echr_check_async() != 0:
        pass


def _clean():
    _, lib = _lib()
    torch.cuda.synchronize()
    rc = lib.echr_check_async()
    if rc != 0:
        msg = lib.echr_last_error()
        _drain()
        raise AssertionError((rc, msg))


def _dev():
    return torch.device('cuda')


def _feats(vid, tap_grad=False):
    tap, c3d, lda = (torch.from_numpy(np.ascontiguousarray(vid[k])).to(_dev()) for k in ('tap', 'c3d', 'lda'))
    return tap.requires_grad_(tap_grad), c3d, lda


def _param_grads(m):
    return {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}


def _forward_backward(opt, params, vid, train=True):
    from echr_amd.misc.utils import LanguageModelCriterion
    m = U.build_gpu_model(opt, params, train)
    tap, c3d, lda = _feats(vid, True)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    pred = m(tap, c3d, lda, labels, vid['ind'], vid['soi'], mode='train')
    loss = LanguageModelCriterion()(pred, labels[:, 1:].to(_dev()), masks[:, 1:].to(_dev()))
    loss.backward()
    torch.cuda.synchronize()
    grads = _param_grads(m)
    grads['tap_feats'] = tap.grad.cpu().numpy() if tap.grad is not None else np.zeros(tuple(tap.shape), np.float32)
    return dict(logp=pred.detach().cpu().numpy(), loss=float(loss.detach()), grads=grads)


def module_pass(name, route, train=True):
    """CaptionGenerator(mode='train') + criterion + backward under the switches `route`: dict(logp, loss, grads), d tap_feats among the grads."""
    opt, params, vid = W.case(name)
    try:
        _config(route)
        got = _forward_backward(opt, params, vid, train)
    finally:
        _config(DEFAULTS)
    _clean()
    return got


def _check(name, got, what):
    ref = W.oracle(name)
    opt = W.case(name)[0]
    tl, ts, tg, tsl = W.gates(name)
    e = W.errors(got, ref, opt)
    print('%s %s: logp %.2e (gate %.1e) loss %.2e (gate %.1e) grad %.2e (%s, gate %.1e) slice %.2e (%s, gate %.1e)'
          % (name, what, e[0], tl, e[1], ts, e[2], e[3], tg, e[4], e[5], tsl))
    assert got['logp'] is None or np.isfinite(got['logp']).all(), what
    assert np.isfinite(got['loss']) and all(v is None or np.isfinite(v).all() for v in got['grads'].values()), what
    assert e[0] < tl, (what, e[0])
    assert e[1] < ts, (what, got['loss'], ref['loss'])
    miss = W.grads_close(got['grads'], ref['grads'], opt, tg, tsl)
    assert not miss, (what, miss)


def _same_bits(a, b):
    assert np.array_equal(a['logp'], b['logp']) and a['loss'] == b['loss']
    for k, g in a['grads'].items():
        assert (g is None and b['grads'][k] is None) or np.array_equal(g, b['grads'][k]), k


# ---- A. attention widths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', W.GROUP['A'])
def test_attention_widths_vs_float64_oracle(name):
    """Every (R, RD) instantiation of att_score / att_bwd / att_post and att_context's column chunks on the launch-per-phase path."""
    _check(name, module_pass(name, ()), 'R %d RD %d' % W.dispatch(W.CASES[name]))


# ---- B. slots, chunk edges, fixed order ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('deterministic', [0, 1])
@pytest.mark.parametrize('slots', W.SLOTS)
@pytest.mark.parametrize('name', W.GROUP['B'])
def test_slot_counts_and_chunk_edges_vs_float64_oracle(name, slots, deterministic):
    """att_slots 2 / 4 / 8 with atomic and fixed-order accumulation, events of 1 .. 65 slots on shared and on disjoint rows; under fixed order
    two runs agree bit for bit."""
    route = (('att_slots', slots), ('deterministic', deterministic))
    got = module_pass(name, route)
    _check(name, got, 'att_slots %d deterministic %d' % (slots, deterministic))
    if deterministic:
        _same_bits(got, module_pass(name, route))


# ---- C. LSTM widths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', W.GROUP['C'])
def test_recurrence_widths_vs_float64_oracle(name):
    """rec_gemm_kernel's 64-wide Nout tiles and 128-wide k slices, lstm_pointwise_* at H = 4 .. 260."""
    c = W.CASES[name]
    _check(name, module_pass(name, ()), 'H %d E %d' % (c['H'], c['E']))


# ---- D. persistent recurrences ----------------------------------------------------------------------------------------------------------
def _persist_launches(fn):
    L, lib = _lib()
    L.check(lib.echr_prof_enable(1), 'prof_enable')
    try:
        out = fn()
        torch.cuda.synchronize()
        ms, fl, by, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        L.check(lib.echr_prof_read(9, C.byref(ms), C.byref(fl), C.byref(by), C.byref(n)), 'prof_read')
    finally:
        L.check(lib.echr_prof_enable(0), 'prof_enable')
    return out, int(n.value)


@pytest.mark.parametrize('route', list(ROUTES_D))
@pytest.mark.parametrize('name', W.GROUP['D'])
def test_persistent_widths_vs_float64_oracle(name, route):
    """H = Ha = 512 at every D the persistent kernels pad, on the persistent route (its launches counted), launch-per-phase and with the
    exact-fp32 GEMMs."""
    got, launches = _persist_launches(lambda: module_pass(name, ROUTES_D[route]))
    print(name, route, 'persistent launches', launches)
    if route == 'persistent':
        assert launches >= 2, launches
    if route == 'launch':
        assert launches == 0, launches
    _check(name, got, route)


def _greedy_gpu(name, persist_sample):
    opt, params, vid = W.case(name)
    m = U.build_gpu_model(opt, params, False)
    try:
        _config([('persist_sample', persist_sample)])
        with torch.no_grad():
            seq, lp = m(*_feats(vid), [], vid['ind'], vid['soi'], mode='eval')
    finally:
        _config(DEFAULTS)
    _clean()
    if len(seq) == 0:
        n = len(vid['ind'])
        return np.zeros((n, 0), np.int64), np.zeros((n, 0), np.float32)
    return seq.cpu().numpy(), lp.cpu().numpy()


def _check_greedy_vs_float64(name, seq, lp):
    """The margin rule: a row is compared up to (not including) its first live pick whose float64 top-1 / top-2 margin is below W.MARGIN."""
    from tests import decoder_regime_ref as D
    rseq, rlp, margin, live = D.greedy64_of(*W.case(name))
    T = min(seq.shape[1], rseq.shape[1])
    checked = 0
    for n in range(rseq.shape[0]):
        for t in range(T):
            if not live[n, t] or margin[n, t] < W.MARGIN:
                break
            assert seq[n, t] == rseq[n, t], (name, n, t)
            assert abs(lp[n, t] - rlp[n, t]) < W.TOL_LOGP, (name, n, t, lp[n, t], rlp[n, t])
            checked += 1
    if bool((margin[live] >= W.MARGIN).all()):
        assert seq.shape == rseq.shape and np.array_equal(seq, rseq)
    return checked


@pytest.mark.parametrize('name', W.GROUP['D'])
def test_persistent_sampler_widths_vs_launch_per_step(name):
    """Greedy decoding as one persistent launch against the launch-per-step form -- same sequences, log-probs to rounding -- and both against
    the float64 greedy decode under the margin rule."""
    outs = [_greedy_gpu(name, flag) for flag in (1, 0)]
    assert outs[0][0].shape == outs[1][0].shape and outs[0][0].shape[0] == 3
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.isfinite(outs[0][1]).all() and np.abs(outs[0][1] - outs[1][1]).max(initial=0.0) < W.TOL_LOGP
    checked = [_check_greedy_vs_float64(name, seq, lp) for seq, lp in outs]
    print(name, 'picks checked against float64:', checked)


# ---- E. the one-call path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', W.ONE_CALL)
def test_one_call_step_vs_float64_oracle(name):
    """fused.FusedTrainStep (echr_train_step) with step=False and tap_grad=: the loss, every gradient and d tap_feats."""
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    opt, params, vid = W.case(name)
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
    f = FusedTrainStep(m, o, grad_clip=None)
    tap, c3d, lda = _feats(vid)
    labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
    g_tap = torch.zeros_like(tap)
    loss = float(f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], step=False, tap_grad=g_tap))
    _clean()
    grads = _param_grads(m)
    grads['tap_feats'] = g_tap.cpu().numpy()
    _check(name, dict(logp=None, loss=loss, grads=grads), 'one-call')


# ---- F. the other consumers of the same launches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [k for k in W.GROUP['F'] if W.is_sat(k)])
def test_one_stream_decoder_widths_vs_float64(name):
    """caption_model='show_attend_tell' (csrc/sat.hip) through the same attention launches, against tests/sat_ref.py in float64."""
    _check(name, module_pass(name, ()), 'one-stream R %d RD %d' % W.dispatch(W.CASES[name]))


DECODED = 'f_dec_d260_ha252'


def test_greedy_decode_widths_vs_float64():
    seq, lp = _greedy_gpu(DECODED, 1)
    checked = _check_greedy_vs_float64(DECODED, seq, lp)
    print(DECODED, 'greedy picks checked against float64:', checked)
    assert checked >= 1


def test_beam_search_widths_vs_float64_host_beam():
    """echr_decoder_beam at B = 3 against the host beam search (tests/beam_ref.py) over the float64 oracle, under the margin rule of
    tests/test_gpu_beam.py: sequences of the gated events exact, their log-probs within the gate, and every event's score equal to the
    oracle's re-score of the device's own hypothesis."""
    from oracle import echr_ref_cpu as O
    from tests import beam_ref
    from tests import decoder_regime_ref as D
    from tests import test_gpu_beam as TB
    B = 3
    opt, params, vid = W.case(DECODED)
    P, video, event, cl, mask = D.contexts64(opt, params, vid)
    with torch.no_grad():
        state0 = O.init_hidden(P, video, event, cl, opt.CG_init_feats_type)
    step, rep_state = beam_ref.oracle_step(P, video, event, cl, mask, B)
    ref = beam_ref.beam_search(step, rep_state(state0), event.shape[0], B, opt.CG_seq_length)
    m = U.build_gpu_model(opt, params, False)
    seq, lp, score = TB._beam(m, TB._contexts(m, vid, vid['soi'], vid['ind']), B)
    _clean()
    L = opt.CG_seq_length
    gated = ref['margin'] >= W.MARGIN
    print(DECODED, 'beam: gated events', int(gated.sum()), 'of', len(gated), 'margins', ref['margin'])
    assert np.array_equal(TB._pad(seq, L)[gated], TB._pad(ref['seq'], L)[gated])
    step1, _ = beam_ref.oracle_step(P, video, event, cl, mask, 1)
    resc, words = beam_ref.rescore(step1, state0, seq, L)
    assert np.all(np.abs(score - resc) <= TB.TOL_SCORE * np.maximum(np.abs(resc), 1.0)), np.abs(score - resc).max()
    T = seq.shape[1]
    for n in np.nonzero(gated)[0]:
        k = min(int(words[n]) + 1, T)
        assert np.abs(lp[n, :k] - ref['logp'][n, :k]).max(initial=0.0) < W.TOL_LOGP
        assert not lp[n, k:].any()


# ---- G. refusals --------------------------------------------------------------------------------------------------------------------------
REFUSED = {
    'Ha=1028': dict(CG_att_hid_size=1028),
    'D=1028': dict(video_dim=1028),
    'D=6': dict(video_dim=6),
    'H=34': dict(CG_rnn_size=34),
    'E=18': dict(CG_input_encoding_size=18),
}


@pytest.mark.parametrize('what', list(REFUSED))
def test_widths_outside_the_rules_are_refused_loudly(what):
    """A width outside check_dims raises EchrHipError that names the rule and the offending value; the next valid call on the same model class
    succeeds and no asynchronous report is left behind."""
    from echr_amd import synth
    from echr_amd._lib import EchrHipError
    _, lib = _lib()
    base = W.case('b_d20_ha24_shared')[0]
    over = dict(W.ENCODER, video_dim=base.video_dim, CG_att_hid_size=base.CG_att_hid_size, CG_rnn_size=base.CG_rnn_size,
                CG_input_encoding_size=base.CG_input_encoding_size, CG_vocab_size=W.V1 - 1, CG_seq_length=W.L - 2)
    over.update(REFUSED[what])
    opt = synth.default_opt(**over)
    params = synth.make_params(opt, W.PARAM_SEED)
    vid = synth.make_video(N=3, A=9, L=W.L, V1=W.V1, seed=7, T_v=16, video_dim=opt.video_dim, hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
    with pytest.raises(EchrHipError) as e:
        _forward_backward(opt, params, vid)
    _drain()
    msg = str(e.value)
    print(what, '->', msg)
    rule = 'H%4==0 and E%4==0' if what.split('=')[0] in ('H', 'E') else 'D%4==0, Ha%4==0, 4 <= D,Ha <= 1024'
    assert rule in msg and what in msg, msg
    _check('a_ha4_d4', module_pass('a_ha4_d4', ()), 'after the refusal of ' + what)
    assert lib.echr_check_async() == 0

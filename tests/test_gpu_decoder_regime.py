"""The decoder's three LSTM streams at TRAINED-WEIGHT scales (-m gpu): every route of the recurrences against a FLOAT64 oracle.

Every other decoder case draws layer{0,1,2}.weight_* in +-1/sqrt(512), the embedding in +-0.1 and C3D rows from N(0, 1): gate pre-activations
stay below 1.1, cell states below 0.7, |C3D| below 4.  The variants of synth.make_decsat leave that regime by scaling only (ECHR widths,
vocabulary 300, N = 12, A = 40, 6 steps unless said; tests/test_decoder_regime_host.py asserts each reach on the float64 oracle):
  gates_sat      embed x10, weight_ih x16, weight_hh x12, forget bias +1: 16-20% of the pre-activations beyond +-8, the largest 26-29 (the
                 float32 sigmoid is exactly 1 beyond 17) -- fast_sigmoid / fast_tanh of csrc/persist.hip lstm_cell and csrc/decoder.hip
                 lstm_pointwise_* far outside their linear part, g (1 - g) and 1 - tc^2 of cg1 at rounding
  gates_sat70    the same over 70 events: more than 64 rows take the launch-per-phase recurrences in training and the chain sampler in decoding
  gates_sat_vb   the same over a 3-video batch (14 events): the *_batch entries
  drift          embed x10, ih x4, hh x2, forget +8, input gate +3, 20 steps: max |c| 19, 5-8% of the cell states beyond 9
  feat_wide      C3D row r times 2^e_r, e_r in [-8, 6], ctx2att.weight x 2^-6: max |C3D| 216 where it was 4, so the per-event bound XCMAX behind
                 the fp32 -> fp16-pair conversion factor 2^(12 - ex) / ssum of the attended context is 2^8 where it was 2^2 or 2^3; event 0 is
                 all zero (bound 0), event 1's largest |element| is exactly a power of two (the ex boundary), event 2 is the ONE row with the
                 video's largest element: its context is that row, 216, and overflows fp16 under the factor of any bound below 2^5
  feat_wide_big  the same on events of 130, 258, 100, 173, ... segments (BIG instantiation).  The 130-, 258- and 173-long events are quiet (|element|
                 < 0.3) but for one element of 4096 in slot 129 (first of the second slot set) / the last slot / slot 129: |context| = 16 .. 32
                 at every step, which overflows fp16 under the factor of a maximum that misses that slot; 16384 stands in the row just past
                 the 100-long event and must not enter its bound

Gates.  e_ref = float32 oracle against float64 oracle on the same inputs (CPU; tools/parity_report.py --decsat prints it), the larger of eval and
train mode: log-probs absolute, loss relative, worst gradient tensor relative to its max-norm, worst GATE SLICE [i | f | g | o] of an LSTM tensor
relative to the slice's own max-norm (in drift one slice dominates the tensor's norm).  The HIP path against float64 is held to max(existing gate,
4 e_ref) per quantity -- 4x: the other summation order and the 1-ulp hardware exp / rcp -- and never above the 1e-4 contract for log-probs and
loss.  gates_sat70 is the one place where the cap binds: over 70 saturated events the float32 reference itself costs 3.1e-5 (log-probs of -50
have an ulp of 3.8e-6), its log-prob gate is the contract, 3.2 e_ref.  (e_ref follows the host's BLAS summation order: a second host measured
gates_sat 3.1e-5 / 9.8e-8 / 2.3e-5 / 2.3e-5 and feat_wide's gate slice 2.8e-5.  The table keeps the smaller figures, so the gates are the stricter.)

  variant         e_ref: logp     loss     grad    slice   |  HIP path measured, worst of eval and train: logp / loss / grad / slice
  gates_sat            1.9e-5   4.6e-8   8.8e-6   1.3e-5   |  h2pair 2.9e-5 / 4.6e-8 / 1.0e-5 / 1.3e-5   fp32 2.4e-5 / 3.1e-8 / 9.7e-6 / 1.1e-5   launch 2.1e-5 / 3.1e-8 / 1.0e-5 / 1.1e-5
  drift                5.5e-6   7.0e-8   2.6e-6   8.6e-6   |  h2pair 6.9e-6 / 7.0e-8 / 4.0e-6 / 8.4e-6   fp32 7.1e-6 / 7.0e-8 / 4.0e-6 / 8.5e-6   launch 6.5e-6 / 7.0e-8 / 4.2e-6 / 8.5e-6
  feat_wide            8.8e-6   7.1e-8   1.4e-5   1.1e-5   |  h2pair 7.1e-6 / 9.6e-9 / 1.4e-5 / 1.6e-5   fp32 9.9e-6 / 9.6e-9 / 1.2e-5 / 1.2e-5   launch 8.7e-6 / 9.6e-9 / 1.3e-5 / 1.3e-5
  feat_wide_big        1.1e-6   4.7e-8   1.9e-6   1.5e-6   |  h2pair 1.6e-6 / 4.7e-8 / 1.2e-6 / 1.4e-6   fp32 1.2e-6 / 4.3e-8 / 1.3e-6 / 1.4e-6   launch 1.6e-6 / 4.7e-8 / 1.3e-6 / 6.1e-7
  gates_sat70          3.1e-5   6.0e-8   1.2e-5   1.9e-5   |  launch 2.4e-5 / 5.0e-8 / 8.5e-6 / 8.5e-6
  gates_sat_vb         1.5e-5   3.9e-8   1.0e-5   1.1e-5   |  forward_batch 1.7e-5 / 6.1e-8 / 1.6e-5 / 2.2e-5   batch step - / 6.1e-8 / 1.6e-5 / 2.2e-5

(h2pair: persistent recurrences on fp16 pairs; fp32: persist_h2 = 0; launch: persist = persist_bwd = 0.)  The one-call path stays at the module
path's figures except feat_wide in fixed-order mode: 3.6e-5 on layer0.weight_hh[g] (gate 4.4e-5; 1.0e-5 in atomic mode), the same bits every run.
Greedy decoding: every token and finish step equal on both routes of all five variants; sampled log-probs within 1.1e-5 (gates_sat, gates_sat70),
3.0e-6 (feat_wide), 2.1e-6 (drift), 9.2e-7 (feat_wide_big).  The single step from drift's state: log-probs 5.2e-6, h' 6.1e-7, c' 2.7e-6 (e_ref
1.4e-6 / 4.1e-7 / 2.7e-6).  No defect: the HIP path sits within 1.5x of the reference's own rounding on every route (3.3x on the one
fixed-order tensor above).

Sensitivity (scratch builds, arithmetic altered only; 45 cases).
 1. Arguments of fast_sigmoid clamped at +-8 in persist.hip's lstm_cell: 26 fail -- every persistent (h2pair, fp32) module-path case of gates_sat,
    drift and feat_wide, their atomic one-call cases, all three batch cases, all four fixture cases, and greedy decoding of gates_sat, drift,
    feat_wide, gates_sat70 (the persistent sampler).  Every launch route, fixed-order mode (it takes the launch recurrences), gates_sat70's module
    path and feat_wide_big (no pre-activation beyond 5) pass.
 2. The new cell state clamped at +-8 in persist.hip's lstm_cell: 10 fail -- drift on h2pair and fp32 (eval and train), drift's atomic one-call
    and fixture cases, greedy decoding of drift, gates_sat and gates_sat70 (19 steps walk |c| past 8 there too); no launch route.  The same clamp in
    decoder.hip's lstm_pointwise_fwd_kernel: 7 fail -- drift on the launch route (eval and train), its fixed-order one-call case, the launch-per-step
    decode of the same three variants, and the single step from the drifted state; no persistent route.
 3. H2_SA raised to 2^15: non-finite gradients / loss in train mode on feat_wide h2pair (module path and atomic one-call) and on gates_sat_vb
    (forward_batch and the batch step); eval mode and every fp32 / launch route pass.  gates_sat itself stays finite: over its 6 steps h = go
    tanh(c) * 2 passes 65520 / 2^15 = 1.99951 only at the last step, whose h feeds no recurrence (gates_sat_vb runs 7 steps; in feat_wide the
    single-row event saturates stream 1 at once).  So the scale's headroom is what the comment claims, a factor of 8, and 2^15 is visible.
 4. The context bound replaced by ex = 3: feat_wide fails on h2pair (eval, train, atomic one-call: non-finite) and on no other route.  The second
    slot set skipped in the BIG maximum: feat_wide_big fails on h2pair (eval and train) and on no other route.  (Both were INVISIBLE on a first
    construction that scaled the rows alone: the attended context is an average and stayed 16x and more below the event's bound, so any bound
    within four binades left hi finite and a smaller one only added precision.  The planted single-row event and the quiet events with one
    element of 4096 are what makes a wrong bound overflow; tests/test_decoder_regime_host.py asserts that on the float64 oracle.)
    The exponent boundary (event 1 of feat_wide, largest element exactly 128) cannot be made visible: the conversion leaves four binades of
    headroom, an ex that is one too small still gives a finite hi.  The same holds for the row past an event's end entering the bound (a larger
    bound seven binades too large costs seven bits of a 22-bit pair).
"""
import numpy as np
import pytest
import torch

from echr_amd import synth
from tests import decoder_regime_ref as D
from tests import util as U

pytestmark = pytest.mark.gpu

TOL_LOGP, TOL_LOSS, TOL_GRAD = 2e-5, 1e-5, 1e-5          # the existing gates (tests/test_gpu_parity.py)
CONTRACT = 1e-4
# e_ref (logp absolute, loss relative, worst gradient tensor, worst LSTM gate slice -- relative to the max-norm): float32 oracle vs float64
# oracle on the CPU, the larger of eval and train mode (tools/parity_report.py --decsat; tests/test_decoder_regime_host.py re-measures it)
E_REF = {
    'gates_sat': (1.93e-5, 4.6e-8, 8.8e-6, 1.25e-5),
    'drift': (5.5e-6, 7.0e-8, 2.6e-6, 8.6e-6),
    'feat_wide': (8.8e-6, 7.1e-8, 1.38e-5, 1.1e-5),
    'feat_wide_big': (1.1e-6, 4.7e-8, 1.9e-6, 1.5e-6),
    'gates_sat70': (3.14e-5, 6.0e-8, 1.2e-5, 1.9e-5),
    'gates_sat_vb': (1.5e-5, 3.9e-8, 1.0e-5, 1.1e-5),
}
# one get_logprobs_state step of drift from the float64 pass's state at its largest |c| (18.5, step 19): float32 oracle vs float64 oracle from the same
# float32 state -- log-probs, h', c' absolute
E_REF_STEP = (1.4e-6, 4.1e-7, 2.7e-6)
ROUTES = {
    'h2pair': (),                                             # persistent recurrences, products on fp16 pairs (the default)
    'fp32': (('persist_h2', 0),),                             # persistent recurrences, exact-fp32 products
    'launch': (('persist', 0), ('persist_bwd', 0)),           # launch-per-phase
}
DEFAULTS = (('persist', 1), ('persist_bwd', 1), ('persist_h2', 1), ('persist_sample', 1))


def gates(name):
    """(log-probs, loss, gradient tensor, gate slice)."""
    e = E_REF[name]
    return (min(max(TOL_LOGP, 4 * e[0]), CONTRACT), min(max(TOL_LOSS, 4 * e[1]), CONTRACT), max(TOL_GRAD, 4 * e[2]), max(TOL_GRAD, 4 * e[3]))


def _lib():
    from echr_amd import _lib as L
    return L, L.load()


def _config(pairs):
    L, lib = _lib()
    for k, v in pairs:
        L.check(lib.echr_config_set(k.encode(), int(v)), 'config_set')


def _drain():
    """Leave no asynchronous report behind for the next test."""
    _, lib = _lib()
    torch.cuda.synchronize()
    while lib.echr_check_async() != 0:
        pass


def _clean(lib):
    torch.cuda.synchronize()
    rc = lib.echr_check_async()
    if rc != 0:
        msg = lib.echr_last_error()
        _drain()
        raise AssertionError((rc, msg))


def _check(name, got, ref, what):
    tl, ts, tg, tsl = gates(name)
    e = D.errors(got, ref)
    print('%s %s: logp %.2e (gate %.1e) loss %.2e (gate %.1e) grad %.2e (%s, gate %.1e) slice %.2e (%s, gate %.1e)'
          % (name, what, e[0], tl, e[1], ts, e[2], e[3], tg, e[4], e[5], tsl))
    logps = got['logp'] if isinstance(got['logp'], list) else [got['logp']]
    assert all(np.isfinite(p).all() for p in logps) and np.isfinite(got['loss']), what
    assert all(v is None or np.isfinite(v).all() for v in got['grads'].values()), what
    assert e[0] < tl, (what, e[0])
    assert e[1] < ts, (what, got['loss'], ref['loss'])
    miss = D.grads_close(got['grads'], ref['grads'], tg, tsl)
    assert not miss, (what, miss)


def _module_pass(name, train_mode, route):
    _, lib = _lib()
    opt, params, vid = D.case(name)
    try:
        _config(ROUTES[route])
        pred, loss, grads, _ = U.run_gpu(opt, params, vid, train_mode)
    finally:
        _config(DEFAULTS)
    _clean(lib)
    return dict(logp=pred, loss=loss, grads=grads)


PERSISTENT = ['gates_sat', 'drift', 'feat_wide', 'feat_wide_big']


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('train_mode', [False, True])
@pytest.mark.parametrize('name', PERSISTENT)
def test_module_path_vs_float64_oracle(name, train_mode, route):
    """CaptionGenerator(mode='train') + criterion + backward, eval and train mode (the oracle gets the same Philox masks): every log-prob, the
    loss, every gradient tensor and every gate slice of the LSTM tensors against float64 -- persistent recurrences on fp16 pairs, persistent in
    exact fp32, launch-per-phase.  feat_wide_big: the BIG instantiation (129 < A <= 258)."""
    _check(name, _module_pass(name, train_mode, route), D.oracle(name, train_mode), 'module path %s train=%d' % (route, train_mode))


@pytest.mark.parametrize('train_mode', [False, True])
def test_module_path_of_70_events_vs_float64_oracle(train_mode):
    """More than 64 rows: the launch-per-phase recurrences are the only form (csrc/decoder.hip lstm_pointwise_*)."""
    _check('gates_sat70', _module_pass('gates_sat70', train_mode, 'h2pair'), D.oracle('gates_sat70', train_mode), 'module path train=%d' % train_mode)


@pytest.mark.parametrize('deterministic', [False, True])
@pytest.mark.parametrize('name', ['gates_sat', 'drift', 'feat_wide'])
def test_one_call_path_vs_float64_oracle(name, deterministic):
    """fused.FusedTrainStep (echr_train_step) with step=False, train mode: the loss and every gradient read back, atomic and fixed-order."""
    import echr_amd
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    _, lib = _lib()
    opt, params, vid = D.case(name)
    ref = D.oracle(name, True)
    dev = torch.device('cuda')
    echr_amd.set_deterministic(deterministic)
    try:
        m = U.build_gpu_model(opt, params, True)
        o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
        f = FusedTrainStep(m, o, grad_clip=None)
        tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
        labels, masks = torch.from_numpy(vid['labels']), torch.from_numpy(vid['masks'])
        loss = float(f(tap, c3d, lda, labels, vid['ind'], vid['soi'], labels[:, 1:], masks[:, 1:], step=False))
    finally:
        echr_amd.set_deterministic(False)
    _clean(lib)
    grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}
    _check(name, dict(logp=ref['logp'], loss=loss, grads=grads), ref, 'one-call deterministic=%d' % deterministic)


def _batch(vids):
    from echr_amd.batch import VideoBatch
    dev = torch.device('cuda')
    keys = ('c3d', 'lda', 'ind', 'soi', 'labels', 'masks')
    return VideoBatch.from_videos([dict({k: v[k] for k in keys}, tap=torch.from_numpy(v['tap']).to(dev)) for v in vids], device=dev)


def test_batch_step_vs_float64_oracle():
    """FusedTrainStep.batch (echr_train_step_batch) with step=False, train mode, on the 3-video batch: the summed loss, the per-video losses and the
    summed gradients against the per-video float64 oracle (tests/vbatch_ref.py)."""
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    _, lib = _lib()
    opt, params, vids = D.case('gates_sat_vb')
    ref = D.oracle('gates_sat_vb', True)
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
    f = FusedTrainStep(m, o, grad_clip=None)
    loss = float(f.batch(_batch(vids), step=False))
    _clean(lib)
    losses = f.last_video_losses.cpu().numpy()
    assert np.abs(losses - ref['losses']).max() < gates('gates_sat_vb')[1] * np.abs(ref['losses']).max()
    grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}
    _check('gates_sat_vb', dict(logp=ref['logp'], loss=loss, grads=grads), ref, 'batch step')


def batch_module_pass(train_mode):
    from echr_amd.misc.utils import LanguageModelCriterion
    _, lib = _lib()
    opt, params, vids = D.case('gates_sat_vb')
    m = U.build_gpu_model(opt, params, train_mode)
    b = _batch(vids)
    logp = m.forward_batch(b, mode='train')
    total, _ = b.criterion(LanguageModelCriterion(), logp)
    total.backward()
    _clean(lib)
    grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else None) for k, p in m.named_parameters()}
    return dict(logp=logp.detach().cpu().numpy(), loss=float(total.detach()), grads=grads)


@pytest.mark.parametrize('train_mode', [False, True])
def test_batch_module_path_vs_float64_oracle(train_mode):
    """CaptionGenerator.forward_batch + the per-video criterion + backward: the log-probs of every video too."""
    _check('gates_sat_vb', batch_module_pass(train_mode), D.oracle('gates_sat_vb', train_mode), 'forward_batch train=%d' % train_mode)


# ---- the reference's own code -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('train_mode', [False, True])
@pytest.mark.parametrize('name', ['gates_sat', 'drift'])
def test_module_path_vs_reference_fixture(name, train_mode):
    """The same against what the reference's own CPU code produced (tests/golden/case_decsat.npz, tools/make_golden.py do_decsat): float32
    summaries, therefore held to the gates above plus nothing."""
    from oracle import summary as SM
    g = U.gold('case_decsat.npz')
    tag = name + ('|train' if train_mode else '|eval')
    got = _module_pass(name, train_mode, 'h2pair')
    pred, loss, grads = got['logp'], got['loss'], got['grads']
    tl, ts, tg, _ = gates(name)
    assert abs(loss - float(g[tag + '|loss'])) < ts * abs(float(g[tag + '|loss']))
    s = SM.summarize_logp(pred)
    assert np.abs(s['slice'] - g[tag + '|logp|slice']).max() < tl and np.abs(s['top1'] - g[tag + '|logp|top1']).max() < tl
    safe = g[tag + '|logp|margin'] > 1e-4
    assert np.array_equal(s['argmax'][safe], g[tag + '|logp|argmax'][safe])
    for key, v in SM.summarize_grads(grads).items():
        ref = g[tag + '|grad|' + key]
        pname = key.split('|')[0]
        if pname in U.NOISE_ONLY:
            assert np.abs(np.asarray(v)).max() < 1e-6 and np.abs(np.asarray(ref)).max() < 1e-6, key
            continue
        scale = max(float(g[tag + '|grad|' + pname + '|linf']), U.GRAD_FLOOR)
        if key.endswith('|l2') or key.endswith('|linf'):
            assert abs(float(v) - float(ref)) < tg * max(abs(float(ref)), U.GRAD_FLOOR), (key, float(v), float(ref))
        else:
            assert np.abs(v - ref).max() < tg * scale, (key, np.abs(v - ref).max() / scale)


# ---- decoding ---------------------------------------------------------------------------------------------------------------------------
def _greedy_gpu(name, persist_sample):
    _, lib = _lib()
    opt, params, vid = D.case(name)
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    try:
        _config([('persist_sample', persist_sample)])
        with torch.no_grad():
            seq, lp = m(*(torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda')), [], vid['ind'], vid['soi'], mode='eval')
    finally:
        _config(DEFAULTS)
    _clean(lib)
    return seq.cpu().numpy(), lp.cpu().numpy()


@pytest.mark.parametrize('name', D.DECODED)
def test_greedy_decoding_vs_float64_oracle(name):
    """mode='eval' over seq_length 19, as ONE persistent launch (persist_sample = 1; 70 events: the chain sampler) and launch-per-step
    (persist_sample = 0): the tokens and the finish step of every row equal the float64 oracle's -- exact, its top-1 / top-2 margin exceeds 1e-4 at
    every pick (tests/test_decoder_regime_host.py) --, the sampled log-probs of every pick within 1e-4, and the two device routes agree with each
    other as in test_persistent_sampler_equals_launch_per_step_sampler."""
    rseq, rlp, margin, live = D.greedy64(name)
    assert float(margin[live].min()) > D.MARGIN
    outs = []
    for flag in (1, 0):
        seq, lp = _greedy_gpu(name, flag)
        e = float(np.abs(lp[live] - rlp[live]).max()) if seq.shape == rseq.shape else float('nan')
        print('%s greedy persist_sample=%d: T %d (oracle %d), sampled logp %.2e' % (name, flag, seq.shape[1], rseq.shape[1], e))
        assert np.isfinite(lp).all()
        assert seq.shape == rseq.shape and np.array_equal(seq, rseq), (name, flag)
        assert np.array_equal((seq > 0).sum(1), (rseq > 0).sum(1))          # finish steps
        assert e < CONTRACT, (name, flag, e)
        outs.append((seq, lp))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.abs(outs[0][1] - outs[1][1])[live].max() < TOL_LOGP


def drift_step_errors():
    """One get_logprobs_state step of drift from D.drift_state(): max |error| of (log-probs, h', c') against float64."""
    _, lib = _lib()
    opt, params, vid = D.case('drift')
    t, it, (h, c), rlogp, (rh, rc) = D.drift_state()
    assert float(c.abs().max()) >= 12.5
    m = U.build_gpu_model(opt, params, False)
    dev = torch.device('cuda')
    tap, c3d, lda = (torch.from_numpy(vid[k]).to(dev) for k in ('tap', 'c3d', 'lda'))
    with torch.no_grad():
        video = m.get_video_context(tap, c3d, lda, vid['ind'], vid['soi'])
        event = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'])
        clip, cmask = m.get_clip_context(tap, c3d, lda, vid['ind'], vid['soi'])
        logp, state = m.lm_model.get_logprobs_state(it.to(dev), video, event, clip, cmask, (h.to(dev).contiguous(), c.to(dev).contiguous()))
    _clean(lib)
    assert all(torch.isfinite(x).all() for x in (logp, state[0], state[1]))
    return [float((a.cpu().double() - r).abs().max()) for a, r in ((logp, rlogp), (state[0], rh), (state[1], rc))]


def test_single_step_from_the_drifted_state_vs_float64_oracle():
    """lm_model.get_logprobs_state (echr_decoder_step) on drift, from the float64 pass's state in front of the step with the largest |c| (18.5):
    log-probs and the new state against float64 from the same (float32-rounded) state; the state at max(1e-5, 4 e_ref) absolute (1e-5: the gate
    test_get_logprobs_state_single_step_vs_oracle holds it to; |c| of 18 has a float32 ulp of 1.9e-6)."""
    e = drift_step_errors()
    tol = (min(max(TOL_LOGP, 4 * E_REF_STEP[0]), CONTRACT), max(1e-5, 4 * E_REF_STEP[1]), max(1e-5, 4 * E_REF_STEP[2]))
    print('drift step: logp %.2e (gate %.1e) h %.2e (gate %.1e) c %.2e (gate %.1e)' % (e[0], tol[0], e[1], tol[1], e[2], tol[2]))
    assert e[0] < tol[0] and e[1] < tol[1] and e[2] < tol[2], e

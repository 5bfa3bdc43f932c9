"""The one-stream decoder's cell kernels (csrc/sat.hip: sat_cell_fwd_kernel, sat_cell_bwd_kernel, sat_add2_kernel) at their TILE EDGES, at
TRAINED-WEIGHT SCALES and on POISONED WORKSPACES (-m gpu), against tests/sat_ref.py carried in float64 on the same float32 inputs.
tests/test_sat_edges_host.py asserts every condition on the inputs on the CPU; tests/sat_regime_ref.py builds the cases.

1. Tile edges (tests/sat_regime_ref.EDGES; 'sat_tiny' widths but D = video_dim and H = CG_rnn_size, A = 7, 6 label columns, vocabulary 30).  The
   forward kernel works on [64 events] x [4 gates x 16 units] tiles and walks K = Dc + H in chunks of 64 floats; the reverse kernel on [64 events] x
   [64 columns of d [att | h]] tiles.  The cases: H below one unit tile (4, 12), a partial second unit block (20), K = 4, 32, 60, exactly 64 (with the
   att | h boundary at 44 and 48), 68 and 132 (ONE live float4 in the last chunk; 4 columns in the last reverse column block), 128, 136 (three
   column blocks, block 1 holds 36 d att and 28 d h columns), no 'C' at H = 64 and 68, the unaligned panel (vec_ic = 0), 1 .. 3 row tiles with 1, 63,
   64 rows in the last, ONE decoder step, a non-zero initial state at H = 20 -- and the boundary at every other float4 position of a chunk
   (BOUNDARY_SWEEP, eval mode).  Each case asserts its property from tile_props(), which reads SKC and SUNITS from the kernel source.
   Gates: those of tests/test_gpu_sat.py, imported (3e-6 / 3e-6 / 5e-5).  The float32 reference arithmetic sits at 3e-7 .. 7e-7 (gradients) here.
   Measured on an MI355X over the 25 cases: log-probs at most 2.2e-7, losses 1.7e-7, the worst gradient tensor 1.5e-6 of its max-norm (the event
   encoder's query_1.bias at ve_h68; the decoder's own tensors stay below 1.2e-6), d tap_feats 4.2e-7; greedy decoding equal at every pick (all
   resolvable), sampled log-probs within 1.6e-7.

2. Trained-weight scales (ECHR widths, N = 12, A = 40, vocabulary 300, 8 steps; made from synth.SAT_CASES by scaling only):
     gates_sat_vec  'VEC' from a non-zero initial state, embed x10, weight_ih_l0 x16, weight_hh_l0 x12: 22.7 % of the pre-activations beyond +-8,
                    the largest 34 -- fast_sigmoid, g (1 - g) and 1 - tc^2 far outside their linear part
     gates_sat_c    the same scaling on 'C' alone: 21.0 %, 32
     gates_sat70    gates_sat_vec over 70 events: two row tiles
     state_far      init_linear scaled until max |h(-1)| = max |c(-1)| = 12 (the LSTM has no bias that could walk the state there); and ONE
                    get_logprobs_state call from the float64 pass's h with c in +-[9, 20] on a quarter of the units and 16 exact zeros
     neg_far        gates_sat_vec with the token columns of the i, f and o rows of weight_ih_l0 x6: pre-activations down to -130 / -120 / -139 in
                    i / f / o -- below -88 __expf(-x) is +inf, the sigmoid must be exactly 0
   Gates: max(gate of tests/test_gpu_sat.py, 4 e_ref) per quantity, log-probs and loss never above the 1e-4 contract; e_ref = the float32 run of
   tests/sat_ref.py against its float64 run on the CPU (one thread), the larger of eval and train mode; 4x: another summation order and the 1-ulp
   hardware exp / rcp.  Log-probs absolute, loss relative, gradients relative to the reference tensor's max-norm (d tap_feats among them), gate
   slices [i | f | g | o] of weight_ih_l0 / weight_hh_l0 relative to the slice's own max-norm.

     variant         e_ref: logp     loss     grad    slice   |  HIP measured (MI355X), worst of eval / train / deterministic: logp / loss / grad / slice
     gates_sat_vec        8.2e-6   7.2e-8   1.0e-5   5.9e-6   |  1.0e-5 / 7.2e-8 / 1.4e-5 / 1.4e-5     greedy: sampled logp 3.5e-6
     gates_sat_c          4.7e-6   7.9e-8   7.8e-6   5.6e-6   |  7.5e-6 / 7.9e-8 / 2.1e-5 / 1.2e-5     greedy 4.0e-6
     gates_sat70          1.1e-5   5.4e-8   1.3e-5   1.2e-5   |  1.3e-5 / 5.4e-8 / 1.3e-5 / 1.2e-5     greedy 4.8e-6
     state_far            1.1e-6   6.0e-8   1.0e-6   7.3e-7   |  4.0e-6 / 5.4e-8 / 2.0e-6 / 2.0e-6     greedy 1.5e-6
     neg_far              7.9e-6   7.4e-8   1.4e-5   1.4e-5   |  7.7e-6 / 6.1e-8 / 2.6e-5 / 1.7e-5     greedy 2.9e-6
     the far step         logp 6.4e-7, h' 9.9e-8, c' 1.8e-6 (|c| up to 20: an ulp of 1.9e-6)   |  1.2e-6 / 2.7e-7 / 4.3e-6 (gates 3.0e-6 / 1e-5 / 1e-5)
   The smallest margin to a gate: state_far's log-probs in deterministic mode, 3.95e-6 under 4.3e-6 (eval 2.1e-6, train 2.5e-6 in the default mode);
   every other figure stays below 0.45 of its gate.  The worst gradient figures (2.1e-5 gates_sat_c, 2.6e-5 neg_far) are alpha_net.weight and the event
   encoder's query_1.weight; the LSTM tensors and their gate slices stay within 2.4x e_ref.
   Greedy decoding (7 picks a row): every pick equal where the float64 decode is resolvable (top-1 / top-2 margin above 1e-4 at the pick and at
   every earlier pick of the row: 100 % of the picks but gates_sat70's 97.6 %).

3. Workspaces and the accumulate contract (deterministic mode; sat_tiny, k64_h20, init_h20 and 'E' alone).  Every torch.empty / torch.empty_like of
   echr_amd/sat.py -- the forward, backward and sampler workspaces, logp, the parameter-gradient buffers of `zeroed` = 0, g_event, g_video, g_h0, seq,
   seq_logp, the counts -- is handed out filled with NaN (integers: 0x5A5A5A5A) and the run compared BIT FOR BIT with the one on zero-filled
   buffers: every bit equal, nothing is read before it is written and every output is overwritten.  `zeroed` = 1 accumulates onto buffers holding
   small integers: every tensor meets the one-ulp bound (ten measured at 0.50 ulp and less; the table now takes one rounding too).  DEFECT FOUND AND FIXED: the embedding table missed the one-ulp bound (1.06 ulp on sat_tiny,
   4.13 ulp on k64_h20, on the <bos> / padding row that the scatter-add rounds once per occurrence); echr_sat_bwd now adds the call's table gradient
   to the caller's buffer once (test_zeroed_backward_accumulates_onto_what_the_buffers_hold).

4. Sensitivity (scratch builds of csrc/sat.hip outside the tree, arithmetic altered only; the 86 cases of this file, run on the build before the embedding fix, whose two
   failing cases are not counted):
   a. `u < H` loosened to `u < roundup(H, 16)` in the forward epilogue: 38 fail -- the float64 comparison of every table case with H % 16 != 0 (h4_e,
      h12_c, k60, k64_h20, k136, ve_h68, unaligned_h20, s1, init_h20) and all 11 boundary-sweep cases (H = 20), greedy decoding of the seven of them
      with more than one unit block, the poisoned runs of k64_h20 and init_h20, nine `zeroed` tensors of k64_h20.  Every case with H % 16 == 0 and all
      of section 2 (H = 512) pass.
   b. `if (k0) __syncthreads()` of the forward kernel removed, `if (ub) __syncthreads()` of the reverse kernel removed: NOT CAUGHT, no case fails on
      either build.  The barrier closes a race between a wave that has finished a chunk's MFMA chain and stores the next chunk into LDS and a wave
      still reading the previous one.  It did not show in any of the 86 cases on an MI355X, presumably because the four waves of a workgroup leave
      the chain within a few cycles of each other and the barrier behind the stores keeps them in step.  The cases with 2, 3 and 16 k chunks / 2 .. 32
      unit blocks are the ones that would show it; a value test cannot make a wave late.
   c. `k < K` dropped from the forward fetch: NOT RUN.  The float4s behind K of the last gate row of the panel and of the last event's h row lie
      past the end of w_hh and of the step's state block: an out-of-bounds read, which no run here does on purpose.  By the
      code: both operands then hold the NEXT row's elements in the columns K .. roundup(K, 64), so every output gains sum_k h[n+1][k'] w[r+1][k'], of
      the size of the pre-activation itself, in every case with K % 64 != 0 -- h4_e, h12_c, k60, k68, k132, k136, ve_h68, s1, eight sweep cases and
      all of section 2 under 'VEC' (K = 1012) -- and nothing changes where K % 64 == 0 (k64_h20, k64_h16, k128, ve_h64, unaligned_h20, init_h20).
   d. fast_sigmoid's argument clamped at +-8: 16 fail -- gates_sat_vec, gates_sat_c, gates_sat70 and neg_far on every route (eval, train, deterministic,
      greedy).  state_far (no pre-activation beyond 7.5), the far step and sections 1 and 3 pass.
   e. tanhf(c)'s argument clamped at +-8, forward and reverse: NOT CAUGHT, and cannot be in float32: tanh(8) = 1 - 2.3e-7, four ulps below the 1.0 that
      tanhf returns from 9.1 on, so h moves by at most 2.3e-7 and 1 - tc^2 by 4.5e-7 -- under state_far's gates (4.3e-6, 1e-5).  What state_far and the far
      step do see is the cell state itself.  Two further builds show it: the NEW CELL STATE clamped at +-8 in the forward kernel -- 5 fail, state_far on
      every route (eval, train, deterministic, greedy) and the far step, nothing else (no other case has |c| above 8.1); tanhf's argument clamped at
      +-4 (tanh(4) = 0.99933) -- 21 fail, every section 2 case on every route and the far step.
   f. The fill of the reverse pass's zero range shortened by DPALL: 39 fail -- the poisoned runs of sat_tiny, k64_h20 and init_h20 ('E' alone never
      touches DPALL), `zeroed` w_c2a / b_c2a of both cases, and, since the allocator hands back blocks that held other tensors a moment ago, also 11
      table cases with 'C', 9 sweep cases and 12 section 2 cases; which of the latter fail depends on what the block held, the poisoned runs do not.
"""
import numpy as np
import pytest
import torch

from tests import sat_ref as R
from tests import sat_regime_ref as G
from tests import test_gpu_sat as T
from tests import util as U

pytestmark = pytest.mark.gpu

CONTRACT = 1e-4
# e_ref (logp absolute, loss relative, worst gradient tensor, worst gate slice of the LSTM tensors): tests/sat_regime_ref.e_ref, re-measured by
# tests/test_sat_edges_host.py
E_REF = {
    'gates_sat_vec': (8.2e-6, 7.2e-8, 1.0e-5, 5.9e-6),
    'gates_sat_c': (4.7e-6, 7.9e-8, 7.8e-6, 5.6e-6),
    'gates_sat70': (1.05e-5, 5.4e-8, 1.32e-5, 1.22e-5),
    'state_far': (1.07e-6, 6.0e-8, 1.04e-6, 7.3e-7),
    'neg_far': (7.9e-6, 7.4e-8, 1.4e-5, 1.4e-5),
}
E_REF_STEP = (6.4e-7, 9.9e-8, 1.83e-6)          # the far step: log-probs, h', c' absolute (tests/sat_regime_ref.far_step_e_ref)
TOL_STATE = 1e-5          # h', c' absolute: a handful of roundings at |c| <= 20, whose float32 ulp is 1.9e-6 (the three-stream decoder's step gate)


def gates(name):
    """(log-probs, loss, gradient tensor, gate slice)."""
    e = E_REF[name]
    return (min(max(T.TOL_LOGP, 4 * e[0]), CONTRACT), min(max(T.TOL_LOSS, 4 * e[1]), CONTRACT), max(T.TOL_GRAD, 4 * e[2]), max(T.TOL_GRAD, 4 * e[3]))


def step_gates():
    return (min(max(T.TOL_LOGP, 4 * E_REF_STEP[0]), CONTRACT), max(TOL_STATE, 4 * E_REF_STEP[1]), max(TOL_STATE, 4 * E_REF_STEP[2]))


def _greedy_gpu(opt, params, vid):
    m = U.build_gpu_model(opt, params, False)
    tap, c3d, lda = T._feats(vid)
    with torch.no_grad():
        seq, lp = m(tap, c3d, lda, [], vid['ind'], vid['soi'], mode='eval')
    torch.cuda.synchronize()
    return seq.cpu().numpy(), lp.cpu().numpy()


def _check_greedy(tag, got, ref, tol, relative=False):
    """Every pick equal, and its log-prob within `tol` (absolute, or relative to the reference's max-norm as tests/test_gpu_sat.py measures it), where
    the float64 decode is resolvable (sat_regime_ref.greedy64_of: `live`)."""
    (seq, lp), (rseq, rlp, mar, live) = got, ref
    w = min(seq.shape[1], rseq.shape[1])
    if live.all():
        assert seq.shape == rseq.shape, (tag, seq.shape, rseq.shape)
    assert live[:, w:].sum() == 0, (tag, seq.shape, rseq.shape)          # a resolvable pick that the device never made
    lv = live[:, :w]
    e = float(np.abs(lp[:, :w][lv] - rlp[:, :w][lv]).max()) / (float(np.abs(rlp[:, :w][lv]).max()) if relative else 1.0)
    print('[%s/greedy] %s, resolvable %.3f, sampled logp %.2e (gate %.1e)' % (tag, tuple(seq.shape), live.mean(), e, tol))
    assert seq.dtype == np.int64 and np.isfinite(lp).all()
    assert np.array_equal(seq[:, :w][lv], rseq[:, :w][lv]) and e < tol, tag


# ---- 1. tile edges -----------------------------------------------------------------------------------------------------------------------------
MAIN = [n for n in G.EDGES if n not in ['b%d' % d for d in G.BOUNDARY_SWEEP]]


@pytest.mark.parametrize('name', MAIN)
def test_tile_edge_against_float64(name):
    """Forward and backward in eval and train mode: log-probs, loss, every parameter gradient, d tap_feats; exact-zero dead attention without 'C'."""
    p = G.check_edge(name)
    opt, params, vid = G.edge_case(name)
    print('[%s] %s' % (name, ' '.join('%s=%d' % kv for kv in sorted(p.items()))))
    for train_mode in (False, True):
        ref = R.run(opt, params, vid, train_mode, dtype=torch.float64)
        T._check_against('%s/%s' % (name, 'train' if train_mode else 'eval'), T._run(opt, params, vid, train_mode), ref, opt)


@pytest.mark.parametrize('name', MAIN)
def test_tile_edge_greedy_decode(name):
    G.check_edge(name)
    opt, params, vid = G.edge_case(name)
    _check_greedy(name, _greedy_gpu(opt, params, vid), G.greedy64_of(opt, params, vid), T.TOL_LOGP, relative=True)


@pytest.mark.parametrize('d', G.BOUNDARY_SWEEP)
def test_att_h_boundary_at_every_float4_of_a_chunk(d):
    """'C' at H = 20, D = 4 .. 64: with the table's cases the att | h boundary has stood at every float4 position 0 .. 15 of a chunk."""
    name = 'b%d' % d
    G.check_edge(name)
    seen = {G.tile_props(*G.edge_case(n))['boundary'] // 4 for n in G.EDGES if G.tile_props(*G.edge_case(n))['Dc']}
    assert seen == set(range(16)), sorted(seen)
    opt, params, vid = G.edge_case(name)
    T._check_against(name + '/eval', T._run(opt, params, vid, False), R.run(opt, params, vid, False, dtype=torch.float64), opt)


# ---- 2. trained-weight scales ------------------------------------------------------------------------------------------------------------------
def _as_dict(run):
    return dict(logp=run[0], loss=run[1], grads=run[2], gtap=run[3])


def _check(name, got, ref, what):
    tl, ts, tg, tsl = gates(name)
    e = G.errors(got, ref)
    print('[%s %s] logp %.2e (gate %.1e) loss %.2e (gate %.1e) grad %.2e (%s, gate %.1e) slice %.2e (%s, gate %.1e)'
          % (name, what, e[0], tl, e[1], ts, e[2][0], e[2][1], tg, e[3][0], e[3][1], tsl))
    assert np.isfinite(got['logp']).all() and np.isfinite(got['loss']) and np.isfinite(got['gtap']).all(), what
    assert all(v is None or np.isfinite(v).all() for v in got['grads'].values()), what
    for k in R.NOISE_ONLY:
        assert float(np.abs(got['grads'][k]).max()) < 1e-6, k
    assert e[0] < tl and e[1] < ts and e[2][0] < tg and e[3][0] < tsl, (what, e)


@pytest.mark.parametrize('train_mode', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('name', list(G.REGIME))
def test_regime_module_path_vs_float64(name, train_mode):
    opt, params, vid = G.case(name)
    _check(name, _as_dict(T._run(opt, params, vid, train_mode)), G.oracle(name, train_mode), 'train' if train_mode else 'eval')


@pytest.mark.parametrize('name', list(G.REGIME))
def test_regime_deterministic_runs_agree_bit_for_bit(name):
    import echr_amd
    opt, params, vid = G.case(name)
    echr_amd.set_deterministic(True)
    try:
        a, b = (_as_dict(T._run(opt, params, vid, True)) for _ in range(2))
    finally:
        echr_amd.set_deterministic(False)
    assert np.array_equal(a['logp'], b['logp']) and a['loss'] == b['loss'] and np.array_equal(a['gtap'], b['gtap'])
    for k in a['grads']:
        assert (a['grads'][k] is None and b['grads'][k] is None) or np.array_equal(a['grads'][k], b['grads'][k]), k
    _check(name, a, G.oracle(name, True), 'deterministic')


@pytest.mark.parametrize('name', list(G.REGIME))
def test_regime_greedy_decode_vs_float64(name):
    opt, params, vid = G.case(name)
    _check_greedy(name, _greedy_gpu(opt, params, vid), G.greedy64(name), gates(name)[0])


def test_single_step_from_a_far_cell_state_vs_float64():
    """get_logprobs_state (echr_sat_step) from sat_regime_ref.far_state(): |c| up to 20 on a quarter of the units, exact zeros on 16."""
    opt, params, vid = G.case('state_far')
    it, (h, c), rlogp, (rh, rc), _ = G.far_state()
    m = U.build_gpu_model(opt, params, False)
    tap, c3d, lda = T._feats(vid)
    dev = tap.device
    with torch.no_grad():
        ev = m.get_event_context(tap, c3d, lda, vid['ind'], vid['soi'])
        vd = m.get_video_context(tap, c3d, lda, vid['ind'], vid['soi'])
        cl, cm = m.get_clip_context(tap, c3d, lda, vid['ind'], vid['soi'])
        lp, (h2, c2) = m.lm_model.get_logprobs_state(it.to(dev), vd, ev, cl, cm, (h.to(dev).contiguous(), c.to(dev).contiguous()))
    torch.cuda.synchronize()
    e = [float(np.abs(a.cpu().numpy().astype(np.float64) - r).max()) for a, r in ((lp, rlogp), (h2, rh), (c2, rc))]
    tol = step_gates()
    print('[far step] logp %.2e (gate %.1e) h %.2e (gate %.1e) c %.2e (gate %.1e)' % (e[0], tol[0], e[1], tol[1], e[2], tol[2]))
    assert all(torch.isfinite(x).all() for x in (lp, h2, c2))
    assert e[0] < tol[0] and e[1] < tol[1] and e[2] < tol[2], e


# ---- 3. workspaces and the accumulate contract ----------------------------------------------------------------------------------------------------
INT_POISON = 0x5A5A5A5A


class _Alloc(object):
    """Stands in for the name `torch` inside echr_amd.sat: empty / empty_like hand out FILLED buffers (poison: NaN / INT_POISON, else zero)."""

    def __init__(self, poison):
        self.poison, self.count = poison, 0

    def __getattr__(self, k):
        return getattr(torch, k)

    def _fill(self, t):
        self.count += 1
        if t.is_floating_point():
            return t.fill_(float('nan') if self.poison else 0.0)
        return t.fill_(INT_POISON if self.poison else 0)

    def empty(self, *a, **k):
        return self._fill(torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._fill(torch.empty_like(*a, **k))


def _ws_case(name):
    if name == 'sat_tiny':
        return G.synth.make_sat_case('sat_tiny')
    if name == 'tiny_e':          # 'E' alone: Dc = 0, ATT / DATT are never written
        return T._edge_case('E', seed=431)
    return G.edge_case(name)


def _all_outputs(opt, params, vid, monkeypatch, poison):
    """A training iteration and a greedy decode with every allocation of echr_amd/sat.py filled: dict of arrays."""
    from echr_amd import sat
    alloc = _Alloc(poison)
    with monkeypatch.context() as mp:
        mp.setattr(sat, 'torch', alloc)
        pred, loss, grads, gtap, _ = T._run(opt, params, vid, True)
        n_train = alloc.count
        seq, lp = _greedy_gpu(opt, params, vid)
    # forward: ws, logp; backward: ws_bwd, 11 parameter gradients (+ g_video, g_event, g_h0); the decode: ws, sampler ws, seq, seq_logp, counts
    assert n_train >= 14 and alloc.count - n_train == 5, (n_train, alloc.count)
    out = {'grad|' + k: v for k, v in grads.items() if v is not None}
    out.update(logp=pred, loss=np.float64(loss), gtap=gtap, seq=seq, seq_logp=lp)
    return out


@pytest.mark.parametrize('name', ['sat_tiny', 'k64_h20', 'init_h20', 'tiny_e'])
def test_poisoned_workspaces_give_the_same_bits(name, monkeypatch):
    """NaN in every buffer the one-stream entries allocate -- workspaces and outputs -- against zeros there: logp, every gradient (those of the event
    encoder, init_linear and tap_feats behind g_event, g_video, g_h0 included), seq and seq_logp bit for bit.  An output that is accumulated into, or
    a workspace range read before it is written, carries the NaN out."""
    import echr_amd
    opt, params, vid = _ws_case(name)
    echr_amd.set_deterministic(True)
    try:
        zero = _all_outputs(opt, params, vid, monkeypatch, False)
        nan = _all_outputs(opt, params, vid, monkeypatch, True)
    finally:
        echr_amd.set_deterministic(False)
    bad = [k for k in zero if not np.all(np.isfinite(nan[k]))]
    diff = [k for k in zero if not np.array_equal(zero[k], nan[k])]
    print('[poison/%s] %d outputs, non-finite %s, differing %s' % (name, len(zero), bad, diff))
    assert set(zero) == set(nan) and not bad and not diff
    if name == 'init_h20':
        assert np.any(zero['grad|lm_model.init_linear.weight'])          # (g_h0 is live)
    assert np.any(zero['gtap']) and np.any(zero['grad|fusion_model.event_emb.weight'])          # (g_event is live)


class _Sink(object):
    """A GradSink whose span is the test's own: SatFunction.backward accumulates into `bufs` with `zeroed` = 1."""

    def __init__(self, bufs):
        self.bufs, self.taken = bufs, 0

    def usable(self):
        return True

    def take(self):
        self.taken += 1
        return self.bufs


_ZEROED = {}


def _zeroed_runs(name):
    """(fresh gradients by parameter name, [(name, integer pattern, buffer after the backward)] in SAT_PARAMS order, tokens [S, N]): once per case."""
    if name in _ZEROED:
        return _ZEROED[name]
    import echr_amd
    opt, params, vid = _ws_case(name)
    echr_amd.set_deterministic(True)
    try:
        fresh = T._run(opt, params, vid, True)[2]
        m = U.build_gpu_model(opt, params, True)
        ps = m.lm_model.native_params()
        pattern = [((torch.arange(p.numel(), device=p.device) % 7) - 3).float().view_as(p).contiguous() for p in ps]
        sink = _Sink([x.clone() for x in pattern])
        m.lm_model._grad_sink = lambda group: sink if len(group) == len(ps) else None          # (init_linear's group keeps its fresh buffers)
        T._run(opt, params, vid, True, m=m)
    finally:
        echr_amd.set_deterministic(False)
    assert sink.taken == 1
    names = {id(p): k for k, p in m.named_parameters()}
    S = R.O.n_decoder_steps(vid['labels'])
    _ZEROED[name] = (fresh, [(names[id(p)], a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64))
                             for p, a, b in zip(ps, pattern, sink.bufs)], vid['labels'][:, :S].T)
    return _ZEROED[name]


@pytest.mark.parametrize('which', range(11), ids=__import__('echr_amd.sat', fromlist=['SAT_PARAMS']).SAT_PARAMS)
@pytest.mark.parametrize('name', ['sat_tiny', 'k64_h20'])
def test_zeroed_backward_accumulates_onto_what_the_buffers_hold(name, which):
    """`zeroed` = 1: the parameter-gradient buffers hold small integers (-3 .. 3) when echr_sat_bwd runs and integer + gradient after it, within ONE
    float32 ulp of the larger of the two magnitudes per element, and the integer itself where the gradient is exactly zero.

    The embedding table was the one tensor that missed this bound (1.06 ulp on sat_tiny, 4.13 ulp on k64_h20): embed_scatter_add adds the gradient
    rows into the table one at a time, so a table row whose token is fed at m positions was rounded m times at the magnitude of what the buffer held
    -- <bos> / the padding 0 is fed 6 and 208 times.  echr_sat_bwd now sums the table gradient from zero in its workspace and adds it to the
    caller's buffer once (`zeroed` = 1 only; onto a zero-filled span the bits are the ones it gave before)."""
    fresh, bufs, tokens = _zeroed_runs(name)
    k, pat, got = bufs[which]
    g = fresh[k].astype(np.float64)
    want = pat + g
    ulp = np.spacing(np.maximum(np.abs(pat), np.abs(want)).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want) / ulp
    print('[zeroed/%s] %s: worst |buffer - (integer + gradient)| = %.2f ulp; %d of %d elements have a zero gradient'
          % (name, k, float(err.max()), int((g == 0).sum()), g.size))
    if which == 0:
        fed = np.bincount(tokens.reshape(-1), minlength=pat.shape[0])
        once = fed == 1
        print('[zeroed/%s] table rows by how often their token is fed: %s; rows fed once: %.2f ulp; worst row: token %d, fed %d times'
              % (name, dict(zip(*np.unique(fed, return_counts=True))), float(err[once].max()) if once.any() else float('nan'),
                 int(err.max(1).argmax()), int(fed[err.max(1).argmax()])))
        assert not (fed <= 1).any() or float(err[fed <= 1].max()) <= 1.0
    assert np.isfinite(got).all() and np.array_equal(got[g == 0], pat[g == 0]), k
    assert float(err.max()) <= 1.0, (k, float(err.max()))

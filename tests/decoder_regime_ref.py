"""CPU side of the decoder's trained-regime cases (synth.make_decsat): the float64 and float32 oracles, a spy on the oracle's LSTM cell, the error
measures of tests/test_gpu_decoder_regime.py (per tensor and, for the LSTM tensors, per gate slice [i | f | g | o]) and the float64 greedy decode
with its top-1 / top-2 margins.  Used by tests/test_decoder_regime_host.py, the GPU file and tools/parity_report.py --decsat."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from echr_amd import synth
from oracle import echr_ref_cpu as O
from tests import clipctx_ref as R
from tests import util as U
from tests import vbatch_ref as VB

SINGLE = [k for k in synth.DECSAT if 'vbatch' not in synth.DECSAT[k]]
DECODED = ['gates_sat', 'drift', 'feat_wide', 'feat_wide_big', 'gates_sat70']
MARGIN = 1e-4          # smallest top-1 / top-2 gap of the float64 greedy decode: the log-prob contract, so no route inside it can pick another word
GATE_NAMES = 'ifgo'


@functools.lru_cache(maxsize=None)
def case(name):
    return synth.make_decsat(name)


def is_lstm(k):
    return '.core.layer' in k


def gate_slices(k, g):
    """[(label, slice of g)] of an LSTM tensor: rows [jH, (j + 1)H) of weight_ih / weight_hh / bias_*, gate order i, f, g, o."""
    H = g.shape[0] // 4
    return [('%s[%s]' % (k, GATE_NAMES[j]), g[j * H:(j + 1) * H]) for j in range(4)]


@functools.lru_cache(maxsize=None)
def oracle(name, train, f64=True):
    """dict(logp, loss, grads) of the oracle in float64 (or float32) on the case's float32 inputs, train mode with the build's Philox masks.
    logp: [N, S, V1], or for the batch a list of [N_v, S_v, V1] (tests/vbatch_ref.py: per-video oracle, gradients summed); `losses` there too."""
    opt, params, vid = case(name)
    dtype = torch.float64 if f64 else torch.float32
    if isinstance(vid, list):
        r = VB.run(opt, params, vid, train, dtype=dtype)
        return dict(logp=r['logp'], loss=r['loss'], losses=r['losses'], grads=r['grads'])
    logp, loss, grads, _ = R.run(opt, params, vid, train, dtype=dtype)
    return dict(logp=logp, loss=loss, grads=grads)


def probe(name):
    """The float64 oracle's teacher-forced eval pass through a spy on oracle.lstm_cell: dict(pre=[3 x [S, N, 4H]], c=[3 x [S, N, H]]) -- gate
    pre-activations and new cell states of streams 0, 1, 2 (core_step calls the cell in that order); of the batch: flat, all videos."""
    opt, params, vid = case(name)
    calls = []
    orig = O.lstm_cell

    def spy(x, h, c, w_ih, w_hh, b_ih, b_hh):
        out = orig(x, h, c, w_ih, w_hh, b_ih, b_hh)
        calls.append(((F.linear(x, w_ih, b_ih) + F.linear(h, w_hh, b_hh)).detach().numpy(), out[1].detach().numpy()))
        return out
    O.lstm_cell = spy
    try:
        if isinstance(vid, list):
            VB.run(opt, params, vid, False, dtype=torch.float64, backward=False)
        else:
            R.run(opt, params, vid, False, backward=False, dtype=torch.float64)
    finally:
        O.lstm_cell = orig
    assert len(calls) % 3 == 0
    join = (lambda xs: np.concatenate([x.reshape(-1) for x in xs])) if isinstance(vid, list) else np.stack
    return dict(pre=[join([c[0] for c in calls[k::3]]) for k in range(3)], c=[join([c[1] for c in calls[k::3]]) for k in range(3)])


def probe_context(name):
    """The attended context [S, N, D] of the float64 oracle's teacher-forced eval pass (a spy on oracle.attention)."""
    opt, params, vid = case(name)
    out = []
    orig = O.attention

    def spy(*a, **k):
        r = orig(*a, **k)
        out.append(r[0].detach().numpy())
        return r
    O.attention = spy
    try:
        R.run(opt, params, vid, False, backward=False, dtype=torch.float64)
    finally:
        O.attention = orig
    return np.stack(out)


def pair_scaled(x, bound):
    """|x| times the persistent kernels' conversion factor 2^(12 - ex) of a context bounded by `bound` (|context| < 2^ex; csrc/persist.hip): fp16
    holds it up to 65504 (from 65520 on it rounds to inf)."""
    ex = int(np.frexp(max(float(bound), 1e-30))[1])
    return np.abs(x) * 2.0 ** (12 - ex)


FP16_INF = 65520.0


def max_fed_h(name):
    """Largest |h| (dropped, train mode, float64 oracle) that is fed to a next step of the batch variant: every step but each video's last."""
    from oracle import echr_ref_cpu as O2
    opt, params, vids = case(name)
    hs = []
    orig = O.core_step

    def spy(*a, **k):
        out = orig(*a, **k)
        hs.append(float(out[1][0].detach().abs().max()))
        return out
    O.core_step = spy
    try:
        VB.run(opt, params, vids, True, dtype=torch.float64, backward=False)
    finally:
        O.core_step = orig
    fed, i = 0.0, 0
    for v in vids:          # the per-video oracle runs the videos in turn
        S = O2.n_decoder_steps(v['labels'])
        fed = max([fed] + hs[i:i + S - 1])
        i += S
    assert i == len(hs)
    return fed


def errors(got, ref):
    """(max |d logp|, relative loss error, worst gradient tensor error, its name, worst LSTM gate-slice error, its label) of `got` against `ref`
    (both dict(logp, loss, grads); a batch's logp: the [N_tot, S, V1] array or the per-video list against the per-video list).  Gradients
    relative to the reference tensor's (slice's) max-norm, util.GRAD_FLOOR below it; util.NOISE_ONLY left out."""
    if isinstance(ref['logp'], list):
        gl = got['logp']
        if not isinstance(gl, list):
            eo = np.cumsum([0] + [r.shape[0] for r in ref['logp']])
            gl = [gl[eo[v]:eo[v + 1], :r.shape[1]] for v, r in enumerate(ref['logp'])]
        e_logp = max(float(np.abs(a - r).max()) for a, r in zip(gl, ref['logp']))
    else:
        assert got['logp'].shape == ref['logp'].shape
        e_logp = float(np.abs(got['logp'] - ref['logp']).max())
    e_loss = abs(got['loss'] - ref['loss']) / abs(ref['loss'])
    worst, worst_s = (0.0, ''), (0.0, '')
    for k, g in ref['grads'].items():
        if g is None or k in U.NOISE_ONLY:
            continue
        worst = max(worst, (U.relerr(got['grads'][k], g, U.GRAD_FLOOR), k))
        if is_lstm(k):
            for (label, gs), (_, rs) in zip(gate_slices(k, got['grads'][k]), gate_slices(k, g)):
                worst_s = max(worst_s, (U.relerr(gs, rs, U.GRAD_FLOOR), label))
    return e_logp, e_loss, worst[0], worst[1], worst_s[0], worst_s[1]


def grads_close(grads, ref_grads, tol, tol_slice):
    """The gradient gate: every tensor (util.grad_close, `tol`) and every gate slice of the LSTM tensors (`tol_slice`), each against its own
    max-norm.  Returns the list of misses [(label, error)]."""
    miss = []
    for k, g in ref_grads.items():
        if g is None:
            if not (grads[k] is None or not np.any(grads[k])):
                miss.append((k, float('inf')))
            continue
        if not U.grad_close(k, grads[k], g, tol):
            miss.append((k, U.relerr(grads[k], g)))
        if is_lstm(k):
            for (label, gs), (_, rs) in zip(gate_slices(k, grads[k]), gate_slices(k, g)):
                if not U.grad_close(label, gs, rs, tol_slice):
                    miss.append((label, U.relerr(gs, rs)))
    return miss


@functools.lru_cache(maxsize=None)
def e_ref(name, train):
    """The float32 oracle against the float64 oracle: (logp absolute, loss relative, worst gradient tensor, name, worst gate slice, label)."""
    return errors(oracle(name, train, False), oracle(name, train, True))


def contexts64(opt, params, vid):
    P = {k: torch.from_numpy(v.copy()).double() for k, v in params.items()}
    tap, c3d, lda = (torch.from_numpy(vid[k]).double() for k in ('tap', 'c3d', 'lda'))
    with torch.no_grad():
        return (P,) + tuple(R.contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi']))


def greedy64_of(opt, params, vid):
    """oracle.decoder_sample in float64: (seq [N, T], sampled log-probs [N, T], top-1 / top-2 margin [N, T], live [N, T]) -- live: the row was
    unfinished BEFORE the pick of that column (the picks that decide its caption, its <eos> included)."""
    P, video, event, cl, mask = contexts64(opt, params, vid)
    N = event.shape[0]
    state = O.init_hidden(P, video, event, cl, opt.CG_init_feats_type)
    seq, slp, mar, live = [], [], [], []
    logprobs = None
    unfinished = torch.ones(N, dtype=torch.bool)
    with torch.no_grad():
        for t in range(opt.CG_seq_length + 1):
            if t == 0:
                it = torch.zeros(N, dtype=torch.long)
            else:
                top = logprobs.topk(2, dim=1)
                sample_lp, it, margin = top.values[:, 0], top.indices[:, 0], top.values[:, 0] - top.values[:, 1]
            logprobs, state = O.logprobs_state(P, it, video, event, cl, mask, state)
            if t >= 1:
                before = unfinished.clone()
                unfinished = unfinished & (it > 0)
                if int(unfinished.sum()) == 0:
                    break
                seq.append(it * unfinished.type_as(it)); slp.append(sample_lp); mar.append(margin); live.append(before)
    return tuple(torch.stack(x, 1).numpy() for x in (seq, slp, mar, live))


@functools.lru_cache(maxsize=None)
def greedy64(name):
    return greedy64_of(*case(name))


def drift_state():
    """The float64 state (h, c) [3, N, H] in front of the teacher-forced step of 'drift' with the largest |c|, the step's tokens, and that step's
    float64 log-probs and new state: (t, it, (h, c), logp, (h', c'))."""
    opt, params, vid = case('drift')
    P, video, event, cl, mask = contexts64(opt, params, vid)
    labels = torch.from_numpy(vid['labels'])
    state = O.init_hidden(P, video, event, cl, opt.CG_init_feats_type)
    hist = []
    with torch.no_grad():
        for t in range(labels.shape[1] - 1):
            logp, new = O.logprobs_state(P, labels[:, t], video, event, cl, mask, state)
            hist.append((t, labels[:, t], state, logp, new))
            state = new
    # the step whose INPUT state has the largest |c|; the state rounded to float32 (what the device is handed), the step redone from exactly that
    t, it, state, _, _ = max(hist, key=lambda r: float(r[2][1].abs().max()))
    state = (state[0].float(), state[1].float())
    with torch.no_grad():
        logp, new = O.logprobs_state(P, it, video, event, cl, mask, (state[0].double(), state[1].double()))
    return t, it, state, logp, new


def drift_step_e_ref():
    """The float32 oracle's step from drift_state()'s state against the float64 one: (log-probs, h', c') absolute."""
    opt, params, vid = case('drift')
    t, it, (h, c), logp, (rh, rc) = drift_state()
    P = {k: torch.from_numpy(v.copy()) for k, v in params.items()}
    tap, c3d, lda = (torch.from_numpy(vid[k]) for k in ('tap', 'c3d', 'lda'))
    with torch.no_grad():
        video, event, cl, mask = R.contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi'])
        l32, (h32, c32) = O.logprobs_state(P, it, video, event, cl, mask, (h, c))
    return tuple(float((a.double() - r).abs().max()) for a, r in ((l32, logp), (h32, rh), (c32, rc)))

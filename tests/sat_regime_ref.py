"""CPU side of tests/test_gpu_sat_edges.py (the one-stream decoder's cell kernels, csrc/sat.hip, at their tile edges and at trained-weight
scales): the edge-shape table with the tile property each case is there for, the scaled variants with the float64 / float32 runs of
tests/sat_ref.py, a probe of the gate pre-activations, the error measures (per tensor and per gate slice [i | f | g | o] of the LSTM tensors)
and the float64 greedy decode with its top-1 / top-2 margins.  Used by tests/test_sat_edges_host.py and the GPU file."""
import contextlib
import functools
import os
import re

import numpy as np
import torch

from echr_amd import synth
from tests import sat_ref as R
from tests import util as U

MARGIN = 1e-4          # top-1 / top-2 gap of the float64 greedy decode above which no route inside the log-prob contract can pick another word
GATE_NAMES = 'ifgo'
LSTM_KEYS = (R.PRE + 'core.rnn.weight_ih_l0', R.PRE + 'core.rnn.weight_hh_l0')


# ---- 1. tile edges --------------------------------------------------------------------------------------------------------------------------
def kernel_constants():
    """SKC (k chunk), SUNITS (hidden units per forward workgroup) as csrc/sat.hip declares them -- read from the source, so that a change there
    shows in the properties below."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'echr_amd', 'csrc', 'sat.hip')).read()
    return tuple(int(re.search(r'constexpr int %s = (\d+);' % k, src).group(1)) for k in ('SKC', 'SUNITS'))


ROWS = 64          # events per workgroup of both cell kernels, columns of d [att | h] per workgroup of the reverse one

# name: feats, N, widths over the 'sat_tiny' ones (D = video_dim: the attended clip's width; H = CG_rnn_size), further _edge_case arguments, and
# `want`: the property the case is there for, in terms of tile_props() -- asserted by both test files.  A = 7, 6 label columns, vocabulary 30.  The
# video seeds: the first of a walk whose float64 greedy decode has a top-1 / top-2 margin above 3e-4 at every pick (tests/test_sat_edges_host.py).
EDGES = {
    'h4_e': dict(seed=512, feats='E', N=3, D=20, H=4, want=dict(K=4, Dc=0, unit_blocks=1, h_rem=4)),
    'h12_c': dict(seed=511, feats='C', N=3, D=20, H=12, want=dict(K=32, unit_blocks=1, h_rem=12)),
    'k60': dict(seed=517, feats='C', N=3, D=40, H=20, want=dict(K=60, k_chunks=1, unit_blocks=2, h_rem=4)),
    'k64_h20': dict(seed=4119, feats='VEC', N=65, D=44, H=20, want=dict(K=64, k_rem=0, boundary=44, row_tiles=2, h_rem=4, vec_ic=1)),
    'k64_h16': dict(seed=1418, feats='C', N=64, D=48, H=16, want=dict(K=64, k_rem=0, boundary=48, row_tiles=1, last_tile_rows=64, h_rem=0, unit_blocks=1)),
    'k68': dict(seed=1420, feats='C', N=129, D=52, H=16, want=dict(K=68, k_chunks=2, live4=1, col_blocks=2, last_block_cols=4, row_tiles=3, last_tile_rows=1)),
    'k128': dict(seed=414, feats='C', N=5, D=112, H=16, want=dict(K=128, k_chunks=2, k_rem=0, col_blocks=2)),
    'k132': dict(seed=415, feats='C', N=5, D=100, H=32, want=dict(K=132, k_chunks=3, live4=1, col_blocks=3, last_block_cols=4)),
    'k136': dict(seed=1516, feats='VEC', N=63, D=100, H=36, want=dict(K=136, col_blocks=3, h_rem=4, unit_blocks=3, split_block=1, split_datt=36, last_tile_rows=63)),
    've_h64': dict(seed=423, feats='VE', N=5, D=20, H=64, want=dict(K=64, Dc=0, k_rem=0, unit_blocks=4, h_rem=0)),
    've_h68': dict(seed=524, feats='VE', N=5, D=20, H=68, want=dict(K=68, Dc=0, live4=1, unit_blocks=5, h_rem=4, col_blocks=2)),
    'unaligned_h20': dict(seed=422, feats='VEC', N=5, D=44, H=20, opt_over=dict(lda_dim=10), want=dict(K=64, vec_ic=0, h_rem=4)),
    # one decoder step (no caption has a word: the label columns behind <bos> are zero): the reverse recurrence runs on the zero carry only
    's1': dict(seed=421, feats='VEC', N=3, D=40, H=20, cap=0, want=dict(K=60, S=1, h_rem=4)),
    # a non-zero initial state off the unit tile: d h0 = d h(-1) + d c(-1) (sat_add2_kernel) over N * H = 100 elements
    'init_h20': dict(seed=513, feats='VEC', N=5, D=44, H=20, opt_over=dict(CG_init_feats_type='VEC'), want=dict(K=64, h_rem=4, init=1)),
}
# the att | h boundary at every float4 position of a chunk that the table above leaves out (D = 4 .. 64 at H = 20; K = 24 .. 84)
BOUNDARY_SWEEP = [4, 8, 12, 16, 24, 28, 32, 36, 56, 60, 64]
for _d in BOUNDARY_SWEEP:
    EDGES['b%d' % _d] = dict(seed=440 + _d, feats='C', N=3, D=_d, H=20, want=dict(K=_d + 20, boundary=_d % 64, h_rem=4))


@functools.lru_cache(maxsize=None)
def edge_case(name):
    from tests.test_gpu_sat import _edge_case
    e = EDGES[name]
    over = dict(video_dim=e['D'], CG_rnn_size=e['H'])
    over.update(e.get('opt_over', {}))
    return _edge_case(e['feats'], N=e['N'], A=7, L=7, seed=e['seed'], cap=e.get('cap'), opt_over=over)


def tile_props(opt, params, vid):
    """What the cell kernels' grids and guards see of a case."""
    SKC, SUNITS = kernel_constants()
    H, N = opt.CG_rnn_size, len(vid['soi'])
    t = opt.CG_input_feats_type
    Dc = opt.video_dim if 'C' in t else 0
    K = Dc + H
    w_ih = params[LSTM_KEYS[0]]
    ldw = w_ih.shape[1]
    p = dict(K=K, Dc=Dc, H=H, N=N, S=R.O.n_decoder_steps(vid['labels']),
             unit_blocks=-(-H // SUNITS), h_rem=H % SUNITS,                      # forward grid.x; units of a partial last unit block (0: full)
             k_chunks=-(-K // SKC), k_rem=K % SKC,                               # rounds of the forward k loop; floats of a partial last chunk
             live4=(K % SKC) // 4 if K % SKC else SKC // 4,                      # float4s of the last chunk that are inside K
             row_tiles=-(-N // ROWS), last_tile_rows=N - (-(-N // ROWS) - 1) * ROWS,
             col_blocks=-(-K // ROWS), last_block_cols=K - (-(-K // ROWS) - 1) * ROWS,        # reverse grid.x; live columns of its last block
             boundary=Dc % SKC,                                                   # position of the att | h boundary inside its chunk
             split_block=Dc // ROWS, split_datt=Dc % ROWS,                        # the reverse column block with d att AND d h columns: how many d att
             vec_ic=int(Dc > 0 and ldw % 4 == 0 and (ldw - Dc) % 4 == 0),         # the attended-clip columns of W_ih start 16-byte aligned
             init=int(any(k in opt.CG_init_feats_type for k in 'VEC')))
    assert H % 4 == 0 and Dc % 4 == 0 and w_ih.shape[0] == 4 * H
    return p


def check_edge(name):
    """The case has the property it is named for."""
    opt, params, vid = edge_case(name)
    p = tile_props(opt, params, vid)
    for k, v in EDGES[name]['want'].items():
        assert p[k] == v, (name, k, p[k], v)
    assert (opt.video_dim, opt.CG_rnn_size, opt.CG_input_feats_type, len(vid['soi'])) == tuple(EDGES[name][k] for k in ('D', 'H', 'feats', 'N'))
    return p


# ---- 2. trained-weight scales ---------------------------------------------------------------------------------------------------------------
GATES_SAT = dict(embed=10.0, ih=16.0, hh=12.0)
NEG_FAR_TOKEN_ROWS = 6.0          # the token columns of the i, f and o rows of weight_ih, on top of GATES_SAT
H0_TARGET = 12.0                  # state_far: init_linear scaled until max |h(-1)| = max |c(-1)| is this
# variant: base case of synth.SAT_CASES, video overrides (the seeds: the first whose float64 greedy decode is resolvable as the host file asks)
REGIME = {
    'gates_sat_vec': dict(base='sat_vec_init', video=dict(seed=104), scale=GATES_SAT),
    'gates_sat_c': dict(base='sat_c', video=dict(seed=101), scale=GATES_SAT),
    'gates_sat70': dict(base='sat_vec_init', video=dict(seed=104, N=70), scale=GATES_SAT),
    'state_far': dict(base='sat_vec_init', video=dict(seed=104), h0=H0_TARGET),
    'neg_far': dict(base='sat_vec_init', video=dict(seed=104), scale=GATES_SAT, token_rows=NEG_FAR_TOKEN_ROWS),
}


@functools.lru_cache(maxsize=None)
def case(name):
    r = REGIME[name]
    c = synth.SAT_CASES[r['base']]
    opt = synth.default_opt(**c['opt'])
    vd = dict(c['video'], **r['video'])
    vid = synth.make_video(V1=opt.CG_vocab_size + 1, video_dim=opt.video_dim, hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim, **vd)
    params = synth.make_sat_params(opt, 0)
    H, E = opt.CG_rnn_size, opt.CG_input_encoding_size
    s = r.get('scale')
    if s:
        params[R.PRE + 'embed.weight'] = params[R.PRE + 'embed.weight'] * np.float32(s['embed'])
        params[LSTM_KEYS[0]] = params[LSTM_KEYS[0]] * np.float32(s['ih'])
        params[LSTM_KEYS[1]] = params[LSTM_KEYS[1]] * np.float32(s['hh'])
    if r.get('token_rows'):
        w = params[LSTM_KEYS[0]].copy()
        for j in (0, 1, 3):          # i, f, o
            w[j * H:(j + 1) * H, :E] *= np.float32(r['token_rows'])
        params[LSTM_KEYS[0]] = w
    if r.get('h0'):
        P, tap, c3d, lda = R.leaves(params, vid, torch.float64, False)
        with torch.no_grad():
            video, event, clip, _ = R.contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi'])
            top = float(R.init_hidden(P, video, event, clip, opt.CG_init_feats_type)[0].abs().max())
        f = np.float32(r['h0'] / top)
        for k in ('init_linear.weight', 'init_linear.bias'):
            params[R.PRE + k] = params[R.PRE + k] * f
    return opt, params, vid


@contextlib.contextmanager
def one_thread():
    """The float32 runs that e_ref is measured from: one thread, so that the summation order of the host's products does not follow its core count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


@functools.lru_cache(maxsize=None)
def oracle(name, train, f64=True):
    """dict(logp, loss, grads, gtap) of tests/sat_ref.run on the case's float32 inputs, train mode with the build's Philox masks."""
    opt, params, vid = case(name)
    with (contextlib.nullcontext() if f64 else one_thread()):
        logp, loss, grads, gtap = R.run(opt, params, vid, train, dtype=torch.float64 if f64 else torch.float32)
    return dict(logp=logp, loss=loss, grads=grads, gtap=gtap)


def probe(name):
    """The float64 teacher-forced eval pass: (pre-activations [S, N, 4H], new cell states [S, N, H], h(-1) [N, H])."""
    opt, params, vid = case(name)
    R.PROBE = []
    try:
        R.run(opt, params, vid, False, backward=False, dtype=torch.float64)
        pre, c = (np.stack([x[k] for x in R.PROBE]) for k in (0, 1))
    finally:
        R.PROBE = None
    P, tap, c3d, lda = R.leaves(params, vid, torch.float64, False)
    with torch.no_grad():
        video, event, clip, _ = R.contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi'])
        h0 = R.init_hidden(P, video, event, clip, opt.CG_init_feats_type)[0][0].numpy()
    return pre, c, h0


def gate_slices(k, g):
    H = g.shape[0] // 4
    return [('%s[%s]' % (k.split('.')[-1], GATE_NAMES[j]), g[j * H:(j + 1) * H]) for j in range(4)]


def errors(got, ref):
    """(max |d logp|, relative loss error, (worst gradient tensor error, name), (worst gate-slice error, label)) of dict(logp, loss, grads, gtap)
    against a reference one: gradients relative to the reference tensor's (slice's) own max-norm, util.GRAD_FLOOR below it; d tap_feats counts as
    a tensor; sat_ref.NOISE_ONLY left out; a tensor without a gradient in the reference has none, or exact zeros."""
    assert got['logp'].shape == ref['logp'].shape
    e_logp = float(np.abs(got['logp'].astype(np.float64) - ref['logp']).max())
    e_loss = abs(got['loss'] - ref['loss']) / abs(ref['loss'])
    worst, worst_s = (U.relerr(got['gtap'], ref['gtap'], U.GRAD_FLOOR), 'tap_feats'), (0.0, '')
    for k, g in ref['grads'].items():
        if g is None:
            assert got['grads'][k] is None or not np.any(got['grads'][k]), k
            continue
        if k in R.NOISE_ONLY:
            continue
        worst = max(worst, (U.relerr(got['grads'][k], g, U.GRAD_FLOOR), k))
        if k in LSTM_KEYS:
            for (label, gs), (_, rs) in zip(gate_slices(k, got['grads'][k]), gate_slices(k, g)):
                worst_s = max(worst_s, (U.relerr(gs, rs, U.GRAD_FLOOR), label))
    return e_logp, e_loss, worst, worst_s


@functools.lru_cache(maxsize=None)
def e_ref(name):
    """The float32 run of tests/sat_ref.py against the float64 one, the larger of eval and train mode: (logp absolute, loss, gradient tensor, gate slice)."""
    e = [errors(oracle(name, t, False), oracle(name, t, True)) for t in (False, True)]
    return (max(x[0] for x in e), max(x[1] for x in e), max(x[2][0] for x in e), max(x[3][0] for x in e))


def greedy64_of(opt, params, vid):
    """tests/sat_ref.sample in float64: (seq [N, T], sampled log-probs [N, T], margin [N, T], live [N, T]).  live: the pick and every earlier pick of
    the row has a top-1 / top-2 margin above MARGIN -- up to there no route inside the log-prob contract can have walked another way."""
    margins = []
    seq, lp = R.sample(opt, params, vid, torch.float64, margins)
    if len(seq) == 0:          # every row's first pick is <eos>
        N = len(vid['soi'])
        return np.zeros((N, 0), np.int64), np.zeros((N, 0)), np.zeros((N, 0)), np.zeros((N, 0), bool)
    seq, lp = seq.numpy(), lp.numpy()
    mar = np.stack(margins, 1)[:, :seq.shape[1]]
    live = np.logical_and.accumulate(mar > MARGIN, axis=1)
    return seq, lp, mar, live


@functools.lru_cache(maxsize=None)
def greedy64(name):
    return greedy64_of(*case(name))


FAR_STEP, FAR_SEED = 3, 77


@functools.lru_cache(maxsize=None)
def far_state():
    """One get_logprobs_state call of 'state_far' with the cell state far outside (-1, 1): h from the float64 teacher-forced pass in front of step
    FAR_STEP, c from the same pass but for a quarter of the units drawn in +-[9, 20] and 16 exact zeros; both rounded to float32 (what the device is
    handed).  Returns (it [N], (h, c) float32 [1, N, H], float64 log-probs, (h', c') float64, the float32 run's (log-probs, h', c'))."""
    opt, params, vid = case('state_far')
    states = []
    P, tap, c3d, lda = R.leaves(params, vid, torch.float64, False)
    labels = torch.from_numpy(vid['labels'])
    with torch.no_grad():
        video, event, clip, mask = R.contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi'])
        R.decoder_forward(P, video, event, clip, mask, labels, opt.CG_input_feats_type, None, opt.CG_init_feats_type, states)
        h, c = (x.float() for x in states[FAR_STEP - 1])
        rs = np.random.RandomState(FAR_SEED)
        shape = tuple(c.shape)
        far = rs.uniform(9.0, 20.0, shape) * rs.choice([-1.0, 1.0], shape)
        pick = rs.uniform(size=shape) < 0.25
        c = torch.where(torch.from_numpy(pick), torch.from_numpy(far).float(), c)
        flat = c.view(-1)
        flat[torch.from_numpy(rs.choice(flat.numel(), 16, replace=False))] = 0.0
        it = labels[:, FAR_STEP]
        logp, (h2, c2) = R.logprobs_state(P, it, video, event, clip, mask, (h.double(), c.double()), opt.CG_input_feats_type)
        P32, tap32, c3d32, lda32 = R.leaves(params, vid, torch.float32, False)
        with one_thread():
            ctx32 = R.contexts(opt, P32, tap32, c3d32, lda32, vid['ind'], vid['soi'])
            l32, (h32, c32) = R.logprobs_state(P32, it, ctx32[0], ctx32[1], ctx32[2], ctx32[3], (h, c), opt.CG_input_feats_type)
    return it, (h, c), logp.numpy(), (h2.numpy(), c2.numpy()), (l32.numpy(), h32.numpy(), c32.numpy())


def far_step_e_ref():
    """(log-probs, h', c') absolute: the float32 step from far_state() against the float64 one."""
    _, _, logp, (h2, c2), (l32, h32, c32) = far_state()
    return tuple(float(np.abs(a.astype(np.float64) - b).max()) for a, b in ((l32, logp), (h32, h2), (c32, c2)))

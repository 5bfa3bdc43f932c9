"""Inputs and CPU references of the proposal side at TRAINED-WEIGHT scales (tests/test_proposal_regime_host.py, tests/test_gpu_proposal_regime.py):

  1. the criterion on PLANTED scores (exactly 0 and 1, the neighbours of 1, a denormal, values on both sides of the 1e-12 floor of torch's
     BCELoss backward), each under label 0 / 1 and mask 1 / 0 -- reference: oracle.tap_criterion in float64 on the same float32 inputs;
  2. the encoder VARIANTS: tests/sst_batch_ref.make_params scaled to saturated gates / drifting cell states / a head whose logits reach +-12
     -- reference: oracle.sst_forward in float64, once per video (tests/sst_batch_ref.run);
  3. score grids drawn with heavy repetition from 1.0, its two float32 predecessors, 0.5, 2^-126, a denormal and 0.0 for the selection.
"""
import functools

import numpy as np
import torch

from oracle import echr_ref_cpu as O
from tests import sst_batch_ref as R
from tests import util as U

# ---- 1. the criterion ---------------------------------------------------------------------------------------------------------------
# 1e-40: a float32 denormal, log = -92.1 (not clamped: a kernel that flushes it to zero shows); 1e-45 (the smallest denormal): log = -103.3, the
# clamp is live; 9e-13 / 1.1e-12: the two sides of the 1e-12 floor of p (1 - p)
PLANTED = np.array([0.0, 1.0, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -23, 1e-40, 1e-45, 1e-30, 1e-20, 1e-13, 9e-13, 1.1e-12, 1e-11], np.float32)
PLANT = [(s, y, m) for s in PLANTED for y in (0.0, 1.0) for m in (1.0, 0.0)]          # (score, label, mask): 48 elements
G_LOSS = 0.37
TOL_ELEM = 1e-5          # |got - ref| <= 1e-5 |ref| + 1e-30 on EVERY gradient element (the elements span 1e-9 .. 1e12)


def bce_inputs(lengths, K, per_video=False, plant='all', seed=0):
    """dict(ro, scores, masks, labels [T_tot, K], w1 [V or 1, K]).  plant='all': the 48 PLANT elements (cut to T_tot * K) spread evenly over
    the batch's elements; an integer i: PLANT[i] alone in element 0; None: nothing planted.  Everything else is uniform(0.02, 0.98) under the
    causal mask of each video."""
    lengths = tuple(int(t) for t in lengths)
    rs = np.random.RandomState(1000 * seed + 7 * sum(lengths) + K + len(lengths))
    ro = R.offsets(lengths)
    T, V = ro[-1], len(lengths)
    scores = rs.uniform(0.02, 0.98, size=(T, K)).astype(np.float32)
    labels = (rs.uniform(size=(T, K)) > 0.8).astype(np.float32)
    masks = np.concatenate([(np.arange(t)[:, None] >= np.arange(K)[None, :]).astype(np.float32) for t in lengths], 0)
    w1 = rs.uniform(0.05, 0.3, size=(V if per_video else 1, K)).astype(np.float32)
    n = T * K
    items = [] if plant is None else (PLANT[:n] if plant == 'all' else [PLANT[plant]])
    pos = (np.arange(len(items)) * n) // max(len(items), 1)
    for p, (s, y, m) in zip(pos, items):
        scores.reshape(-1)[p], labels.reshape(-1)[p], masks.reshape(-1)[p] = s, y, m
    return dict(ro=ro, scores=scores, masks=masks, labels=labels, w1=w1, per_video=per_video, planted=pos)


def bce_reference(inp, g_loss=G_LOSS):
    """oracle.tap_criterion in float64, once per video: (losses [V], d (g_loss * sum of the losses) / d scores [T_tot, K]), both float64."""
    ro, losses, g = inp['ro'], [], []
    for v, (a, b) in enumerate(zip(ro[:-1], ro[1:])):
        s = torch.from_numpy(inp['scores'][a:b]).double().requires_grad_(True)
        w1 = torch.from_numpy(inp['w1'][v if inp['per_video'] else 0]).double()
        loss = O.tap_criterion(s, torch.from_numpy(inp['masks'][a:b]).double(), torch.from_numpy(inp['labels'][a:b]).double(), w1)
        (g_loss * loss).backward()
        losses.append(float(loss.detach()))
        g.append(s.grad.numpy())
    return np.asarray(losses), np.concatenate(g, 0)


def elem_ratio(got, ref):
    """max over the elements of |got - ref| / (|ref| + 1e-30 / TOL_ELEM): <= TOL_ELEM is the gradient gate."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (np.abs(ref) + 1e-30 / TOL_ELEM)).max())


# ---- 2. the encoder -----------------------------------------------------------------------------------------------------------------
# scale factors on make_params' tensors (uniform(-1, 1) / sqrt(H)); `forget` is added to the forget slice [H, 2H) of both layers' bias_ih;
# `lengths` is the batch, video `single` of it (the longest) is also run alone
VARIANTS = {
    'gates_sat': dict(D=500, H=512, K=16, w_ih=8.0, w_hh=4.0, head=30.0, forget=1.0, lengths=(1, 2, 40, 17, 40), single=2, loss='sums'),
    'drift': dict(D=500, H=512, K=16, w_ih=4.0, w_hh=2.0, head=10.0, forget=6.0, lengths=(1, 2, 100, 17), single=2, loss='sums'),
    'bce_chain': dict(D=500, H=512, K=16, w_ih=8.0, w_hh=4.0, head=20.0, forget=1.0, lengths=(1, 2, 40, 17, 40), single=2, loss='bce'),
    'small_h': dict(D=20, H=24, K=8, w_ih=8.0, w_hh=4.0, head=30.0, forget=1.0, lengths=(1, 2, 12, 5), single=2, loss='sums'),
}
TAP_WEIGHT = 0.1          # bce_chain: loss = criterion + 0.1 (tap * wt).sum()
SEED = 45                 # of the parameters and inputs of every variant: with it bce_chain's largest |head logit| over its batch is 12.5 (float64 oracle)


@functools.lru_cache(maxsize=None)
def make_variant(name):
    """(spec, params, inputs): inputs = dict(x, wt, ws, ro, masks, labels, w1) over the variant's batch; read-only, shared."""
    spec = VARIANTS[name]
    D, H, K = spec['D'], spec['H'], spec['K']
    rs = np.random.RandomState(SEED)
    params = R.make_params(rs, D, H, K)
    for l in (0, 1):
        params['rnn.weight_ih_l%d' % l] *= np.float32(spec['w_ih'])
        params['rnn.weight_hh_l%d' % l] *= np.float32(spec['w_hh'])
        params['rnn.bias_ih_l%d' % l][H:2 * H] += np.float32(spec['forget'])
    params['scores.weight'] *= np.float32(spec['head'])
    params['scores.bias'] *= np.float32(spec['head'])
    x, wt, ws, ro = R.make_inputs(rs, spec['lengths'], D, H, K)
    masks = np.concatenate([(np.arange(t)[:, None] >= np.arange(K)[None, :]).astype(np.float32) for t in spec['lengths']], 0)
    labels = (rs.uniform(size=masks.shape) > 0.8).astype(np.float32)
    w1 = rs.uniform(0.05, 0.3, size=K).astype(np.float32)
    return spec, params, dict(x=x, wt=wt, ws=ws, ro=ro, masks=masks, labels=labels, w1=w1)


def rows(name, batch):
    """(first row, row offsets) of the run: the whole batch, or video `single` of it alone."""
    spec, _, inp = make_variant(name)
    if batch:
        return 0, list(inp['ro'])
    a, b = inp['ro'][spec['single']], inp['ro'][spec['single'] + 1]
    return a, [0, b - a]


def oracle(name, train, batch, dtype=torch.float64):
    """tests/sst_batch_ref.run on the variant: dict(tap, scores, grads, loss).  The single-video run draws its own dropout mask (rows 0 .. T of a
    [T, H] call), as SST.forward on that video does.  bce_chain differentiates criterion + TAP_WEIGHT (tap * wt).sum() and reports the criterion
    (the sum of the videos' losses): the signed tap term cancels, so the relative error of the whole would measure that cancellation."""
    spec, params, inp = make_variant(name)
    r0, ro = rows(name, batch)
    sl = slice(r0, r0 + ro[-1])
    x, wt, ws, mk, lb = (inp[k][sl] for k in ('x', 'wt', 'ws', 'masks', 'labels'))
    loss = None
    if spec['loss'] == 'bce':
        c = lambda t: torch.from_numpy(t).to(dtype)

        def loss(v, a, b, tap, sc):
            crit = O.tap_criterion(sc, c(mk[a:b]), c(lb[a:b]), c(inp['w1']))
            return crit + TAP_WEIGHT * (tap * c(wt[a:b])).sum(), crit
    return R.run(params, x, wt, ws, ro, train, dtype=dtype, loss=loss)


@functools.lru_cache(maxsize=None)
def oracle64(name, train, batch):
    return oracle(name, train, batch, torch.float64)


def errors(got, ref):
    """(max |d tap|, max |d scores|, relative loss error, worst gradient tensor relative to its max-norm, its name)."""
    worst = max((U.relerr(got['grads'][k], g, U.GRAD_FLOOR), k) for k, g in ref['grads'].items())
    return (float(np.abs(got['tap'] - ref['tap']).max()), float(np.abs(got['scores'] - ref['scores']).max()),
            abs(got['loss'] - ref['loss']) / abs(ref['loss']), worst[0], worst[1])


def e_ref(name, train, batch):
    """The float32 oracle (the reference's own arithmetic) against the float64 oracle on the same inputs."""
    return errors(oracle(name, train, batch, torch.float32), oracle64(name, train, batch))


def probe(name, batch=False):
    """The float64 oracle's eval-mode forward of video `single` (or of every video of the batch), with every layer's gate activations and cell
    states recorded: dict(gates [2][rows, 3H] = i | f | o, c [2][rows, H], z [rows, K] head logits, scores32 = the float32 oracle's scores)."""
    spec, params, inp = make_variant(name)
    r0, ro = rows(name, batch)
    rec = []
    orig = O.lstm_cell

    def spy(xt, h, c, w_ih, w_hh, b_ih, b_hh):
        g = torch.nn.functional.linear(xt, w_ih, b_ih) + torch.nn.functional.linear(h, w_hh, b_hh)
        i, f, _, o = g.chunk(4, 1)
        h2, c2 = orig(xt, h, c, w_ih, w_hh, b_ih, b_hh)
        rec.append((torch.sigmoid(torch.cat([i, f, o], 1)).numpy(), c2.numpy()))
        return h2, c2
    out = dict(gates=[[], []], c=[[], []], z=[], scores32=[])
    P64 = {k: torch.from_numpy(v).double() for k, v in params.items()}
    P32 = {k: torch.from_numpy(v) for k, v in params.items()}
    for a, b in zip(ro[:-1], ro[1:]):
        x = torch.from_numpy(inp['x'][r0 + a:r0 + b])
        del rec[:]
        O.lstm_cell = spy
        try:
            with torch.no_grad():
                tap, _ = O.sst_forward(P64, x.double())
        finally:
            O.lstm_cell = orig
        with torch.no_grad():
            out['z'].append(torch.nn.functional.linear(tap, P64['scores.weight'], P64['scores.bias']).numpy())
            out['scores32'].append(O.sst_forward(P32, x)[1].numpy())
        T = b - a
        for l in (0, 1):          # sst_forward runs layer 0 over all T steps, then layer 1
            out['gates'][l] += [r[0] for r in rec[l * T:(l + 1) * T]]
            out['c'][l] += [r[1] for r in rec[l * T:(l + 1) * T]]
    return dict(gates=[np.concatenate(g, 0) for g in out['gates']], c=[np.concatenate(c, 0) for c in out['c']],
                z=np.concatenate(out['z'], 0), scores32=np.concatenate(out['scores32'], 0))


# ---- 3. the selection ---------------------------------------------------------------------------------------------------------------
ONE, PRED = np.float32(1.0), np.float32(1.0 - 2.0 ** -24)          # 0x3F800000 and 0x3F7FFFFF: keys that differ in all four radix digits
PRED2 = np.float32(1.0 - 2.0 ** -23)                               # 0x3F7FFFFE: differs from PRED in the last bit, so the LAST radix pass decides
CLASSES = np.array([ONE, PRED, PRED2, 0.5, 2.0 ** -126, 1e-40, 0.0], np.float32)
I_DENORMAL = 5


def saturated_grid(T, K, seed=0, p=(0.25, 0.2, 0.15, 0.15, 0.1, 0.1, 0.05)):
    """[T, K] float32 scores drawn from CLASSES with probabilities p."""
    rs = np.random.RandomState(seed + 31 * T + K)
    return CLASSES[rs.choice(len(CLASSES), size=(T, K), p=p)]


def class_counts(scores):
    """Number of causal cells (n >= k) of every class, in CLASSES' (descending) order."""
    T, K = scores.shape
    causal = np.arange(T)[:, None] >= np.arange(K)[None, :]
    return [int((causal & (scores.view(np.uint32) == c.view(np.uint32))).sum()) for c in CLASSES.reshape(-1, 1)]

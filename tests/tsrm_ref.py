"""Reference side of the event-encoder route tests (CPU only; tests/test_tsrm_ref_host.py, tests/test_gpu_tsrm_routes.py and
tools/parity_report.py --tsrm share it).

The event-relation encoder (csrc/tsrm.hip) is compared against oracle.echr_ref_cpu.tsrm_forward carried out in float64 on the same
float32 inputs and the same dropout masks.  This module holds the inputs (parameters of any widths, event lists, event features), that
float64 run with its gradients, the position embedding on its own, a numpy transcription of the device's sin / cos helper, and the table of
cases with the conditions each case has to satisfy (checked on the float64 reference alone by the host test).
"""
import math

import numpy as np
import torch

from echr_amd import philox
from oracle import echr_ref_cpu as O

PREFIX = 'fusion_model.'
# the order of echr_tsrm_args / echr_tsrm_grads (echr_amd.functional.TSRM_PARAMS): w_emb, b_emb, w_fc1, b_fc1, w_fc2, b_fc2, w_q, b_q, w_k, b_k, w_out, b_out
NAMES = tuple(PREFIX + n for n in (
    'event_emb.weight', 'event_emb.bias', 'enc_attn.pair_pos_fc1.weight', 'enc_attn.pair_pos_fc1.bias',
    'enc_attn.pair_pos_fc2.weight', 'enc_attn.pair_pos_fc2.bias', 'enc_attn.query_1.weight', 'enc_attn.query_1.bias',
    'enc_attn.key_1.weight', 'enc_attn.key_1.bias', 'enc_attn.linear_out_1.weight', 'enc_attn.linear_out_1.bias'))
FC2_BIAS = PREFIX + 'enc_attn.pair_pos_fc2.bias'
FST = ('fST0', 'fST1', 'fST2', 'fST3')          # fst_mode 0..3; 4 = use_posit = 0
# what a combination does not reach (no gradient): fST3 ignores the affinities, use_posit = 0 the position MLP
UNREACHED = {3: NAMES[6:10], 4: NAMES[2:6]}
P_DROP = 0.3
SEED, OFFSET = 0x5EED0123456789, 7          # the dropout stream of tests/util.py


def shapes(Din, Df, Do, G):
    return dict(zip(NAMES, ((Df, Din), (Df,), (Df, Df), (Df,), (G, Df), (G,), (Df, Df), (Df,), (Df, Df), (Df,), (Do, Df, 1, 1), (Do,))))


def make_params(Din, Df, Do, G, seed, gate_shift=0.0, qk_scale=1.0):
    """The twelve fusion_model.* tensors (float32), uniform +-1/sqrt(fan_in), drawn in sorted-name order from one RandomState.
    gate_shift: the two halves of pair_pos_fc2.bias moved by +-shift (synth.make_case does the same for 'fst2'); qk_scale multiplies
    query_1.weight and key_1.weight (the affinities grow by its square)."""
    rs = np.random.RandomState(seed)
    shp = shapes(Din, Df, Do, G)
    out = {}
    for name in sorted(shp):
        wname = name[:-len('.bias')] + '.weight' if name.endswith('.bias') else name
        r = 1.0 / math.sqrt(int(np.prod(shp[wname][1:])))
        out[name] = rs.uniform(-r, r, size=shp[name]).astype(np.float32)
    if gate_shift:
        b = out[FC2_BIAS]
        b[:len(b) // 2] += np.float32(gate_shift)
        b[len(b) // 2:] -= np.float32(gate_shift)
    if qk_scale != 1.0:
        for n in (NAMES[6], NAMES[8]):
            out[n] = (out[n] * np.float32(qk_scale)).astype(np.float32)
    return out


def make_events(N, T_v, max_len, seed):
    """int64 [N, 2] half-open [start, end) inside T_v rows, lengths 1..max_len (max_len >= 3).  Event 0 has length 1 (N = 1), otherwise
    length 3 with event 1 of length 1 on its middle row: two events with equal centres (the 1e-3 floor of dc) and an event of length 1."""
    assert max_len >= 3 and T_v >= max_len
    rs = np.random.RandomState(seed)
    ln = rs.randint(1, max_len + 1, size=N)
    st = np.array([rs.randint(0, T_v - l + 1) for l in ln])
    if N == 1:
        ln[0] = 1
        st[0] = min(st[0], T_v - 1)
    else:
        ln[0], ln[1] = 3, 1
        st[0] = min(st[0], T_v - 3)
        st[1] = st[0] + 1
    return np.stack([st, st + ln], 1).astype(np.int64)


def make_ech(N, Din, seed):
    return np.random.RandomState(seed).standard_normal((N, Din)).astype(np.float32)


def out_weight(N, Do):
    """The fixed w of the scalar (out * w).sum() whose gradients are compared (d out = w)."""
    return np.random.RandomState(4242).uniform(-1.0, 1.0, size=(N, Do)).astype(np.float32)


def drop_mask(N, G):
    """The device's mask of the post-softmax dropout: element (n, g, j) of one [N, G, N] Philox draw (batch-global n, j in a batch)."""
    return philox.scale_mask((N, G, N), P_DROP, SEED, OFFSET, philox.SITE_TSRM, 0)


def run(params, ech, soi, G, mode, drop_mask, vid=None, dtype=torch.float64):
    """(out [N, Do], d ech [N, Din], {name: gradient or None}) of (out * w).sum(), w = out_weight, through oracle.tsrm_forward in `dtype`.
    vid (int [N], non-decreasing): one call per video, rows concatenated; video v sees the block drop_mask[rows_v][:, :, rows_v]."""
    P = {k: torch.from_numpy(np.ascontiguousarray(params[k])).to(dtype).requires_grad_(True) for k in NAMES}
    x = torch.from_numpy(np.ascontiguousarray(ech)).to(dtype).requires_grad_(True)
    soi = np.asarray(soi, dtype=np.int64)
    N = x.shape[0]
    kw = dict(fST_type=FST[mode], use_posit=1) if mode < 4 else dict(use_posit=0)
    dm = None if drop_mask is None else torch.from_numpy(np.ascontiguousarray(drop_mask)).to(dtype)
    vid = np.zeros(N, np.int64) if vid is None else np.asarray(vid, dtype=np.int64)
    outs = []
    for v in np.unique(vid):
        rows = torch.from_numpy(np.nonzero(vid == v)[0])
        m = None if dm is None else dm[rows][:, :, rows]
        outs.append(O.tsrm_forward(P, x[rows], soi[rows.numpy()], G, m, **kw))
    out = torch.cat(outs, 0)
    w = torch.from_numpy(out_weight(N, out.shape[1])).to(dtype)
    (out * w).sum().backward()
    grads = {k: (p.grad.numpy().copy() if p.grad is not None else None) for k, p in P.items()}
    return out.detach().numpy().copy(), x.grad.numpy().copy(), grads


def probe(params, ech, soi, G, mode):
    """float64: (gate [N, G, N] of the position MLP, softmax weights [N, G, N]) of a single-video call."""
    P = {k: torch.from_numpy(np.ascontiguousarray(params[k])).double() for k in NAMES}
    rec = {}
    orig = torch.softmax

    def spy(x, dim):
        rec['w'] = orig(x, dim)
        return rec['w']
    torch.softmax = spy
    try:
        with torch.no_grad():
            kw = dict(fST_type=FST[mode], use_posit=1) if mode < 4 else dict(use_posit=0)
            O.tsrm_forward(P, torch.from_numpy(ech).double(), np.asarray(soi), G, None, **kw)
    finally:
        torch.softmax = orig
    N = len(soi)
    with torch.no_grad():
        Df = P[NAMES[2]].shape[1]
        pos = torch.from_numpy(O.position_embedding(O.position_matrix(np.asarray(soi)), Df)).float().double().view(N * N, Df)
        p1 = torch.tanh(pos @ P[NAMES[2]].t() + P[NAMES[3]])
        gate = (p1 @ P[NAMES[4]].t() + P[NAMES[5]]).view(N, N, G).transpose(1, 2)
    return gate.numpy(), rec['w'].numpy()


def posemb(soi, Df):
    """float64 [N, N, Df]: the formula of oracle.position_embedding with dl the float32 value csrc/tsrm.hip documents -- the correctly
    rounded float32 log of the float32 quotient l_j / l_i."""
    soi = np.asarray(soi, dtype=np.int64)
    start, end = soi[:, 0:1], soi[:, 1:2]
    center = 0.5 * (start + end)
    length = (end - start).astype(np.float32)
    dc = np.maximum(np.abs((center - center.T) / length), 1e-3)
    ratio = (length.T / length).astype(np.float32)
    dl = np.log(ratio.astype(np.float64)).astype(np.float32).astype(np.float64)
    return O.position_embedding(np.concatenate((dc[:, :, None], dl[:, :, None]), axis=2), Df)


def _fma64(a, b, c):
    """a * b + c with the product carried exactly (Dekker's split): what the device's float64 fma returns, to the last bit or so."""
    p = a * b
    s = 134217729.0          # 2^27 + 1
    ah = a * s; ah = ah - (ah - a); al = a - ah
    bh = b * s; bh = bh - (bh - b); bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return (p + c) + e


def sincos_f64arg_np(x):
    """csrc/tsrm.hip's sincos_f64arg line by line: quadrant reduction in float64 (two-term pi / 2), the degree-9 / degree-10 polynomials in
    float32 (numpy rounds every float32 operation; the device may contract a * b + c into one rounding)."""
    x = np.asarray(x, dtype=np.float64)
    f = np.float32
    q = np.rint(x * 0.6366197723675814)
    r = _fma64(-q, 6.123233995736766e-17, _fma64(-q, 1.5707963267948966, x)).astype(np.float32)
    r2 = r * r
    sp = r + r * r2 * (f(-1.6666667e-1) + r2 * (f(8.3333333e-3) + r2 * (f(-1.9841270e-4) + r2 * f(2.7557319e-6))))
    cp = f(1.0) + r2 * (f(-0.5) + r2 * (f(4.1666667e-2) + r2 * (f(-1.3888889e-3) + r2 * (f(2.4801587e-5) + r2 * f(-2.7557319e-7)))))
    n = q.astype(np.int64) & 3
    ss = np.where(n & 1, cp, sp)
    cs = np.where(n & 1, sp, cp)
    s = np.where(n & 2, -ss, ss)
    c = np.where((n + 1) & 2, -cs, cs)
    return s.astype(np.float32), c.astype(np.float32)


# ---- the widths and the cases of tests/test_gpu_tsrm_routes.py ---------------------------------------------------------------------------
DIN = 12
WIDTHS = {           # Df, Do, G
    'S': (64, 64, 2),            # head dim 32: fused heads for N <= 64; posemb_rows
    'ODD': (48, 24, 4),          # head dim 12: general route at any N; Df / 4 = 12: posemb_kernel, one partial chunk; Do != Df: ungrouped projections
    'ODD2': (80, 80, 4),         # Df / 4 = 20: posemb_kernel, two chunks, the second partial
    'H256': (256, 256, 8),       # fused heads; skinny_nt<16>; pair_gate<16>; h2 fc1 from the fp32 embedding (no packed form)
    'FULL': (512, 512, 16),      # the model's widths
}
T_V, MAX_LEN = 40, 8
PEAK_SCALES = (8.0, 10.0, 12.0, 14.0, 16.0, 18.0, 20.0, 24.0, 28.0, 32.0)          # qk_scale of a peaked case: the first of these that meets PEAK_MEDIAN (host test)
PEAK_MEDIAN = 0.9
FST2_BAND = (1e-6, 0.05)


def _case(name, width, counts, mode=0, train=True, zeroed=0, inference=0, gate_shift=0.0, qk_scale=1.0, peaked=False):
    counts = (counts,) if isinstance(counts, int) else tuple(counts)
    return name, dict(name=name, width=width, counts=counts, N=sum(counts), mode=mode, train=train, zeroed=zeroed, inference=inference,
                      gate_shift=gate_shift, qk_scale=qk_scale, peaked=peaked, backward=not inference)


# qk_scale of the peaked cases, chosen on the float64 reference (the smallest of PEAK_SCALES with a median top weight >= PEAK_MEDIAN;
# test_tsrm_ref_host.py::test_peaked_scales_are_the_smallest_that_qualify re-derives every one)
PEAK_QK = {('S', 33, 0): 16.0, ('S', 65, 0): 18.0, ('S', 130, 0): 18.0, ('S', 33, 1): 10.0, ('S', 65, 1): 12.0, ('S', 130, 1): 12.0,
           ('FULL', 64, 0): 16.0}


def _cases():
    c = []
    # 1. routes at their N boundaries (train mode, dropout, fST0)
    for N in (1, 2, 33, 63, 64, 65, 127, 128, 130):
        c.append(_case('route-S-%d' % N, 'S', N))
    for N in (1, 5, 70):
        c.append(_case('route-ODD-%d' % N, 'ODD', N))
    c.append(_case('route-ODD2-9', 'ODD2', 9))
    for N in (31, 32, 66):
        c.append(_case('route-H256-%d' % N, 'H256', N))
    for N in (6, 66):
        for z in (0, 1):
            c.append(_case('route-FULL-%d-z%d' % (N, z), 'FULL', N, zeroed=z))
    c.append(_case('route-FULL-130-z1', 'FULL', 130, zeroed=1))
    # 2. every combinator on every route
    for N in (33, 65, 130):
        for mode in range(5):
            # (modes 3 / 4 accumulate, zeroed = 1: what the combination does not reach then keeps a sentinel bit for bit)
            c.append(_case('fst%d-S-%d' % (mode, N), 'S', N, mode=mode, gate_shift=1.0 if mode == 2 else 0.0, zeroed=1 if mode >= 3 else 0))
    # 3. peaked softmaxes
    for train in (False, True):
        for (width, N, mode), s in sorted(PEAK_QK.items()):
            c.append(_case('peak-%s-%d-fst%d-%s' % (width, N, mode, 'train' if train else 'eval'), width, N, mode=mode, train=train, qk_scale=s, peaked=True))
    # 4. multi-video batches
    for counts in ((20, 13), (1, 40, 24), (64, 1, 65)):
        for mode in (0, 2):
            c.append(_case('batch-%s-fst%d' % ('_'.join(map(str, counts)), mode), 'S', counts, mode=mode, gate_shift=1.0 if mode == 2 else 0.0))
    # 5. inference tables
    for width in ('FULL', 'H256'):
        c.append(_case('tables-%s-130' % width, width, 130, train=False, inference=1))
    return dict(c)


CASES = _cases()


def case_inputs(spec):
    """(params, ech [N, Din], soi [N, 2], vid [N] or None, drop mask [N, G, N] or None) of a case."""
    Df, Do, G = WIDTHS[spec['width']]
    N = spec['N']
    seed = 100 + N + 7 * spec['mode']
    params = make_params(DIN, Df, Do, G, seed, spec['gate_shift'], spec['qk_scale'])
    soi = np.concatenate([make_events(n, T_V, MAX_LEN, seed + 31 * v) for v, n in enumerate(spec['counts'])], 0)
    vid = np.repeat(np.arange(len(spec['counts'])), spec['counts']) if len(spec['counts']) > 1 else None
    ech = make_ech(N, DIN, seed + 1)
    return params, ech, soi, vid, (drop_mask(N, G) if spec['train'] else None)


def reference(spec, dtype=torch.float64):
    params, ech, soi, vid, dm = case_inputs(spec)
    return run(params, ech, soi, WIDTHS[spec['width']][2], spec['mode'], dm, vid, dtype)


def bounds(soi):
    """(max_len, max_span) as echr_amd.functional.event_index_tensors derives them."""
    soi = np.asarray(soi, dtype=np.int64)
    ln = soi[:, 1] - soi[:, 0]
    c2 = 2 * soi[:, 0] + ln
    return int(ln.max()), int(c2.max() - c2.min())


def rel(a, b, floor=0.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor, 1e-30))


def noise_only(spec):
    """Parameters whose true gradient is exactly zero, so that both sides hold rounding noise only (the softmax is invariant under a shift
    of a whole row): pair_pos_fc2.bias where the gate enters additively (fST1, fST3; tests/test_gpu_timed_path.py), key_1.bias where the
    affinity does (fST1, fST2, use_posit = 0: the bias adds q_n . b_k to every entry of row n)."""
    return ((FC2_BIAS,) if spec['mode'] in (1, 3) else ()) + ((NAMES[9],) if spec['mode'] in (1, 2, 4) else ())


def e_ref(spec, grad_floor=1e-5):
    """(out, worst gradient incl. d ech, its name, noise): float32 oracle against float64 oracle, each tensor relative to the float64
    max-norm; noise = the largest absolute value either oracle holds in a noise_only tensor."""
    o64, x64, g64 = reference(spec, torch.float64)
    o32, x32, g32 = reference(spec, torch.float32)
    worst = (rel(x32, x64, grad_floor), 'd ech')
    noise = 0.0
    if spec['backward']:
        for k, g in g64.items():
            if g is not None and k not in noise_only(spec):
                worst = max(worst, (rel(g32[k], g, grad_floor), k))
        for k in noise_only(spec):
            assert float(np.abs(g64[k]).max()) < 1e-12, (k, np.abs(g64[k]).max())
            noise = max(noise, float(np.abs(g32[k]).max()))
    return rel(o32, o64), worst[0], worst[1], noise

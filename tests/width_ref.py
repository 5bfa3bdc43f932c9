"""CPU side of the decoder-width tests (tests/test_gpu_decoder_widths.py): the case table, the float64 / float32 oracles, the error measures
(per tensor and per slice of the varied axis) and the two mutants that tests/test_width_ref_host.py uses.  Pure CPU (numpy / torch).

The decoder kernels dispatch on width (csrc/decoder.hip):
    R  = ceil(Ha / 256) in 1..4     att_score_kernel<R, SLOTS>, att_post_kernel<R>, att_bwd_kernel<R, RD, SLOTS>
    RD = ceil(D / 256) in 1..4      att_bwd_kernel<R, RD, SLOTS>
    SLOTS in {2, 4, 8}              the att_slots switch; a chunk of att_score / att_bwd / dq_fold is 4 * SLOTS slots, of att_post 8 slots
and every instantiation loads its rows with clamped addresses and masks the duplicated lanes.  The persistent recurrences (csrc/persist.hip)
take H = Ha = 512 with any D in [8, 512], D % 4 == 0, zero-padded to 512 in groups of 8 columns, 16 groups per wave.

A case fixes the widths D / Ha / H / E (video_dim, CG_att_hid_size, CG_rnn_size, CG_input_encoding_size), the planted event lengths and the
row layout; the event encoder keeps the widths of synth.CASES['tiny'] (d_feats = d_o = 32, n_head = 4, hidden_dim = 24, lda_dim = 12), the
vocabulary is V1 = 31 and the label width L = 5.  Parameters are synth.make_params(opt, 3); the video is synth.make_video with its event
intervals overwritten."""
import functools

import numpy as np
import torch

from echr_amd import synth
from tests import clipctx_ref as R
from tests import sat_ref as SR
from tests import util as U

ENCODER = dict(d_feats=32, d_o=32, n_head=4, hidden_dim=24, lda_dim=12)
V1, L = 31, 5
PARAM_SEED = 3
LENS = (1, 5, 9)                                  # groups A, C, D, E, F: A = 9
SLOT_LENS = (1, 7, 8, 9, 31, 32, 33, 65)          # group B: A = 65
BIG_LENS = (130, 1, 44)                           # group D, the BIG instantiations of the persistent kernels: A = 130
SLOTS = (2, 4, 8)

HA_VALUES = (4, 252, 256, 260, 508, 516, 768, 772, 1020, 1024)
D_VALUES = (4, 124, 132, 256, 260, 500, 516, 768, 772, 1024)
HE_VALUES = ((4, 4), (36, 20), (60, 16), (132, 132), (260, 4))
# both sides of K = 4H = 32, below which the three accumulating d XT products of the backward run one behind the other (csrc/decoder.hip)
HE_EXTRA = ((8, 8), (12, 12))
PERSIST_D = (8, 12, 124, 128, 132, 256, 260, 388, 508, 512)
REC_TILE, REC_KSLICE = 64, 128                    # rec_gemm_kernel: Nout tile, k slice
CTX_CHUNK = 128                                   # att_context_kernel: column chunk
PH = 512                                          # the persistent kernels' H = Ha

# (Ha, D) of group A: every (R, RD) pair, every listed value
_A_PAIRS = ((4, 4), (252, 260), (256, 516), (256, 772),
            (260, 124), (260, 500), (508, 768), (508, 1024),
            (516, 132), (516, 260), (768, 516), (516, 772),
            (772, 256), (1020, 500), (772, 516), (1024, 1024),
            (1020, 4), (4, 1024))


def _table():
    t = {}
    seed = 500
    for ha, d in _A_PAIRS:
        seed += 1
        t['a_ha%d_d%d' % (ha, d)] = dict(group='A', D=d, Ha=ha, H=32, E=16, lens=LENS, T_v=16, seed=seed)
    for d, ha in ((20, 24), (516, 260)):
        for layout in ('shared', 'disjoint'):
            seed += 1
            # shared: 186 slots on 80 rows, so events overlap (atomic adds; dpall_fold under fixed order); disjoint: back to back, 186 rows
            t['b_d%d_ha%d_%s' % (d, ha, layout)] = dict(group='B', D=d, Ha=ha, H=32, E=16, lens=SLOT_LENS, layout=layout,
                                                       T_v=80 if layout == 'shared' else sum(SLOT_LENS), seed=seed)
    for h, e in HE_VALUES:
        seed += 1
        t['c_h%d_e%d' % (h, e)] = dict(group='C', D=20, Ha=24, H=h, E=e, lens=LENS, T_v=16, seed=seed)
    for d in PERSIST_D:
        seed += 1
        t['d_d%d' % d] = dict(group='D', D=d, Ha=PH, H=PH, E=16, lens=LENS, T_v=16, seed=seed)
    t['d_d512_e512'] = dict(group='D', D=512, Ha=PH, H=PH, E=512, lens=LENS, T_v=16, seed=seed + 1)
    t['d_d12_big'] = dict(group='D', D=12, Ha=PH, H=PH, E=16, lens=BIG_LENS, T_v=136, seed=seed + 2)
    t['d_d512_big'] = dict(group='D', D=512, Ha=PH, H=PH, E=16, lens=BIG_LENS, T_v=136, seed=seed + 3)
    # group F: the one-stream decoder (input [token | video | event | attended clip]) and the decoding case
    t['f_sat_d260_ha252'] = dict(group='F', D=260, Ha=252, H=32, E=16, lens=LENS, T_v=16, seed=seed + 4, sat=True)
    t['f_sat_d772_ha516'] = dict(group='F', D=772, Ha=516, H=32, E=16, lens=LENS, T_v=16, seed=seed + 5, sat=True)
    t['f_dec_d260_ha252'] = dict(group='F', D=260, Ha=252, H=36, E=20, lens=LENS, T_v=16, seed=seed + 6)
    for i, (h, e) in enumerate(HE_EXTRA):
        t['c_h%d_e%d' % (h, e)] = dict(group='C', D=20, Ha=24, H=h, E=e, lens=LENS, T_v=16, seed=seed + 7 + i)
    return t


CASES = _table()
GROUP = {g: [k for k, c in CASES.items() if c['group'] == g] for g in 'ABCDF'}
ONE_CALL = ('a_ha772_d516', 'c_h132_e132', 'd_d12')          # group E
MUTATED = GROUP['A'] + GROUP['B'] + GROUP['D']
PERSIST_BIG = ('d_d12_big', 'd_d512_big')


def dispatch(c):
    """(R, RD) of a case."""
    return (c['Ha'] + 255) // 256, (c['D'] + 255) // 256


def is_sat(name):
    return bool(CASES[name].get('sat'))


@functools.lru_cache(maxsize=None)
def case(name):
    """(opt, params, video) of a CASES entry.  The returned arrays are shared: do not write to them."""
    c = CASES[name]
    over = dict(ENCODER, video_dim=c['D'], CG_att_hid_size=c['Ha'], CG_rnn_size=c['H'], CG_input_encoding_size=c['E'],
                CG_vocab_size=V1 - 1, CG_seq_length=L - 2)
    if c.get('sat'):
        over.update(caption_model='show_attend_tell', CG_num_layers=1, CG_input_feats_type='VEC')
    opt = synth.default_opt(**over)
    params = synth.make_sat_params(opt, PARAM_SEED) if c.get('sat') else synth.make_params(opt, PARAM_SEED)
    lens = np.asarray(c['lens'], np.int64)
    vid = synth.make_video(N=len(lens), A=int(lens.max()), L=L, V1=V1, seed=c['seed'], T_v=c['T_v'], min_len=1, video_dim=opt.video_dim,
                           hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
    # make_video draws the event lengths at random: plant them
    if c.get('layout') == 'disjoint':
        start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    else:
        start = np.minimum(vid['soi'][:, 0], vid['T_v'] - lens)
    vid['soi'] = np.stack([start, start + lens], 1).astype(np.int64)
    vid['ind'] = (vid['soi'][:, 1] - 1).astype(np.int64)
    assert vid['soi'].min() >= 0 and vid['soi'][:, 1].max() <= vid['T_v']
    return opt, params, vid


def rows_shared(vid):
    """True when two events of the video share a feature row."""
    cov = np.zeros(vid['T_v'], np.int64)
    for s, e in vid['soi']:
        cov[int(s):int(e)] += 1
    return bool(cov.max() > 1)


# ---- the oracles ---------------------------------------------------------------------------------------------------------------------------
def run_oracle(opt, params, vid, train=True, f64=True):
    """dict(logp, loss, grads) of the CPU oracle on the float32 inputs, carried in float64 (or float32); train mode with the build's Philox
    masks.  grads holds every parameter's gradient and d tap_feats under 'tap_feats'."""
    dtype = torch.float64 if f64 else torch.float32
    run = SR.run if getattr(opt, 'caption_model', '') == 'show_attend_tell' else R.run
    logp, loss, grads, g_tap = run(opt, params, vid, train, dtype=dtype)
    grads = dict(grads, tap_feats=g_tap)
    return dict(logp=logp, loss=loss, grads=grads)


@functools.lru_cache(maxsize=None)
def oracle(name, train=True, f64=True):
    return run_oracle(*case(name), train=train, f64=f64)


def mutant(name, which):
    """The float64 oracle with the last float4 of one axis contributing nothing: 'alpha' -- alpha_net.weight[:, -4:] = 0 (the last float4 of
    Ha); 'c3d' -- c3d[:, -4:] = 0 (the last float4 of a clip row)."""
    opt, params, vid = case(name)
    if which == 'alpha':
        k = [k for k in params if k.endswith('alpha_net.weight')][0]
        params = dict(params, **{k: params[k].copy()})
        params[k][:, -4:] = 0.0
    else:
        assert which == 'c3d'
        vid = dict(vid, c3d=vid['c3d'].copy())
        vid['c3d'][:, -4:] = 0.0
    return run_oracle(opt, params, vid, True, True)


# ---- the measures --------------------------------------------------------------------------------------------------------------------------
def noise_only(k):
    return k in U.NOISE_ONLY or k in SR.NOISE_ONLY


def context_col0(opt):
    """First column of the attended context in the input weight of the LSTM that reads it."""
    if getattr(opt, 'caption_model', '') != 'show_attend_tell':
        return opt.CG_input_encoding_size
    ft = opt.CG_input_feats_type
    return opt.CG_input_encoding_size + (opt.lda_dim if 'V' in ft else 0) + (opt.d_o if 'E' in ft else 0)


def _tails(n):
    """The last float4 and the last, possibly partial, 256-wide chunk of an axis of length n."""
    return (('last4', slice(n - 4, n)), ('last256', slice(256 * ((n - 1) // 256), n)))


def width_slices(k, g, opt):
    """[(label, slice of g)] of a gradient tensor along its varied axes: ctx2att.weight rows (Ha) and columns (D), ctx2att.bias, h2att.weight
    rows / h2att.bias (Ha), alpha_net.weight columns (Ha), the context columns [col0, col0 + D) of the LSTM input weight that reads them."""
    D, Ha = opt.video_dim, opt.CG_att_hid_size
    out = []
    if k.endswith('ctx2att.weight'):
        out += [('%s[rows %s]' % (k, n), g[s]) for n, s in _tails(Ha)] + [('%s[cols %s]' % (k, n), g[:, s]) for n, s in _tails(D)]
    elif k.endswith('ctx2att.bias') or k.endswith('h2att.weight') or k.endswith('h2att.bias'):
        out += [('%s[rows %s]' % (k, n), g[s]) for n, s in _tails(Ha)]
    elif k.endswith('alpha_net.weight'):
        out += [('%s[cols %s]' % (k, n), g[:, s]) for n, s in _tails(Ha)]
    elif k.endswith('core.layer1.weight_ih') or k.endswith('core.rnn.weight_ih_l0'):
        c0 = context_col0(opt)
        ctx = g[:, c0:c0 + D]
        out += [('%s[ctx cols %s]' % (k, n), ctx[:, s]) for n, s in _tails(D)]
    return out


def grad_err(got, ref):
    """The figure util.grad_close judges: max|got - ref| less its 1e-9 absolute allowance, relative to the reference's max-norm (util.GRAD_FLOOR
    below it) -- grad_close(name, got, ref, tol) holds exactly when grad_err(got, ref) <= tol.  The allowance matters for the attention tensors
    of the H = 512 cases, whose max-norm is 1e-6 .. 1e-4 with three events."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return max(float(np.abs(got - ref).max()) - 1e-9, 0.0) / max(float(np.abs(ref).max()), U.GRAD_FLOOR)


def errors(got, ref, opt):
    """(max |d logp|, relative loss error, worst gradient tensor error, its name, worst slice error, its label) of `got` against `ref` (both
    dict(logp, loss, grads)).  Gradients by grad_err, relative to the reference tensor's (slice's own) max-norm; the tensors whose true
    gradient is zero (NOISE_ONLY) left out.  got['logp'] None: log-probs not judged (0.0)."""
    e_logp = 0.0
    if got['logp'] is not None:
        assert got['logp'].shape == ref['logp'].shape, (got['logp'].shape, ref['logp'].shape)
        e_logp = float(np.abs(got['logp'] - ref['logp']).max())
    e_loss = abs(got['loss'] - ref['loss']) / abs(ref['loss'])
    worst, worst_s = (0.0, ''), (0.0, '')
    for k, g in ref['grads'].items():
        if g is None or noise_only(k) or k not in got['grads']:
            continue
        worst = max(worst, (grad_err(got['grads'][k], g), k))
        for (label, gs), (_, rs) in zip(width_slices(k, got['grads'][k], opt), width_slices(k, g, opt)):
            worst_s = max(worst_s, (grad_err(gs, rs), label))
    return e_logp, e_loss, worst[0], worst[1], worst_s[0], worst_s[1]


def grads_close(grads, ref_grads, opt, tol, tol_slice):
    """The gradient gate: every tensor (util.grad_close, `tol`) and every width slice (`tol_slice`), each against its own max-norm.  Returns
    the misses [(label, error)]."""
    miss = []
    for k, g in ref_grads.items():
        if k not in grads:
            continue
        if g is None:
            if not (grads[k] is None or not np.any(grads[k])):
                miss.append((k, float('inf')))
            continue
        name = U.NOISE_ONLY[0] if noise_only(k) else k
        if grads[k] is None:
            miss.append((k, float('nan')))
            continue
        if not U.grad_close(name, grads[k], g, tol):
            miss.append((k, grad_err(grads[k], g)))
        if noise_only(k):
            continue
        for (label, gs), (_, rs) in zip(width_slices(k, grads[k], opt), width_slices(k, g, opt)):
            if not U.grad_close(label, gs, rs, tol_slice):
                miss.append((label, grad_err(gs, rs)))
    return miss


@functools.lru_cache(maxsize=None)
def e_ref(name):
    """The float32 oracle against the float64 oracle in train mode: (logp absolute, loss relative, worst tensor, name, worst slice, label)."""
    return errors(oracle(name, True, False), oracle(name, True, True), case(name)[0])


# ---- the gates -----------------------------------------------------------------------------------------------------------------------------
TOL_LOGP, TOL_LOSS, TOL_GRAD = 2e-5, 1e-5, 1e-5          # the existing gates (tests/test_gpu_parity.py)
CONTRACT = 1e-4
# e_ref per case (log-probs absolute, loss relative, worst gradient tensor, worst width slice -- grad_err), float32 oracle against float64
# oracle on the CPU, train mode: tools/parity_report.py --widths prints it, tests/test_width_ref_host.py re-measures it.  The largest entries
# are 6.4e-7 / 1.8e-7 / 1.3e-6 / 1.4e-6: 4 e_ref stays below every existing gate (2.6e-6 < 2e-5, 7.2e-7 < 1e-5, 5.2e-6 and 5.6e-6 < 1e-5), so the
# plain gates stand for every case, the slices included.
E_REF = {
    'a_ha4_d4': (2.4e-7, 1.7e-8, 3.1e-7, 3.1e-7),
    'a_ha252_d260': (2.9e-7, 1.1e-7, 3.3e-7, 3.3e-7),
    'a_ha256_d516': (3.3e-7, 4.4e-8, 4.5e-7, 4.5e-7),
    'a_ha256_d772': (3.3e-7, 7.7e-8, 6.7e-7, 1.1e-6),
    'a_ha260_d124': (2.8e-7, 8.8e-8, 3.3e-7, 2.1e-7),
    'a_ha260_d500': (3.3e-7, 4.3e-8, 1.3e-6, 1.3e-6),
    'a_ha508_d768': (2.9e-7, 5.1e-8, 4.5e-7, 4.7e-7),
    'a_ha508_d1024': (3.8e-7, 1.1e-8, 5.2e-7, 5.5e-7),
    'a_ha516_d132': (3.2e-7, 3.7e-9, 3.2e-7, 3.2e-7),
    'a_ha516_d260': (3.5e-7, 4.9e-8, 4.3e-7, 2.1e-7),
    'a_ha768_d516': (3.1e-7, 1.1e-8, 3.6e-7, 4.6e-7),
    'a_ha516_d772': (3.0e-7, 3.3e-8, 3.2e-7, 1.2e-6),
    'a_ha772_d256': (2.6e-7, 1.8e-7, 4.9e-7, 2.3e-7),
    'a_ha1020_d500': (2.7e-7, 8.5e-8, 5.3e-7, 4.8e-7),
    'a_ha772_d516': (2.9e-7, 5.2e-8, 5.4e-7, 5.2e-7),
    'a_ha1024_d1024': (3.7e-7, 6.0e-8, 6.6e-7, 7.3e-7),
    'a_ha1020_d4': (2.7e-7, 4.7e-8, 2.1e-7, 8.9e-8),
    'a_ha4_d1024': (2.8e-7, 7.1e-8, 1.1e-6, 1.4e-6),
    'b_d20_ha24_shared': (2.8e-7, 7.0e-8, 1.3e-7, 1.3e-7),
    'b_d20_ha24_disjoint': (3.1e-7, 8.2e-8, 1.7e-7, 1.7e-7),
    'b_d516_ha260_shared': (3.5e-7, 1.7e-8, 6.0e-7, 2.8e-7),
    'b_d516_ha260_disjoint': (6.1e-7, 3.0e-8, 1.2e-6, 1.2e-6),
    'c_h4_e4': (2.7e-7, 9.5e-8, 1.7e-7, 6.0e-8),
    'c_h36_e20': (2.6e-7, 4.9e-9, 1.9e-7, 1.9e-7),
    'c_h60_e16': (2.4e-7, 3.6e-8, 2.5e-7, 1.4e-7),
    'c_h132_e132': (2.5e-7, 1.1e-7, 4.9e-7, 4.7e-7),
    'c_h260_e4': (2.4e-7, 1.7e-8, 1.9e-7, 2.1e-7),
    'c_h8_e8': (2.6e-7, 2.6e-8, 1.9e-7, 1.5e-7),
    'c_h12_e12': (2.5e-7, 4.6e-8, 1.9e-7, 4.0e-7),
    'd_d8': (2.5e-7, 8.7e-9, 2.6e-7, 1.5e-7),
    'd_d12': (2.6e-7, 6.6e-8, 4.5e-7, 4.5e-7),
    'd_d124': (2.8e-7, 2.5e-8, 5.4e-7, 5.4e-7),
    'd_d128': (3.1e-7, 7.0e-8, 3.5e-7, 5.8e-7),
    'd_d132': (4.1e-7, 1.3e-8, 3.9e-7, 3.9e-7),
    'd_d256': (3.8e-7, 2.9e-8, 3.7e-7, 5.2e-7),
    'd_d260': (3.9e-7, 1.0e-7, 5.4e-7, 2.9e-7),
    'd_d388': (5.0e-7, 1.7e-9, 3.3e-7, 3.7e-7),
    'd_d508': (5.0e-7, 2.6e-8, 4.2e-7, 5.0e-7),
    'd_d512': (3.8e-7, 4.1e-8, 4.6e-7, 4.3e-7),
    'd_d512_e512': (4.3e-7, 5.5e-8, 4.0e-7, 4.0e-7),
    'd_d12_big': (2.4e-7, 2.1e-8, 3.1e-7, 3.4e-7),
    'd_d512_big': (6.4e-7, 2.2e-8, 4.0e-7, 3.7e-7),
    'f_sat_d260_ha252': (2.7e-7, 2.5e-8, 5.4e-7, 5.4e-7),
    'f_sat_d772_ha516': (3.1e-7, 6.1e-8, 4.5e-7, 5.0e-7),
    'f_dec_d260_ha252': (2.6e-7, 8.2e-8, 5.5e-7, 5.5e-7),
}
PLAIN = (TOL_LOGP, TOL_LOSS, TOL_GRAD, TOL_GRAD)
MARGIN = 1e-4          # top-1 / top-2 gap of the float64 decode below which a float32 route may pick another word (tests/test_gpu_beam.py)


def gates(name):
    """(log-probs, loss, gradient tensor, width slice): max(existing gate, 4 e_ref), log-probs and loss never above the contract."""
    e = E_REF[name]
    return (min(max(TOL_LOGP, 4 * e[0]), CONTRACT), min(max(TOL_LOSS, 4 * e[1]), CONTRACT), max(TOL_GRAD, 4 * e[2]), max(TOL_GRAD, 4 * e[3]))

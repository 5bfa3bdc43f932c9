"""The event-relation encoder (csrc/tsrm.hip) on every kernel route, against a FLOAT64 oracle (-m gpu).

echr_tsrm_fwd / echr_tsrm_bwd and their _batch forms are called directly through echr_amd._lib, the way functional._tsrm_forward /
_tsrm_backward call them, on the cases of tests/tsrm_ref.py (CASES: widths, event counts, combinator, dropout, TsrmGrads.zeroed, inference).
`out`, d ech and the twelve parameter gradients of (out * w).sum() are compared with tsrm_ref.run in float64 on the same float32 inputs and
the same Philox masks, each tensor relative to the float64 tensor's max-norm.  Workspaces arrive filled with NaN, gradient buffers with NaN
(zeroed = 0), zeros (zeroed = 1) or a sentinel (parameters the combinator does not reach).

Which test reaches which route, and how the route is asserted (launch counts of the library's profiler: kind 0 = fp32-path products incl.
the skinny kernel, kind 7 = h2 products; `rule` = the dispatch rule fixes it and the counts cannot tell):

  tsrm_rowhead_fwd / _bwd, tsrm_colhead_bwd  route-S-{1,2,33,63,64}, route-H256-*, route-FULL-{6,66}, fst*-S-33, peak-*-33, peak-FULL-64, batch-20_13:
                                             2 (forward) / 4 (backward) fp32 launches fewer than the general route (head_fused_ok: N <= 64, Df = Do = 32 G)
  general route, tsrm_softmax_fwd_kernel     route-S-{65,127}, route-ODD-{1,5,70}, route-ODD2-9, fst*-S-65, peak-S-65-*, batch-1_40_24 (N = 65): counts; rule N < 128
  tsrm_softmax_rows_kernel                   route-S-{128,130}, route-FULL-130-z1 (16 heads, four per wave), fst*-S-130, peak-S-130-*, batch-64_1_65, tables-*:
                                             counts of the general route; rule N >= 128
  tsrm_softmax_bwd_kernel                    every general-route case with a backward pass (all but tables-*)
  fc1 on fp32 / on h2                        route-H256-31 (961 pairs) / route-H256-32 (1024): kind 7 count 0 / 1, forward and backward
  skinny_nt<16> / <32>                       route-H256-66 / route-FULL-66, -130 (rule gemm_skinny_ok: >= 4096 pairs, Df 256 / 512; 4356 = 272 * 16 + 4 rows)
  posemb_packed_kernel                       route-FULL-66-*, route-FULL-130-z1 (rule: >= 4096 pairs and posemb_packed_ok; Df = 256 has no packed form)
  pair_mlp_bwd_kernel                        route-FULL-{6,66,130}-z1: 2 fp32 launches fewer in the backward than zeroed = 0 (36, 4356, 16900 pairs: last block of 4 rows)
  ungrouped projections                      route-ODD-*: 3 + 3 + 3 launches instead of 1 + 1 + 1 (Do != Df)
  pair_phi / pair_gate<32> / <16>            tables-FULL-130 / tables-H256-130: kind 7 count 2 (the two table products) against 1 (dense fc1); 16900 pairs: last tile of 4
  posemb_rows_kernel / posemb_kernel         test_position_embedding_alone (Df 32, 512 with the switch on / every other combination); inside the encoder
                                             route-ODD-* (Df / 4 = 12) and route-ODD2-9 (Df / 4 = 20) take posemb_kernel with a partial last chunk (rule of posemb())
  fst_combine / fst_grad, modes 0..4         fst{0..4}-S-{33,65,130}: rowhead kernels, softmax_fwd + softmax_bwd, softmax_rows + softmax_bwd

Gates.  e_ref = the error of tsrm_ref.run(dtype = float32) against tsrm_ref.run(dtype = float64), measured on the CPU (tools/parity_report.py
--tsrm prints the table below); the gate of the HIP path against float64 is max(existing gate, 4 * e_ref) with the existing gates 1e-5 for
`out` and 1e-5 (util.grad_close, with its floor) for gradients -- the rule of tests/test_gpu_attention_regime.py; 4x: the HIP path rounds in
the same precision but sums in the order of MFMA tiles and split-K.  E_REF holds (out, worst gradient incl. d ech, noise) per case.  (The float32 oracle's
rounding depends on the host's BLAS blocking, so a second measurement moves single figures by up to 2x; the committed table is the gate.
The HIP path measured at most 0.45 of its gate on an MI355X: peak-FULL-64-fst0-eval, out 8.9e-6 of 2.0e-5.)
Tensors whose true gradient is exactly zero (tsrm_ref.noise_only: the float64 oracle holds < 1e-12 there) are held on the absolute scale:
max(1e-6, 4 * the largest value the float32 oracle holds in them).

Sensitivity (scratch copies of csrc/tsrm.hip, never committed): which test fails under each mutation.
  * fst_combine cases 1 and 2 swapped inside tsrm_softmax_rows_kernel only (run on an MI355X): fst1-S-130 (out off by 4.4x its max-norm),
    fst2-S-130 (0.078), peak-S-130-fst1-eval / -train (1.1) and batch-64_1_65-fst2 (0.050) fail; every other fst*, peak-* and batch-* case passes
    (the groups that were run).
  * pair_gate_kernel without the clamp `row = M - 1` that goes with the `orow < M` guard: lanes 4..15 of the last tile (rows 16900..16911 of
    tables-*-130) form i = 130 and read ev_start[130] / ev_len[130], one element past the arrays.  An out-of-bounds read: not run.  From
    the code, the table rows such a lane then gathers stay inside the tables (li, lj and the span are clamped) and its MFMA row is never
    stored (`orow < M`), so no output changes: no comparison can see it, only a memory checker on a host build of the index arithmetic could.
  * posemb_kernel without `k >= F4`: a thread writes 16 frequencies where Df / 4 = 8, 12 or 20 leaves 8, 12 or 4; o[k] with k >= F4 puts
    sines over the cosine segment of the same pair, o[3 F4 + k] reaches the next pair's row and, for the last pair, past the buffer.  An
    out-of-bounds write: not run.  test_position_embedding_alone[32-0], [48-*] and [80-*] compare every element and fail on the overwritten
    cosines; route-ODD-* and route-ODD2-9 see the same embedding inside the encoder.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import tsrm_ref as R, util as U

pytestmark = pytest.mark.gpu

TOL_OUT, TOL_GRAD = 1e-5, 1e-5          # the existing gates (tests/test_gpu_parity.py: event context 1e-5, TOL_GRAD)
TOL_TABLE_VS_DENSE = 2e-6               # test_event_context_inference_tables_vs_oracle
POSEMB_GATE = 1e-6                      # absolute: about eight float32 ulps of 1 (the kernel claims ~1e-7; the host test measures the transcription at 8.3e-8)
TOL_NOISE = 1e-6                        # absolute, tensors whose true gradient is exactly zero (util.grad_close's rule for NOISE_ONLY)
SENT = -77.25
KINDS = (0, 6, 7)                       # echr_prof_read: fp32 path, bf16x3, h2

# e_ref per case: (out, worst gradient incl. d ech, largest |value| in a noise-only tensor), float32 oracle vs float64 oracle on the CPU --
# tools/parity_report.py --tsrm (the comment names the worst gradient tensor)
E_REF = {
    'route-S-1': (1.7e-07, 4.2e-07, 0.0e+00),                     # d ech
    'route-S-2': (1.7e-07, 3.2e-07, 0.0e+00),                     # enc_attn.key_1.bias
    'route-S-33': (2.0e-07, 7.2e-07, 0.0e+00),                    # enc_attn.pair_pos_fc1.weight
    'route-S-63': (2.3e-07, 8.0e-07, 0.0e+00),                    # enc_attn.key_1.bias
    'route-S-64': (1.9e-07, 8.3e-07, 0.0e+00),                    # enc_attn.pair_pos_fc2.weight
    'route-S-65': (2.2e-07, 5.2e-07, 0.0e+00),                    # enc_attn.pair_pos_fc1.weight
    'route-S-127': (2.8e-07, 2.1e-06, 0.0e+00),                   # enc_attn.pair_pos_fc2.weight
    'route-S-128': (2.5e-07, 1.0e-06, 0.0e+00),                   # enc_attn.pair_pos_fc1.weight
    'route-S-130': (3.0e-07, 7.7e-07, 0.0e+00),                   # enc_attn.query_1.bias
    'route-ODD-1': (7.6e-08, 2.6e-07, 0.0e+00),                   # d ech
    'route-ODD-5': (1.5e-07, 2.9e-06, 0.0e+00),                   # enc_attn.pair_pos_fc2.bias
    'route-ODD-70': (1.5e-07, 6.8e-07, 0.0e+00),                  # enc_attn.pair_pos_fc1.weight
    'route-ODD2-9': (1.9e-07, 6.3e-07, 0.0e+00),                  # enc_attn.key_1.bias
    'route-H256-31': (1.8e-07, 7.3e-07, 0.0e+00),                 # enc_attn.pair_pos_fc2.weight
    'route-H256-32': (2.0e-07, 7.9e-07, 0.0e+00),                 # enc_attn.pair_pos_fc1.weight
    'route-H256-66': (2.8e-07, 9.2e-07, 0.0e+00),                 # enc_attn.key_1.bias
    'route-FULL-6-z0': (1.5e-07, 5.0e-07, 0.0e+00),               # enc_attn.key_1.bias
    'route-FULL-6-z1': (1.5e-07, 5.0e-07, 0.0e+00),               # enc_attn.key_1.bias
    'route-FULL-66-z0': (4.2e-07, 7.4e-07, 0.0e+00),              # d ech
    'route-FULL-66-z1': (4.2e-07, 7.4e-07, 0.0e+00),              # d ech
    'route-FULL-130-z1': (3.2e-07, 1.1e-06, 0.0e+00),             # enc_attn.pair_pos_fc1.weight
    'fst0-S-33': (2.0e-07, 7.2e-07, 0.0e+00),                     # enc_attn.pair_pos_fc1.weight
    'fst1-S-33': (1.9e-07, 1.6e-06, 3.0e-07),                     # enc_attn.pair_pos_fc1.bias
    'fst2-S-33': (1.9e-07, 7.8e-07, 3.5e-08),                     # enc_attn.pair_pos_fc1.bias
    'fst3-S-33': (1.9e-07, 1.6e-06, 4.8e-07),                     # enc_attn.pair_pos_fc1.bias
    'fst4-S-33': (1.5e-07, 3.8e-07, 3.4e-08),                     # enc_attn.key_1.weight
    'fst0-S-65': (2.2e-07, 5.2e-07, 0.0e+00),                     # enc_attn.pair_pos_fc1.weight
    'fst1-S-65': (2.1e-07, 1.3e-06, 2.4e-07),                     # enc_attn.pair_pos_fc1.bias
    'fst2-S-65': (1.8e-07, 5.6e-06, 5.6e-08),                     # enc_attn.pair_pos_fc2.bias
    'fst3-S-65': (1.9e-07, 1.1e-06, 2.7e-07),                     # enc_attn.pair_pos_fc1.bias
    'fst4-S-65': (2.0e-07, 3.5e-07, 3.7e-08),                     # enc_attn.key_1.weight
    'fst0-S-130': (3.0e-07, 7.7e-07, 0.0e+00),                    # enc_attn.query_1.bias
    'fst1-S-130': (2.3e-07, 9.5e-07, 6.0e-08),                    # enc_attn.pair_pos_fc1.bias
    'fst2-S-130': (2.7e-07, 8.2e-07, 6.7e-08),                    # enc_attn.pair_pos_fc2.bias
    'fst3-S-130': (2.7e-07, 1.2e-06, 4.8e-07),                    # enc_attn.pair_pos_fc1.bias
    'fst4-S-130': (2.0e-07, 5.4e-07, 7.5e-08),                    # d ech
    'peak-FULL-64-fst0-eval': (5.0e-06, 5.6e-06, 0.0e+00),        # enc_attn.query_1.weight
    'peak-S-33-fst0-eval': (9.4e-07, 2.3e-06, 0.0e+00),           # enc_attn.pair_pos_fc1.weight
    'peak-S-33-fst1-eval': (2.3e-06, 3.5e-06, 6.6e-07),           # enc_attn.pair_pos_fc2.weight
    'peak-S-65-fst0-eval': (2.3e-06, 1.0e-05, 0.0e+00),           # enc_attn.pair_pos_fc2.bias
    'peak-S-65-fst1-eval': (2.4e-06, 5.0e-06, 8.4e-07),           # enc_attn.key_1.weight
    'peak-S-130-fst0-eval': (3.8e-06, 5.5e-06, 0.0e+00),          # d ech
    'peak-S-130-fst1-eval': (2.9e-06, 5.4e-06, 2.6e-06),          # d ech
    'peak-FULL-64-fst0-train': (4.8e-06, 6.0e-06, 0.0e+00),       # enc_attn.pair_pos_fc2.bias
    'peak-S-33-fst0-train': (9.6e-07, 2.4e-06, 0.0e+00),          # enc_attn.pair_pos_fc1.weight
    'peak-S-33-fst1-train': (2.4e-06, 4.0e-06, 1.5e-06),          # enc_attn.query_1.weight
    'peak-S-65-fst0-train': (2.3e-06, 8.7e-06, 0.0e+00),          # enc_attn.pair_pos_fc2.bias
    'peak-S-65-fst1-train': (1.9e-06, 5.3e-06, 1.5e-06),          # enc_attn.key_1.weight
    'peak-S-130-fst0-train': (3.2e-06, 1.0e-05, 0.0e+00),         # enc_attn.query_1.weight
    'peak-S-130-fst1-train': (2.8e-06, 5.3e-06, 3.0e-06),         # d ech
    'batch-20_13-fst0': (1.9e-07, 4.5e-07, 0.0e+00),              # enc_attn.pair_pos_fc2.weight
    'batch-20_13-fst2': (2.4e-07, 3.3e-05, 4.1e-08),              # enc_attn.pair_pos_fc2.bias
    'batch-1_40_24-fst0': (1.2e-07, 4.3e-07, 0.0e+00),            # enc_attn.key_1.weight
    'batch-1_40_24-fst2': (1.2e-07, 1.2e-06, 5.0e-08),            # enc_attn.pair_pos_fc2.bias
    'batch-64_1_65-fst0': (1.0e-07, 8.0e-07, 0.0e+00),            # enc_attn.pair_pos_fc1.weight
    'batch-64_1_65-fst2': (1.1e-07, 1.2e-05, 7.5e-08),            # enc_attn.pair_pos_fc2.bias
    'tables-FULL-130': (4.8e-07, 7.1e-07, 0.0e+00),               # d ech
    'tables-H256-130': (3.3e-07, 7.6e-07, 0.0e+00),               # d ech
}


def gates(name):
    e = E_REF[name]
    return max(TOL_OUT, 4 * e[0]), max(TOL_GRAD, 4 * e[1]), max(TOL_NOISE, 4 * e[2])


def _libs():
    from echr_amd import _lib as L
    return L, L.load()


def _counts(fn):
    """{kind: launches the library's profiler counted while fn ran}."""
    L, lib = _libs()
    L.check(lib.echr_prof_enable(1), 'prof_enable')
    try:
        fn()
        torch.cuda.synchronize()
        n = {}
        for kind in KINDS:
            ms, fl, by, cnt = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
            L.check(lib.echr_prof_read(kind, C.byref(ms), C.byref(fl), C.byref(by), C.byref(cnt)), 'prof_read')
            n[kind] = cnt.value
    finally:
        L.check(lib.echr_prof_enable(0), 'prof_enable')
    return n


# ---- the dispatch rules of csrc/tsrm.hip, restated: launches per profiler kind ----------------------------------------------------------
def fused_heads(N, Df, Do, G):
    return N <= 64 and Df == 32 * G and Do == 32 * G          # head_fused_ok


def expect_fwd(N, Df, Do, G, mode, tables=False):
    f32 = 1 + (1 if Do == Df else 3)          # event embedding; query | key | output projection (grouped when Do = Df)
    h2 = 0
    if mode != 4:
        if tables:
            h2 += 2                           # F_c and F_l; the gates come from pair_gate_kernel
        else:
            if N * N >= 1024:
                h2 += 1                       # fc1 on packed operands
            else:
                f32 += 1
            f32 += 1                          # fc2: the fp32 product or the skinny kernel
    if not fused_heads(N, Df, Do, G):
        f32 += 2                              # Q K^T and WD . XW around the softmax kernel
    return {0: f32, 6: 0, 7: h2}


def expect_bwd(N, Df, Do, G, mode, zeroed):
    f32 = h2 = 0
    if not fused_heads(N, Df, Do, G):
        f32 += 4                              # d WD, d XW, d Q, d K
    if mode != 4:
        if not (zeroed and Df == 512 and G == 16):
            f32 += 2                          # d W_fc2 and d P1 (pair_mlp_bwd_kernel otherwise)
        if N * N >= 1024:
            h2 += 1                           # d W_fc1
        else:
            f32 += 1
    f32 += 1 if (Do == Df and Df > 32) else 3          # d X
    f32 += 1 if Do == Df else 3                        # d W_q, d W_k, d W_out
    f32 += 2                                           # d W_emb, d ech
    return {0: f32, 6: 0, 7: h2}


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(n):
    return torch.full((int(n),), float('nan'), device='cuda', dtype=torch.float32)


def gpu_run(spec, bounds=(0, 0), backward=None):
    """The case through the C ABI: (out, d ech, {name: gradient}, launch counts forward, launch counts backward); host arrays."""
    L, lib = _libs()
    params, ech, soi, vid, _ = R.case_inputs(spec)
    Df, Do, G = R.WIDTHS[spec['width']]
    N, Din, mode = spec['N'], R.DIN, spec['mode']
    backward = spec['backward'] if backward is None else backward
    ps = [_dev(params[k].reshape(Do, Df) if k == R.NAMES[10] else params[k]) for k in R.NAMES]
    ech_d = _dev(ech)
    ev_start, ev_len = _dev(soi[:, 0].astype(np.int32)), _dev((soi[:, 1] - soi[:, 0]).astype(np.int32))
    ws = _nan(lib.echr_tsrm_ws_floats(N, Din, Df, Do, G))
    out = _nan(N * Do).view(N, Do)
    d = L.Dropout(R.SEED, R.OFFSET, 1 if spec['train'] else 0, R.P_DROP, 0.5, 0.5)
    x = vid_d = None
    if vid is not None:
        vid_d = _dev(vid.astype(np.int32))
        x = L.BatchExt(len(spec['counts']), L.ptr(vid_d, torch.int32), None, None, None)

    def args(inference, max_len, max_span):
        return L.TsrmArgs(N, Din, Df, Do, G, *[L.ptr(p) for p in ps], L.ptr(ech_d), L.ptr(ev_start, torch.int32), L.ptr(ev_len, torch.int32),
                          L.ptr(ws), L.ptr(out), inference, max_len, max_span, mode)

    def fwd():
        a = args(spec['inference'], *bounds)
        if x is not None:
            L.check(lib.echr_tsrm_fwd_batch(C.byref(a), C.byref(d), C.byref(x), L.stream_ptr()), 'tsrm_fwd_batch')
        else:
            L.check(lib.echr_tsrm_fwd(C.byref(a), C.byref(d), L.stream_ptr()), 'tsrm_fwd')
    nf = _counts(fwd)
    assert lib.echr_check_async() == 0, lib.echr_last_error()
    if not backward:
        return out.cpu().numpy(), None, None, nf, None
    zeroed = spec['zeroed']
    unreached = R.UNREACHED.get(mode, ())
    grads = [torch.full_like(p, SENT) if k in unreached else (torch.zeros_like(p) if zeroed else torch.full_like(p, float('nan')))
             for k, p in zip(R.NAMES, ps)]
    g_ech = _nan(N * Din).view(N, Din)
    g_out = _dev(R.out_weight(N, Do))
    wsb = _nan(lib.echr_tsrm_ws_bwd_floats(N, Din, Df, Do, G))

    def bwd():
        a = args(0, 0, 0)
        g = L.TsrmGrads(*[L.ptr(t) for t in grads], L.ptr(g_ech), L.ptr(g_out), L.ptr(wsb), zeroed)
        if x is not None:
            L.check(lib.echr_tsrm_bwd_batch(C.byref(a), C.byref(g), C.byref(d), C.byref(x), L.stream_ptr()), 'tsrm_bwd_batch')
        else:
            L.check(lib.echr_tsrm_bwd(C.byref(a), C.byref(g), C.byref(d), L.stream_ptr()), 'tsrm_bwd')
    nb = _counts(bwd)
    assert lib.echr_check_async() == 0, lib.echr_last_error()
    return (out.cpu().numpy(), g_ech.cpu().numpy(), {k: t.cpu().numpy().reshape(params[k].shape) for k, t in zip(R.NAMES, grads)}, nf, nb)


@functools.lru_cache(maxsize=None)
def _ref64(name):
    return R.reference(R.CASES[name])


def errors(spec, got, ref):
    """(error of out, worst gradient error incl. d ech, its name, largest |value| in a noise-only tensor), as tsrm_ref.e_ref forms them."""
    out, dech, grads = got[:3]
    ro, rx, rg = ref
    worst, noise = (0.0, '-'), 0.0
    if dech is not None:
        worst = (R.rel(dech, rx, U.GRAD_FLOOR), 'd ech')
        for k, g in rg.items():
            if g is not None and k not in R.noise_only(spec):
                worst = max(worst, (R.rel(grads[k], g, U.GRAD_FLOOR), k))
        noise = max([float(np.abs(grads[k]).max()) for k in R.noise_only(spec)] + [0.0])
    return R.rel(out, ro), worst[0], worst[1], noise


def check(spec, got, ref, what=''):
    name = spec['name']
    to, tg, tn = gates(name)
    out, dech, grads = got[:3]
    ro, rx, rg = ref
    assert out.shape == ro.shape and np.isfinite(out).all(), (name, what)
    e = errors(spec, got, ref)
    print('%s %s: out %.3e (gate %.2e)  worst gradient %.3e (%s, gate %.2e)  noise %.1e (gate %.1e)' % (name, what, e[0], to, e[1], e[2], tg, e[3], tn))
    assert e[0] < to, (name, what, e[0])
    if dech is None:
        return
    assert np.isfinite(dech).all() and U.grad_close('d ech', dech, rx, tg), (name, what, R.rel(dech, rx))
    for k, g in rg.items():
        if g is None:
            # a parameter the combinator does not reach: the library accumulates nothing there (exact zeros at most) -- the sentinel is back bit for bit
            assert spec['zeroed'] == 1 or spec['mode'] == 4
            assert np.array_equal(grads[k], np.full_like(grads[k], SENT)), (name, what, k)
        elif k in R.noise_only(spec):
            assert np.abs(grads[k]).max() < tn and np.abs(g).max() < 1e-12, (name, what, k, np.abs(grads[k]).max())
        else:
            assert np.isfinite(grads[k]).all(), (name, what, k)
            assert U.grad_close(k, grads[k], g, tg), (name, what, k, R.rel(grads[k], g))


def check_route(spec, got, tables=False):
    Df, Do, G = R.WIDTHS[spec['width']]
    nf, nb = got[3], got[4]
    assert nf == expect_fwd(spec['N'], Df, Do, G, spec['mode'], tables), (spec['name'], 'forward launches', nf)
    if nb is not None:
        assert nb == expect_bwd(spec['N'], Df, Do, G, spec['mode'], spec['zeroed']), (spec['name'], 'backward launches', nb)


def _group(prefix):
    return [n for n in R.CASES if n.split('-')[0].startswith(prefix)]


@pytest.mark.parametrize('name', _group('route'))
def test_routes_at_their_boundaries(name):
    """Train mode, dropout, fST0: forward and backward at the event counts where the dispatch changes."""
    spec = R.CASES[name]
    got = gpu_run(spec)
    check_route(spec, got)
    check(spec, got, _ref64(name))


def test_route_counts_tell_the_routes_apart():
    """The restated rules at the boundaries the cases sit on: a case that moved to the other side of one would change these counts."""
    S, H, F = R.WIDTHS['S'], R.WIDTHS['H256'], R.WIDTHS['FULL']
    assert expect_fwd(64, *S, 0)[0] + 2 == expect_fwd(65, *S, 0)[0] and expect_bwd(64, *S, 0, 0)[0] + 4 == expect_bwd(65, *S, 0, 0)[0]
    assert (expect_fwd(31, *H, 0)[7], expect_fwd(32, *H, 0)[7]) == (0, 1) and (expect_bwd(31, *H, 0, 0)[7], expect_bwd(32, *H, 0, 0)[7]) == (0, 1)
    assert expect_bwd(66, *F, 0, 0)[0] == expect_bwd(66, *F, 0, 1)[0] + 2
    assert expect_fwd(130, *F, 0, tables=True)[7] == 2 and expect_fwd(130, *F, 0)[7] == 1
    assert not fused_heads(1, *R.WIDTHS['ODD']) and not fused_heads(9, *R.WIDTHS['ODD2'])


@pytest.mark.parametrize('name', _group('fst'))
def test_every_combinator_on_every_route(name):
    """fST0..fST3 and use_posit = 0 through the fused heads (N = 33), tsrm_softmax_fwd / _bwd (65) and tsrm_softmax_rows / _bwd (130)."""
    spec = R.CASES[name]
    got = gpu_run(spec)
    check_route(spec, got)
    check(spec, got, _ref64(name))


@pytest.mark.parametrize('mode', [3, 4])
def test_unreached_gradients_when_the_library_overwrites(mode):
    """zeroed = 0 (the library stores its gradients): use_posit = 0 leaves the position MLP's four buffers untouched; fST3 reaches query / key
    with d aff = 0 exactly and stores exact zeros."""
    spec = dict(R.CASES['fst%d-S-65' % mode], zeroed=0)
    got = gpu_run(spec)
    check_route(spec, got)
    for k in R.UNREACHED[mode]:
        want = SENT if mode == 4 else 0.0
        assert np.array_equal(got[2][k], np.full_like(got[2][k], want)), k


@pytest.mark.parametrize('name', _group('peak'))
def test_peaked_softmaxes(name):
    """query / key scaled until the median largest weight is >= 0.9 (host test): a wrong row maximum or a lane beyond N in the reductions moves these outputs."""
    spec = R.CASES[name]
    got = gpu_run(spec)
    check_route(spec, got)
    check(spec, got, _ref64(name))


@pytest.mark.parametrize('name', _group('batch'))
def test_multi_video_batches(name):
    """(20, 13): fused heads; (1, 40, 24): N = 65, a one-event video first, a video boundary inside the first 64-lane pass;
    (64, 1, 65): N = 130, the rows kernel, a one-event video whose row sits at the end of the first pass."""
    spec = R.CASES[name]
    got = gpu_run(spec)
    check_route(spec, got)
    check(spec, got, _ref64(name))


@pytest.mark.parametrize('name', _group('tables'))
def test_inference_tables(name):
    """inference = 1 with the host-known bounds: tabulated fc1 and pair_gate_kernel (16900 pairs: its last tile holds 4 live rows) against
    float64, against the dense path (pair_tables = 0) and without bounds (dense fallback)."""
    L, lib = _libs()
    spec = R.CASES[name]
    soi = R.case_inputs(spec)[2]
    from echr_amd import functional as EF
    ev = EF.event_index_tensors(soi, np.zeros(len(soi), np.int64), torch.device('cuda'))
    b = ev[1].echr_bounds
    assert b == R.bounds(soi)
    ref = _ref64(name)
    tab = gpu_run(spec, bounds=b)
    check_route(spec, tab, tables=True)
    try:
        L.check(lib.echr_config_set(b'pair_tables', 0), 'config_set')
        dense = gpu_run(spec, bounds=b)
    finally:
        L.check(lib.echr_config_set(b'pair_tables', 1), 'config_set')
    nob = gpu_run(spec, bounds=(0, 0))
    check_route(spec, dense)
    check_route(spec, nob)
    for what, got in (('tables', tab), ('pair_tables = 0', dense), ('no bounds', nob)):
        check(spec, got, ref, what)
    print('%s: tables vs dense %.3e, no bounds vs dense %.3e' % (name, R.rel(tab[0], dense[0]), R.rel(nob[0], dense[0])))
    assert R.rel(tab[0], dense[0]) < TOL_TABLE_VS_DENSE and R.rel(nob[0], dense[0]) < TOL_TABLE_VS_DENSE


POSEMB_SOI = np.array([[0, 1], [8191, 8192], [100, 300], [199, 201], [5, 6], [7, 20], [8191, 8391], [3, 4], [50, 61]])


@functools.lru_cache(maxsize=None)
def _posemb64(Df):
    return R.posemb(POSEMB_SOI, Df)


@pytest.mark.parametrize('rows', [1, 0])
@pytest.mark.parametrize('Df', [32, 48, 80, 512])
def test_position_embedding_alone(Df, rows):
    """functional.position_embedding: posemb_rows_kernel where Df / 4 divides 256 and the switch is on (32, 512), posemb_kernel otherwise --
    Df / 4 = 8 and 12: one partial chunk of 16 frequencies, 20: two chunks, the second partial, 128: eight full ones.  9 events: length 1,
    equal centres (events 2 and 3), lengths 1 and 200, starts of 8191 (arguments up to 8.3e5 rad)."""
    L, lib = _libs()
    from echr_amd import functional as EF
    ev_start = _dev(POSEMB_SOI[:, 0].astype(np.int32))
    ev_len = _dev((POSEMB_SOI[:, 1] - POSEMB_SOI[:, 0]).astype(np.int32))
    try:
        L.check(lib.echr_config_set(b'posemb_rows', rows), 'config_set')
        pos = EF.position_embedding(ev_start, ev_len, Df)
        torch.cuda.synchronize()
    finally:
        L.check(lib.echr_config_set(b'posemb_rows', 1), 'config_set')
    assert lib.echr_check_async() == 0
    pos = pos.cpu().numpy()
    ref = _posemb64(Df)
    assert pos.shape == ref.shape
    e = float(np.abs(pos - ref).max())
    print('posemb Df=%d rows=%d: max abs error %.3e' % (Df, rows, e))
    assert e < POSEMB_GATE

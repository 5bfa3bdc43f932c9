"""Token selection of the decoders on exactly known logits (-m gpu): the multinomial draw, the greedy arg-max and the beam pick of every
vocabulary-width form, replayed against tests/select_ref.py.

With lm_model.logit.weight = 0 every product form of the logits -- the fp32 MFMA k-slice slabs, the h2 product, the plain product, the
persistent decoder's fp16-pair image -- yields exactly 0 + b_logit at every row and step, whatever the state, the dropout or the contexts.
The logits are therefore known on the host bit for bit, and so are the uniforms (echr_amd/philox.py: sample_u24), so every draw of a
decode is replayed: the device token must be the float64 inverse-CDF pick, except within DELTA of an interval boundary, where it may be
the neighbour (select_ref.check_draws).  Ties are exact: the arg-max kernels must take the lowest index, the beam step the smaller slot,
then the smaller token.

Measured on an MI355X (the draws of test_multinomial_decode_replays_draw_by_draw): of 104 000 observable draws 46 differed from the
float64 pick, the farthest 2.3e-7 from the boundary it crossed (per V1: 257 and 2048 none; 2049 1.3e-7; 5120 1.6e-7; 5121 1.4e-7;
12288 2.3e-7; 12289 2.1e-7) -- DELTA = 1e-6 stands.

Not covered on purpose: the branch `target >= total` of the multinomial kernels needs u24 = 2^24 - 1, about one draw in 10^7; searching
seeds for it is not worth a test.

Gates: tokens exact (outside DELTA of a boundary), log-probs and scores 1e-4 per token against float64 (the gate of
test_multinomial_sampling_distribution_and_reproducibility for the same quantity)."""
import functools

import numpy as np
import pytest
import torch

from echr_amd import synth
from tests import select_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

TOL_LOGP = 1e-4
L_SAMPLE = R.SEQ_LEN
L_GREEDY = 6
NATIVE = (['lm_model.embed.weight', 'lm_model.logit.weight', 'lm_model.logit.bias']
          + ['lm_model.core.layer%d.%s' % (k, n) for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh') for k in range(3)]
          + ['lm_model.core.attention.' + n for n in ('ctx2att.weight', 'ctx2att.bias', 'h2att.weight', 'h2att.bias', 'alpha_net.weight',
                                                      'alpha_net.bias')])


def _lib():
    from echr_amd import _lib as L
    return L.load()


@functools.lru_cache(maxsize=None)
def _params(V1):
    """The decoder's parameters at the default widths (H = 512: 3H is a multiple of 128, the slab form applies) in the order of
    OldModel.native_params, logit.weight zeroed; built once per V1, the bias is swapped per case."""
    opt = synth.default_opt(vocab_size=V1 - 1, seq_length=L_SAMPLE)
    p = synth.make_params(opt, 0)
    p['lm_model.logit.weight'] = np.zeros_like(p['lm_model.logit.weight'])
    return [torch.from_numpy(p[k]).cuda() for k in NATIVE]


def _with_bias(V1, bias):
    ps = _params(V1)
    ps[2].copy_(torch.from_numpy(np.asarray(bias, np.float32)))
    return ps


@functools.lru_cache(maxsize=None)
def _inputs(N):
    """One synthetic video with N events of up to 6 segments on 40 feature rows; random scene / event contexts (nothing here depends on
    them).  For the batch entries: 3 scene vectors and a non-decreasing video index with a one-event video."""
    from echr_amd import functional as EF
    dev = torch.device('cuda')
    v = synth.make_video(N, 6, 8, 10, seed=1900 + N, T_v=40)
    rs = np.random.RandomState(1901 + N)
    ev = EF.event_index_tensors(v['soi'], v['ind'], dev, 40)
    sizes = [N // 3, 1, N - N // 3 - 1] if N >= 3 else [N]
    vid = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    return dict(c3d=torch.from_numpy(v['c3d']).to(dev), ev_start=ev[0], ev_len=ev[1], A=ev[3],
                video=torch.from_numpy(v['lda']).to(dev), event=torch.from_numpy((0.5 * rs.standard_normal((N, 512))).astype(np.float32)).to(dev),
                videos=torch.from_numpy(np.abs(rs.standard_normal((len(sizes), 100))).astype(np.float32) / 100).to(dev),
                vid=torch.from_numpy(vid).to(dev), vid_host=vid)


def _np(t, N, width):
    """A returned [N, T] tensor (or [] when T == 0) zero-padded to [N, width] on the host."""
    out = np.zeros((N, width), np.float64 if (isinstance(t, torch.Tensor) and t.is_floating_point()) else np.int64)
    if isinstance(t, torch.Tensor):
        out[:, :t.shape[1]] = t.cpu().numpy()
    return out


def _width(t):
    return t.shape[1] if isinstance(t, torch.Tensor) else 0


# ---- 4. multinomial replay --------------------------------------------------------------------------------------------------------
def _sample(entry, N, ps, T, seed):
    """(seq_full [N, L], logp_full [N, L], returned width, video_words or None) of one multinomial decode through echr_amd.functional."""
    from echr_amd import functional as EF
    i = _inputs(N)
    Ls = L_SAMPLE
    if entry == 'batch':
        drop = EF.DropState(U.SEED, U.OFFSET, True)
        seq, slp, vw = EF.sample_train_batch(i['videos'], i['event'], i['c3d'], i['ev_start'], i['ev_len'], i['vid'], i['A'], Ls, ps, drop,
                                             temperature=T, seed=seed)
        return _np(seq, N, Ls), _np(slp, N, Ls), _width(seq), vw
    dbg = {}
    drop = EF.DropState(U.SEED, U.OFFSET, True) if entry == 'train' else None
    seq, slp = EF.greedy_sample(i['video'], i['event'], i['c3d'], i['ev_start'], i['ev_len'], i['A'], Ls, ps, debug=dbg, multinomial=True,
                                temperature=T, seed=seed, drop=drop)
    full, lp = dbg['seq_full'].cpu().numpy(), dbg['logp_full'].double().cpu().numpy()
    assert torch.equal(dbg['last_logits'], ps[2].expand(N, -1))          # the handle itself: the product contributes exactly 0
    assert np.array_equal(_np(seq, N, _width(seq)), full[:, :_width(seq)])
    if _width(seq):
        assert torch.equal(slp, dbg['logp_full'][:, :_width(seq)])
    return full, lp, _width(seq), None


@pytest.mark.parametrize('entry,N,V1,kind', R.MULTINOMIAL_PARAMS)
def test_multinomial_decode_replays_draw_by_draw(entry, N, V1, kind):
    """Every draw of a 20-step decode against the float64 inverse CDF at the Philox uniforms of (seed, batch-global row, step), temperatures
    1.0 and 0.7 (and 0 = 1 once), a 32-bit and a 56-bit seed: sample_step behind the slab sum / the h2 product / the plain product, with the
    dropout active, and sample_row_step<8 | 20 | 48 | 0> from slabs and on finished logits (the forms: select_ref.MULTINOMIAL_CASES)."""
    lib = _lib()
    bias, marked = R.bias_design(V1, kind, V1)
    ps = _with_bias(V1, bias)
    x = bias.astype(np.float64)
    lse = x.max() + np.log(np.exp(x - x.max()).sum())
    temps = R.TEMPERATURES + ((0.0,) if (entry, V1, kind) == ('eval', 2049, 'edges') else ())
    if entry == 'eval_plain':
        assert lib.echr_config_set(b'gemm_h2', 0) == 0
    try:
        for T in temps:
            for seed in R.SEEDS:
                ref = R.replay_multinomial(bias, T, seed, N, L_SAMPLE, vid=_inputs(N)['vid_host'])
                R.input_conditions(ref, marked, kind)
                full, lp, width, vw = _sample(entry, N, ps, T, seed)
                c = R.check_draws(full, ref)
                print('select-draws', entry, N, V1, kind, T, hex(seed), c)
                assert c['bad_a'] == 0 and c['bad_b'] == 0, (T, seed, c)
                assert np.array_equal(full, R.emitted(full))                      # zero behind each row's <eos>
                assert width == ref['T_out'], (width, ref['T_out'])
                assert np.array_equal(full, ref['seq']) or c['differ'] > 0
                if vw is not None:
                    assert vw.tolist() == ref['video_words'][:-1].tolist()
                # log-probs: the un-tempered log-softmax value of the token the device drew, wherever it was emitted
                ob = ref['observable'] & (np.arange(L_SAMPLE)[None, :] < (width if entry == 'batch' else L_SAMPLE))
                raw = np.where(ob, full, 0)
                assert np.isfinite(lp).all()
                assert np.abs(lp - (x[raw] - lse))[ob].max(initial=0.0) < TOL_LOGP
                same = ob & (full == ref['tok'])
                assert np.abs(lp - ref['logp'])[same].max(initial=0.0) < TOL_LOGP
    finally:
        if entry == 'eval_plain':
            lib.echr_config_set(b'gemm_h2', 1)
    assert lib.echr_check_async() == 0


# ---- 5. greedy ties and negative rows ---------------------------------------------------------------------------------------------
GREEDY_FORMS = ([('persist', V1, N) for V1 in (5001, 5121, 10241) for N in (5, 64)]
                + [('chain', V1, N) for V1 in (2048, 2049, 5121, 12289) for N in (5, 64)]          # greedy_step_kernel<8>, <20>, <48>, <0>
                + [('many', 5121, 192)])
GREEDY_KINDS = ('ties', 'ties_high', 'ties_far', 'negative', 'eos_tie')


@pytest.mark.parametrize('kind', GREEDY_KINDS)
@pytest.mark.parametrize('form,V1,N', GREEDY_FORMS)
def test_greedy_takes_the_lowest_index_on_exact_ties(form, V1, N, kind):
    """Exact ties of the row maximum (select_ref.greedy_ties_design) through the persistent decoder (the 64-bit ordered-key atomic max over
    64 logits workgroups of 80 columns, one to three column chunks), the launch-per-step chain (greedy_step_kernel<8>, <20>, <48>, <0> at
    V1 = 2048, 2049, 5121, 12289) and the batched many-row chain (h2 logits): the lowest tied index at every row and step, also on an
    all-negative row; a tie with <eos> ends every row at once.  Two runs are bit-identical."""
    from echr_amd import functional as EF
    lib = _lib()
    bias, want, _ = R.greedy_ties_design(V1, kind)
    ps = _with_bias(V1, bias)
    i = _inputs(N)
    assert lib.echr_config_set(b'persist_sample', 1 if form in ('persist', 'many') else 0) == 0
    if form == 'many':
        assert lib.echr_config_set(b'persist_sample_max', 100) == 0
    runs = []
    try:
        for _ in range(2):
            dbg = {}
            seq, slp = EF.greedy_sample(i['video'], i['event'], i['c3d'], i['ev_start'], i['ev_len'], i['A'], L_GREEDY, ps, debug=dbg)
            runs.append((seq, slp, dbg))
    finally:
        lib.echr_config_set(b'persist_sample', 1)
        lib.echr_config_set(b'persist_sample_max', 512)
    seq, slp, dbg = runs[0]
    full, lp = dbg['seq_full'].cpu().numpy(), dbg['logp_full'].double().cpu().numpy()
    assert np.isfinite(lp).all()
    if form != 'persist':          # (the persistent decoder keeps its logits on chip)
        assert torch.equal(dbg['last_logits'], ps[2].expand(N, -1))
    assert (full == want).all(), (np.unique(full).tolist(), want)
    if kind == 'eos_tie':
        assert isinstance(seq, list) and seq == [] and slp == []          # the module path's empty result
        assert np.abs(lp[:, 0] - R.greedy_logp(bias, 0)).max() < TOL_LOGP
        if form == 'persist':
            assert dbg['stopped_early'] == 1          # (one 64-event group: the persistent launch leaves at the step nobody is unfinished)
    else:
        assert tuple(seq.shape) == (N, L_GREEDY) and np.array_equal(seq.cpu().numpy(), full)
        assert np.abs(lp - R.greedy_logp(bias, want)).max() < TOL_LOGP
    assert torch.equal(runs[1][2]['seq_full'], dbg['seq_full']) and torch.equal(runs[1][2]['logp_full'], dbg['logp_full'])
    assert lib.echr_check_async() == 0


# ---- 6. beam ties -----------------------------------------------------------------------------------------------------------------
BEAM_EVENTS = 4
BEAM_PARAMS = [(V1, B, kind) for V1 in (512, 513, 2049, 5121) for B in (1, 3, 16) for kind in ('one', 'one_eos', 'two') if not (kind == 'two' and B == 1)]


@functools.lru_cache(maxsize=None)
def _beam_case(V1, B, kind):
    bias, Lb = R.beam_class_design(V1, B, kind)
    return bias, Lb, R.beam_reference(bias, BEAM_EVENTS, B, Lb)


def _check_beam(seq, logp, score, ref, Lb):
    N = ref['words'].shape[0]
    T = int(ref['words'].max())
    assert _width(seq) == T
    got = _np(seq, N, T)
    assert np.array_equal(got, ref['seq'])
    assert np.array_equal((got != 0).sum(1), ref['words'])
    sc = score.double().cpu().numpy()
    assert np.isfinite(sc).all()
    tokens = np.minimum(ref['words'] + 1, Lb)          # (<eos> included when the result ends inside Lb steps)
    assert (np.abs(sc - ref['score']) <= TOL_LOGP * tokens).all(), (sc, ref['score'])
    if T:
        lp = logp.double().cpu().numpy()
        assert np.isfinite(lp).all() and np.abs(lp - ref['logp']).max() < TOL_LOGP


@pytest.mark.parametrize('V1,B,kind', BEAM_PARAMS)
def test_beam_ties_go_to_the_smaller_slot_then_the_smaller_token(V1, B, kind):
    """beam_step_kernel<8 | 32 | 80 | 0> (V1 = 512, 513, 2049, 5121) on logits whose candidates tie exactly in float32 and in float64
    (select_ref.beam_class_design) against tests/beam_ref.beam_search on the float64 log-softmax of the same row: one class (the tie rules
    decide the whole search), one class with <eos> in it (<eos> takes slot 0 at once; equal or lower scores never replace the result), two
    classes over two steps (x + y against y + x across slots)."""
    from echr_amd import functional as EF
    bias, Lb, ref = _beam_case(V1, B, kind)
    ps = _with_bias(V1, bias)
    i = _inputs(BEAM_EVENTS)
    seq, logp, score = EF.beam_search(i['video'], i['event'], i['c3d'], i['ev_start'], i['ev_len'], i['A'], Lb, ps, B)
    _check_beam(seq, logp, score, ref, Lb)
    assert _lib().echr_check_async() == 0


@pytest.mark.parametrize('V1,B,kind', [(2049, 3, 'one'), (513, 16, 'two')])
def test_beam_ties_over_a_two_video_batch(V1, B, kind):
    from echr_amd import functional as EF
    bias, Lb, ref = _beam_case(V1, B, kind)
    ps = _with_bias(V1, bias)
    i = _inputs(BEAM_EVENTS)
    vid = torch.tensor([0, 0, 1, 1], dtype=torch.int32, device='cuda')
    seq, logp, score, vw = EF.beam_search_batch(i['videos'][:2].contiguous(), i['event'], i['c3d'], i['ev_start'], i['ev_len'], vid, i['A'], Lb, ps, B)
    _check_beam(seq, logp, score, ref, Lb)
    assert vw.tolist() == [int(ref['words'][:2].max()), int(ref['words'][2:].max())]
    assert _lib().echr_check_async() == 0

"""CPU: the argument contract of the functional layer's decode and autograd entries -- beam_search, beam_search_batch, greedy_sample,
sample_train_batch, InitState and DecoderFunction, each in its single-video and its batched (vid=) form -- against the refusals recorded
BEFORE the single and the batched forms shared one Function / one launcher (tests/golden/functional_contract.json: the batched rows were
recorded through the then separate InitStateBatch / DecoderBatchFunction with the same arguments).

Every call runs on CPU tensors, where each path ends in a Python refusal or in EchrHipError (the library has no CPU path: _lib.ptr refuses
the first tensor) before any kernel runs.  One valid argument set per entry with ONE thing wrong; a record is (entry, variation, exception
type, message) and both are compared.  The refusal of `prep` together with `vid` is new with the shared DecoderFunction and asserted on its
own.  Also here: _stop_step on count vectors, and that the `keep` object of the decode set-up holds the per-slot repeated rows.
"""
import json
import os

import pytest
import torch

from echr_amd import functional as EF
from echr_amd._lib import EchrHipError

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'functional_contract.json')
V1, E, H, Ha, N, V, De, D, Dv, T, SEQ = 7, 4, 4, 4, 5, 2, 6, 4, 3, 9, 5


def base():
    """A valid argument set: V = 2 videos with 2 + 3 events over T = 9 rows; 'video' is the batched [V, Dv], 'video_one' a single video's."""
    z = torch.zeros
    params = [z(V1, E), z(V1, 3 * H), z(V1), z(4 * H, E + De), z(4 * H, E + D), z(4 * H, E + Dv)] + [z(4 * H, H)] * 3 + [z(4 * H)] * 6 + \
             [z(Ha, D), z(Ha), z(Ha, H), z(Ha), z(1, Ha), z(1)]
    f = lambda *s: torch.arange(float(torch.Size(s).numel())).reshape(*s)
    return dict(video=f(V, Dv), video_one=f(Dv), event=f(N, De), c3d=f(T, D), ev_start=torch.arange(N, dtype=torch.int32),
                ev_len=torch.ones(N, dtype=torch.int32), vid=torch.tensor([0, 0, 1, 1, 1], dtype=torch.int32), params=params, beam_size=2,
                tokens=torch.zeros(3, N, dtype=torch.int32), h0=f(N, 3 * H), tap=f(T, D), w=z(3 * H, Dv + De + D), b=z(3 * H),
                drop=EF.DropState(training=True), greedy_drop=None, multinomial=False)


USE = (True, True, True)
CALLS = {
    'beam_search': lambda a: EF.beam_search(a['video_one'], a['event'], a['c3d'], a['ev_start'], a['ev_len'], 1, SEQ, a['params'], a['beam_size']),
    'beam_search_batch': lambda a: EF.beam_search_batch(a['video'], a['event'], a['c3d'], a['ev_start'], a['ev_len'], a['vid'], 1, SEQ, a['params'],
                                                        a['beam_size']),
    'greedy_sample': lambda a: EF.greedy_sample(a['video_one'], a['event'], a['c3d'], a['ev_start'], a['ev_len'], 1, SEQ, a['params'],
                                                multinomial=a['multinomial'], drop=a['greedy_drop']),
    'greedy_sample(vid=)': lambda a: EF.greedy_sample(a['video'], a['event'], a['c3d'], a['ev_start'], a['ev_len'], 1, SEQ, a['params'],
                                                      multinomial=a['multinomial'], drop=a['greedy_drop'], vid=a['vid'], h0=a['h0']),
    'sample_train_batch': lambda a: EF.sample_train_batch(a['video'], a['event'], a['c3d'], a['ev_start'], a['ev_len'], a['vid'], 1, SEQ, a['params'],
                                                          a['drop']),
    'InitState': lambda a: EF.InitState.apply(a['video_one'], a['event'], a['c3d'], a['ev_start'], a['ev_len'], 1, None, USE, None, a['w'], a['b']),
    'InitState(vid=)': lambda a: EF.InitState.apply(a['video'], a['event'], a['c3d'], a['ev_start'], a['ev_len'], 0, a['vid'], USE, None, a['w'], a['b']),
    'DecoderFunction': lambda a: EF.DecoderFunction.apply(a['video_one'], a['event'], a['c3d'], a['ev_start'], a['ev_len'], a['tokens'], 1, False,
                                                          a['drop'], None, None, None, None, 0, None, *a['params']),
    'DecoderFunction(vid=)': lambda a: EF.DecoderFunction.apply(a['video'], a['event'], a['c3d'], a['ev_start'], a['ev_len'], a['tokens'], 1, False,
                                                                a['drop'], None, None, a['h0'], a['tap'], 0, a['vid'], *a['params']),
}
BEAM = ('beam_search', 'beam_search_batch')
BATCHED = ('beam_search_batch', 'greedy_sample(vid=)', 'sample_train_batch', 'InitState(vid=)', 'DecoderFunction(vid=)')
GREEDY = ('greedy_sample', 'greedy_sample(vid=)')
INIT = ('InitState', 'InitState(vid=)')
EVERY = tuple(CALLS)


def _swap_video(a):
    a['video'], a['video_one'] = a['video_one'], a['video']


# (variation, the entries it is applied to, the edit of the valid argument set)
VARIATIONS = [
    ('valid arguments on the CPU', EVERY, lambda a: None),
    ('beam_size 0', BEAM, lambda a: a.update(beam_size=0)),
    ('beam_size above the vocabulary', BEAM, lambda a: a.update(beam_size=V1 + 1)),
    ('beam_size above BEAM_MAX', BEAM, lambda a: a.update(beam_size=EF.BEAM_MAX + 1)),
    ('video of the wrong rank', EVERY, _swap_video),
    ('vid one entry short', BATCHED, lambda a: a.update(vid=a['vid'][:-1])),
    ('ev_start one entry short', EVERY, lambda a: a.update(ev_start=a['ev_start'][:-1])),
    ('ev_len one entry short', EVERY, lambda a: a.update(ev_len=a['ev_len'][:-1])),
    ('V > N', BATCHED, lambda a: a.update(video=torch.zeros(N + 1, Dv))),
    ('drop without multinomial', GREEDY, lambda a: a.update(greedy_drop=a['drop'])),
    ('vid with multinomial', ('greedy_sample(vid=)',), lambda a: a.update(multinomial=True)),
    ('drop missing', ('sample_train_batch',), lambda a: a.update(drop=None)),
    ('init_linear width mismatch', INIT, lambda a: a.update(w=torch.zeros(3 * H, Dv + De + D + 1))),
]


def record(calls=CALLS):
    out = []
    for variation, entries, edit in VARIATIONS:
        for e in entries:
            a = base()
            edit(a)
            try:
                calls[e](a)
                out.append([e, variation, '', ''])
            except Exception as ex:          # noqa: BLE001 (the record IS the exception)
                out.append([e, variation, type(ex).__name__, str(ex)])
    return out


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_every_recorded_call_was_refused():
    """The fixture itself: every call ended in an exception, the valid ones in the library's EchrHipError, and the Python refusals that the
    other host tests match on are among them."""
    want = _fixture()
    assert len(want) == sum(len(entries) for _, entries, _ in VARIATIONS) and all(r[2] for r in want)
    by = {(e, v): (t, m) for e, v, t, m in want}
    assert all(by[e, 'valid arguments on the CPU'][0] == 'EchrHipError' for e in EVERY)
    for e in BEAM:
        assert by[e, 'beam_size 0'][0] == by[e, 'beam_size above BEAM_MAX'][0] == 'ValueError' and 'beam_size' in by[e, 'beam_size 0'][1]
    for e in ('beam_search_batch', 'sample_train_batch'):
        assert by[e, 'video of the wrong rank'] == ('ValueError', 'video must be [V, Dv], one scene vector per video (got (3,))')
        for v in ('vid', 'ev_start', 'ev_len'):
            assert by[e, v + ' one entry short'][0] == 'ValueError' and 'one entry per event' in by[e, v + ' one entry short'][1]
        assert by[e, 'V > N'][0] == 'ValueError' and 'between 1 video' in by[e, 'V > N'][1]
    assert by['greedy_sample(vid=)', 'vid with multinomial'][0] == 'NotImplementedError'
    assert by['greedy_sample', 'drop without multinomial'][0] == by['sample_train_batch', 'drop missing'][0] == 'ValueError'
    assert all(by[e, 'init_linear width mismatch'] == ('EchrHipError', 'init_linear is 14 wide, the selected contexts give 13') for e in INIT)


def test_refusals_are_the_recorded_ones():
    got, want = record(), _fixture()
    assert [r[:2] for r in got] == [r[:2] for r in want]
    for g, w in zip(got, want):
        assert g == w, (g, w)


def test_prepared_forward_with_a_batch_is_refused_in_python():
    a = base()
    with pytest.raises(ValueError, match='decoder_prepare'):
        EF.DecoderFunction.apply(a['video'], a['event'], a['c3d'], a['ev_start'], a['ev_len'], a['tokens'], 1, False, a['drop'], None, dict(), None,
                                 None, 0, a['vid'], *a['params'])


def test_decoder_input_positions():
    """The two module constants name where h0 and tap sit among DecoderFunction's inputs (backward indexes needs_input_grad with them)."""
    names = EF.DecoderFunction.forward.__code__.co_varnames[1:]
    assert names[EF.DEC_H0_ARG] == 'h0' and names[EF.DEC_TAP_ARG] == 'tap' and names[:15].index('vid') == 14


def test_stop_step():
    """The first step with nobody unfinished (counts[t], t = 1 .. L; counts[0] is not a step)."""
    assert EF._stop_step([0, 0, 0, 0, 0], 4) == 0          # all zero from step 1 on
    assert EF._stop_step([1, 0, 0, 0, 0], 4) == 0          # (counts[0] is the launch's own flag)
    assert EF._stop_step([0, 5, 3, 1, 1], 4) == 4          # never zero
    assert EF._stop_step([0, 5, 3, 1, 0], 4) == 3          # zero at the last step
    assert EF._stop_step([0, 5, 0, 2, 0], 4) == 1          # the FIRST zero counts
    assert EF._stop_step([0, 5, 3, 1, 1, 0, 0, 2], 4) == 4          # entries behind L + 1 (a batch's widths) are not steps


def test_keep_holds_the_repeated_rows():
    """rep > 1: the rows the call's arguments point to are the per-slot repeats, and they are the tensors `keep` holds (event-major: row n * rep
    + j is slot j of event n); what is shared between the slots, and everything at rep = 1, is the caller's own tensor."""
    a = base()
    k = EF._decode_inputs(a['video'], a['event'], a['c3d'], a['ev_start'], a['ev_len'], a['params'], a['h0'], a['vid'], rep=3)
    for name in ('event', 'ev_start', 'ev_len', 'h0', 'vid'):
        t = getattr(k, name)
        assert t is not a[name] and t.shape[0] == 3 * N and t.is_contiguous() and torch.equal(t, a[name].repeat_interleave(3, 0)), name
    assert k.video is a['video'] and k.c3d is a['c3d'] and all(p is q for p, q in zip(k.ps, a['params']))
    k = EF._decode_inputs(a['video_one'], a['event'], a['c3d'], a['ev_start'], a['ev_len'], a['params'], None, None)
    assert k.event is a['event'] and k.ev_start is a['ev_start'] and k.ev_len is a['ev_len'] and k.h0 is None and k.vid is None
    half = a['event'].to(torch.float16)          # a converted input is held too: the call reads the fp32 copy
    k = EF._decode_inputs(a['video_one'], half, a['c3d'], a['ev_start'], a['ev_len'], a['params'], None, None)
    assert k.event.dtype is torch.float32 and torch.equal(k.event, a['event'])

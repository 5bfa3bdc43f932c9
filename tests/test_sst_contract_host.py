"""CPU: the refusal contract of the proposal encoder -- the six C entries echr_sst_fwd, echr_sst_fwd_states, echr_sst_head_fwd, echr_sst_bwd,
echr_sst_fwd_batch and echr_sst_bwd_batch, the Python layer (SST.forward / SST.forward_batch) and the four workspace-size entries -- against
what was recorded BEFORE the single-video and the batched call shared one forward and one backward (tests/golden/sst_contract.json).

Every C call is a valid argument set with exactly ONE thing wrong, so it is refused by the entry's own checks before the first HIP call: the
device pointers are a made-up address that nothing dereferences, only row_offset_host is real memory (the checks read it).  A record is
(entry, variation, return code, echr_last_error() text); all four are compared.  No valid call is sent: `test_every_recorded_call_was_refused`
holds the fixture to that.  The batch entries are recorded over three videos and over one (`(V=1)`), because a one-video batch is the
single-video call and answers with its names.  Workspace sizes may shrink but not grow.
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from echr_amd import _lib as L
from echr_amd import models, synth

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sst_contract.json')
ADDR = 0x10000          # stands for every device pointer: never dereferenced, every call ends in the checks
T, D, H, K = 9, 20, 24, 8
OFFSETS = {3: [0, 3, 7, 9], 1: [0, 9]}


class Call:
    """One valid argument set: echr_sst_args, echr_sst_grads, echr_sst_batch over V videos, echr_dropout."""

    def __init__(self, V):
        two = lambda: (L.c_f * 2)(ADDR, ADDR)
        self.a = L.SstArgs(T, D, H, K, 0.5, two(), two(), two(), two(), ADDR, ADDR, ADDR, ADDR, ADDR, ADDR)
        self.g = L.SstGrads(two(), two(), two(), two(), ADDR, ADDR, ADDR, ADDR, ADDR, 0)
        self.x = L.SstBatch(V, ADDR, None)
        self.drop = L.Dropout(1, 0, 1, 0.0, 0.0, 0.0)
        self.null_args = self.null_grads = self.null_batch = False
        self.offsets(OFFSETS[V])

    def offsets(self, ro):
        self.ro = np.ascontiguousarray(np.asarray(ro, dtype=np.int32))          # (held here: the struct keeps the bare address)
        self.x.row_offset_host = self.ro.ctypes.data

    def refs(self):
        return (None if self.null_args else C.byref(self.a), None if self.null_grads else C.byref(self.g),
                None if self.null_batch else C.byref(self.x), C.byref(self.drop))


def _entries():
    lib = L.load()

    def fwd(name):
        return lambda c, V: getattr(lib, name)(c.refs()[0], c.refs()[3], None)
    return {
        'echr_sst_fwd': fwd('echr_sst_fwd'),
        'echr_sst_fwd_states': fwd('echr_sst_fwd_states'),
        'echr_sst_head_fwd': lambda c, V: lib.echr_sst_head_fwd(c.refs()[0], None),
        'echr_sst_bwd': lambda c, V: lib.echr_sst_bwd(c.refs()[0], c.refs()[1], c.refs()[3], None),
        'echr_sst_fwd_batch': lambda c, V: lib.echr_sst_fwd_batch(c.refs()[0], c.refs()[2], c.refs()[3], None),
        'echr_sst_bwd_batch': lambda c, V: lib.echr_sst_bwd_batch(c.refs()[0], c.refs()[2], c.refs()[1], c.refs()[3], None),
    }


SINGLE = ('echr_sst_fwd', 'echr_sst_fwd_states', 'echr_sst_head_fwd', 'echr_sst_bwd')
BATCH = ('echr_sst_fwd_batch', 'echr_sst_bwd_batch')
BWD = ('echr_sst_bwd', 'echr_sst_bwd_batch')
EVERY = SINGLE + BATCH


def _set(path, value):
    def edit(c):
        obj, name = (c.a, path) if not path.startswith('g.') else (c.g, path[2:])
        if '[' in name:
            name, i = name[:-3], int(name[-2])
            getattr(obj, name)[i] = value
        else:
            setattr(obj, name, value)
    return edit


def _too_long(c):
    c.a.T, c.a.H = 1 << 19, 4096          # T_tot * H = 2^31
    c.offsets(list(c.ro[:-1]) + [1 << 19])


# (variation, the entries it is refused by, the edit of the valid argument set)
VARIATIONS = [
    ('null args', EVERY, lambda c: setattr(c, 'null_args', True)),
    ('H % 4 != 0', EVERY, _set('H', 22)),
    ('H > 4096', EVERY, _set('H', 4100)),
    ('T = 0', EVERY, _set('T', 0)),
    ('null x', EVERY, _set('x', None)),
    ('null ws', EVERY, _set('ws', None)),
    ('null tap_feats', EVERY, _set('tap_feats', None)),
    ('null scores', EVERY, _set('scores', None)),
    ('null w_ih[0]', EVERY, _set('w_ih[0]', None)),
    ('null b_hh[1]', EVERY, _set('b_hh[1]', None)),
    ('null w_sc', EVERY, _set('w_sc', None)),
    ('null b_sc', EVERY, _set('b_sc', None)),
    ('null grads', BWD, lambda c: setattr(c, 'null_grads', True)),
    ('null ws_bwd', BWD, _set('g.ws_bwd', None)),
    ('both upstream gradients null', BWD, lambda c: (_set('g.g_tap', None)(c), _set('g.g_scores', None)(c))),
    ('null batch', BATCH, lambda c: setattr(c, 'null_batch', True)),
    ('n_videos = 0', BATCH, lambda c: setattr(c.x, 'n_videos', 0)),
    ('null row_offset', BATCH, lambda c: setattr(c.x, 'row_offset', None)),
    ('null row_offset_host', BATCH, lambda c: setattr(c.x, 'row_offset_host', None)),
    ('offsets start at 1', BATCH, lambda c: c.offsets([1] + list(c.ro[1:]))),
    ('offsets end at T - 1', BATCH, lambda c: c.offsets(list(c.ro[:-1]) + [T - 1])),
    ('a video with no row', BATCH, lambda c: c.offsets([0, 3, 3, 9] if len(c.ro) == 4 else [0, 0])),
    ('T * H = 2^31', BATCH, _too_long),
]


def record_c():
    lib, entries, out = L.load(), _entries(), []
    for variation, names, edit in VARIATIONS:
        for e in names:
            for V in ((3, 1) if e in BATCH else (None,)):
                if V == 1 and variation == 'a video with no row':
                    continue          # (a one-video batch without a row IS 'offsets end at T - 1' or 'T = 0': more than one thing wrong)
                c = Call(V or 1)
                edit(c)
                rc = entries[e](c, V)
                msg = lib.echr_last_error() if rc else b''
                out.append([e if V != 1 else e + '(V=1)', variation, rc, msg.decode() if msg else ''])
    return out


def _sst():
    return models.setup_tap(synth.default_opt(video_dim=D, hidden_dim=H, K=K))


PY_CALLS = [
    ('SST.forward', 'CPU tensor', lambda m: m(torch.zeros(7, D))),
    ('SST.forward_batch', 'CPU matrix', lambda m: m.forward_batch(torch.zeros(7, D), [0, 3, 7])),
    ('SST.forward_batch', 'CPU matrix, one video', lambda m: m.forward_batch(torch.zeros(7, D), [0, 7])),
    ('SST.forward_batch', 'CPU list', lambda m: m.forward_batch([torch.zeros(3, D), torch.zeros(4, D)])),
    ('SST.forward_batch', 'matrix without offsets', lambda m: m.forward_batch(torch.zeros(7, D))),
    ('SST.forward_batch', 'list with offsets', lambda m: m.forward_batch([torch.zeros(7, D)], [0, 7])),
    ('SST.forward_batch', 'empty list', lambda m: m.forward_batch([])),
    ('SST.forward_batch', 'a video of rank 1', lambda m: m.forward_batch([torch.zeros(D)])),
    ('SST.forward_batch', 'matrix of rank 3', lambda m: m.forward_batch(torch.zeros(1, 7, D), [0, 7])),
    ('SST.forward_batch', 'list with an empty video', lambda m: m.forward_batch([torch.zeros(3, D), torch.zeros(0, D)])),
] + [('SST.forward_batch', 'offsets %s' % ro, (lambda ro: lambda m: m.forward_batch(torch.zeros(7, D), ro))(ro))
     for ro in ([1, 3, 7], [0, 3, 3, 7], [0, 3, 6], [0, 3, 9], [0], [0, 5, 3, 7], [0.5, 7])]


def record_py():
    out = []
    for entry, variation, call in PY_CALLS:
        try:
            call(_sst())
            out.append([entry, variation, '', ''])
        except Exception as ex:          # noqa: BLE001 (the record IS the exception)
            out.append([entry, variation, type(ex).__name__, str(ex)])
    return out


SHAPES = [(1, 20, 24, 8, 1), (5, 20, 24, 8, 1), (8, 20, 24, 8, 3), (1, 500, 512, 16, 1), (37, 500, 512, 16, 1), (50, 500, 512, 16, 5),
          (50, 500, 512, 16, 9), (256, 500, 512, 256, 8), (33, 7, 4096, 3, 33)]


def record_sizes():
    lib = L.load()
    return [[list(s), lib.echr_sst_ws_floats(*s[:4]), lib.echr_sst_ws_bwd_floats(*s[:4]), lib.echr_sst_batch_ws_floats(*s),
             lib.echr_sst_batch_ws_bwd_floats(*s)] for s in SHAPES]


def record():
    return dict(c=record_c(), python=record_py(), sizes=record_sizes())


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_every_recorded_call_was_refused():
    """The fixture itself: no call went through (a non-zero code and a message that names the entry's own `who`), every variation of the
    issue's list is there for every entry it applies to, and the Python layer refused with the two exception types the other tests match on."""
    want = _fixture()
    assert all(rc != 0 and msg for _, _, rc, msg in want['c'])
    n_batch = sum(len([e for e in names if e in BATCH]) for _, names, _ in VARIATIONS)
    assert len(want['c']) == sum(len(names) for _, names, _ in VARIATIONS) + n_batch - len(BATCH)
    by = {(e, v): m for e, v, _, m in want['c']}
    assert by['echr_sst_fwd_states', 'T = 0'].startswith('sst_fwd:') and by['echr_sst_head_fwd', 'null w_sc'].startswith('sst_head_fwd:')
    assert by['echr_sst_bwd_batch', 'null grads'] == 'sst_bwd_batch: missing buffers' and by['echr_sst_bwd_batch(V=1)', 'null grads'] == 'sst_bwd: missing buffers'
    assert '2^31' in by['echr_sst_fwd_batch', 'T * H = 2^31'] and 'video 1 has no row' in by['echr_sst_bwd_batch', 'a video with no row']
    assert all(t in ('EchrHipError', 'ValueError') for _, _, t, _ in want['python'])
    assert [r[0] for r in want['sizes']] == [list(s) for s in SHAPES]


def test_c_refusals_are_the_recorded_ones():
    got, want = record_c(), _fixture()['c']
    assert [r[:2] for r in got] == [r[:2] for r in want]
    for g, w in zip(got, want):
        assert g == w, (g, w)


def test_python_refusals_are_the_recorded_ones():
    got, want = record_py(), _fixture()['python']
    assert [r[:2] for r in got] == [r[:2] for r in want]
    for g, w in zip(got, want):
        assert g == w, (g, w)


def test_workspaces_did_not_grow():
    for (shape, *got), (_, *want) in zip(record_sizes(), _fixture()['sizes']):
        assert all(0 < g <= w for g, w in zip(got, want)), (shape, got, want)

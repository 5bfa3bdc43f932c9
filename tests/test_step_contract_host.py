"""CPU: the argument contract of the six one-call train-step entries (echr_train_step, _rw, _clip, _batch, _batch_tap, _batch_clip;
csrc/step.hip validate_step) and of their workspace sizing, against values recorded from the library BEFORE the entries shared one
descriptor and one validator (tests/golden/step_contract.json).

Sizes: every echr_train_step*_ws_floats over SHAPES x clip_parts 1/2/3 x with / without init_linear x n_videos 1/3 x (host_nll, n_active)
-- arithmetic only.  Refusals: per entry, one valid argument set with ONE rule broken; the call is made with a NULL stream and must come
back with -22 and the recorded message before anything touches the device.  Every argument set here ends with do_step = 1 WITHOUT optimiser
state: that is the last check in front of the first device call, so a case whose own rule did not fire is refused there (and recorded as
such) instead of reaching a launch.  The pointers are the constant P: nothing in front of that check reads through them.

`python tests/test_step_contract_host.py --record` rewrites the fixture from the library that is built.
"""
import ctypes as C
import itertools
import json
import os
import sys

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from echr_amd import _lib as L

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_contract.json')
P = 0x1000          # a non-NULL "pointer"
ENTRIES = ('', '_rw', '_clip', '_batch', '_batch_tap', '_batch_clip')
#          N   S   V1     H    Dv   De   Dc
SHAPES = [(3, 3, 31, 8, 5, 6, 7),
          (4, 5, 301, 64, 100, 48, 20),
          (64, 20, 5001, 512, 100, 512, 500),
          (72, 7, 10241, 128, 612, 96, 33)]
CRITERION = ((0, 0), (1, 0), (1, 4))          # (host_nll, n_active)


def _args(shape, clip_parts=1, w_init=False, host_nll=1, n_active=0):
    """An argument struct every entry accepts up to `optimiser state missing` (ER3, scene context without 'VH')."""
    N, S, V1, H, Dv, De, Dc = shape
    a = L.TrainStepArgs()
    t, d = a.tsrm, a.dec
    a.Ht = H
    t.N, t.Din, t.Df, t.Do, t.G = N, Dc + H, De, De, 4
    d.N, d.A, d.Tv, d.H, d.E, d.Ha, d.De, d.Dv, d.V1, d.S = N, 4, 9, H, H, H, De, Dv, V1, S
    d.D = {1: Dc, 2: H, 3: Dc + H}[clip_parts]
    a.tap = a.host_index = a.loss = a.g_loss = a.flat_g = a.ws = P
    a.ws_floats = 1
    a.event_parts, a.vh_offset, a.overlap_encoder = 3, -1, 1
    a.host_nll, a.n_active = host_nll, n_active
    if not host_nll:
        a.nll_target = a.nll_mask = P
    if w_init:
        a.w_init = a.b_init = a.g_w_init = a.g_b_init = P
        a.init_use_v = a.init_use_e = 1
    a.do_step = 1          # flat_p / adam_m / adam_v stay NULL: see the module docstring
    return a


def _x(shape, clip_parts, rw=0):
    return L.ClipStepArgs(clip_parts, shape[6], P, rw, None)


def _bx(n_videos):
    return L.BatchExt(n_videos, None, P, None, None)


def sizes(lib):
    out = []
    for shape, cp, wi, V, (hn, na) in itertools.product(SHAPES, (1, 2, 3), (False, True), (1, 3), CRITERION):
        a, x, bx = _args(shape, cp, wi, hn, na), _x(shape, cp), _bx(V)
        ra, rx, rb = C.byref(a), C.byref(x), C.byref(bx)
        if cp == 1:
            row = [lib.echr_train_step_ws_floats(ra), lib.echr_train_step_rw_ws_floats(ra), lib.echr_train_step_batch_ws_floats(ra, rb),
                   lib.echr_train_step_batch_tap_ws_floats(ra, rb)]
        else:
            x1 = _x(shape, cp, 1)
            row = [lib.echr_train_step_clip_ws_floats(ra, rx), lib.echr_train_step_clip_ws_floats(ra, C.byref(x1)),
                   lib.echr_train_step_batch_clip_ws_floats(ra, rx, rb)]
        out.append(row)
    # the arguments every sizing function answers with -1
    a, x, bx, b0, x1 = _args(SHAPES[0]), _x(SHAPES[0], 2), _bx(1), _bx(0), _x(SHAPES[0], 1)
    ra, rx, rb = C.byref(a), C.byref(x), C.byref(bx)
    out.append([lib.echr_train_step_ws_floats(None), lib.echr_train_step_rw_ws_floats(None), lib.echr_train_step_clip_ws_floats(None, rx),
                lib.echr_train_step_clip_ws_floats(ra, None), lib.echr_train_step_batch_ws_floats(None, rb), lib.echr_train_step_batch_ws_floats(ra, None),
                lib.echr_train_step_batch_ws_floats(ra, C.byref(b0)), lib.echr_train_step_batch_tap_ws_floats(ra, C.byref(b0)),
                lib.echr_train_step_batch_clip_ws_floats(None, rx, rb), lib.echr_train_step_batch_clip_ws_floats(ra, None, rb),
                lib.echr_train_step_batch_clip_ws_floats(ra, rx, None), lib.echr_train_step_batch_clip_ws_floats(ra, rx, C.byref(b0)),
                lib.echr_train_step_batch_clip_ws_floats(ra, C.byref(x1), rb)])
    return out


class Call(object):
    """One call of `entry` on a valid argument set (batch_tap and the g_tap form of batch_clip with g_tap; the others without)."""

    def __init__(self, entry, clip_parts=3, g_tap=None, rw=0):
        self.entry = entry
        clip = 'clip' in entry
        self.a = _args(SHAPES[0], clip_parts if clip else 1)
        self.x = _x(SHAPES[0], clip_parts, rw) if clip else None
        self.bx = _bx(2) if 'batch' in entry else None
        self.weight, self.row_offset = None, P
        if entry == '_batch_tap' if g_tap is None else g_tap:
            self.a.g_tap = P
        self.null = ()

    def run(self, lib):
        ref = lambda name: None if (name in self.null or getattr(self, name) is None) else C.byref(getattr(self, name))
        a, x, bx, w, ro, e = ref('a'), ref('x'), ref('bx'), self.weight, self.row_offset, self.entry
        rc = {'': lambda: lib.echr_train_step(a, None), '_rw': lambda: lib.echr_train_step_rw(a, w, None),
              '_clip': lambda: lib.echr_train_step_clip(a, x, None), '_batch': lambda: lib.echr_train_step_batch(a, bx, w, P, None),
              '_batch_tap': lambda: lib.echr_train_step_batch_tap(a, bx, w, P, ro, None),
              '_batch_clip': lambda: lib.echr_train_step_batch_clip(a, x, bx, w, P, ro, None)}[e]()
        return [rc, (lib.echr_last_error() or b'').decode()]


def _set(path, value):
    def edit(c):
        obj, names = c, path.split('.')
        for n in names[:-1]:
            obj = getattr(obj, n)
        setattr(obj, names[-1], value)
    return edit


def _null(name):
    def edit(c):
        c.null = c.null + (name,)
    return edit


def _all(*edits):
    def edit(c):
        for e in edits:
            e(c)
    return edit


WEIGHTED = ('_rw', '_batch', '_batch_tap', '_batch_clip')
BATCHED = ('_batch', '_batch_tap', '_batch_clip')
CLIPPED = ('_clip', '_batch_clip')
# (rule, the entries that have it, the edit that breaks it, keyword arguments of Call)
RULES = [
    ('valid up to the optimiser state', ENTRIES, lambda c: None, {}),
    ('null args', ENTRIES, _null('a'), {}),
    # the checks at the head of the shared implementation, reached through every entry
    ('missing buffers', ENTRIES, _set('a.loss', None), {}),
    ('prepared without overlap_encoder', ('',), _all(_set('a.prepared', 1), _set('a.overlap_encoder', 0)), {}),
    ('event_parts', ENTRIES, _set('a.event_parts', 4), {}),
    ('shapes disagree', ENTRIES, _set('a.tsrm.Do', 5), {}),
    ('vh span', ('', '_clip', '_batch_tap', '_batch_clip'), _all(_set('a.g_tap', P), _set('a.vh_offset', 4), _set('a.tap_rows', 0)), {}),
    ('init_linear incomplete', ENTRIES, _set('a.w_init', P), {}),
    # criterion weights present and not given twice
    ('weights missing', WEIGHTED, _set('a.host_nll', 0), {}),
    ('weights twice', WEIGHTED, _set('weight', P), {}),
    ('weights missing', ('_clip',), _set('a.host_nll', 0), dict(rw=1)),
    ('weights twice', ('_clip',), _set('x.weight', P), dict(rw=1)),
    ('weights unread without rw', ('_clip',), _set('x.weight', P), dict(rw=0)),
    # 0 < n_videos <= N && video
    ('no batch extension', BATCHED, _null('bx'), {}),
    ('n_videos 0', BATCHED, _set('bx.n_videos', 0), {}),
    ('n_videos > N', BATCHED, _set('bx.n_videos', 4), {}),
    ('no video', BATCHED, _set('bx.video', None), {}),
    # clip_parts 2 or 3, with dec.D matching
    ('no clip extension', CLIPPED, _null('x'), {}),
    ('clip_parts 1', CLIPPED, _set('x.clip_parts', 1), {}),
    ('c3d missing', CLIPPED, _set('x.c3d', None), {}),
    ('tap missing', CLIPPED, _set('a.tap', None), {}),
    ('dec.D of CC+CH', CLIPPED, _set('a.dec.D', 7), dict(clip_parts=3)),
    ('dec.D of CH', CLIPPED, _set('a.dec.D', 7), dict(clip_parts=2)),
    # prepared / defer_update / mid_cb / g_tap
    ('prepared', ('_rw', '_clip') + BATCHED, _set('a.prepared', 1), {}),
    ('defer_update', BATCHED, _set('a.defer_update', 1), {}),
    ('mid_cb', ('_batch_tap', '_batch_clip'), _set('a.mid_cb', P), {}),
    ('mid_cb unread', ('_batch',), _set('a.mid_cb', P), {}),
    ('g_tap refused', ('_batch',), _set('a.g_tap', P), {}),
    ('g_tap required', ('_batch_tap',), _set('a.g_tap', None), {}),
    ('g_tap with forward_only', ('_batch_tap', '_batch_clip'), _set('a.forward_only', 1), dict(g_tap=True)),
    ('g_tap either way', ('_batch_clip',), lambda c: None, dict(g_tap=True)),
    # handover needs do_step = 0
    ('handover with do_step', BATCHED, _set('a.handover', 1), {}),
    # 'VH' needs row_offset
    ('VH without row_offset', ('_batch_tap', '_batch_clip'), _all(_set('a.vh_offset', 0), _set('a.tap_rows', 9), _set('row_offset', None)), dict(g_tap=True)),
    ('VH without g_tap needs none', ('_batch_clip',), _all(_set('a.vh_offset', 0), _set('row_offset', None)), {}),
    # an initial state that reads the clip has no row gradient
    ('init_use_c', CLIPPED, _all(_set('a.w_init', P), _set('a.b_init', P), _set('a.init_use_c', 1)), {}),
    # the order of the checks: two rules broken, the earlier one reports
    ('prepared before init_use_c', ('_clip',), _all(_set('a.prepared', 1), _set('a.w_init', P), _set('a.init_use_c', 1)), {}),
    ('init_use_c before weights', ('_clip',), _all(_set('a.w_init', P), _set('a.init_use_c', 1), _set('a.host_nll', 0)), dict(rw=1)),
    ('weights before init_use_c', ('_batch_clip',), _all(_set('a.w_init', P), _set('a.init_use_c', 1), _set('a.host_nll', 0)), {}),
    ('VH before prepared', ('_batch_tap',), _all(_set('a.vh_offset', 0), _set('row_offset', None), _set('a.prepared', 1)), {}),
    ('prepared before VH', ('_batch_clip',), _all(_set('a.vh_offset', 0), _set('row_offset', None), _set('a.prepared', 1)), dict(g_tap=True)),
    ('handover before init_use_c', ('_batch_clip',), _all(_set('a.handover', 1), _set('a.w_init', P), _set('a.init_use_c', 1)), {}),
    ('weights before g_tap', ('_batch', '_batch_tap'), _all(_set('a.host_nll', 0), _set('a.g_tap', None), _set('a.prepared', 1)), {}),
    ('extension before clip rows', ('_batch_clip',), _all(_set('bx.n_videos', 0), _set('x.c3d', None)), {}),
]


def refused(lib):
    out = {}
    for rule, entries, edit, kw in RULES:
        for e in entries:
            c = Call(e, **kw)
            edit(c)
            key = 'train_step%s: %s%s' % (e, rule, ''.join(' %s=%s' % kv for kv in sorted(kw.items())))
            assert key not in out, key
            out[key] = c.run(lib)
    return out


def record(lib):
    return dict(sizes=sizes(lib), refused=refused(lib))


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_every_case_is_refused_before_the_device():
    """The fixture itself: every recorded call came back -22 with a message that names the entry or the shared implementation."""
    want = _fixture()['refused']
    assert len(want) > 100
    for key, (rc, msg) in want.items():
        assert rc == -22 and msg.startswith('train_step'), (key, rc, msg)
    heads = {key.split(':')[0] for key in want}
    assert heads == {'train_step' + e for e in ENTRIES}


def test_workspace_sizes_are_the_recorded_ones():
    got, want = sizes(L.load()), _fixture()['sizes']
    assert len(got) == len(want) == len(SHAPES) * 3 * 2 * 2 * len(CRITERION) + 1
    assert all(s > 0 for row in want[:-1] for s in row) and all(s == -1 for s in want[-1])
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)


def test_refusals_are_the_recorded_ones():
    got, want = refused(L.load()), _fixture()['refused']
    assert set(got) == set(want)
    for key in want:
        assert got[key] == want[key], (key, got[key], want[key])


if __name__ == '__main__':
    if '--record' not in sys.argv:
        sys.exit('usage: python tests/test_step_contract_host.py --record')
    rec = record(L.load())
    for key, (rc, msg) in rec['refused'].items():
        assert rc == -22, (key, rc, msg)          # (anything else went past the argument checks)
    with open(FIXTURE, 'w') as f:
        row = lambda items: ',\n'.join('  ' + json.dumps(i) for i in items)          # one case per line
        f.write('{\n "refused": {\n%s\n },\n "sizes": [\n%s\n ]\n}\n'
                % (row(sorted(rec['refused'].items())).replace('["train', '"train').replace('", [', '": [').replace(']]', ']'), row(rec['sizes'])))
    print('wrote %s: %d size rows, %d refused calls' % (FIXTURE, len(rec['sizes']), len(rec['refused'])))

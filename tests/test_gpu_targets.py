"""Proposal targets and caption-event samples on the GPU (-m gpu): echr_amd.targets.build (echr_tap_targets_batch, echr_prop_events_batch)
against tests/targets_ref.py, which tests/test_targets_host.py pins to the reference's recorded outputs.  Everything is compared EXACTLY:
iou as float32 bits, every index and label matrix, n_good, both event forms.  The arithmetic is correctly rounded fp64 without a product,
and the sample is a pure function of integer keys, so there is no tolerance to state."""
import functools

import numpy as np
import pytest
import torch

from echr_amd import synth
from tests import targets_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD5EED0123          # (both halves of the key are non-zero)


def _stamps(rs, T, G):
    """G random segments of a T-row video (T >= 2)."""
    out = []
    for _ in range(G):
        s = int(rs.randint(0, T - 1))
        out.append((s, int(rs.randint(s + 1, T))))
    return out


@functools.lru_cache(maxsize=None)
def _oracle(T, K, stamps, thr=0.5, good=0.8):
    return R.video_targets(T, K, np.asarray(stamps, np.int64).reshape(-1, 2), thr, good)


def _key(videos):
    return [(int(T), tuple(tuple(int(x) for x in s) for s in st)) for T, st in videos]


def _check(videos, K, cap, seed=SEED, draw=None, thr=0.5, good=0.8):
    """build in both event forms against the oracle, video by video; returns (sampled Targets, the oracle's per-video dicts)."""
    from echr_amd import targets as TG
    videos = _key(videos)
    V = len(videos)
    draw = list(range(V)) if draw is None else list(draw)
    ts = TG.build(videos, K, thr, good, prop_sample_num=cap, seed=seed, events='sampled', draw=draw)
    ta = TG.build(videos, K, thr, good, prop_sample_num=cap, seed=seed, events='all', draw=draw)
    refs = [_oracle(T, K, st, thr, good) for T, st in videos]
    ro = np.concatenate([[0], np.cumsum([T for T, _ in videos])])
    assert np.array_equal(ts.row_offset, ro) and ts.row_offset.dtype == np.int32
    for t in (ts, ta):
        host = {k: getattr(t, k).cpu().numpy() for k in ('iou', 'gts_index', 'tap_masks', 'tap_labels', 'good_gt')}
        assert host['iou'].dtype == np.float32 and host['gts_index'].dtype == np.int32 and host['good_gt'].dtype == np.int32
        for name, a in host.items():
            want = np.concatenate([r[name] for r in refs], 0)
            assert a.shape == want.shape == (ro[-1], K), name
            if name == 'iou':
                a, want = a.view(np.uint32), want.view(np.uint32)
            assert np.array_equal(a, want), (name, int((a != want).sum()))
        assert t.n_good.tolist() == [r['n_good'] for r in refs]
        assert t.keep == [v for v, (T, _) in enumerate(videos) if refs[v]['n_good'] > 0 and T > 1]
    for v, r in enumerate(refs):
        want = R.sampled_events(r['good_gt'], cap, seed, draw[v])
        ind, soi, cg = R.lists(want)
        assert ts.n_events[v] == len(want) == min(r['n_good'], cap), v
        assert np.array_equal(ts.ind[v], ind) and np.array_equal(ts.soi[v], soi) and np.array_equal(ts.cg[v], cg), v
        every = R.all_events(r['good_gt'])
        ind, soi, cg = R.lists(every[:cap])
        assert ta.n_events[v] == len(every) == r['n_good'], v          # the uncut count
        assert np.array_equal(ta.ind[v], ind) and np.array_equal(ta.soi[v], soi) and np.array_equal(ta.cg[v], cg), v
    return ts, refs


def test_small_k_valid_region_edges():
    """K = 5 (off a wave): one and two rows (the valid region empty / a single cell), T < K, T = K, T = K + 1; no annotation, one segment,
    two identical segments, a segment that overlaps nothing."""
    K = 5
    videos = [(1, []), (2, [(0, 1)]), (3, [(0, 2)]), (5, [(1, 4), (1, 4)]), (6, [(0, 5), (2, 3)]), (30, []), (23, [(2, 9), (2, 9), (20, 22)])]
    ts, refs = _check(videos, K, cap=64)
    assert refs[0]['tap_masks'].sum() == 0 and refs[1]['tap_masks'].sum() == 1
    assert (refs[5]['gts_index'][refs[5]['tap_masks'] > 0] == -1).all()                       # no annotation: -1
    tie = refs[3]
    assert (tie['gts_index'][tie['tap_masks'] > 0] == 1).all()                                # identical segments: the later index
    last = refs[6]
    zero = (last['iou'] == 0) & (last['tap_masks'] > 0)
    assert zero.any() and (last['gts_index'][zero] == 2).all()                                # overlaps nothing: G_v - 1
    assert 0 not in ts.keep and 5 not in ts.keep


def test_k64_caps_around_n_good():
    """K = 64 (a wave), three videos of 70 / 37 / 129 rows; the cap below, at and above the videos' n_good, and 1 and 1024."""
    videos = [(70, [(0, 12), (10, 40), (10, 40), (33, 69), (50, 51), (2, 66)]), (37, [(3, 20)]), (129, [(0, 128), (5, 9), (5, 9), (100, 101)]),
              (9, [])]
    n = [_oracle(T, 64, st)['n_good'] for T, st in _key(videos)]
    assert n[3] == 0 and 1 < n[2] < n[1] - 1 and n[1] + 1 < n[0] <= 1024
    for cap in (n[1], n[1] - 1, n[1] + 1, n[2], 1, 1024):          # video 1: n_good equal to, above and below the cap; video 3: none
        _check(videos, 64, cap)


def test_k256_more_than_1024_candidates():
    """K = 256, T = 256, four segments: more than 1024 good proposals at cap = 64 (the radix select's ranks) and at cap = 1024."""
    videos = [(256, [(10, 230), (0, 255), (40, 90), (100, 101)])]
    T, st = _key(videos)[0]
    assert _oracle(T, 256, st)['n_good'] > 1024
    _check(videos, 256, 64)
    _check(videos, 256, 1024)


def test_seventeen_videos_and_other_thresholds():
    """V = 17 with row counts that are no multiple of the row tile or of anything else, 0 .. 5 segments each; the reference's defaults and a
    pair of other thresholds (a float32 compare against (float)0.3 / (float)0.65)."""
    rs = np.random.RandomState(17)
    lengths = [3, 41, 7, 1, 19, 33, 2, 9, 27, 5, 13, 38, 11, 6, 29, 17, 23]
    videos = [(T, _stamps(rs, T, int(rs.randint(0, 6))) if T > 1 else []) for T in lengths]
    _check(videos, 12, cap=8)
    _check(videos, 12, cap=8, thr=0.3, good=0.65)


def test_a_video_alone_equals_itself_inside_a_batch():
    """The matrices of a video do not depend on the batch, and with the same draw id neither does its sample; another draw id or seed gives
    another sample."""
    K, cap = 16, 6
    rs = np.random.RandomState(3)
    videos = [(31, _stamps(rs, 31, 3)), (40, [(3, 9), (3, 9), (20, 31), (36, 38)]), (18, _stamps(rs, 18, 2))]
    batch, refs = _check(videos, K, cap, draw=[7, 11, 2])
    assert refs[1]['n_good'] > cap
    alone, _ = _check(videos[1:2], K, cap, draw=[11])
    a, b = int(batch.row_offset[1]), int(batch.row_offset[2])
    for name in ('iou', 'gts_index', 'tap_masks', 'tap_labels', 'good_gt'):
        assert torch.equal(getattr(batch, name)[a:b], getattr(alone, name)), name
    assert np.array_equal(batch.ind[1], alone.ind[0]) and np.array_equal(batch.soi[1], alone.soi[0]) and np.array_equal(batch.cg[1], alone.cg[0])
    other, _ = _check(videos[1:2], K, cap, draw=[12])
    assert not (np.array_equal(other.ind[0], alone.ind[0]) and np.array_equal(other.soi[0], alone.soi[0]))
    other, _ = _check(videos[1:2], K, cap, seed=SEED + 1, draw=[11])
    assert not (np.array_equal(other.ind[0], alone.ind[0]) and np.array_equal(other.soi[0], alone.soi[0]))


def test_two_calls_are_bit_identical():
    from echr_amd import targets as TG
    rs = np.random.RandomState(5)
    videos = _key([(T, _stamps(rs, T, 4)) for T in (45, 70, 12)])
    runs = [TG.build(videos, 32, prop_sample_num=16, seed=SEED) for _ in range(2)]
    for name in ('iou', 'gts_index', 'tap_masks', 'tap_labels', 'good_gt'):
        assert torch.equal(getattr(runs[0], name), getattr(runs[1], name)), name
    assert np.array_equal(runs[0].n_good, runs[1].n_good) and np.array_equal(runs[0].n_events, runs[1].n_events)
    for v in range(3):
        assert np.array_equal(runs[0].ind[v], runs[1].ind[v]) and np.array_equal(runs[0].soi[v], runs[1].soi[v])
        assert np.array_equal(runs[0].cg[v], runs[1].cg[v])


def test_library_refusals_name_their_argument():
    """With device buffers in place the checks still refuse ahead of the launch (the null-pointer forms run in the host suite)."""
    from echr_amd import _lib as L
    lib = L.load()
    dev = torch.device('cuda')
    z = torch.zeros(64, dtype=torch.int32, device=dev)
    f = torch.zeros(64, dtype=torch.float32, device=dev)
    p, q = z.data_ptr(), f.data_ptr()
    assert lib.echr_tap_targets_batch(p, p, p, 1, 4, 2000, 1025, 4, 0.5, 0.8, q, p, q, q, p, p, None) == -22
    assert b'at most 1024' in lib.echr_last_error()
    assert lib.echr_prop_events_batch(p, p, 1, 4, 4, 1025, 1, 0, p, p, p, None) == -22 and b'prop_sample_num' in lib.echr_last_error()
    assert lib.echr_prop_events_batch(p, p, 1, 4, 4, 4, 1, 0, None, p, p, None) == -22 and b'draw' in lib.echr_last_error()


def _models(opt, params, sst_params):
    from echr_amd import models
    from echr_amd.fused import FusedTrainStep, JointBatchStep
    from echr_amd.optim import ClampAdam
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-9, arena=m.build_arena())
    tm = models.setup_tap(opt)
    tm.load_state_dict({k: torch.from_numpy(v) for k, v in sst_params.items()})
    tm = tm.to(torch.device('cuda'))
    tm.train()
    tm.set_dropout_state(U.SEED, U.OFFSET)
    to = ClampAdam(tm.parameters(), lr=1e-9, arena=tm.build_arena())
    return m, tm, JointBatchStep(FusedTrainStep(m, o), tm, to, lambda1=0.01, lambda2=1.0)


def _grads(model):
    ar = model._echr_arena
    return [ar.grad_view(i).detach().cpu().numpy().copy() for i, _ in enumerate(model.named_parameters())]


def test_joint_batch_step_on_built_targets_equals_the_host_built_ones():
    """End to end: one JointBatchStep iteration (train mode, deterministic sums) fed by targets.build -- device matrices, Targets.videos --
    equals the same step fed the oracle's host-built matrices and event lists: loss and both models' gradients bit for bit.  One video has
    no good proposal and is dropped from both."""
    import echr_amd
    from echr_amd import targets as TG
    K, cap, L = 16, 5, 9
    opt = synth.default_opt(CG_vocab_size=300, CG_seq_length=L - 2, K=K)
    params, sst_params = synth.make_params(opt, 0), synth.make_sst_params(opt)
    vids = [synth.make_gt_video(T, G, L, opt.CG_vocab_size + 1, seed=900 + i, max_len=14) for i, (T, G) in enumerate(((34, 3), (21, 0), (40, 4)))]
    draw = [4, 5, 6]
    refs = [R.video_targets(v['T_v'], K, v['featstamps']) for v in vids]
    assert [r['n_good'] > 0 for r in refs] == [True, False, True]
    w1 = [np.random.RandomState(70 + i).uniform(0.05, 0.3, size=K).astype(np.float32) for i in range(3)]
    keys = ('c3d', 'lda')
    host_videos, host_masks, host_labels = [], [], []
    for v in (0, 2):
        ind, soi, cg = R.lists(R.sampled_events(refs[v]['good_gt'], cap, SEED, draw[v]))
        host_videos.append(dict({k: vids[v][k] for k in keys}, ind=ind, soi=soi, labels=vids[v]['gt_labels'][cg], masks=vids[v]['gt_masks'][cg]))
        host_masks.append(torch.from_numpy(refs[v]['tap_masks']))
        host_labels.append(torch.from_numpy(refs[v]['tap_labels']))
    echr_amd.set_deterministic(True)
    try:
        out = []
        for built in (False, True):
            m, tm, js = _models(opt, params, sst_params)
            if built:
                t = TG.build(vids, K, prop_sample_num=cap, seed=SEED, draw=draw)
                assert t.keep == [0, 2]
                videos = t.videos([{k: v[k] for k in keys} for v in vids], [v['gt_labels'] for v in vids], [v['gt_masks'] for v in vids])
                loss = js(videos, t.kept(t.tap_masks), t.kept(t.tap_labels), [w1[v] for v in t.keep], step=False)
            else:
                loss = js(host_videos, host_masks, host_labels, [w1[0], w1[2]], step=False)
            torch.cuda.synchronize()
            out.append((float(loss), float(js.tap_loss), float(js.cg_loss), _grads(m), _grads(tm)))
    finally:
        echr_amd.set_deterministic(False)
    (l0, t0, c0, g0, s0), (l1, t1, c1, g1, s1) = out
    assert np.isfinite(l0) and l0 == l1 and t0 == t1 and c0 == c1
    assert any(g.any() for g in g0) and any(g.any() for g in s0)
    for a, b in zip(g0 + s0, g1 + s1):
        assert np.array_equal(a, b)

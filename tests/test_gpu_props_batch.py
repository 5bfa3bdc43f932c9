"""echr_top_proposals_batch / echr_top_proposals_nms_batch (one workgroup per video, one call for the batch) against the reference's own
per-video outputs (tests/golden/props_batch.npz) and the CPU statement of the layout (tests/props_batch_ref.py).  Every integer output and
`conf` (a single fp32 product, or a copy) is compared bit for bit.

Shapes: lengths (1, 40, 7, 24, 96) with K = 32 -- a one-row video first, T_v < K and T_v > K mixed, 40*32 and 96*32 cells beyond one
1024-element compaction chunk."""
import numpy as np
import pytest
import torch

from tests import props_batch_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

INT_KEYS = ('count', 'event_offset', 'vid', 'ind', 'feat', 'ind_abs', 'feat_abs')


@pytest.fixture(scope='module')
def gold():
    g = U.gold('props_batch.npz')
    g['ro'] = R.offsets(g['lengths'].tolist())
    return g


def run_gpu(scores, ro, topN, thres=0.0, overlap=0.0, mask=None):
    """The batched entry through eval_utils.top_proposals_batch_device: host copies cut to the total, plus the raw device dict."""
    from echr_amd import eval_utils as EU
    sel = EU.top_proposals_batch_device(torch.from_numpy(np.ascontiguousarray(scores)).cuda(), ro, mask, topN, thres, overlap)
    torch.cuda.synchronize()
    n = int(sel['count'][len(ro) - 1])
    out = {k: sel[k].cpu().numpy() for k in ('count', 'event_offset')}
    out.update({k: sel[k][:n].cpu().numpy() for k in ('vid', 'ind', 'feat', 'ind_abs', 'feat_abs', 'conf')})
    return out


def assert_same(got, want):
    for k in INT_KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    assert got['conf'].dtype == np.float32 and np.array_equal(got['conf'].view(np.uint32), want['conf'].view(np.uint32))


@pytest.mark.parametrize('case', [0, 1, 2, 3])
def test_threshold_batch_vs_reference_fixture_and_ref(gold, case):
    """case 0 plain, 1 ties beyond topN (scores quantised to 1/16), 2 val_thres above every score of video 2 (an empty segment in the
    middle of event_offset), 3 topN = 100000; with the explicit causal mask and with NULL (which must equal it)."""
    g, ro = gold, gold['ro']
    scores, topN, thres = g['t%d|scores' % case], int(g['t%d|topN' % case]), float(g['t%d|thres' % case])
    mask = R.causal_mask(g['lengths'].tolist(), int(g['K']))
    want = R.select(scores, ro, topN, thres)
    explicit = run_gpu(scores, ro, topN, thres, mask=mask)
    null = run_gpu(scores, ro, topN, thres)
    for got in (explicit, null):
        assert got['count'][:5].tolist() == g['t%d|count' % case].tolist()
        assert np.array_equal(got['ind'], g['t%d|ind' % case]) and np.array_equal(got['feat'], g['t%d|feat' % case])
        assert np.array_equal(got['conf'], g['t%d|conf' % case])
        assert_same(got, want)
    if case == 1:
        assert explicit['count'][:5].max() > topN
    if case == 2:
        assert explicit['count'][2] == 0 and explicit['event_offset'][2] == explicit['event_offset'][3] < explicit['event_offset'][4]


def test_threshold_batch_with_a_non_causal_mask(gold):
    """An explicit mask that is not the causal one (fractional weights, zeros inside the causal region) against the ref."""
    g, ro = gold, gold['ro']
    rs = np.random.RandomState(5)
    mask = (R.causal_mask(g['lengths'].tolist(), 32) * rs.choice([0.0, 0.5, 1.0], size=g['t0|scores'].shape)).astype(np.float32)
    assert_same(run_gpu(g['t0|scores'], ro, 50, 0.1, mask=mask), R.select(g['t0|scores'], ro, 50, 0.1, mask=mask))


@pytest.mark.parametrize('case', [0, 1, 2, 3])
def test_nms_batch_vs_reference_fixture_and_ref(gold, case):
    """overlap 0.5 / 0.9 x topN 12 / 1000; the one-row video has no candidate: count 0."""
    g, ro = gold, gold['ro']
    ov, topN = float(g['n%d|overlap' % case]), int(g['n%d|topN' % case])
    got = run_gpu(g['n|scores'], ro, topN, overlap=ov)
    assert got['count'][:5].tolist() == g['n%d|count' % case].tolist() and got['count'][0] == 0
    assert np.array_equal(got['feat'], g['n%d|props' % case]) and np.array_equal(got['conf'], g['n%d|conf' % case].astype(np.float32))
    assert_same(got, R.select(g['n|scores'], ro, topN, overlap=ov))


def test_one_video_batch_equals_the_single_video_entries():
    """V = 1: both batched entries against echr_top_proposals / echr_top_proposals_nms on the grids of proposals.npz, bit for bit."""
    from echr_amd import eval_utils as EU
    g = U.gold('proposals.npz')
    f2t = lambda s, e, n, d: 0
    for i in range(3):
        scores, mask, topN = g['g%d|scores' % i], g['g%d|mask' % i], int(g['g%d|topN' % i])
        T = scores.shape[0]
        ind, feat, conf = EU.top_proposals_device(torch.from_numpy(scores).cuda(), mask, topN, 0.0)
        for m in (mask, None):
            got = run_gpu(scores, [0, T], topN, mask=m)
            assert got['count'].tolist() == [len(ind), len(ind), int((feat[:, 1] - feat[:, 0]).max())] and got['event_offset'].tolist() == [0, len(ind)]
            assert np.array_equal(got['ind'], ind.cpu().numpy()) and np.array_equal(got['feat'], feat.cpu().numpy())
            assert np.array_equal(got['conf'].view(np.uint32), conf.cpu().numpy().view(np.uint32))
            assert np.array_equal(got['ind_abs'], got['ind']) and np.array_equal(got['feat_abs'], got['feat']) and not got['vid'].any()
        scores, topN, ov = g['n%d|scores' % i], int(g['n%d|topN' % i]), float(g['n%d|overlap' % i])
        _, props, _, _, conf = EU.gettop1000_nms(torch.from_numpy(scores).cuda(), None, [], 1.0, f2t, overlap=ov, topN=topN)
        got = run_gpu(scores, [0, scores.shape[0]], topN, overlap=ov)
        assert got['count'][:2].tolist() == [len(props), len(props)]
        assert np.array_equal(got['feat'], props) and np.array_equal(got['conf'].astype(np.float64), conf) and np.array_equal(got['ind'], props[:, 1] - 1)


def test_absolute_indices_total_and_largest_length(gold):
    g, ro = gold, gold['ro']
    for got in (run_gpu(g['t1|scores'], ro, 50), run_gpu(g['n|scores'], ro, 1000, overlap=0.9)):
        V = 5
        assert got['count'][V] == got['count'][:V].sum() == len(got['vid']) == got['event_offset'][V]
        assert np.array_equal(got['event_offset'], R.offsets(got['count'][:V]))
        assert np.array_equal(got['vid'], np.repeat(np.arange(V), got['count'][:V]))
        assert np.array_equal(got['ind_abs'], got['ind'] + ro[got['vid']]) and np.array_equal(got['feat_abs'], got['feat'] + ro[got['vid']][:, None])
        assert got['count'][V + 1] == (got['feat'][:, 1] - got['feat'][:, 0]).max()
        lo, hi = ro[got['vid']], ro[got['vid'] + 1]
        assert np.all(got['feat_abs'][:, 0] >= lo) and np.all(got['feat_abs'][:, 1] <= hi) and np.all(got['ind_abs'] < hi)


def test_a_batch_without_any_pick_reports_zero(gold):
    """val_thres above every score: every count, the total and the largest length are 0."""
    got = run_gpu(gold['t0|scores'], gold['ro'], 50, 2.0)
    assert got['count'].tolist() == [0] * 7 and got['event_offset'].tolist() == [0] * 6 and len(got['vid']) == 0

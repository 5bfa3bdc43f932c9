"""GPU (-m gpu): the six self-critical runs of tests/scst_unify_runs.py equal, bit for bit, the record made BEFORE the two step classes
shared one iteration and the two module paths one body (tests/golden/scst_unify.json, tools/make_golden_scst_unify.py; that commit
reproduced the record across two processes).  Deterministic mode, drawn captions: no kernel and no launch order differs, so any
difference is a behaviour change -- no tolerance."""
import functools
import json
import os

import pytest

from tests import scst_unify_runs as S
from tests import util as U

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _record():
    with open(os.path.join(U.GOLD, 'scst_unify.json')) as f:
        return json.load(f)


def test_the_record_covers_every_run_with_drawn_captions_and_live_rewards():
    rec = _record()
    assert sorted(rec) == sorted(S.RUNS)
    for name, r in rec.items():
        assert any(any(row) for row in r['gen']) and any(b != '0' for b in r['reward']) and r['loss'] != '00000000', name
        assert (r.get('applied_steps') == 1 and len(r['params']) == 64) == ('step|' in name), name
        assert (r['video_words'] is not None) == ('batch' in name), name


@pytest.mark.parametrize('name', S.RUNS)
def test_run_is_bitwise_the_recorded_one(name):
    import echr_amd
    echr_amd.set_deterministic(True)
    try:
        got = S.run(name)
    finally:
        echr_amd.set_deterministic(False)
    want = _record()[name]
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], (name, k)


def test_single_video_step_keeps_its_refusals_of_a_pinned_gen_result_with_a_row_too_many():
    """The step takes N from the tensor it was given: a reward with the tensor's rows passes the reward check and FusedTrainStep._setup
    refuses the labels; a reward with the events' rows is refused against the tensor's own shape.  Both as before the shared iteration."""
    import numpy as np
    import torch
    from echr_amd.fused import SelfCriticalStep
    opt, params, vid, _ = S._single()
    m, o, f = S._model(opt, params)
    args = tuple(torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda')) + (vid['ind'], vid['soi'])
    N = len(vid['soi'])
    gen = np.ones((N + 1, 3), np.int64)
    for step in (SelfCriticalStep(f, lambda g, b: np.zeros(len(g), np.float32)), SelfCriticalStep(f)):
        kw = {} if step.reward_fn is not None else dict(reward=np.zeros(N + 1, np.float32))
        with pytest.raises(ValueError, match='^labels have %d rows for %d events$' % (N + 1, N)):
            step(*args, gen_result=gen, step=False, **kw)
    with pytest.raises(ValueError, match=r'^reward must be \[N, T\] or \[N\] \(got \(%d, 3\) for gen_result \(%d, 3\)\)$' % (N, N + 1)):
        SelfCriticalStep(f)(*args, gen_result=gen, reward=np.zeros(N, np.float32), step=False)

"""Inputs and CPU-oracle results of the batched beam tests (tests/test_gpu_beam_batch.py): videos built like given_videos of
tests/test_gpu_eval_batch.py -- every one with its own 'tap' and its own lda, so a wrong per-slot `vid` changes the results -- and the
host beam search of tests/beam_ref.py per video, computed once per (case, <eos> bias, beam size) and shared by the tests (read only)."""
import functools

import numpy as np

from echr_amd import synth
from tests import beam_ref

DURATION = 60.0
# name -> (events per video, seed).  'small': 27 events, at most 135 rows -- the few-rows form of the chain; with +0.25 on the <eos> logit
# bias videos 0, 1, 2 and 5 are empty and videos 3 and 4 mix one 9-word caption with 0-word ones.  'slab': 65 events, 195 / 325 rows at
# B = 3 / 5 -- across SAMP_SLAB_ROWS = 192, the many-rows form.
CASES = {'small': ((3, 4, 12, 3, 4, 1), 1070), 'slab': ((12, 1, 16, 9, 14, 3, 10), 1300)}
# (case, <eos> bias, B) -> events the oracle margin gates at 1e-4, measured with the CPU oracle alone
MIN_GATED = {('small', 0.0, 1): 26, ('small', 0.0, 2): 27, ('small', 0.0, 3): 25, ('small', 0.0, 5): 20,
             ('small', 0.25, 2): 25, ('small', 0.25, 3): 26, ('small', 0.25, 5): 21,
             ('slab', 0.0, 3): 57, ('slab', 0.0, 5): 54}


def make_opt():
    opt, params, _ = synth.make_case('c1')
    opt.K = 8
    return opt, params


def biased(params, eos_bias):
    """`params` with eos_bias added to the <eos> logit bias."""
    if not eos_bias:
        return params
    params = dict(params)
    params['lm_model.logit.bias'] = params['lm_model.logit.bias'].copy()
    params['lm_model.logit.bias'][0] += np.float32(eos_bias)
    return params


@functools.lru_cache(maxsize=None)
def videos(case):
    opt, _ = make_opt()
    counts, seed = CASES[case]
    out = []
    for i, n in enumerate(counts):
        v = synth.make_video(n, 16, 11, opt.CG_vocab_size + 1, seed=seed + i, T_v=20 + 3 * i, min_len=8, video_dim=opt.video_dim,
                             hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
        out.append(dict(c3d=v['c3d'], tap=v['tap'], lda=v['lda'], ind=v['ind'], soi=v['soi'], duration=DURATION,
                        timestamps=[[float(s), float(e)] for s, e in np.asarray(v['soi']).tolist()]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle(case, eos_bias, B):
    """Per video: beam_ref.oracle_beam's dict (seq [N_v, T_v], logp, score, words, margin), float64 scores."""
    opt, params = make_opt()
    params = biased(params, eos_bias)
    return tuple(beam_ref.oracle_beam(opt, params, v, B, v['soi'], v['ind']) for v in videos(case))


def gated(case, eos_bias, B, margin):
    """Per video: the boolean mask of events whose oracle margin reaches `margin`."""
    return [r['margin'] >= margin for r in oracle(case, eos_bias, B)]

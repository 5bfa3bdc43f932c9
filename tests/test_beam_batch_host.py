"""Beam search over a multi-video batch on the host (no GPU): the new entry points exist, their argument checks and refusals, the
arithmetic of VideoBatch.beam_groups, the library symbol, and that forward_batch / caption_videos keep their own refusals."""
import os
import re

import numpy as np
import pytest
import torch

from echr_amd import eval_utils as EU, functional as EF, synth
from echr_amd._lib import EchrHipError
from echr_amd.batch import VideoBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(**over):
    import echr_amd
    opt, params, vids = synth.make_vbatch('vbctx')
    for k, v in over.items():
        setattr(opt, k, v)
    return echr_amd.CaptionGenerator(opt).eval(), VideoBatch.from_videos(vids)


def test_entry_points_exist():
    import echr_amd
    assert callable(echr_amd.CaptionGenerator.beam_batch) and callable(EU.caption_videos_beam) and callable(EF.beam_search_batch)
    assert callable(VideoBatch.beam_groups)
    names = EU.caption_videos_beam.__code__.co_varnames[:EU.caption_videos_beam.__code__.co_argcount]
    assert names[:5] == ('tap_model', 'cg_model', 'videos', 'featstamp_to_time', 'beam_size') and 'max_rows' in names
    for k in ('vocab', 'topN', 'nms_threshold', 'val_score_thres', 'flag_eval_what', 'event_group_rows'):          # caption_videos' other arguments
        assert k in names
    # the greedy entry keeps its shape: no beam argument or variable of that name
    assert 'beam_size' not in EU.caption_videos.__code__.co_varnames


def test_symbol_is_declared_exported_and_prototyped():
    from echr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'echr_hip.h')).read()
    assert re.search(r'int echr_decoder_beam_batch\(const echr_beam_args\* \w+, const echr_batch_ext\* \w+, int32_t\* video_words, void\* stream\);', hdr)
    fn = _lib.load().echr_decoder_beam_batch
    assert len(fn.argtypes) == 4 and fn.restype is _lib.i32


def test_beam_batch_on_cpu_tensors_raises():
    m, b = _model()
    with pytest.raises(EchrHipError):
        m.beam_batch(b, 3)
    with pytest.raises(EchrHipError):
        m.beam_batch(b, 1, event_group_rows=4, max_rows=None)


def test_beam_batch_bad_beam_size_and_mode():
    m, b = _model()
    for bad in (0, -1, EF.BEAM_MAX + 1):
        with pytest.raises(ValueError):
            m.beam_batch(b, bad)
    m.train()
    with pytest.raises(ValueError):
        m.beam_batch(b, 3)          # beam search is an evaluation decode (OldModel.sample refuses it in training mode too)
    m.eval()
    with pytest.raises(ValueError):
        m.beam_batch(b, 3, max_rows=0)
    with pytest.raises(ValueError):
        m.beam_batch(b, 3, event_group_rows=0)


def test_beam_batch_option_refusals():
    for over in (dict(CG_init_feats_type='V'), dict(CG_init_feats_type='VEC'), dict(clip_context_type='CH'), dict(clip_context_type='CC+CH')):
        m, b = _model(**over)
        with pytest.raises(NotImplementedError):
            m.beam_batch(b, 3)


def test_forward_batch_still_refuses_beams_and_names_beam_batch():
    m, b = _model()
    with pytest.raises(NotImplementedError, match='beam_batch'):
        m.forward_batch(b, mode='eval', beam_size=3)


def test_beam_groups_arithmetic():
    counts = (3, 4, 12, 3, 4, 1)
    eo = np.concatenate([[0], np.cumsum(counts)])
    T = 4
    b = VideoBatch(torch.zeros(T * len(counts), 2), torch.zeros(T * len(counts), 2), torch.zeros(len(counts), 2), np.arange(len(counts) + 1) * T, eo,
                   np.concatenate([np.tile([[v * T, v * T + 2]], (n, 1)) for v, n in enumerate(counts)]),
                   np.concatenate([np.full(n, v * T + 1) for v, n in enumerate(counts)]))
    whole = [(0, 6, 0, 27)]
    assert b.beam_groups(3, None) == whole and b.beam_groups(3, 81) == whole and b.beam_groups(1, 27) == whole
    # 40 rows at B = 3 hold 13 events: [0,2) has 7; the 12-event video (36 rows) fits alone but not with a neighbour; [3,6) has 8
    assert b.beam_groups(3, 40) == [(0, 2, 0, 7), (2, 3, 7, 19), (3, 6, 19, 27)]
    # 80 rows: 26 events -- everything but the last video
    assert b.beam_groups(3, 80) == [(0, 5, 0, 26), (5, 6, 26, 27)]
    # a video above the budget runs alone; below one event's rows every video does
    alone = [(v, v + 1, int(eo[v]), int(eo[v + 1])) for v in range(6)]
    assert b.beam_groups(3, 1) == alone and b.beam_groups(5, 4) == alone
    assert b.beam_groups(5, 35) == [(0, 2, 0, 7), (2, 3, 7, 19), (3, 5, 19, 26), (5, 6, 26, 27)]          # 7 events per run
    for runs in (b.beam_groups(2, 17), b.beam_groups(16, 100)):
        assert [r[0] for r in runs] == [0] + [r[1] for r in runs[:-1]] and runs[-1][1] == 6
        assert all(r[2] == eo[r[0]] and r[3] == eo[r[1]] for r in runs)
    for bad in (0, -3):
        with pytest.raises(ValueError):
            b.beam_groups(3, bad)
        with pytest.raises(ValueError):
            b.beam_groups(bad, 10)


def test_beam_search_batch_argument_checks():
    V1, E, H, Ha, N, V, De, D, Dv = 7, 4, 4, 4, 5, 2, 6, 4, 3
    z = torch.zeros
    params = [z(V1, E), z(V1, 3 * H), z(V1), z(4 * H, E + De), z(4 * H, E + D), z(4 * H, E + Dv)] + [z(4 * H, H)] * 3 + [z(4 * H)] * 6 + \
             [z(Ha, D), z(Ha), z(Ha, H), z(Ha), z(1, Ha), z(1)]
    video, event, c3d = z(V, Dv), z(N, De), z(9, D)
    ev_start, ev_len = torch.zeros(N, dtype=torch.int32), torch.ones(N, dtype=torch.int32)
    vid = torch.tensor([0, 0, 1, 1, 1], dtype=torch.int32)
    for bad in (0, V1 + 1, EF.BEAM_MAX + 1):
        with pytest.raises(ValueError, match='beam_size'):
            EF.beam_search_batch(video, event, c3d, ev_start, ev_len, vid, 1, 5, params, bad)
    with pytest.raises(ValueError, match='video'):
        EF.beam_search_batch(video[0], event, c3d, ev_start, ev_len, vid, 1, 5, params, 2)
    with pytest.raises(ValueError, match='one entry per event'):
        EF.beam_search_batch(video, event, c3d, ev_start, ev_len, vid[:-1], 1, 5, params, 2)
    with pytest.raises(ValueError, match='one entry per event'):
        EF.beam_search_batch(video, event, c3d, ev_start[:-1], ev_len, vid, 1, 5, params, 2)
    with pytest.raises(ValueError, match='between 1 video'):
        EF.beam_search_batch(z(N + 1, Dv), event, c3d, ev_start, ev_len, vid, 1, 5, params, 2)
    with pytest.raises(EchrHipError):          # valid arguments on the CPU: the library has no CPU path
        EF.beam_search_batch(video, event, c3d, ev_start, ev_len, vid, 1, 5, params, 2)


def test_caption_videos_beam_checks():
    import echr_amd
    from echr_amd import models as EM
    opt, params, _ = synth.make_case('c1')
    opt.K = 8
    cg, tap = echr_amd.CaptionGenerator(opt), EM.setup_tap(opt)
    f2t = lambda s, e, n, d: [s, e]
    vids = [dict(c3d=torch.zeros(6, opt.video_dim), lda=torch.zeros(opt.lda_dim), duration=1.0)]
    with pytest.raises(EchrHipError):
        EU.caption_videos_beam(tap, cg, vids, f2t, 3)
    for bad in (0, EF.BEAM_MAX + 1):
        with pytest.raises(ValueError, match='beam_size'):
            EU.caption_videos_beam(tap, cg, vids, f2t, bad)
    with pytest.raises(ValueError):
        EU.caption_videos_beam(tap, cg, vids, f2t, 3, flag_eval_what='gt_tap_cg')
    with pytest.raises(ValueError):
        EU.caption_videos_beam(tap, cg, [], f2t, 3)

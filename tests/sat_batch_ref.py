"""CPU reference of the one-stream decoder over a multi-video batch -- TEST INFRASTRUCTURE: tests/sat_ref.py run ONCE PER VIDEO, then
composed under the rules of echr_amd/batch.py (as tests/vbatch_ref.py composes the three-stream oracle):

  * log-probs: per video [N_v, S_v, V1] -- the batched output's rows of video v, cut to the video's own step count;
  * loss = the sum over the videos of LanguageModelCriterion (each with its own normaliser, no 1/V), and the per-video losses;
  * gradients = the sum over the videos (the reference's m_batch accumulation, train.py:281-283,313-317); d tap per video;
  * training mode: video v gets the rows [e0:e1] of the batch's [N_tot, H] output masks and [e0:e1, :, e0:e1] of the event encoder's
    [N_tot, G, N_tot] mask, drawn with echr_amd/philox.py for the batch-global shapes: the device keys a site by the batch-global element.

Also the named multi-video cases of tests/test_sat_batch_host.py / test_gpu_sat_batch.py (CASES, make_case): TINY widths unless said.
tools/make_golden_sat_batch.py checks `run` and `sample` against the reference's own modules."""
import numpy as np
import torch

from echr_amd import synth
from oracle import echr_ref_cpu as O
from tests import sat_ref as R
from tests import util as U

TINY = dict(video_dim=20, hidden_dim=24, lda_dim=12, d_feats=32, d_o=32, n_head=4, CG_rnn_size=32, CG_input_encoding_size=16,
            CG_att_hid_size=24, CG_vocab_size=30, CG_seq_length=5)
SMALL_VOCAB = dict(CG_vocab_size=60, CG_seq_length=4)          # the ECHR widths (H = 512, D = 500, lda 100) with a vocabulary a test can hold
_SAT = dict(caption_model='show_attend_tell', CG_num_layers=1)

# videos: (events, widest event A, feature rows T_v, label width L) per video; `one`: (video, event) cut to ONE row; seeds: video v = seed + v
CASES = {
    # the reference's fixture (tests/golden/case_sat_batch.npz): three ragged videos
    'fixture': dict(opt=TINY, videos=((2, 7, 10, 7), (3, 6, 12, 6), (1, 5, 9, 7)), seed=503),
    # (1, 3, 2) events on (9, 14, 11) rows, A = 7; one event one row long; the last video's captions hold 2 words: 3 steps against 6
    'edge3': dict(opt=TINY, videos=((1, 7, 9, 7), (3, 6, 14, 7), (2, 5, 11, 4)), one=(1, 1), seed=520),
    # 65 rows: a video boundary inside a 64-row tile (52 | 13 rows: row 64 is the tile boundary inside video 4)
    'tile65': dict(opt=TINY, videos=((13, 6, 16, 5),) * 5, seed=540),
    'widths': dict(opt=SMALL_VOCAB, videos=((2, 9, 12, 5), (1, 6, 10, 5)), seed=560),
    # greedy decodes that end at different steps across the videos: widths (3, 5, 5) (eos: the <eos> logit's bias and the scale of its
    # weight row, so that it follows the state closely enough to win at some step)
    'eos': dict(opt=TINY, videos=((2, 7, 10, 7), (3, 6, 12, 6), (2, 5, 9, 7)), seed=601, eos=(-0.15, 4.0)),
}


def make_case(name, feats='VEC', **over):
    """(opt, params, [video dicts]) of a named case with CG_input_feats_type `feats`; `over`: further option overrides."""
    c = CASES[name]
    opt = synth.default_opt(**dict(dict(_SAT, **c['opt']), CG_input_feats_type=feats, **over))
    videos = []
    for v, (n, a, t, l) in enumerate(c['videos']):
        vd = synth.make_video(n, a, l, opt.CG_vocab_size + 1, seed=c['seed'] + v, T_v=t, min_len=2, video_dim=opt.video_dim,
                              hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim)
        if c.get('one', (None,))[0] == v:
            e = c['one'][1]
            vd['soi'][e, 1] = vd['soi'][e, 0] + 1
            vd['ind'][e] = vd['soi'][e, 0]
        videos.append(vd)
    params = synth.make_sat_params(opt, 0)
    if 'eos' in c:
        b, w = params['lm_model.logit.bias'].copy(), params['lm_model.logit.weight'].copy()
        b[0], w[0] = c['eos'][0], w[0] * np.float32(c['eos'][1])
        params['lm_model.logit.bias'], params['lm_model.logit.weight'] = b, w
    return opt, params, videos


def offsets(videos):
    eo = [0]
    for v in videos:
        eo.append(eo[-1] + len(v['soi']))
    return eo


def sliced_drop(opt, n_tot, e0, e1):
    """sat_ref's `drop` callable for the events [e0, e1) of a batch of n_tot events: slices of the batch-global masks."""
    base = U.oracle_drop(opt)

    def drop(site, step, shape):
        if site == 'tsrm':
            return base(site, step, (n_tot, shape[1], n_tot))[e0:e1, :, e0:e1].contiguous()
        return base(site, step, (n_tot, shape[1]))[e0:e1].contiguous()
    return drop


def run(opt, params, videos, train_mode, dtype=torch.float32, backward=True):
    """dict(logp=[per video [N_v,S_v,V1]], loss=sum, losses=[V], grads={name: summed gradient or None}, g_tap=[per video [T_v,Ht]])."""
    P = {k: torch.from_numpy(np.ascontiguousarray(v).copy()).to(dtype).requires_grad_(backward) for k, v in params.items()}
    eo = offsets(videos)
    logps, losses, g_taps = [], [], []
    for v, vid in enumerate(videos):
        tap = torch.from_numpy(np.ascontiguousarray(vid['tap']).copy()).to(dtype).requires_grad_(backward)
        c3d, lda = (torch.from_numpy(np.ascontiguousarray(vid[k])).to(dtype) for k in ('c3d', 'lda'))
        labels = torch.from_numpy(np.ascontiguousarray(vid['labels']))
        masks = torch.from_numpy(np.ascontiguousarray(vid['masks'])).to(dtype)
        drop = sliced_drop(opt, eo[-1], eo[v], eo[v + 1]) if train_mode else None
        video, event, clip, mask = R.contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi'], drop)
        logp = R.decoder_forward(P, video, event, clip, mask, labels, opt.CG_input_feats_type, drop, opt.CG_init_feats_type)
        loss = O.lm_criterion(logp, labels[:, 1:], masks[:, 1:])
        if backward:
            loss.backward()          # accumulates into P[k].grad: the sum over the videos
            g_taps.append(tap.grad.numpy().copy() if tap.grad is not None else np.zeros(tuple(tap.shape), tap.detach().numpy().dtype))
        logps.append(logp.detach().numpy())
        losses.append(float(loss.detach()))
    grads = {k: (p.grad.numpy().copy() if p.grad is not None else None) for k, p in P.items()} if backward else None
    return dict(logp=logps, loss=float(np.sum(np.asarray(losses, np.float64))), losses=np.asarray(losses), grads=grads, g_tap=g_taps)


def sample(opt, params, videos, dtype=torch.float32):
    """Greedy decode per video (eval mode): [(seq int64 [N_v,T_v], logp, margin [N_v,T_v])]; ([], [], []) for a video that generates
    nothing.  margin[:, t]: the top-1 / top-2 gap of the step that chose seq[:, t]."""
    out = []
    for vid in videos:
        margins = []
        seq, slp = R.sample(opt, params, vid, dtype, margins)
        if isinstance(seq, list):
            out.append(([], [], []))
            continue
        out.append((seq.numpy(), slp.numpy(), np.stack(margins[:seq.shape[1]], 1)))
    return out


def stack_sample(per_video, videos):
    """The batched decode from the per-video ones: (seq int64 [N_tot, T], margin [N_tot, T], widths [V]) with T the longest video's
    width; behind its own width a video's rows are finished: zeros (OldModel.sample pads finished rows, OldModel_NEW.py:171-183), margin
    inf there (a zero needs no resolving)."""
    eo = offsets(videos)
    widths = [0 if isinstance(s, list) else int(s.shape[1]) for s, _, _ in per_video]
    T = max(widths)
    seq = np.zeros((eo[-1], T), np.int64)
    margin = np.full((eo[-1], T), np.inf)
    for v, (s, _, m) in enumerate(per_video):
        if widths[v]:
            seq[eo[v]:eo[v + 1], :widths[v]] = s
            margin[eo[v]:eo[v + 1], :widths[v]] = m
    return seq, margin, np.asarray(widths)


def resolvable(per_video, min_margin=1e-4):
    """Per video the positions a float32 decode must reproduce, bool [N_v, T_v]: position t of a row counts while the margins of its
    decisions 0 .. t all exceed min_margin (a row that takes the other branch of an unresolvable decision decodes another caption from
    there on)."""
    out = []
    for s, _, m in per_video:
        if isinstance(s, list):
            out.append(np.zeros((0, 0), bool))
            continue
        out.append(np.logical_and.accumulate(np.asarray(m) > min_margin, axis=1))
    return out

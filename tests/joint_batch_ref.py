"""CPU reference of the joint 'tap_cg' iteration over a multi-video batch (fused.JointBatchStep): oracle/echr_ref_cpu.py run ONCE PER VIDEO,

    sst_forward(c3d_v) -> caption_forward on that tap -> lambda1 * tap_criterion + lambda2 * lm_criterion -> backward()

accumulating into shared parameter dicts of both models (the reference's m_batch accumulation, train.py:281-283,313-329): the losses are
reported per video and unscaled, the gradients are the sums over the videos, there is no 1/V.  Training mode: video v is fed rows
[row_offset[v], row_offset[v+1]) of the batch's inter-layer SST mask (as tests/sst_batch_ref.py does) and vbatch_ref.sliced_drop for the
caption sites -- one dropout counter per model and call, keyed by the batch-global element.
"""
import numpy as np
import torch

from echr_amd import philox, synth
from oracle import echr_ref_cpu as O
from tests import util as U
from tests import vbatch_ref as VR

K = 16
LAMBDA1 = 0.01          # opts.py:194-196; the caption side then supplies > 99 % of the SST gradients' max-norm: they test the d tap hand-over


def row_offsets(vids):
    ro = [0]
    for v in vids:
        ro.append(ro[-1] + min(len(v['c3d']), len(v['tap'])))
    return ro


def tap_inputs(vids, K=K, seed=5):
    """Per video: (masks [T_v, K], labels [T_v, K], w1 [K]) of the proposal criterion, shaped as synth.make_c5 shapes them (w1 per video)."""
    rs = np.random.RandomState(seed)
    out = []
    for a, b in zip(row_offsets(vids)[:-1], row_offsets(vids)[1:]):
        T = b - a
        lab = (rs.uniform(size=(T, K)) > 0.9).astype(np.float32)
        mk = (np.arange(T)[:, None] >= np.arange(K)[None, :]).astype(np.float32)
        out.append((mk, lab, rs.uniform(0.05, 0.3, size=(K,)).astype(np.float32)))
    return out


def setup(case='vbctx', K=K):
    """(opt, caption params, SST params, videos, proposal-criterion inputs) of a named multi-video case."""
    opt, params, vids = synth.make_vbatch(case)
    opt.K = K
    return opt, params, synth.make_sst_params(opt), vids, tap_inputs(vids, K)


def setup_wide(V=9, events=8, K=K, seed=1400):
    """V videos of `events` events, T_v in 30..40 rows, small vocabulary: more than 64 events with V = 9 (launch-per-phase recurrences) and
    more videos than one persistent proposal-encoder launch carries."""
    opt = synth.default_opt(CG_vocab_size=300, CG_seq_length=7, K=K)
    vids = synth.make_vbatch_videos(V, (events, events), (3, 24), (30, 40), (6, 9), opt.CG_vocab_size + 1, seed, V * events, None,
                                    opt.video_dim, opt.hidden_dim, opt.lda_dim)
    return opt, synth.make_params(opt, 0), synth.make_sst_params(opt), vids, tap_inputs(vids, K)


def run(opt, params, sst_params, vids, tap_in, train_mode, lambda1=LAMBDA1, lambda2=1.0, dtype=torch.float32):
    """dict(tap_losses [V], cg_losses [V], grads {caption parameter: summed gradient or None}, sst_grads {SST parameter: summed gradient},
    row_offset, event_offset)."""
    P = {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_(True) for k, v in params.items()}
    S = {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_(True) for k, v in sst_params.items()}
    eo, ro = VR.offsets(vids), row_offsets(vids)
    H = opt.hidden_dim
    mask = None
    if train_mode and opt.rnn_dropout > 0:
        mask = torch.from_numpy(philox.scale_mask((ro[-1], H), opt.rnn_dropout, U.SEED, U.OFFSET, philox.SITE_SST, 0)).to(dtype)
    tl, cl = [], []
    for v, vid in enumerate(vids):
        T = ro[v + 1] - ro[v]
        c3d = torch.from_numpy(np.ascontiguousarray(vid['c3d'][:T])).to(dtype)
        tap, sc = O.sst_forward(S, c3d, mask[ro[v]:ro[v + 1]].contiguous() if mask is not None else None)
        mk, lab, w1 = (torch.from_numpy(x).to(dtype) for x in tap_in[v])
        tloss = O.tap_criterion(sc, mk, lab, w1)
        drop = VR.sliced_drop(opt, eo[-1], eo[v], eo[v + 1]) if train_mode else None
        if drop is not None and dtype != torch.float32:
            drop = (lambda d0: (lambda *a: d0(*a).to(dtype)))(drop)
        labels = torch.from_numpy(np.ascontiguousarray(vid['labels']))
        masks = torch.from_numpy(np.ascontiguousarray(vid['masks'])).to(dtype)
        logp = O.caption_forward(P, tap, c3d, torch.from_numpy(vid['lda']).to(dtype), labels, vid['ind'], vid['soi'], 'train', drop, opt.n_head,
                                 video_context_type=opt.video_context_type, event_context_type=opt.event_context_type,
                                 fST_type=getattr(opt, 'fST_type', 'fST0'), use_posit=opt.use_posit)
        closs = O.lm_criterion(logp, labels[:, 1:], masks[:, 1:])
        (lambda1 * tloss + lambda2 * closs).backward()          # .grad accumulates: the sum over the videos
        tl.append(float(tloss.detach()))
        cl.append(float(closs.detach()))
    return dict(tap_losses=np.asarray(tl), cg_losses=np.asarray(cl),
                grads={k: (p.grad.numpy().copy() if p.grad is not None else None) for k, p in P.items()},
                sst_grads={k: p.grad.numpy().copy() for k, p in S.items()}, row_offset=ro, event_offset=eo)

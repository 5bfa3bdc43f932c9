"""CPU reference of the batched proposal encoder (models.SST.forward_batch): oracle/echr_ref_cpu.sst_forward run ONCE PER VIDEO (every video
from the zero state), then

  * outputs: the videos' tap_feats / scores rows concatenated in batch order;
  * gradients: the sum over the videos (the reference's m_batch accumulation, train.py:281-283,313-317);
  * training mode: video v is fed rows [row_offset[v], row_offset[v+1]) of the batch's inter-layer dropout mask
    philox.scale_mask((T_tot, H), p, seed, offset, SITE_SST, 0) -- one counter per call, keyed by the batch-global element.
"""
import numpy as np
import torch

from oracle import echr_ref_cpu as O
from tests import util as U

NAMES = ('rnn.weight_ih_l0', 'rnn.weight_hh_l0', 'rnn.bias_ih_l0', 'rnn.bias_hh_l0', 'rnn.weight_ih_l1', 'rnn.weight_hh_l1', 'rnn.bias_ih_l1',
         'rnn.bias_hh_l1', 'scores.weight', 'scores.bias')


def make_params(rs, D, H, K):
    shapes = {'rnn.weight_ih_l0': (4 * H, D), 'rnn.weight_hh_l0': (4 * H, H), 'rnn.bias_ih_l0': (4 * H,), 'rnn.bias_hh_l0': (4 * H,),
              'rnn.weight_ih_l1': (4 * H, H), 'rnn.weight_hh_l1': (4 * H, H), 'rnn.bias_ih_l1': (4 * H,), 'rnn.bias_hh_l1': (4 * H,),
              'scores.weight': (K, H), 'scores.bias': (K,)}
    return {k: (rs.uniform(-1, 1, size=s) / np.sqrt(H)).astype(np.float32) for k, s in shapes.items()}


def offsets(lengths):
    ro = [0]
    for t in lengths:
        ro.append(ro[-1] + int(t))
    return ro


def make_inputs(rs, lengths, D, H, K):
    """(x [T_tot, D], upstream weights on tap [T_tot, H] and on scores [T_tot, K], row offsets)."""
    ro = offsets(lengths)
    T = ro[-1]
    return (rs.standard_normal((T, D)).astype(np.float32), rs.standard_normal((T, H)).astype(np.float32),
            rs.standard_normal((T, K)).astype(np.float32), ro)


def module(params, D, H, K, train, p=0.5):
    """models.setup_tap on the GPU with `params` loaded, its dropout stream at (U.SEED, U.OFFSET)."""
    from echr_amd import models, synth
    m = models.setup_tap(synth.default_opt(video_dim=D, hidden_dim=H, K=K, rnn_dropout=p))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.cuda()
    m.train() if train else m.eval()
    m.set_dropout_state(U.SEED, U.OFFSET)
    return m


def run(params, x, wt, ws, ro, train, p=0.5, dtype=None, loss=None):
    """The oracle once per video: dict(tap [T_tot, H], scores [T_tot, K], grads {name: summed gradient}, loss = the videos' sum).
    dtype=torch.float64: the same float32 inputs (and the same dropout mask) carried through the oracle in double precision.
    loss(v, a, b, tap, scores) -> video v's scalar (rows a..b of the batch), or (scalar to differentiate, scalar to report); None: the weighted
    sums (tap * wt).sum() + (scores * ws).sum()."""
    from echr_amd import philox
    cast = (lambda t: t) if dtype is None else (lambda t: t.to(dtype))
    H = params['rnn.weight_hh_l0'].shape[1]
    T = ro[-1]
    mask = torch.from_numpy(philox.scale_mask((T, H), p, U.SEED, U.OFFSET, philox.SITE_SST, 0)) if train else None
    P = {k: cast(torch.from_numpy(v.copy())).requires_grad_(True) for k, v in params.items()}
    taps, scs, total = [], [], 0.0
    for v, (a, b) in enumerate(zip(ro[:-1], ro[1:])):
        tap, sc = O.sst_forward(P, cast(torch.from_numpy(x[a:b])), cast(mask[a:b].contiguous()) if mask is not None else None)
        if loss is None:
            l = (tap * cast(torch.from_numpy(wt[a:b]))).sum() + (sc * cast(torch.from_numpy(ws[a:b]))).sum()
        else:
            l = loss(v, a, b, tap, sc)
        l, rep = l if isinstance(l, tuple) else (l, l)
        l.backward()          # .grad accumulates: the sum
        total += float(rep.detach())
        taps.append(tap.detach().numpy())
        scs.append(sc.detach().numpy())
    return dict(tap=np.concatenate(taps, 0), scores=np.concatenate(scs, 0), grads={k: P[k].grad.numpy() for k in NAMES}, loss=total)


def gpu_pass(m, x, wt, ws, ro):
    """forward_batch + backward of the same weighted sums on the GPU: dict(tap, scores, grads)."""
    dev = torch.device('cuda')
    for p in m.parameters():
        p.grad = None
    tap, sc = m.forward_batch(torch.from_numpy(x).to(dev), ro)
    ((tap * torch.from_numpy(wt).to(dev)).sum() + (sc * torch.from_numpy(ws).to(dev)).sum()).backward()
    torch.cuda.synchronize()
    return dict(tap=tap.detach().cpu().numpy(), scores=sc.detach().cpu().numpy(), grads={k: p.grad.cpu().numpy() for k, p in m.named_parameters()})

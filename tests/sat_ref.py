"""CPU reference of the one-stream attention decoder (`caption_model='show_attend_tell'`, one LSTM layer; reference
models/OldModel_NEW.py:98-187 over :190-274) -- TEST INFRASTRUCTURE, written from the arithmetic, in torch:

    q = h2att(h(t-1))                         the UNDROPPED top-layer state
    w = softmax(alpha_net(tanh(ctx2att(clip) + q))) over all A padded slots, x mask, renormalised
    att = sum_a w_a clip_a
    x = [embed(it) | video if 'V' | event if 'E' | att if 'C']
    gates = x . W_ih^T + h(t-1) . W_hh^T       no bias, order i, f, g, o;  c = f c + i g;  h = o tanh(c)
    logp = log_softmax(logit(dropout(h)))      the one dropout site ('out', [N, H])

The state handed on is (h, c), each [1, N, H], undropped.  Contexts, criterion, the event encoder and init_linear are the pieces of
oracle/echr_ref_cpu.py (video_context, clip_context, event_pool, event_context, lm_criterion); tools/make_golden_sat.py checks this file
against the reference's own modules, tests/test_sat_host.py against the fixtures it wrote.  Every function takes the dtype its tensors
arrive in (float32 / float64)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import echr_ref_cpu as O
from tests import util as U

PRE = 'lm_model.'
# d loss / d alpha_net.bias is exactly zero in real arithmetic (the slot softmax is shift invariant): every side holds rounding noise
# (tests/util.NOISE_ONLY names the three-stream decoder's)
NOISE_ONLY = (PRE + 'core.alpha_net.bias',)
PROBE = None          # a list here receives what core_step saw


def attention(P, h, clip, mask):
    N, A, D = clip.shape
    p = F.linear(clip.reshape(N * A, D), P[PRE + 'core.ctx2att.weight'], P[PRE + 'core.ctx2att.bias']).view(N, A, -1)
    q = F.linear(h, P[PRE + 'core.h2att.weight'], P[PRE + 'core.h2att.bias'])
    e = F.linear(torch.tanh(p + q.unsqueeze(1)).view(N * A, -1), P[PRE + 'core.alpha_net.weight'], P[PRE + 'core.alpha_net.bias']).view(N, A)
    w = torch.softmax(e, 1) * mask
    w = w / w.sum(1, keepdim=True)
    return torch.bmm(w.unsqueeze(1), clip).squeeze(1)


def core_step(P, xt, video, event, clip, mask, state, feats_type):
    """ShowAttendTellCore.forward: (h [N,H], (h [1,N,H], c [1,N,H]))."""
    h, c = state[0][-1], state[1][-1]
    N = xt.shape[0]
    parts = [xt]
    if 'V' in feats_type:
        parts.append(video.reshape(1, -1).expand(N, video.numel()))
    if 'E' in feats_type:
        parts.append(event)
    if 'C' in feats_type:
        parts.append(attention(P, h, clip, mask))
    assert len(parts) > 1, 'CG_input_feats_type selects nothing: the reference fails there (torch.cat of an empty list)'
    g = F.linear(torch.cat(parts, 1), P[PRE + 'core.rnn.weight_ih_l0']) + F.linear(h, P[PRE + 'core.rnn.weight_hh_l0'])
    i, f, gg, o = g.chunk(4, 1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    if PROBE is not None:          # (tests/sat_regime_ref.probe: the gate pre-activations [N, 4H] and the new cell state [N, H] of every step)
        PROBE.append((g.detach().numpy().copy(), c2.detach().numpy().copy()))
    h2 = torch.sigmoid(o) * torch.tanh(c2)
    return h2, (h2.unsqueeze(0), c2.unsqueeze(0))


def logprobs_state(P, it, video, event, clip, mask, state, feats_type, dm_out=None):
    """OldModel.get_logprobs_state."""
    out, state = core_step(P, F.embedding(it, P[PRE + 'embed.weight']), video, event, clip, mask, state, feats_type)
    if dm_out is not None:
        out = out * dm_out
    return torch.log_softmax(F.linear(out, P[PRE + 'logit.weight'], P[PRE + 'logit.bias']), 1), state


def init_hidden(P, video, event, clip, init_feats_type=''):
    """OldModel.init_hidden with num_layers = 1: zeros, or h(-1) = c(-1) = init_linear(cat([video | event | clip.mean(1)])) as [1,N,H]."""
    N, H = event.shape[0], P[PRE + 'core.rnn.weight_hh_l0'].shape[1]
    if not any(k in init_feats_type for k in 'VEC'):
        return (event.new_zeros(1, N, H), event.new_zeros(1, N, H))
    feats = []
    if 'V' in init_feats_type:
        feats.append(video.reshape(1, -1).expand(N, video.numel()))
    if 'E' in init_feats_type:
        feats.append(event)
    if 'C' in init_feats_type:
        feats.append(clip.mean(1))
    m = F.linear(torch.cat(feats, 1), P[PRE + 'init_linear.weight'], P[PRE + 'init_linear.bias']).view(N, 1, H).transpose(0, 1)
    return (m, m)


def decoder_forward(P, video, event, clip, mask, seq, feats_type, drop=None, init_feats_type='', states=None):
    """OldModel.forward, teacher forcing with its early break.  drop: None or the callable of tests/util.oracle_drop (site 'out' only).
    `states`: a list that receives every step's (h, c)."""
    N, H = event.shape[0], P[PRE + 'core.rnn.weight_hh_l0'].shape[1]
    state = init_hidden(P, video, event, clip, init_feats_type)
    outs = []
    for i in range(seq.shape[1] - 1):
        if i >= 1 and int(seq[:, i].sum()) == 0:
            break
        dm = drop('out', i, (N, H)).to(event.dtype) if drop is not None else None
        lp, state = logprobs_state(P, seq[:, i], video, event, clip, mask, state, feats_type, dm)
        outs.append(lp)
        if states is not None:
            states.append(state)
    return torch.stack(outs, 1)


def decoder_sample(P, video, event, clip, mask, seq_length, feats_type, init_feats_type='', margins=None):
    """The greedy branch of OldModel.sample with its trimming: (seq int64 [N,T], logp [N,T]) or ([], []).  `margins`: a list that receives
    per decision step the top-1 / top-2 margin of every row [N]."""
    N = event.shape[0]
    state = init_hidden(P, video, event, clip, init_feats_type)
    seq, slp, logprobs, unfinished = [], [], None, None
    for t in range(seq_length + 1):
        if t == 0:
            it = torch.zeros(N, dtype=torch.long)
        else:
            sample_lp, it = torch.max(logprobs, 1)
            if margins is not None:
                top = torch.topk(logprobs, 2, 1).values
                margins.append((top[:, 0] - top[:, 1]).detach().numpy().copy())
        logprobs, state = logprobs_state(P, it, video, event, clip, mask, state, feats_type)
        if t >= 1:
            unfinished = (it > 0) if t == 1 else unfinished & (it > 0)
            if int(unfinished.sum()) == 0:
                break
            seq.append(it * unfinished.type_as(it))
            slp.append(sample_lp)
    if not seq:
        return [], []
    return torch.stack(seq, 1), torch.stack(slp, 1)


def contexts(opt, P, tap, c3d, lda, ind, soi, drop=None):
    """(video, event, clip, mask) as CaptionGenerator.forward builds them ('CC' rows; 'ER*' through the event encoder, 'EC' / 'EH' direct)."""
    video = O.video_context(lda, c3d, tap, opt.video_context_type)
    et = opt.event_context_type
    if et == 'EC':
        event = O.event_pool(c3d, soi)
    elif et == 'EH':
        event = tap[torch.as_tensor(np.asarray(ind), dtype=torch.long)]
    else:
        N = len(soi)
        dmask = drop('tsrm', 0, (N, opt.n_head, N)).to(c3d.dtype) if drop is not None else None
        event = O.event_context(P, tap, c3d, ind, soi, opt.n_head, dmask, et, getattr(opt, 'fST_type', 'fST0'), opt.use_posit)
    clip, mask = O.clip_context(c3d, soi)
    return video, event, clip, mask


def leaves(params, vid, dtype=torch.float32, grad=True):
    P = {k: torch.from_numpy(np.ascontiguousarray(v).copy()).to(dtype).requires_grad_(grad) for k, v in params.items()}
    tap = torch.from_numpy(np.ascontiguousarray(vid['tap']).copy()).to(dtype).requires_grad_(grad)
    c3d, lda = (torch.from_numpy(np.ascontiguousarray(vid[k])).to(dtype) for k in ('c3d', 'lda'))
    return P, tap, c3d, lda


def run(opt, params, vid, train_mode, backward=True, dtype=torch.float32, states=None):
    """(log-probs [N,S,V1], loss, parameter gradients, d tap_feats) of CaptionGenerator.forward(mode='train') + LanguageModelCriterion."""
    P, tap, c3d, lda = leaves(params, vid, dtype, backward)
    labels = torch.from_numpy(np.ascontiguousarray(vid['labels']))
    masks = torch.from_numpy(np.ascontiguousarray(vid['masks'])).to(dtype)
    drop = U.oracle_drop(opt) if train_mode else None
    video, event, clip, mask = contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi'], drop)
    logp = decoder_forward(P, video, event, clip, mask, labels, opt.CG_input_feats_type, drop, opt.CG_init_feats_type, states)
    loss = O.lm_criterion(logp, labels[:, 1:], masks[:, 1:])
    grads = g_tap = None
    if backward:
        loss.backward()
        grads = {k: (p.grad.numpy().copy() if p.grad is not None else None) for k, p in P.items()}
        g_tap = tap.grad.numpy().copy() if tap.grad is not None else np.zeros(tuple(tap.shape), tap.detach().numpy().dtype)
    return logp.detach().numpy(), float(loss.detach()), grads, g_tap


def sample(opt, params, vid, dtype=torch.float32, margins=None):
    """Greedy decode in eval mode: (seq, logp)."""
    P, tap, c3d, lda = leaves(params, vid, dtype, False)
    with torch.no_grad():
        video, event, clip, mask = contexts(opt, P, tap, c3d, lda, vid['ind'], vid['soi'])
        return decoder_sample(P, video, event, clip, mask, opt.CG_seq_length, opt.CG_input_feats_type, opt.CG_init_feats_type, margins)

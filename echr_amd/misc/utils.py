"""Criteria and optimiser helpers with the reference's names (misc/utils.py:15-122)."""
import torch
import torch.nn as nn

from .. import functional as EF


def if_use_att(caption_model):
    return not (caption_model in ('show_tell', 'all_img', 'fc') or 'allimg' in caption_model)


def decode_sequence(ix_to_word, seq):
    """Index rows -> strings; 0 terminates a row (misc/utils.py:24-38)."""
    rows = seq.tolist() if hasattr(seq, 'tolist') else seq
    out = []
    for row in rows:
        words = []
        for ix in row:
            if ix <= 0:
                break
            words.append(ix_to_word[str(int(ix))])
        out.append(' '.join(words))
    return out


class LanguageModelCriterion(nn.Module):
    """Masked NLL over log-probs [N,S,V+1] (misc/utils.py:62-75), evaluated by echr_nll_loss_fwd."""

    def forward(self, input, target, mask):
        # when `input` comes straight from the native decoder, its backward takes the criterion's gradient in fused form
        # (echr_dec_grads.nll_*: softmax - one-hot in one pass) instead of a dense [N,S,V+1] tensor; see MaskedNLL.backward
        # (a one-video node only, vid None: the log-probs of a batch go through VideoBatch.criterion's per-video slices and take the dense gradient)
        fn = input.grad_fn
        node = fn if (EF.FUSED_NLL[0] and type(fn).__name__ == 'DecoderFunctionBackward' and fn.vid is None) else None
        return EF.MaskedNLL.apply(input, target.to(input.device), mask.to(input.device), node)


class RewardCriterion(nn.Module):
    """Self-critical policy-gradient loss (misc/utils.py:48-59): sum(-input * reward * mask) / sum(mask) with mask = [1 | seq > 0][:, :-1]
    (the step that emitted <eos> counts; no epsilon, unlike LanguageModelCriterion).  input: sample_logprobs [N,T]; seq: gen_result [N,T];
    reward [N,T] (or [N], one value per caption), signed.  Device tensors run through echr_reward_loss_fwd / _bwd; host tensors (rewards
    computed and kept on the host, unit checks) are reduced on the host with the same formula."""

    def forward(self, input, seq, reward):
        reward = torch.as_tensor(reward, dtype=torch.float32)
        seq = torch.as_tensor(seq)
        if reward.dim() == 1:
            reward = reward[:, None].expand(seq.shape[0], seq.shape[1])
        if not input.is_cuda:
            mask = (seq > 0).float()
            mask = torch.cat([mask.new_ones(mask.size(0), 1), mask[:, :-1]], 1).reshape(-1)
            return torch.sum(-input.reshape(-1) * reward.reshape(-1).to(input.dtype) * mask.to(input.dtype)) / torch.sum(mask)
        return EF.RewardLoss.apply(input, seq.to(input.device), reward.to(input.device).contiguous())


class TAPModelCriterion(nn.Module):
    """Weighted BCE of the proposal head (misc/utils.py:78-99), evaluated by echr_tap_bce_fwd/bwd."""

    def forward(self, scores, masks, labels, w1):
        return EF.TapBCE.apply(scores, masks.to(scores.device), labels.to(scores.device), w1.to(scores.device))

    def forward_batch(self, scores, masks, labels, w1, row_offset):
        """The criterion over a multi-video batch in two launches (echr_tap_bce_fwd_batch) and one for its gradient: `scores`, `masks`,
        `labels` are the concatenated [T_tot, K] matrices, `row_offset` [V+1] the videos' rows, `w1` one [K] weight vector for all videos, a
        list of V, or [V, K].  Returns (sum over the videos, per-video losses [V]); the gradient flows through the sum (the per-video losses
        are reported values).  Each video keeps its own mean over its T_v x K elements, no 1/V -- what tap_criterion_batch computes."""
        dev = scores.device
        ro = EF.sst_row_offsets(row_offset, scores.shape[0])
        if isinstance(w1, (list, tuple)):
            if len(w1) != len(ro) - 1:
                raise ValueError('w1 must be one weight vector or one per video')
            w1 = torch.stack([torch.as_tensor(w).reshape(-1).to(dev) for w in w1], 0)
        ro_dev = row_offset if (isinstance(row_offset, torch.Tensor) and row_offset.is_cuda and row_offset.dtype == torch.int32) \
            else torch.from_numpy(ro).to(dev)
        return EF.TapBCEBatch.apply(scores, masks.to(dev), labels.to(dev), w1.to(dev), ro_dev)


def tap_criterion_batch(crit, scores, masks, labels, w1, row_offset):
    """TAPModelCriterion over a multi-video batch: `scores`, `masks`, `labels` are the concatenated [T_tot, K] matrices, `row_offset` [V+1]
    the videos' rows, `w1` one [K] weight vector for all videos or a list of V.  Returns (sum over the videos, per-video losses [V]): each
    video keeps its own mean over its T_v x K elements (no 1/V), as V single-video iterations summed (train.py:281-283)."""
    ro = [int(r) for r in (row_offset.tolist() if hasattr(row_offset, 'tolist') else row_offset)]
    if len(ro) < 2 or ro[0] != 0 or any(b <= a for a, b in zip(ro[:-1], ro[1:])) or ro[-1] != scores.shape[0]:
        raise ValueError('row_offset must start at 0, grow strictly and end at the number of score rows (%d): %s' % (scores.shape[0], ro))
    per_w1 = isinstance(w1, (list, tuple))
    if per_w1 and len(w1) != len(ro) - 1:
        raise ValueError('w1 must be one weight vector or one per video')
    per = [crit(scores[a:b], masks[a:b], labels[a:b], w1[v] if per_w1 else w1) for v, (a, b) in enumerate(zip(ro[:-1], ro[1:]))]
    per = torch.stack(per)
    return per.sum(), per


def set_lr(optimizer, lr):
    for group in optimizer.param_groups:
        group['lr'] = lr


def clip_gradient(optimizer, grad_clip):
    """Element-wise clamp of every gradient to +-grad_clip (misc/utils.py:107-111).

    With echr_amd.optim.ClampAdam the clamp is folded into the fused step kernel (it is recorded here and
    applied inside `step()`); for any other optimiser the clamp runs as its own HIP kernel per tensor."""
    from ..optim import ClampAdam
    if isinstance(optimizer, ClampAdam):
        # The reference clamps the RUNNING gradient after every backward (train.py:313-317): with m_batch > 1 it computes
        # clamp(clamp(g1) + g2).  Per-tensor gradients are clamped in place here.  With the flat arena (ClampAdam.defer_clamp, default on)
        # the clamp is left to the fused step kernel and, should another backward accumulate before the step, applied right before that
        # accumulation -- the same trajectory for any m_batch; only `.grad` read between this call and step() shows unclamped values
        # (set optimizer.defer_clamp = False to clamp in place here, one more 174 MB pass).
        optimizer.clamp_grads_(float(grad_clip))
        optimizer.pending_clip = float(grad_clip)
        return
    for group in optimizer.param_groups:
        for p in group['params']:
            if p.grad is not None:
                EF.clamp_(p.grad.data, grad_clip)


def fix_model_parameters(model):
    for p in model.parameters():
        p.requires_grad = False


def unfix_model_parameters(model):
    for p in model.parameters():
        p.requires_grad = True

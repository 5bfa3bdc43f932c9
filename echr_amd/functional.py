"""torch.autograd bindings of the HIP hot path (one Function per fused region).

PyTorch is plumbing here: it owns device memory, streams and the autograd graph edges; all arithmetic
happens in libechr_hip.so (include/echr_hip.h).  Every call fails loudly when the library or the GPU
is missing -- there is no eager/PyTorch fallback.
"""
import ctypes as C
import os
import types

import numpy as np
import torch

from . import _lib as L


class DropState:
    """Dropout configuration of one forward call (counter-based; see echr_amd/philox.py)."""

    def __init__(self, seed=0, offset=0, training=False, p_tsrm=0.3, p_h=0.5, p_out=0.5):
        self.seed, self.offset, self.training = int(seed), int(offset), bool(training)
        self.p_tsrm, self.p_h, self.p_out = float(p_tsrm), float(p_h), float(p_out)

    def c(self):
        return L.Dropout(self.seed & 0xFFFFFFFFFFFFFFFF, self.offset & 0xFFFFFFFF, 1 if self.training else 0,
                         self.p_tsrm, self.p_h, self.p_out)


def event_index_tensors(soi_select_list, ind_select_list, device, n_rows=None):
    """(ev_start, ev_len, ind) int32 device tensors + max length A from the reference's list inputs
    (numpy int arrays or python lists; CaptionGenerator.py:17, train.py:265-271)."""
    soi = np.asarray(soi_select_list, dtype=np.int64).reshape(-1, 2)
    ind = np.asarray(ind_select_list, dtype=np.int64).reshape(-1)
    lens = soi[:, 1] - soi[:, 0]
    if len(soi) == 0 or lens.min() <= 0:
        raise ValueError('every event needs at least one segment (soi=%s)' % (soi.tolist(),))
    if len(ind) != len(soi):
        raise ValueError('ind_select_list and soi_select_list differ in length (%d vs %d)' % (len(ind), len(soi)))
    if n_rows is not None and (soi.min() < 0 or soi[:, 1].max() > n_rows or ind.min() < 0 or ind.max() >= n_rows):
        raise ValueError('event intervals / anchors fall outside the %d feature rows' % n_rows)
    packed = np.stack([soi[:, 0], lens, ind]).astype(np.int32)
    t = upload(torch.from_numpy(packed), device)
    ev_start, ev_len = t[0].contiguous(), t[1].contiguous()
    c2 = 2 * soi[:, 0] + lens
    ev_len.echr_bounds = (int(lens.max()), int(c2.max() - c2.min()))      # host-known index bounds (echr_tsrm_args.max_len / max_span)
    return ev_start, ev_len, t[2].contiguous(), int(lens.max())


def upload(host_tensor, device):
    """Small host -> device copy that does not stall the host: staged through a pinned buffer from PyTorch's caching host allocator (it
    recycles a block only after the copy that reads it has completed).  A copy from pageable memory makes the host wait until the
    stream has drained, i.e. for the whole previous iteration, and the GPU then idles while the host issues the next one."""
    if host_tensor.is_cuda:
        return host_tensor
    if device.type != 'cuda':
        return host_tensor.to(device)
    stage = torch.empty(host_tensor.shape, dtype=host_tensor.dtype, pin_memory=True)
    stage.copy_(host_tensor)
    return stage.to(device, non_blocking=True)


def rows_disjoint(soi_select_list):
    """True when no two events share a segment row (then d P_all rows are stored instead of atomically added)."""
    soi = np.asarray(soi_select_list, dtype=np.int64).reshape(-1, 2)
    o = soi[np.argsort(soi[:, 0], kind='stable')]
    return bool(np.all(o[1:, 0] >= o[:-1, 1]))


FUSED_NLL = [os.environ.get('ECHR_FUSED_NLL', '1') != '0']        # see MaskedNLL.backward
ASYNC_TAIL = [os.environ.get('ECHR_ASYNC_TAIL', '1') != '0']        # decoder backward: run the last stage on a second stream (arena path); tests may switch it off


def _f32c(t):
    # (inside autograd.Function.forward / backward grad mode is off: inputs can be used and saved as they are)
    if t.dtype is torch.float32 and t.is_contiguous() and (not t.requires_grad or not torch.is_grad_enabled()):
        return t
    return t.detach().to(torch.float32).contiguous()


class GradSink(object):
    """Where a backward Function should write its parameter gradients: the module's flat arena (echr_amd/arena.py).

    Used only when EVERY parameter of the group currently has .grad None -- then the Function zero-fills the group's span
    once, lets the library accumulate into it (`zeroed` = 1) and returns fresh arena views that autograd adopts as .grad
    without a copy.  If any .grad already exists (gradient accumulation) the Function falls back to private buffers so
    that autograd's `grad += new` sees two distinct tensors."""

    def __init__(self, arena, params):
        self.arena, self.params = arena, list(params)
        self.slots = [arena.slot(p) for p in self.params]

    def usable(self):
        ok = all(s is not None for s in self.slots) and all(p.grad is None for p in self.params)
        if not ok:
            # gradient accumulation (a second backward before the optimiser step): a clamp that clip_gradient left to the fused step
            # kernel has to be applied to the running gradient NOW, before autograd adds this backward's gradients to it -- the
            # reference computes clamp(clamp(g1) + g2), not clamp(g1 + g2) (train.py:313-317)
            self.arena.flush_deferred_clamp()
        return ok

    def take(self, defer_zero=False):
        """Fresh arena views of the group's gradients over a zero-filled span.  defer_zero: the caller zero-fills the span itself (the
        decoder backward folds it into its own multi-range fill launch) -- returns (views, span tensor)."""
        lo, hi = self.arena.span(self.slots)
        if self.arena.whole_zero_pass:
            # an earlier Function of THIS backward pass (the decoder, which runs first) zero-filled the whole arena: nothing to fill
            views = [self.arena.grad_view(s) for s in self.slots]
            return (views, None) if defer_zero else views
        if defer_zero and all(p.grad is None for p in self.arena.params):
            lo, hi = 0, self.arena.total      # fresh step: ONE fill covers every group's span and the never-used parameters' slots
            self.arena.whole_zero_pass = True  # valid until this backward pass ends (autograd end-of-pass callback)
            torch.autograd.Variable._execution_engine.queue_callback(self.arena.end_backward_pass)
        span = self.arena.flat_g[lo:hi]
        if not defer_zero:
            span.zero_()
        self.arena.note_zeroed(lo, hi)
        views = [self.arena.grad_view(s) for s in self.slots]
        return (views, span) if defer_zero else views

    def has_hooks(self):
        """True when a parameter of the group carries tensor hooks (DDP / FSDP style post-accumulate hooks, register_hook): they read the
        gradient inside the backward pass, so it must be final when the Function returns (no asynchronous tail)."""
        return any(getattr(p, '_backward_hooks', None) or getattr(p, '_post_accumulate_grad_hooks', None) for p in self.params)


# --------------------------------------------------------------------------------------------------
class EventPoolGather(torch.autograd.Function):
    """ech = [mean-pooled C3D rows | tap[ind]]  (CaptionGenerator.py:111-114,121,128); `parts`: 3 = both ('ER3'), 1 = the pooled rows only
    ('ER1'), 2 = the anchors' SST states only ('ER2').  With event_context_type 'EC' / 'EH' the result of parts 1 / 2 IS the event context
    (CaptionGenerator.py:131-137: no event encoder behind it)."""

    @staticmethod
    def forward(ctx, c3d, tap, ev_start, ev_len, ind, parts=3):
        lib = L.load()
        c3d, tap = _f32c(c3d), _f32c(tap)
        N = ev_start.numel()
        D, Ht = (c3d.shape[1] if parts & 1 else 0), (tap.shape[1] if parts & 2 else 0)
        ech = torch.empty(N, D + Ht, device=c3d.device, dtype=torch.float32)
        L.check(lib.echr_event_pool_gather_fwd(L.ptr(c3d), L.ptr(tap), L.ptr(ev_start, torch.int32), L.ptr(ev_len, torch.int32),
                                               L.ptr(ind, torch.int32), L.ptr(ech), N, D, Ht, L.stream_ptr()), 'event_pool_gather_fwd')
        ctx.save_for_backward(ind)
        ctx.shape = (tap.shape, D, Ht, N)
        return ech

    @staticmethod
    def backward(ctx, g_ech):
        lib = L.load()
        (ind,) = ctx.saved_tensors
        tap_shape, D, Ht, N = ctx.shape
        g_tap = None
        if ctx.needs_input_grad[1] and Ht > 0:
            g_tap = torch.zeros(tap_shape, device=g_ech.device, dtype=torch.float32)
            L.check(lib.echr_event_pool_gather_bwd(L.ptr(_f32c(g_ech)), L.ptr(ind, torch.int32), L.ptr(g_tap), N, D, Ht,
                                                   L.stream_ptr()), 'event_pool_gather_bwd')
        return None, g_tap, None, None, None, None


# --------------------------------------------------------------------------------------------------
TSRM_PARAMS = ('w_emb', 'b_emb', 'w_fc1', 'b_fc1', 'w_fc2', 'b_fc2', 'w_q', 'b_q', 'w_k', 'b_k', 'w_out', 'b_out')


def batch_ext(vid, video=None, g_video=None, n_videos=None, H=None):
    """(echr_batch_ext, its scratch tensor or None) of a multi-video batch (echr_amd/batch.py): vid int32 [N] device, video / g_video
    [V, Dv]; H (decoder entries): rnn_size, sizes the scratch the library works in during the call -- keep the tensor alive until the
    call's kernels have run."""
    V = int(n_videos if n_videos is not None else video.shape[0])
    xws = None
    if H is not None:
        xws = torch.empty(L.load().echr_batch_ws_floats(vid.numel(), V, int(H)), device=vid.device, dtype=torch.float32)
    return L.BatchExt(V, L.ptr(vid, torch.int32), L.ptr(video) if video is not None else None,
                      L.ptr(g_video) if g_video is not None else None, L.ptr(xws) if xws is not None else None), xws


class TSRMFunction(torch.autograd.Function):
    """MA_Attention8.forward (MA_attention_8_NEW.py:35-49, :101-177)."""

    @staticmethod
    def forward(ctx, ech, ev_start, ev_len, n_head, drop, sink, bounds, *params):
        return _tsrm_forward(ctx, ech, ev_start, ev_len, n_head, drop, sink, bounds, params)

    @staticmethod
    def backward(ctx, g_out):
        g_ech, grads = _tsrm_backward(ctx, g_out)
        return (g_ech, None, None, None, None, None, None) + grads


class TSRMBatchFunction(torch.autograd.Function):
    """TSRMFunction over the events of several videos: an event attends to the events of its own video only (`vid` int32 [N] device,
    non-decreasing; echr_tsrm_fwd_batch / _bwd_batch)."""

    @staticmethod
    def forward(ctx, ech, ev_start, ev_len, vid, n_videos, n_head, drop, sink, bounds, *params):
        return _tsrm_forward(ctx, ech, ev_start, ev_len, n_head, drop, sink, bounds, params, batch=(vid, int(n_videos)))

    @staticmethod
    def backward(ctx, g_out):
        g_ech, grads = _tsrm_backward(ctx, g_out)
        return (g_ech, None, None, None, None, None, None, None, None) + grads


def _tsrm_forward(ctx, ech, ev_start, ev_len, n_head, drop, sink, bounds, params, batch=None):
    # bounds: None or (inference, max_len, max_span[, fst_mode]) = echr_tsrm_args' last fields.  `inference` must be decided by the CALLER
    # (grad mode is always off inside forward, and needs_input_grad ignores torch.no_grad())
    lib = L.load()
    ctx.batch = batch
    ctx.sink = sink
    ech = _f32c(ech)
    ps = [_f32c(p) for p in params]
    N, Din = ech.shape
    Df, Do = ps[0].shape[0], ps[10].shape[0]
    if ps[0].shape[1] != Din:
        raise L.EchrHipError('event features are %d wide, fusion_model.event_emb expects %d (video_dim + hidden_dim: CaptionGenerator.py:121-125)'
                             % (Din, ps[0].shape[1]))
    ws = torch.empty(lib.echr_tsrm_ws_floats(N, Din, Df, Do, n_head), device=ech.device, dtype=torch.float32)
    out = torch.empty(N, Do, device=ech.device, dtype=torch.float32)
    a = L.TsrmArgs(N, Din, Df, Do, n_head, *[L.ptr(p) for p in ps], L.ptr(ech), L.ptr(ev_start, torch.int32),
                   L.ptr(ev_len, torch.int32), L.ptr(ws), L.ptr(out), *(bounds or (0, 0, 0)))
    d = drop.c()
    if batch is not None:
        x, _ = batch_ext(batch[0], n_videos=batch[1])
        L.check(lib.echr_tsrm_fwd_batch(C.byref(a), C.byref(d), C.byref(x), L.stream_ptr()), 'tsrm_fwd_batch')
    else:
        L.check(lib.echr_tsrm_fwd(C.byref(a), C.byref(d), L.stream_ptr()), 'tsrm_fwd')
    ctx.save_for_backward(ech, ev_start, ev_len, ws, out, *ps)
    ctx.meta = (N, Din, Df, Do, n_head, drop, int(a.fst_mode))
    return out


def _tsrm_backward(ctx, g_out):
    lib = L.load()
    ech, ev_start, ev_len, ws, out, *ps = ctx.saved_tensors
    N, Din, Df, Do, G, drop, fst_mode = ctx.meta
    g_out = _f32c(g_out)
    zeroed = 1 if (ctx.sink is not None and ctx.sink.usable()) else 0
    grads = ctx.sink.take() if zeroed else [torch.empty_like(p) for p in ps]
    if zeroed:
        grads[10] = grads[10].view(ps[10].shape)              # linear_out_1.weight [d_o, d_feats, 1, 1] -> [d_o, d_feats]
    g_ech = torch.empty_like(ech)
    wsb = torch.empty(lib.echr_tsrm_ws_bwd_floats(N, Din, Df, Do, G), device=ech.device, dtype=torch.float32)
    a = L.TsrmArgs(N, Din, Df, Do, G, *[L.ptr(p) for p in ps], L.ptr(ech), L.ptr(ev_start, torch.int32),
                   L.ptr(ev_len, torch.int32), L.ptr(ws), L.ptr(out), 0, 0, 0, fst_mode)
    g = L.TsrmGrads(*[L.ptr(x) for x in grads], L.ptr(g_ech), L.ptr(g_out), L.ptr(wsb), zeroed)
    if not zeroed and fst_mode in (3, 4):          # parameters the chosen combination does not reach: the library writes nothing there
        for i in ((6, 7, 8, 9) if fst_mode == 3 else (2, 3, 4, 5)):
            grads[i].zero_()
    d = drop.c()
    if ctx.batch is not None:
        x, _ = batch_ext(ctx.batch[0], n_videos=ctx.batch[1])
        L.check(lib.echr_tsrm_bwd_batch(C.byref(a), C.byref(g), C.byref(d), C.byref(x), L.stream_ptr()), 'tsrm_bwd_batch')
    else:
        L.check(lib.echr_tsrm_bwd(C.byref(a), C.byref(g), C.byref(d), L.stream_ptr()), 'tsrm_bwd')
    return g_ech, tuple(grads)


def position_embedding(ev_start, ev_len, d_pos):
    """[N,N,d_pos] fp32 pairwise position embedding generated on device (MA_attention_8_NEW.py:39-41)."""
    lib = L.load()
    N = ev_start.numel()
    pos = torch.empty(N, N, d_pos, device=ev_start.device, dtype=torch.float32)
    L.check(lib.echr_tsrm_posemb(L.ptr(ev_start, torch.int32), L.ptr(ev_len, torch.int32), L.ptr(pos), N, d_pos, L.stream_ptr()),
            'tsrm_posemb')
    return pos


# --------------------------------------------------------------------------------------------------
# parameter order of the decoder Functions
DEC_PARAMS = ('embed', 'w_logit', 'b_logit',
              'w_ih0', 'w_ih1', 'w_ih2', 'w_hh0', 'w_hh1', 'w_hh2', 'b_ih0', 'b_ih1', 'b_ih2', 'b_hh0', 'b_hh1', 'b_hh2',
              'w_c2a', 'b_c2a', 'w_h2a', 'b_h2a', 'w_alpha', 'b_alpha')
DEC_H0_ARG, DEC_TAP_ARG = 11, 12          # positions of `h0` and `tap` among DecoderFunction's inputs (needs_input_grad)


def _dec_args(ps, c3d, ev_start, ev_len, event, video, tokens, A, S, ws, logp, disjoint=False, n_de=None, prepared=0, train=0, h0=None):
    (embed, w_logit, b_logit, wi0, wi1, wi2, wh0, wh1, wh2, bi0, bi1, bi2, bh0, bh1, bh2, w_c2a, b_c2a, w_h2a, b_h2a,
     w_alpha, b_alpha) = ps
    N, De = event.shape if event is not None else n_de
    Tv, D = c3d.shape
    H = wh0.shape[1]
    E = embed.shape[1]
    Ha = w_c2a.shape[0]
    Dv = video.shape[-1]          # ([Dv], or [V, Dv] in a multi-video batch)
    V1 = embed.shape[0]
    assert wi0.shape[1] == E + De and wi1.shape[1] == E + D and wi2.shape[1] == E + Dv, 'LSTM input widths do not match the contexts'
    return L.DecArgs(N, A, Tv, D, H, E, Ha, De, Dv, V1, S, 1 if disjoint else 0,
                     L.ptr(embed), L.ptr(w_logit), L.ptr(b_logit),
                     L.ptr3((wi0, wi1, wi2), 'w_ih'), L.ptr3((wh0, wh1, wh2), 'w_hh'), L.ptr3((bi0, bi1, bi2), 'b_ih'),
                     L.ptr3((bh0, bh1, bh2), 'b_hh'),
                     L.ptr(w_c2a), L.ptr(b_c2a), L.ptr(w_h2a), L.ptr(b_h2a), L.ptr(w_alpha), L.ptr(b_alpha),
                     L.ptr(c3d), L.ptr(ev_start, torch.int32), L.ptr(ev_len, torch.int32), L.ptr(event), L.ptr(video),
                     L.ptr(tokens, torch.int32) if tokens is not None else None, L.ptr(ws), L.ptr(logp) if logp is not None else None,
                     int(prepared), int(train), None, 0, L.ptr(h0) if h0 is not None else None)


def decoder_prepare(video, c3d, ev_start, ev_len, tokens, A, disjoint, params):
    """Start the event-independent part of the decoder forward (echr_decoder_fwd_prepare) on the library's second stream, BEFORE the
    event encoder is launched on the current stream; returns the handle DecoderFunction.forward continues from."""
    lib = L.load()
    video, c3d = _f32c(video), _f32c(c3d)
    ps = [_f32c(p) for p in params]
    S, N = tokens.shape
    V1, E = ps[0].shape
    De = ps[3].shape[1] - E                       # layer0.weight_ih is [4H, E + event_context_dim]
    logp = torch.empty(N, S, V1, device=c3d.device, dtype=torch.float32)
    # echr_dec_args.train: a backward pass can follow (decided here: grad mode is off inside the Function's forward)
    train = 1 if (torch.is_grad_enabled() and any(p.requires_grad for p in params)) else 0
    a = _dec_args(ps, c3d, ev_start, ev_len, None, video, tokens, A, S, None, logp, disjoint, n_de=(N, De), train=train)
    ws = _decoder_ws(a, c3d.device)
    L.check(lib.echr_decoder_fwd_prepare(C.byref(a), L.stream_ptr()), 'decoder_fwd_prepare')
    return dict(ws=ws, logp=logp, video=video, c3d=c3d, ps=ps, tokens=tokens, A=A, disjoint=disjoint, train=train)


def decoder_prepare_cancel():
    """Drop a decoder_prepare() handle that no forward will consume: the current stream waits for the library's second stream, so the
    handle's buffers can go back to the allocator."""
    L.check(L.load().echr_decoder_fwd_prepare_cancel(L.stream_ptr()), 'decoder_fwd_prepare_cancel')


class InitState(torch.autograd.Function):
    """OldModel.init_hidden with CG_init_feats_type (OldModel_NEW.py:79-96): h0 [N, 3H] = init_linear(cat([video | event | clip.mean(1)])) -- the
    tensor the reference then views as (N, 3, H) and transposes; the decoder entry points take it in this layout (echr_dec_args.h0).

    `vid` (int32 [N] device; None = one video, `video` [Dv]): the events of several videos (echr_init_state_fwd_batch / _bwd_batch) -- `video` is
    [V, Dv] and event n reads row vid[n], `A` is not read; the clip mean of an event divides by the padded clip length of ITS video (the
    largest ev_len among that video's events, formed on the device: h0.grad_fn.video_len).  Row n of h0 [N_tot, 3H] is what the single-video
    call returns for that event in its own video; backward returns d video [V, Dv] (a fixed-order segmented sum) and d event, and
    accumulates init_linear's gradients over all rows (GradSink arena accumulation)."""

    @staticmethod
    def forward(ctx, video, event, c3d, ev_start, ev_len, A, vid, use, sink, w, b):
        lib = L.load()
        video, event, c3d, w, b = _f32c(video), _f32c(event), _f32c(c3d), _f32c(w), _f32c(b)
        N, De = event.shape
        if vid is not None:
            if video.dim() != 2:
                raise ValueError('video must be [V, Dv], one scene vector per video (got %s)' % (tuple(video.shape),))
            V = video.shape[0]
            if vid.numel() != N or ev_start.numel() != N or ev_len.numel() != N or not 1 <= V <= N:
                raise ValueError('vid, ev_start and ev_len need one entry per event (%d) and 1 <= V <= N (V = %d)' % (N, V))
        Dv = video.numel() if vid is None else video.shape[1]
        Dsel = sum(d for u, d in zip(use, (Dv, De, c3d.shape[1])) if u)
        if w.shape[1] != Dsel:
            raise L.EchrHipError('init_linear is %d wide, the selected contexts give %d' % (w.shape[1], Dsel))
        feats = torch.empty(N, w.shape[1], device=event.device, dtype=torch.float32)
        h0 = torch.empty(N, w.shape[0], device=event.device, dtype=torch.float32)
        a = _init_state_args(video, event, c3d, ev_start, ev_len, A, vid, use, w, b, feats, h0)
        if vid is not None:
            vlen = torch.empty(V, device=event.device, dtype=torch.int32)
            x, _ = batch_ext(vid, video)
            L.check(lib.echr_init_state_fwd_batch(C.byref(a), C.byref(x), L.ptr(vlen, torch.int32), L.stream_ptr()), 'init_state_fwd_batch')
            ctx.video_len = vlen          # the per-video padded clip lengths the device formed (written with 'C' only; h0.grad_fn.video_len)
        else:
            L.check(lib.echr_init_state_fwd(C.byref(a), L.stream_ptr()), 'init_state_fwd')
        ctx.save_for_backward(video, event, c3d, ev_start, ev_len, vid, w, b, feats)
        ctx.meta = (A, use)
        ctx.sink = sink
        return h0

    @staticmethod
    def backward(ctx, g_h0):
        lib = L.load()
        video, event, c3d, ev_start, ev_len, vid, w, b, feats = ctx.saved_tensors
        A, use = ctx.meta
        g_h0 = _f32c(g_h0)
        zeroed = 1 if (ctx.sink is not None and ctx.sink.usable()) else 0
        g_w, g_b = ctx.sink.take() if zeroed else (torch.empty_like(w), torch.empty_like(b))
        g_video = torch.empty_like(video) if (use[0] and ctx.needs_input_grad[0]) else None
        g_event = torch.zeros_like(event) if (use[1] and ctx.needs_input_grad[1]) else None
        dfeats = torch.empty_like(feats)
        a = _init_state_args(video, event, c3d, ev_start, ev_len, A, vid, use, w, b, feats, None)
        # (d video of a batch travels in echr_batch_ext, like `video` itself)
        g = L.InitStateGrads(L.ptr(g_h0), L.ptr(g_w), L.ptr(g_b), L.ptr(g_video) if vid is None else None, L.ptr(g_event), L.ptr(dfeats), zeroed)
        if vid is not None:
            x, _ = batch_ext(vid, video, g_video)
            L.check(lib.echr_init_state_bwd_batch(C.byref(a), C.byref(g), C.byref(x), L.stream_ptr()), 'init_state_bwd_batch')
        else:
            L.check(lib.echr_init_state_bwd(C.byref(a), C.byref(g), L.stream_ptr()), 'init_state_bwd')
        return g_video, g_event, None, None, None, None, None, None, None, g_w, g_b


def _init_state_args(video, event, c3d, ev_start, ev_len, A, vid, use, w, b, feats, h0):
    """echr_init_state_args of InitState's forward (h0: the output) and backward (h0 None).  A batch (vid) passes `video` in echr_batch_ext
    and A = 0."""
    one = vid is None
    return L.InitStateArgs(event.shape[0], video.numel() if one else video.shape[1], event.shape[1], c3d.shape[1], w.shape[0],
                           int(use[0]), int(use[1]), int(use[2]), int(A) if one else 0, L.ptr(video) if one else None, L.ptr(event), L.ptr(c3d),
                           L.ptr(ev_start, torch.int32), L.ptr(ev_len, torch.int32), L.ptr(w), L.ptr(b), L.ptr(feats), L.ptr(h0))


class ColMean(torch.autograd.Function):
    """x.mean(0) of a [T, D] feature matrix: the 'VC' / 'VH' scene contexts (CaptionGenerator.py:95-99)."""

    @staticmethod
    def forward(ctx, x):
        x = _f32c(x)
        out = torch.empty(x.shape[1], device=x.device, dtype=torch.float32)
        L.check(L.load().echr_col_mean_fwd(L.ptr(x), x.shape[0], x.shape[1], x.shape[1], L.ptr(out), L.stream_ptr()), 'col_mean_fwd')
        ctx.shape = tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        T, D = ctx.shape
        gx = torch.zeros(T, D, device=g.device, dtype=torch.float32)
        L.check(L.load().echr_col_mean_bwd(L.ptr(_f32c(g)), T, D, D, L.ptr(gx), L.stream_ptr()), 'col_mean_bwd')
        return gx


class SegColMean(torch.autograd.Function):
    """ColMean per video of a batch: [V, D] column means over the row segments [row_offset[v], row_offset[v+1]) of the concatenated
    feature matrix x [sum T_v, D], one launch (echr_seg_col_mean_fwd / _bwd); row_offset int32 [V+1] device."""

    @staticmethod
    def forward(ctx, x, row_offset):
        x = _f32c(x)
        V = row_offset.numel() - 1
        out = torch.empty(V, x.shape[1], device=x.device, dtype=torch.float32)
        L.check(L.load().echr_seg_col_mean_fwd(L.ptr(x), L.ptr(row_offset, torch.int32), V, x.shape[1], x.shape[1], L.ptr(out), x.shape[1],
                                               L.stream_ptr()), 'seg_col_mean_fwd')
        ctx.save_for_backward(row_offset)
        ctx.shape = tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        (row_offset,) = ctx.saved_tensors
        T, D = ctx.shape
        gx = torch.zeros(T, D, device=g.device, dtype=torch.float32)
        L.check(L.load().echr_seg_col_mean_bwd(L.ptr(_f32c(g)), D, L.ptr(row_offset, torch.int32), row_offset.numel() - 1, D, D, L.ptr(gx),
                                               L.stream_ptr()), 'seg_col_mean_bwd')
        return gx, None


class DecoderFunction(torch.autograd.Function):
    """OldModel.forward with the ThreeStream core (OldModel_NEW.py:98-137, :376-401, :801-823): log-probs [N,S,V1].  Every input has a fixed
    position (DEC_H0_ARG, DEC_TAP_ARG: where backward reads needs_input_grad); the absent optional ones are None, None, 0, None:

    `prep`: the handle of decoder_prepare(), which already ran the event-independent part on its workspace (one video only).
    `h0` [N, 3H]: the initial state of CG_init_feats_type (InitState's rows; None = zeros); backward returns d h0.
    `tap`, `col0` ('CH' / 'CC+CH'): the rows c3d[:, col0 : col0 + tap width] are tap[:Tv]; backward returns d tap [T, Ht]
    (echr_decoder_row_grad behind echr_decoder_bwd).
    `vid` (int32 [N] device): the events of several videos (echr_decoder_fwd_batch / _bwd_batch) -- `video` is [V, Dv], one scene vector per
    video, and event n reads row vid[n]; `c3d` is the batch's row source (VideoBatch.clip_rows()); backward returns d video [V, Dv]."""

    @staticmethod
    def forward(ctx, video, event, c3d, ev_start, ev_len, tokens, A, disjoint, drop, sink, prep, h0, tap, col0, vid, *params):
        if prep is not None and vid is not None:
            raise ValueError('a decoder_prepare() handle belongs to one video: a batch (vid) runs its forward without one')
        return _decoder_forward(ctx, video, event, c3d, ev_start, ev_len, tokens, A, disjoint, drop, sink, prep, h0, tap, col0, vid, params)

    @staticmethod
    def backward(ctx, g_logp):
        g_video, g_event, g_h0, g_tap, grads = _decoder_backward(ctx, g_logp)
        return (g_video, g_event, None, None, None, None, None, None, None, None, None, g_h0, g_tap, None, None) + grads


def _decoder_ws(a, dev):
    """The workspace of the decoder call `a` (echr_decoder_ws_floats), allocated on `dev` and entered as a.ws."""
    ws = torch.empty(L.load().echr_decoder_ws_floats(C.byref(a)), device=dev, dtype=torch.float32)
    a.ws = L.ptr(ws)
    return ws


def _decoder_forward(ctx, video, event, c3d, ev_start, ev_len, tokens, A, disjoint, drop, sink, prep, h0, tap, col0, vid, params):
    lib = L.load()
    ctx.sink = sink
    ctx.vid = vid
    ctx.tap_meta = (tuple(tap.shape), int(col0)) if tap is not None else None
    event = _f32c(event)
    h0 = _f32c(h0) if h0 is not None else None
    S, N = tokens.shape
    if prep is not None:
        video, c3d, ps, logp, ws = prep['video'], prep['c3d'], prep['ps'], prep['logp'], prep['ws']
        train = prep['train']
        a = _dec_args(ps, c3d, ev_start, ev_len, event, video, tokens, A, S, ws, logp, disjoint, prepared=1, train=train, h0=h0)
    else:
        video, c3d = _f32c(video), _f32c(c3d)
        ps = [_f32c(p) for p in params]
        V1 = ps[0].shape[0]
        logp = torch.empty(N, S, V1, device=event.device, dtype=torch.float32)
        train = 1 if any(ctx.needs_input_grad) else 0
        a = _dec_args(ps, c3d, ev_start, ev_len, event, video, tokens, A, S, None, logp, disjoint, train=train, h0=h0)
        ws = _decoder_ws(a, event.device)
    d = drop.c()
    if vid is not None:
        x, ctx.xws = batch_ext(vid, video, H=ps[6].shape[1])          # (kept with the node: the forward's kernels read it in stream order)
        L.check(lib.echr_decoder_fwd_batch(C.byref(a), C.byref(d), C.byref(x), L.stream_ptr()), 'decoder_fwd_batch')
    else:
        L.check(lib.echr_decoder_fwd(C.byref(a), C.byref(d), L.stream_ptr()), 'decoder_fwd')
    ctx.save_for_backward(video, event, c3d, ev_start, ev_len, tokens, ws, logp, *ps)
    ctx.h0 = h0
    ctx.meta = (A, S, drop, disjoint, train)
    return logp


def _decoder_backward(ctx, g_logp):
    lib = L.load()
    video, event, c3d, ev_start, ev_len, tokens, ws, logp, *ps = ctx.saved_tensors
    A, S, drop, disjoint, train = ctx.meta
    # criterion gradient left here in sparse form by MaskedNLL.backward (LanguageModelCriterion on this node's output)
    pend = ctx.__dict__.pop('_echr_pending_nll', None)     # one entry per LanguageModelCriterion applied to this node's output
    fused = None
    if pend:
        if len(pend) == 1 and getattr(g_logp, '_echr_nll_placeholder', False) and g_logp.stride() == (0, 0, 0):
            fused, g_logp = pend[0], None
        else:          # other consumers of the log-probs (or several criteria): their accumulated gradient plus every criterion's dense one
            for pe in pend:
                g_logp = g_logp + MaskedNLL.dense_grad(pe[0], pe[1], pe[2], pe[3], *logp.shape)
    if g_logp is not None:
        g_logp = _f32c(g_logp)
    zeroed = 1 if (ctx.sink is not None and ctx.sink.usable()) else 0
    zero_span = None
    if zeroed:
        grads, zero_span = ctx.sink.take(defer_zero=True)      # zero-filled inside echr_decoder_bwd's first stage (one fill launch less)
    else:
        red = getattr(ctx.sink.arena, 'early_reducer', None) if ctx.sink is not None else None
        if red is not None:
            red.check_no_backward_while_in_flight()      # accumulating into ranges whose all-reduce already started
        grads = [torch.empty_like(p) for p in ps]
        grads[0].zero_()                                 # embedding table gradient is scatter-added
    g_event = torch.empty_like(event)
    g_video = torch.empty_like(video) if ctx.needs_input_grad[0] else None
    h0 = ctx.h0
    g_h0 = torch.empty_like(h0) if (h0 is not None and ctx.needs_input_grad[DEC_H0_ARG]) else None
    want_tap = ctx.tap_meta is not None and ctx.needs_input_grad[DEC_TAP_ARG]
    a = _dec_args(ps, c3d, ev_start, ev_len, event, video, tokens, A, S, ws, logp, disjoint, train=train, h0=h0)
    wsb = torch.empty(lib.echr_decoder_ws_bwd_floats(C.byref(a)), device=event.device, dtype=torch.float32)
    gp = [L.ptr(x) for x in grads]
    g = L.DecGrads(gp[0], gp[1], gp[2], (L.c_f * 3)(*gp[3:6]), (L.c_f * 3)(*gp[6:9]), (L.c_f * 3)(*gp[9:12]),
                   (L.c_f * 3)(*gp[12:15]), gp[15], gp[16], gp[17], gp[18], gp[19], gp[20],
                   L.ptr(g_event), L.ptr(g_video) if ctx.vid is None else None, L.ptr(g_logp) if g_logp is not None else None,
                   L.ptr(fused[0], fused[0].dtype) if fused else None, L.ptr(fused[1]) if fused else None, L.ptr(fused[3]) if fused else None,
                   L.ptr(wsb), zeroed, 0, 0, L.ptr(fused[2][1:2]) if fused else None,
                   L.ptr(zero_span) if zero_span is not None else None, zero_span.numel() if zero_span is not None else 0,
                   1 if (fused and fused[0].dtype == torch.int64) else 0, 0, None, 0, L.ptr(g_h0) if g_h0 is not None else None)
    d = drop.c()
    if ctx.vid is not None:
        x, xws = batch_ext(ctx.vid, video, g_video, H=ps[6].shape[1])
        bwd = lambda: L.check(lib.echr_decoder_bwd_batch(C.byref(a), C.byref(g), C.byref(d), C.byref(x), L.stream_ptr()), 'decoder_bwd_batch')
    else:
        xws = None
        bwd = lambda: L.check(lib.echr_decoder_bwd(C.byref(a), C.byref(g), C.byref(d), L.stream_ptr()), 'decoder_bwd')
    hook = getattr(ctx.sink.arena, 'early_grad_hook', None) if zeroed else None
    staged = hook is not None and getattr(ctx.sink.arena, 'early_staged', True)
    if staged:
        # data parallel: hand gradients to the reducer as soon as they are final; it starts their all-reduce on the collective
        # stream while the next stage runs on this one.  params order = OldModel.native_params():
        #   [0] embed, [1] logit.weight, [2] logit.bias, [3:6] weight_ih, [6:9] weight_hh, [9:12] bias_ih, [12:15] bias_hh, ...
        sp = ctx.sink.params
        for phase, ready in ((1, [sp[1], sp[2]]), (3, list(sp[3:15])), (4, None)):
            g.phase = phase
            bwd()
            if ready is not None:
                hook(ready)
    else:
        # arena path: the returned parameter gradients are views that autograd adopts without touching them, so the last stage of
        # the backward (attention-parameter / embedding gradients) may still be running on the library's second stream while
        # autograd goes on with the event encoder's backward; an end-of-backward callback joins the streams and only then lets go
        # of the workspaces that stage reads
        # (not when a parameter hook would read those gradients inside the backward pass, nor under create_graph, where autograd may
        # clone them: the gradients must then be final when this Function returns)
        g.async_tail = 1 if (zeroed and ASYNC_TAIL[0] and not ctx.sink.has_hooks() and not torch.is_grad_enabled()) else 0
        if g.async_tail and hook is None:
            # no data-parallel hand-over waits for the LSTM-layer gradients: only d event is formed on this stream, the rest of that stage
            # runs on the library's second helper stream and is joined with the tail by the end-of-backward callback
            g.async_tail = 2
        if g.async_tail == 2 and g_video is not None:
            # Rule: a gradient this Function RETURNS is final in this stream's order.  With async_tail = 2 the LSTM-layer stage, which forms
            # d video, runs on a helper stream that is joined only at the end of the backward pass, while d video's consumers -- the scene
            # mean's backward, autograd's sum with InitState's d video -- run on this stream right behind this node without a join.  So a node
            # whose d video is wanted ('VH' with a tap_feats that requires grad) keeps that stage on this stream; only the tail is asynchronous
            g.async_tail = 1
        bwd()
        if hook is not None:
            # data parallel, one-call form: the LSTM-layer gradients (and everything else part A of the backward produced) are final in
            # stream order now; the reducer starts their all-reduce, which overlaps the asynchronous tail and the event encoder's backward
            hook(list(ctx.sink.params[3:15]), after_recurrence=True)
        if g.async_tail and not want_tap:
            keep = [ws, wsb, logp, c3d, tokens, ev_start, ev_len, g_logp, fused, xws]
            sp = L.stream_ptr()

            def _join(keep=keep, sp=sp):
                L.check(lib.echr_stream_join(sp), 'stream_join')
                del keep[:]
            torch.autograd.Variable._execution_engine.queue_callback(_join)
    g_tap = None
    if want_tap:
        # d rows of the tap columns (echr_decoder_row_grad): orders the asynchronous tail, whose d P_all it reads, on this stream first --
        # every workspace read of that tail then precedes this return in stream order
        (T, Ht), col0 = ctx.tap_meta
        g_tap = torch.zeros(T, Ht, device=event.device, dtype=torch.float32)
        rws = torch.empty(lib.echr_decoder_row_grad_ws_floats(C.byref(a), Ht), device=event.device, dtype=torch.float32)
        r = L.RowGradArgs(col0, Ht, L.ptr(g_tap), Ht, L.ptr(rws))
        L.check(lib.echr_decoder_row_grad(C.byref(a), C.byref(g), C.byref(r), L.stream_ptr()), 'decoder_row_grad')
    return g_video, g_event, g_h0, g_tap, tuple(grads)


def clip_rows(c3d, tap):
    """The 'CC+CH' row source [T, Dc + Ht] = [c3d | tap] over T = min(rows) (echr_clip_rows; no graph: the decoder's backward returns the
    tap columns' gradient itself)."""
    c3d, tap = _f32c(c3d.detach()), _f32c(tap.detach())
    T = min(c3d.shape[0], tap.shape[0])
    rows = torch.empty(T, c3d.shape[1] + tap.shape[1], device=tap.device, dtype=torch.float32)
    L.check(L.load().echr_clip_rows(L.ptr(c3d), c3d.shape[1], L.ptr(tap), tap.shape[1], L.ptr(rows), T, L.stream_ptr()), 'clip_rows')
    return rows


def _check_beam_size(beam_size, V1, note=''):
    """int(beam_size), or ValueError outside [1, min(BEAM_MAX, V1)]; `note` follows the range in the message (functional's own wording)."""
    B = int(beam_size)
    if not 1 <= B <= min(BEAM_MAX, V1):
        raise ValueError('beam_size must be in [1, %d]%s, got %d' % (min(BEAM_MAX, V1), note, B))
    return B


def _stop_step(counts, L_):
    """The width a decode over L_ steps is cut at: t - 1 for the first step t in 1 .. L_ with counts[t] == 0, nobody unfinished
    (OldModel_NEW.py:179-180), or L_."""
    return next((t - 1 for t in range(1, L_ + 1) if counts[t] == 0), L_)


def _cut(seq, slp, T):
    return ([], []) if T == 0 else (seq[:, :T].contiguous(), slp[:, :T].contiguous())


def _decode_inputs(video, event, c3d, ev_start, ev_len, params, h0, vid, rep=1, check_batch=False):
    """The tensors a decode call reads, converted, as one object (fields video, event, c3d, ev_start, ev_len, ps, h0, vid; _decode_call adds
    the workspaces ws / xws, a launcher its own).  rep > 1 (beam slots): event, ev_start, ev_len, h0 and vid are repeated per slot,
    event-major -- row n * rep + j is slot j of event n; the clip rows and scene vectors stay shared.  check_batch: the shape rules of a
    batch (ValueError)."""
    if check_batch:
        if video.dim() != 2:
            raise ValueError('video must be [V, Dv], one scene vector per video (got %s)' % (tuple(video.shape),))
        N, V = event.shape[0], video.shape[0]
        if vid.dim() != 1 or vid.numel() != N or ev_start.numel() != N or ev_len.numel() != N:
            raise ValueError('vid, ev_start and ev_len need one entry per event (%d)' % N)
        if not 1 <= V <= N:
            raise ValueError('a batch has between 1 video and one video per event (V = %d, N = %d)' % (V, N))
    k = types.SimpleNamespace(video=_f32c(video), event=_f32c(event), c3d=_f32c(c3d), ev_start=ev_start, ev_len=ev_len,
                              ps=[_f32c(p) for p in params], h0=_f32c(h0) if h0 is not None else None, vid=vid, ws=None, xws=None)
    if rep > 1:
        # (event, the large one, LAST: repeated first it cost the single-video beam decode about 10 us per call, measured -- the later repeats
        # appear to wait for its copy kernel, which otherwise runs behind the host's set-up of the call)
        for name in ('vid', 'ev_start', 'ev_len', 'h0', 'event'):
            if getattr(k, name) is not None:
                setattr(k, name, getattr(k, name).repeat_interleave(rep, dim=0).contiguous())
    return k


def _decode_call(video, event, c3d, ev_start, ev_len, A, seq_length, params, h0, vid, rep=1, check_batch=False):
    """The set-up every decode launcher shares: (echr_dec_args without tokens / logp, echr_batch_ext or None, keep).  `keep`
    (_decode_inputs) holds EVERY tensor whose raw pointer went into the two structs -- converted inputs and parameters, repeated rows,
    the decoder workspace, the batch scratch.  The library reads them until the call's kernels have run: a launcher adds the buffers it
    allocates itself and holds `keep` until its host read and echr_check_async are behind it."""
    k = _decode_inputs(video, event, c3d, ev_start, ev_len, params, h0, vid, rep, check_batch)
    a = _dec_args(k.ps, k.c3d, k.ev_start, k.ev_len, k.event, k.video, None, A, seq_length, None, None, h0=k.h0)
    k.ws = _decoder_ws(a, k.event.device)
    x = None
    if vid is not None:
        x, k.xws = batch_ext(k.vid, k.video, H=k.ps[6].shape[1])
    return a, x, k


def _sample(video, event, c3d, ev_start, ev_len, A, seq_length, params, h0, vid, drop, multinomial, temperature, seed, table_cache, debug,
            defer, widths):
    """The launcher of greedy_sample and (widths=True: the per-video widths behind the unfinished counts, checked against them and returned)
    of sample_train_batch."""
    lib = L.load()
    a, x, keep = _decode_call(video, event, c3d, ev_start, ev_len, A, seq_length, params, h0, vid, check_batch=widths)
    N, dev = keep.event.shape[0], keep.event.device
    V = keep.video.shape[0] if widths else 0
    wss = keep.wss = torch.empty(lib.echr_sampler_ws_floats(C.byref(a)), device=dev, dtype=torch.float32)
    seq = torch.empty(N, seq_length, device=dev, dtype=torch.int64)
    slp = torch.empty(N, seq_length, device=dev, dtype=torch.float32)
    counts = torch.empty(seq_length + 1 + (V + 1 if widths else 0), device=dev, dtype=torch.int32)          # n_unfinished [L+1] (| video_words [V+1])
    tables, valid = None, 0
    if table_cache is not None and not multinomial:
        nt = lib.echr_sampler_table_floats(C.byref(a))
        if nt > 0:
            key = (PARAM_EPOCH[0], nt, str(dev)) + tuple((p.data_ptr(), p._version) for p in params)
            tables = table_cache.get('tables')
            if tables is None or tables.numel() != nt or tables.device != dev:
                tables = table_cache['tables'] = torch.empty(nt, device=dev, dtype=torch.float32)
                table_cache['key'] = None
            valid = 1 if table_cache.get('key') == key else 0
            table_cache['key'] = None      # marked valid again only once this call has completed without an error
    sa = L.SampleArgs(a, seq_length, L.ptr(seq, torch.int64), L.ptr(slp), L.ptr(counts, torch.int32), L.ptr(wss),
                      1 if multinomial else 0, float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF,
                      L.ptr(tables) if tables is not None else None, valid)
    dc = drop.c() if drop is not None else None
    what = 'decoder_sample_train_batch' if widths else 'decoder_sample'
    if widths:
        L.check(lib.echr_decoder_sample_train_batch(C.byref(sa), C.byref(dc), C.byref(x), counts.data_ptr() + 4 * (seq_length + 1), L.stream_ptr()), what)
    elif vid is not None:
        L.check(lib.echr_decoder_sample_batch(C.byref(sa), C.byref(x), L.stream_ptr()), 'decoder_sample_batch')
    elif drop is not None:
        L.check(lib.echr_decoder_sample_train(C.byref(sa), C.byref(dc), L.stream_ptr()), 'decoder_sample_train')
    else:
        L.check(lib.echr_decoder_sample(C.byref(sa), L.stream_ptr()), what)

    def finish(keep=keep):          # (`keep`: what the queued kernels read, held until the host read below)
        host = counts.cpu().numpy()                # the only device->host sync of the whole decode
        L.check(lib.echr_check_async(), what)
        if tables is not None:
            table_cache['key'] = key
        if debug is not None:                      # tests: the raw logits [N,V1] of the last decoder step (sampler workspace: XT | LOGITS | ...)
            V1, E = keep.ps[0].shape
            o = (N * E + 63) // 64 * 64
            debug['last_logits'] = wss[o:o + N * V1].view(N, V1).clone()
            debug['seq_full'], debug['logp_full'] = seq.clone(), slp.clone()
            debug['stopped_early'] = int(host[0])      # persistent decoder: 1 = every event had emitted <eos> before seq_length and the launch stopped there
        T = _stop_step(host, seq_length)
        if not widths:
            return _cut(seq, slp, T)
        vw = host[seq_length + 1:].astype(np.int64)
        if int(vw[V]) != T:
            raise L.EchrHipError('decoder_sample_train_batch: widths %s disagree with the unfinished counts %s'
                                 % (vw.tolist(), host[:seq_length + 1].tolist()))
        return _cut(seq, slp, T) + (vw[:V],)
    # a deferred decode's uncut output for work queued ahead of the host read (echr_amd.reward): seq [N, seq_length] is written up to the
    # stop step only, counts[:seq_length + 1] is n_unfinished
    finish.seq, finish.counts = seq, counts
    return finish if defer else finish()


def greedy_sample(video, event, c3d, ev_start, ev_len, A, seq_length, params, debug=None, multinomial=False, temperature=1.0, seed=0,
                  table_cache=None, h0=None, drop=None, vid=None, defer=False):
    """OldModel.sample (OldModel_NEW.py:139-187) with every step on device; one host sync at the end.  Greedy arg-max by default
    (sample_max = 1); multinomial=True draws each token from softmax(logp / temperature) (:160-168) with the library's Philox stream
    keyed by `seed`.

    `table_cache`: a dict owned by the caller (one per model); the persistent decoder's parameter-only operands (token-side gate tables,
    logit-weight image) are kept in it and reused while the parameters are unchanged (data pointers, torch version counters and the
    library's own PARAM_EPOCH).

    `drop` (a training-mode DropState, multinomial only): the sampled pass of self-critical training -- the decoder's dropout is active
    with the masks echr_decoder_fwd draws for the same state at the same step (echr_decoder_sample_train).

    `vid` (int32 [N] device): greedy decode of a multi-video batch -- `video` is [V, Dv] and event n reads row vid[n]
    (echr_decoder_sample_batch); `h0` is then the batched InitState's [N, 3H] (an initial state takes the per-step chain at every row count).

    Returns (seq int64 [N,T], logp fp32 [N,T]) with T <= seq_length, or ([], []) when nothing was generated.
    `defer=True`: the decode is queued and a function is returned that performs the host read and returns the result -- a caller with
    several decodes in flight pays one stream drain for all of them (fused.SelfCriticalBatchStep)."""
    if vid is not None and (multinomial or drop is not None):
        raise NotImplementedError('the batched decode here is the greedy one (the sampled pass of a batch is sample_train_batch)')
    if drop is not None and not multinomial:
        raise ValueError('a dropout state is taken by the multinomial decode only (the greedy baseline runs in eval mode)')
    return _sample(video, event, c3d, ev_start, ev_len, A, seq_length, params, h0, vid, drop, multinomial, temperature, seed, table_cache, debug,
                   defer, False)


def sample_train_batch(video, event, c3d, ev_start, ev_len, vid, A, seq_length, params, drop, temperature=1.0, seed=0, defer=False, h0=None):
    """The sampled pass of self-critical training over a multi-video batch (echr_decoder_sample_train_batch): `greedy_sample(...,
    multinomial=True, drop=)` with `video` [V, Dv] and `vid` int32 [N] (device, non-decreasing) naming each event's video.  The decoder's
    dropout is active under `drop` with the masks the batched teacher-forced forward draws at the same step; the draws are keyed (seed,
    batch-global row, step); `h0` [N, 3H]: the batched InitState's initial state (None = zeros).

    Returns (seq int64 [N,T], logp fp32 [N,T], video_words): video_words is a host int64 [V] with the width each video's own call cuts its
    output at (the largest number of non-zero tokens among its rows) and T = max(video_words); ([], [], zeros) when T == 0.  One host read
    per call: the per-step unfinished counts and video_words travel in one vector.  `defer=True`: as in greedy_sample."""
    if drop is None:
        raise ValueError('the sampled pass of self-critical training needs the iteration\'s dropout state')
    return _sample(video, event, c3d, ev_start, ev_len, A, seq_length, params, h0, vid, drop, True, temperature, seed, None, None, defer, True)


BEAM_MAX = 16          # echr_decoder_beam's largest beam


def _beam(video, event, c3d, ev_start, ev_len, vid, A, seq_length, params, beam_size, h0):
    """The launcher of beam_search (vid None: echr_decoder_beam) and beam_search_batch (echr_decoder_beam_batch): (seq [N, seq_length], logp,
    score, widths) with `widths` the one host read of the decode as host int64 -- [T] for one video, video_words [V] | T for a batch."""
    lib = L.load()
    B = _check_beam_size(beam_size, params[0].shape[0], ' (and <= the vocabulary size + 1)')
    i32 = lambda t: t.to(torch.int32)
    a, x, keep = _decode_call(video, event, c3d, i32(ev_start), i32(ev_len), A, seq_length, params, h0, i32(vid) if vid is not None else None,
                              rep=B, check_batch=vid is not None)
    N, dev = event.shape[0], keep.event.device
    seq = torch.empty(N, seq_length, device=dev, dtype=torch.int64)
    slp = torch.empty(N, seq_length, device=dev, dtype=torch.float32)
    score = torch.empty(N, device=dev, dtype=torch.float32)
    words = torch.empty(N + 1, device=dev, dtype=torch.int32)
    ba = L.BeamArgs(a, B, seq_length, L.ptr(seq, torch.int64), L.ptr(slp), L.ptr(score), L.ptr(words, torch.int32), None)
    keep.wsb = torch.empty(lib.echr_beam_ws_floats(C.byref(ba)), device=dev, dtype=torch.float32)
    ba.ws_beam = L.ptr(keep.wsb)
    if vid is None:          # (either branch ends in the only device->host sync of the whole decode)
        what = 'decoder_beam'
        L.check(lib.echr_decoder_beam(C.byref(ba), L.stream_ptr()), what)
        widths = [words[N].item()]
    else:
        what, vwords = 'decoder_beam_batch', torch.empty(keep.video.shape[0] + 1, device=dev, dtype=torch.int32)
        L.check(lib.echr_decoder_beam_batch(C.byref(ba), C.byref(x), L.ptr(vwords, torch.int32), L.stream_ptr()), what)
        widths = vwords.cpu().numpy()
    L.check(lib.echr_check_async(), what)
    del keep          # (held up to here: the library read its tensors through raw pointers)
    return seq, slp, score, np.asarray(widths, dtype=np.int64)


def beam_search(video, event, c3d, ev_start, ev_len, A, seq_length, params, beam_size, h0=None):
    """Beam search (OldModel.sample with opt beam_size, eval mode) with every step on device; one host sync at the end
    (echr_decoder_beam).  Each event's beam_size slots are rows of one decode over N * beam_size event-major rows: event, ev_start,
    ev_len and h0 are repeated per slot (the clip rows and their attention projection stay shared).  Per step the beam_size largest
    s_j + logp_j[v] over the alive slots win (ties to the smaller slot, then the smaller token); <eos> or the last step finishes a
    hypothesis, and an event keeps the finished one with the greatest score.  No length penalty.

    Returns (seq int64 [N,T], logp fp32 [N,T], score fp32 [N]): T = the longest result's word count, seq its words then zeros, logp
    its token log-probs with the <eos> one at each row's word count (when inside T) then zeros, score the sum of its log-probs (<eos>
    included).  seq and logp are [] when T == 0.  beam_size = 1 gives the greedy decode's seq up to each row's first <eos>."""
    seq, slp, score, widths = _beam(video, event, c3d, ev_start, ev_len, None, A, seq_length, params, beam_size, h0)
    return _cut(seq, slp, int(widths[0])) + (score,)


def beam_search_batch(video, event, c3d, ev_start, ev_len, vid, A, seq_length, params, beam_size, trim=True, h0=None):
    """`beam_search` over the events of a multi-video batch in one decode (echr_decoder_beam_batch): `video` is [V, Dv], `vid` int32 [N]
    (device, non-decreasing) names each event's video, `c3d` / `ev_start` are the batch's concatenated rows and batch-absolute starts.
    event, ev_start, ev_len, vid and `h0` (the batched InitState's [N, 3H]; None = zeros) are repeated per slot.

    Returns (seq int64 [N,T], logp fp32 [N,T], score fp32 [N], video_words): video_words is a host int64 [V] with the longest result's
    word count of each video -- the width that video's decode has alone -- and T = max(video_words).  A video's rows are zero from its
    own width on in seq; its logp may hold the <eos> log-prob of a full-width row in that column.  seq and logp are [] when T == 0.  One
    host read (video_words) per call.  trim=False returns seq and logp at their full width [N, seq_length] whatever T is (a caller that
    assembles several decodes into one result, CaptionGenerator.beam_batch, cuts once at the end)."""
    seq, slp, score, widths = _beam(video, event, c3d, ev_start, ev_len, vid, A, seq_length, params, beam_size, h0)
    return ((seq, slp) if not trim else _cut(seq, slp, int(widths[-1]))) + (score, widths[:-1])


def decoder_step(it, video, event, c3d, ev_start, ev_len, A, state, params, drop=None):
    """OldModel.get_logprobs_state (OldModel_NEW.py:133-137): ONE timestep, state in / state out.

    it int [N] tokens; state = (h [3,N,H] dropped outputs, c [3,N,H]).  Returns (log-probs [N,V1], (h', c')).  Forward only."""
    lib = L.load()
    video, event, c3d = _f32c(video), _f32c(event), _f32c(c3d)
    ps = [_f32c(p) for p in params]
    N = event.shape[0]
    dev = event.device
    V1 = ps[0].shape[0]
    tok = it.to(device=dev, dtype=torch.int32).contiguous()
    h_in, c_in = _f32c(state[0]), _f32c(state[1])
    if tuple(h_in.shape) != tuple(c_in.shape) or h_in.shape[0] != 3 or h_in.shape[1] != N:
        raise ValueError('state must be a pair of [3,N,H] tensors (got %s, %s)' % (tuple(h_in.shape), tuple(c_in.shape)))
    logp = torch.empty(N, V1, device=dev, dtype=torch.float32)
    a = _dec_args(ps, c3d, ev_start, ev_len, event, video, tok, A, 1, None, logp)
    ws = _decoder_ws(a, dev)          # noqa: F841
    h_out, c_out = torch.empty_like(h_in), torch.empty_like(c_in)
    d = (drop if drop is not None else DropState(training=False)).c()
    L.check(lib.echr_decoder_step(C.byref(a), L.ptr(h_in), L.ptr(c_in), L.ptr(h_out), L.ptr(c_out), C.byref(d), L.stream_ptr()), 'decoder_step')
    return logp, (h_out, c_out)


def tsrm_attention(roi_feat, position_embedding, n_head, params, d_o, drop=None, fst_mode=0):
    """attention_module_multi_head.forward (MA_attention_8_NEW.py:101-177) on the embedded events roi_feat [N,Df] and the pairwise
    position embedding [N,N,Df].  params = (fc1.w, fc1.b, fc2.w, fc2.b, q.w, q.b, k.w, k.b, out.w [Do,Df], out.b).  Forward only."""
    lib = L.load()
    x, pos = _f32c(roi_feat), _f32c(position_embedding)
    ps = [_f32c(p) for p in params]
    N, Df = x.shape
    if tuple(pos.shape) != (N, N, Df):
        raise ValueError('position_embedding must be [N,N,%d] (got %s)' % (Df, tuple(pos.shape)))
    Din = Df
    ws = torch.empty(lib.echr_tsrm_ws_floats(N, Din, Df, d_o, n_head), device=x.device, dtype=torch.float32)
    out = torch.empty(N, d_o, device=x.device, dtype=torch.float32)
    a = L.TsrmArgs(N, Din, Df, d_o, n_head, None, None, *[L.ptr(p) for p in ps], None, None, None, L.ptr(ws), L.ptr(out), 0, 0, 0, fst_mode)
    d = (drop if drop is not None else DropState(training=False)).c()
    L.check(lib.echr_tsrm_attn_fwd(C.byref(a), L.ptr(x), L.ptr(pos), C.byref(d), L.stream_ptr()), 'tsrm_attn_fwd')
    return out


# --------------------------------------------------------------------------------------------------
_ZERO_PLACEHOLDER = {}


def _nll_target(target, S):
    """Targets for the criterion kernels: int64 (the reference's LongTensor labels) and int32 are both read in place."""
    t = target[:, :S]
    if t.dtype not in (torch.int64, torch.int32):
        t = t.to(torch.int64)
    return t.contiguous()


class GatherTokens(torch.autograd.Function):
    """Teacher-forced log-probs [N,S,V1] gathered at the tokens seq [N,T] (T <= S): the `sampleLogprobs = logprobs.gather(1, it)` of
    OldModel.sample (OldModel_NEW.py:168) recomputed from a teacher-forced pass (echr_gather_tokens_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, logp, seq):
        lib = L.load()
        N, S, V1 = logp.shape
        T = seq.shape[1]
        if seq.shape[0] != N or T > S:
            raise ValueError('seq %s does not fit log-probs %s' % (tuple(seq.shape), tuple(logp.shape)))
        logp = _f32c(logp)
        sq = seq.to(device=logp.device, dtype=torch.int64).contiguous()
        out = torch.empty(N, T, device=logp.device, dtype=torch.float32)
        L.check(lib.echr_gather_tokens_fwd(L.ptr(logp), L.ptr(sq, torch.int64), L.ptr(out), N, S, T, V1, L.stream_ptr()), 'gather_tokens_fwd')
        ctx.save_for_backward(sq)
        ctx.shape = (N, S, T, V1)
        return out

    @staticmethod
    def backward(ctx, g):
        (sq,) = ctx.saved_tensors
        N, S, T, V1 = ctx.shape
        g_logp = torch.empty(N, S, V1, device=sq.device, dtype=torch.float32)
        L.check(L.load().echr_gather_tokens_bwd(L.ptr(_f32c(g)), L.ptr(sq, torch.int64), L.ptr(g_logp), N, S, T, V1, L.stream_ptr()),
                'gather_tokens_bwd')
        return g_logp, None


class RewardLoss(torch.autograd.Function):
    """RewardCriterion.forward (misc/utils.py:48-59) on device: sum(-input * reward * mask) / sum(mask), mask = [1 | seq > 0][:, :-1]."""

    @staticmethod
    def forward(ctx, input, seq, reward):
        lib = L.load()
        N, T = input.shape
        x = _f32c(input)
        sq = seq.to(device=x.device, dtype=torch.int64).contiguous()
        rw = _f32c(reward.to(device=x.device, dtype=torch.float32))
        if tuple(sq.shape) != (N, T) or tuple(rw.shape) != (N, T):
            raise ValueError('RewardCriterion: input %s, seq %s and reward %s must all be [N, T]' % (tuple(input.shape), tuple(seq.shape), tuple(reward.shape)))
        out = torch.empty(2, device=x.device, dtype=torch.float32)
        L.check(lib.echr_reward_loss_fwd(L.ptr(x), L.ptr(sq, torch.int64), L.ptr(rw), L.ptr(out), N, T, L.stream_ptr()), 'reward_loss_fwd')
        ctx.save_for_backward(sq, rw, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        sq, rw, out = ctx.saved_tensors
        N, T = sq.shape
        g_in = torch.empty(N, T, device=sq.device, dtype=torch.float32)
        L.check(L.load().echr_reward_loss_bwd(L.ptr(sq, torch.int64), L.ptr(rw), L.ptr(out), L.ptr(_f32c(g).reshape(1)), L.ptr(g_in), N, T,
                                              L.stream_ptr()), 'reward_loss_bwd')
        return g_in, None, None


class MaskedNLL(torch.autograd.Function):
    """LanguageModelCriterion.forward (misc/utils.py:66-75) on device."""

    @staticmethod
    def forward(ctx, logp, target, mask, node=None):
        lib = L.load()
        ctx.node = node
        N, S, V1 = logp.shape
        logp = logp.contiguous()
        tgt = _nll_target(target, S)
        msk = mask[:, :S].to(torch.float32).contiguous()
        out = torch.empty(2, device=logp.device, dtype=torch.float32)
        fn = lib.echr_nll_loss_fwd_i64 if tgt.dtype == torch.int64 else lib.echr_nll_loss_fwd
        L.check(fn(L.ptr(logp), L.ptr(tgt, tgt.dtype), L.ptr(msk), L.ptr(out), N, S, V1, L.stream_ptr()), 'nll_loss_fwd')
        ctx.save_for_backward(tgt, msk, out)
        ctx.shape = (N, S, V1)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        tgt, msk, out = ctx.saved_tensors
        N, S, V1 = ctx.shape
        if ctx.node is not None:
            # the log-probs came from DecoderFunction: leave the criterion's gradient with that node in its sparse form (targets, mask,
            # upstream scalar) and hand autograd a stride-0 all-zero placeholder.  DecoderFunction.backward takes the fused path when the
            # placeholder arrives untouched, and adds the dense form when other consumers of the log-probs contributed gradients too.
            ctx.node.__dict__.setdefault('_echr_pending_nll', []).append((tgt, msk, out, _f32c(g).reshape(1)))
            z = _ZERO_PLACEHOLDER.get(msk.device)
            if z is None:                         # one zero scalar per device, filled once (never written: only ever expanded)
                z = _ZERO_PLACEHOLDER[msk.device] = torch.zeros((), device=msk.device, dtype=torch.float32)
            ph = z.expand(N, S, V1)
            ph._echr_nll_placeholder = True
            return ph, None, None, None
        return MaskedNLL.dense_grad(tgt, msk, out, g, N, S, V1), None, None, None

    @staticmethod
    def dense_grad(tgt, msk, out, g, N, S, V1):
        lib = L.load()
        g_logp = torch.empty(N, S, V1, device=msk.device, dtype=torch.float32)
        fn = lib.echr_nll_loss_bwd_i64 if tgt.dtype == torch.int64 else lib.echr_nll_loss_bwd
        L.check(fn(L.ptr(tgt, tgt.dtype), L.ptr(msk), L.ptr(out), L.ptr(_f32c(g).reshape(1)), L.ptr(g_logp), N, S, V1,
                   L.stream_ptr()), 'nll_loss_bwd')
        return g_logp


# Bumped by every parameter update the library performs through raw pointers (clamp_adam_: torch's per-tensor version counters do not see
# those writes); part of the key of caches of parameter-derived operands (OldModel.sample's decoding tables).
PARAM_EPOCH = [0]


def clamp_adam_(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, clip=100.0, applied=None):
    """In-place fused clamp(+-clip) + Adam over flat fp32 buffers (misc/utils.py:107-111 + optim.Adam).  `applied`: optional int32 device
    tensor [1] the launch increments iff the update was applied (echr_clamp_adam_counted)."""
    lib = L.load()
    PARAM_EPOCH[0] += 1
    L.check(lib.echr_clamp_adam_counted(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), int(step), float(lr), float(beta1),
                                        float(beta2), float(eps), float(clip), None if applied is None else L.ptr(applied, torch.int32),
                                        L.stream_ptr()), 'clamp_adam')


def clamp_(g, clip):
    lib = L.load()
    L.check(lib.echr_clamp(L.ptr(g), g.numel(), float(clip), L.stream_ptr()), 'clamp')
    return g


def gemm(A, B, trans_b=True, bias=None, algo=0):
    """C = A @ B^T (trans_b) or A @ B on the fp32 MFMA path; exposed for kernel-level parity tests."""
    lib = L.load()
    M, K = A.shape
    Nn = B.shape[0] if trans_b else B.shape[1]
    Cc = torch.empty(M, Nn, device=A.device, dtype=torch.float32)
    d = L.GemmDesc()
    d.A, d.B, d.C = L.ptr(A), L.ptr(B), L.ptr(Cc)
    d.M, d.N, d.K = M, Nn, K
    d.sam, d.sak = K, 1
    d.sbk, d.sbn = (1, K) if trans_b else (Nn, 1)
    d.ldc = Nn
    d.batch, d.alpha, d.beta, d.split_k, d.algo = 1, 1.0, 0.0, -1, algo
    d.bias = L.ptr(bias) if bias is not None else None
    L.check(lib.echr_gemm_f32(C.byref(d), L.stream_ptr()), 'gemm_f32')
    return Cc


# --------------------------------------------------------------------------------------------------
class SSTFunction(torch.autograd.Function):
    """SST.forward (models/sst_model.py:31-40): 2-layer LSTM + sigmoid proposal head, native.  Without offsets (`ro_host` None) x is one video
    [T, D] (echr_sst_fwd / echr_sst_bwd); with them it is the concatenated [T_tot, D] matrix of a multi-video batch (echr_sst_fwd_batch /
    echr_sst_bwd_batch): `ro_host` the validated int32 offsets (sst_row_offsets), `ro_dev` their device copy, and the parameter gradients are
    the sum over the videos."""

    @staticmethod
    def forward(ctx, x, ro_host, ro_dev, p_drop, drop, sink, *params):
        ctx.sink = sink
        x = _f32c(x)
        ps = [_f32c(p) for p in params]           # w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1, w_sc, b_sc
        T, H, K = x.shape[0], ps[1].shape[1], ps[8].shape[0]
        ws = SSTFunction._workspace(x, ps, ro_host, 'ws')
        tap = torch.empty(T, H, device=x.device, dtype=torch.float32)
        scores = torch.empty(T, K, device=x.device, dtype=torch.float32)
        SSTFunction._call('fwd', ro_host, ro_dev, drop, SSTFunction._args(ps, x, p_drop, ws, tap, scores))
        ctx.save_for_backward(x, ws, tap, scores, *([] if ro_host is None else [ro_dev]), *ps)
        ctx.meta = (p_drop, drop, ro_host)
        return tap, scores

    @staticmethod
    def _args(ps, x, p_drop, ws, tap, scores):
        T, D = x.shape
        H, K = ps[1].shape[1], ps[8].shape[0]
        two = lambda a, b: (L.c_f * 2)(L.ptr(a), L.ptr(b))
        return L.SstArgs(T, D, H, K, float(p_drop), two(ps[0], ps[4]), two(ps[1], ps[5]), two(ps[2], ps[6]), two(ps[3], ps[7]),
                         L.ptr(ps[8]), L.ptr(ps[9]), L.ptr(x), L.ptr(ws), L.ptr(tap), L.ptr(scores))

    @staticmethod
    def _workspace(x, ps, ro_host, which):
        """The forward ('ws') or backward ('ws_bwd') workspace of the call: the batch entries size their own."""
        lib = L.load()
        dims = (x.shape[0], x.shape[1], ps[1].shape[1], ps[8].shape[0])
        n = getattr(lib, 'echr_sst_%s_floats' % which)(*dims) if ro_host is None else \
            getattr(lib, 'echr_sst_batch_%s_floats' % which)(*dims, len(ro_host) - 1)
        return torch.empty(n, device=x.device, dtype=torch.float32)

    @staticmethod
    def _call(direction, ro_host, ro_dev, drop, a, *grads):
        """echr_sst_<direction> on the argument struct `a` (and the gradient struct), or its _batch form when the call has offsets."""
        lib = L.load()
        rest = [C.byref(g) for g in grads] + [C.byref(drop.c()), L.stream_ptr()]
        if ro_host is None:
            L.check(getattr(lib, 'echr_sst_' + direction)(C.byref(a), *rest), 'sst_' + direction)
        else:
            bx = L.SstBatch(len(ro_host) - 1, L.ptr(ro_dev, torch.int32), ro_host.ctypes.data)
            L.check(getattr(lib, 'echr_sst_%s_batch' % direction)(C.byref(a), C.byref(bx), *rest), 'sst_%s_batch' % direction)

    @staticmethod
    def backward(ctx, g_tap, g_scores):
        p_drop, drop, ro_host = ctx.meta
        x, ws, tap, scores, *ps = ctx.saved_tensors
        ro_dev = ps.pop(0) if ro_host is not None else None
        # flat arena (no gradient live yet): ONE zero fill of the span, then every product accumulates (`zeroed`): the split-K weight-gradient
        # products would otherwise zero-fill their own outputs, one launch each
        use_arena = ctx.sink is not None and ctx.sink.usable()
        grads = ctx.sink.take() if use_arena else [torch.empty_like(p) for p in ps]
        wsb = SSTFunction._workspace(x, ps, ro_host, 'ws_bwd')
        g_tap, g_scores = (_f32c(t) if t is not None else None for t in (g_tap, g_scores))          # (held: the call reads the fp32 copies)
        two = lambda a_, b_: (L.c_f * 2)(L.ptr(a_), L.ptr(b_))
        g = L.SstGrads(two(grads[0], grads[4]), two(grads[1], grads[5]), two(grads[2], grads[6]), two(grads[3], grads[7]),
                       L.ptr(grads[8]), L.ptr(grads[9]), L.ptr(g_tap), L.ptr(g_scores), L.ptr(wsb), 1 if use_arena else 0)
        SSTFunction._call('bwd', ro_host, ro_dev, drop, SSTFunction._args(ps, x, p_drop, ws, tap, scores), g)
        return (None,) * 6 + tuple(grads)


def sst_row_offsets(row_offset, rows):
    """Validated host int32 copy of a batch's row offsets [V+1]: they start at 0, every video has a row, the last one equals `rows`."""
    ro = np.asarray(row_offset.detach().cpu().numpy() if isinstance(row_offset, torch.Tensor) else row_offset)
    if ro.ndim != 1 or len(ro) < 2 or not np.issubdtype(ro.dtype, np.integer) and np.any(ro != np.floor(ro)):
        raise ValueError('row_offset must be a vector of V + 1 integers')
    ro = ro.astype(np.int64)
    if ro[0] != 0:
        raise ValueError('row_offset must start at 0 (got %d)' % ro[0])
    if np.any(np.diff(ro) <= 0):
        raise ValueError('every video needs at least one feature row (row_offset=%s)' % ro.tolist())
    if int(ro[-1]) != int(rows):
        raise ValueError('row_offset ends at %d but the features have %d rows' % (ro[-1], rows))
    return np.ascontiguousarray(ro.astype(np.int32))


class TapBCE(torch.autograd.Function):
    """TAPModelCriterion.forward (misc/utils.py:78-99) on device."""

    @staticmethod
    def forward(ctx, scores, masks, labels, w1):
        lib = L.load()
        scores, masks, labels, w1 = _f32c(scores), _f32c(masks), _f32c(labels), _f32c(w1).reshape(-1)
        T, K = scores.shape
        buf = torch.empty(65, device=scores.device, dtype=torch.float32)          # loss | 64 partial sums
        loss = buf[:1]
        L.check(lib.echr_tap_bce_fwd_ws(L.ptr(scores), L.ptr(masks), L.ptr(labels), L.ptr(w1), L.ptr(loss), L.ptr(buf[1:]), T, K, L.stream_ptr()),
                'tap_bce_fwd')
        ctx.save_for_backward(scores, masks, labels, w1)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        lib = L.load()
        scores, masks, labels, w1 = ctx.saved_tensors
        T, K = scores.shape
        gs = torch.empty_like(scores)
        L.check(lib.echr_tap_bce_bwd(L.ptr(scores), L.ptr(masks), L.ptr(labels), L.ptr(w1), L.ptr(_f32c(g).reshape(1)), L.ptr(gs), T, K,
                                     L.stream_ptr()), 'tap_bce_bwd')
        return gs, None, None, None


class TapBCEBatch(torch.autograd.Function):
    """TAPModelCriterion over a multi-video batch (echr_tap_bce_fwd_batch / _bwd_batch): scores / masks / labels are the concatenated
    [T_tot, K] matrices, `ro_dev` the int32 device row offsets [V+1], w1 [K] (all videos) or [V, K].  Returns (sum over the videos,
    per-video losses [V]); each video keeps its own mean over T_v x K, no 1/V."""

    @staticmethod
    def forward(ctx, scores, masks, labels, w1, ro_dev):
        lib = L.load()
        scores, masks, labels, w1 = _f32c(scores), _f32c(masks), _f32c(labels), _f32c(w1)
        T, K = scores.shape
        V = ro_dev.numel() - 1
        w1_ld = 0 if w1.numel() == K else K
        if tuple(masks.shape) != (T, K) or tuple(labels.shape) != (T, K) or (w1_ld and tuple(w1.shape) != (V, K)):
            raise ValueError('masks / labels must be shaped like scores %s, w1 [K] or [V, K] (got %s, %s, %s)'
                             % ((T, K), tuple(masks.shape), tuple(labels.shape), tuple(w1.shape)))
        buf = torch.empty(1 + 64 * V, device=scores.device, dtype=torch.float32)          # sum | 64 partial sums per video
        per = torch.empty(V, device=scores.device, dtype=torch.float32)
        L.check(lib.echr_tap_bce_fwd_batch(L.ptr(scores), L.ptr(masks), L.ptr(labels), L.ptr(w1), w1_ld, L.ptr(ro_dev, torch.int32), V, K,
                                           L.ptr(per), L.ptr(buf[:1]), L.ptr(buf[1:]), L.stream_ptr()), 'tap_bce_fwd_batch')
        ctx.save_for_backward(scores, masks, labels, w1, ro_dev)
        ctx.meta = (V, w1_ld)
        ctx.mark_non_differentiable(per)
        return buf[0], per

    @staticmethod
    def backward(ctx, g, _g_per):
        lib = L.load()
        scores, masks, labels, w1, ro_dev = ctx.saved_tensors
        V, w1_ld = ctx.meta
        T, K = scores.shape
        gs = torch.empty_like(scores)
        L.check(lib.echr_tap_bce_bwd_batch(L.ptr(scores), L.ptr(masks), L.ptr(labels), L.ptr(w1), w1_ld, L.ptr(ro_dev, torch.int32), V, K, T,
                                           L.ptr(_f32c(g).reshape(1)), L.ptr(gs), L.stream_ptr()), 'tap_bce_bwd_batch')
        return gs, None, None, None, None


def h2_pack(x, transposed=False):
    """h2-packed image (two block-scaled fp16 planes, include/echr_hip.h) of the operand x [R,K] -- or, with transposed=True,
    of x^T for x stored [K,R] (the pack transposes on the fly).  Returns (uint8 buffer, R, K)."""
    lib = L.load()
    x = _f32c(x)
    if transposed:
        K, R = x.shape
        s_row, s_col = 1, x.stride(0)
    else:
        R, K = x.shape
        s_row, s_col = x.stride(0), 1
    buf = torch.empty(int(lib.echr_h2_bytes(R, K)), device=x.device, dtype=torch.uint8)
    L.check(lib.echr_h2_pack(L.ptr(x), R, K, s_row, s_col, buf.data_ptr(), L.stream_ptr()), 'h2_pack')
    return buf, R, K


def gemm_h2(a_packed, b_packed, bias=None):
    """C[M,N] = A . B^T (+ bias) from two h2-packed operands."""
    lib = L.load()
    (ab, M, K), (bb, N, K2) = a_packed, b_packed
    if K != K2:
        raise ValueError('contraction lengths differ (%d vs %d)' % (K, K2))
    out = torch.empty(M, N, device=ab.device, dtype=torch.float32)
    d = L.GemmDesc()
    d.A, d.B, d.C = ab.data_ptr(), bb.data_ptr(), out.data_ptr()
    d.M, d.N, d.K = M, N, K
    d.sam, d.sak, d.sbk, d.sbn = K, 1, 1, K
    d.ldc, d.batch, d.alpha, d.beta, d.split_k, d.algo = N, 1, 1.0, 0.0, -1, 2
    if bias is not None:
        d.bias = L.ptr(_f32c(bias))
    L.check(lib.echr_gemm_f32(C.byref(d), L.stream_ptr()), 'gemm_h2')
    return out

"""The one-stream attention decoder (`caption_model='show_attend_tell'`, one LSTM layer) on libechr_hip.so: the autograd Function over
echr_sat_fwd / echr_sat_bwd, one get_logprobs_state (echr_sat_step) and the greedy decode (echr_sat_sample); over a multi-video batch
(echr_amd.batch.VideoBatch) SatBatchFunction over echr_sat_fwd_batch / _bwd_batch and sat_greedy_sample(vid=) over echr_sat_sample_batch.  Reference:
models/OldModel_NEW.py:98-187 (OldModel) over :190-274 (ShowAttendTellCore).  The helpers mirror functional.DecoderFunction /
decoder_step / greedy_sample; nothing here changes those."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import functional as EF

# parameter order of the Functions below (ShowAttendTellModel.native_params())
SAT_PARAMS = ('embed', 'w_logit', 'b_logit', 'w_ih', 'w_hh', 'w_c2a', 'b_c2a', 'w_h2a', 'b_h2a', 'w_alpha', 'b_alpha')
SAT_H0_ARG = 10          # position of `h0` among SatFunction's inputs (needs_input_grad)
FEAT_V, FEAT_E, FEAT_C = 1, 2, 4


def feats_bits(input_feats_type):
    """echr_sat_args.feats of a CG_input_feats_type string (the reference tests membership: OldModel_NEW.py:218-242)."""
    t = input_feats_type or ''
    return (FEAT_V if 'V' in t else 0) | (FEAT_E if 'E' in t else 0) | (FEAT_C if 'C' in t else 0)


def _opt(t):
    return EF._f32c(t) if t is not None else None


def _sat_args(ps, feats, c3d, ev_start, ev_len, event, video, tokens, A, S, ws, logp, disjoint=False, train=0, h0=None):
    embed, w_logit, b_logit, w_ih, w_hh, w_c2a, b_c2a, w_h2a, b_h2a, w_alpha, b_alpha = ps
    N = ev_start.numel()
    Tv, D = c3d.shape
    H = w_hh.shape[1]
    V1, E = embed.shape
    Ha = w_c2a.shape[0]
    De = event.shape[1] if event is not None else 0
    Dv = video.shape[-1] if video is not None else 0
    X = (Dv if feats & FEAT_V else 0) + (De if feats & FEAT_E else 0) + (D if feats & FEAT_C else 0)
    if w_ih.shape[1] != E + X or w_logit.shape[1] != H or w_c2a.shape[1] != D:
        raise L.EchrHipError('show_attend_tell: the LSTM input is %d wide, the token and the selected contexts give %d (logit %s, ctx2att %s)'
                             % (w_ih.shape[1], E + X, tuple(w_logit.shape), tuple(w_c2a.shape)))
    return L.SatArgs(N, A, Tv, D, H, E, Ha, De, Dv, V1, S, feats, 1 if disjoint else 0,
                     L.ptr(embed), L.ptr(w_logit), L.ptr(b_logit), L.ptr(w_ih), L.ptr(w_hh),
                     L.ptr(w_c2a), L.ptr(b_c2a), L.ptr(w_h2a), L.ptr(b_h2a), L.ptr(w_alpha), L.ptr(b_alpha),
                     L.ptr(c3d), L.ptr(ev_start, torch.int32), L.ptr(ev_len, torch.int32),
                     L.ptr(event) if feats & FEAT_E else None, L.ptr(video) if feats & FEAT_V else None,
                     L.ptr(tokens, torch.int32) if tokens is not None else None, L.ptr(h0) if h0 is not None else None,
                     L.ptr(ws) if ws is not None else None, L.ptr(logp) if logp is not None else None, int(train))


def _sat_ws(a, dev):
    ws = torch.empty(L.load().echr_sat_ws_floats(C.byref(a)), device=dev, dtype=torch.float32)
    a.ws = L.ptr(ws)
    return ws


class BatchVid(object):
    """`vid` of a multi-video batch for the echr_sat_*_batch entries: the video of every event, checked on the HOST (the library sees a
    device pointer) and uploaded once.  vid: host integers [N]; n_videos: V; dev: an int32 device copy the caller already has
    (VideoBatch.dev('vid')), else `device` to upload to.  Raises ValueError for an empty or decreasing vid, entries outside [0, V) and
    V outside [1, N]."""

    def __init__(self, vid, n_videos, dev=None, device=None):
        self.host = check_vid(vid, n_videos)
        self.n_videos = int(n_videos)
        self.dev = dev if dev is not None else torch.from_numpy(self.host).to(device)
        if self.dev.numel() != len(self.host):
            raise ValueError('the device copy of vid has %d entries, the host vector %d' % (self.dev.numel(), len(self.host)))


def check_vid(vid, n_videos):
    """The layout contract of echr_batch_ext.vid as int32 [N]: 1 <= n_videos <= N, entries in [0, n_videos), non-decreasing."""
    v = np.asarray(vid.detach().cpu().numpy() if isinstance(vid, torch.Tensor) else vid).reshape(-1)
    V = int(n_videos)
    if V < 1 or V > len(v):
        raise ValueError('n_videos=%d: a batch holds 1 <= n_videos <= N videos (N = %d events)' % (V, len(v)))
    if v.min() < 0 or v.max() >= V:
        raise ValueError('vid names videos outside [0, n_videos=%d)' % V)
    if np.any(np.diff(v.astype(np.int64)) < 0):
        raise ValueError('vid decreases: the events of a video are contiguous and videos keep their order (vid non-decreasing)')
    return np.ascontiguousarray(v, dtype=np.int32)


def _sat_batch_ext(vid, video, feats, N, H, g_video=None):
    """(echr_batch_ext, its scratch or None) of a one-stream call: the scratch is read with 'V' only."""
    if not isinstance(vid, BatchVid):
        raise TypeError('vid must be a sat.BatchVid (the host-checked video index of the batch)')
    if vid.dev.numel() != N:
        raise ValueError('vid needs one entry per event (%d), got %d' % (N, vid.dev.numel()))
    xws = None
    if feats & FEAT_V:
        if video is None or video.dim() != 2 or video.shape[0] != vid.n_videos:
            raise ValueError("'V' needs video [n_videos=%d, Dv], one scene vector per video (got %s)"
                             % (vid.n_videos, None if video is None else tuple(video.shape)))
        xws = torch.empty(L.load().echr_sat_batch_ws_floats(N, vid.n_videos, H), device=vid.dev.device, dtype=torch.float32)
    return L.BatchExt(vid.n_videos, L.ptr(vid.dev, torch.int32), L.ptr(video) if feats & FEAT_V else None,
                      L.ptr(g_video) if g_video is not None else None, L.ptr(xws) if xws is not None else None), xws


class SatBatchFunction(torch.autograd.Function):
    """SatFunction over the events of V videos (echr_sat_fwd_batch / _bwd_batch): `video` is [V, Dv] and row n reads video[vid[n]]; c3d holds
    the concatenated rows, ev_start is batch-absolute, A the widest event of the batch, h0 the batched InitState's [N, H].  Row n of the
    log-probs [N_tot, S, V1] is what SatFunction returns for that event in its own video (under equal dropout masks: the one site is keyed
    by the batch-global row).  backward returns d video [V, Dv] (a fixed-order segmented sum), d event, d h0 and the eleven parameter
    gradients, summed over the videos; with a GradSink they are accumulated into the arena's views.  `vid`: a BatchVid."""

    @staticmethod
    def forward(ctx, video, event, c3d, ev_start, ev_len, tokens, A, disjoint, drop, sink, h0, feats, vid, *params):
        lib = L.load()
        video, event, c3d = _opt(video), _opt(event), EF._f32c(c3d)
        h0 = EF._f32c(h0) if h0 is not None else None
        ps = [EF._f32c(p) for p in params]
        S, N = tokens.shape
        x, xws = _sat_batch_ext(vid, video, feats, N, ps[4].shape[1])
        logp = torch.empty(N, S, ps[0].shape[0], device=c3d.device, dtype=torch.float32)
        train = 1 if any(ctx.needs_input_grad) else 0
        a = _sat_args(ps, feats, c3d, ev_start, ev_len, event, video, tokens, A, S, None, logp, disjoint, train, h0)
        ws = _sat_ws(a, c3d.device)
        d = drop.c()
        L.check(lib.echr_sat_fwd_batch(C.byref(a), C.byref(d), C.byref(x), L.stream_ptr()), 'sat_fwd_batch')
        ctx.save_for_backward(video, event, c3d, ev_start, ev_len, tokens, ws, logp, *ps)
        ctx.h0, ctx.sink, ctx.vid = h0, sink, vid
        ctx.meta = (A, S, drop, disjoint, train, feats)
        return logp

    @staticmethod
    def backward(ctx, g_logp):
        lib = L.load()
        video, event, c3d, ev_start, ev_len, tokens, ws, logp, *ps = ctx.saved_tensors
        A, S, drop, disjoint, train, feats = ctx.meta
        g_logp = EF._f32c(g_logp)
        zeroed = 1 if (ctx.sink is not None and ctx.sink.usable()) else 0
        grads = ctx.sink.take() if zeroed else [torch.empty_like(p) for p in ps]
        h0 = ctx.h0
        g_video = torch.empty_like(video) if (feats & FEAT_V and ctx.needs_input_grad[0]) else None
        g_event = torch.empty_like(event) if (feats & FEAT_E and ctx.needs_input_grad[1]) else None
        g_h0 = torch.empty_like(h0) if (h0 is not None and ctx.needs_input_grad[SAT_H0_ARG]) else None
        a = _sat_args(ps, feats, c3d, ev_start, ev_len, event, video, tokens, A, S, ws, logp, disjoint, train, h0)
        x, xws = _sat_batch_ext(ctx.vid, video, feats, tokens.shape[1], ps[4].shape[1], g_video)          # noqa: F841 (d video travels in echr_batch_ext)
        wsb = torch.empty(lib.echr_sat_ws_bwd_floats(C.byref(a)), device=c3d.device, dtype=torch.float32)
        g = L.SatGrads(*[L.ptr(t) for t in grads], L.ptr(g_event) if g_event is not None else None, None,
                       L.ptr(g_h0) if g_h0 is not None else None, L.ptr(g_logp), L.ptr(wsb), zeroed)
        d = drop.c()
        L.check(lib.echr_sat_bwd_batch(C.byref(a), C.byref(g), C.byref(d), C.byref(x), L.stream_ptr()), 'sat_bwd_batch')
        return (g_video, g_event, None, None, None, None, None, None, None, None, g_h0, None, None) + tuple(grads)


class SatFunction(torch.autograd.Function):
    """OldModel.forward over ShowAttendTellCore: log-probs [N,S,V1].  backward returns the gradients of video ('V'), event ('E'), h0 and the
    eleven parameters; with a GradSink the parameter gradients are accumulated into the arena's views."""

    @staticmethod
    def forward(ctx, video, event, c3d, ev_start, ev_len, tokens, A, disjoint, drop, sink, h0, feats, *params):
        lib = L.load()
        video, event, c3d = _opt(video), _opt(event), EF._f32c(c3d)
        h0 = EF._f32c(h0) if h0 is not None else None
        ps = [EF._f32c(p) for p in params]
        S, N = tokens.shape
        logp = torch.empty(N, S, ps[0].shape[0], device=c3d.device, dtype=torch.float32)
        train = 1 if any(ctx.needs_input_grad) else 0
        a = _sat_args(ps, feats, c3d, ev_start, ev_len, event, video, tokens, A, S, None, logp, disjoint, train, h0)
        ws = _sat_ws(a, c3d.device)
        d = drop.c()
        L.check(lib.echr_sat_fwd(C.byref(a), C.byref(d), L.stream_ptr()), 'sat_fwd')
        ctx.save_for_backward(video, event, c3d, ev_start, ev_len, tokens, ws, logp, *ps)
        ctx.h0, ctx.sink = h0, sink
        ctx.meta = (A, S, drop, disjoint, train, feats)
        return logp

    @staticmethod
    def backward(ctx, g_logp):
        lib = L.load()
        video, event, c3d, ev_start, ev_len, tokens, ws, logp, *ps = ctx.saved_tensors
        A, S, drop, disjoint, train, feats = ctx.meta
        g_logp = EF._f32c(g_logp)          # (LanguageModelCriterion hands this node its dense gradient: misc/utils.py keeps the sparse form for DecoderFunction)
        zeroed = 1 if (ctx.sink is not None and ctx.sink.usable()) else 0
        grads = ctx.sink.take() if zeroed else [torch.empty_like(p) for p in ps]
        h0 = ctx.h0
        g_video = torch.empty_like(video) if (feats & FEAT_V and ctx.needs_input_grad[0]) else None
        g_event = torch.empty_like(event) if (feats & FEAT_E and ctx.needs_input_grad[1]) else None
        g_h0 = torch.empty_like(h0) if (h0 is not None and ctx.needs_input_grad[SAT_H0_ARG]) else None
        a = _sat_args(ps, feats, c3d, ev_start, ev_len, event, video, tokens, A, S, ws, logp, disjoint, train, h0)
        wsb = torch.empty(lib.echr_sat_ws_bwd_floats(C.byref(a)), device=c3d.device, dtype=torch.float32)
        g = L.SatGrads(*[L.ptr(x) for x in grads], L.ptr(g_event) if g_event is not None else None,
                       L.ptr(g_video) if g_video is not None else None, L.ptr(g_h0) if g_h0 is not None else None, L.ptr(g_logp), L.ptr(wsb), zeroed)
        d = drop.c()
        L.check(lib.echr_sat_bwd(C.byref(a), C.byref(g), C.byref(d), L.stream_ptr()), 'sat_bwd')
        return (g_video, g_event, None, None, None, None, None, None, None, None, g_h0, None) + tuple(grads)


def sat_step(it, video, event, c3d, ev_start, ev_len, A, state, params, feats, drop=None):
    """OldModel.get_logprobs_state over ShowAttendTellCore: ONE timestep.  it int [N]; state = (h [1,N,H], c [1,N,H]), the undropped state.
    Returns (log-probs [N,V1], (h', c')).  Forward only."""
    lib = L.load()
    video, event, c3d = _opt(video), _opt(event), EF._f32c(c3d)
    ps = [EF._f32c(p) for p in params]
    N, dev, V1, H = ev_start.numel(), c3d.device, ps[0].shape[0], ps[4].shape[1]
    tok = it.to(device=dev, dtype=torch.int32).contiguous()
    h_in, c_in = EF._f32c(state[0]), EF._f32c(state[1])
    if tuple(h_in.shape) != (1, N, H) or tuple(c_in.shape) != (1, N, H):
        raise ValueError('state must be a pair of [1,%d,%d] tensors (got %s, %s)' % (N, H, tuple(h_in.shape), tuple(c_in.shape)))
    logp = torch.empty(N, V1, device=dev, dtype=torch.float32)
    a = _sat_args(ps, feats, c3d, ev_start, ev_len, event, video, tok, A, 1, None, logp)
    ws = _sat_ws(a, dev)          # noqa: F841
    h_out, c_out = torch.empty_like(h_in), torch.empty_like(c_in)
    d = (drop if drop is not None else EF.DropState(training=False)).c()
    L.check(lib.echr_sat_step(C.byref(a), L.ptr(h_in), L.ptr(c_in), L.ptr(h_out), L.ptr(c_out), C.byref(d), L.stream_ptr()), 'sat_step')
    return logp, (h_out, c_out)


def sat_greedy_sample(video, event, c3d, ev_start, ev_len, A, seq_length, params, feats, h0=None, vid=None):
    """The greedy branch of OldModel.sample over ShowAttendTellCore with every step on device; one host read at the end.  Returns (seq int64
    [N,T], logp fp32 [N,T]) with T <= seq_length, or ([], []).
    `vid` (a BatchVid): the rows of several videos in one decode (echr_sat_sample_batch) -- `video` is [V, Dv], h0 the batched InitState's;
    every row stops on its own <eos> and T is the width of the batch's longest caption (a video's own width: its rows' non-zero tokens)."""
    lib = L.load()
    video, event, c3d = _opt(video), _opt(event), EF._f32c(c3d)
    ps = [EF._f32c(p) for p in params]
    h0 = EF._f32c(h0) if h0 is not None else None
    N, dev = ev_start.numel(), c3d.device
    a = _sat_args(ps, feats, c3d, ev_start, ev_len, event, video, None, A, seq_length, None, None, h0=h0)
    ws = _sat_ws(a, dev)          # noqa: F841
    wss = torch.empty(lib.echr_sat_sampler_ws_floats(C.byref(a)), device=dev, dtype=torch.float32)
    seq = torch.empty(N, seq_length, device=dev, dtype=torch.int64)
    slp = torch.empty(N, seq_length, device=dev, dtype=torch.float32)
    counts = torch.empty(seq_length + 1, device=dev, dtype=torch.int32)
    sa = L.SatSampleArgs(a, seq_length, L.ptr(seq, torch.int64), L.ptr(slp), L.ptr(counts, torch.int32), L.ptr(wss))
    if vid is not None:
        x, xws = _sat_batch_ext(vid, video, feats, N, ps[4].shape[1])          # noqa: F841
        L.check(lib.echr_sat_sample_batch(C.byref(sa), C.byref(x), L.stream_ptr()), 'sat_sample_batch')
    else:
        L.check(lib.echr_sat_sample(C.byref(sa), L.stream_ptr()), 'sat_sample')
    host = counts.cpu().numpy()                # the only device->host sync of the decode
    L.check(lib.echr_check_async(), 'sat_sample')
    return EF._cut(seq, slp, EF._stop_step(host, seq_length))

"""One training iteration of the caption path as ONE library call (echr_train_step, include/echr_hip.h).

Reference protocol (train.py:281-317, m_batch = 1):
    optimizer.zero_grad(); pred = cg_model(tap_feats, c3d_feats, lda_feats, labels, ind, soi, mode='train')
    loss = crit(pred, labels[:, 1:], masks[:, 1:]); loss.backward(); clip_gradient(optimizer, c); optimizer.step()
`FusedTrainStep(model, optimizer)(...)` is that sequence without autograd: Python fills one argument struct (pointers are stable: flat
parameter / gradient arena, one persistent workspace), packs the index vectors, and makes ONE ctypes call; the library sequences the
same entry points the autograd Functions of echr_amd/functional.py call.  The autograd path stays the general one (gradient
accumulation, other consumers of the log-probs, joint training of the proposal encoder, hooks); both produce the same update
(tests/test_gpu_parity.py::test_fused_train_step_equals_autograd_path).
"""
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib as L
from . import batch as VB
from . import functional as EF
from . import reward as RW
from .models.OldModel_NEW import n_decoder_steps
from .optim import ClampAdam


class FusedTrainStep(object):
    LOSS_SLOTS = 16
    # The library entries of the one-call step (csrc/step.hip).  ENTRIES: which argument structs lead an entry's argument list -- they are
    # ALL the arguments of its *_ws_floats -- and how many of (weight, video_loss, row_offset) follow them in front of the stream.
    ENTRIES = {'train_step': ('a', 0), 'train_step_rw': ('a', 1), 'train_step_clip': ('ax', 0),
               'train_step_batch': ('ab', 2), 'train_step_batch_tap': ('ab', 3), 'train_step_batch_clip': ('axb', 3)}
    # ROUTES: which entry runs a call, keyed by (a VideoBatch?, 'CH' / 'CC+CH' rows?, tap_grad?, weighted criterion?).  _setup sizes the
    # workspace and _launch calls the entry through this ONE table (per object: _routes).  (echr_train_step_clip reads `weighted` from
    # x.rw; a batch always brings weights; echr_train_step_batch_clip runs with tap_grad or without.)
    ROUTES = {(b, c, g, w): ('train_step_batch_clip' if c else 'train_step_batch_tap' if g else 'train_step_batch') if b else
                            ('train_step_clip' if c else 'train_step_rw' if w else 'train_step')
              for b in (False, True) for c in (False, True) for g in (False, True) for w in (False, True)}

    def __init__(self, model, optimizer, grad_clip=None):
        if not isinstance(optimizer, ClampAdam) or optimizer.arena is None:
            raise ValueError('FusedTrainStep needs echr_amd.optim.ClampAdam built with the flat arena (model.build_arena())')
        arena = optimizer.arena
        if hasattr(model, '_require_three_stream'):          # (the one-stream decoder trains on the autograd path: forward, backward, ClampAdam.step)
            model._require_three_stream('fused.%s (the one-call training steps)' % type(self).__name__)
        if getattr(model, '_echr_arena', None) is not arena or not arena.params_in_arena():
            raise ValueError('the optimiser\'s arena is not the model\'s (call model.build_arena() after .cuda(), pass it to ClampAdam)')
        # ('EC' / 'EH': no event encoder -- echr_train_step_args.event_direct; anything else was refused by the model's constructor)
        self.direct = model.event_direct()
        if not self.direct and (not hasattr(model, 'fusion_model') or model.opt.event_context_type not in model.EVENT_ENCODED):
            raise NotImplementedError('the fused step needs the TSRM event encoder (event_context_type ER1 / ER2 / ER3) or a direct event '
                                      'context (EC / EH)')
        if len(optimizer.param_groups) != 1 or {id(p) for p in optimizer.param_groups[0]['params']} != {id(p) for p in arena.params}:
            raise ValueError('the optimiser must hold exactly the model\'s parameters in one group')
        self.model, self.optim, self.arena = model, optimizer, arena
        self.grad_clip = grad_clip if grad_clip is not None else optimizer.grad_clip
        self.lib = L.load()
        # (the helper streams now rather than at the first iteration: their hardware queues then do not depend on what creates streams in between.
        # A process that brings up an RCCL communicator should call echr_streams_init() BEFORE init_process_group -- INTEGRATION.md)
        with torch.cuda.device(arena.flat_p.device):
            L.check(self.lib.echr_streams_init(), 'streams_init')
        self.dev = arena.flat_p.device
        self.a = L.TrainStepArgs()
        # frame-level context (CaptionGenerator.clip_parts): 1 = 'CC'; 2 = 'CH' / 3 = 'CC+CH' run through echr_train_step_clip, whose extension
        # struct carries the C3D features (the decoder's row source is then tap_feats, or [c3d | tap] formed in the library's workspace)
        self.clip = model.clip_parts()
        self._dc = model.opt.video_dim
        self.x = L.ClipStepArgs(self.clip, self._dc, None, 0, None)
        self.bx = L.BatchExt(0, None, None, None, None)          # the multi-video extension: _setup(batch=) fills n_videos and video
        ra, rx, rb = C.byref(self.a), C.byref(self.x), C.byref(self.bx)
        refs = dict(a=(ra,), ax=(ra, rx), ab=(ra, rb), axb=(ra, rx, rb))
        self._routes = {k: (e, refs[self.ENTRIES[e][0]], self.ENTRIES[e][1]) for k, e in self.ROUTES.items()}          # key -> (entry, structs, n)
        self._batched = self._prepared = self._pending_deferred = self.mid_called = False
        self._unused = self.last_video_losses = None
        # ONE ctypes trampoline per callback and object (building a CFUNCTYPE per call is host time inside the timed multi-rank loop); each
        # forwards to the callback of the current call.  An exception inside a ctypes callback cannot propagate: kept, re-raised behind the call
        self._cb_error = self._cb_cur = self._mid_cur = None
        self._cb_keep, self._mid_keep = L.HANDOVER_FN(self._on_handover), L.MID_FN(self._on_mid)
        self._cb_ptr, self._mid_ptr = C.cast(self._cb_keep, C.c_void_p), C.cast(self._mid_keep, C.c_void_p)
        self.ws = None
        self.one = torch.ones(1, device=self.dev, dtype=torch.float32)
        self.loss_ring = torch.zeros(self.LOSS_SLOTS, 2, device=self.dev, dtype=torch.float32)
        self.calls = 0
        self._fill_static()

    def join(self):
        """Make the current stream wait for a deferred update (defer_update=True); no-op otherwise."""
        L.check(self.lib.echr_stream_join(L.stream_ptr()), 'stream_join')

    def _join_deferred(self):
        if self._pending_deferred:
            # a deferred update may still be reading the previous call's inputs (c3d, the staged indices) on the library's streams: order this
            # stream behind it BEFORE the references to them are dropped and torch's allocator may hand that memory to someone else
            self.join()
            self._pending_deferred = False

    def _begin(self, what, prepare=None):
        """The head of every step that runs on this object.  `prepare`: what a pending prepare() means to the caller -- None: its second
        half has to come first; a name: a batch form, with which prepare() does not combine; True: nothing (the caller is that second half,
        or runs no library step)."""
        if self._prepared and prepare is not True:
            if prepare is None:
                raise RuntimeError('prepare() must be followed by a call with prepared=True')
            raise NotImplementedError('prepare() runs ahead of ONE video\'s call: it does not combine with %s' % prepare)
        # a persistent launch of an EARLIER iteration gave up: the optimiser kernels queued behind it skipped their updates (parameters and
        # moments untouched) while the step was already counted -- L.check lets every optimiser wind its count back to the updates its own
        # device word says were applied (ClampAdam._on_async_abort), here and at every other site that can surface the -62
        rc = self.lib.echr_check_async()
        if rc:
            L.check(rc, what + ' (asynchronous failure of an earlier call)')
        self._join_deferred()

    def _launch(self, slot, st, forward_only, *, rw=False, weight=None, video_loss=None, row_offset=None, handover=False, handover_cb=None,
                mid_cb=None, g_loss=None, prepared=False, keep=()):
        """The ONE place that calls a train-step entry, on what _setup (or prepare() + _set_tap) described.  `rw`: the criterion is weighted
        (`weight`: the weights as a device tensor when they did not travel with the index vectors); `video_loss` [V] out and `row_offset`
        int32 [V+1]: device tensors of the batch entries; `g_loss`: a one-element device tensor in place of the unit scalar, for this call
        only; `keep`: what else must stay alive until the next _setup.  Returns the loss (_finish)."""
        a = self.a
        a.prepared, a.handover = 1 if prepared else 0, 1 if handover else 0
        # (echr_train_step_args.handover_cb / mid_cb; handover_user / mid_user stay NULL)
        self._cb_error, self._cb_cur, self._mid_cur, self.mid_called = None, handover_cb, mid_cb, False
        a.handover_cb = self._cb_ptr if (handover and handover_cb is not None) else None
        a.mid_cb = self._mid_ptr if mid_cb is not None else None
        # (set BEFORE the call: if it fails half-way, helper-stream work may already be queued, and the next _setup must join it before it
        # drops the references to this call's inputs)
        self._pending_deferred = bool(a.defer_update)
        self._keep = self._keep + (weight, row_offset, g_loss) + tuple(keep)
        entry, refs, n = self._routes[self._batched, self.clip != 1, bool(a.g_tap), rw]
        if g_loss is not None:
            a.g_loss = L.ptr(g_loss)
        try:
            extra = (L.ptr(weight), L.ptr(video_loss), L.ptr(row_offset, torch.int32))[:n] if n else ()
            L.check(getattr(self.lib, 'echr_' + entry)(*refs, *extra, L.stream_ptr()), entry)
        finally:
            a.g_loss = self.one.data_ptr()
        if self._cb_error is not None:
            e, self._cb_error = self._cb_error, None
            raise e
        return self._finish(slot, st, forward_only)

    # ---- pointers that never change: parameters and their gradient slots ------------------------------------------------------
    def _fill_static(self):
        a, m, ar = self.a, self.model, self.arena
        gp = lambda p: ar.flat_g.data_ptr() + 4 * ar.offsets[ar.slot(p)]
        lm, tp = m.lm_model, ()
        if not self.direct:          # (a direct event context leaves tsrm / tsrm_g zeroed: the library does not read them)
            fm = m.fusion_model
            tp = fm.native_params()
            tsrm_params = (fm.event_emb.weight, fm.event_emb.bias, fm.enc_attn.pair_pos_fc1.weight, fm.enc_attn.pair_pos_fc1.bias,
                           fm.enc_attn.pair_pos_fc2.weight, fm.enc_attn.pair_pos_fc2.bias, fm.enc_attn.query_1.weight, fm.enc_attn.query_1.bias,
                           fm.enc_attn.key_1.weight, fm.enc_attn.key_1.bias, fm.enc_attn.linear_out_1.weight, fm.enc_attn.linear_out_1.bias)
            for name, p, v in zip(EF.TSRM_PARAMS, tsrm_params, tp):
                setattr(a.tsrm, name, L.ptr(v))
                setattr(a.tsrm_g, 'g_' + name, gp(p))
            a.tsrm.Din, a.tsrm.Df, a.tsrm.Do, a.tsrm.G = tp[0].shape[1], tp[0].shape[0], tp[10].shape[0], fm.enc_attn.group
            a.tsrm.fst_mode = fm.fst_mode()
        ps = lm.native_params()
        (embed, w_logit, b_logit, wi0, wi1, wi2, wh0, wh1, wh2, bi0, bi1, bi2, bh0, bh1, bh2, w_c2a, b_c2a, w_h2a, b_h2a, w_alpha, b_alpha) = ps
        d, g = a.dec, a.dec_g
        d.embed, d.w_logit, d.b_logit = L.ptr(embed), L.ptr(w_logit), L.ptr(b_logit)
        d.w_ih, d.w_hh = L.ptr3((wi0, wi1, wi2), 'w_ih'), L.ptr3((wh0, wh1, wh2), 'w_hh')
        d.b_ih, d.b_hh = L.ptr3((bi0, bi1, bi2), 'b_ih'), L.ptr3((bh0, bh1, bh2), 'b_hh')
        d.w_c2a, d.b_c2a, d.w_h2a, d.b_h2a, d.w_alpha, d.b_alpha = (L.ptr(x) for x in (w_c2a, b_c2a, w_h2a, b_h2a, w_alpha, b_alpha))
        g.g_embed, g.g_w_logit, g.g_b_logit = gp(embed), gp(w_logit), gp(b_logit)
        g.g_w_ih = (L.c_f * 3)(gp(wi0), gp(wi1), gp(wi2))
        g.g_w_hh = (L.c_f * 3)(gp(wh0), gp(wh1), gp(wh2))
        g.g_b_ih = (L.c_f * 3)(gp(bi0), gp(bi1), gp(bi2))
        g.g_b_hh = (L.c_f * 3)(gp(bh0), gp(bh1), gp(bh2))
        g.g_w_c2a, g.g_b_c2a, g.g_w_h2a, g.g_b_h2a, g.g_w_alpha, g.g_b_alpha = (gp(x) for x in (w_c2a, b_c2a, w_h2a, b_h2a, w_alpha, b_alpha))
        d.H, d.E, d.Ha, d.V1 = wh0.shape[1], embed.shape[1], w_c2a.shape[0], embed.shape[0]
        d.D = w_c2a.shape[1]
        d.De, d.Dv = wi0.shape[1] - d.E, wi2.shape[1] - d.E
        # (the width check wi0.shape[1] - E == De: against the encoder's output, or the C3D rows' / the proposal encoder's states' width)
        want_de = a.tsrm.Do if not self.direct else (m.opt.video_dim if self.direct == 1 else m.opt.hidden_dim)
        if wi1.shape[1] != d.E + d.D or want_de != d.De:
            raise ValueError('LSTM input widths do not match the contexts')
        a.flat_g, a.n_flat, a.flat_p = ar.flat_g.data_ptr(), ar.total, ar.flat_p.data_ptr()
        a.g_loss = self.one.data_ptr()
        # the reference's non-recipe options (CaptionGenerator.py:106-130 event_context_type; OldModel_NEW.py:72-96 CG_init_feats_type)
        a.event_parts = m.EVENT_ENCODED.get(m.opt.event_context_type, 0)
        a.event_direct = self.direct          # 1 = 'EC', 2 = 'EH': event_parts is not read then
        if getattr(lm, 'CG_init_feats_dim', 0):
            t = lm.CG_init_feats_type
            a.w_init, a.b_init = L.ptr(lm.init_linear.weight), L.ptr(lm.init_linear.bias)
            a.g_w_init, a.g_b_init = gp(lm.init_linear.weight), gp(lm.init_linear.bias)
            a.init_use_v, a.init_use_e, a.init_use_c = int('V' in t), int('E' in t), int('C' in t)
        else:
            a.w_init = a.b_init = a.g_w_init = a.g_b_init = None
            a.init_use_v = a.init_use_e = a.init_use_c = 0
        a.vh_offset, a.tap_rows = -1, 0
        self._keep = (tp, ps)          # (fusion_model.native_params() builds a view of linear_out_1.weight: keep it alive)
        self._epoch_ptrs = (ar.flat_p.data_ptr(), ar.flat_g.data_ptr())

    def _flat_state(self):
        o = self.optim
        if o._flat is None:
            if any(o.state[p] for p in self.arena.params):
                raise RuntimeError('per-tensor optimiser state exists (resumed run on the per-tensor path): load it with ClampAdam.load_state_dict '
                                   'on an arena optimiser, or use the autograd path')
            o._flat = dict(step=0, m=torch.zeros_like(self.arena.flat_p), v=torch.zeros_like(self.arena.flat_p))
        return o._flat

    def prepare(self, c3d_feats, lda_feats, lm_labels, ind_select_list, soi_select_list, targets, masks):
        """Joint 'tap_cg' iteration (train.py:300-313), optional first half: everything of the iteration that does not read tap_feats (index
        staging, the decoder's event-independent part, the gradient-arena fill) starts on the library's prepare stream and runs beside the
        proposal encoder's forward queued next.  Follow with `self(tap_feats, <the same arguments>, prepared=True, ...)`."""
        if hasattr(c3d_feats, 'event_slices'):
            raise NotImplementedError('prepare() runs ahead of ONE video\'s call: it does not take a VideoBatch')
        if self.clip != 1:
            raise NotImplementedError("clip_context_type with 'CH': the attended rows are tap_feats and their attention projection is part of the "
                                      "event-independent half, prepare() runs ahead of them (call without prepare(); JointTrainStep(early_prepare=False))")
        if self.direct:
            raise NotImplementedError("event_context_type 'EC' / 'EH': the library refuses prepared = 1 with a direct event context "
                                      "(echr_train_step_args.event_direct) -- call without prepare(); JointTrainStep does so by itself")
        self._setup(None, c3d_feats, lda_feats, lm_labels, ind_select_list, soi_select_list, targets, masks, True, False, None, False)
        L.check(self.lib.echr_train_step_prepare(C.byref(self.a), L.stream_ptr()), 'train_step_prepare')
        self._prepared = True

    def cancel_prepare(self):
        """Abandon a prepare() whose second half will not follow (the caller's code between the two raised): the prepare stream's work is
        ordered before the workspace can be reused and the object accepts ordinary calls again."""
        if self._prepared:
            self._prepared = False
            L.check(self.lib.echr_decoder_fwd_prepare_cancel(L.stream_ptr()), 'decoder_fwd_prepare_cancel')

    def __call__(self, tap_feats, c3d_feats, lda_feats, lm_labels, ind_select_list, soi_select_list, targets, masks, step=True, forward_only=False,
                 tap_grad=None, defer_update=False, prepared=False, handover=False, handover_cb=None, mid_cb=None, g_loss=None):
        """One iteration; returns the loss as a 0-d device tensor (no host sync).  `targets` / `masks`: what the reference hands its
        criterion (labels[:, 1:], masks[:, 1:]), host or device tensors.  step=False stops after the backward pass and exposes the
        gradients as `.grad` views of the arena (data-parallel reduce, inspection); the caller then steps the optimiser itself.
        `tap_grad`: a zero-filled float32 device tensor shaped like `tap_feats` that receives d loss / d tap_feats (added in place) -- the
        joint 'tap_cg' iteration of train.py:300-313 backpropagates it into the proposal encoder together with its own loss:
        `torch.autograd.backward([tap_loss, tap_feats], [None, tap_grad])`.  `defer_update=True` (with tap_grad and step): the call returns
        once tap_grad and the loss are final in stream order; the parameter gradients and the Adam update finish on the library's helper
        streams beside the proposal encoder's backward.  The next call joins by itself; call `join()` before touching the model's parameters
        in any other way (saving, evaluating, the autograd path).  `prepared=True`: `prepare()` ran with the same arguments.
        `handover=True` (with step=False): the backward pass records the data-parallel hand-over points (echr_handover_wait; DataParallelStep);
        `handover_cb(which, stream_ptr)`: called on the host from inside the call at each point (echr_train_step_args.handover_cb).
        `mid_cb()` (joint form): called on the host from inside the call right behind the work that leads to tap_grad, before the
        parameter-gradient tail is forked (echr_train_step_args.mid_cb; JointTrainStep queues the proposal encoder's backward there);
        `self.mid_called` says whether the library took that form.  `g_loss`: a one-element device tensor that scales every gradient of
        this call (JointTrainStep's lambda2); the returned loss stays unscaled."""
        self._begin('train_step', True if prepared else None)
        if prepared:
            if not self._prepared or not step or forward_only:
                raise RuntimeError('prepared=True needs a preceding prepare() and a full training step')
            self._prepared = False
            self._set_tap(EF._f32c(tap_feats), tap_grad, defer_update, True, False)
            slot, st = self._slot, self._state
        else:
            slot, st = self._setup(tap_feats, c3d_feats, lda_feats, lm_labels, ind_select_list, soi_select_list, targets, masks, step, forward_only,
                                   tap_grad, defer_update)
        return self._launch(slot, st, forward_only, handover=handover and not step and not forward_only, handover_cb=handover_cb, mid_cb=mid_cb,
                            g_loss=g_loss, prepared=prepared)

    def _on_handover(self, which, stream, _user):
        try:
            self._cb_cur(int(which), int(stream))
        except BaseException as e:          # noqa: BLE001
            self._cb_error = e

    def _on_mid(self, _stream, _user):
        self.mid_called = True
        try:
            self._mid_cur()
        except BaseException as e:          # noqa: BLE001
            self._cb_error = e

    def batch(self, batch, step=True, forward_only=False, device_criterion=False, video_losses=True, **unsupported):
        """One iteration over a multi-video batch (echr_amd.batch.VideoBatch) as ONE call (echr_train_step_batch): the reference's
        `m_batch = V` protocol (train.py:281-283,313-317) -- the loss is the SUM over the videos of LanguageModelCriterion (each video with
        its own normaliser), the gradients are summed over the videos, then ONE clamp and ONE Adam step.  Returns the summed loss as a 0-d
        device tensor; `last_video_losses` holds the per-video losses as a device vector [V].  step=False stops after the backward pass and
        exposes the summed gradients as `.grad` views, forward_only=True stops after the criterion, as __call__ does.
        `device_criterion=True` hands targets / masks / weights over as device tensors (all rows) instead of with the index vectors;
        `video_losses=False` skips the per-video losses (`last_video_losses` is then None).
        A model with 'CH' / 'CC+CH' rows takes a batch built for them (VideoBatch.from_videos(..., clip_context_type=)) and runs
        echr_train_step_batch_clip; a model with an initial decoder state takes a batch built for it (CG_init_feats_type=): the call
        forms the state of all rows and init_linear's gradients itself (echr_init_state_fwd_batch / _bwd_batch)."""
        if unsupported:
            raise NotImplementedError('FusedTrainStep.batch does not take %s: tap_grad / defer_update / prepared over a batch are follow-ups '
                                      '(one video per call); the hand-over points of a batch are batch_handover(), the data-parallel step over '
                                      'batches is DataParallelBatchStep' % sorted(unsupported))
        return self._batch_call(batch, step, forward_only, device_criterion, video_losses)

    def batch_handover(self, batch, handover_cb=None, device_criterion=False, video_losses=True):
        """batch(step=False) with the data-parallel hand-over points recorded (echr_train_step_args.handover over echr_train_step_batch /
        echr_train_step_batch_clip): `handover_cb(which, stream_ptr)` is called on the host from inside the call at each point, as __call__
        does for one video; echr_handover_wait is the event form.  DataParallelBatchStep is the caller."""
        return self._batch_call(batch, False, False, device_criterion, video_losses, True, handover_cb)

    def _batch_call(self, batch, step, forward_only, device_criterion, video_losses, handover=False, handover_cb=None):
        m = self.model
        m._check_batch_options(batch)
        self._begin('train_step_batch', 'batch()')
        if batch.labels is None:
            raise ValueError('the batch carries no labels')
        with torch.no_grad():
            video = EF._f32c(m.get_video_context_batch(batch))
        w = batch.criterion_weights()
        tg, mk = batch.targets, batch.crit_masks
        w_dev = None
        if device_criterion:
            tg, mk = tg.to(self.dev), mk.to(self.dev)
            w_dev = torch.from_numpy(w).to(self.dev)
        slot, st = self._setup(batch.tap, batch.c3d, video, batch.labels, batch.ind, batch.soi, tg, mk, step, forward_only, None, False,
                               weights=w, batch=batch)
        self.last_video_losses = torch.empty(batch.n_videos, device=self.dev, dtype=torch.float32) if video_losses else None
        return self._launch(slot, st, forward_only, rw=True, weight=w_dev, video_loss=self.last_video_losses,
                            handover=handover and not step and not forward_only, handover_cb=handover_cb, keep=(video,))

    def _batch_tap(self, batch, tap_grad, ro_dev, video_losses, g_loss=None, step=True, handover=False, handover_cb=None):
        """The caption side of the joint iteration over a batch (echr_train_step_batch_tap; fused.JointBatchStep): batch() with the zero-filled
        `tap_grad` [T_tot, Ht] receiving d loss / d batch.tap.  `ro_dev`: the batch's row offsets as an int32 device vector [V+1];
        `video_losses`: device [V] out; `g_loss`: a one-element device tensor that scales every gradient (lambda2; None = 1) -- the returned
        loss and the per-video losses stay unscaled.  `handover` / `handover_cb` (with step=False): as batch_handover."""
        with torch.no_grad():
            video = EF._f32c(self.model.get_video_context_batch(batch))
        slot, st = self._setup(batch.tap, batch.c3d, video, batch.labels, batch.ind, batch.soi, batch.targets, batch.crit_masks, step, False,
                               tap_grad, False, weights=batch.criterion_weights(), batch=batch)
        self.last_video_losses = video_losses
        return self._launch(slot, st, False, rw=True, video_loss=video_losses, row_offset=ro_dev, handover=handover and not step,
                            handover_cb=handover_cb, g_loss=g_loss, keep=(video,))

    def _set_tap(self, tap, tap_grad, defer_update, step, forward_only):
        a, d = self.a, self.a.dec
        parts, want = (self.direct, a.dec.De) if self.direct else (a.event_parts, a.tsrm.Din)
        if (tap.shape[1] if parts & 2 else 0) + (self._dc if parts & 1 else 0) != want or tap.shape[0] < self._tv_needed:
            raise L.EchrHipError('tap_feats %s do not match the model / the event anchors' % (tuple(tap.shape),))
        a.tap, a.Ht = tap.data_ptr(), tap.shape[1]
        self._tap_keep = tap
        if tap_grad is not None and not forward_only:
            if not (tap_grad.is_cuda and tap_grad.dtype == torch.float32 and tap_grad.is_contiguous() and tuple(tap_grad.shape) == tuple(tap.shape)):
                raise ValueError('tap_grad must be a contiguous float32 device tensor shaped like tap_feats %s' % (tuple(tap.shape),))
            a.g_tap = tap_grad.data_ptr()
        else:
            a.g_tap = None
        a.defer_update = 1 if (defer_update and tap_grad is not None and step and not forward_only) else 0
        # 'VH' (scene context = tap_feats.mean(0), CaptionGenerator.py:95-99) with tap_grad: the library spreads d video's span back over g_tap
        vt = self.model.opt.video_context_type
        if 'VH' in vt and a.g_tap:
            o = self.model.opt
            a.vh_offset = (o.lda_dim if 'VL' in vt else 0) + (o.video_dim if 'VC' in vt else 0)
            a.tap_rows = tap.shape[0]
        else:
            a.vh_offset, a.tap_rows = -1, 0

    def _setup(self, tap_feats, c3d_feats, lda_feats, lm_labels, ind_select_list, soi_select_list, targets, masks, step, forward_only,
               tap_grad, defer_update, drop=None, weights=None, batch=None):
        """(`drop`: the iteration's dropout state when the caller already drew it -- SelfCriticalStep's sampled pass used it; `weights`:
        host [N, >= S] criterion weights of echr_train_step_rw, travelling with the index vectors; `batch`: a VideoBatch -- the arguments
        are then its concatenated features / batch-absolute indices, `lda_feats` is the scene matrix [V, Dv]; with device targets the
        host `weights` do not travel with the index vectors -- FusedTrainStep.batch hands their device copy to echr_train_step_batch itself)"""
        a, m, ar, lib = self.a, self.model, self.arena, self.lib
        self._join_deferred()
        if not c3d_feats.is_cuda:
            raise L.EchrHipError('FusedTrainStep runs on the GPU only')
        if (ar.flat_p.data_ptr(), ar.flat_g.data_ptr()) != self._epoch_ptrs or not ar.params_in_arena():
            raise RuntimeError('the parameter arena moved since this FusedTrainStep was built')
        soi = np.asarray(soi_select_list, dtype=np.int64).reshape(-1, 2)
        ind = np.asarray(ind_select_list, dtype=np.int64).reshape(-1)
        lens = soi[:, 1] - soi[:, 0]
        N = len(soi)
        Tv = c3d_feats.shape[0] if tap_feats is None else min(c3d_feats.shape[0], tap_feats.shape[0])
        if N == 0 or lens.min() <= 0:
            raise ValueError('every event needs at least one segment (soi=%s)' % (soi.tolist(),))
        if len(ind) != N:
            raise ValueError('ind_select_list and soi_select_list differ in length (%d vs %d)' % (len(ind), N))
        if soi.min() < 0 or soi[:, 1].max() > Tv or ind.min() < 0 or ind.max() >= Tv:
            raise ValueError('event intervals / anchors fall outside the %d feature rows' % Tv)
        labels = lm_labels.numpy() if isinstance(lm_labels, torch.Tensor) and not lm_labels.is_cuda else np.asarray(lm_labels.cpu() if isinstance(lm_labels, torch.Tensor) else lm_labels)
        S = n_decoder_steps(labels)
        if S == 0:
            raise ValueError('label tensor needs at least two columns')
        if labels.shape[0] != N:
            raise ValueError('labels have %d rows for %d events' % (labels.shape[0], N))
        c3d, lda = EF._f32c(c3d_feats), EF._f32c(lda_feats)
        tap = None if tap_feats is None else EF._f32c(tap_feats)
        vt = m.opt.video_context_type
        if vt != 'VL' and batch is None:
            # scene context 'VC' / 'VH' (CaptionGenerator.py:87-104): the mean rows are formed ahead of the call (two small launches); what the
            # library sees as its `video` vector is the concatenation.  'VH' makes the scene vector a function of tap_feats: with tap_grad the
            # library routes d video's span back into it (echr_train_step_args.vh_offset, _set_tap).  prepare() runs before tap_feats exist
            if 'VH' in vt and tap is None:
                raise NotImplementedError("video_context_type with 'VH': the scene vector needs tap_feats, prepare() runs ahead of them "
                                          "(call without prepare())")
            with torch.no_grad():
                lda = EF._f32c(m.get_video_context(tap, c3d, lda, ind_select_list, soi_select_list))
        self._tv_needed = int(max(soi[:, 1].max(), ind.max() + 1))
        # Criterion inputs.  On the host (numpy / CPU tensors, as the reference's loader hands them over, train.py:273-279): they travel with
        # the index vectors, and the rows whose mask is non-zero are listed -- the masked-out label positions behind a caption's end cannot
        # reach the loss (misc/utils.py:66-75 multiplies by the mask), so training forms logits, d logits and the logit-layer products on the
        # active rows only.  On the device: used in place, all rows.
        host_nll = not (isinstance(targets, torch.Tensor) and targets.is_cuda) and not (isinstance(masks, torch.Tensor) and masks.is_cuda)
        if weights is not None and not host_nll and batch is None:
            raise ValueError('criterion weights travel with host targets / masks')
        act = None
        if host_nll:
            tg_h = np.ascontiguousarray(np.asarray(targets)[:, :S], dtype=np.int32)
            mk_h = np.ascontiguousarray(np.asarray(masks)[:, :S], dtype=np.float32)
            if tg_h.shape != (N, S) or mk_h.shape != (N, S):
                raise ValueError('targets / masks must be [N, >= S] (got %s, %s)' % (tuple(np.asarray(targets).shape), tuple(np.asarray(masks).shape)))
            if not forward_only:
                # active = up to the LAST non-zero mask entry of each caption: a position behind it reaches neither the loss nor, through
                # the recurrence, any earlier gradient, so every gradient of the reverse recurrence is exactly zero there and the
                # weight-gradient products skip those rows as well (a zero inside a caption stays listed: later steps feed back into it)
                live = np.flip(np.logical_or.accumulate(np.flip(mk_h != 0, 1), 1), 1)
                act = np.flatnonzero(live.T.reshape(-1)).astype(np.int32)               # time-major rows t*N + n, ascending
                if act.size == 0 or act.size == N * S:
                    act = None
        n_act = 0 if act is None else int(act.size)
        n_w = 0 if (weights is None or not host_nll) else N * S
        n_b = 0 if batch is None else N          # echr_train_step_batch: the index vectors end with vid [N]
        host = np.empty((3 + S) * N + n_act + (2 * N * S if host_nll else 0) + n_w + n_b, dtype=np.int32)
        host[:N], host[N:2 * N], host[2 * N:3 * N] = soi[:, 0], lens, ind
        host[3 * N:(3 + S) * N] = labels[:, :S].T.reshape(-1)
        o = (3 + S) * N
        if n_act:
            host[o:o + n_act] = act
        if host_nll:
            host[o + n_act:o + n_act + N * S] = tg_h.reshape(-1)
            host[o + n_act + N * S:o + n_act + 2 * N * S] = mk_h.reshape(-1).view(np.int32)
            if n_w:
                w_h = np.ascontiguousarray(np.asarray(weights)[:, :S], dtype=np.float32)
                if w_h.shape != (N, S):
                    raise ValueError('weights must be [N, >= S] (got %s)' % (tuple(np.asarray(weights).shape),))
                host[o + n_act + 2 * N * S:o + n_act + 3 * N * S] = w_h.reshape(-1).view(np.int32)
            tgt = msk = None
        else:
            tgt = EF._nll_target(targets if targets.is_cuda else EF.upload(targets, self.dev), S)
            msk = (masks if masks.is_cuda else EF.upload(masks, self.dev))[:, :S].to(torch.float32).contiguous()
        if n_b:
            host[-n_b:] = batch.vid
        d = a.dec
        a.tsrm.N = d.N = N
        d.A, d.Tv, d.S, d.rows_disjoint = int(lens.max()), c3d.shape[0], S, 1 if EF.rows_disjoint(soi) else 0
        if c3d.shape[1] != self._dc or (lda.numel() if batch is None else lda.shape[-1]) != d.Dv:
            raise L.EchrHipError('feature widths do not match the model (c3d %d, lda %d)' % (c3d.shape[1], lda.numel()))
        d.c3d, d.video = c3d.data_ptr(), lda.data_ptr()
        if self.clip != 1:
            if tap is None:
                raise NotImplementedError("clip_context_type with 'CH' needs tap_feats (prepare() runs ahead of them)")
            # the row source: tap_feats ('CH') or [c3d | tap] ('CC+CH') over the rows both cover; c3d travels in the extension struct
            d.Tv = tap.shape[0] if self.clip == 2 else min(c3d.shape[0], tap.shape[0])
            d.c3d = None
            self.x.c3d = c3d.data_ptr()
        # (tgt / msk: converted copies that only the argument struct's raw pointers reference -- after prepare() the caller allocates
        # before the second half reads them, so they must stay alive until the next _setup)
        self._keep = (c3d, lda, host, tgt, msk)
        if tap is None:                        # prepare(): tap_feats arrive with the second half
            a.tap, a.Ht, a.g_tap, a.defer_update = None, m.opt.hidden_dim, None, 0
        else:
            self._set_tap(tap, tap_grad, defer_update, step, forward_only)
        a.host_index = host.ctypes.data
        a.n_active, a.host_nll = n_act, 1 if host_nll else 0
        if host_nll:
            a.nll_target, a.nll_target_i64, a.nll_mask = None, 0, None
        else:
            a.nll_target, a.nll_target_i64, a.nll_mask = tgt.data_ptr(), 1 if tgt.dtype == torch.int64 else 0, msk.data_ptr()
        self.last_active_rows = n_act
        if drop is None:
            drop = m.lm_model.next_drop_state(m.encoder_dropout_p())
            drop.training = m.training
        a.drop = drop.c()
        self._batched = batch is not None
        if batch is not None:
            self.bx.n_videos, self.bx.video = batch.n_videos, lda.data_ptr()
        # ('CH' / 'CC+CH': x.rw says whether ONE video's criterion is weighted; a batch's weights travel as the batched entry's own)
        self.x.rw = 1 if (weights is not None and batch is None) else 0
        entry, refs, _ = self._routes[self._batched, self.clip != 1, bool(a.g_tap), weights is not None]
        need = getattr(lib, 'echr_%s_ws_floats' % entry)(*refs)
        if self.ws is None or self.ws.numel() < need:
            self.join()                        # (a deferred update may still be reading the old workspace on the helper streams)
            self.ws = None                     # (released in stream order by the caching allocator)
            self.ws = torch.empty(need, device=self.dev, dtype=torch.float32)
        a.ws, a.ws_floats = self.ws.data_ptr(), self.ws.numel()
        slot = self.loss_ring[self.calls % self.LOSS_SLOTS]
        self.calls += 1
        a.loss = slot.data_ptr()
        a.overlap_encoder = 1 if m.overlap_encoder else 0
        a.forward_only = 1 if forward_only else 0
        a.do_step = 1 if (step and not forward_only) else 0
        o = self.optim
        if not forward_only:
            for p in ar.params:                # the arena is rewritten from scratch: stale .grad views must not survive as "accumulated" gradients
                if p.grad is not None:
                    p.grad = None
            ar.deferred_clamp = None
            ar.end_backward_pass()
        if a.do_step:
            st = self._flat_state()
            group = o.param_groups[0]
            clip = o.pending_clip if o.pending_clip is not None else self.grad_clip
            o.pending_clip = None
            a.adam_m, a.adam_v, a.adam_step = st['m'].data_ptr(), st['v'].data_ptr(), st['step'] + 1
            a.adam_applied = o.applied_counter(self.dev).data_ptr()
            a.lr, (a.beta1, a.beta2), a.eps = group['lr'], group['betas'], group['eps']
            a.clip = float('inf') if clip is None else float(clip)
        else:
            st = None
        self._slot, self._state = slot, st
        return slot, st

    def _finish(self, slot, st, forward_only):
        a, m, ar = self.a, self.model, self.arena
        if a.do_step:
            st['step'] += 1
            self.optim._count_step([st])
            EF.PARAM_EPOCH[0] += 1
            ar._zeroed = []
        elif not forward_only:
            # gradients are final in stream order: expose them the way the autograd path does (views of the arena); never-used
            # parameters keep .grad None (their slots are zero)
            unused = self._unused
            if unused is None:
                unused = self._unused = {id(p) for p in list(m.lm_model.core.fusion_layer.parameters()) +
                                         (list(m.fusion_model.h2a_layer.parameters()) if hasattr(m, 'fusion_model') else [])}
            for i, p in enumerate(ar.params):
                if id(p) not in unused:
                    p.grad = ar.grad_view(i)
            ar._zeroed = [(0, ar.total)]
        return slot[0]


class _SelfCriticalIteration(object):
    """What SelfCriticalStep and SelfCriticalBatchStep share: ONE self-critical training iteration (CaptionGenerator.py:32-37 +
    RewardCriterion, misc/utils.py:48-59; train.py:241-245, 303-308 past --self_critical_after) on the one-call path of `fused` (a
    FusedTrainStep):

      the event context in training mode under the iteration's dropout state -> the sampled decode with the decoder's dropout active under
      the same state (or a pinned gen_result) -> the greedy baseline in eval mode -> the device reward, if any, queued behind both -> the
      host reads -> the reward (device CiderDReward, host callable or an explicit `reward`) -> batch.sampled_criterion -> the
      reward-weighted step on the teacher-forced tokens [0 | gen_result | 0] with the same dropout state: the encoder is recomputed, then
      clamp + Adam as FusedTrainStep does (applied-update counting included).

    A class supplies what differs: its checks ahead of the reference rules and FusedTrainStep._begin, `_contexts`,
    `_sample` / `_greedy` / `_device_reward` (how the decodes and the device reward are queued), `_read`, `_host_reward`, `_criterion` and
    `_step`.  The recomputed event context equals the sampling one within fp32 rounding (bitwise under echr_amd.set_deterministic(True)):
    the same kernels on the same inputs and masks."""
    REWARD_FORM = 'batch'          # batch.reward_matrix's form of a whole reward; BEGIN: the arguments of FusedTrainStep._begin

    def __init__(self, fused, reward_fn=None):
        if not isinstance(fused, FusedTrainStep):
            raise TypeError('%s wraps a FusedTrainStep' % type(self).__name__)
        self.fused, self.reward_fn = fused, reward_fn

    def _iterate(self, x, gen_result, reward, step, refs, **launch):
        """(loss 0-d device tensor, gen_result [N,T] int64 host, greedy_res [N,T'] int64 host, reward [N,T] fp32 host, the groups' widths)."""
        on_device = RW.check_reward_refs(self.reward_fn, refs, reward)
        self.fused._begin(*self.BEGIN)
        if on_device:          # (uploads ahead of everything the iteration queues: a host-to-device copy waits for the stream)
            refs = self.reward_fn.scorer.to(self.fused.dev).device_refs(refs)
        with torch.no_grad():
            c = self._contexts(x, gen_result, on_device)
            self.last_event = c.event          # the event context the decodes read (inspection: the step recomputes it)
            # both decodes and the device reward are queued ahead of the batched form's first read (the single-video sampled decode reads
            # its own counts); the reward is read behind the drain the decodes pay anyway
            sampled = self._sample(c) if gen_result is None else None
            greedy_f = self._greedy(c)
            r_dev = self._device_reward(c, sampled, greedy_f, refs) if on_device else None
            gen_h, greedy, widths, slices = self._read(x, c, sampled, gen_result, greedy_f)
        greedy_h = greedy.cpu() if isinstance(greedy, torch.Tensor) else torch.zeros(c.N, 0, dtype=torch.int64)
        N, T = gen_h.shape[0], int(max(widths))          # (the rows of a pinned gen_result: _setup refuses a wrong count)
        if T == 0:
            raise ValueError('every caption drew <eos> at its first step: nothing to train on (OldModel.sample returns [] then)')
        if r_dev is not None:
            r = VB.reward_matrix(r_dev.cpu(), N, T, self.REWARD_FORM)          # (the stream is drained: a copy of N floats)
            for s, wv in zip(slices, widths):          # one value per caption over its group's own width, zero behind it
                r[s, wv:] = 0.0
        elif reward is None:
            if self.reward_fn is None:
                raise ValueError('%s needs reward_fn or an explicit reward' % type(self).__name__)
            r = self._host_reward(x, gen_h, greedy_h, widths, slices)
        else:
            r = np.ascontiguousarray(VB.reward_matrix(reward, N, T, self.REWARD_FORM))
        labels, mask, w = self._criterion(x, gen_h, r, widths, slices)
        return self._step(x, c, labels, mask, w, step, **launch), gen_h, greedy_h, torch.from_numpy(r), widths

    def _criterion(self, x, gen_h, r, widths, slices):
        return VB.sampled_criterion(gen_h, r, widths, slices, self.REWARD_FORM)


class SelfCriticalStep(_SelfCriticalIteration):
    """The self-critical iteration of ONE video: echr_decoder_sample_train (the slab-sum + draw pair), the persistent greedy decoder,
    echr_train_step_rw with the criterion weight reward * mask (the step normalises with the mask).

    `reward_fn(gen_result, greedy_res)` receives int64 host tensors [N,T] / [N,T'] and returns the reward [N,T] or [N] (one value per
    caption, broadcast over its steps), e.g. CIDEr(gen) - CIDEr(greedy) on the decoded strings."""
    BEGIN, REWARD_FORM = ('self_critical_step',), 'single'

    def batch(self, *args, **kwargs):
        """Multi-video batches (FusedTrainStep.batch) are not part of this step yet: the sampled and greedy decodes and the reward take one video per call."""
        raise NotImplementedError('SelfCriticalStep takes one video per call: self-critical training over a VideoBatch is '
                                  'SelfCriticalBatchStep(fused)(batch) (the module path: CaptionGenerator.train_rl_batch)')

    def __call__(self, tap_feats, c3d_feats, lda_feats, ind_select_list, soi_select_list, gen_result=None, reward=None, step=True, refs=None):
        """Returns (loss 0-d device tensor, gen_result [N,T] int64 host, greedy_res [N,T'] int64 host, reward [N,T] fp32 host).
        `gen_result` (optional): score these captions instead of drawing them (tests pin the sample this way), at the width they come
        with; `reward` (optional): use it instead of calling reward_fn.  step=False stops after the backward pass (gradients as `.grad`
        views, as FusedTrainStep).  `refs` (with an echr_amd.reward.CiderDReward as reward_fn): the packed references of the events in row
        order -- the reward is then scored on the device behind the greedy decode and read behind the greedy decode's own stream drain."""
        return self._iterate((tap_feats, c3d_feats, lda_feats, ind_select_list, soi_select_list), gen_result, reward, step, refs)[:4]

    def _contexts(self, x, gen_result, on_device):
        tap, c3d, lda, ind, soi = x
        m = self.fused.model
        drop = m.lm_model.next_drop_state(m.encoder_dropout_p())
        drop.training = m.training
        ev = EF.event_index_tensors(soi, ind, c3d.device, min(c3d.shape[0], tap.shape[0]))
        video = m.get_video_context(*x)
        clip, clip_mask = m.get_clip_context(*x, _ev=ev)
        event = m.get_event_context(*x, _ev=ev, _drop=drop)
        # (a pinned gen_result goes to the device behind the contexts; the device reward scores it at its own width)
        gen = None if gen_result is None else torch.as_tensor(gen_result).to(dtype=torch.int64)
        return SimpleNamespace(N=len(soi), lm=m.lm_model, drop=drop, event=event, decode=(video, event, clip, clip_mask), gen=gen,
                               gen_d=gen.to(c3d.device) if on_device and gen is not None else None)

    def _sample(self, c):
        return c.lm.sample_train(*c.decode, c.drop)[0]

    def _greedy(self, c):
        was_training = c.lm.training
        c.lm.eval()
        try:
            return c.lm.sample(*c.decode, {'defer': True})
        finally:
            c.lm.train(was_training)

    def _device_reward(self, c, sampled, greedy_f, refs):
        gen_d = c.gen_d if sampled is None else sampled
        if isinstance(gen_d, torch.Tensor) and gen_d.shape[1] > 0:          # gen at its own width, the greedy decode at its device counts
            return self.reward_fn(gen_d, greedy_f.seq, refs, greedy_counts=greedy_f.counts)

    def _read(self, x, c, sampled, gen_result, greedy_f):
        greedy, _ = greedy_f()          # (the greedy decode's own counter read drains the stream)
        gen = c.gen if sampled is None else sampled
        gen_h = gen.cpu() if isinstance(gen, torch.Tensor) else torch.zeros(c.N, 0, dtype=torch.int64)
        return gen_h, greedy, [gen_h.shape[1]], [slice(0, gen_h.shape[0])]          # one group: the tensor as it came

    def _host_reward(self, x, gen_h, greedy_h, widths, slices):
        return VB.reward_matrix(self.reward_fn(gen_h, greedy_h), gen_h.shape[0], widths[0], 'single')

    def _step(self, x, c, labels, mask, w, step):
        tap, c3d, lda, ind, soi = x
        f = self.fused
        slot, st = f._setup(tap, c3d, lda, labels, ind, soi, labels[:, 1:], mask, step, False, None, False, drop=c.drop, weights=w)
        return f._launch(slot, st, False, rw=True)


class SelfCriticalBatchStep(_SelfCriticalIteration):
    """The self-critical iteration over a multi-video batch (echr_amd.batch.VideoBatch): the reference's m_batch = V protocol past
    --self_critical_after (train.py:241-245, 281-283, 303-308) without V sequential calls.  ONE event context over the batch, the sampled
    decode of all N_tot rows (echr_decoder_sample_train_batch, the one-launch multinomial step) and their greedy baseline, ONE host sync
    (both decodes are queued before either is read), echr_train_step_batch with the weights of VideoBatch.reward_weights: the loss is the
    SUM over the videos of RewardCriterion, each video at its own width and with its own normaliser; gradients are summed over the
    videos, then one clamp + Adam.

    `reward_fn(gen_v, greedy_v)` is called once per video, in order, with that video's rows cut to its own widths -- the arguments a
    single-video SelfCriticalStep passes -- and returns [N_v, T_v] or [N_v]; it is not called for a video whose sample has width 0 (that
    video contributes loss 0 and no gradient); `current_video` names the video of the call in progress.  `last_video_losses` holds the
    per-video losses as a device vector [V]."""
    BEGIN, last_video_losses, current_video = ('self_critical_batch_step', 'a batch step'), None, None

    def __call__(self, batch, gen_result=None, reward=None, step=True):
        """Returns (loss 0-d device tensor, gen_result [N_tot,T] int64 host, greedy_res [N_tot,T'] int64 host, reward [N_tot,T] fp32 host,
        video_words int64 [V] host); T = max(video_words).  `gen_result` [N_tot, >= T]: score these captions instead of drawing them;
        `reward` ([N_tot,T] or [N_tot]): use it instead of calling reward_fn.  step=False stops after the backward pass (the summed
        gradients as `.grad` views).  The batch need not carry labels.  Raises ValueError when every video's sample has width 0.
        With an echr_amd.reward.CiderDReward as reward_fn the references travel with the batch: `batch.refs`, the packed references of its
        events in row order (echr_amd.reward.pack_refs).  Both decodes are then scored on the device (their uncut sequences and device
        counts) ahead of the iteration's one host read, and the [N_tot] reward is read behind the same stream drain; a video whose sample
        has width 0 gets reward 0, as with a callable.  A CiderDReward without batch.refs is a ValueError, batch.refs with a plain
        callable a TypeError."""
        return self._iterate(batch, gen_result, reward, step, batch.refs)

    def handover(self, batch, handover_cb=None, gen_result=None, reward=None, refs=None):
        """__call__(step=False) with the data-parallel hand-over points recorded, as FusedTrainStep.batch_handover (DataParallelBatchStep).
        `refs`: instead of batch.refs."""
        return self._iterate(batch, gen_result, reward, False, batch.refs if refs is None else refs, handover=True, handover_cb=handover_cb)

    def _iterate(self, batch, *args, **launch):
        self.fused.model._check_batch_options(batch)          # (ahead of the reference rules and of everything that touches the device)
        return _SelfCriticalIteration._iterate(self, batch, *args, **launch)

    def _contexts(self, batch, gen_result, on_device):
        m = self.fused.model
        # (a pinned gen_result goes to the device ahead of everything the iteration queues)
        gen_d = torch.as_tensor(gen_result).to(self.fused.dev) if on_device and gen_result is not None else None
        video, event, ev_start, ev_len, A, vid, drop = m._batch_contexts(batch, None)
        video = EF._f32c(video)
        # (CG_init_feats_type: both decodes start from the batch's initial state; the step recomputes it inside the call)
        h0 = m._batch_initial_state(batch, video, event, ev_start, ev_len, vid)
        return SimpleNamespace(N=batch.n_events, lm=m.lm_model, drop=drop, event=event, video=video, gen_d=gen_d, A=A, vid=vid, h0=h0,
                               decode=(video, event, batch.clip_rows(), ev_start, ev_len))

    def _sample(self, c):
        return EF.sample_train_batch(*c.decode, c.vid, c.A, c.lm.seq_length, c.lm.native_params(), c.drop, seed=c.lm._sample_seed(), defer=True,
                                     h0=c.h0)

    def _greedy(self, c):
        return EF.greedy_sample(*c.decode, c.A, c.lm.seq_length, c.lm.native_params(), table_cache=c.lm.sample_tables(), vid=c.vid, defer=True,
                                h0=c.h0)

    def _device_reward(self, c, sampled, greedy_f, refs):
        if sampled is not None:          # the uncut sequences at their device counts; a pinned gen_result at its own width
            return self.reward_fn(sampled.seq, greedy_f.seq, refs, gen_counts=sampled.counts, greedy_counts=greedy_f.counts)
        width = min(c.gen_d.shape[1], c.lm.seq_length)
        return self.reward_fn(c.gen_d, greedy_f.seq, refs, gen_width=width, greedy_counts=greedy_f.counts)

    def _read(self, batch, c, sampled, gen_result, greedy_f):
        # the one host sync of the iteration: the first read drains the stream, both decodes included
        if sampled is not None:
            gen, _, vw = sampled()
            gen_h = gen.cpu() if isinstance(gen, torch.Tensor) else torch.zeros(c.N, 0, dtype=torch.int64)
        else:
            vw = batch.caption_widths(gen_result)
            gen_h = torch.from_numpy(VB._np(gen_result, np.int64)[:, :int(vw.max())]).contiguous()
        return gen_h, greedy_f()[0], vw, batch.event_slices

    def _host_reward(self, batch, gen_h, greedy_h, vw, slices):
        r = np.zeros(tuple(gen_h.shape), dtype=np.float32)
        for v, (s, wv, wg) in enumerate(zip(slices, vw.tolist(), batch.caption_widths(greedy_h).tolist())):
            if wv:
                self.current_video = v
                r[s, :wv] = VB.reward_matrix(self.reward_fn(gen_h[s, :wv], greedy_h[s, :wg]), s.stop - s.start, wv, 'video')
        return r

    def _criterion(self, batch, gen_h, r, vw, slices):
        return batch.reward_weights(gen_h, r, vw)

    def _step(self, batch, c, labels, mask, w, step, handover=False, handover_cb=None):
        f = self.fused
        slot, st = f._setup(batch.tap, batch.c3d, c.video, labels, batch.ind, batch.soi, labels[:, 1:], mask, step, False, None, False,
                            drop=c.drop, weights=w, batch=batch)
        self.last_video_losses = f.last_video_losses = torch.empty(batch.n_videos, device=f.dev, dtype=torch.float32)
        return f._launch(slot, st, False, rw=True, video_loss=self.last_video_losses, handover=handover and not step, handover_cb=handover_cb,
                         keep=(c.video,))


class _JointStep(object):
    """What JointTrainStep and JointBatchStep share: the constructor checks and the proposal encoder's bookkeeping around its own calls."""

    def _init_joint(self, fused, tap_model, tap_optim, lambda1, lambda2, tap_grad_clip):
        name = type(self).__name__
        if not isinstance(fused, FusedTrainStep):
            raise TypeError('%s wraps a FusedTrainStep' % name)
        ar = getattr(tap_model, '_echr_arena', None)
        if not isinstance(tap_optim, ClampAdam) or tap_optim.arena is None or tap_optim.arena is not ar or not ar.params_in_arena():
            raise ValueError('%s needs the proposal encoder on a flat arena (tap_model.build_arena()) and a ClampAdam built with it' % name)
        if len(tap_optim.param_groups) != 1 or {id(p) for p in tap_optim.param_groups[0]['params']} != {id(p) for p in ar.params}:
            raise ValueError('the proposal encoder\'s optimiser must hold exactly its parameters in one group')
        self.fused, self.tap_model, self.tap_optim, self.tap_arena = fused, tap_model, tap_optim, ar
        self.lambda1, self.lambda2, self.tap_grad_clip = float(lambda1), float(lambda2), tap_grad_clip
        self.lib, self.dev = fused.lib, fused.dev
        self._buf_key, self._bufs = None, None

    def _new_tap_backward(self):
        """The proposal encoder's arena at the head of an iteration: no stale `.grad` view or deferred clamp survives into the new backward."""
        ar = self.tap_arena
        for p in ar.params:
            p.grad = None
        ar.deferred_clamp = None
        ar.end_backward_pass()

    def _sst_grads(self, B):
        """echr_sst_grads: the proposal encoder's gradient slots in its arena, d tap_feats and d scores from the buffers `B`."""
        ar, nps = self.tap_arena, self.tap_model.native_params()
        one = lambda i: ar.flat_g.data_ptr() + 4 * ar.offsets[ar.slot(nps[i])]
        two = lambda i, j: (L.c_f * 2)(one(i), one(j))
        return L.SstGrads(two(0, 4), two(1, 5), two(2, 6), two(3, 7), one(8), one(9), L.ptr(B['g_tap']), L.ptr(B['g_scores']), L.ptr(B['wsb']), 1)


class JointTrainStep(_JointStep):
    """The joint 'tap_cg' iteration of the reference (train.py:292-329: tap_feats, props = tap_model(c3d); cg forward; loss = lambda1 *
    tap_loss + lambda2 * cg_loss; backward; clip + step of both optimisers) around `FusedTrainStep`, without an autograd graph:

        [prepare: the caption side's tap-independent half starts]  ->  proposal encoder forward + weighted BCE (echr_sst_fwd,
        echr_tap_bce_fwd)  ->  echr_train_step(tap_grad, defer_update) -- and from INSIDE that call, right behind the work that leads to
        d loss / d tap_feats (echr_train_step_args.mid_cb): the proposal encoder's backward (echr_tap_bce_bwd, echr_sst_bwd) and its clamp +
        Adam; the caption side's parameter-gradient tail and update are forked behind it.

    Why the hook: the proposal encoder's reverse recurrence is one 64-workgroup launch that waits for d tap_feats alone.  Issued from
    Python after the call returned (torch.autograd.backward walking the SST graph) it started ~0.57 ms after d tap_feats was final, behind
    the host's issue of the caption tail; issued from the hook it starts at once and the chip-filling tail follows it instead of
    preceding it.  Same sums as loss.backward() on the joint loss: gradients of both models, both updates."""

    def __init__(self, fused, tap_model, tap_optim, lambda1=1.0, tap_grad_clip=None, early_prepare=True, order=None, lambda2=1.0):
        self._init_joint(fused, tap_model, tap_optim, lambda1, lambda2, tap_grad_clip)
        # (a direct event context 'EC' / 'EH' runs without the prepare half: the library refuses prepared = 1 there and ignores defer_update --
        # the plain form runs and the proposal encoder's backward follows the call, as with 'VH', an initial state or 'CH' rows)
        self.early = bool(early_prepare) and not fused.direct
        # 'after' (default): the proposal encoder's backward is queued when the caption call has returned -- on the caller's stream right behind
        # d tap_feats, BESIDE the caption side's tail on the library's streams; 'hook': from inside the call, the tail forked behind it
        # (serialised: measured 3.19 vs 3.00 ms per config-5 iteration)
        self.order = order or os.environ.get('ECHR_JOINT_ORDER', 'after')
        self.lam = torch.full((1,), self.lambda1, device=self.dev, dtype=torch.float32)
        # lambda2 (train.py:322-329) scales the caption term: it travels as the caption call's g_loss scalar (every caption-side gradient and
        # d tap_feats carry it) and multiplies the returned cg term; 1.0 keeps the call's own unit scalar and today's arithmetic
        self.lam2 = None if self.lambda2 == 1.0 else torch.full((1,), self.lambda2, device=self.dev, dtype=torch.float32)
        self.tap_loss = None

    def _buffers(self, T, D, H, K):
        key = (T, D, H, K)
        if self._buf_key != key:
            self.fused.join()          # (a deferred update may still read the old tap_feats)
            lib, dev, f32 = self.lib, self.dev, torch.float32
            self._bufs = dict(ws=torch.empty(lib.echr_sst_ws_floats(T, D, H, K), device=dev, dtype=f32),
                              wsb=torch.empty(lib.echr_sst_ws_bwd_floats(T, D, H, K), device=dev, dtype=f32),
                              tap=torch.empty(T, H, device=dev, dtype=f32), scores=torch.empty(T, K, device=dev, dtype=f32),
                              g_tap=torch.empty(T, H, device=dev, dtype=f32), g_scores=torch.empty(T, K, device=dev, dtype=f32),
                              loss=torch.zeros(65, device=dev, dtype=f32))
            self._buf_key = key
        return self._bufs

    def batch(self, *args, **kwargs):
        """Multi-video batches (FusedTrainStep.batch) are not part of this step yet: the proposal encoder runs over one video, and d tap_feats (tap_grad) / the deferred update are single-video forms."""
        raise NotImplementedError('JointTrainStep takes one video per call (tap_grad with defer_update / prepare are single-video forms): '
                                  'the joint iteration over a VideoBatch is fused.JointBatchStep')

    def __call__(self, c3d_feats, lda_feats, lm_labels, ind_select_list, soi_select_list, targets, masks, tap_masks, tap_labels, w1):
        """Returns (lambda1 * tap_loss + lambda2 * cg_loss) as a 0-d device tensor; `self.tap_loss` / `self.cg_loss` hold the two (unscaled) terms."""
        lib, f, tm = self.lib, self.fused, self.tap_model
        c3d = EF._f32c(c3d_feats)
        ps = [EF._f32c(p) for p in tm.native_params()]
        T, D = c3d.shape
        H, K = ps[1].shape[1], ps[8].shape[0]
        B = self._buffers(T, D, H, K)
        ar = self.tap_arena
        self._new_tap_backward()
        if self.early:          # the caption side's tap-independent half beside the proposal encoder's forward (which leaves 192 CUs idle)
            f.prepare(c3d, lda_feats, lm_labels, ind_select_list, soi_select_list, targets, masks)
        try:
            # the gradient span of the proposal encoder and d tap_feats: zero-filled HERE, off the chain that later leads to its backward
            ar.flat_g.zero_()
            B['g_tap'].zero_()
            p_drop, drop = tm._next_drop()
            sa = EF.SSTFunction._args(ps, c3d, p_drop, B['ws'], B['tap'], B['scores'])
            dc = drop.c()
            L.check(lib.echr_sst_fwd_states(C.byref(sa), C.byref(dc), L.stream_ptr()), 'sst_fwd_states')           # models/sst_model.py:31-37
            mk, lb, ww = (EF._f32c(x if x.is_cuda else x.to(self.dev)) for x in (tap_masks, tap_labels, w1))
            ww = ww.reshape(-1)

            def tap_criterion():
                # (the proposal head and its criterion, queued BEHIND the caption call: the caption side waits for tap_feats alone, and these kernels would sit between the
                # proposal encoder's forward and the event encoder on the one stream that is the iteration's critical chain there)
                L.check(lib.echr_sst_head_fwd(C.byref(sa), L.stream_ptr()), 'sst_head_fwd')                          # models/sst_model.py:38-39
                L.check(lib.echr_tap_bce_fwd_ws(L.ptr(B['scores']), L.ptr(mk), L.ptr(lb), L.ptr(ww), L.ptr(B['loss'][:1]), L.ptr(B['loss'][1:]), T, K,
                                                L.stream_ptr()), 'tap_bce_fwd')                                        # misc/utils.py:78-99

            def sst_backward():
                # d (lambda1 * tap_loss) / d scores, then the proposal encoder's backward with d loss / d tap_feats from the caption side
                tap_criterion()
                L.check(lib.echr_tap_bce_bwd(L.ptr(B['scores']), L.ptr(mk), L.ptr(lb), L.ptr(ww), L.ptr(self.lam), L.ptr(B['g_scores']), T, K,
                                             L.stream_ptr()), 'tap_bce_bwd')
                L.check(lib.echr_sst_bwd(C.byref(sa), C.byref(self._sst_grads(B)), C.byref(dc), L.stream_ptr()), 'sst_bwd')
                self.tap_optim.step_flat_raw(self.tap_grad_clip)                                                         # train.py:315-317 for tap_optimizer

            cg = f(B['tap'], c3d, lda_feats, lm_labels, ind_select_list, soi_select_list, targets, masks, tap_grad=B['g_tap'], defer_update=True,
                   prepared=self.early, mid_cb=sst_backward if self.order == 'hook' else None, g_loss=self.lam2)
        except BaseException:
            f.cancel_prepare()
            raise
        if not f.mid_called:          # the library ran the plain form (options the deferred form declines): the same work, behind the call
            sst_backward()
        self._keep = (c3d, mk, lb, ww, ps)
        self.tap_loss, self.cg_loss = B['loss'][0], cg
        if self.lam2 is not None:
            return self.lam[0] * B['loss'][0] + self.lam2[0] * cg
        return self.lam[0] * B['loss'][0] + cg


class JointBatchStep(_JointStep):
    """The joint 'tap_cg' iteration (train.py:292-329) over a multi-video batch (echr_amd.batch.VideoBatch) of V videos, without an autograd
    graph -- the batch contract of echr_amd/batch.py extended to both models:

        echr_sst_fwd_batch (tap_feats and scores of the V videos)  ->  echr_tap_bce_fwd_batch  ->  echr_train_step_batch_tap: the caption side
        as ONE call that also returns d loss / d batch.tap  ->  echr_tap_bce_bwd_batch, echr_sst_bwd_batch  ->  one clamp + Adam per model.

    loss = lambda1 * sum_v TAPModelCriterion(video v) + lambda2 * sum_v LanguageModelCriterion(video v); each video keeps its own normaliser
    (the mean over its own T_v x K, times K; sum(mask_v) + 1e-6), there is no 1/V, the gradients of both models are sums over the videos.
    One dropout counter per model and call, keyed by the batch-global element; a one-video batch computes what JointTrainStep computes.
    Nothing is deferred or hooked here (defer_update, prepare, mid_cb stay single-video forms)."""

    def __init__(self, fused, tap_model, tap_optim, lambda1=1.0, lambda2=1.0, tap_grad_clip=None):
        self._init_joint(fused, tap_model, tap_optim, lambda1, lambda2, tap_grad_clip)
        self.lam = torch.full((2,), self.lambda1, device=self.dev, dtype=torch.float32)
        self.lam[1] = self.lambda2
        self.tap_loss = self.cg_loss = self.last_tap_losses = self.last_video_losses = None
        self.last_batch = None

    def _buffers(self, T, V, D, H, K):
        key = (T, V, D, H, K)
        if self._buf_key != key:
            self.fused.join()          # (work of an earlier call may still read the old tap_feats)
            lib, dev, f32 = self.lib, self.dev, torch.float32
            self._bufs = dict(ws=torch.empty(lib.echr_sst_batch_ws_floats(T, D, H, K, V), device=dev, dtype=f32),
                              wsb=torch.empty(lib.echr_sst_batch_ws_bwd_floats(T, D, H, K, V), device=dev, dtype=f32),
                              tap=torch.empty(T, H, device=dev, dtype=f32), scores=torch.empty(T, K, device=dev, dtype=f32),
                              g_tap=torch.empty(T, H, device=dev, dtype=f32), g_scores=torch.empty(T, K, device=dev, dtype=f32),
                              loss=torch.zeros(1, device=dev, dtype=f32), tap_losses=torch.zeros(V, device=dev, dtype=f32),
                              video_losses=torch.zeros(V, device=dev, dtype=f32), part=torch.empty(64 * V, device=dev, dtype=f32))
            self._buf_key = key
        return self._bufs

    def _row_offsets(self, rows, T):
        ro = EF.sst_row_offsets(rows, T)
        return ro, self.tap_model.row_offsets_dev(ro, self.dev)

    def _sst_forward(self, c3d, rows):
        """The proposal encoder over the concatenated c3d rows into this object's buffers (echr_sst_fwd_batch; no graph): returns tap [T_tot, H]."""
        tm = self.tap_model
        if not c3d.is_cuda:
            raise L.EchrHipError('JointBatchStep runs on the GPU only')
        c3d = EF._f32c(c3d)
        ps = [EF._f32c(p) for p in tm.native_params()]
        T, D = c3d.shape
        H, K = ps[1].shape[1], ps[8].shape[0]
        if D != ps[0].shape[1]:
            raise L.EchrHipError('c3d features are %d wide, the proposal encoder reads %d' % (D, ps[0].shape[1]))
        ro, ro_dev = self._row_offsets(rows, T)
        V = len(ro) - 1
        B = self._buffers(T, V, D, H, K)
        p_drop, drop = tm._next_drop()
        sa = EF.SSTFunction._args(ps, c3d, p_drop, B['ws'], B['tap'], B['scores'])
        bx = L.SstBatch(V, L.ptr(ro_dev, torch.int32), ro.ctypes.data)
        dc = drop.c()
        L.check(self.lib.echr_sst_fwd_batch(C.byref(sa), C.byref(bx), C.byref(dc), L.stream_ptr()), 'sst_fwd_batch')
        self._sst = (sa, bx, dc, ro, ro_dev, ps, c3d, V, T, K)
        return B['tap']

    def _tap_inputs(self, x, T, K, name):
        if isinstance(x, (list, tuple)):
            x = torch.cat([torch.as_tensor(t).to(self.dev) for t in x], 0)
        x = torch.as_tensor(x)
        x = EF._f32c(x if x.is_cuda else x.to(self.dev))
        if tuple(x.shape) != (T, K):
            raise ValueError('%s must be the concatenated [T_tot, K] = [%d, %d] matrix or one [T_v, K] matrix per video (got %s)' % (name, T, K, tuple(x.shape)))
        return x

    def __call__(self, videos_or_batch, tap_masks, tap_labels, w1, step=True, handover=False, handover_cb=None, cg_done=None):
        """One iteration; returns lambda1 * tap_loss + lambda2 * cg_loss as a 0-d device tensor (no host sync).  `videos_or_batch`: the dicts
        VideoBatch.from_videos takes (no 'tap' needed), or a ready VideoBatch whose `tap` is ignored: the batch's tap_feats are the proposal
        encoder's forward of this call.  `tap_masks` / `tap_labels`: the concatenated [T_tot, K] matrices or one [T_v, K] per video; `w1`:
        one [K] weight vector for all videos, or one per video (a list, or [V, K]).  `tap_loss` / `cg_loss` hold the two sums over the videos,
        `last_tap_losses` / `last_video_losses` the per-video terms [V] (device tensors), `last_batch` the VideoBatch the call ran on.
        step=False stops after the backward passes and leaves both models' summed gradients in their arenas (`.grad` views); the proposal
        encoder's `.grad` views are set after a step as well.  `handover` / `handover_cb` (with step=False): the caption call records the
        data-parallel hand-over points of the captioner's arena (FusedTrainStep.batch_handover); `cg_done()`: called right behind the caption
        call, where the captioner's whole arena is final in stream order and the proposal encoder's backward is not yet queued."""
        from .batch import VideoBatch
        lib, f = self.lib, self.fused
        m = f.model
        # (a list of video dicts becomes a batch built for the model's clip context below; a ready batch must already be)
        m._check_batch_options(videos_or_batch if isinstance(videos_or_batch, VideoBatch) else None)
        f._begin('joint_batch_step', 'JointBatchStep')          # (a deferred single-video update may still read buffers this call rewrites)
        ar = self.tap_arena
        self._new_tap_backward()
        if isinstance(videos_or_batch, VideoBatch):
            src = videos_or_batch
            if src.labels is None:
                raise ValueError('the batch carries no labels')
            tap = self._sst_forward(src.c3d, src.row_offset)
            batch = VideoBatch(src.c3d, tap, src.lda, src.row_offset, src.event_offset, src.soi, src.ind, src.labels, src.masks,
                               clip_context_type=src.clip_context_type, CG_init_feats_type=src.CG_init_feats_type)
        else:
            batch = VideoBatch.from_videos(videos_or_batch, device=self.dev, tap_fn=self._sst_forward,
                                           clip_context_type=m.opt.clip_context_type,
                                           CG_init_feats_type=getattr(m.opt, 'CG_init_feats_type', ''))
            if batch.labels is None:
                raise ValueError('the videos carry no labels / masks')
        sa, bx, dc, ro, ro_dev, ps, c3d, V, T, K = self._sst
        B = self._bufs
        ar.flat_g.zero_()
        B['g_tap'].zero_()
        mk, lb = self._tap_inputs(tap_masks, T, K, 'tap_masks'), self._tap_inputs(tap_labels, T, K, 'tap_labels')
        if isinstance(w1, (list, tuple)):
            if len(w1) != V:
                raise ValueError('w1 must be one weight vector or one per video (%d given for %d videos)' % (len(w1), V))
            w1 = torch.stack([torch.as_tensor(t).reshape(-1).to(self.dev) for t in w1], 0)
        ww = torch.as_tensor(w1)
        ww = EF._f32c(ww if ww.is_cuda else ww.to(self.dev))
        if ww.numel() == K:
            ww, w1_ld = ww.reshape(-1), 0
        elif tuple(ww.shape) == (V, K):
            w1_ld = K
        else:
            raise ValueError('w1 must be [K] = [%d] or [V, K] = [%d, %d] (got %s)' % (K, V, K, tuple(ww.shape)))
        # proposal criterion (misc/utils.py:78-99 per video): per-video losses and their sum in one fixed order
        L.check(lib.echr_tap_bce_fwd_batch(L.ptr(B['scores']), L.ptr(mk), L.ptr(lb), L.ptr(ww), w1_ld, L.ptr(ro_dev, torch.int32), V, K,
                                           L.ptr(B['tap_losses']), L.ptr(B['loss']), L.ptr(B['part']), L.stream_ptr()), 'tap_bce_fwd_batch')
        # the caption side: forward, criterion, backward, d loss / d batch.tap, clamp + Adam -- ONE call; lambda2 travels as its g_loss scalar
        cg = f._batch_tap(batch, B['g_tap'], ro_dev, B['video_losses'], g_loss=self.lam[1:], step=step, handover=handover, handover_cb=handover_cb)
        if cg_done is not None:
            cg_done()
        # d (lambda1 * sum_v tap_loss_v) / d scores, then the proposal encoder's backward with d loss / d tap_feats from the caption side
        L.check(lib.echr_tap_bce_bwd_batch(L.ptr(B['scores']), L.ptr(mk), L.ptr(lb), L.ptr(ww), w1_ld, L.ptr(ro_dev, torch.int32), V, K, T,
                                           L.ptr(self.lam[:1]), L.ptr(B['g_scores']), L.stream_ptr()), 'tap_bce_bwd_batch')
        L.check(lib.echr_sst_bwd_batch(C.byref(sa), C.byref(bx), C.byref(self._sst_grads(B)), C.byref(dc), L.stream_ptr()), 'sst_bwd_batch')
        if step:
            self.tap_optim.step_flat_raw(self.tap_grad_clip)          # train.py:315-317 for tap_optimizer
        else:
            ar._zeroed = [(0, ar.total)]
        # the proposal encoder's summed gradient stays readable as `.grad` views of its arena, as after an autograd iteration (behind a step
        # too: the update reads the arena and leaves it as it is)
        for i, p in enumerate(ar.params):
            p.grad = ar.grad_view(i)
        self._keep = (c3d, mk, lb, ww, ps, batch)
        self.last_batch = batch
        self.tap_loss, self.cg_loss = B['loss'][0], cg
        self.last_tap_losses, self.last_video_losses = B['tap_losses'], B['video_losses']
        return self.lam[0] * B['loss'][0] + self.lam[1] * cg


class _DataParallelExchange(object):
    """What DataParallelStep and DataParallelBatchStep share: the hand-over ranges of the captioner's arena, how an early range reaches the
    collective stream (`via`), the ONE wait, the exchange instrumentation.  The collective sequencing itself is parallel.StagedExchange."""

    def _init_exchange(self, fused, group, overlap, algo, via):
        from . import parallel
        self.P, self.fused, self.group, self.overlap, self.algo = parallel, fused, group, bool(overlap), algo
        # how an early range reaches the collective stream: 'callback' (default) = queued from inside the call with the library's stream current
        # (echr_train_step_args.handover_cb), 'event' = a side stream per range that waits for the hand-over event (echr_handover_wait)
        self.via = via or os.environ.get('ECHR_DP_VIA', 'callback')
        self._ext, self._keep = {}, None
        ar, lm = fused.arena, fused.model.lm_model
        core = lm.core
        lstm = [p for k in range(3) for p in getattr(core, 'layer%d' % k).parameters()]
        self.ranges = []
        for which, params in ((0, [lm.logit.weight, lm.logit.bias]), (1, lstm)):
            slots = sorted(ar.slot(p) for p in params)
            if slots == list(range(slots[0], slots[-1] + 1)):          # one contiguous arena range (it is, for the reference's module order)
                self.ranges.append((which,) + tuple(ar.span(slots)))
        self._range = {which: (lo, hi) for which, lo, hi in self.ranges}
        self.side = [torch.cuda.Stream(device=fused.dev) for _ in self.ranges] if (self.overlap and self.via != 'callback') else []
        self.ex = parallel.StagedExchange(group, algo)
        self.n_collectives = 0
        self.n_early = 0
        # opt-in instrumentation (bench.py's exchange pass): HIP events around the caller's stream's wait for the collectives -- what of the
        # exchange the backward tail did NOT hide -- and the ranges of the last step (name, bytes, early or not)
        self.measure = False
        self.exposed_ms = []
        self.last_ranges = []

    def exchange_report(self):
        """After a measured pass (`self.measure = True`, then a device synchronisation): median / max of the time the caller's stream
        waited for the collectives per step [ms] -- the EXPOSED part of the exchange -- and the ranges of the last step."""
        ms = sorted(a.elapsed_time(b) for a, b in self.exposed_ms)
        self.exposed_ms = []
        names = {0: 'logit layer', 1: 'LSTM layers'}
        rmap = {(lo, hi): names[w] for w, (lo, hi) in self._range.items()}
        return dict(exposed_ms_median=round(ms[len(ms) // 2], 4) if ms else None, exposed_ms_max=round(ms[-1], 4) if ms else None, steps=len(ms),
                    ranges=[dict(name=r.get('name') or rmap.get((r['lo'], r['hi']), 'remainder'), bytes=r['bytes'], early=r['early'])
                            for r in self.last_ranges],
                    n_collectives=self.n_collectives, n_early=self.n_early)

    def _in_order(self):
        """True when every collective of this step ran on ONE in-order device stream (the nccl = RCCL backend: one stream per process group
        and device), so that waiting for the last one queued waits for all of them.  ECHR_DP_WAIT_ALL=1: wait for each."""
        import torch.distributed as dist
        if os.environ.get('ECHR_DP_WAIT_ALL') == '1':
            return False
        try:
            return dist.get_backend(self.group) == 'nccl'
        except Exception:
            return False

    @staticmethod
    def _active():
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized()

    def _at_handover(self, which, stream_ptr):
        # host callback from inside the one-call step, right behind the last launch that writes the range: the collective is queued with the
        # library's own stream as the CURRENT stream, so torch.distributed orders its collective stream behind exactly this point -- no side
        # stream, no further event (five or more streams on this runtime's four hardware queues share queues, and a wait queued on a shared
        # queue stalls the unrelated stream behind it: measured +0.2 ms per iteration with two side streams)
        rng = self._range.get(which)
        if rng is None:
            return
        f = self.fused
        ext = self._ext.get(stream_ptr)
        if ext is None:
            ext = self._ext[stream_ptr] = torch.cuda.ExternalStream(stream_ptr, device=f.dev)
        with torch.cuda.stream(ext):
            self.ex.reduce_early(f.arena.flat_g, rng[0], rng[1])

    def _early_by_event(self):
        """The event form (echr_handover_wait): one side stream per range."""
        f = self.fused
        for (which, lo, hi), s in zip(self.ranges, self.side):
            with torch.cuda.stream(s):
                rc = f.lib.echr_handover_wait(which, L.stream_ptr())
                if rc < 0:
                    L.check(rc, 'handover_wait')
                if rc == 0:          # (1: this configuration recorded no hand-over point -- the range joins the remainder)
                    self.ex.reduce_early(f.arena.flat_g, lo, hi)

    def _wait(self):
        """The remaining ranges are queued: the caller's stream waits ONCE, for the last collective, where one in-order stream ran them all."""
        ex = self.ex
        self.n_early, self.n_collectives, self.last_ranges = ex.n_early, ex.n_collectives, ex.ranges
        ev = None
        if self.measure:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()          # the caller's stream is behind the whole backward pass here: what follows is waiting for the wire
        ex.wait(self._in_order())
        self._keep = ex.works          # (the handles not waited for only have to stay alive until the last one is done)
        if ev is not None:
            ev[1].record()
            self.exposed_ms.append(ev)


class DataParallelStep(_DataParallelExchange):
    """One data-parallel iteration on the one-call path: the SAME host path for every world size.

    rank r:  echr_train_step(step=False, handover) on its own video  ->  SUM over ranks of the flat gradient arena  ->  clip_gradient + Adam,
    identically on every rank -- the reference's m_batch accumulation (train.py:281-283 sums the per-video gradients, :313-317 clamps the sum
    and steps once) with the m_batch videos on R ranks: SUM without 1/R, clamp AFTER the reduce.

    The exchange is staged: the backward pass inside the call hands over two contiguous arena ranges long before its last kernel -- the
    logit layer (35 % of the gradient bytes, final ~0.1 ms behind the reverse recurrence, on the library's tail stream) and the three LSTM
    layers (39 %, final behind the grouped weight-gradient product on its prepare stream).  For each, the library calls back on the host
    right behind the last launch that writes the range (echr_train_step_args.handover_cb) and the range's collective is queued with that
    library stream as the CURRENT stream (torch.distributed orders its collective stream behind the current stream), so it runs beside the
    rest of the tail and the event encoder's backward without any further stream or event (`via='event'`: the older form -- one side
    stream per range waits for the hand-over event, echr_handover_wait); the remaining ranges (event encoder + embedding, attention: 26 %)
    follow from the caller's stream, asynchronously too, and the caller's stream waits ONCE, for the last collective queued.  Every collective starts behind the reverse recurrence and is
    waited for before clamp + Adam, i.e. before the next iteration's forward recurrence: no collective kernel is ever resident beside a
    persistent pair.  `overlap=False`: ONE collective on the whole arena behind the call.  A FusedTrainStep built for 'CH' / 'CC+CH' runs
    echr_train_step_clip, which records the same two points (the clip-row gradient is no part of the arena)."""

    def __init__(self, fused, group=None, overlap=True, algo=None, via=None):
        self._init_exchange(fused, group, overlap, algo, via)

    def batch(self, *args, **kwargs):
        """Multi-video batches are not part of this step: one video per rank and call."""
        raise NotImplementedError('DataParallelStep takes one video per rank and call: a VideoBatch per rank is DataParallelBatchStep')

    def __call__(self, *args, **kw):
        f, ar = self.fused, self.fused.arena
        active = self._active()
        self.ex.begin()
        use_cb = self.overlap and active and self.via == 'callback'
        loss = f(*args, step=False, handover=self.overlap and active, handover_cb=self._at_handover if use_cb else None, **kw)
        if active:
            if self.overlap and not use_cb:
                self._early_by_event()
            # the remaining ranges, asynchronously as well: queued back to back on the collective stream behind the caller's stream's position
            # (= the end of the backward pass), waited for ONCE -- a blocking collective costs two cross-stream edges (10-20 us each on this
            # runtime) before the next one may even be queued
            self.ex.reduce_rest(ar.flat_g)
            self._wait()
        else:
            self.n_collectives = 0
        o = f.optim
        if f.grad_clip is not None:
            from .misc.utils import clip_gradient
            clip_gradient(o, f.grad_clip)          # (recorded; the clamp itself is fused into the step kernel)
        o.step()
        return loss


class DataParallelBatchStep(_DataParallelExchange):
    """One data-parallel iteration over multi-video batches: the batch steps times DataParallelStep.  `inner` is a FusedTrainStep (run
    through its batch form), a JointBatchStep or a SelfCriticalBatchStep.

    rank r:  the inner step on the rank's own VideoBatch -- its shard of the update's m_batch videos (parallel.shard_batch) -- with step=False
    and the hand-over points recorded  ->  SUM over ranks of every flat arena the step filled  ->  ONE clamp + Adam per model
    (ClampAdam.step_flat_raw), identically on every rank.  The reference's m_batch protocol (train.py:281-283,313-317) with the videos on R
    ranks: loss and gradients are the SUM over all videos of all ranks, no 1/R and no 1/V, every video with its own criterion normaliser,
    the clamp AFTER the reduce.

    The captioner's arena goes staged exactly as DataParallelStep's (the shared parallel.StagedExchange: the logit-layer and LSTM-layer
    ranges from the hand-over callback, or `via='event'`; the remainder behind the call; `overlap=False`: one collective).  With a
    JointBatchStep the remainder is queued right behind the caption call and the proposal encoder's arena follows as one more collective
    behind echr_sst_bwd_batch.  One wait for the last collective where one in-order stream runs them all (RCCL).

    A rank whose shard is empty passes None: it zero-fills its arena(s), runs no library step and queues the same collectives in the same
    order from the caller's stream.  Which early ranges exist is the library's to say (a configuration may record neither point, or one),
    and an empty rank cannot see it, so the ranks AGREE once: the first call of every rank records which points fired without queueing
    from them, one two-element MIN collective (its result read on the host: the one synchronisation, of the first call only) settles the
    set, and that call's early ranges go out behind it from the caller's stream.  From then on working ranks queue exactly the agreed
    points from the hand-over callback (or event), empty ranks the same ranges in the same order -- LSTM layers, then logit layer from
    the callback; logit, LSTM in the event form -- and a point outside the set joins the remainder on every rank.  A rank whose later
    call misses an agreed point raises instead of queueing a different sequence.  Replicas never diverge, no rank blocks.

    The call returns the rank-local summed loss as a 0-d device tensor (no host sync; 0 for an empty shard).  `reduce_loss=True`: the SUM
    over ranks instead, from one further one-element collective; with `n_videos` (the update's global video count, sharded round-robin)
    that collective also carries the per-video losses and `last_video_losses` holds the global batch's in rank-major shard order
    (parallel.shard_order, parallel.loss_slots).  Dropout: the rank is mixed into the model's seed (OldModel.next_drop_state);
    set_dropout_state pins it."""

    def __init__(self, inner, group=None, overlap=True, algo=None, via=None, reduce_loss=False):
        if isinstance(inner, FusedTrainStep):
            kind, fused = 'caption', inner
        elif isinstance(inner, JointBatchStep):
            kind, fused = 'joint', inner.fused
        elif isinstance(inner, SelfCriticalBatchStep):
            kind, fused = 'scst', inner.fused
        else:
            raise TypeError('DataParallelBatchStep wraps a FusedTrainStep, a JointBatchStep or a SelfCriticalBatchStep')
        self.inner, self.kind = inner, kind
        self._init_exchange(fused, group, overlap, algo, via)
        self.reduce_loss = bool(reduce_loss)
        self.last_video_losses = self.last_result = None
        self._zero = torch.zeros(1, device=fused.dev, dtype=torch.float32)
        self.points = None          # the hand-over points the ranks agreed on (a tuple in queueing order), None before the first call
        self._fired = set()

    def _order(self, points):
        return tuple(w for w in ((1, 0) if self.via == 'callback' else (0, 1)) if w in points and w in self._range)

    def _at_handover(self, which, stream_ptr):
        self._fired.add(which)
        if self.points is not None and which in self.points:
            _DataParallelExchange._at_handover(self, which, stream_ptr)

    def _captioner_exchange(self, empty):
        """Behind the caption call (an empty rank: behind its zero fill), on the caller's stream: the captioner's arena is final in stream
        order.  First call: the agreement, then its early ranges from here; later calls: the empty rank's early ranges, the event form's
        waits; then the remainder."""
        import torch.distributed as dist
        f, ex = self.fused, self.ex
        flat = f.arena.flat_g
        if self.overlap and self.points is None:
            if empty:
                have = [1, 1]
            elif self.via == 'callback':
                have = [int(w in self._fired) for w in (0, 1)]
            else:
                have = []
                for w in (0, 1):
                    rc = f.lib.echr_handover_wait(w, L.stream_ptr())
                    if rc < 0:
                        L.check(rc, 'handover_wait')
                    have.append(int(rc == 0))
            mask = torch.tensor(have, device=f.dev, dtype=torch.int32)
            dist.all_reduce(mask, op=dist.ReduceOp.MIN, group=self.group)
            self.points = self._order({w for w, ok in enumerate(mask.tolist()) if ok})
            for w in self.points:
                ex.reduce_early(flat, *self._range[w])
        elif self.overlap and empty:
            for w in self.points:
                ex.reduce_early(flat, *self._range[w])
        elif self.overlap:
            if self.via != 'callback':
                for (which, lo, hi), s in zip(self.ranges, self.side):
                    if which in self.points:
                        with torch.cuda.stream(s):
                            rc = f.lib.echr_handover_wait(which, L.stream_ptr())
                            if rc < 0:
                                L.check(rc, 'handover_wait')
                            if rc == 0:
                                self._fired.add(which)
                                ex.reduce_early(flat, lo, hi)
            missing = [w for w in self.points if w not in self._fired]
            if missing:
                raise RuntimeError('this rank\'s call recorded no hand-over point %s, which the ranks agreed on at their first call: every rank '
                                   'must keep the configuration it started with (its collectives would no longer match the other ranks\')' % missing)
        ex.reduce_rest(flat)

    def __call__(self, batch, *args, n_videos=None, **kw):
        """`batch`: the rank's VideoBatch (JointBatchStep: or its list of video dicts), None for an empty shard; further arguments are the
        inner step's (JointBatchStep: tap_masks, tap_labels, w1; SelfCriticalBatchStep: gen_result=, reward=).  Returns the loss; a
        SelfCriticalBatchStep's other results are kept in `last_result`."""
        import torch.distributed as dist
        f, inner = self.fused, self.inner
        active = self._active()
        ex = self.ex.begin()
        ho = self.overlap and active
        cb = self._at_handover if (ho and self.via == 'callback') else None
        empty = batch is None or (isinstance(batch, (list, tuple)) and len(batch) == 0)
        self._fired = set()
        self.last_result = None
        cg_done = (lambda: self._captioner_exchange(empty)) if active else None
        if empty:
            f._begin('data_parallel_batch_step', True)
            f.arena.zero_as_final()
            if self.kind == 'joint':
                inner.tap_arena.zero_as_final()
            loss, losses = self._zero[0], None
        elif self.kind == 'caption':
            loss = f.batch_handover(batch, cb, **kw) if ho else f.batch(batch, step=False, **kw)
            losses = f.last_video_losses
        elif self.kind == 'scst':
            out = inner.handover(batch, cb, *args, **kw) if ho else inner(batch, *args, step=False, **kw)
            loss, self.last_result = out[0], out[1:]
            losses = inner.last_video_losses
        else:
            loss = inner(batch, *args, step=False, handover=ho, handover_cb=cb, cg_done=cg_done, **kw)
            losses = inner.lam[0] * inner.last_tap_losses + inner.lam[1] * inner.last_video_losses
        if cg_done is not None and (empty or self.kind != 'joint'):
            cg_done()
        if active:
            if self.kind == 'joint':          # the proposal encoder's arena: one more collective, behind echr_sst_bwd_batch
                ex.reduce_rest(inner.tap_arena.flat_g)
                ex.ranges[-1]['name'] = 'proposal encoder'
            if self.reduce_loss:
                # the loss (and, with n_videos, the per-video losses at their rank-major slots: every other rank adds zeros there) as ONE
                # further collective; no host sync -- the slots are device copies
                n, lo = self.P.loss_slots(n_videos, dist.get_rank(self.group), dist.get_world_size(self.group), 0 if losses is None else len(losses))
                buf = torch.zeros(n, device=f.dev, dtype=torch.float32)
                buf[0] = loss
                if n > 1 and losses is not None:
                    buf[lo:lo + len(losses)] = losses
                ex.reduce_rest(buf)
                ex.ranges[-1]['name'] = 'loss'
                loss = buf[0]
                self.last_video_losses = buf[1:] if n > 1 else losses
            else:
                self.last_video_losses = losses
            self._wait()
        else:
            self.n_collectives = self.n_early = 0
            self.last_video_losses = losses
        L.check(f.lib.echr_check_async(), 'data_parallel_batch_step')
        f.optim.step_flat_raw(f.grad_clip)
        f.arena._zeroed = []          # (as behind the one-call step's own update: the arena holds the reduced gradient, not zeros)
        if self.kind == 'joint':
            inner.tap_optim.step_flat_raw(inner.tap_grad_clip)
            inner.tap_arena._zeroed = []
        return loss

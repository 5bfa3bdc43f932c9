"""CaptionGenerator -- drop-in for the reference's CaptionGenerator.py (:7-167) on MI355X.

Same constructor side effects on `opt` (video/event/clip_context_dim, :56-84), same `forward`
signature and live modes ('train' -> log-probs [N,S,V+1]; 'eval' -> (seq, logp); 'train_rl' -> (gen_result, sample_logprobs,
greedy_res), self-critical training), same sub-module
names (`fusion_model`, `lm_model`) and state_dict keys (event_context_type 'EC' / 'EH' builds no
`fusion_model`, as in the reference).  The three context levels are built without
python loops over events: index lists are uploaded once as int32 (start, length, anchor) vectors and
every kernel addresses the video features through them.
"""
import os

import numpy as np
import torch
from torch import nn

from . import functional as EF
from . import models
from .models.OldModel_NEW import ClipView, caption_labels


class CaptionGenerator(nn.Module):
    # event_context_type (CaptionGenerator.py:106-137), exact values: through the TSRM event encoder -> which of (pooled C3D rows, anchor state)
    # it reads; EVENT_DIRECT: the same pieces AS the event vector, no encoder (the "captioner without event relations" ablation)
    EVENT_ENCODED = {'ER1': 1, 'ER2': 2, 'ER3': 3}
    EVENT_DIRECT = {'EC': 1, 'EH': 2}

    def __init__(self, opt):
        super(CaptionGenerator, self).__init__()
        self.opt = opt
        et = opt.event_context_type
        if et not in self.EVENT_ENCODED and et not in self.EVENT_DIRECT:
            raise NotImplementedError("event_context_type=%r: the live values are ER1 / ER2 / ER3 (through the TSRM event encoder) and EC / EH (the "
                                      "event vector itself, no encoder).  The reference runs no other: 'EC' and 'EH' together ('ECEH', 'EC+EH') fail in "
                                      "get_event_context, where torch.cat(event_feats, 0) joins a video_dim-wide and a hidden_dim-wide tensor along dim 0 "
                                      "(CaptionGenerator.py:132-133), and a value with neither ('') returns None (:134-135), which the decoder's "
                                      "torch.cat((xt, None)) refuses" % (et,))
        self.change_context_dim()
        if 'TSRM' in opt.fusion_model and et in self.EVENT_ENCODED:          # ('EC' / 'EH': no fusion_model attribute, no fusion_model.* keys)
            self.fusion_model = models.setup_fusion(opt)
        self.lm_model = models.setup_lm(opt)
        self.overlap_encoder = os.environ.get('ECHR_OVERLAP_ENCODER', '1') != '0'        # 'train' mode: run the decoder's event-independent precompute concurrently with the event encoder
        if not any(k in opt.video_context_type for k in ('VL', 'VC', 'VH')) or not self.clip_parts():
            raise NotImplementedError('the HIP path implements the ECHR recipe: video_context_type from VL / VC / VH (any combination), '
                                      'event_context_type ER1 / ER2 / ER3 / EC / EH, clip_context_type CC / CH / CC+CH (experiments/train_ECHR.sh, opts.py:130)')
        if self.clip_parts() & 2 and 'C' in opt.CG_init_feats_type:
            raise NotImplementedError("clip_context_type with 'CH' and a CG_init_feats_type that reads the clip: the initial state's clip mean has "
                                      "no gradient into tap_feats on the HIP path")

    def clip_parts(self):
        """Frame-level context rows as the reference tests them (`in`, CaptionGenerator.py:140-167): 1 = 'CC' (C3D rows), 2 = 'CH' (the
        proposal encoder's states), 3 = both, C3D first ('CC+CH', also spelt 'CCCH'); 0 = neither."""
        ct = self.opt.clip_context_type
        return (1 if 'CC' in ct else 0) | (2 if 'CH' in ct else 0)

    def event_direct(self):
        """0: the event context goes through the event encoder ('ER1' / 'ER2' / 'ER3'); 1 = 'EC' (the mean of the event's C3D rows), 2 = 'EH' (the
        proposal encoder's state at the event's anchor): the event vector itself, no `fusion_model` (echr_train_step_args.event_direct)."""
        return self.EVENT_DIRECT.get(self.opt.event_context_type, 0)

    def encoder_dropout_p(self):
        """The dropout probability of the event encoder's one site; 0.0 without an encoder ('EC' / 'EH': no site is drawn)."""
        return self.fusion_model.enc_attn.dropout.p if hasattr(self, 'fusion_model') else 0.0

    def one_stream(self):
        """True with caption_model='show_attend_tell' (models.ShowAttendTellModel): the one-stream decoder of echr_amd.sat."""
        return type(self.lm_model).__name__ == 'ShowAttendTellModel'

    def _require_live_decoder(self):
        """The configuration check of forward(), ahead of every argument: the one-stream decoder runs with one LSTM layer, a non-empty
        CG_input_feats_type and 'CC' rows (ShowAttendTellModel._require_live names the option otherwise)."""
        if self.one_stream():
            self.lm_model._require_live()
            if self.clip_parts() & 2:
                self.lm_model._refuse("clip_context_type=%r -- the one-stream decoder attends over the C3D rows ('CC'); 'CH' rows (the gradient into "
                                      "tap_feats through the clip context) are a follow-up" % (self.opt.clip_context_type,))

    def _require_three_stream(self, what):
        """Entries that only the three-stream decoder has (beam search, self-critical training, the fused steps)."""
        if self.one_stream():
            self.lm_model._refuse("%s runs on the three_stream decoder; the one-stream decoder runs forward(mode='train' / 'eval') and "
                                  "forward_batch(mode='train' / 'eval')" % what)

    def _check_batch_decoder(self, batch, what):
        """A batch is built for one decoder (VideoBatch(..., caption_model=)): a one-stream model refuses a plain (or missing) batch with a
        NotImplementedError that names the keyword, a three-stream model refuses a one-stream batch with a ValueError."""
        built = bool(getattr(batch, 'one_stream', False))
        if self.one_stream() and not built:
            self.lm_model._refuse("%s takes a batch built for this decoder -- VideoBatch.from_videos(..., caption_model='show_attend_tell'): a "
                                  "plain batch is the three_stream decoder's" % what)
        if built and not self.one_stream():
            raise ValueError("the batch was built for caption_model='show_attend_tell', the model has %r" % (self.opt.caption_model,))

    def build_arena(self):
        """Pack parameters and gradients into flat device buffers (echr_amd/arena.py).  Call after .cuda(); enables the
        single-launch fused optimiser step and the single-bucket gradient all-reduce."""
        from .arena import ParamArena
        arena = ParamArena(self)
        self.lm_model._echr_arena_ref = arena
        if hasattr(self, 'fusion_model'):
            self.fusion_model._echr_arena_ref = arena
        return arena

    def set_dropout_state(self, seed, calls=0):
        """Pin the counter-based dropout stream (tests / reproducible runs)."""
        self.lm_model._drop_seed = int(seed)
        self.lm_model._drop_calls = int(calls)

    def forward(self, tap_feats, c3d_feats, lda_feats, lm_labels, ind_select_list, soi_select_list, mode='train', gen_result=None,
                beam_size=1, return_score=False):
        """`gen_result` (mode='train_rl' only, optional): score these captions [N,T] instead of drawing them (tests, replayed samples).
        `beam_size` (mode='eval' only): > 1 decodes by beam search (OldModel.sample with opt beam_size); `return_score` (with beam_size > 1)
        appends each caption's score, the sum of its token log-probs (<eos> included)."""
        if mode not in ('train', 'eval', 'train_rl'):
            raise NotImplementedError("mode=%r: 'train', 'eval' and 'train_rl' are the reference's live modes (SURVEY section 2 row 12)" % (mode,))
        if gen_result is not None and mode != 'train_rl':
            raise ValueError("gen_result is taken by mode='train_rl' only")
        if beam_size != 1 and mode != 'eval':
            raise ValueError("beam_size is taken by mode='eval' only")
        if return_score and (mode != 'eval' or beam_size == 1):
            raise ValueError("return_score is taken by mode='eval' with beam_size > 1 only")
        self._require_live_decoder()
        if mode == 'train_rl':
            self._require_three_stream("mode='train_rl' (self-critical training)")
        if beam_size != 1:
            self._require_three_stream('beam_size=%r (beam search)' % (beam_size,))
        if self.one_stream() and self.lm_model.training and self.lm_model.ss_prob > 0.0:
            self.lm_model._refuse('ss_prob > 0 -- scheduled sampling is never enabled by the reference and is not on the HIP path')
        if not c3d_feats.is_cuda:
            raise EF.L.EchrHipError('CaptionGenerator runs on the GPU only: move the module and its inputs with .cuda()')
        ev = EF.event_index_tensors(soi_select_list, ind_select_list, c3d_feats.device, min(c3d_feats.shape[0], tap_feats.shape[0]))
        drop = self.lm_model.next_drop_state(self.encoder_dropout_p())
        drop.training = self.training
        video = self.get_video_context(tap_feats, c3d_feats, lda_feats, ind_select_list, soi_select_list)
        clip, clip_mask = self.get_clip_context(tap_feats, c3d_feats, lda_feats, ind_select_list, soi_select_list, _ev=ev)
        prepared = None
        if mode == 'train' and self.overlap_encoder and not self.one_stream():
            # the decoder's event-independent precompute starts on a second stream and overlaps the event encoder launched next
            prepared = self.lm_model.prepare(video, clip, clip_mask, lm_labels)
        try:
            event = self.get_event_context(tap_feats, c3d_feats, lda_feats, ind_select_list, soi_select_list, _ev=ev, _drop=drop)
        except Exception:
            if prepared is not None:
                EF.decoder_prepare_cancel()      # the second stream still writes the handle's buffers: order them before they are freed
            raise
        if mode == 'train':
            return self.lm_model(video, event, clip, clip_mask, lm_labels, drop=drop, prepared=prepared)
        if mode == 'train_rl':
            return self._train_rl(video, event, clip, clip_mask, drop, gen_result)
        if beam_size != 1:
            return self.lm_model.sample(video, event, clip, clip_mask, {'beam_size': beam_size, 'return_score': return_score})
        return self.lm_model.sample(video, event, clip, clip_mask)

    def forward_batch(self, batch, mode='train', beam_size=1, event_group_rows=None):
        """`forward` over a multi-video batch (echr_amd.batch.VideoBatch): mode='train' returns the log-probs [N_tot, S, V+1] of all events
        (rows of video v: batch.event_slices[v]; S = the widest video's step count) with the usual autograd edges -- parameters, and
        batch.tap through 'ER2' / 'ER3' and 'VH'; mode='eval' returns the greedy (seq, logp) of all rows.  Rows of video v equal what
        forward() returns for that video alone; apply the criterion with `batch.criterion(crit, logp)` (per-video normalisers, summed).
        One dropout counter per call, every site keyed by the batch-global element index.
        `event_group_rows` (mode='eval' only; None = one block-diagonal call over all N_tot events): an integer G runs the event encoder once per
        run of `batch.event_groups(G)` -- consecutive videos with at most G events together -- so that the pair work and the workspace are bounded
        by G * N_tot instead of N_tot^2; a run of one video takes the single-video encoder with that video's own inference bounds (the tabulated
        pair MLP of large inference calls).  The greedy decode stays ONE call over all rows.  The training backward is not grouped.
        With event_context_type 'EC' / 'EH' there is no event encoder: `event_group_rows` is accepted and has no effect (it only bounds the
        encoder's pair work), here and in beam_batch.
        `beam_size` stays 1 here: beam search over a batch is `beam_batch`.
        With caption_model='show_attend_tell' the batch must have been built for the one-stream decoder (VideoBatch.from_videos(...,
        caption_model='show_attend_tell')): both modes then run echr_amd.sat's batched entries (SatBatchFunction, sat_greedy_sample(vid=))
        with the same contexts, edges and `event_group_rows`; beam_batch, train_rl_batch and the fused steps stay the three-stream decoder's."""
        self._check_batch_decoder(batch, 'forward_batch (a multi-video batch)')
        if mode == 'train_rl':
            raise NotImplementedError("mode='train_rl' takes one video per call: self-critical training over a batch is "
                                      "train_rl_batch(batch) (one call: fused.SelfCriticalBatchStep)")
        if mode not in ('train', 'eval'):
            raise NotImplementedError("mode=%r: batches run 'train' and 'eval'" % (mode,))
        if beam_size != 1:
            raise NotImplementedError('beam search over a batch is beam_batch(batch, beam_size) (eval_utils.caption_videos_beam): forward_batch '
                                      'decodes greedily')
        if event_group_rows is not None and mode != 'eval':
            raise ValueError("event_group_rows is taken by mode='eval' only")
        groups = batch.event_groups(event_group_rows) if event_group_rows is not None else None
        video, event, ev_start, ev_len, A, vid, drop = self._batch_contexts(batch, groups, need_labels=mode == 'train')
        lm = self.lm_model
        disjoint = EF.rows_disjoint(batch.soi)
        if mode == 'eval':
            with torch.no_grad():
                if self.one_stream():
                    from . import sat
                    return sat.sat_greedy_sample(video, event, batch.c3d, ev_start, ev_len, A, lm.seq_length, lm.native_params(), lm._require_live(),
                                                 h0=self._batch_initial_state(batch, video, event, ev_start, ev_len, vid),
                                                 vid=sat.BatchVid(batch.vid, batch.n_videos, dev=vid))
                return EF.greedy_sample(video, event, batch.clip_rows(), ev_start, ev_len, A, lm.seq_length, lm.native_params(),
                                        table_cache=lm.sample_tables(), vid=vid,
                                        h0=self._batch_initial_state(batch, video, event, ev_start, ev_len, vid))
        if lm.training and lm.ss_prob > 0.0:
            raise NotImplementedError('scheduled sampling (ss_prob > 0) is never enabled by the reference and is not on the HIP path')
        tokens = lm._tokens(batch.labels, batch.device)
        h0 = self._batch_initial_state(batch, video, event, ev_start, ev_len, vid)
        return self._batch_decoder(batch, video, event, ev_start, ev_len, tokens, A, disjoint, drop, h0, vid)

    def _batch_decoder(self, batch, video, event, ev_start, ev_len, tokens, A, disjoint, drop, h0, vid):
        """The teacher-forced log-probs of a batch (functional.DecoderFunction with vid).  With 'CH' / 'CC+CH' rows it takes batch.tap and its
        first column in the row source: the row source carries no graph, the decoder's backward returns d tap itself (as ClipView.grad_src /
        grad_col0 arrange for one video)."""
        ps = self.lm_model.native_params()
        if self.one_stream():          # (sat.SatBatchFunction: 'CC' rows only, the batch was refused otherwise when it was built)
            from . import sat
            return sat.SatBatchFunction.apply(video, event, batch.c3d, ev_start, ev_len, tokens, A, disjoint, drop, self.lm_model._grad_sink(ps),
                                              h0, self.lm_model._require_live(), sat.BatchVid(batch.vid, batch.n_videos, dev=vid), *ps)
        return EF.DecoderFunction.apply(video, event, batch.clip_rows(), ev_start, ev_len, tokens, A, disjoint, drop, self.lm_model._grad_sink(ps),
                                        None, h0, batch.tap if batch.clip_parts > 1 else None, int(batch.clip_col0), vid, *ps)

    def _batch_initial_state(self, batch, video, event, ev_start, ev_len, vid):
        """None (the recipe: zero state) or h0 [N_tot, 3H] ([N_tot, H] for the one-stream decoder) of CG_init_feats_type over a batch (functional.InitState with vid): every event from
        its own video's scene vector, its event context and its clip mean over its own video's padded clip length.  The clip mean reads
        C3D rows only (the constructor refuses 'C' with 'CH' rows)."""
        lm = self.lm_model
        if not getattr(lm, 'CG_init_feats_dim', 0):
            return None
        t = lm.CG_init_feats_type
        w, b = lm.init_linear.weight, lm.init_linear.bias
        return EF.InitState.apply(video, event, batch.clip_rows(), ev_start, ev_len, 0, vid, ('V' in t, 'E' in t, 'C' in t), lm._grad_sink((w, b)), w, b)

    def _batch_contexts(self, batch, groups, need_labels=False):
        """What forward_batch and beam_batch hand to the decoder: the checks of a batched call, then (video [V, Dv], event [N_tot, d_o],
        ev_start, ev_len, A, vid, drop) -- the scene vectors, and the event encoder as one block-diagonal call or once per run of `groups`."""
        self._check_batch_decoder(batch, 'a multi-video batch (VideoBatch)')
        self._check_batch_options(batch)
        self._require_live_decoder()
        if not batch.c3d.is_cuda:
            raise EF.L.EchrHipError('CaptionGenerator runs on the GPU only: build the batch on the device (VideoBatch.from_videos(..., device=))')
        if need_labels and batch.labels is None:
            raise ValueError("mode='train' needs a batch with labels")
        ev_start, ev_len, ind, A = EF.event_index_tensors(batch.soi, batch.ind, batch.device, batch.c3d.shape[0])
        vid = batch.dev('vid')
        lm = self.lm_model
        drop = lm.next_drop_state(self.encoder_dropout_p())
        drop.training = self.training
        video = self.get_video_context_batch(batch)
        if self.event_direct():
            # 'EC' / 'EH': ev_start / ind are batch-absolute, so the pooled rows / the anchors' states of all videos ARE the event vectors;
            # there is no pair work for `groups` to bound
            event = EF.EventPoolGather.apply(batch.c3d, batch.tap, ev_start, ev_len, ind, self.event_direct())
            return video, event, ev_start, ev_len, A, vid, drop
        fm = self.fusion_model
        parts = self.EVENT_ENCODED[self.opt.event_context_type]
        ech = EF.EventPoolGather.apply(batch.c3d, batch.tap, ev_start, ev_len, ind, parts)
        params = fm.native_params()
        infer = not (torch.is_grad_enabled() and (ech.requires_grad or any(p.requires_grad for p in params)))
        if groups is not None:
            event = self._event_context_groups(batch, groups, ech, ev_start, ev_len, vid, drop, params)
        else:
            # (index bounds 0, 0: the tabulated pair MLP of large inference calls is keyed by one video's bounds)
            event = EF.TSRMBatchFunction.apply(ech, ev_start, ev_len, vid, batch.n_videos, fm.enc_attn.group, drop, fm._grad_sink(),
                                               (1 if infer else 0, 0, 0, fm.fst_mode()), *params)
        return video, event, ev_start, ev_len, A, vid, drop

    def beam_batch(self, batch, beam_size, event_group_rows=None, max_rows=8192):
        """Beam search (forward(mode='eval', beam_size=, return_score=True)) over a multi-video batch, eval mode only.  Returns (seq int64
        [N_tot, T], logp fp32 [N_tot, T], score fp32 [N_tot], video_words host int64 [V]): video_words[v] is the width video v's decode has
        alone -- its rows batch.event_slices[v], cut to that many columns, are what the single-video call returns for it (an all-zero
        video_words[v] is that call's ([], [])) -- and T = max(video_words); seq and logp are [] when T == 0.
        The contexts are forward_batch(mode='eval')'s, `event_group_rows` included.
        `max_rows`: the decode keeps seq_length + 1 states of every one of its events * beam_size rows, so it runs once per run of
        `batch.beam_groups(beam_size, max_rows)` -- consecutive videos with at most max_rows rows together; a video above the budget runs
        alone, None is one decode over the batch.  Each run is one echr_decoder_beam_batch call and one host read (its video_words)."""
        self._require_three_stream('beam_batch (beam search over a multi-video batch)')
        B = EF._check_beam_size(beam_size, self.lm_model.vocab_size + 1)
        if self.training or self.lm_model.training:
            raise ValueError('beam search is an evaluation decode: call eval() first')
        groups = batch.event_groups(event_group_rows) if event_group_rows is not None else None
        runs = batch.beam_groups(B, max_rows)
        with torch.no_grad():
            video, event, ev_start, ev_len, A, vid, _ = self._batch_contexts(batch, groups)
            lm = self.lm_model
            L, N, ro = lm.seq_length, batch.n_events, batch.row_offset
            rows = batch.clip_rows()
            h0 = self._batch_initial_state(batch, video, event, ev_start, ev_len, vid)          # (run-local rows below: the plain row slice)
            if len(runs) == 1:
                seq, logp, score, video_words = EF.beam_search_batch(video, event, rows, ev_start, ev_len, vid, A, L, lm.native_params(), B,
                                                                     trim=False, h0=h0)
            else:
                seq = torch.empty(N, L, device=batch.device, dtype=torch.int64)
                logp = torch.empty(N, L, device=batch.device, dtype=torch.float32)
                score = torch.empty(N, device=batch.device, dtype=torch.float32)
                video_words = np.zeros(batch.n_videos, np.int64)
                for v0, v1, e0, e1 in runs:          # run-local rows: the run's own feature rows, scene vectors and video numbers
                    r0, r1 = int(ro[v0]), int(ro[v1])
                    seq[e0:e1], logp[e0:e1], score[e0:e1], video_words[v0:v1] = EF.beam_search_batch(
                        video[v0:v1], event[e0:e1], rows[r0:r1], ev_start[e0:e1] - r0, ev_len[e0:e1], vid[e0:e1] - v0, A, L,
                        lm.native_params(), B, trim=False, h0=None if h0 is None else h0[e0:e1])
        T = int(video_words.max())
        if T == 0:
            return [], [], score, video_words
        return seq[:, :T].contiguous(), logp[:, :T].contiguous(), score, video_words

    def train_rl_batch(self, batch, gen_result=None, seed=None):
        """Self-critical training (forward(mode='train_rl'), CaptionGenerator.py:32-37) over a multi-video batch: the reference's m_batch = V
        protocol in one pass.  One training-mode event context under the call's dropout state; the multinomial decode of all N_tot rows with
        the decoder's dropout active under that state (echr_decoder_sample_train_batch; draws keyed by `seed`, default the model's next
        sample seed); the greedy baseline in eval mode without a graph; then the teacher-forced recompute on [0 | gen | 0] under the SAME
        state, gathered at the tokens, with the autograd edges of forward_batch('train').
        Returns (gen_result int64 [N_tot, T], sample_logprobs [N_tot, T], greedy_res, video_words host int64 [V]): video_words[v] is the
        width video v's own call cuts its sample at and T = max(video_words) -- rows batch.event_slices[v] cut to video_words[v] columns
        are what forward(mode='train_rl') returns for that video.  Apply the criterion with `batch.reward_criterion(crit, sample_logprobs,
        gen_result, reward, video_words)`.  gen_result and sample_logprobs are [] when T == 0.
        `gen_result` [N_tot, >= T]: score these captions instead of drawing them.  The batch need not carry labels."""
        self._require_three_stream('train_rl_batch (self-critical training over a multi-video batch)')
        video, event, ev_start, ev_len, A, vid, drop = self._batch_contexts(batch, None)
        lm = self.lm_model
        if lm.training and lm.ss_prob > 0.0:
            raise NotImplementedError('scheduled sampling (ss_prob > 0) is never enabled by the reference and is not on the HIP path')
        # (the initial state once, with its graph: the two decodes read its values, the teacher-forced recompute carries the gradient)
        h0 = self._batch_initial_state(batch, video, event, ev_start, ev_len, vid)
        rows, ps = batch.clip_rows(), lm.native_params()

        def sample(ev, h0_d):
            gen, _, video_words = EF.sample_train_batch(video, ev, rows, ev_start, ev_len, vid, A, lm.seq_length, ps, drop,
                                                        seed=lm._sample_seed() if seed is None else int(seed), h0=h0_d)
            return gen, video_words
        greedy = lambda ev, h0_d: EF.greedy_sample(video, ev, rows, ev_start, ev_len, A, lm.seq_length, ps, table_cache=lm.sample_tables(), vid=vid,
                                                   h0=h0_d)[0]
        logprobs = lambda gen: self._batch_decoder(batch, video, event, ev_start, ev_len, lm._tokens(caption_labels(gen), batch.device), A,
                                                   EF.rows_disjoint(batch.soi), drop, h0, vid)
        return self._self_critical(event, h0, gen_result, sample, greedy, logprobs, batch.caption_widths)

    def _self_critical(self, event, h0, gen_result, sample, greedy, logprobs, widths=None):
        """The one body of forward(mode='train_rl') and train_rl_batch.  `event` (and `h0`, or None) carry their graphs; the two decodes read
        their values only: `sample(event, h0)` -> (gen or [], video_words or None) and `greedy(event, h0)` -> greedy_res get them detached
        and run without a graph.  `gen_result` pins the sample instead (`widths(gen_result)`: its video_words, the batched form's cut).
        `logprobs(gen)`: the teacher-forced log-probs of [0 | gen | 0] under the call's dropout state WITH the graph; they are gathered at
        the tokens here.  Returns (gen, sample_logprobs, greedy_res), then video_words if there are any."""
        ev_d, h0_d = event.detach(), None if h0 is None else h0.detach()
        with torch.no_grad():
            if gen_result is None:
                gen, video_words = sample(ev_d, h0_d)
            else:
                video_words = None if widths is None else widths(gen_result)
                gen = torch.as_tensor(gen_result)
                gen = (gen if widths is None else gen[:, :int(video_words.max())]).to(device=event.device, dtype=torch.int64).contiguous()
            greedy_res = greedy(ev_d, h0_d)
        tail = () if video_words is None else (video_words,)
        if isinstance(gen, list) or gen.numel() == 0:
            return ([], [], greedy_res) + tail          # every row drew <eos> first (OldModel.sample returns [] then, :186-187)
        return (gen, EF.GatherTokens.apply(logprobs(gen), gen), greedy_res) + tail

    def _event_context_groups(self, batch, groups, ech, ev_start, ev_len, vid, drop, params):
        """The event encoder of an inference batch, one call per run of videos (VideoBatch.event_groups), into one [N_tot, d_o] matrix.  The
        kernels compare `vid` for equality only and the pair geometry reads differences of the intervals, so a run is the plain row slice of
        the batch's tensors (its first vid need not be 0, its rows stay batch-absolute)."""
        fm = self.fusion_model
        lens = batch.soi[:, 1] - batch.soi[:, 0]
        c2 = 2 * batch.soi[:, 0] + lens
        with torch.no_grad():
            event = torch.empty(batch.n_events, fm.output_dim, device=batch.device, dtype=torch.float32)
            for v0, v1, e0, e1 in groups:
                s = slice(e0, e1)
                if v1 - v0 == 1:
                    bounds = (1, int(lens[s].max()), int(c2[s].max() - c2[s].min()), fm.fst_mode())
                    event[s] = EF.TSRMFunction.apply(ech[s], ev_start[s], ev_len[s], fm.enc_attn.group, drop, None, bounds, *params)
                else:
                    event[s] = EF.TSRMBatchFunction.apply(ech[s], ev_start[s], ev_len[s], vid[s], v1 - v0, fm.enc_attn.group, drop, None,
                                                          (1, 0, 0, fm.fst_mode()), *params)
        return event

    def _check_batch_options(self, batch=None):
        """The batch must have been built for the model's initial decoder state and frame-level context (VideoBatch.from_videos(...,
        CG_init_feats_type=, clip_context_type=)): a plain batch with a model that has either raises NotImplementedError and names the
        keyword, any other mismatch is a ValueError.  Not covered (follow-up): a batch per rank of the per-video data-parallel hand-over."""
        # (batch None: the entry builds the batch itself, for this model's options)
        want = getattr(self.opt, 'CG_init_feats_type', '') or ''
        got = want if batch is None else (getattr(batch, 'CG_init_feats_type', '') or '')
        if set(want) != set(got):
            if not got:
                raise NotImplementedError("CG_init_feats_type=%r: a plain batch starts from the zero state -- build it for the model's initial "
                                          "state: VideoBatch.from_videos(..., CG_init_feats_type=%r)" % (want, want))
            raise ValueError('the batch was built for CG_init_feats_type=%r, the model has %r' % (got, want))
        # (batch None: the entry builds the batch itself, for this model's clip context)
        have = self.clip_parts() if batch is None else getattr(batch, 'clip_parts', 1)
        if self.clip_parts() != have:
            if have == 1:
                raise NotImplementedError("clip_context_type=%r: a plain batch attends over the C3D rows ('CC') only -- build it for the model's "
                                          "clip context: VideoBatch.from_videos(..., clip_context_type=%r)"
                                          % (self.opt.clip_context_type, self.opt.clip_context_type))
            raise ValueError('the batch was built for clip_context_type=%r, the model has %r'
                             % (getattr(batch, 'clip_context_type', 'CC'), self.opt.clip_context_type))
        arena = getattr(self, '_echr_arena', None)
        if arena is not None and (getattr(arena, 'early_grad_hook', None) is not None or getattr(arena, 'early_reducer', None) is not None):
            raise NotImplementedError('data-parallel gradient hand-over (parallel.EarlyReducer / DataParallelStep) takes one video per rank and '
                                      'call: a VideoBatch per rank is a follow-up')

    def get_video_context_batch(self, batch):
        """Scene context of a batch, one vector per video [V, Dv]: 'VL' the video's lda_feats, 'VC' / 'VH' the column mean over THAT video's
        rows of c3d / tap (echr_seg_col_mean_fwd), concatenated in that order."""
        vt = self.opt.video_context_type
        parts = []
        if 'VL' in vt:
            parts.append(EF._f32c(batch.lda))
        if 'VC' in vt:
            parts.append(EF.SegColMean.apply(batch.c3d, batch.dev('row_offset')))
        if 'VH' in vt:
            parts.append(EF.SegColMean.apply(batch.tap, batch.dev('row_offset')))
        return parts[0] if len(parts) == 1 else torch.cat(parts, 1)

    def _train_rl(self, video, event, clip, clip_mask, drop, gen_result):
        """Self-critical training (CaptionGenerator.py:32-37): a multinomial sample under the iteration's dropout state, the greedy baseline in
        eval mode without a graph, both on the same event context; `sample_logprobs` is the teacher-forced recompute of the sample under the
        SAME dropout state gathered at its tokens, so the gradient reaches the decoder, `event` and the encoder as mode='train' does."""
        lm = self.lm_model

        def greedy(ev, _h0):
            was_training = lm.training
            lm.eval()
            try:
                return lm.sample(video, ev, clip, clip_mask)[0]
            finally:
                lm.train(was_training)
        # (the initial state of CG_init_feats_type is made inside the decoder's own calls, from the event context each is given)
        return self._self_critical(event, None, gen_result, lambda ev, _h0: (lm.sample_train(video, ev, clip, clip_mask, drop)[0], None), greedy,
                                   lambda gen: lm(video, event, clip, clip_mask, caption_labels(gen), drop=drop))

    def change_context_dim(self):
        opt = self.opt
        vt, et, ct = opt.video_context_type, opt.event_context_type, opt.clip_context_type
        opt.video_context_dim = (opt.lda_dim if 'VL' in vt else 0) + (opt.video_dim if 'VC' in vt else 0) + \
                                (opt.hidden_dim if 'VH' in vt else 0)
        if 'ER' in et:
            opt.event_context_dim = opt.d_o
        else:
            opt.event_context_dim = (opt.video_dim if 'EC' in et else 0) + (opt.hidden_dim if 'EH' in et else 0)
        opt.clip_context_dim = (opt.video_dim if 'CC' in ct else 0) + (opt.hidden_dim if 'CH' in ct else 0)

    def get_video_context(self, tap_feats, c3d_feats, lda_feats, ind_select_list, soi_select_list):
        """Scene context (CaptionGenerator.py:87-104): 'VL' the LDA topic vector as is, 'VC' / 'VH' the mean over all T_v rows of the C3D
        features / the proposal encoder's states (echr_col_mean_fwd), concatenated in that order."""
        vt = self.opt.video_context_type
        if vt == 'VL':
            return lda_feats
        parts = []
        if 'VL' in vt:
            parts.append(EF._f32c(lda_feats).reshape(-1))
        if 'VC' in vt:
            parts.append(EF.ColMean.apply(c3d_feats))
        if 'VH' in vt:
            parts.append(EF.ColMean.apply(tap_feats))
        return parts[0] if len(parts) == 1 else torch.cat(parts, 0)

    def get_event_context(self, tap_feats, c3d_feats, lda_feats, ind_select_list, soi_select_list, _ev=None, _drop=None):
        """TSRM over the per-event features (CaptionGenerator.py:106-130): 'ER1' the mean-pooled C3D rows, 'ER2' the SST state at the anchor,
        'ER3' (the recipe) both, concatenated.  'EC' / 'EH': those features as they are, [N, video_dim] / [N, hidden_dim], without the encoder;
        'EH' carries EventPoolGather's autograd edge into tap_feats."""
        ev_start, ev_len, ind, _ = _ev if _ev is not None else EF.event_index_tensors(soi_select_list, ind_select_list, c3d_feats.device)
        if self.event_direct():          # 'EC' / 'EH' (:131-137): the pooled rows / the anchors' states themselves
            return EF.EventPoolGather.apply(c3d_feats, tap_feats, ev_start, ev_len, ind, self.event_direct())
        parts = self.EVENT_ENCODED[self.opt.event_context_type]
        ech = EF.EventPoolGather.apply(c3d_feats, tap_feats, ev_start, ev_len, ind, parts)
        return self.fusion_model(ech, soi_select_list, ev_tensors=(ev_start, ev_len), drop=_drop)

    def get_clip_context(self, tap_feats, c3d_feats, lda_feats, ind_select_list, soi_select_list, _ev=None):
        """Frame-level context over the rows of 'CC' (c3d_feats), 'CH' (tap_feats) or 'CC+CH' ([c3d | tap] on the feature axis).  Internal
        callers get a zero-copy ClipView (+ None mask) whose rows' tap columns receive their gradient through the decoder's backward
        (echr_decoder_row_grad); external callers (no `_ev`) get the reference's padded [N,A,D] tensor and [N,A] mask (CaptionGenerator.py:140-167)."""
        parts = self.clip_parts()
        if _ev is not None:
            ev_start, ev_len, _, A = _ev
            if parts == 1:
                return ClipView(c3d_feats, ev_start, ev_len, A, EF.rows_disjoint(soi_select_list)), None
            rows = tap_feats if parts == 2 else EF.clip_rows(c3d_feats, tap_feats)
            col0 = 0 if parts == 2 else c3d_feats.shape[1]
            return ClipView(rows, ev_start, ev_len, A, EF.rows_disjoint(soi_select_list), grad_src=tap_feats, grad_col0=col0), None
        if parts == 1:
            rows = c3d_feats
        elif parts == 2:
            rows = tap_feats
        else:
            T = min(c3d_feats.shape[0], tap_feats.shape[0])
            rows = torch.cat([c3d_feats[:T], tap_feats[:T]], 1)
        ev_start, ev_len, _, A = EF.event_index_tensors(soi_select_list, ind_select_list, rows.device)
        return ClipView(rows, ev_start, ev_len, A).materialize()

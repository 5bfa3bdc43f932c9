"""Three-stream attention caption decoder -- drop-in for the reference's models/OldModel_NEW.py
(the `three_stream` branch that models.setup_lm can return: OldModel :18-187, Attention :366-401,
ThreeStream_Core :762-823, ThreestreamModel :1040-1043).

Also the one-stream decoder of the reference's default options: ShowAttendTellCore :190-274, ShowAttendTellModel :1009-1012, live with one
LSTM layer through echr_amd.sat (echr_sat_fwd / _bwd / _step / _sample).

Module/parameter names and shapes match the reference so `state_dict()`s are interchangeable.  The
sub-modules (nn.Embedding, nn.Linear, nn.LSTMCell) are parameter containers only: `forward` and
`sample` run the whole sequence through libechr_hip.so (echr_decoder_fwd/bwd, echr_decoder_sample).
"""
import numpy as np
import torch
import torch.nn as nn

from .. import functional as EF


class ClipView(object):
    """The frame-level ('CC') context without the zero-padded copy: event n's slot a is row
    ev_start[n] + a of `feats` [T,D] (CaptionGenerator.py:140-167 materialises [N,A,D] + mask instead)."""

    def __init__(self, feats, ev_start, ev_len, max_len, rows_disjoint=False, grad_src=None, grad_col0=0):
        self.feats, self.ev_start, self.ev_len, self.max_len = feats, ev_start, ev_len, int(max_len)
        self.rows_disjoint = bool(rows_disjoint)          # no two events share a row of `feats`
        # 'CH' / 'CC+CH': the tensor whose rows fill columns [grad_col0, grad_col0 + its width) of `feats` (tap_feats) -- the decoder's backward
        # returns its gradient; None: `feats` is data ('CC')
        self.grad_src, self.grad_col0 = grad_src, int(grad_col0)

    @property
    def shape(self):
        return (self.ev_start.numel(), self.max_len, self.feats.shape[1])

    def materialize(self):
        """(clip [N,A,D], mask [N,A]) exactly as the reference builds them (pure data movement)."""
        N, A, D = self.shape
        a = torch.arange(A, device=self.feats.device)
        mask = (a[None, :] < self.ev_len[:, None].long())
        rows = (self.ev_start[:, None].long() + a[None, :]).clamp_(max=self.feats.shape[0] - 1)
        clip = self.feats[rows] * mask[:, :, None].to(self.feats.dtype)
        return clip, mask.to(self.feats.dtype)

    @staticmethod
    def from_padded(clip, clip_mask):
        """Wrap a reference-style padded clip tensor [N,A,D] + prefix mask [N,A] (one small D2H sync for the lengths)."""
        N, A, D = clip.shape
        lens = clip_mask.reshape(N, A).sum(1).round().to(torch.int32)
        if int(lens.min()) <= 0:
            raise ValueError('clip_mask has an empty row')
        starts = (torch.arange(N, device=clip.device, dtype=torch.int32) * A)
        return ClipView(clip.reshape(N * A, D).contiguous(), starts.contiguous(), lens.contiguous(), A, rows_disjoint=True)


def n_decoder_steps(seq):
    """Iterations of the teacher-forced loop incl. its early break on an all-zero label column
    (OldModel_NEW.py:105,122), computed once on the host instead of one device sync per step."""
    if isinstance(seq, torch.Tensor):
        nz = (seq != 0).any(0).cpu().numpy()
    else:
        nz = (np.asarray(seq) != 0).any(0)
    L = len(nz)
    S = 0
    for i in range(L - 1):
        if i >= 1 and not nz[i]:
            break
        S += 1
    return S


def caption_labels(gen):
    """[0 | gen | 0]: the teacher-forced tokens of captions gen [N, T] as int64 [N, T+2] -- a torch tensor on gen's device or a numpy
    array, as gen is."""
    N, T = gen.shape
    labels = torch.zeros(N, T + 2, dtype=torch.int64, device=gen.device) if isinstance(gen, torch.Tensor) else np.zeros((N, T + 2), np.int64)
    labels[:, 1:T + 1] = gen
    return labels


class OldModel(nn.Module):
    def __init__(self, opt):
        super(OldModel, self).__init__()
        self.CG_init_feats_type = opt.CG_init_feats_type
        self.opt = opt
        self.vocab_size = opt.CG_vocab_size
        self.input_encoding_size = opt.CG_input_encoding_size
        self.rnn_type = opt.CG_rnn_type
        self.rnn_size = opt.CG_rnn_size
        self.num_layers = opt.CG_num_layers
        self.drop_prob_lm = opt.CG_drop_prob
        self.seq_length = opt.CG_seq_length
        self.CG_init_feats_dim = self.decide_init_feats_dim()
        self.ss_prob = 0.0
        if self.CG_init_feats_dim:
            # non-zero initial state (OldModel_NEW.py:38-39, :79-96): h(-1) = c(-1) = init_linear(cat(selected contexts)); registered ahead of
            # `embed` like the reference does
            self.init_linear = nn.Linear(self.CG_init_feats_dim, self.num_layers * self.rnn_size)
        self.embed = nn.Embedding(self.vocab_size + 1, self.input_encoding_size)
        one_stream = opt.caption_model == 'show_attend_tell'
        if not one_stream and ('three_stream' not in opt.caption_model or 'three_stream_2stream' in opt.caption_model):
            raise NotImplementedError('caption_model=%r: the three_stream and show_attend_tell decoders are on the HIP path' % (opt.caption_model,))
        self.logit = nn.Linear((1 if one_stream else 3) * self.rnn_size, self.vocab_size + 1)          # OldModel_NEW.py:41-51
        self.dropout = nn.Dropout(self.drop_prob_lm)
        self.init_weights()
        self._drop_seed = None
        self._drop_calls = 0

    def decide_init_feats_dim(self):
        t, o = self.CG_init_feats_type, self.opt
        return (o.video_context_dim if 'V' in t else 0) + (o.event_context_dim if 'E' in t else 0) + \
               (o.clip_context_dim if 'C' in t else 0)

    def init_weights(self):
        r = 0.1                                            # OldModel_NEW.py:66-70
        with torch.no_grad():
            self.embed.weight.uniform_(-r, r)
            self.logit.bias.zero_()
            self.logit.weight.uniform_(-r, r)

    # ---- dropout bookkeeping ----------------------------------------------------------------------
    def next_drop_state(self, p_tsrm=0.3):
        """Dropout configuration for the next forward: fresh Philox offset per training-mode call."""
        if self._drop_seed is None:
            seed = int(torch.initial_seed())
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                # data parallel: every rank must draw its OWN masks (replicas see different videos, like m_batch different iterations
                # of the reference), so the rank is mixed into the seed
                seed ^= ((torch.distributed.get_rank() + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
            self._drop_seed = seed & 0xFFFFFFFFFFFFFFFF
        st = EF.DropState(self._drop_seed, self._drop_calls, self.training, p_tsrm, self._stream_dropout_p(), self.dropout.p)
        if self.training:
            self._drop_calls += 1
        return st

    def _stream_dropout_p(self):
        """p of the per-stream dropout sites (echr_dropout.p_h): the three-stream core's; a core without such sites returns 0."""
        return self.core.dropout0.p

    def native_params(self):
        cached = self.__dict__.get('_native_params')
        if cached is not None:
            return cached
        self.__dict__['_native_params'] = self._native_params_now()          # Parameter OBJECTS are stable (.data may move into an arena)
        return self.__dict__['_native_params']

    def invalidate_native_caches(self):
        """Forget the cached Parameter tuple and the greedy decoder's parameter-derived tables.  Called by everything of nn.Module that can
        REPLACE Parameter objects or rewrite their storage behind torch's version counters (`_apply`: .to / .cuda / to_empty; load_state_dict,
        also with assign=True; pickling).  Code that re-assigns a sub-module's Parameter by hand (weight tying, pruning) or writes through
        `.data` must call it too."""
        self.__dict__.pop('_native_params', None)
        self.__dict__.pop('_sample_tables', None)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_native_caches()
        return super(OldModel, self)._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self.invalidate_native_caches()
        return super(OldModel, self)._load_from_state_dict(*args, **kwargs)

    def __getstate__(self):
        d = dict(self.__dict__)          # the caches hold Parameter references / a large device tensor: neither belongs in a pickle or a deepcopy
        d.pop('_native_params', None)
        d.pop('_sample_tables', None)
        return d

    def sample_tables(self):
        """The dict the greedy decodes keep their parameter-derived operands in (EF.greedy_sample's table_cache), reused across calls until
        invalidate_native_caches() drops it."""
        return self.__dict__.setdefault('_sample_tables', {})

    def _grad_sink(self, params):
        """Where the backward of a Function over `params` writes their gradients: the module's flat arena, or None without one."""
        arena = getattr(self, '_echr_arena_ref', None)
        return EF.GradSink(arena, params) if arena is not None else None

    def _native_params_now(self):
        c = self.core
        a = c.attention
        return (self.embed.weight, self.logit.weight, self.logit.bias,
                c.layer0.weight_ih, c.layer1.weight_ih, c.layer2.weight_ih,
                c.layer0.weight_hh, c.layer1.weight_hh, c.layer2.weight_hh,
                c.layer0.bias_ih, c.layer1.bias_ih, c.layer2.bias_ih,
                c.layer0.bias_hh, c.layer1.bias_hh, c.layer2.bias_hh,
                a.ctx2att.weight, a.ctx2att.bias, a.h2att.weight, a.h2att.bias, a.alpha_net.weight, a.alpha_net.bias)

    @staticmethod
    def _clip_view(clip, clip_mask):
        return clip if isinstance(clip, ClipView) else ClipView.from_padded(clip, clip_mask)

    def _tokens(self, seq, dev):
        """[S,N] time-major int32 input tokens of the teacher-forced loop (S = its iteration count, OldModel_NEW.py:105,122)."""
        S = n_decoder_steps(seq)
        if S == 0:
            raise ValueError('label tensor needs at least two columns')
        seq_t = torch.as_tensor(np.asarray(seq) if not isinstance(seq, torch.Tensor) else seq)
        if seq_t.is_cuda:
            return seq_t[:, :S].t().to(device=dev, dtype=torch.int32).contiguous()
        # host labels: slice / transpose / cast on the host, ONE small H2D copy instead of three device ops
        return EF.upload(seq_t[:, :S].t().to(torch.int32).contiguous(), dev)

    def prepare(self, video, clip, clip_mask, seq):
        """Start the part of forward() that does not need the event context (packs, ctx2att over the video, token-side gate products) on
        the library's second stream; call BEFORE launching the event encoder and pass the result to forward(prepared=...)."""
        if self.training and self.ss_prob > 0.0:
            raise NotImplementedError('scheduled sampling (ss_prob > 0) is never enabled by the reference and is not on the HIP path')
        cv = self._clip_view(clip, clip_mask)
        tokens = self._tokens(seq, cv.feats.device)
        return EF.decoder_prepare(video, cv.feats, cv.ev_start, cv.ev_len, tokens, cv.max_len, cv.rows_disjoint, self.native_params())

    def forward(self, video, event, clip, clip_mask, seq, drop=None, prepared=None):
        """Teacher-forced log-probs [N,S,V+1] (OldModel_NEW.py:98-130)."""
        if self.training and self.ss_prob > 0.0:
            raise NotImplementedError('scheduled sampling (ss_prob > 0) is never enabled by the reference and is not on the HIP path')
        cv = self._clip_view(clip, clip_mask)
        tokens = prepared['tokens'] if prepared is not None else self._tokens(seq, event.device)
        if drop is None:
            drop = self.next_drop_state()
        ps = self.native_params()
        return EF.DecoderFunction.apply(video, event, cv.feats, cv.ev_start, cv.ev_len, tokens, cv.max_len, cv.rows_disjoint, drop,
                                        self._grad_sink(ps), prepared, self._initial_state(video, event, cv), cv.grad_src, cv.grad_col0, None, *ps)

    def _initial_state(self, video, event, cv):
        """None (the recipe: zero state) or h0 [N, 3H] = init_linear(cat([video | event | clip.mean(1)])) (OldModel_NEW.py:79-92) -- the decoder
        entry points take the map in this layout; the reference's view(N, 3, H).transpose(0, 1) is `init_hidden`'s."""
        if not self.CG_init_feats_dim:
            return None
        t = self.CG_init_feats_type
        w, b = self.init_linear.weight, self.init_linear.bias
        return EF.InitState.apply(video, event, cv.feats, cv.ev_start, cv.ev_len, cv.max_len, None, ('V' in t, 'E' in t, 'C' in t),
                                  self._grad_sink((w, b)), w, b)

    def init_hidden(self, video, event, clip, clip_mask=None):
        """Initial state (h, c), each [3,N,H] (OldModel_NEW.py:72-96): zeros, or -- with CG_init_feats_type -- the init_linear map for both."""
        n = event.shape[0] if event is not None else clip.shape[0]
        w = self.logit.weight
        if not self.CG_init_feats_dim:
            return (w.new_zeros(self.num_layers, n, self.rnn_size), w.new_zeros(self.num_layers, n, self.rnn_size))
        h0 = self._initial_state(video, event, self._clip_view(clip, clip_mask))
        m = h0.view(n, self.num_layers, self.rnn_size).transpose(0, 1)
        return (m, m)

    def get_logprobs_state(self, it, video, event, clip, clip_mask, state):
        """One decoder timestep, state in / state out (OldModel_NEW.py:133-137): (log-probs [N,V+1], (h', c')).

        Runs through echr_decoder_step; forward only (the reference's training loop is forward(), which keeps the whole
        sequence inside the library).  In training mode each call draws a fresh dropout stream."""
        cv = self._clip_view(clip, clip_mask)
        drop = self.next_drop_state()
        with torch.no_grad():
            return EF.decoder_step(it, video, event, cv.feats, cv.ev_start, cv.ev_len, cv.max_len, state, self.native_params(), drop)

    def sample(self, video, event, clip, clip_mask, opt={}):
        """OldModel.sample (OldModel_NEW.py:139-187).  beam_size = 1: greedy arg-max (sample_max = 1, the recipe's setting) or, with
        sample_max = 0, a draw from softmax(logp / temperature) per step (:160-168).  The draws come from the library's counter-based
        Philox stream (seed: set_dropout_state / torch.initial_seed, advanced once per call), not from torch.multinomial's generator: same
        distribution, different random numbers.

        beam_size = B > 1 (the reference's `--beam_size`, whose beam branch is commented out there): beam search on device
        (functional.beam_search), eval mode and sample_max = 1 only.  Returns (seq, logp) like the greedy decode; logp is 0 after a row's
        <eos> where the greedy decode keeps the raw arg-max log-probs.  opt['return_score'] = True appends score [N], the sum of each
        result's token log-probs (<eos> included).  opt['defer'] = True (beam_size 1): the decode is queued and EF.greedy_sample's deferred
        handle is returned instead of the result."""
        beam = int(opt.get('beam_size', 1))
        if beam != 1:
            EF._check_beam_size(beam, self.vocab_size + 1)
            if opt.get('sample_max', 1) != 1:
                raise ValueError('beam search decodes by score: it does not combine with sample_max = 0')
            if self.training:
                raise ValueError('beam search is an evaluation decode: call eval() first')
            cv = self._clip_view(clip, clip_mask)
            with torch.no_grad():
                seq, logp, score = EF.beam_search(video, event, cv.feats, cv.ev_start, cv.ev_len, cv.max_len, self.seq_length,
                                                  self.native_params(), beam, h0=self._initial_state(video, event, cv))
            return (seq, logp, score) if opt.get('return_score', False) else (seq, logp)
        cv = self._clip_view(clip, clip_mask)
        multinomial = opt.get('sample_max', 1) != 1
        seed = self._sample_seed() if multinomial else 0
        with torch.no_grad():
            return EF.greedy_sample(video, event, cv.feats, cv.ev_start, cv.ev_len, cv.max_len, self.seq_length,
                                    self.native_params(), multinomial=multinomial, temperature=float(opt.get('temperature', 1.0)),
                                    seed=seed, table_cache=self.sample_tables(), h0=self._initial_state(video, event, cv),
                                    defer=bool(opt.get('defer', False)))


    def _sample_seed(self):
        """Seed of the next multinomial decode: one per call, derived from the (rank-mixed) dropout seed."""
        if self._drop_seed is None:
            self.next_drop_state()                         # derives the (rank-mixed) seed once
        self._sample_calls = getattr(self, '_sample_calls', 0) + 1
        return (self._drop_seed * 0x9E3779B97F4A7C15 + self._sample_calls) & 0xFFFFFFFFFFFFFFFF

    def sample_train(self, video, event, clip, clip_mask, drop, temperature=1.0, seed=None):
        """The sampled pass of self-critical training (CaptionGenerator.py:33 -> sample(..., {'sample_max': 0}) in training mode,
        OldModel_NEW.py:139-187): a multinomial draw per step with the decoder's dropout active under `drop`, the masks that forward() draws
        for the same state at the same step (echr_decoder_sample_train).  Returns (gen_result int64 [N,T], log-probs at the drawn tokens
        [N,T]) without a graph, or ([], []); score the tokens with sequence_logprobs() for the gradient."""
        cv = self._clip_view(clip, clip_mask)
        seed = self._sample_seed() if seed is None else int(seed)
        with torch.no_grad():
            return EF.greedy_sample(video, event, cv.feats, cv.ev_start, cv.ev_len, cv.max_len, self.seq_length, self.native_params(),
                                    multinomial=True, temperature=float(temperature), seed=seed, h0=self._initial_state(video, event, cv),
                                    drop=drop)

    def sequence_logprobs(self, video, event, clip, clip_mask, seq, drop=None):
        """Log-probs [N,T] of the given captions seq [N,T] (zero after a row's <eos>): the teacher-forced forward() on [0 | seq | 0] under
        `drop`, gathered at seq -- with the drop state of the sampled pass these are its `sampleLogprobs` up to each row's <eos>, and the
        gradient flows through the decoder into `event` like forward()'s (the sampling loop keeps no graph)."""
        seq = torch.as_tensor(seq)
        logp = self.forward(video, event, clip, clip_mask, caption_labels(seq), drop=drop)
        return EF.GatherTokens.apply(logp, seq)


class Attention(nn.Module):
    """Additive attention parameters (OldModel_NEW.py:366-375); arithmetic fused into the decoder kernels."""

    def __init__(self, opt):
        super(Attention, self).__init__()
        self.rnn_size = opt.CG_rnn_size
        self.att_hid_size = opt.CG_att_hid_size
        self.att_feat_size = opt.clip_context_dim
        self.ctx2att = nn.Linear(self.att_feat_size, self.att_hid_size)
        self.h2att = nn.Linear(self.rnn_size, self.att_hid_size)
        self.alpha_net = nn.Linear(self.att_hid_size, 1)


class ThreeStream_Core(nn.Module):
    """Three independent LSTM-cell streams (event / attended clip / scene) + late fusion (OldModel_NEW.py:762-799)."""

    def __init__(self, opt):
        super(ThreeStream_Core, self).__init__()
        self.opt = opt
        self.input_encoding_size = opt.CG_input_encoding_size
        self.rnn_type = opt.CG_rnn_type
        self.rnn_size = opt.CG_rnn_size
        self.drop_prob_lm = opt.CG_drop_prob
        self.fc_feat_size = opt.CG_fc_feat_size
        self.att_feat_size = opt.clip_context_dim
        self.att_hid_size = opt.CG_att_hid_size
        # accepted and ignored, exactly as the reference's ThreeStream_Core does: CG_input_dim is computed (:775-776,:790-799) and never used --
        # no layer is sized by it and forward (:801-823) never reads it
        self.CG_input_feats_type = opt.CG_input_feats_type
        self.CG_input_dim = sum(d for c, d in (('V', opt.video_context_dim), ('E', opt.event_context_dim), ('C', opt.clip_context_dim))
                                if c in self.CG_input_feats_type)
        E = self.input_encoding_size
        self.layer0 = nn.LSTMCell(opt.event_context_dim + E, self.rnn_size)
        self.layer1 = nn.LSTMCell(opt.clip_context_dim + E, self.rnn_size)
        self.layer2 = nn.LSTMCell(opt.video_context_dim + E, self.rnn_size)
        self.fusion_layer = nn.Linear(self.rnn_size * 3, self.rnn_size)      # registered, never used (:783)
        self.attention = Attention(opt)
        self.dropout0 = nn.Dropout(0.5)
        self.dropout1 = nn.Dropout(0.5)
        self.dropout2 = nn.Dropout(0.5)


class ThreestreamModel(OldModel):
    def __init__(self, opt):
        super(ThreestreamModel, self).__init__(opt)
        self.core = ThreeStream_Core(opt)


class ShowAttendTellCore(nn.Module):
    """Parameter container with the reference's layout (OldModel_NEW.py:190-216): nn.LSTM(E + input_dim, H, num_layers, bias=False) +
    the additive-attention projections.  No arithmetic: see ShowAttendTellModel."""

    def __init__(self, opt):
        super(ShowAttendTellCore, self).__init__()
        self.opt = opt
        t = opt.CG_input_feats_type
        self.CG_input_dim = (opt.video_context_dim if 'V' in t else 0) + (opt.event_context_dim if 'E' in t else 0) + \
                            (opt.clip_context_dim if 'C' in t else 0)                                        # :219-227
        self.rnn = getattr(nn, opt.CG_rnn_type.upper())(opt.CG_input_encoding_size + self.CG_input_dim, opt.CG_rnn_size, opt.CG_num_layers,
                                                        bias=False, dropout=opt.CG_drop_prob if opt.CG_num_layers > 1 else 0.0)          # (one layer: nn.LSTM's own dropout has no site)
        if opt.CG_att_hid_size > 0:
            self.ctx2att = nn.Linear(opt.clip_context_dim, opt.CG_att_hid_size)
            self.h2att = nn.Linear(opt.CG_rnn_size, opt.CG_att_hid_size)
            self.alpha_net = nn.Linear(opt.CG_att_hid_size, 1)
        else:
            self.ctx2att = nn.Linear(opt.clip_context_dim, 1)
            self.h2att = nn.Linear(opt.CG_rnn_size, 1)


class ShowAttendTellModel(OldModel):
    """`caption_model='show_attend_tell'` (models/__init__.py:7-8, OldModel_NEW.py:1009-1012), the reference's default decoder: ONE attention
    LSTM stream whose input is [token | video if 'V' | event if 'E' | attended clip if 'C'] (CG_input_feats_type), one dropout site on its
    output, logit [V+1, H].  state_dict-compatible with the reference (embed, logit, core.rnn.*, core.ctx2att / h2att / alpha_net).

    Live on the HIP path (echr_amd.sat over echr_sat_fwd / _bwd / _step / _sample) with CG_num_layers == 1, an LSTM, CG_att_hid_size > 0 and
    a non-empty CG_input_feats_type: forward (teacher forcing, with its autograd graph), get_logprobs_state, init_hidden and the greedy
    sample.  Every other configuration CONSTRUCTS -- experiments/train_SST.sh builds the three-layer one while the captioner stays idle
    (train.py:291-295) and reads / writes its checkpoints -- and refuses at call time, before any argument is touched.  The state handed from
    step to step is the UNDROPPED (h, c), each [1, N, H]."""

    def __init__(self, opt):
        super(ShowAttendTellModel, self).__init__(opt)
        self.core = ShowAttendTellCore(opt)

    def _refuse(self, what):
        raise NotImplementedError("caption_model='show_attend_tell': %s" % what)

    def _require_live(self):
        """The configuration check of every entry: NotImplementedError naming the option, or the echr_sat_args.feats bits."""
        o = self.opt
        if o.CG_num_layers != 1:
            self._refuse('CG_num_layers=%r -- one LSTM layer runs on the HIP path; a deeper stack is a parameter container (the recipe that '
                         'builds it, experiments/train_SST.sh, never runs the captioner)' % (o.CG_num_layers,))
        if o.CG_rnn_type.lower() != 'lstm':
            self._refuse("CG_rnn_type=%r -- the HIP path runs the 'lstm' cell" % (o.CG_rnn_type,))
        if not o.CG_att_hid_size > 0:
            self._refuse('CG_att_hid_size=%r -- the HIP path runs the attention with a hidden layer (CG_att_hid_size > 0)' % (o.CG_att_hid_size,))
        from ..sat import feats_bits
        feats = feats_bits(o.CG_input_feats_type)
        if not feats:
            self._refuse("CG_input_feats_type=%r selects none of 'V', 'E', 'C' -- the reference fails there too (torch.cat of an empty list in "
                         "get_input_feats, OldModel_NEW.py:241)" % (o.CG_input_feats_type,))
        return feats

    def _clip(self, clip, clip_mask):
        cv = self._clip_view(clip, clip_mask)
        if cv.grad_src is not None:
            self._refuse("clip_context_type with 'CH' -- the one-stream decoder attends over the C3D rows ('CC'); the gradient into tap_feats "
                         "through the clip rows is a follow-up")
        return cv

    def next_drop_state(self, p_tsrm=0.3):
        """Dropout configuration for the next forward: the decoder's one site is on its output (p_h is not drawn)."""
        self._require_live()
        return super(ShowAttendTellModel, self).next_drop_state(p_tsrm)

    def _stream_dropout_p(self):
        return 0.0

    def _native_params_now(self):
        c = self.core
        return (self.embed.weight, self.logit.weight, self.logit.bias, c.rnn.weight_ih_l0, c.rnn.weight_hh_l0,
                c.ctx2att.weight, c.ctx2att.bias, c.h2att.weight, c.h2att.bias, c.alpha_net.weight, c.alpha_net.bias)

    def prepare(self, *a, **k):
        self._refuse('prepare() -- the overlap-encoder pre-compute belongs to the three_stream decoder')

    def forward(self, video=None, event=None, clip=None, clip_mask=None, seq=None, drop=None, prepared=None):
        """Teacher-forced log-probs [N,S,V+1] (OldModel_NEW.py:98-130)."""
        from .. import sat
        feats = self._require_live()
        if prepared is not None:
            self.prepare()
        if self.training and self.ss_prob > 0.0:
            self._refuse('ss_prob > 0 -- scheduled sampling is never enabled by the reference and is not on the HIP path')
        cv = self._clip(clip, clip_mask)
        tokens = self._tokens(seq, cv.feats.device)
        if drop is None:
            drop = self.next_drop_state()
        ps = self.native_params()
        return sat.SatFunction.apply(video, event, cv.feats, cv.ev_start, cv.ev_len, tokens, cv.max_len, cv.rows_disjoint, drop,
                                     self._grad_sink(ps), self._initial_state(video, event, cv), feats, *ps)

    def init_hidden(self, video=None, event=None, clip=None, clip_mask=None):
        """Initial state (h, c), each [1,N,H] (OldModel_NEW.py:72-96)."""
        self._require_live()
        return super(ShowAttendTellModel, self).init_hidden(video, event, clip, clip_mask)

    def get_logprobs_state(self, it=None, video=None, event=None, clip=None, clip_mask=None, state=None):
        """One decoder timestep (OldModel_NEW.py:133-137): (log-probs [N,V+1], (h', c')), the state undropped and [1,N,H].  Forward only; in
        training mode each call draws a fresh dropout stream."""
        from .. import sat
        feats = self._require_live()
        cv = self._clip(clip, clip_mask)
        drop = self.next_drop_state()
        with torch.no_grad():
            return sat.sat_step(it, video, event, cv.feats, cv.ev_start, cv.ev_len, cv.max_len, state, self.native_params(), feats, drop)

    def sample(self, video=None, event=None, clip=None, clip_mask=None, opt={}):
        """The greedy branch of OldModel.sample (OldModel_NEW.py:139-187): (seq, logp), or ([], [])."""
        from .. import sat
        feats = self._require_live()
        if int(opt.get('beam_size', 1)) != 1:
            self._refuse('beam_size=%r -- beam search runs on the three_stream decoder; this one decodes greedily' % (opt.get('beam_size'),))
        if opt.get('sample_max', 1) != 1:
            self._refuse('sample_max=0 -- the multinomial decode runs on the three_stream decoder; this one decodes greedily')
        cv = self._clip(clip, clip_mask)
        with torch.no_grad():
            return sat.sat_greedy_sample(video, event, cv.feats, cv.ev_start, cv.ev_len, cv.max_len, self.seq_length, self.native_params(), feats,
                                         h0=self._initial_state(video, event, cv))

    def sample_train(self, *a, **k):
        self._refuse("mode='train_rl' -- self-critical training (the sampled pass) runs on the three_stream decoder")

    def sequence_logprobs(self, *a, **k):
        self._refuse("mode='train_rl' -- self-critical training (the sample's log-probs) runs on the three_stream decoder")


def _ablation(name):
    class _Unsupported(nn.Module):
        def __init__(self, *a, **k):
            raise NotImplementedError('%s is an ablation variant outside the ECHR hot path (SURVEY section 2 row 4)' % name)
    _Unsupported.__name__ = name
    return _Unsupported


# names the reference's models/__init__.py imports (models/__init__.py:1); ThreestreamModel is live, ShowAttendTellModel holds parameters
for _n in ('AllImgModel', 'H3Model', 'TwostreamModel', 'Twostream_jump_Model', 'TwostreamModel_3LSTM',
           'H3denseModel', 'H3denaddModel', 'ThreestreamModel_2stream', 'ThreestreamModel_2stream_LDA',
           'ThreestreamModel_2stream_CC'):
    globals()[_n] = _ablation(_n)

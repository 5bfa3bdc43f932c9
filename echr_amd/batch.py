"""Multi-video batches of the caption path: plain data + validation, no kernels.

The reference runs ONE video per call (`batch_size = 1`, opts.py:187) and sums the gradients of `m_batch` videos before one clamp +
step (train.py:281-283,313-317).  A `VideoBatch` is those `m_batch` videos as one call: the feature rows of the videos are concatenated,
the event intervals / anchors become batch-absolute row indices, and every event remembers its video (`vid`).  The batched entry points
(`CaptionGenerator.forward_batch`, `FusedTrainStep.batch`) then compute what V single-video calls compute:

  * an event attends only to the events of its own video, and reads its own video's scene vector;
  * the loss is the SUM over the videos of LanguageModelCriterion, each video with its own normaliser `sum(mask_v) + 1e-6`, the mask
    cut to the video's own step count (no 1/V);
  * gradients are the sum over the videos, then ONE clamp and ONE Adam step;
  * a batched call consumes ONE dropout counter and keys every site by the batch-global element index.

A batch is built for ONE frame-level context (`clip_context_type`, default 'CC'): with 'CH' / 'CC+CH' the decoder attends over
`clip_rows()` -- tap, or [c3d | tap] -- and d tap gains the attended rows' gradient; the entry points refuse a batch built for another
context than the model's.  Likewise a batch is built for the model's initial decoder state (`CG_init_feats_type`, default '': zeros):
with 'V' / 'E' / 'C' every event starts from init_linear over its OWN video's scene vector, its event context and its clip mean over
its own video's padded clip length.  And a batch is built for ONE decoder (`caption_model`, default the three-stream recipe's):
`caption_model='show_attend_tell'` is the one-stream decoder of echr_amd.sat, which attends over the C3D rows only -- such a batch
refuses 'CH' rows when it is built, a three-stream model refuses it, and a one-stream model refuses a batch built without the keyword.
"""
import numpy as np
import torch

from .models.OldModel_NEW import caption_labels, n_decoder_steps

_KEYS = ('c3d', 'tap', 'lda', 'ind', 'soi')


def _np(x, dtype):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


# whose reward: (it may be wider than T, its refusal) -- a batch's, a single video's, one video's of a batch from reward_fn
_REWARD_FORMS = {'batch': (True, 'reward must be [N_tot, T] or [N_tot] (got %s for gen_result %s)'),
                 'single': (False, 'reward must be [N, T] or [N] (got %s for gen_result %s)'),
                 'video': (False, 'reward_fn must return [N_v, T_v] or [N_v] (got %s for a video of %s)')}


def reward_matrix(reward, N, T, form='batch'):
    """A reward [N] (one value per caption, broadcast over its steps) or [N, T] ('batch': [N, >= T]) as float32 [N, T]; any other shape
    is the ValueError of `form` (_REWARD_FORMS)."""
    wider, msg = _REWARD_FORMS[form]
    r = _np(reward, np.float32)
    if r.ndim == 1:
        r = np.repeat(r[:, None], T, 1)
    if (r.shape[0] != N or r.ndim != 2 or r.shape[1] < T) if wider else (r.shape != (N, T)):
        raise ValueError(msg % (r.shape, (N, T)))
    return r[:, :T]


def sampled_criterion(gen, reward, widths, slices, form='batch'):
    """RewardCriterion (misc/utils.py:48-59) of sampled captions as the reward-weighted one-call steps take it (host arrays).  gen
    [N, >= T], reward [N] or [N, >= T] (reward_matrix, in `form`), and groups of rows `slices` with their own widths
    `widths`, T = max(widths): the videos of a batch at their video_words, or one group at the width of the tensor it was given.  Returns
    labels int64 [N, T+2] = [0 | gen | 0] (T+1 teacher-forced steps), mask float32 [N, T+1] -- [1 | gen > 0][:, :-1] over a group's own
    width and zero from there on (at the batch's width the longest row of a narrower video would otherwise gain its <eos> position; the
    step behind the last token, whose target is the trailing 0, always has mask 0) -- and reward * mask [N, T+1], undivided."""
    g = _np(gen, np.int64)
    T = int(max(widths)) if len(widths) else 0
    if g.ndim != 2 or T > g.shape[1]:
        raise ValueError('video_words %s exceed gen_result %s' % (list(map(int, widths)), g.shape))
    g = g[:, :T]
    r = reward_matrix(reward, len(g), T, form)
    mask = np.zeros((len(g), T + 1), np.float32)
    w = np.zeros_like(mask)
    for s, wv in zip(slices, map(int, widths)):
        if wv:
            mask[s, 0] = 1.0
            mask[s, 1:wv] = g[s, :wv - 1] > 0
            w[s, :wv] = r[s, :wv] * mask[s, :wv]
    return caption_labels(g), mask, w


def _check_decoder(caption_model, clip_context_type):
    """True for a batch of the one-stream decoder (caption_model='show_attend_tell'), False for the three-stream one (None or a
    'three_stream' name); refuses what the named decoder cannot take."""
    one_stream = caption_model == 'show_attend_tell'
    if caption_model is not None and not one_stream and 'three_stream' not in caption_model:
        raise ValueError("caption_model=%r: a batch is built for the three_stream decoder (the default) or 'show_attend_tell'" % (caption_model,))
    if one_stream and 'CH' in clip_context_type:
        raise NotImplementedError("caption_model='show_attend_tell' with clip_context_type=%r: the one-stream decoder attends over the C3D rows "
                                  "('CC'); 'CH' rows (the gradient into tap_feats through the clip context) are a follow-up" % (clip_context_type,))
    return one_stream


class VideoBatch(object):
    """V >= 1 videos as one batch.  Build it with `from_videos`.

    Attributes (V videos, N_tot events, T_tot feature rows):
      c3d [T_tot, D], tap [T_tot, Ht]   concatenated features (per video its first min(len(c3d), len(tap)) rows); `tap` keeps its graph
      lda [V, lda_dim]                  one LDA vector per video
      row_offset int64 [V+1]            feature rows of video v = [row_offset[v], row_offset[v+1])
      event_offset int64 [V+1]          events of video v = [event_offset[v], event_offset[v+1])
      vid int32 [N_tot]                 video of event n (non-decreasing)
      soi int64 [N_tot, 2], ind int64 [N_tot]   batch-absolute event intervals / anchors
      labels int64 [N_tot, L], masks float32 [N_tot, L]   stacked, zero padded to the widest video's L (host tensors; None without labels);
                                        a video's mask is zero behind ITS OWN step count S_v (column 1 + S_v onwards)
      S                                 decoder steps of the stacked labels; steps[v] = S_v
      event_slices                      slice of the event axis per video; split(x) cuts a [N_tot, ...] result accordingly
      clip_context_type, clip_parts     the frame-level context the batch was built for: 1 = 'CC' (default), 2 = 'CH', 3 = 'CC+CH';
                                        clip_rows() is the decoder's row source -- c3d, tap or [c3d | tap]
      CG_init_feats_type                the initial decoder state the batch was built for ('' = zeros, else from 'V', 'E', 'C')
      caption_model, one_stream         the decoder the batch was built for: None (the three-stream recipe) or 'show_attend_tell'
      refs                              optional, set by the caller: the packed references of the N_tot events in row order
                                        (echr_amd.reward.pack_refs) -- what fused.SelfCriticalBatchStep scores a CiderDReward against
    """

    def __init__(self, c3d, tap, lda, row_offset, event_offset, soi, ind, labels=None, masks=None, *, caption_model=None, CG_init_feats_type='',
                 clip_context_type='CC'):
        self.c3d, self.tap, self.lda = c3d, tap, lda
        self.refs = None
        self.caption_model = caption_model
        self.one_stream = _check_decoder(caption_model, clip_context_type)
        self.CG_init_feats_type = str(CG_init_feats_type or '')
        if set(self.CG_init_feats_type) - set('VEC') or len(set(self.CG_init_feats_type)) != len(self.CG_init_feats_type):
            raise ValueError("CG_init_feats_type=%r: the initial state reads 'V', 'E' and / or 'C', each at most once" % (CG_init_feats_type,))
        # the frame-level context the batch is built for, tested with `in` as CaptionGenerator.clip_parts does ('CCCH' means 'CC+CH')
        self.clip_context_type = clip_context_type
        self.clip_parts = (1 if 'CC' in clip_context_type else 0) | (2 if 'CH' in clip_context_type else 0)
        if not self.clip_parts:
            raise ValueError("clip_context_type=%r: a batch attends over 'CC', 'CH' or 'CC+CH' rows" % (clip_context_type,))
        self._clip_rows = None
        self.row_offset = np.asarray(row_offset, dtype=np.int64)
        self.event_offset = np.asarray(event_offset, dtype=np.int64)
        self.soi = np.asarray(soi, dtype=np.int64).reshape(-1, 2)
        self.ind = np.asarray(ind, dtype=np.int64).reshape(-1)
        self.n_videos = len(self.row_offset) - 1
        self.vid = np.repeat(np.arange(self.n_videos, dtype=np.int32), np.diff(self.event_offset)).astype(np.int32)
        self.labels, self.masks = labels, masks
        self.steps, self.S = None, 0
        self._dev = {}
        self.validate()
        if labels is not None:
            self.steps = [n_decoder_steps(labels[s].numpy()) for s in self.event_slices]
            self.S = n_decoder_steps(labels.numpy())

    # ---- construction -------------------------------------------------------------------------------------------------------
    @classmethod
    def from_videos(cls, videos, device=None, tap_model=None, tap_fn=None, *, caption_model=None, CG_init_feats_type='', clip_context_type='CC'):
        """`videos`: a list of dicts with the arguments of a single-video call -- 'c3d' [T, D], 'tap' [T', Ht], 'lda' [lda_dim], 'ind' [N_v],
        'soi' [N_v, 2] (indices local to the video) and, for training, 'labels' / 'masks' [N_v, L_v] -- or a dict of parallel lists under
        the same keys.  Features may be numpy arrays or tensors on any device; they are concatenated on `device` (default: the device of
        the first video's c3d when it is a tensor, else the CPU).
        With `tap_model` (a models.SST on the GPU) the videos need no 'tap': `tap` is the encoder's forward_batch over the concatenated c3d --
        ONE call for the V videos -- and keeps its autograd graph into the encoder; a 'tap' entry is then ignored.
        `tap_fn(c3d_all, rows)` (instead of tap_model): any other producer of the [T_tot, Ht] matrix from the concatenated c3d and the row
        offsets (fused.JointBatchStep runs the encoder into its own buffers, without a graph).
        `clip_context_type`: the model's frame-level context ('CC', 'CH', 'CC+CH'); the batched entry points refuse a batch built for
        another one.
        `CG_init_feats_type`: the model's initial decoder state ('' = zeros; else from 'V', 'E', 'C'), under the same rule.
        `caption_model`: the model's decoder -- None / a 'three_stream' name (the default) or 'show_attend_tell' (the one-stream decoder,
        'CC' rows only), under the same rule.  The three options are keyword-only."""
        _check_decoder(caption_model, clip_context_type)          # (ahead of any tensor work)
        if isinstance(videos, dict):
            n = len(videos['c3d'])
            videos = [{k: v[i] for k, v in videos.items()} for i in range(n)]
        videos = list(videos)
        if tap_fn is not None and tap_model is not None:
            raise ValueError('tap_model and tap_fn exclude each other')
        no_tap = tap_model is not None or tap_fn is not None
        if not videos:
            raise ValueError('a batch needs at least one video')
        for i, v in enumerate(videos):
            missing = [k for k in _KEYS if k not in v and not (k == 'tap' and no_tap)]
            if missing:
                raise ValueError('video %d lacks %s' % (i, missing))
        if device is None and tap_model is not None:
            device = next(tap_model.parameters()).device
        if device is None:
            c0 = videos[0]['c3d']
            device = c0.device if isinstance(c0, torch.Tensor) else torch.device('cpu')
        device = torch.device(device)
        as_t = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        c3ds, taps, ldas, sois, inds, rows, counts = [], [], [], [], [], [0], [0]
        with_labels = [('labels' in v and v['labels'] is not None) for v in videos]
        if any(with_labels) and not all(with_labels):
            raise ValueError('either every video carries labels / masks or none does')
        for i, v in enumerate(videos):
            c3d = as_t(v['c3d'])
            tap = c3d if no_tap else as_t(v['tap'])
            if c3d.dim() != 2 or tap.dim() != 2:
                raise ValueError('video %d: c3d / tap must be [T, D] matrices' % i)
            T = min(c3d.shape[0], tap.shape[0])
            soi = _np(v['soi'], np.int64).reshape(-1, 2)
            ind = _np(v['ind'], np.int64).reshape(-1)
            if len(soi) == 0:
                raise ValueError('video %d has no event' % i)
            if len(ind) != len(soi):
                raise ValueError('video %d: ind_select_list and soi_select_list differ in length (%d vs %d)' % (i, len(ind), len(soi)))
            if (soi[:, 1] - soi[:, 0]).min() <= 0:
                raise ValueError('video %d: every event needs at least one segment (soi=%s)' % (i, soi.tolist()))
            if soi.min() < 0 or soi[:, 1].max() > T or ind.min() < 0 or ind.max() >= T:
                raise ValueError('video %d: event intervals / anchors fall outside its %d feature rows' % (i, T))
            c3ds.append(c3d[:T].to(device=device, dtype=torch.float32))
            if not no_tap:
                taps.append(tap[:T].to(device=device, dtype=torch.float32))
            ldas.append(as_t(v['lda']).reshape(-1).to(device=device, dtype=torch.float32))
            sois.append(soi + rows[-1])
            inds.append(ind + rows[-1])
            rows.append(rows[-1] + T)
            counts.append(counts[-1] + len(soi))
        if len({c.shape[1] for c in c3ds}) != 1 or len({t.shape[1] for t in taps}) > 1 or len({l.numel() for l in ldas}) != 1:
            raise ValueError('the videos of a batch must share their feature widths')
        labels = masks = None
        if all(with_labels):
            labels, masks = cls._stack_labels(videos, counts)
        c3d_all = torch.cat(c3ds, 0)
        if tap_fn is not None:
            tap_all = tap_fn(c3d_all, rows)
        else:
            tap_all = torch.cat(taps, 0) if tap_model is None else tap_model.forward_batch(c3d_all, rows)[0]
        return cls(c3d_all, tap_all, torch.stack(ldas, 0), rows, counts, np.concatenate(sois, 0), np.concatenate(inds, 0),
                   labels, masks, clip_context_type=clip_context_type, CG_init_feats_type=CG_init_feats_type, caption_model=caption_model)

    @staticmethod
    def _stack_labels(videos, counts):
        lab = [_np(v['labels'], np.int64) for v in videos]
        msk = [_np(v['masks'], np.float32) for v in videos]
        for i, (l, m) in enumerate(zip(lab, msk)):
            n = counts[i + 1] - counts[i]
            if l.ndim != 2 or l.shape != m.shape or l.shape[0] != n:
                raise ValueError('video %d: labels %s / masks %s must both be [%d events, L]' % (i, l.shape, m.shape, n))
            if l.shape[1] < 2:
                raise ValueError('video %d: label tensor needs at least two columns' % i)
        Lw = max(l.shape[1] for l in lab)
        labels = np.zeros((counts[-1], Lw), np.int64)
        masks = np.zeros((counts[-1], Lw), np.float32)
        for i, (l, m) in enumerate(zip(lab, msk)):
            s_v = n_decoder_steps(l)
            labels[counts[i]:counts[i + 1], :l.shape[1]] = l
            # LanguageModelCriterion cuts target and mask to the log-probs' step count (misc/utils.py:66-75): the video's OWN S_v
            masks[counts[i]:counts[i + 1], :min(l.shape[1], 1 + s_v)] = m[:, :1 + s_v]
        return torch.from_numpy(labels), torch.from_numpy(masks)

    # ---- validation ---------------------------------------------------------------------------------------------------------
    def validate(self):
        """The layout contract: events of a video are contiguous, videos keep their order (vid non-decreasing, every video has an event),
        and an event's rows and anchor lie inside its own video.  Raises ValueError otherwise."""
        V, ro, eo = self.n_videos, self.row_offset, self.event_offset
        if V < 1 or len(eo) != V + 1 or ro[0] != 0 or eo[0] != 0:
            raise ValueError('a batch needs at least one video and offsets that start at 0')
        if np.any(np.diff(ro) <= 0) or np.any(np.diff(eo) <= 0):
            raise ValueError('every video needs at least one feature row and one event')
        vid = np.asarray(self.vid)
        N = int(eo[-1])
        if len(vid) != N or len(self.soi) != N or len(self.ind) != N:
            raise ValueError('vid / soi / ind must have one entry per event (%d)' % N)
        if np.any(np.diff(vid) < 0):
            raise ValueError('events of a video must be contiguous and videos must keep their order (vid non-decreasing)')
        if not np.array_equal(vid, np.repeat(np.arange(V), np.diff(eo))):
            raise ValueError('vid does not match event_offset')
        lo, hi = ro[vid], ro[vid + 1]
        if np.any(self.soi[:, 1] <= self.soi[:, 0]) or np.any(self.soi[:, 0] < lo) or np.any(self.soi[:, 1] > hi) or \
                np.any(self.ind < lo) or np.any(self.ind >= hi):
            raise ValueError('an event interval / anchor falls outside the feature rows of its video')
        if int(ro[-1]) != self.c3d.shape[0] or self.c3d.shape[0] != self.tap.shape[0] or self.lda.shape[0] != V:
            raise ValueError('feature tensors do not match the offsets')
        if (self.labels is None) != (self.masks is None):
            raise ValueError('labels and masks come together')
        if self.labels is not None and (tuple(self.labels.shape) != tuple(self.masks.shape) or self.labels.shape[0] != N):
            raise ValueError('labels / masks must be [%d events, L]' % N)

    # ---- views --------------------------------------------------------------------------------------------------------------
    @property
    def n_events(self):
        return int(self.event_offset[-1])

    @property
    def device(self):
        return self.c3d.device

    @property
    def event_slices(self):
        eo = self.event_offset
        return [slice(int(eo[v]), int(eo[v + 1])) for v in range(self.n_videos)]

    def split(self, x):
        """Cut a [N_tot, ...] result (tensor or array) into its per-video pieces."""
        if len(x) != self.n_events:
            raise ValueError('split() takes a result with one row per event (%d), got %d' % (self.n_events, len(x)))
        return [x[s] for s in self.event_slices]

    def event_groups(self, G):
        """Cut the video axis into runs of consecutive videos whose events number at most `G` together: a list of (v0, v1, e0, e1) -- videos
        [v0, v1), events [e0, e1) -- in order, every video in exactly one run.  A video with more than G events is a run of its own.  The
        inference pass runs the event encoder once per run (CaptionGenerator.forward_batch(event_group_rows=G)), so its pair work and
        workspace are bounded by G * N_tot instead of N_tot^2."""
        G = int(G)
        if G < 1:
            raise ValueError('event_group_rows must be a positive number of events (got %r)' % (G,))
        eo, V = self.event_offset, self.n_videos
        runs, v0 = [], 0
        while v0 < V:
            v1 = v0 + 1
            while v1 < V and eo[v1 + 1] - eo[v0] <= G:
                v1 += 1
            runs.append((v0, v1, int(eo[v0]), int(eo[v1])))
            v0 = v1
        return runs

    def beam_groups(self, beam_size, max_rows):
        """The runs of a beam decode (CaptionGenerator.beam_batch): consecutive videos whose events * beam_size decoder rows number at most
        `max_rows` together, as (v0, v1, e0, e1) like event_groups.  A video above the budget is a run of its own; max_rows=None is one
        run over the batch.  The chain keeps seq_length + 1 states per row, so the budget bounds the decode's workspace."""
        B = int(beam_size)
        if B < 1:
            raise ValueError('beam_size must be positive (got %r)' % (beam_size,))
        if max_rows is None:
            return [(0, self.n_videos, 0, self.n_events)]
        if int(max_rows) < 1:
            raise ValueError('max_rows must be a positive number of decoder rows (got %r)' % (max_rows,))
        return self.event_groups(max(1, int(max_rows) // B))

    def video(self, v):
        """Video v as the dict of a single-video call (local indices, its own label width and step count)."""
        s, r0, r1 = self.event_slices[v], int(self.row_offset[v]), int(self.row_offset[v + 1])
        d = dict(c3d=self.c3d[r0:r1], tap=self.tap[r0:r1], lda=self.lda[v], soi=self.soi[s] - r0, ind=self.ind[s] - r0,
                 clip_context_type=self.clip_context_type, CG_init_feats_type=self.CG_init_feats_type)
        if self.labels is not None:
            w = self.steps[v] + 1          # S_v steps read label columns 0 .. S_v - 1 and target columns 1 .. S_v
            d['labels'], d['masks'] = self.labels[s, :w], self.masks[s, :w]
        return d

    def clip_rows(self):
        """The decoder's row source over the T_tot rows: c3d ('CC'), tap ('CH') or [c3d | tap] ('CC+CH'; formed once per batch by
        functional.clip_rows and cached).  It carries no graph: the decoder's backward returns d tap itself."""
        if self.clip_parts == 1:
            return self.c3d
        if self.clip_parts == 2:
            return self.tap
        if self._clip_rows is None:
            from . import functional as EF
            self._clip_rows = EF.clip_rows(self.c3d, self.tap)
        return self._clip_rows

    @property
    def clip_col0(self):
        """First tap column of clip_rows() (the decoder's d tap reads the row gradient from there)."""
        return self.c3d.shape[1] if self.clip_parts == 3 else 0

    def dev(self, name):
        """int32 device copy of 'vid' / 'row_offset' (cached)."""
        t = self._dev.get(name)
        if t is None:
            t = self._dev[name] = torch.from_numpy(np.asarray(getattr(self, name)).astype(np.int32)).to(self.device)
        return t

    @property
    def targets(self):
        return self.labels[:, 1:]

    @property
    def crit_masks(self):
        return self.masks[:, 1:]

    # ---- criterion ----------------------------------------------------------------------------------------------------------
    def criterion(self, crit, logp):
        """LanguageModelCriterion per video on the batch's log-probs [N_tot, S, V1]: returns (sum over the videos, per-video losses [V]).
        Each video keeps its own normaliser sum(mask_v) + 1e-6 (its mask is zero behind its own step count); no 1/V."""
        if self.labels is None:
            raise ValueError('the batch carries no labels')
        per = [crit(logp[s], self.targets[s], self.crit_masks[s]) for s in self.event_slices]
        per = torch.stack(per)
        return per.sum(), per

    def criterion_weights(self, S=None):
        """Per-position weights of the one-call step (host, float32 [N_tot, S]): w[n, t] = mask[n, t] / (sum(mask of video vid[n]) + 1e-6) --
        with them the batch's loss is sum(-logp[target] * w) and the per-video normalisers cannot be got wrong downstream."""
        S = self.S if S is None else S
        mk = np.ascontiguousarray(self.crit_masks.numpy()[:, :S], dtype=np.float32)
        w = np.empty_like(mk)
        for s in self.event_slices:
            w[s] = mk[s] / (mk[s].sum(dtype=np.float32) + np.float32(1e-6))
        return w

    # ---- self-critical training (CaptionGenerator.train_rl_batch, fused.SelfCriticalBatchStep) --------------------------------------
    def caption_widths(self, gen_result):
        """video_words (host int64 [V]) of sampled captions gen_result [N_tot, T]: the largest number of non-zero tokens among the rows of
        each video -- the width at which that video's own call cuts its output (it stops at the first step after which none of its rows is
        unfinished, OldModel_NEW.py:179-180)."""
        g = _np(gen_result, np.int64)
        if g.ndim != 2 or g.shape[0] != self.n_events:
            raise ValueError('gen_result must be [%d events, T] (got %s)' % (self.n_events, g.shape))
        words = (g != 0).sum(1)
        return np.asarray([int(words[s].max()) for s in self.event_slices], dtype=np.int64)

    def reward_criterion(self, crit, sample_logprobs, gen_result, reward, video_words):
        """RewardCriterion per video: `crit` on the rows of video v and its first video_words[v] columns -- the tensors that video's own
        call returns, so its longest row's <eos> position stays outside the criterion -- each video with its own normaliser sum(mask_v), no
        1/V.  A video of width 0 is skipped (its own call returns []: loss 0, no gradient).  `reward`: [N_tot, T] or [N_tot].
        Returns (sum over the videos, per-video losses [V])."""
        vw = np.asarray(video_words, dtype=np.int64).reshape(-1)
        if len(vw) != self.n_videos:
            raise ValueError('video_words needs one width per video (%d), got %d' % (self.n_videos, len(vw)))
        gen = torch.as_tensor(gen_result)
        N, T = gen.shape
        if int(vw.max()) > T or sample_logprobs.shape[0] != N or sample_logprobs.shape[1] < int(vw.max()):
            raise ValueError('video_words %s exceed gen_result %s / sample_logprobs %s' % (vw.tolist(), (N, T), tuple(sample_logprobs.shape)))
        r = torch.from_numpy(np.ascontiguousarray(reward_matrix(reward, N, T)))
        per = []
        for s, w in zip(self.event_slices, vw.tolist()):
            if w == 0:
                per.append(sample_logprobs.new_zeros(()))
            else:
                per.append(crit(sample_logprobs[s, :w].contiguous(), gen[s, :w].contiguous(), r[s, :w].contiguous()))
        per = torch.stack(per)
        return per.sum(), per

    def reward_weights(self, gen_result, reward, video_words):
        """The criterion of reward_criterion as the one-call step takes it (host arrays): labels, mask and reward * mask of
        `sampled_criterion` over the batch's videos, the weights divided by each video's own sum(mask) --
        w[n, t] = reward[n, t] * mask[n, t] / sum(mask of video vid[n]): the loss is sum(-logp[target] * w) with denominator 1."""
        g = _np(gen_result, np.int64)
        vw = np.asarray(video_words, dtype=np.int64).reshape(-1)
        if g.ndim != 2 or g.shape[0] != self.n_events or len(vw) != self.n_videos:
            raise ValueError('gen_result must be [%d events, T] and video_words [%d]' % (self.n_events, self.n_videos))
        slices = self.event_slices
        labels, mask, w = sampled_criterion(g, reward, vw, slices)
        for s, wv in zip(slices, vw.tolist()):
            if wv:
                w[s, :wv] /= mask[s, :wv].sum(dtype=np.float32)
        return labels, mask, w

"""SST proposal encoder -- the PRODUCER of `tap_feats` for the caption path (reference: models/sst_model.py:5-40;
SURVEY section 8-f row 1).

Parameter names (`rnn.weight_ih_l0` ..., `scores.*`) are nn.LSTM's / nn.Linear's, so the reference's checkpoints load.
On the GPU the arithmetic runs in libechr_hip.so (echr_sst_fwd / echr_sst_bwd: batched input GEMMs + one fused
GEMV+cell launch per timestep); the nn.LSTM module is only the parameter container.  On CPU tensors it falls back to
nothing -- like the rest of echr_amd it raises.
"""
import torch
from torch import nn

from .. import functional as EF


class SST(nn.Module):
    """2-layer LSTM over the C3D segment sequence + a K-way sigmoid head (K anchor lengths ending at every segment)."""

    def __init__(self, opt):
        super().__init__()
        self.K = opt.K
        self.video_dim = opt.video_dim
        self.rnn_type = opt.tap_rnn_type
        self.rnn_num_layers = opt.rnn_num_layers
        self.rnn_dropout = opt.rnn_dropout
        self.data_for_test = []
        if opt.rnn_num_layers != 2 or str(opt.tap_rnn_type).upper() != 'LSTM':
            raise NotImplementedError('the HIP path implements the shipped SST: a 2-layer LSTM (opts.py:72-78)')
        self.scores = nn.Linear(opt.hidden_dim, self.K)
        self.rnn = nn.LSTM(input_size=opt.video_dim, hidden_size=opt.hidden_dim, num_layers=opt.rnn_num_layers,
                           dropout=opt.rnn_dropout, batch_first=True)
        self._drop_seed = None
        self._drop_calls = 0
        self._ro_cache = {}

    # The reference overrides train()/eval() so that they ONLY switch the LSTM's inter-layer dropout (sst_model.py:25-29);
    # module.training is left alone on purpose.
    def _set_dropout(self, on):
        self.rnn.dropout = self.rnn_dropout if on else 0

    def train(self, mode=True):
        self._set_dropout(bool(mode))

    def eval(self):
        self._set_dropout(False)

    def set_dropout_state(self, seed, calls=0):
        self._drop_seed, self._drop_calls = int(seed), int(calls)

    def native_params(self):
        r = self.rnn
        return (r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0, r.weight_ih_l1, r.weight_hh_l1, r.bias_ih_l1, r.bias_hh_l1,
                self.scores.weight, self.scores.bias)

    def _next_drop(self):
        """(p, DropState) of the inter-layer dropout for this call, and the counter moves on: ONE counter per call, over a batch too (the mask
        is keyed by the batch-global row)."""
        p = float(self.rnn.dropout)
        if self._drop_seed is None:
            self._drop_seed = (int(torch.initial_seed()) ^ 0x55AA) & 0xFFFFFFFFFFFFFFFF
        drop = EF.DropState(self._drop_seed, self._drop_calls, p > 0.0)
        if p > 0.0:
            self._drop_calls += 1
        return p, drop

    def row_offsets_dev(self, ro, device):
        """Device copy of validated offsets (EF.sst_row_offsets), kept for the batches a training loop repeats: a pageable host-to-device copy
        synchronises the stream."""
        key = (ro.tobytes(), str(device))
        ro_dev = self._ro_cache.get(key)
        if ro_dev is None:
            if len(self._ro_cache) >= 64:
                self._ro_cache.clear()
            ro_dev = self._ro_cache[key] = torch.from_numpy(ro).to(device)
        return ro_dev

    def _run(self, features, ro=None):
        """SSTFunction on one video (ro None) or on a batch with its validated offsets."""
        p, drop = self._next_drop()
        arena = getattr(self, '_echr_arena', None)
        sink = EF.GradSink(arena, self.native_params()) if arena is not None else None
        ro_dev = self.row_offsets_dev(ro, features.device) if ro is not None else None
        return EF.SSTFunction.apply(features, ro, ro_dev, p, drop, sink, *self.native_params())

    def forward(self, features):
        """features [T, video_dim] -> (tap_feats [T, hidden_dim], proposal scores [T, K] in (0,1))."""
        if not features.is_cuda:
            raise EF.L.EchrHipError('SST runs on the GPU only: move the module and its inputs with .cuda()')
        return self._run(features)

    def forward_batch(self, features, row_offset=None):
        """The encoder over V videos in one call.  `features`: the concatenated [T_tot, video_dim] matrix with `row_offset` [V+1] (video v owns
        rows row_offset[v] .. row_offset[v+1]), or a list of per-video [T_v, video_dim] matrices (then row_offset is derived).  Returns
        (tap_feats [T_tot, hidden_dim], scores [T_tot, K]) in the same layout: the rows of a video equal forward() on that video alone (every
        video starts from the zero state), parameter gradients are the sum over the videos.  One dropout counter per call; the mask is keyed
        by the batch-global row, so a one-video batch equals forward()."""
        if isinstance(features, (list, tuple)):
            if row_offset is not None:
                raise ValueError('row_offset comes with a concatenated matrix, not with a list of videos')
            if not features:
                raise ValueError('a batch needs at least one video')
            if any((not isinstance(f, torch.Tensor)) or f.dim() != 2 for f in features):
                raise ValueError('every video must be a [T, video_dim] tensor')
            row_offset = [0]
            for f in features:
                row_offset.append(row_offset[-1] + f.shape[0])
            ro = EF.sst_row_offsets(row_offset, row_offset[-1])
            if not all(f.is_cuda for f in features):
                raise EF.L.EchrHipError('SST runs on the GPU only: move the module and its inputs with .cuda()')
            features = torch.cat(list(features), 0)
        else:
            if row_offset is None:
                raise ValueError('a concatenated feature matrix needs its row_offset')
            if features.dim() != 2:
                raise ValueError('features must be a [T_tot, video_dim] matrix')
            ro = EF.sst_row_offsets(row_offset, features.shape[0])
            if not features.is_cuda:
                raise EF.L.EchrHipError('SST runs on the GPU only: move the module and its inputs with .cuda()')
        if len(ro) == 2:
            return self.forward(features)          # one video: today's call (the library's batch entries reduce to it as well)
        return self._run(features, ro)

    def build_arena(self):
        """Pack parameters and gradients into flat device buffers (echr_amd/arena.py): ClampAdam(..., arena=...) then updates the whole
        proposal encoder in ONE launch, as CaptionGenerator.build_arena() does for the caption path.  Call after .cuda()."""
        from ..arena import ParamArena
        return ParamArena(self)

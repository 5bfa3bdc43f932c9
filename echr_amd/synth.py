"""Synthetic options, parameters and video batches for the ECHR caption hot path.

There is no dataset in this environment, so tests, golden fixtures and bench.py all draw their
inputs from `np.random.RandomState` streams defined here (portable between the build container
and the GPU box).  Shapes follow the ECHR recipe (reference: experiments/train_ECHR.sh:5 and the
defaults in opts.py:81-161): the batch axis is the N events of ONE video (opts.py:93,187).
"""
import math
from types import SimpleNamespace

import numpy as np


def default_opt(vocab_size=5000, seq_length=19, **over):
    """The option namespace CaptionGenerator reads, at the values train_ECHR.sh selects."""
    opt = SimpleNamespace(
        caption_model='three_stream', CG_num_layers=3,
        video_context_type='VL', event_context_type='ER3', clip_context_type='CC',
        lda_dim=100, video_dim=500, hidden_dim=512,
        fusion_model='TSRM8', use_posit=1, n_head=16, d_feats=512, d_o=512, fST_type='fST0',
        CG_rnn_size=512, CG_rnn_type='lstm', CG_input_encoding_size=512, CG_att_hid_size=512,
        CG_fc_feat_size=512, CG_drop_prob=0.5, CG_input_feats_type='', CG_init_feats_type='',
        CG_vocab_size=vocab_size, CG_seq_length=seq_length,
        video_context_dim=0, event_context_dim=0, clip_context_dim=0,
        K=256, tap_model='SST', tap_rnn_type='LSTM', rnn_num_layers=2, rnn_dropout=0.5,
        grad_clip=100.0, lr=5e-5, optim_alpha=0.9, optim_beta=0.999, optim_epsilon=1e-8, weight_decay=0,
    )
    for k, v in over.items():
        setattr(opt, k, v)
    return opt


def state_dict_shapes(opt):
    """Name -> shape of CaptionGenerator.state_dict() (printed from the reference)."""
    V1 = opt.CG_vocab_size + 1
    H = opt.CG_rnn_size
    E = opt.CG_input_encoding_size
    Ha = opt.CG_att_hid_size
    D = opt.video_dim
    Df = opt.d_feats
    G = opt.n_head
    et = opt.event_context_type                       # TSRM input (MA_attention_8_NEW.py:13-20): ER1 pooled C3D, ER2 SST state, ER3 both
    tsrm_in = opt.video_dim if 'ER1' in et else (opt.hidden_dim if 'ER2' in et else opt.video_dim + opt.hidden_dim)
    vt = opt.video_context_type
    vi = (opt.lda_dim if 'VL' in vt else 0) + (opt.video_dim if 'VC' in vt else 0) + (opt.hidden_dim if 'VH' in vt else 0)
    ct = getattr(opt, 'clip_context_type', 'CC')      # frame-level rows: 'CC' C3D, 'CH' the SST states, 'CC+CH' both (CaptionGenerator.py:80-84)
    # event context width (:66-74): d_o behind the event encoder; 'EC' the pooled C3D rows, 'EH' the anchor's SST state -- no fusion_model.* keys
    direct = 'ER' not in et
    ev_w = opt.d_o if not direct else (opt.video_dim if 'EC' in et else 0) + (opt.hidden_dim if 'EH' in et else 0)
    ev, cl = ev_w, (opt.video_dim if 'CC' in ct else 0) + (opt.hidden_dim if 'CH' in ct else 0)      # context widths; vi: VL / VC / VH (:56-64)
    s = {
        'fusion_model.h2a_layer.weight': (10, 10), 'fusion_model.h2a_layer.bias': (10,),
        'fusion_model.event_emb.weight': (Df, tsrm_in), 'fusion_model.event_emb.bias': (Df,),
        'fusion_model.enc_attn.pair_pos_fc1.weight': (Df, Df), 'fusion_model.enc_attn.pair_pos_fc1.bias': (Df,),
        'fusion_model.enc_attn.pair_pos_fc2.weight': (G, Df), 'fusion_model.enc_attn.pair_pos_fc2.bias': (G,),
        'fusion_model.enc_attn.query_1.weight': (Df, Df), 'fusion_model.enc_attn.query_1.bias': (Df,),
        'fusion_model.enc_attn.key_1.weight': (Df, Df), 'fusion_model.enc_attn.key_1.bias': (Df,),
        'fusion_model.enc_attn.linear_out_1.weight': (opt.d_o, Df, 1, 1), 'fusion_model.enc_attn.linear_out_1.bias': (opt.d_o,),
        'lm_model.embed.weight': (V1, E),
        'lm_model.logit.weight': (V1, 3 * H), 'lm_model.logit.bias': (V1,),
    }
    if direct:
        s = {k: v for k, v in s.items() if not k.startswith('fusion_model.')}
    it = getattr(opt, 'CG_init_feats_type', '')       # non-zero initial state (OldModel_NEW.py:38-39,55-63): Linear(selected context widths -> 3H)
    init_in = (vi if 'V' in it else 0) + (ev if 'E' in it else 0) + (cl if 'C' in it else 0)
    if init_in:
        s['lm_model.init_linear.weight'] = (3 * H, init_in)
        s['lm_model.init_linear.bias'] = (3 * H,)
    for k, cin in ((0, ev + E), (1, cl + E), (2, vi + E)):
        s['lm_model.core.layer%d.weight_ih' % k] = (4 * H, cin)
        s['lm_model.core.layer%d.weight_hh' % k] = (4 * H, H)
        s['lm_model.core.layer%d.bias_ih' % k] = (4 * H,)
        s['lm_model.core.layer%d.bias_hh' % k] = (4 * H,)
    s.update({
        'lm_model.core.fusion_layer.weight': (H, 3 * H), 'lm_model.core.fusion_layer.bias': (H,),
        'lm_model.core.attention.ctx2att.weight': (Ha, cl), 'lm_model.core.attention.ctx2att.bias': (Ha,),
        'lm_model.core.attention.h2att.weight': (Ha, H), 'lm_model.core.attention.h2att.bias': (Ha,),
        'lm_model.core.attention.alpha_net.weight': (1, Ha), 'lm_model.core.attention.alpha_net.bias': (1,),
    })
    return s


def _init_range(name, shapes, H):
    if name in ('lm_model.embed.weight', 'lm_model.logit.weight'):
        return 0.1                                    # OldModel_NEW.py:66-70
    if name == 'lm_model.logit.bias':
        return 0.0
    if '.core.layer' in name:
        return 1.0 / math.sqrt(H)                     # nn.LSTMCell default
    wname = name[:-len('.bias')] + '.weight' if name.endswith('.bias') else name
    fan_in = int(np.prod(shapes[wname][1:]))          # nn.Linear / Conv2d: bound = 1/sqrt(fan_in)
    return 1.0 / math.sqrt(fan_in)


def make_params(opt, seed=0):
    """Deterministic parameter set keyed by state-dict name (float32 numpy arrays).

    Filled in sorted-name order from one RandomState so that the reference-side golden tool and
    the build draw identical values without storing any weights."""
    rs = np.random.RandomState(seed)
    out = {}
    shapes = state_dict_shapes(opt)
    for name in sorted(shapes):
        shp = shapes[name]
        r = _init_range(name, shapes, opt.CG_rnn_size)
        out[name] = rs.uniform(-r, r, size=shp).astype(np.float32) if r > 0 else np.zeros(shp, np.float32)
    return out


def make_video(N, A, L, V1, seed=1234, T_v=None, full_len=False, min_len=4, video_dim=500, hidden_dim=512, lda_dim=100, disjoint=False):
    """One synthetic video: features, N events (half-open [s,e) segment intervals), captions.

    full_len=True makes every event exactly A segments long (the dense N x A x D case BASELINE
    quotes); otherwise lengths are uniform in [min_len, A] with at least one event of length A
    (SURVEY 8-d config 2).  Captions: column 0 = BOS (0), tokens in [1, V1), zero padded; at least
    one caption uses all L-2 token slots so the decoder runs the full L-1 steps.  disjoint=True lays the events out
    back to back on a T_v = N*A video (every event owns its own A feature rows: the dense [N x A x D] block).  The mask follows
    dataloader.py:437-439 (`nonzeros + 2` ones)."""
    rs = np.random.RandomState(seed)
    if disjoint:                      # N non-overlapping events of A segments: N*A distinct feature rows
        full_len, T_v = True, N * A
    if T_v is None:
        T_v = A + max(8, A // 4)
    lens = np.full(N, A, dtype=np.int64) if full_len else rs.randint(min(min_len, A), A + 1, size=N)
    lens[rs.randint(0, N)] = A
    starts = np.array([rs.randint(0, T_v - l + 1) for l in lens], dtype=np.int64)
    if disjoint:
        starts = np.arange(N, dtype=np.int64) * A
    soi = np.stack([starts, starts + lens], axis=1)
    ind = soi[:, 1] - 1                                   # proposal anchored at its last segment
    c3d = rs.standard_normal((T_v, video_dim)).astype(np.float32)
    tap = (0.5 * rs.standard_normal((T_v, hidden_dim))).astype(np.float32)
    lda = np.abs(rs.standard_normal(lda_dim)).astype(np.float32)
    lda /= lda.sum()
    labels = np.zeros((N, L), dtype=np.int64)
    masks = np.zeros((N, L), dtype=np.float32)
    max_tok = L - 2
    cap_len = rs.randint(1, max_tok + 1, size=N) if max_tok >= 1 else np.zeros(N, np.int64)
    if max_tok >= 1:
        cap_len[rs.randint(0, N)] = max_tok
    for i in range(N):
        labels[i, 1:1 + cap_len[i]] = rs.randint(1, V1, size=cap_len[i])
        masks[i, :cap_len[i] + 2] = 1.0
    return dict(c3d=c3d, tap=tap, lda=lda, labels=labels, masks=masks,
                ind=ind.astype(np.int64), soi=soi.astype(np.int64), T_v=T_v)


def make_gt_video(T_v, G, L, V1, seed=1234, min_len=2, max_len=None, video_dim=500, hidden_dim=512, lda_dim=100):
    """One synthetic ANNOTATED video, as a dataset gives it: features and G ground-truth segments with one caption each -- no proposal
    labels and no event lists; echr_amd.targets.build makes those.  'featstamps' int64 [G, 2]: integer (start, end) rows with
    0 <= start < end <= T_v - 1 and end - start in [min_len, max_len] (default: up to T_v - 1; segment 0 is the longest allowed);
    'gt_labels' int64 [G, L] / 'gt_masks' float32 [G, L] in make_video's caption layout (column 0 = BOS, `nonzeros + 2` ones);
    'c3d', 'tap', 'lda', 'T_v' as make_video.  L >= 3; T_v >= 2 when G > 0 (a one-row video admits no segment)."""
    rs = np.random.RandomState(seed)
    max_len = T_v - 1 if max_len is None else min(int(max_len), T_v - 1)
    min_len = max(1, min(int(min_len), max_len))
    lens = rs.randint(min_len, max_len + 1, size=G)
    if G:
        lens[0] = max_len
    starts = np.array([rs.randint(0, T_v - l) for l in lens], dtype=np.int64).reshape(-1)
    stamps = np.stack([starts, starts + lens], 1).astype(np.int64).reshape(-1, 2)
    c3d = rs.standard_normal((T_v, video_dim)).astype(np.float32)
    tap = (0.5 * rs.standard_normal((T_v, hidden_dim))).astype(np.float32)
    lda = np.abs(rs.standard_normal(lda_dim)).astype(np.float32)
    lda /= lda.sum()
    labels = np.zeros((G, L), dtype=np.int64)
    masks = np.zeros((G, L), dtype=np.float32)
    for i in range(G):
        n = int(rs.randint(1, L - 1)) if i else L - 2          # caption 0 uses all L - 2 token slots
        labels[i, 1:1 + n] = rs.randint(1, V1, size=n)
        masks[i, :n + 2] = 1.0
    return dict(c3d=c3d, tap=tap, lda=lda, featstamps=stamps, gt_labels=labels, gt_masks=masks, T_v=T_v)


# Named parity / bench cases (BASELINE.json `configs`).  `opt` = overrides of default_opt.
CASES = {
    # every width shrunk (all multiples of 4) so that full tensors fit in a fixture
    'tiny': dict(opt=dict(video_dim=20, hidden_dim=24, lda_dim=12, d_feats=32, d_o=32, n_head=4, CG_rnn_size=32,
                          CG_input_encoding_size=16, CG_att_hid_size=24, CG_vocab_size=30, CG_seq_length=5),
                 video=dict(N=3, A=7, L=7, seed=11)),
    # config 1: N=2 events on a 16-segment video, 10 decoder steps, ECHR widths, V1 = 5001
    'c1': dict(opt=dict(CG_vocab_size=5000, CG_seq_length=9), video=dict(N=2, A=16, L=11, seed=21, T_v=16)),
    # config 2/3 shape with ragged event lengths in [4,128]
    'c2': dict(opt=dict(CG_vocab_size=5000, CG_seq_length=19), video=dict(N=64, A=128, L=21, seed=31)),
    # config 2/3 shape, every event 128 segments long (the dense batch 64 x 128 seg x 500-d bench workload)
    'c2full': dict(opt=dict(CG_vocab_size=5000, CG_seq_length=19), video=dict(N=64, A=128, L=21, seed=41, full_len=True)),
    # scene context from all three sources (CaptionGenerator.py:87-104): cat(lda, c3d.mean(0), tap.mean(0)), 100 + 500 + 512 wide
    'vctx': dict(opt=dict(video_context_type='VLVCVH', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=61)),
    # event-context variants (CaptionGenerator.py:106-130): TSRM over the pooled C3D rows only / the anchors' SST states only
    'er1': dict(opt=dict(event_context_type='ER1', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=62)),
    'er2': dict(opt=dict(event_context_type='ER2', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=63)),
    # gate / affinity combinators of the event encoder (MA_attention_8_NEW.py:148-157) and the encoder without its position branch
    'fst1': dict(opt=dict(fST_type='fST1', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=64)),
    # (fST2 takes log(clamp(gate, 1e-6)): a gate just above zero amplifies the documented 1-ulp deviation of the device's position embedding by
    # 1 / gate, so the case keeps its gates away from zero -- heads 0..7 shifted by +1 (gates 0.36 .. 1.73), heads 8..15 by -1 (all clamped))
    'fst2': dict(opt=dict(fST_type='fST2', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=65), gate_shift=1.0),
    'fst3': dict(opt=dict(fST_type='fST3', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=66)),
    'noposit': dict(opt=dict(use_posit=0, CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=67)),
    # non-zero initial decoder state (OldModel_NEW.py:79-96): h(-1) = c(-1) = init_linear(cat([scene | event | clip.mean(1)])), ragged events so
    # that the mean over the PADDED frame slots differs from a mean over each event's own rows
    'init': dict(opt=dict(CG_init_feats_type='VEC', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=68)),
    'initc': dict(opt=dict(CG_init_feats_type='C', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=69)),
    # self-critical training with captions that end at different steps (tests/golden/case_scst_eos.npz): the 'tiny' widths with more events
    # and steps; tools/make_golden_scst.py picks the reference's draw seed whose rows finish at three or more different steps
    'tiny_eos': dict(opt=dict(video_dim=20, hidden_dim=24, lda_dim=12, d_feats=32, d_o=32, n_head=4, CG_rnn_size=32,
                              CG_input_encoding_size=16, CG_att_hid_size=24, CG_vocab_size=30, CG_seq_length=6),
                     video=dict(N=8, A=7, L=8, seed=13)),
    # frame-level context over the proposal encoder's states (CaptionGenerator.py:140-167): 'CH' (the clip rows are tap_feats, D = 512) and
    # 'CC+CH' (c3d and tap rows side by side, D = 1012) at the vctx / er2 shape; 'ch64': 'CH' at the ECHR widths with 64 ragged, overlapping
    # events (c2-like), where D = 512 runs the persistent recurrence and decoding kernels
    'ch': dict(opt=dict(clip_context_type='CH', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=71)),
    'cch': dict(opt=dict(clip_context_type='CC+CH', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=72)),
    'ch64': dict(opt=dict(clip_context_type='CH', CG_vocab_size=5000, CG_seq_length=19), video=dict(N=64, A=128, L=21, seed=73)),
    # the event vector without the event encoder (CaptionGenerator.py:131-137): 'EC' the mean of the event's C3D rows (layer0.weight_ih is
    # [4H, E + 500]), 'EH' the proposal encoder's state at the anchor ([4H, E + 512]); no fusion_model.* parameters
    'ec': dict(opt=dict(event_context_type='EC', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=74)),
    'eh': dict(opt=dict(event_context_type='EH', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=75)),
    # EXACTLY the layout bench.py times (BASELINE config 3): 64 disjoint 128-segment events on a T_v = 8192 video
    'c3bench': dict(opt=dict(CG_vocab_size=5000, CG_seq_length=19), video=dict(N=64, A=128, L=21, seed=1234, disjoint=True)),
}


# The one-stream decoder (caption_model='show_attend_tell', one LSTM layer: echr_amd.sat).  `opt` = overrides of default_opt; the context
# widths follow CaptionGenerator.change_context_dim.
#   sat_tiny   the 'tiny' widths and video, input [token | video | event | attended clip]
#   the others at N = 12, A = 40, V1 = 301, seq_length 7 (tests/golden/case_sat.npz): 'C' alone; 'E' alone (the attention is computed by the
#   reference and never read: its parameters get no gradient); 'VE'; 'VEC' from a non-zero initial state; 'VEC' with the event vector and the
#   scene context reading the proposal encoder's states (gradients into tap_feats)
_SAT = dict(caption_model='show_attend_tell', CG_num_layers=1)
SAT_CASES = {
    'sat_tiny': dict(opt=dict(_SAT, CG_input_feats_type='VEC', video_dim=20, hidden_dim=24, lda_dim=12, d_feats=32, d_o=32, n_head=4, CG_rnn_size=32,
                              CG_input_encoding_size=16, CG_att_hid_size=24, CG_vocab_size=30, CG_seq_length=5),
                     video=dict(N=3, A=7, L=7, seed=11)),
    'sat_c': dict(opt=dict(_SAT, CG_input_feats_type='C', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=101)),
    'sat_e': dict(opt=dict(_SAT, CG_input_feats_type='E', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=102)),
    'sat_ve': dict(opt=dict(_SAT, CG_input_feats_type='VE', CG_vocab_size=300, CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=103)),
    'sat_vec_init': dict(opt=dict(_SAT, CG_input_feats_type='VEC', CG_init_feats_type='VEC', CG_vocab_size=300, CG_seq_length=7),
                         video=dict(N=12, A=40, L=9, seed=104)),
    'sat_vec_eh': dict(opt=dict(_SAT, CG_input_feats_type='VEC', event_context_type='EH', video_context_type='VLVCVH', CG_vocab_size=300,
                                CG_seq_length=7), video=dict(N=12, A=40, L=9, seed=105)),
}


def sat_state_dict_shapes(opt):
    """Name -> shape of CaptionGenerator.state_dict() with caption_model='show_attend_tell' (printed from the reference: models/OldModel_NEW.py
    :36-51, :190-216): the event encoder's keys as in state_dict_shapes, then embed, logit [V1, H], init_linear [L*H, .], core.rnn.* (no
    biases) and the three attention projections directly under core."""
    s = {k: v for k, v in state_dict_shapes(opt).items() if k.startswith('fusion_model.')}
    V1, H, E, Ha, nl = opt.CG_vocab_size + 1, opt.CG_rnn_size, opt.CG_input_encoding_size, opt.CG_att_hid_size, opt.CG_num_layers
    vt, et, ct = opt.video_context_type, opt.event_context_type, getattr(opt, 'clip_context_type', 'CC')
    vi = (opt.lda_dim if 'VL' in vt else 0) + (opt.video_dim if 'VC' in vt else 0) + (opt.hidden_dim if 'VH' in vt else 0)
    ev = opt.d_o if 'ER' in et else (opt.video_dim if 'EC' in et else 0) + (opt.hidden_dim if 'EH' in et else 0)
    cl = (opt.video_dim if 'CC' in ct else 0) + (opt.hidden_dim if 'CH' in ct else 0)
    width = lambda t: (vi if 'V' in t else 0) + (ev if 'E' in t else 0) + (cl if 'C' in t else 0)
    s.update({'lm_model.embed.weight': (V1, E), 'lm_model.logit.weight': (V1, H), 'lm_model.logit.bias': (V1,)})
    if width(getattr(opt, 'CG_init_feats_type', '')):
        s['lm_model.init_linear.weight'] = (nl * H, width(opt.CG_init_feats_type))
        s['lm_model.init_linear.bias'] = (nl * H,)
    for l in range(nl):
        s['lm_model.core.rnn.weight_ih_l%d' % l] = (4 * H, E + width(opt.CG_input_feats_type) if l == 0 else H)
        s['lm_model.core.rnn.weight_hh_l%d' % l] = (4 * H, H)
    s.update({'lm_model.core.ctx2att.weight': (Ha, cl), 'lm_model.core.ctx2att.bias': (Ha,),
              'lm_model.core.h2att.weight': (Ha, H), 'lm_model.core.h2att.bias': (Ha,),
              'lm_model.core.alpha_net.weight': (1, Ha), 'lm_model.core.alpha_net.bias': (1,)})
    return s


def make_sat_params(opt, seed=0):
    """make_params for the one-stream decoder: sorted-name order from one RandomState, the reference's initial ranges (embed / logit +-0.1,
    nn.LSTM and nn.Linear +-1/sqrt(fan))."""
    rs = np.random.RandomState(seed)
    shapes = sat_state_dict_shapes(opt)
    out = {}
    for name in sorted(shapes):
        shp = shapes[name]
        r = 1.0 / math.sqrt(opt.CG_rnn_size) if '.core.rnn.' in name else _init_range(name, shapes, opt.CG_rnn_size)
        out[name] = rs.uniform(-r, r, size=shp).astype(np.float32) if r > 0 else np.zeros(shp, np.float32)
    return out


def make_sat_case(name, param_seed=0, video_seed=None):
    """(opt, params, video) of a named one-stream case; `video_seed` replaces the case's own (tools/make_golden_sat.py picks it)."""
    c = SAT_CASES[name]
    opt = default_opt(**c['opt'])
    vd = dict(c['video'])
    if video_seed is not None:
        vd['seed'] = video_seed
    vid = make_video(V1=opt.CG_vocab_size + 1, video_dim=opt.video_dim, hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim, **vd)
    return opt, make_sat_params(opt, param_seed), vid


def sst_param_shapes(opt):
    """Name -> shape of SST.state_dict() (models/sst_model.py:12,22-23: nn.LSTM(video_dim, hidden_dim, 2 layers) + Linear(hidden_dim, K))."""
    H, D, K = opt.hidden_dim, opt.video_dim, opt.K
    s = {}
    for l, cin in ((0, D), (1, H)):
        s['rnn.weight_ih_l%d' % l] = (4 * H, cin)
        s['rnn.weight_hh_l%d' % l] = (4 * H, H)
        s['rnn.bias_ih_l%d' % l] = (4 * H,)
        s['rnn.bias_hh_l%d' % l] = (4 * H,)
    s['scores.weight'] = (K, H)
    s['scores.bias'] = (K,)
    return s


def make_sst_params(opt, seed=7):
    rs = np.random.RandomState(seed)
    r = 1.0 / math.sqrt(opt.hidden_dim)
    shapes = sst_param_shapes(opt)
    return {k: rs.uniform(-r, r, size=shapes[k]).astype(np.float32) for k in sorted(shapes)}


def make_c5(seed=51, N=64, T_v=256, L=21, V1=5001):
    """BASELINE config 5: ONE 256-segment video; SST proposal encoder over all 256 segments -> tap_feats -> caption path on N
    proposals of 4..256 segments (at least one spans the whole video), joint loss lambda1 * tap + lambda2 * cg (train.py:322-329).
    Returns (opt, caption params, SST params, video dict incl. the proposal-loss inputs)."""
    opt = default_opt(vocab_size=V1 - 1, seq_length=L - 2)
    opt.lambda1, opt.lambda2 = 0.01, 1.0                   # opts.py:194-196
    vid = make_video(N, T_v, L, V1, seed=seed, T_v=T_v)
    rs = np.random.RandomState(seed + 1000)
    vid['tap_labels'] = (rs.uniform(size=(T_v, opt.K)) > 0.9).astype(np.float32)
    vid['tap_masks'] = (np.arange(T_v)[:, None] >= np.arange(opt.K)[None, :]).astype(np.float32)
    vid['w1'] = rs.uniform(0.05, 0.3, size=(opt.K,)).astype(np.float32)
    return opt, make_params(opt, 0), make_sst_params(opt), vid


def make_case(name, param_seed=0):
    """(opt, params, video) of a named case."""
    c = CASES[name]
    opt = default_opt(**c['opt'])
    vid = make_video(V1=opt.CG_vocab_size + 1, video_dim=opt.video_dim, hidden_dim=opt.hidden_dim,
                     lda_dim=opt.lda_dim, **c['video'])
    params = make_params(opt, param_seed)
    if c.get('gate_shift'):
        b = params['fusion_model.enc_attn.pair_pos_fc2.bias']
        b[:len(b) // 2] += np.float32(c['gate_shift'])
        b[len(b) // 2:] -= np.float32(c['gate_shift'])
    return opt, params, vid


# Greedy-decoding cases whose captions END AT DIFFERENT STEPS (OldModel_NEW.py:171-183: per-row `unfinished` state).  With the plain
# synthetic initialisation a caption ends at its first word or never; here the token embedding is scaled up (the recurrences become
# token-driven, so the <eos> margin moves from step to step) and the <eos> row of the logit layer is widened.  The event lists of the
# fixtures (tests/golden/case_eosmix.npz: `soi`, `ind`) are selections / re-orderings of the video made here, chosen by
# tools/make_golden.py from the reference's own decode: 'b' puts the 64 earliest-finishing events first (one 64-event group is done
# long before the others), 'c' keeps only events that finish (the whole batch stops before seq_length).
EOSMIX = {
    'a': dict(N=64, seed=109, eos_scale=2.0),
    'b': dict(N=150, seed=322, eos_scale=2.5),
    'c': dict(N=150, seed=322, eos_scale=2.5),
}


def make_eosmix(name, A=24, embed_scale=10.0):
    """(opt, params, video) of a mixed-finish decoding case at the ECHR widths (V1 = 5001, seq_length 19)."""
    c = EOSMIX[name]
    opt = default_opt(vocab_size=5000, seq_length=19)
    params = make_params(opt, 0)
    params['lm_model.embed.weight'] = (params['lm_model.embed.weight'] * np.float32(embed_scale)).astype(np.float32)
    params['lm_model.logit.weight'][0] *= np.float32(c['eos_scale'])
    vid = make_video(c['N'], A, 21, 5001, seed=c['seed'], T_v=4 * A)
    return opt, params, vid


# Training in the PEAKED regime: a trained captioner's softmax puts > 0.9 of its mass on one word at most positions, so d logits =
# softmax - onehot spans dozens of binades inside one row (and inside one 256-wide k segment of the h2 operand format), which the
# random-initialisation cases (near-uniform softmax) never exercise.  Weights cannot be trained here and shipped (fixtures store no
# weights), so the regime is constructed: the logit layer is scaled up (every row's soft-max collapses onto its arg-max) and the token
# embedding too (token-driven recurrences: the peak moves from step to step); the CAPTIONS are then chosen so that most positions'
# target IS that arg-max -- tools/make_golden.py do_peaked runs the reference's own teacher-forced forward (train mode, the build's
# dropout masks) to its fixed point and stores labels / masks in tests/golden/case_peaked.npz; one row in ten keeps a random word
# (a confidently wrong prediction: loss terms of ~100, d logits of -1 / +1).
PEAKED = dict(N=64, A=128, L=21, seed=77, logit_scale=60.0, embed_scale=10.0, wrong_every=10)


def make_peaked(labels=None, masks=None):
    """(opt, params, video) of the peaked-softmax training case at the ECHR widths (N64 x A<=128 ragged, S = 20, V1 = 5001).  `labels` /
    `masks`: the fixture's captions (tests/golden/case_peaked.npz); without them the video carries random captions (what do_peaked starts from)."""
    c = PEAKED
    opt = default_opt(vocab_size=5000, seq_length=c['L'] - 2)
    params = make_params(opt, 0)
    params['lm_model.logit.weight'] = (params['lm_model.logit.weight'] * np.float32(c['logit_scale'])).astype(np.float32)
    params['lm_model.embed.weight'] = (params['lm_model.embed.weight'] * np.float32(c['embed_scale'])).astype(np.float32)
    vid = make_video(c['N'], c['A'], c['L'], 5001, seed=c['seed'])
    if labels is not None:
        vid['labels'], vid['masks'] = np.asarray(labels, np.int64).copy(), np.asarray(masks, np.float32).copy()
    return opt, params, vid


# The additive attention at TRAINED-WEIGHT scales.  make_params draws ctx2att / h2att / alpha_net in +-1/sqrt(fan_in) and make_video draws
# C3D rows from N(0, 1): |p| = |ctx2att(c3d)| and |q| = |h2att(h1)| stay near 1, sum|alpha| near 11 and the slot softmax near uniform.  A trained
# checkpoint is not there, and three pieces of the attention kernels depend on it: the max exchange of the split softmax (sum|alpha| > 40),
# the factored tanh(p + q) = 1 - 2 / (e^{2p} e^{2q} + 1) whose factors are formed from p and q separately, and its conditioning at large
# |p| + |q|.  The variants below are built from make_params / make_video by SCALING only (no stored weights):
#   alpha_sum   alpha_net.weight rescaled so that sum|alpha| has this value (asserted here)
#   c2a / h2a   (weight scale, bias scale) of ctx2att / h2att
#   cross       c: on attention columns 0..3 ctx2att.bias = +c and h2att.bias = -(c - 10) (p ~ +c, q ~ -(c - 10), p + q ~ +10), on columns
#               4..7 the mirrored signs (p + q ~ -10): both arguments beyond +-43, their sum where tanh is +-1 to 4e-9 but not "0"
#   coherent    b: ctx2att.bias = b * sign(alpha_j) (with alpha_sum): tanh(p + q) takes the sign of alpha_j on most columns, so the scores of ALL slots
#               sit near +0.8 sum|alpha| (scores of random sign stay within a few ||alpha||_2 ~ +-30, where an unshifted exp is still finite)
#   lens        event lengths written over the first events (thirds of an event without a valid slot: 43 / 86 / 129 boundaries)
ATTSAT = {
    'below': dict(alpha_sum=39.0, video=dict(N=40, A=129, seed=81)),
    'above': dict(alpha_sum=41.0, video=dict(N=40, A=129, seed=81)),
    # N64 x A128, V1 = 5001, 20 steps: the benchmarked shape
    'above64': dict(alpha_sum=41.0, vocab=5000, seq_length=19, video=dict(N=64, A=128, seed=82)),
    'alpha_big': dict(alpha_sum=150.0, coherent=2.0, video=dict(N=64, A=129, seed=83)),
    # three 64-event groups, the last one partly filled (training takes the launch-per-phase recurrences there, decoding the persistent one per group)
    'alpha_big150': dict(alpha_sum=150.0, coherent=2.0, video=dict(N=150, A=100, seed=88)),
    'pq_wide': dict(c2a=(12.0, 12.0), h2a=(40.0, 500.0), video=dict(N=40, A=129, seed=84)),
    'pq_cross': dict(cross=60.0, video=dict(N=12, A=60, seed=85)),
    'short': dict(alpha_sum=41.0, lens=(1, 2, 43, 44, 86, 87, 129), video=dict(N=40, A=129, seed=86)),
    'short_big': dict(alpha_sum=41.0, lens=(130, 172, 173, 258, 1, 44, 87), video=dict(N=24, A=258, seed=87, min_len=100)),
}
ATTSAT_CROSS_COLS = 4


def make_attsat(name, clip_context_type='CC'):
    """(opt, params, video) of a trained-attention-regime case (see ATTSAT).  Small shapes (vocabulary 300, 6 steps) except 'above64'.
    `clip_context_type` 'CH' / 'CC+CH': the same construction over the frame-level context of that type (ctx2att is 512 / 1012 wide)."""
    c = ATTSAT[name]
    L = c.get('seq_length', 5) + 2
    opt = default_opt(vocab_size=c.get('vocab', 300), seq_length=L - 2, clip_context_type=clip_context_type)
    params = make_params(opt, 0)
    vid = make_video(L=L, V1=opt.CG_vocab_size + 1, **c['video'])
    att = 'lm_model.core.attention.'
    f32 = np.float32
    if 'alpha_sum' in c:
        w = params[att + 'alpha_net.weight']
        w = (w.astype(np.float64) * (c['alpha_sum'] / np.abs(w.astype(np.float64)).sum())).astype(f32)
        got = float(np.abs(w.astype(np.float64)).sum())
        assert abs(got - c['alpha_sum']) < 1e-3 * c['alpha_sum'], got          # far inside the distance to the switch at 40
        params[att + 'alpha_net.weight'] = w
    if 'coherent' in c:
        params[att + 'ctx2att.bias'] = (f32(c['coherent']) * np.sign(params[att + 'alpha_net.weight'][0])).astype(f32)
    for key, lin in (('c2a', 'ctx2att'), ('h2a', 'h2att')):
        if key in c:
            params[att + lin + '.weight'] = (params[att + lin + '.weight'] * f32(c[key][0])).astype(f32)
            params[att + lin + '.bias'] = (params[att + lin + '.bias'] * f32(c[key][1])).astype(f32)
    if 'cross' in c:
        k, cc = ATTSAT_CROSS_COLS, f32(c['cross'])
        params[att + 'ctx2att.bias'][:k] = cc
        params[att + 'h2att.bias'][:k] = -(cc - f32(10.0))
        params[att + 'ctx2att.bias'][k:2 * k] = -cc
        params[att + 'h2att.bias'][k:2 * k] = cc - f32(10.0)
    if 'lens' in c:
        lens = np.asarray(c['lens'], np.int64)
        soi = vid['soi']
        soi[:len(lens), 0] = np.minimum(soi[:len(lens), 0], vid['T_v'] - lens)
        soi[:len(lens), 1] = soi[:len(lens), 0] + lens
        vid['ind'] = (soi[:, 1] - 1).astype(np.int64)
    return opt, params, vid


# The decoder's three LSTM streams at TRAINED-WEIGHT scales.  make_params draws layer{0,1,2}.weight_* in +-1/sqrt(512) and the embedding in +-0.1:
# gate pre-activations stay below 1.1, cell states below 0.7, and the attended context (rows from N(0, 1)) below 4.  The variants below leave
# that regime by SCALING only (no stored weights), at the ECHR widths (H = Ha = 512, D = 500: the persistent kernels' shape), vocabulary 300,
# greedy decoding over seq_length 19:
#   embed / ih / hh   scale of embed.weight and of weight_ih / weight_hh of all three layers
#   forget / igate    added to bias_ih[H:2H] / bias_ih[0:H] of all three layers
#   steps             teacher-forced decoder steps (default 6)
#   feat              (lo, hi): C3D row r is multiplied by 2^e_r, e_r a uniform integer in [lo, hi] (RandomState(video seed + 1000)): the bound on
#                     |context| of the persistent kernels' fp32 -> fp16-pair conversion differs from event to event by up to 14 binades
#   c2a_w             scale of ctx2att.weight (keeps |p| inside the factored tanh's domain under `feat`)
#   plant 'events'    event 0 becomes rows [0, 3) and those rows are zeroed (context bound 0); one element of event 1 becomes the power of two
#                     just above every other |element| of that event (the exponent boundary of the bound); event 2 becomes the ONE row that
#                     holds the video's largest |element|: its attended context IS that row (|context| = 216, where the average over a longer
#                     event stays far below its bound), so a conversion factor formed for the usual |context| < 8 overflows fp16 there
#   plant 'big'       events 0..3 are laid out back to back -- 130 rows, 258 rows, 100 rows, one row that belongs to none of the four, 173 rows.
#                     Events 0, 1, 3 are quiet (row exponents lo .. lo + 3: |element| < 0.3) but for ONE element of 4096: in slot 129 of event 0
#                     (its last, the first of the second slot set), in the last slot of event 1, in slot 129 of event 3.  Spread over the event
#                     by the near-uniform attention it leaves |context| ~ 4096 / length = 16 .. 32, a hundred times the other rows' bound: a
#                     maximum that misses that slot gives a conversion factor under which the context overflows fp16.  The row just PAST
#                     event 2's end holds 16384 and must not enter event 2's bound
#   vbatch            a multi-video batch (make_vbatch_videos) instead of one video
# Video seeds of the decoded variants: the first of 91, 191, ... (92, 192, ...; 93, ...; 94, ...; 95, ...) whose float64-oracle greedy decode keeps a
# top-1 / top-2 margin above 1e-4 at every step of every unfinished row (91 .. 94 hold it; 95 and 195 miss it: 4.0e-5, 4.9e-5) -- and, for
# gates_sat70, whose float32-oracle log-prob error stays below a third of the 1e-4 contract: over 70 events the float32 reference itself costs
# 3.1e-5 .. 5.1e-5 in train mode (log-probs of -50 have an ulp of 3.8e-6), so 4 e_ref leaves the contract at every seed and the gate there is the
# contract itself (295 holds the margin with e_ref 5.1e-5; 395: 3.1e-5).  tests/test_decoder_regime_host.py asserts all of it.
_GATES_SAT = dict(embed=10.0, ih=16.0, hh=12.0, forget=1.0)
_FEAT_WIDE = dict(feat=(-8, 6), c2a_w=2.0 ** -6)
DECSAT = {
    'gates_sat': dict(_GATES_SAT, video=dict(N=12, A=40, seed=91)),
    'drift': dict(embed=10.0, ih=4.0, hh=2.0, forget=8.0, igate=3.0, steps=20, video=dict(N=12, A=40, seed=92)),
    'feat_wide': dict(_FEAT_WIDE, plant='events', video=dict(N=12, A=40, seed=93)),
    # events of up to 258 segments: the BIG instantiation of the persistent kernels (129 < A <= 258)
    'feat_wide_big': dict(_FEAT_WIDE, plant='big', video=dict(N=10, A=258, seed=94, T_v=700, min_len=100)),
    # more than 64 rows: the launch-per-phase recurrences in training, the chain sampler in decoding
    'gates_sat70': dict(_GATES_SAT, video=dict(N=70, A=40, seed=395)),
    'gates_sat_vb': dict(_GATES_SAT, vbatch=dict(V=3, events=(3, 6), max_events=16, seg=(3, 40), T=(40, 80), L=(6, 8), seed=96)),
}
DECSAT_BIG_LENS = (130, 258, 100, 173)
DECSAT_BIG_TOP = np.float32(4096.0)


def decsat_event_max(vid, n):
    """(largest |C3D| element of event n, its slot)."""
    s, e = (int(x) for x in vid['soi'][n])
    a = np.abs(vid['c3d'][s:e])
    return float(a.max()), int(np.unravel_index(int(a.argmax()), a.shape)[0])


def _pow2_above(x):
    return float(2.0 ** (math.floor(math.log2(x)) + 1))


def make_decsat(name):
    """(opt, params, video) of a trained-decoder-regime case (see DECSAT); 'gates_sat_vb': (opt, params, [videos])."""
    c = DECSAT[name]
    f32 = np.float32
    opt = default_opt(vocab_size=300, seq_length=19)
    H = opt.CG_rnn_size
    params = make_params(opt, 0)
    params['lm_model.embed.weight'] = (params['lm_model.embed.weight'] * f32(c.get('embed', 1.0))).astype(f32)
    for k in range(3):
        pre = 'lm_model.core.layer%d.' % k
        params[pre + 'weight_ih'] = (params[pre + 'weight_ih'] * f32(c.get('ih', 1.0))).astype(f32)
        params[pre + 'weight_hh'] = (params[pre + 'weight_hh'] * f32(c.get('hh', 1.0))).astype(f32)
        params[pre + 'bias_ih'][:H] += f32(c.get('igate', 0.0))
        params[pre + 'bias_ih'][H:2 * H] += f32(c.get('forget', 0.0))
    att = 'lm_model.core.attention.'
    params[att + 'ctx2att.weight'] = (params[att + 'ctx2att.weight'] * f32(c.get('c2a_w', 1.0))).astype(f32)
    V1 = opt.CG_vocab_size + 1
    if 'vbatch' in c:
        return opt, params, make_vbatch_videos(V1=V1, **c['vbatch'])
    vid = make_video(L=c.get('steps', 6) + 1, V1=V1, **c['video'])
    c3d, soi = vid['c3d'], vid['soi']
    if 'feat' in c:
        lo, hi = c['feat']
        e = np.random.RandomState(c['video']['seed'] + 1000).randint(lo, hi + 1, size=c3d.shape[0])
        if c.get('plant') == 'big':
            starts = (0, 130, 388, 489)          # row 488: just past event 2's end, inside none of the four
            for n, (s, l) in enumerate(zip(starts, DECSAT_BIG_LENS)):
                soi[n] = (s, s + l)
                if n != 2:
                    e[s:s + l] = lo + (e[s:s + l] - lo) % 4          # the quiet events: exponents lo .. lo + 3
        c3d *= np.ldexp(f32(1.0), e).astype(f32)[:, None]
    if c.get('plant') == 'events':
        soi[0] = (0, 3)
        c3d[0:3] = 0.0
        r = int(np.abs(c3d).max(1).argmax())
        soi[2] = (r, r + 1)
        s, e = (int(x) for x in soi[1])
        c3d[s + (e - s) // 2, 7] = -f32(_pow2_above(np.abs(c3d[s:e]).max()))
    elif c.get('plant') == 'big':
        c3d[0 + 129, 3] = DECSAT_BIG_TOP
        c3d[130 + 257, 499] = -DECSAT_BIG_TOP
        c3d[488, 11] = f32(4.0) * DECSAT_BIG_TOP
        c3d[489 + 129, 250] = DECSAT_BIG_TOP
    vid['ind'] = (soi[:, 1] - 1).astype(np.int64)
    return opt, params, vid


# Multi-video batches (echr_amd/batch.py): V videos of a few events each, as caption pre-training on ground-truth events sees them
# (train.py:268-271), with ragged event counts, event lengths, video lengths and label widths.  Video v of a case is
# make_video(seed = case seed + v); the per-video shapes come from one RandomState(case seed).
#   vb16   16 videos, 2..6 events each (N_tot <= 64: the persistent recurrences' shape), events of 3..60 segments, T_v 40..160, up to 20
#          decoder steps, ECHR widths, V1 = 5001, scene context 'VL'
#          (case seed 1000: the first of 900, 1000, 1100, ... whose greedy decode keeps a top-1 / top-2 margin above 2e-5 at every step of
#          every row -- tools/make_golden_vbatch.py asserts it on the reference's own decode)
#   vbctx  5 videos incl. a one-event video, scene context from all three sources ('VLVCVH': per-video column means), 'ER3', small vocabulary
#   vb24 / vb33  24 / 33 videos of 4 events, small vocabulary
#   vbscst 4 videos of 3..6 events at the 'tiny_eos' widths (self-critical training over a batch)
#   vbch / vbcch  the vbctx construction (5 videos incl. a one-event video, 'VLVCVH', 'ER3', ragged label widths) with at most 16 events and the
#          frame-level context 'CH' (D = 512: the persistent recurrences, all three gradient paths into tap) / 'CC+CH' (D = 1012: launch-per-phase)
#   vbch33 'CH' over 33 videos of 4 events (132 rows: launch-per-phase recurrences, the chain sampler, the event encoder's general kernels)
#   vbinit / vbinitch  the vbctx construction with at most 16 events and the non-zero initial decoder state: 'VEC' over 'CC' rows (<= 64 rows: a
#          zero-state batch would take the persistent recurrences here, this one must not; the per-video longest events differ, so a batch-wide
#          divisor of the clip mean shows) / 'VE' over 'CH' rows (init_linear's d video through 'VH' into tap beside the three other paths)
#   vbinit33 'VEC' over 33 videos of 4 events (132 rows: the chain sampler, the event encoder's general kernels)
VBATCH = {
    'vb16': dict(opt=dict(CG_vocab_size=5000, CG_seq_length=19), V=16, events=(2, 6), max_events=64, seg=(3, 60), T=(40, 160), L=(12, 21), seed=1000),
    'vbctx': dict(opt=dict(video_context_type='VLVCVH', CG_vocab_size=300, CG_seq_length=7), V=5, events=(1, 4), single=2, max_events=64, seg=(3, 30),
                  T=(30, 60), L=(6, 9), seed=950),
    # more than 64 events: the launch-per-phase recurrences and the event encoder's general softmax kernels (96 events: one wave per (event,
    # head); 132 events: the row kernel)
    'vb24': dict(opt=dict(CG_vocab_size=300, CG_seq_length=7), V=24, events=(4, 4), max_events=96, seg=(3, 30), T=(30, 80), L=(6, 9), seed=1200),
    'vb33': dict(opt=dict(CG_vocab_size=300, CG_seq_length=7), V=33, events=(4, 4), max_events=132, seg=(3, 30), T=(30, 80), L=(6, 9), seed=1300),
    # self-critical training over a batch (tests/golden/case_scst_batch.npz): the 'tiny_eos' widths (V1 = 31, seq_length 6), 4 videos of 3..6
    # events; tools/make_golden_scst_batch.py picks the reference's draw seeds whose per-video sample widths differ
    'vbscst': dict(opt=dict(video_dim=20, hidden_dim=24, lda_dim=12, d_feats=32, d_o=32, n_head=4, CG_rnn_size=32, CG_input_encoding_size=16,
                            CG_att_hid_size=24, CG_vocab_size=30, CG_seq_length=6),
                   V=4, events=(3, 6), max_events=64, seg=(3, 9), T=(12, 24), L=(8, 8), seed=1400),
    # frame-level contexts over a batch (tests/golden/case_clip_batch.npz; case seeds picked like vb16's: tools/make_golden_clip_batch.py asserts
    # the greedy margins)
    'vbch': dict(opt=dict(clip_context_type='CH', video_context_type='VLVCVH', CG_vocab_size=300, CG_seq_length=7), V=5, events=(1, 4), single=2,
                 max_events=16, seg=(3, 30), T=(30, 60), L=(6, 9), seed=1500),
    'vbcch': dict(opt=dict(clip_context_type='CC+CH', video_context_type='VLVCVH', CG_vocab_size=300, CG_seq_length=7), V=5, events=(1, 4), single=2,
                  max_events=16, seg=(3, 30), T=(30, 60), L=(6, 9), seed=1600),
    'vbch33': dict(opt=dict(clip_context_type='CH', CG_vocab_size=300, CG_seq_length=7), V=33, events=(4, 4), max_events=132, seg=(3, 30), T=(30, 80),
                   L=(6, 9), seed=1700),
    # the initial decoder state over a batch (tests/golden/case_init_batch.npz; case seeds picked like vb16's: tools/make_golden_init_batch.py
    # asserts the greedy margins; vbinit's is also the first of 1800, 1900, ... whose longest event sits in a one-event video, so that every
    # multi-event video's padded clip length is below the batch-wide one)
    'vbinit': dict(opt=dict(CG_init_feats_type='VEC', video_context_type='VLVCVH', CG_vocab_size=300, CG_seq_length=7), V=5, events=(1, 4), single=2,
                   max_events=16, seg=(3, 30), T=(30, 60), L=(6, 9), seed=2800),
    'vbinitch': dict(opt=dict(CG_init_feats_type='VE', clip_context_type='CH', video_context_type='VLVCVH', CG_vocab_size=300, CG_seq_length=7), V=5,
                     events=(1, 4), single=2, max_events=16, seg=(3, 30), T=(30, 60), L=(6, 9), seed=1900),
    # (vbinit33 has no reference fixture: its seed is the first of 2000, 2100, ... whose ORACLE greedy margin exceeds 2e-5 -- init_batch_ref.greedy_margin,
    # asserted by tests/test_init_batch_host.py)
    'vbinit33': dict(opt=dict(CG_init_feats_type='VEC', CG_vocab_size=300, CG_seq_length=7), V=33, events=(4, 4), max_events=132, seg=(3, 30), T=(30, 80),
                     L=(6, 9), seed=2300),
}


def make_vbatch_videos(V, events, seg, T, L, V1, seed, max_events=64, single=None, video_dim=500, hidden_dim=512, lda_dim=100):
    """V synthetic videos (make_video dicts) with events[0]..events[1] events each (`single`: the index of a video that gets exactly one),
    at most max_events in all, the longest event of a video in seg[0]..seg[1] segments (the others from seg[0] up to it), T_v in T, label
    width L_v in L (at least one caption of a video uses all L_v - 2 token slots, so the video runs L_v - 1 steps)."""
    rs = np.random.RandomState(seed)
    counts = rs.randint(events[0], events[1] + 1, size=V)
    if single is not None:
        counts[single] = 1
    while counts.sum() > max_events:
        counts[int(np.argmax(counts))] -= 1
    vids = []
    for v in range(V):
        A = int(rs.randint(max(seg[0], 8), seg[1] + 1))
        Tv = int(rs.randint(max(T[0], A), T[1] + 1))
        Lv = int(rs.randint(L[0], L[1] + 1))
        vids.append(make_video(int(counts[v]), A, Lv, V1, seed=seed + v, T_v=Tv, min_len=seg[0], video_dim=video_dim, hidden_dim=hidden_dim,
                               lda_dim=lda_dim))
    return vids


def make_vbatch(name, param_seed=0):
    """(opt, params, [video dicts]) of a named multi-video case."""
    c = VBATCH[name]
    opt = default_opt(**c['opt'])
    vids = make_vbatch_videos(c['V'], c['events'], c['seg'], c['T'], c['L'], opt.CG_vocab_size + 1, c['seed'], c['max_events'], c.get('single'),
                              opt.video_dim, opt.hidden_dim, opt.lda_dim)
    return opt, make_params(opt, param_seed), vids

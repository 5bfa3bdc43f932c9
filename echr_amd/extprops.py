"""External temporal-event proposals, selected on the device: the reference's flag_eval_what = 'SOTA_TEP'
(eval_utils.py:76-104, fed by dataloader.py:292-296, 304-318, 509-524).  The events to caption come from somebody else's proposal file --
per video a list of (start s, end s) segments with a score each -- instead of the SST encoder's score grid.

`select` filters the proposals of V videos by greedy cluster NMS over their timestamps (eval_utils.gettopN_nms), a score threshold and topN,
converts the survivors to feature rows (dataloader.timestamp_to_featstamp, Python 2 rounding) and crops over-long ones to the anchor count;
`nms` is the device form of eval_utils.gettopN_nms for one list.  The kernels are csrc/extprops.hip (echr_nms_segments_batch,
echr_ext_proposals_batch).  There is no host fallback.

The crop offset is not numpy's randint: proposal i of a video draws a Philox word keyed by (seed, the video's draw id) at site
philox.SITE_CROP, and r = (word * n) >> 32 is the offset among the n = e - s - K + 1 admissible ones -- reproducible, and the same for a
video alone and inside any batch."""
import numpy as np
import torch

from . import _lib as L

MAX_P = 4096                 # ECHR_EXTPROPS_MAX_P: external proposals per video (four register slots per thread of a 1024-thread workgroup)
MAX_VIDEOS = 65535           # ECHR_EXTPROPS_MAX_VIDEOS


def check_overlap(nms_threshold):
    """0 <= nms_threshold < 1 as a float, else ValueError."""
    thr = float(nms_threshold)
    if not 0.0 <= thr < 1.0:
        raise ValueError('nms_threshold must satisfy 0 <= nms_threshold < 1 (got %r): at 1 the reference re-picks the same proposal until its '
                         'round limit (the best never leaves the alive set), above 1 its argmax has an empty cluster to read' % (nms_threshold,))
    return thr


def _segments(stamps, scores, what):
    """([P, 2] float64, [P] float64) of one list, checked: shapes, finite values, end >= start.  ValueError names the first violation."""
    sc = np.asarray(scores, dtype=np.float64).reshape(-1)
    st = np.asarray(stamps, dtype=np.float64)
    st = st.reshape(-1, 2) if st.size else np.zeros((0, 2))
    if len(st) != len(sc):
        raise ValueError('%s: %d segments and %d scores' % (what, len(st), len(sc)))
    if len(sc) > MAX_P:
        raise ValueError('%s has %d proposals (at most ECHR_EXTPROPS_MAX_P = %d)' % (what, len(sc), MAX_P))
    bad = np.nonzero(~(np.isfinite(st).all(1) & np.isfinite(sc)))[0]
    if bad.size:
        raise ValueError('%s: proposal %d is not finite (segment %r, score %r)' % (what, bad[0], st[bad[0]].tolist(), sc[bad[0]]))
    bad = np.nonzero(st[:, 1] < st[:, 0])[0]
    if bad.size:
        raise ValueError('%s: proposal %d has end < start (%r)' % (what, bad[0], st[bad[0]].tolist()))
    return st, sc


def _device(device):
    dev = torch.device('cuda') if device is None else torch.device(device)
    if dev.type != 'cuda':
        raise L.EchrHipError('extprops runs on the GPU only (got %s); echr_amd has no CPU path' % dev)
    return dev


def _upload(doubles, ints, dev):
    """One host-to-device copy of float64 vectors followed by int32 vectors; returns their device pointers (and the buffer, to keep it)."""
    d = np.concatenate([np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in doubles])
    i = np.concatenate([np.ascontiguousarray(x, dtype=np.int32).reshape(-1) for x in ints])
    buf = torch.from_numpy(np.concatenate([d.view(np.uint8), i.view(np.uint8)])).to(dev)
    base, ptrs = buf.data_ptr(), []
    off = 0
    for x in doubles:
        ptrs.append(base + off)
        off += 8 * int(np.size(x))
    for x in ints:
        ptrs.append(base + off)
        off += 4 * int(np.size(x))
    return buf, ptrs


def nms(props, prop_scores, sent_score, nms_overlap=0.999, topN=1000, device=None):
    """eval_utils.gettopN_nms on the device for one list: (props[pick], prop_scores[pick], pick), `pick` in round order (a list of ints; a
    proposal whose overlap with a round's best EQUALS nms_overlap is clustered and stays alive, so it can be picked again -- the reference's
    behaviour).  `sent_score` ranks the members of a cluster (caption confidences for re-ranking; pass prop_scores for the SOTA_TEP call).
    Ties of prop_scores go to the larger index, ties of sent_score to the member that comes first in ascending (prop_score, index) order."""
    thr = check_overlap(nms_overlap)
    st, sc = _segments(props, prop_scores, 'nms')
    ss = np.asarray(sent_score, dtype=np.float64).reshape(-1)
    if len(ss) != len(sc) or not np.isfinite(ss).all():
        raise ValueError('nms: sent_score must hold one finite value per proposal (%d)' % len(sc))
    if int(topN) < 1:
        raise ValueError('topN must be at least 1 (got %d)' % int(topN))
    dev = _device(device)
    P = len(sc)
    if P == 0:
        return np.asarray(props).reshape(0, 2), np.asarray(prop_scores).reshape(0), []
    rounds = min(int(topN), P)                           # a round removes its best: there are at most P
    lib = L.load()
    with torch.cuda.device(dev):
        buf, (st_d, sc_d, ss_d, po_d) = _upload([st, sc, ss], [np.array([0, P])], dev)
        out = torch.empty(rounds + 1, device=dev, dtype=torch.int32)
        L.check(lib.echr_nms_segments_batch(st_d, sc_d, ss_d, po_d, 1, P, P, thr, rounds, out.data_ptr(), out[rounds:].data_ptr(),
                                            L.stream_ptr()), 'nms_segments_batch')
        host = out.cpu().numpy()
    pick = host[:int(host[rounds])].astype(np.int64).tolist()
    return np.asarray(props)[pick, :], np.asarray(prop_scores)[pick], pick


def _video(vid, v):
    """(T_v, duration, segments or None, scores or None) of video dict v."""
    if 'nfeats' in vid:
        T = vid['nfeats']
    elif 'T_v' in vid:
        T = vid['T_v']
    elif 'c3d' in vid:
        T = vid['c3d'].shape[0]
    else:
        raise ValueError("video %d carries none of 'nfeats', 'T_v' and 'c3d'" % v)
    return int(T), float(vid['duration']), vid.get('SOTA_timestamps'), vid.get('SOTA_Prop_score')


class Selection(object):
    """The result of `select`.  Per video v (host arrays): pick[v] the kept original proposal indices (ascending), ind[v] = e and
    soi[v] = [s, e + 1] in feature rows (int64), scores[v] their external scores and timestamps[v] their ORIGINAL external segments in seconds
    (float64 [n, 2]; the reference reports SOTA_timestamps, not rows converted back).  bad: the videos the reference skips (no proposal
    file entry, or at most one feature row); event_offset int64 [V + 1]."""

    def __init__(self, pick, ind, soi, scores, timestamps, bad, event_offset):
        self.pick, self.ind, self.soi, self.scores, self.timestamps, self.bad, self.event_offset = pick, ind, soi, scores, timestamps, bad, event_offset

    @property
    def n_videos(self):
        return len(self.pick)


def select(videos, K, topN=1000, nms_threshold=0.0, val_score_thres=0.0, nms_rounds=1000, seed=0, draw=None, crop=True, device=None):
    """The SOTA_TEP selection of V videos.  `videos`: dicts with 'SOTA_timestamps' [P_v, 2] (seconds), 'SOTA_Prop_score' [P_v] (the
    reference's key names), 'duration' and 'nfeats' / 'T_v' / 'c3d'.  A video whose score list is None or missing, or that has at most one
    feature row, is "bad": the reference `continue`s past it; it selects nothing and is listed in the result's `bad`.

    nms_threshold > 0 filters by eval_utils.gettopN_nms over the timestamps with sent_score = prop_scores and `nms_rounds` rounds (the
    reference passes the literal 1000); then, in file order, a picked proposal is kept if its score >= val_score_thres, until `topN` are
    kept.  Each kept segment becomes rows (s, e) by dataloader.timestamp_to_featstamp; with `crop`, one with e - s >= K + 1 is cut to K
    rows at an offset drawn from (seed, draw[v], its index) -- draw defaults to the video's position.

    The host checks its copies (vectorised numpy, before the upload): non-finite values, end < start, duration <= 0, nms_threshold outside
    [0, 1), topN < 1, more than MAX_P proposals, a draw id outside [0, 2^31) -- ValueError names the first violation.  One packed upload,
    two or three launches, ONE device-to-host read.  Returns Selection."""
    K, topN, rounds = int(K), int(topN), int(nms_rounds)
    thr = check_overlap(nms_threshold)
    if K < 1:
        raise ValueError('K must be at least 1 (got %d)' % K)
    if topN < 1:
        raise ValueError('topN must be at least 1 (got %d)' % topN)
    if rounds < 1:
        raise ValueError('nms_rounds must be at least 1 (got %d)' % rounds)
    vals = float(val_score_thres)
    if not np.isfinite(vals):
        raise ValueError('val_score_thres must be finite (got %r)' % (val_score_thres,))
    videos = list(videos)
    V = len(videos)
    if not 1 <= V <= MAX_VIDEOS:
        raise ValueError('between 1 and %d videos per call (got %d)' % (MAX_VIDEOS, V))
    rows, durs, stamps, scores, bad = [], [], [], [], []
    for v, vid in enumerate(videos):
        T, dur, st, sc = _video(vid, v)
        if not (np.isfinite(dur) and dur > 0.0):
            raise ValueError('video %d: duration must be positive and finite (got %r)' % (v, dur))
        if sc is None or st is None or T <= 1:
            bad.append(v)
            st, sc = np.zeros((0, 2)), np.zeros(0)
        else:
            st, sc = _segments(st, sc, 'video %d' % v)
        rows.append(T)
        durs.append(dur)
        stamps.append(st)
        scores.append(sc)
    dr = np.arange(V, dtype=np.int64) if draw is None else np.asarray(draw, dtype=np.int64).reshape(-1)
    if dr.size != V or (dr < 0).any() or (dr >= 2 ** 31).any():
        raise ValueError('draw must hold one stream id in [0, 2^31) per video (%d videos)' % V)
    if max(rows) >= 2 ** 31:
        raise ValueError('a video of %d rows (below 2^31)' % max(rows))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    dev = _device(device)
    counts = np.array([len(s) for s in scores], dtype=np.int64)
    po = np.concatenate([[0], np.cumsum(counts)])
    P_tot, P_max = int(po[-1]), int(counts.max())
    cap = int(np.minimum(counts, topN).sum())
    st_all, sc_all = np.concatenate(stamps, 0), np.concatenate(scores)
    if P_tot == 0:
        empty = [np.zeros(0, np.int64) for _ in range(V)]
        return Selection(empty, list(empty), [np.zeros((0, 2), np.int64) for _ in range(V)], [np.zeros(0) for _ in range(V)],
                         [np.zeros((0, 2)) for _ in range(V)], bad, np.zeros(V + 1, np.int64))
    use_nms = thr > 0.0
    rounds = min(rounds, P_max)                          # a round removes its best: a video has at most P_v of them
    lib = L.load()
    with torch.cuda.device(dev):
        buf, (st_d, sc_d, du_d, po_d, ro_d, dr_d) = _upload([st_all, sc_all, durs], [po, rows, dr], dev)          # one upload
        i32 = dict(device=dev, dtype=torch.int32)
        out = torch.empty(2 * (V + 1) + 4 * cap, **i32)          # count | event_offset | index | ind | soi: the call's one host read
        work = torch.empty(3 * P_tot + (V * (rounds + 1) if use_nms else 0), **i32)
        base, wbase = out.data_ptr(), work.data_ptr()
        pick_d = pcount_d = None
        stream = L.stream_ptr()
        if use_nms:
            pick_d, pcount_d = wbase + 4 * 3 * P_tot, wbase + 4 * (3 * P_tot + V * rounds)
            L.check(lib.echr_nms_segments_batch(st_d, sc_d, None, po_d, V, P_tot, P_max, thr, rounds, pick_d, pcount_d, stream), 'nms_segments_batch')
        L.check(lib.echr_ext_proposals_batch(st_d, sc_d, po_d, ro_d, du_d, pick_d, pcount_d, rounds, V, P_tot, P_max, K, topN, vals,
                                             1 if crop else 0, seed, dr_d, wbase, cap, base, base + 4 * (V + 1), base + 4 * 2 * (V + 1),
                                             base + 4 * (2 * (V + 1) + cap), base + 4 * (2 * (V + 1) + 2 * cap), stream), 'ext_proposals_batch')
        host = out.cpu().numpy().astype(np.int64)
    eo = host[V + 1:2 * (V + 1)]
    n = int(eo[V])
    body = host[2 * (V + 1):]
    index, ind, soi = body[:cap][:n], body[cap:2 * cap][:n], body[2 * cap:].reshape(-1, 2)[:n]
    sl = [slice(int(eo[v]), int(eo[v + 1])) for v in range(V)]
    pick = [index[s].copy() for s in sl]
    return Selection(pick, [ind[s].copy() for s in sl], [soi[s].copy() for s in sl], [scores[v][pick[v]] for v in range(V)],
                     [stamps[v][pick[v]] for v in range(V)], bad, eo.copy())

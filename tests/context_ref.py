"""Float64 statements of the context-building operations (csrc/core.hip: event_pool_gather, col_mean, seg_col_mean; csrc/clipctx.hip: clip_rows)
on float32 inputs, each with the error bound the float32 kernel may use.  CPU only (numpy).

The bounds count the kernel's own roundings and are not tuned; u = 2^-24 is the unit roundoff of float32.  A sum of k terms goes through
k - 1 additions that round, in whatever tree the kernel forms it (adding a zero partial sum is exact), so each term is carried through at
most k - 1 roundings: |error| <= (k - 1) u sum|x| to first order, for every summation order.  What follows the sum is counted on top.

The cases of the attended-row gradient (tests/test_gpu_context_edges.py, section B) are defined here as well, so that the host test can
check their conditioning with the very inputs the device test runs."""
import numpy as np

U32 = 2.0 ** -24


def _f64(x):
    return np.asarray(x, np.float64)


# ---- pooled event vector and anchor gather -------------------------------------------------------------------------------------------
def event_pool(c3d, tap, ev_start, ev_len, ind, parts):
    """ech = [mean of c3d[start : start + len] | tap[ind]] (parts 3; 1: the pooled part only; 2: the gathered part only).
    Returns (ref float64 [N, D + Ht], bound float64 [N, D], D): the gathered columns ref[:, D:] are copies (bit-exact in float32); the
    pooled element may be off by (len + 2) u mean_a|x| -- len - 1 additions, one division, and one of slack for the second-order terms."""
    D = c3d.shape[1] if parts & 1 else 0
    Ht = tap.shape[1] if parts & 2 else 0
    N = len(ev_start)
    ref = np.zeros((N, D + Ht), np.float64)
    bound = np.zeros((N, D), np.float64)
    for n in range(N):
        s, l = int(ev_start[n]), int(ev_len[n])
        if D:
            x = _f64(c3d[s:s + l])
            ref[n, :D] = x.sum(0) / l
            bound[n] = (l + 2) * U32 * np.abs(x).sum(0) / l
        if Ht:
            ref[n, D:] = _f64(tap[int(ind[n])])
    return ref, bound, D


def event_gather_bwd(d_ech, ind, T, D, Ht, base):
    """d_tap = base with d_ech[:, D:] index-added at the anchor rows ind.  Returns (ref float64 [T, Ht], fixed float32 [T, Ht], bound
    float64 [T, Ht], sharers int [T]).  `fixed` is the fixed-order float32 value: the first event of an anchor row owns it, adds the rows
    of the events that share the anchor in ascending event order starting from zero, and adds that sum onto base in one addition.
    bound = k u (|base| + sum|terms|) for a row shared by k events (k additions in either mode); 0 on rows that are no anchor."""
    d = np.asarray(d_ech, np.float32)[:, D:D + Ht]
    base = np.asarray(base, np.float32).reshape(T, Ht)
    ref = _f64(base).copy()
    mag = np.abs(_f64(base))
    fixed = base.copy()
    sharers = np.zeros(T, np.int64)
    ind = [int(i) for i in ind]
    for n, r in enumerate(ind):
        ref[r] += _f64(d[n])
        mag[r] += np.abs(_f64(d[n]))
        sharers[r] += 1
    for n, r in enumerate(ind):
        if r in ind[:n]:
            continue
        acc = np.zeros(Ht, np.float32)
        for m in range(n, len(ind)):
            if ind[m] == r:
                acc = (acc + d[m]).astype(np.float32)
        fixed[r] = (base[r] + acc).astype(np.float32)
    bound = sharers[:, None] * U32 * mag
    bound[sharers == 0] = 0.0
    return ref, fixed, bound, sharers


# ---- scene means -------------------------------------------------------------------------------------------------------------------------
def col_mean(x):
    """x.mean(0).  Returns (ref float64 [cols], bound): (rows + 3) u mean|x| -- rows - 1 additions, the rounding of 1 / rows, the product,
    and slack."""
    x = _f64(x)
    rows = x.shape[0]
    return x.sum(0) / rows, (rows + 3) * U32 * np.abs(x).sum(0) / rows


def col_mean_bwd(g, rows, base):
    """gx = base + g / rows on every row.  Returns (ref float64 [rows, cols], bound): 3 u (|base| + |g| / rows) -- the kernel forms
    g * (1 / rows) (two roundings) and makes one addition onto base."""
    term = _f64(g)[None, :] / rows
    base = _f64(base)
    return base + term, 3 * U32 * (np.abs(base) + np.abs(term))


def seg_col_mean(x, row_offset):
    """Per segment v the mean of rows [row_offset[v], row_offset[v + 1]).  Returns (ref float64 [V, cols], bound [V, cols]); an empty
    segment gives exactly 0.0 with bound 0."""
    x = _f64(x)
    V = len(row_offset) - 1
    ref = np.zeros((V, x.shape[1]), np.float64)
    bound = np.zeros_like(ref)
    for v in range(V):
        r0, r1 = int(row_offset[v]), int(row_offset[v + 1])
        if r1 > r0:
            ref[v], bound[v] = col_mean(x[r0:r1])
    return ref, bound


def seg_col_mean_bwd(g, row_offset, base):
    """gx = base with g[v] / rows(v) added on the rows of segment v; rows of no segment and empty segments leave base untouched (bound 0
    there).  Returns (ref float64, bound)."""
    g = _f64(g)
    ref = _f64(base).copy()
    bound = np.zeros_like(ref)
    for v in range(len(row_offset) - 1):
        r0, r1 = int(row_offset[v]), int(row_offset[v + 1])
        if r1 > r0:
            ref[r0:r1], bound[r0:r1] = col_mean_bwd(g[v], r1 - r0, ref[r0:r1])
    return ref, bound


# ---- the [c3d | tap] row source -----------------------------------------------------------------------------------------------------------
def clip_rows(c3d, tap):
    """[c3d[:T] | tap[:T]] over T = min(rows): pure data movement, bit-exact."""
    T = min(c3d.shape[0], tap.shape[0])
    return np.concatenate([np.asarray(c3d)[:T], np.asarray(tap)[:T]], axis=1)


# ---- per-row comparison --------------------------------------------------------------------------------------------------------------------
def per_row_relerr(got, ref64, floor_frac=1e-2):
    """(err [rows], zero [rows]): err[r] = max|got[r] - ref[r]| / max(max|ref[r]|, floor_frac * max|ref|); zero[r]: the reference row is
    exactly zero.  The floor keeps a row a hundred times smaller than the largest from being judged on its own rounding noise."""
    got, ref = _f64(got), _f64(ref64)
    row_max = np.abs(ref).max(1)
    floor = floor_frac * float(np.abs(ref).max())
    den = np.maximum(np.maximum(row_max, floor), 1e-300)
    return np.abs(got - ref).max(1) / den, row_max == 0.0


def covered_rows(soi, T):
    """bool [T]: the row lies inside at least one event."""
    cov = np.zeros(T, bool)
    for s, e in np.asarray(soi, np.int64).reshape(-1, 2):
        cov[int(s):int(e)] = True
    return cov


# ---- the attended-row gradient alone: cases --------------------------------------------------------------------------------------------------
# event_context_type 'EC' + video_context_type 'VL': tap_feats reaches the loss through the attended rows (echr_decoder_row_grad) only.
# Videos as tests/test_gpu_sat._edge_case builds them: synth.make_video plus a `lens` override of the first events, vocabulary 30, five
# steps, the widths of synth.CASES['tiny'] as a three-stream model.  T_v: chosen so that rows outside every event exist (all but 'disjoint',
# whose events tile the video).
SLOT_LENS = (1, 7, 8, 9, 16, 17)
ROW_GRAD_CASES = {
    # slot-chunk tails 1, 7, 8 (RG_SLOTS = 8); events whose second / third chunk lies past len; nc = 24 of 256 column threads busy
    'slots_ch': dict(clip='CH', N=6, A=17, lens=SLOT_LENS, T_v=40, seed=401),
    # the same events behind the 20 C3D columns: column offset col0 = 20 into W_ih1 and W_c2a
    'slots_cch': dict(clip='CC+CH', N=6, A=17, lens=SLOT_LENS, T_v=40, seed=402),
    # nc = 260: one full pass of the 256-thread column loop and a pass of 4
    'nc260': dict(clip='CH', N=4, A=9, over=dict(hidden_dim=260), seed=403),
    # no two events share a row: the plain read-modify-write branch (rows_disjoint = 1)
    'disjoint': dict(clip='CH', N=4, A=9, disjoint=True, seed=404),
    # A < 8: a single partial slot chunk (T_v = 6: the three events overlap and leave a row free)
    'a3': dict(clip='CH', N=3, A=3, lens=(1, 2, 3), T_v=6, seed=405),
    # D = 21 + 24 = 45: not a multiple of 4
    'odd_dc': dict(clip='CC+CH', N=4, A=9, over=dict(video_dim=21), seed=406),
}
ROW_GRAD_L = 7          # label width: CG_seq_length = 5


def make_row_grad_case(name):
    """(opt, params, video) of a ROW_GRAD_CASES entry."""
    from echr_amd import synth
    c = ROW_GRAD_CASES[name]
    o = dict(synth.CASES['tiny']['opt'], event_context_type='EC', video_context_type='VL', clip_context_type=c['clip'],
             CG_vocab_size=30, CG_seq_length=ROW_GRAD_L - 2)
    o.update(c.get('over', {}))
    opt = synth.default_opt(**o)
    vid = synth.make_video(N=c['N'], A=c['A'], L=ROW_GRAD_L, V1=opt.CG_vocab_size + 1, seed=c['seed'], video_dim=opt.video_dim,
                           hidden_dim=opt.hidden_dim, lda_dim=opt.lda_dim, disjoint=c.get('disjoint', False), T_v=c.get('T_v'),
                           min_len=min(4, c['A']))
    if 'lens' in c:          # the first events get these lengths
        ln = np.asarray(c['lens'], np.int64)
        soi = vid['soi']
        soi[:len(ln), 0] = np.minimum(soi[:len(ln), 0], vid['T_v'] - ln)
        soi[:len(ln), 1] = soi[:len(ln), 0] + ln
        vid['ind'] = (soi[:, 1] - 1).astype(np.int64)
    return opt, synth.make_params(opt, 0), vid

"""Host references of the decoders' token selection on exactly known logits (numpy, float64; no GPU).

With lm_model.logit.weight = 0 every form of the logits product gives exactly 0 + b_logit at every row and step, so the logits row of a
whole decode is one known float32 vector.  The uniforms of the multinomial draw are known too (echr_amd/philox.py: sample_u24 is
bit-identical to the device generator), so every draw of a decode can be replayed, not merely its distribution:

  bias_design          logit-bias vectors whose probability mass sits where the multinomial kernels can go wrong (csrc/core.hip: thread th
                       owns the contiguous chunk [CH th, CH th + CH), CH = ceil(V1 / 256)): chunk edges, the middle thread, the row's end
  replay_multinomial   the expected decode in float64: tokens by inverse CDF in index order, the <eos> bookkeeping, the log-probs
  check_draws          the two rules a device decode is held to (below)
  draw_f32             the device arithmetic line by line in float32 -- validates the checker (and its power: mutations) without a GPU
  greedy_ties_design   bias vectors with exact ties for the arg-max kernels (lowest index wins)
  beam_class_design    bias vectors whose beam search is decided by the tie rules alone (smaller slot, then smaller token)

The rules of check_draws, at every observable position (up to and including a row's first <eos>):
  (a) the float64 interval [cdf[g-1], cdf[g]] of the token g the device emitted, widened by DELTA on both sides, contains u;
  (b) where u is farther than DELTA from both ends of the expected token's interval (`near` false), g is the expected token.

DELTA = 1e-6: a float32 emulation of the device arithmetic (draw_f32) over 40 960 draws -- V1 in {31, 257, 2048, 2049, 5121, 12288,
12289, 13001}, T in {1.0, 0.7}, N = 64, L = 20, seeds 11 and 0x5EED0123456789, 'edges' with seed = V1 -- disagreed with the float64
inverse CDF on at most 5 draws per 2560, every one of them within 2.3e-7 of an interval boundary.  DELTA is about four times that (the
device expf may differ from numpy's by an ulp).  The lightest token interval of those inputs (about 1e-5 at V1 = 13001) is still ten
times DELTA, so rule (a) alone catches a pick that is off by one anywhere."""
import numpy as np

from echr_amd import philox

DELTA = 1e-6
THREADS = 256          # the multinomial kernels' workgroup: one contiguous chunk of the row per thread
ZERO_MASS = -1e30      # exp((ZERO_MASS - max) / T) is exactly 0 in float32 and in float64


def chunking(V1):
    """(CH, c_last): the chunk length of the multinomial kernels and the first index of the last chunk that holds a token."""
    CH = (V1 + THREADS - 1) // THREADS
    return CH, ((V1 - 1) // CH) * CH


def marked_indices(V1):
    """The indices at which a chunked inverse-CDF walk can go wrong: both sides of the first chunk edge, of the middle thread's edge and of
    the last occupied chunk's, and the row's end (those inside (0, V1))."""
    CH, c_last = chunking(V1)
    cand = {1, CH - 1, CH, CH + 1, 128 * CH - 1, 128 * CH, c_last - 1, c_last, V1 - 2, V1 - 1}
    return sorted(i for i in cand if 0 < i < V1)


def bias_design(V1, kind, seed):
    """(bias float32 [V1], marked indices).
    'edges'   N(0, 1) with every marked index at 4 % and <eos> at 2 % of the unmarked row's mass
    'eos'     'edges' with <eos> at 50 %: rows finish at every step
    'sparse'  about a dozen tokens from N(0, 1) -- chunk edges and chunk middles of the first 201 chunks -- and exactly zero mass everywhere else:
              whole chunks, the last ones among them, carry nothing, and <eos> never comes"""
    rs = np.random.RandomState(seed)
    CH, c_last = chunking(V1)
    if kind in ('edges', 'eos'):
        b = rs.standard_normal(V1).astype(np.float32)
        lse = float(np.log(np.exp(b.astype(np.float64)).sum()))
        marked = marked_indices(V1)
        b[marked] = np.float32(lse + np.log(0.04))
        b[0] = np.float32(lse + np.log(0.02 if kind == 'edges' else 0.5))
        return b, marked
    if kind == 'sparse':
        cand = {1, CH - 1, CH, CH + 1, 5 * CH + CH // 2, 37 * CH + CH // 2, 64 * CH, 65 * CH - 1, 128 * CH - 1, 128 * CH, 129 * CH, 200 * CH + CH // 2}
        live = sorted(i for i in cand if 0 < i < V1 - CH)          # (nothing in the last chunk)
        b = np.full(V1, ZERO_MASS, np.float32)
        b[live] = rs.standard_normal(len(live)).astype(np.float32)
        return b, live
    raise ValueError(kind)


def inv_temperature(temperature):
    """The device's float32 1 / T (T <= 0 means 1), as a python float."""
    T = np.float32(temperature if temperature > 0 else 1.0)
    return float(np.float32(1.0) / T)


def emitted(picks):
    """The emitted sequence of raw picks [N, L]: zero from a row's first <eos> on (the network keeps consuming the raw pick)."""
    picks = np.asarray(picks, np.int64)
    un = np.cumprod(picks > 0, axis=1).astype(bool)
    return np.where(un, picks, 0)


def replay_multinomial(bias, temperature, seed, N, L, vid=None):
    """The expected multinomial decode of N rows and L steps over the logits row `bias` (float32 [V1]) in float64."""
    x = np.asarray(bias, np.float32).astype(np.float64)
    V1 = x.shape[0]
    inv = inv_temperature(temperature)
    p = np.exp((x - x.max()) * inv)
    p /= p.sum()
    cdf = np.cumsum(p)
    u = philox.sample_u24(N, L, seed).astype(np.float64) * 2.0 ** -24
    last = int(np.nonzero(p > 0)[0][-1])
    tok = np.minimum(np.searchsorted(cdf, u, side='right'), last).astype(np.int64)          # first index whose inclusive prefix exceeds u
    lo = np.where(tok > 0, cdf[np.maximum(tok - 1, 0)], 0.0)
    hi = cdf[tok]
    near = (u - lo < DELTA) | (hi - u < DELTA)
    un = np.cumprod(tok > 0, axis=1).astype(bool)                  # unfinished AFTER step t
    observable = np.ones((N, L), bool)
    observable[:, 1:] = un[:, :-1]
    seq = np.where(un, tok, 0)
    lse = x.max() + np.log(np.exp(x - x.max()).sum())
    n_unfinished = np.concatenate([[N], un.sum(0)]).astype(np.int64)          # [0] is not a count of the decode (never compared)
    T_out = next((t - 1 for t in range(1, L + 1) if n_unfinished[t] == 0), L)
    ref = dict(tok=tok, near=near, observable=observable, seq=seq, logp=x[tok] - lse, n_unfinished=n_unfinished, T_out=T_out,
               u=u, cdf=cdf, p=p, eos_near=int((observable & (np.abs(u - cdf[0]) < DELTA)).sum()))
    if vid is not None:
        vid = np.asarray(vid, np.int64)
        V = int(vid.max()) + 1
        words = (seq != 0).sum(1)
        ref['video_words'] = np.array([words[vid == v].max() if (vid == v).any() else 0 for v in range(V)] + [words.max()], np.int64)
    return ref


def check_draws(got_seq, ref):
    """Rules (a) and (b) (module docstring) on the emitted sequence got_seq [N, L] of a device decode.  Returns the counts: observable
    positions, near-boundary ones, positions that differ from the float64 pick, violations of (a) and of (b), and `worst`: the largest
    distance |u - nearest end of the expected token's interval| among the positions that differ (0.0 when none does)."""
    g = np.asarray(got_seq, np.int64)
    ob, u, cdf, tok = ref['observable'], ref['u'], ref['cdf'], ref['tok']
    assert g.shape == tok.shape, (g.shape, tok.shape)
    inside = (g >= 0) & (g < cdf.shape[0])
    gc = np.clip(g, 0, cdf.shape[0] - 1)
    lo = np.where(gc > 0, cdf[np.maximum(gc - 1, 0)], 0.0)
    hi = cdf[gc]
    ok_a = inside & (u >= lo - DELTA) & (u <= hi + DELTA)
    differ = ob & (g != tok)
    tlo = np.where(tok > 0, cdf[np.maximum(tok - 1, 0)], 0.0)
    dist = np.minimum(np.abs(u - tlo), np.abs(cdf[tok] - u))
    return dict(observable=int(ob.sum()), near=int((ob & ref['near']).sum()), differ=int(differ.sum()),
                bad_a=int((ob & ~ok_a).sum()), bad_b=int((differ & ~ref['near']).sum()),
                worst=float(dist[differ].max()) if differ.any() else 0.0)


def draw_f32(bias, temperature, u24, mutate=None):
    """Raw picks [N, L] of sample_step_kernel's arithmetic (csrc/core.hip) in float32, line by line: weights relative to the row maximum,
    per-thread masses of the contiguous chunks added in index order, the sequential 256-entry prefix, target = float32(u24) * 2^-24 *
    total, the owner (first thread whose inclusive prefix exceeds the target; the last thread when rounding pushes the target to the
    total), the owner's walk and its chunk-end fallback (the last index of the chunk with non-zero mass).

    `mutate` plants one mistake (tests of the checker's power): 'pick_plus_one', 'ch_floor' (CH = V1 // 256), 'strided' (thread th owns
    th, th + 256, ...), 'no_temp_walk' (temperature left out of the walk)."""
    f32 = np.float32
    x = np.asarray(bias, f32)
    V1 = x.shape[0]
    inv = f32(inv_temperature(temperature))
    m = x.max()
    e = np.exp(((x - m) * inv).astype(f32)).astype(f32)                     # the mass pass
    ew = np.exp((x - m).astype(f32)).astype(f32) if mutate == 'no_temp_walk' else e          # the walk
    CH = V1 // THREADS if mutate == 'ch_floor' else (V1 + THREADS - 1) // THREADS
    if mutate == 'strided':
        own = [np.arange(th, V1, THREADS) for th in range(THREADS)]
    else:
        own = [np.arange(min(V1, th * CH), min(V1, th * CH + CH)) for th in range(THREADS)]
    pre = np.zeros(THREADS + 1, f32)
    acc = f32(0.0)
    for th in range(THREADS):          # (np.add.accumulate adds sequentially, in the array's own precision)
        mass = np.add.accumulate(np.concatenate([np.zeros(1, f32), e[own[th]]]), dtype=f32)[-1]
        acc = f32(acc + mass)
        pre[th + 1] = acc
    total = pre[THREADS]
    u24 = np.asarray(u24, np.int64)
    out = np.zeros(u24.shape, np.int64)
    for idx in np.ndindex(*u24.shape):
        target = f32(f32(f32(u24[idx]) * f32(2.0 ** -24)) * total)
        th = int(np.searchsorted(pre[1:], target, side='right'))          # pre[th] <= target < pre[th + 1]
        if th >= THREADS:
            th = THREADS - 1                                                # target >= total
        js = own[th]
        walk = np.add.accumulate(np.concatenate([pre[th:th + 1], ew[js]]), dtype=f32)[1:]
        hit = np.nonzero(walk > target)[0]
        if len(hit):
            pick = int(js[hit[0]])
        else:                                                               # rounding at the chunk end
            pick = max(0, int(js[-1]) if len(js) else V1 - 1)
            while pick > 0 and not ew[pick] > 0:
                pick -= 1
        if mutate == 'pick_plus_one':
            pick = min(pick + 1, V1 - 1)
        out[idx] = pick
    return out


# ---- the multinomial cases of tests/test_gpu_select.py (the host test asserts the input conditions on every one of them) -----------
SEQ_LEN = 20
TEMPERATURES = (1.0, 0.7)
SEEDS = (11, 0x5EED0123456789)
# (entry, N, V1, designs).  Entries: 'eval' greedy_sample(multinomial=True) in eval mode (sample_step behind the slab sum; N >= 192: behind
# the h2 logits product), 'eval_plain' the same with gemm_h2 = 0 for the call (plain product), 'train' greedy_sample(drop=) with the dropout
# active, 'batch' sample_train_batch over 3 videos (sample_row_step<8 | 20 | 48 | 0> from slabs; N >= 192: on finished logits)
MULTINOMIAL_CASES = (
    ('eval', 64, 257, ('edges',)), ('eval', 64, 2049, ('edges', 'sparse', 'eos')), ('eval', 64, 12289, ('edges', 'sparse', 'eos')),
    ('eval', 192, 5121, ('edges',)), ('eval_plain', 192, 5121, ('edges',)), ('train', 33, 2048, ('edges',)),
    ('batch', 64, 2048, ('edges',)), ('batch', 64, 2049, ('edges', 'sparse', 'eos')), ('batch', 64, 5120, ('edges',)),
    ('batch', 64, 5121, ('edges',)), ('batch', 64, 12288, ('edges',)), ('batch', 64, 12289, ('edges', 'sparse', 'eos')),
    ('batch', 192, 5121, ('edges',)),
)
MULTINOMIAL_PARAMS = [(entry, N, V1, kind) for entry, N, V1, kinds in MULTINOMIAL_CASES for kind in kinds]
# the input conditions (properties of the float64 replay alone)
NEAR_SHARE_MAX = 0.05          # near-boundary share of the observable positions
OBSERVABLE_MIN = {'edges': 0.60, 'sparse': 1.0, 'eos': 0.0}          # ('eos': rows finish at once by design)
MARKED_SHARE_MIN = 0.10        # share of the observable draws that land on a marked index or on <eos>


def input_conditions(ref, marked, kind):
    """Assert the conditions on the inputs of a multinomial case (float64 replay `ref` of bias_design's `marked` indices)."""
    ob = ref['observable']
    n_obs = int(ob.sum())
    assert int((ob & ref['near']).sum()) <= NEAR_SHARE_MAX * n_obs, (int((ob & ref['near']).sum()), n_obs)
    assert n_obs >= OBSERVABLE_MIN[kind] * ob.size, (n_obs, ob.size)
    hits = int((ob & np.isin(ref['tok'], list(marked) + [0])).sum())
    assert hits >= MARKED_SHARE_MIN * n_obs, (hits, n_obs)
    assert ref['eos_near'] == 0          # no observable draw within DELTA of the <eos> boundary: the rows' ends are unambiguous


# ---- greedy arg-max: exact ties and negative rows -------------------------------------------------------------------------------
TIE_I0 = 79          # the last column of the persistent decoder's first logits workgroup (80 columns each)


def greedy_tie_indices(V1):
    i0 = TIE_I0
    idx = {i0, i0 + 1, i0 + 80, V1 - 1}
    if 5120 + i0 < V1:
        idx.add(5120 + i0)          # the same column of the persistent decoder's second 5120-column chunk
    return sorted(idx)


def greedy_ties_design(V1, kind, seed=0):
    """(bias float32 [V1], expected token, tied indices): exact ties of the row maximum; the lowest tied index wins.
    'ties'       the level m at {79, 80, 159, 5199 (where the row is that long), V1 - 1}: the tied maxima straddle two logits workgroups of the persistent
                 decoder, two of its column chunks and the row's end; everything else N(0, 1) shifted below m
    'ties_high'  the same set without its two lowest members
    'ties_far'   the same set without its three lowest members (what remains is 5199 and / or the row's last index): the winner is
                 outside the first register chunk of every thread of the launch-per-step kernels
    'negative'   the 'ties' indices at -50 and every other entry in [-60, -51]: the ordered key on negative floats
    'eos_tie'    'ties' with index 0 tied too: every row finishes at step 0"""
    rs = np.random.RandomState(1000 + V1 + seed)
    tied = greedy_tie_indices(V1)
    if kind == 'negative':
        b = rs.uniform(-60.0, -51.0, V1).astype(np.float32)
        level = np.float32(-50.0)
    else:
        level = np.float32(1.5)
        b = rs.standard_normal(V1).astype(np.float32)
        b -= np.float32(b.max() - level + np.float32(0.5))          # the largest untied entry sits about 0.5 below the level
        if kind == 'ties_high':
            tied = tied[2:]
        elif kind == 'ties_far':
            tied = tied[3:]
        elif kind == 'eos_tie':
            tied = [0] + tied
        elif kind != 'ties':
            raise ValueError(kind)
    b[tied] = level
    rest = np.delete(b, tied)
    assert rest.max() < level and (b[tied] == level).all()
    return b, int(tied[0]), tied


def greedy_logp(bias, tok):
    x = np.asarray(bias, np.float32).astype(np.float64)
    return float(x[tok] - (x.max() + np.log(np.exp(x - x.max()).sum())))


# ---- beam search: searches decided by the tie rules alone -----------------------------------------------------------------------
def beam_form_width(V1):
    """EPW of beam_step_kernel's form for this vocabulary (a lane holds columns lane + 64 i, i < EPW; 0: streamed)."""
    return 8 if V1 <= 512 else (32 if V1 <= 2048 else (80 if V1 <= 5120 else 0))


def beam_class_design(V1, B, kind, seed=0):
    """(bias float32 [V1], L): logits rows on which every comparison of the beam search that matters is an exact tie in float32 and in
    float64 alike (a tie is between sums of identical terms in one order, or between x + y and y + x).
    'one'      a set X of 2B + 3 indices at one level -- V1 - 1, both sides of a lane stride (63, 64, 65) and both sides of the next narrower
               form's width 64 EPW among them -- everything else at least 30 below; L = 5
    'one_eos'  'one' with index 0 in X: <eos> wins slot 0 at once and keeps the result
    'two'      X of 2 indices, a class Y of 2B indices 1.5 below, the rest at least 30 below; L = 2 (x + y = y + x is exact; three terms
               would not be)"""
    rs = np.random.RandomState(2000 + V1 + 17 * B + seed)
    b = (-30.0 - rs.uniform(0.0, 4.0, V1)).astype(np.float32)
    edge = max([w for w in (512, 2048, 5120) if w < V1] or [256])          # the widest narrower form's 64 EPW (256: inside the narrowest)
    anchors = [V1 - 1, 63, 64, edge - 1, edge, 65, 3, V1 - 2]          # (the first 2B + 3 are taken: 5 when B = 1)
    pool = [i for i in dict.fromkeys(anchors) if 0 < i < V1]
    more = [int(i) for i in rs.permutation(np.arange(1, V1)) if int(i) not in pool]
    pool = pool + more

    def take(k, skip=()):
        out = [i for i in pool if i not in skip][:k]
        assert len(out) == k
        return sorted(out)
    if kind in ('one', 'one_eos'):
        X = take(2 * B + 3)
        if kind == 'one_eos':
            X = [0] + X[1:]          # (X is sorted: its smallest member gives way, V1 - 1 stays)
        b[X] = np.float32(1.0)
        return b, 5
    if kind == 'two':
        X = [edge - 1, V1 - 1]
        Y = take(2 * B, skip=X)
        b[X] = np.float32(1.0)
        b[Y] = np.float32(-0.5)
        return b, 2
    raise ValueError(kind)


def beam_reference(bias, N, B, L):
    """tests/beam_ref.beam_search over rows that all carry the float64 log-softmax of `bias` (the state is a dummy)."""
    import torch
    from tests import beam_ref
    x = np.asarray(bias, np.float32).astype(np.float64)
    lp = torch.from_numpy(x - (x.max() + np.log(np.exp(x - x.max()).sum())))

    def step(it, state):
        return lp[None, :].expand(it.shape[0], -1), state
    return beam_ref.beam_search(step, None, N, B, L, permute=lambda state, idx: state)

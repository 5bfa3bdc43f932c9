"""CIDEr-D on the GPU (-m gpu): echr_ciderd_score against the float64 oracle tests/ciderd_ref.py, its edges, its bitwise guarantees, and
the self-critical steps with the device reward.

Gate: 1e-5 absolute on scores and rewards.  Scores lie in [0, 10] and the kernel's arithmetic is fp64, so what separates it from the
oracle is the output's fp32 rounding: <= 2^-21 = 4.8e-7 per score and <= 1e-6 for a reward (a difference of two rounded scores)."""
import functools

import numpy as np
import pytest
import torch

from echr_amd import reward as RW
from echr_amd import synth
from tests import ciderd_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu

TOL = 1e-5


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _words(rs, top, lo, hi):
    return rs.randint(1, top + 1, size=rs.randint(lo, hi + 1)).tolist()


def _pad(row, width):
    return (list(row) + [0] * width)[:width]


def _candidates(rs, docs, L, top, n_rows):
    """n_rows caption rows [n_rows, L] for documents docs[n % len(docs)], cycling four kinds: a random row; a reference with one token
    replaced; a reference with its first bigram repeated in front; the reference itself.  The first random row of a document avoids the
    document's own tokens where it can (a score of exactly 0 needs that: 9 tokens leave little room for chance)."""
    rows, doc_of = [], []
    for n in range(n_rows):
        d = n % len(docs)
        ref = list(docs[d][rs.randint(len(docs[d]))])
        kind = (n // len(docs)) % 4
        if kind == 0:
            used = {t for r in docs[d] for t in r}
            free = [t for t in range(1, top + 1) if t not in used]
            if free and n < len(docs):
                row = [free[i] for i in rs.randint(len(free), size=L)]          # l = L: no end token either
            else:
                row = _words(rs, top, 0, L)
        elif kind == 1:
            row = list(ref)
            if row:
                row[rs.randint(len(row))] = int(rs.randint(1, top + 1))
        elif kind == 2:
            row = ref[:2] + ref
        else:
            row = ref
        rows.append(_pad(row, L))
        doc_of.append(d)
    return np.asarray(rows, np.int64), doc_of


def _make(seed, n_docs, L, top, n_rows, refs_per_doc=(1, 3), words=(3, 7)):
    rs = np.random.RandomState(seed)
    docs = [[_words(rs, top, *words) for _ in range(rs.randint(refs_per_doc[0], refs_per_doc[1] + 1))] for _ in range(n_docs)]
    rows, doc_of = _candidates(rs, docs, L, top, n_rows)
    seqs = [[R.sequence(r, L) for r in d] for d in docs]
    df, n = R.document_frequency(seqs)
    sc = RW.CiderD.from_corpus(docs, L, top).cuda()
    ref_sets = [seqs[d] for d in doc_of]
    packed = sc.pack_refs([docs[d] for d in doc_of]).cuda()
    want = np.asarray(R.score_rows(rows, ref_sets, df, n, L))
    return dict(sc=sc, rows=rows, packed=packed, want=want, ref_sets=ref_sets, df=df, n=n, L=L, docs=docs, doc_of=doc_of)


@functools.lru_cache(maxsize=None)
def _main():
    """9 tokens, L = 8, 16 documents of 1..3 references, 64 rows (16 of each kind)."""
    return _make(11, 16, 8, 9, 64)


def _gpu(c, rows=None, **kw):
    rows = c['rows'] if rows is None else rows
    t = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    return c['sc'].score(t, c['packed'], **kw)


def _check(got, want, what=''):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == np.shape(want) and np.isfinite(got).all()
    err = np.abs(got - want).max() if got.size else 0.0
    print('%s max |gpu - oracle| = %.3e over %d rows' % (what, err, got.size))
    assert err < TOL, (what, err)


# ---- the main case ----------------------------------------------------------------------------------------------------------------
def test_main_case_meets_the_overlap_condition_and_matches_the_oracle():
    c = _main()
    # the condition, on the oracle alone, before the GPU result is looked at
    per, clipped = zip(*[R.order_values(R.sequence(r, c['L']), refs, c['df'], c['n']) for r, refs in zip(c['rows'], c['ref_sets'])])
    frac = (np.asarray(per) != 0.0).mean(0)
    print('rows with a non-zero val_n, n = 1..4: %s; clipped rows %d; zeros %d; tens %d'
          % (frac.tolist(), sum(clipped), int((c['want'] == 0).sum()), int((np.abs(c['want'] - 10.0) < 1e-9).sum())))
    assert (frac >= 0.5).all(), frac
    assert any(clipped)
    assert (c['want'] == 0.0).any() and (np.abs(c['want'] - 10.0) < 1e-9).any()
    assert c['want'].min() >= 0.0 and c['want'].max() <= 10.0 + 1e-9
    got = _gpu(c)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (64,)
    _check(got, c['want'], 'main')
    g = got.cpu().numpy()
    assert (g[c['want'] == 0.0] == 0.0).all() and g.min() >= 0.0 and g.max() <= 10.0


@pytest.mark.parametrize('n_rows', [1, 67])
def test_row_counts(n_rows):
    c = _make(79, 16, 8, 9, 67)
    if n_rows == 1:          # the best-scoring row, alone
        i = int(np.argmax(c['want']))
        assert c['want'][i] > 1.0
        c = dict(c, rows=c['rows'][i:i + 1], want=c['want'][i:i + 1], packed=c['sc'].pack_refs([c['docs'][c['doc_of'][i]]]).cuda())
    _check(_gpu(c), c['want'], 'N = %d' % n_rows)


def test_seq_length_3_has_no_4_gram():
    c = _make(21, 8, 3, 9, 32, words=(0, 3))
    assert all(len(s) <= 3 for refs in c['ref_sets'] for s in refs) and (c['want'] > 0).any()
    _check(_gpu(c), c['want'], 'L = 3')


def test_seq_length_63():
    c = _make(22, 6, 63, 9, 24, words=(40, 63))
    assert max(len(s) for refs in c['ref_sets'] for s in refs) == 63 and (c['want'] > 0).mean() >= 0.5
    assert any(not r.all() for r in c['rows']) and any(r.all() for r in c['rows'])          # rows with and without an end token
    _check(_gpu(c), c['want'], 'L = 63')


def test_one_to_five_references_mixed_in_one_call():
    c = _make(23, 10, 8, 9, 40, refs_per_doc=(1, 5))
    assert {len(r) for r in c['ref_sets']} == {1, 2, 3, 4, 5}
    _check(_gpu(c), c['want'], 'R = 1..5')


def test_single_document_corpus_scores_zero_without_nan():
    c = _make(24, 1, 8, 9, 8)
    assert c['n'] == 1 and not c['want'].any()
    got = _gpu(c).cpu().numpy()
    assert (got == 0.0).all()


@pytest.mark.parametrize('entries', [0, 1])
def test_empty_and_one_entry_tables(entries):
    c = dict(_main())
    df = {(5,): 3} if entries else {}
    n = 7
    keys = [int(RW.pack_keys((5,), 1)[0])] if entries else []
    c['sc'] = RW.CiderD(keys, list(df.values()), n, c['L'], 9).cuda()
    want = np.asarray(R.score_rows(c['rows'], c['ref_sets'], df, n, c['L']))
    assert (want > 0).any()
    if entries:          # the entry matters: without it the oracle's scores move
        assert np.abs(want - np.asarray(R.score_rows(c['rows'], c['ref_sets'], {}, n, c['L']))).max() > 1e-3
    _check(_gpu(c), want, '%d-entry table' % entries)


def _edge_key_case(docs, L, top, cand):
    seqs = [[R.sequence(r, L) for r in d] for d in docs]
    df, n = R.document_frequency(seqs)
    sc = RW.CiderD.from_corpus(docs, L, top).cuda()
    cs = R.sequence(cand, L)
    grams = {g for k in R.ORDERS for g in R.ngrams(cs, k)}
    first, last = RW.unpack_key(sc.keys[0]), RW.unpack_key(sc.keys[-1])
    assert first in grams and last in grams          # the candidate queries the table's first and last key
    want = R.score(cs, seqs[0], df, n)
    for g in (first, last):                          # a miss at either end would move the score
        miss = dict(df)
        del miss[g]
        assert abs(R.score(cs, seqs[0], miss, n) - want) > 1e-3, g
    got = sc.score(torch.tensor([_pad(cand, L)]).cuda(), sc.pack_refs([docs[0]]).cuda())
    _check(got, np.asarray([want]), 'edge keys')
    return sc


def test_queries_equal_to_the_first_and_last_key():
    docs = [[[9, 9, 9, 9, 1]], [[9, 9, 9, 9, 2]], [[3, 4, 0]], [[1, 2]], [[5, 5, 5, 5, 5, 5]]]          # the last one carries no end token
    _edge_key_case(docs, 6, 9, [9, 9, 9, 9, 3])


def test_keys_with_the_top_bit_set():
    top = 39999          # V1 = 40000
    docs = [[[39999, 39999, 39999, 39999, 1]], [[39999, 39999, 39999, 39999, 2]], [[3, 32767, 0]], [[1, 2, 3, 32767]], [[7] * 6]]
    sc = _edge_key_case(docs, 6, top, [39999, 39999, 39999, 39999, 3])
    assert int(sc.keys[-1]) >> 63 == 1 and int((sc.keys >> np.uint64(63)).sum()) >= 2
    # a candidate whose 4-gram sits between the two signed halves of the table
    seqs = [[R.sequence(r, 6) for r in d] for d in docs]
    df, n = R.document_frequency(seqs)
    rows = np.asarray([_pad([1, 2, 3, 32767], 6), _pad([3, 32767], 6), _pad([1, 2, 3, 32766], 6)])
    want = np.asarray(R.score_rows(rows, [seqs[3], seqs[2], seqs[3]], df, n, 6))
    assert abs(want[0] - 10.0) < 1e-9
    _check(sc.score(torch.from_numpy(rows).cuda(), sc.pack_refs([docs[3], docs[2], docs[3]]).cuda()), want, 'top bit')


# ---- widths, dtypes, strides ------------------------------------------------------------------------------------------------------
def _cut_case():
    """The main case with every caption shortened to at most 5 words: any width from 5 up holds all of it."""
    c = dict(_main())
    rows = c['rows'].copy()
    rows[:, 5:] = 0
    c['rows'] = rows
    c['want'] = np.asarray(R.score_rows(rows, c['ref_sets'], c['df'], c['n'], c['L']))
    return c


def test_reward_with_gen_and_greedy_of_different_widths():
    c = _cut_case()
    m = _main()
    gen = torch.from_numpy(np.ascontiguousarray(c['rows'][:, :5])).cuda()          # cut at 5: rows of 5 words have lost their <eos> column
    greedy = torch.from_numpy(m['rows'][::-1].copy()).cuda()                       # width 8, other captions
    want = 0.7 * (c['want'] - np.asarray(R.score_rows(m['rows'][::-1], c['ref_sets'], c['df'], c['n'], c['L'])))
    assert np.abs(want).max() > 1.0
    got = c['sc'].reward(gen, greedy, c['packed'], weight=0.7)
    assert got.dtype == torch.float32 and tuple(got.shape) == (64,)
    _check(got, want, 'reward')
    _check(RW.CiderDReward(c['sc'], 0.7)(gen, greedy, c['packed']), want, 'CiderDReward')


def test_int32_and_strided_inputs_are_bitwise_the_contiguous_int64_result():
    c = _main()
    base = _gpu(c)
    rows = torch.from_numpy(c['rows']).cuda()
    assert torch.equal(_gpu(c, rows.to(torch.int32)), base)
    wide = torch.full((64, 16), 7, dtype=torch.int64, device='cuda')
    wide[:, ::2] = rows
    assert not wide[:, ::2].is_contiguous() and torch.equal(_gpu(c, wide[:, ::2]), base)
    tr = rows.t().contiguous().t()                                                   # column-major storage
    assert tr.stride() == (1, 64) and torch.equal(_gpu(c, tr), base)
    assert torch.equal(_gpu(c, tr.to(torch.int32)), base)


@pytest.mark.parametrize('T', [5, 7])
def test_columns_past_the_width_are_never_read(T):
    c = _cut_case()
    L = c['L']
    clean = torch.from_numpy(c['rows']).cuda()
    base = _gpu(c, clean)
    _check(base, c['want'], 'clean')
    junk = clean.clone()
    junk[:, T:] = torch.randint(1, 10, (64, L - T), device='cuda')
    junk[:, L - 1] = 2 ** 40 + 5                                                     # nothing a decoder could have written
    assert torch.equal(_gpu(c, junk, width=T), base)                                 # the host width
    counts = torch.full((L + 1,), 3, dtype=torch.int32, device='cuda')
    counts[T + 1:] = 0                                                               # nobody unfinished after step T + 1: the cut is T
    assert torch.equal(_gpu(c, junk, counts=counts), base)                           # the device counts
    counts0 = counts.clone()
    counts0[0] = 0                                                                   # element 0 is not a step count (functional._stop_step)
    assert torch.equal(_gpu(c, junk, counts=counts0), base)


def test_counts_that_never_reach_zero_give_the_full_width():
    c = _main()
    counts = torch.full((c['L'] + 1,), 2, dtype=torch.int32, device='cuda')
    assert torch.equal(_gpu(c, counts=counts), _gpu(c))


def test_two_calls_and_a_row_permutation_agree_bitwise():
    c = _main()
    a, b = _gpu(c), _gpu(c)
    assert torch.equal(a, b)
    perm = np.random.RandomState(5).permutation(64)
    packed = c['sc'].pack_refs([c['docs'][c['doc_of'][i]] for i in perm]).cuda()
    got = c['sc'].score(torch.from_numpy(c['rows'][perm]).cuda(), packed)
    assert torch.equal(got, a[torch.from_numpy(perm).cuda()])
    one = c['sc'].score(torch.from_numpy(c['rows'][17:18]).cuda(), c['sc'].pack_refs([c['docs'][c['doc_of'][17]]]).cuda())
    assert torch.equal(one, a[17:18])                                                # a row alone in its launch


# ---- the steps --------------------------------------------------------------------------------------------------------------------
CASE = 'vbscst'


def _perturb(rs, words, top):
    w = list(words)
    if w:
        w[rs.randint(len(w))] = int(rs.randint(1, top + 1))
    return w


@functools.lru_cache(maxsize=None)
def _step_case():
    """The vbscst videos; an event's references are its own label, a perturbed copy of it, and -- the labels are random words, which a
    random model's captions share next to nothing with -- perturbed copies of the captions the reference's fixture holds for the event."""
    from tests import scst_batch_ref as SR
    opt, params, videos = synth.make_vbatch(CASE)
    L, top = opt.CG_seq_length, opt.CG_vocab_size
    g = U.gold('case_scst_batch.npz')
    gens, _, greedys, _, _ = SR.load_fixture(g, len(videos))
    rs = np.random.RandomState(9)
    docs = []
    for v, vid in enumerate(videos):
        for e, lab in enumerate(np.asarray(vid['labels'])):
            own = list(R.label_sequence(lab, L))
            refs = [own, _perturb(rs, [t for t in own if t], top)]
            for cap in (gens[v][e], greedys[v][e]):
                words = [int(t) for t in R.sequence(cap, L) if t]
                refs.append(_perturb(rs, words, top) if rs.rand() < 0.7 else words)
            docs.append(refs)
    seqs = [[R.sequence(r, L) for r in d] for d in docs]
    df, n = R.document_frequency(seqs)
    sc = RW.CiderD.from_corpus(docs, L, top).cuda()
    return dict(opt=opt, params=params, videos=videos, docs=docs, seqs=seqs, df=df, n=n, sc=sc, L=L,
                gen=SR.stack(gens, videos, np.int64), packed=sc.pack_refs(docs).cuda())


def _batch(videos):
    from echr_amd.batch import VideoBatch
    b = VideoBatch.from_videos([{k: v[k] for k in ('c3d', 'tap', 'lda', 'ind', 'soi')} for v in videos], device=torch.device('cuda'))
    assert b.refs is None
    return b


def _fused(c):
    from echr_amd.fused import FusedTrainStep
    from echr_amd.optim import ClampAdam
    m = U.build_gpu_model(c['opt'], c['params'], True)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
    return m, FusedTrainStep(m, o)


def _want_matrix(c, gen_h, greedy_h, slices_widths, weight, seqs=None):
    """The oracle's reward matrix: one value per caption over its video's own width, zero past it."""
    seqs = c['seqs'] if seqs is None else seqs
    r = np.asarray(R.reward_rows(gen_h.numpy(), greedy_h.numpy(), seqs, c['df'], c['n'], c['L'], weight))
    want = np.zeros(tuple(gen_h.shape))
    for s, w in slices_widths:
        want[s, :w] = r[s, None]
    return want, r


@pytest.mark.parametrize('pinned', [False, True])
def test_batch_step_reward_matrix_and_bitwise_replay(pinned):
    import echr_amd
    from echr_amd.fused import SelfCriticalBatchStep
    c = _step_case()
    echr_amd.set_deterministic(True)
    try:
        m, fs = _fused(c)
        b = _batch(c['videos'])
        step = SelfCriticalBatchStep(fs, RW.CiderDReward(c['sc'], weight=0.5))
        m.set_dropout_state(77, 3)
        b.refs = c['packed']
        loss, gen_h, greedy_h, reward, vw = step(b, gen_result=c['gen'] if pinned else None, step=False)
        want, r = _want_matrix(c, gen_h, greedy_h, zip(b.event_slices, vw.tolist()), 0.5)
        assert len(set(vw.tolist())) > 1 or not pinned                               # videos cut at different widths
        assert (r != 0).mean() >= 0.5 and len(np.unique(np.round(r, 6))) > len(r) // 2
        got = reward.numpy()
        assert got.dtype == np.float32 and got.shape == want.shape
        print('batch step (%s): max |reward - oracle| = %.3e' % ('pinned' if pinned else 'sampled', np.abs(got - want).max()))
        assert np.abs(got - want).max() < TOL
        for s, w in zip(b.event_slices, vw.tolist()):                                # broadcast per caption, zero past the video's width
            assert (got[s, :w] == got[s, :1]).all() and not got[s, w:].any()
        l1, g1 = float(loss), fs.arena.flat_g.clone()
        # the same call with that matrix as reward=: same kernels, same inputs
        m.set_dropout_state(77, 3)
        b.refs = None
        loss2 = SelfCriticalBatchStep(fs)(b, gen_result=gen_h, reward=reward, step=False)[0]
        assert float(loss2) == l1 and torch.equal(fs.arena.flat_g, g1)
        assert float(g1.abs().max()) > 0
    finally:
        echr_amd.set_deterministic(False)


def test_single_video_step_reward_and_bitwise_replay():
    import echr_amd
    from echr_amd.fused import SelfCriticalStep
    c = _step_case()
    v = 1
    vid = c['videos'][v]
    first = sum(len(x['soi']) for x in c['videos'][:v])
    rows = slice(first, first + len(vid['soi']))
    packed = c['sc'].pack_refs(c['docs'][rows]).cuda()
    echr_amd.set_deterministic(True)
    try:
        m, fs = _fused(c)
        tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
        step = SelfCriticalStep(fs, RW.CiderDReward(c['sc'], weight=2.0))
        for gen_result in (None, c['gen'][rows][:, :int((c['gen'][rows] > 0).sum(1).max())]):
            m.set_dropout_state(78, 5)
            loss, gen_h, greedy_h, reward = step(tap, c3d, lda, vid['ind'], vid['soi'], gen_result=gen_result, refs=packed, step=False)
            want, r = _want_matrix(c, gen_h, greedy_h, [(slice(None), gen_h.shape[1])], 2.0, c['seqs'][rows])
            print('single step: max |reward - oracle| = %.3e' % np.abs(reward.numpy() - want).max())
            assert np.abs(reward.numpy() - want).max() < TOL and (r != 0).any()
            l1, g1 = float(loss), fs.arena.flat_g.clone()
            m.set_dropout_state(78, 5)
            loss2 = SelfCriticalStep(fs)(tap, c3d, lda, vid['ind'], vid['soi'], gen_result=gen_h, reward=reward, step=False)[0]
            assert float(loss2) == l1 and torch.equal(fs.arena.flat_g, g1)
    finally:
        echr_amd.set_deterministic(False)


def _host_only(method, name):
    def guarded(self, *a, **k):
        assert not self.is_cuda, 'device read through .%s() instead of .cpu()' % name
        return method(self, *a, **k)
    return guarded


def _host_reads(monkeypatch, call):
    """Every device-to-host read of `call` -- the steps read through Tensor.cpu() and nothing else -- as (the stream was idle when the
    read was issued, shape, dtype), plus the number of explicit synchronisations.  A read issued on an idle stream is a copy; a read
    issued behind queued work is a drain."""
    log, syncs = [], [0]
    orig_cpu, orig_sync = torch.Tensor.cpu, torch.cuda.synchronize

    def cpu(self, *a, **k):
        if self.is_cuda:
            log.append((bool(torch.cuda.current_stream().query()), tuple(self.shape), self.dtype))
        return orig_cpu(self, *a, **k)

    def sync(*a, **k):
        syncs[0] += 1
        return orig_sync(*a, **k)
    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, 'cpu', cpu)
        mp.setattr(torch.cuda, 'synchronize', sync)
        for name in ('item', 'tolist', 'numpy'):          # any other way out of the device would hide a drain from this count
            mp.setattr(torch.Tensor, name, _host_only(getattr(torch.Tensor, name), name))
        call()
    return log, syncs[0]


def test_the_device_reward_adds_one_small_copy_and_no_drain(monkeypatch):
    """How a drain is observed: Tensor.cpu() is the steps' only way to the host (the wrapper refuses .item() / .tolist() / .numpy() on
    device tensors and counts torch.cuda.synchronize), and the wrapper asks the stream whether it is idle as each read is issued.  With a
    plain callable every read after the decode counts' one finds the stream idle; with CiderDReward there is exactly one read more, the
    [N] fp32 reward, it comes last and it too finds the stream idle -- nothing was queued behind the drain that today's path already pays."""
    from echr_amd.fused import SelfCriticalBatchStep, SelfCriticalStep
    c = _step_case()
    m, fs = _fused(c)
    b, bd = _batch(c['videos']), _batch(c['videos'])
    bd.refs = c['packed']
    N = b.n_events
    plain = SelfCriticalBatchStep(fs, lambda gen_v, greedy_v: np.zeros(gen_v.shape[0], np.float32))
    dev = SelfCriticalBatchStep(fs, RW.CiderDReward(c['sc']))
    plain(b, step=False), dev(bd, step=False)          # (first calls allocate)
    torch.cuda.synchronize()
    p_log, p_sync = _host_reads(monkeypatch, lambda: plain(b, step=False))
    torch.cuda.synchronize()
    d_log, d_sync = _host_reads(monkeypatch, lambda: dev(bd, step=False))
    torch.cuda.synchronize()
    print('batch step reads, callable: %s\nbatch step reads, CiderDReward: %s' % (p_log, d_log))
    assert p_sync == d_sync == 0
    assert len(d_log) == len(p_log) + 1
    assert [x[1:] for x in d_log[:-1]] == [x[1:] for x in p_log]
    assert d_log[-1] == (True, (N,), torch.float32)
    assert all(idle for idle, _, _ in p_log[1:]) and all(idle for idle, _, _ in d_log[1:])          # one drain at the most, the first read
    # the single-video step: its two decodes each read their counts today; the reward's read comes behind both, on an idle stream
    vid = c['videos'][0]
    n0 = len(vid['soi'])
    packed = c['sc'].pack_refs(c['docs'][:n0]).cuda()
    tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
    args = (tap, c3d, lda, vid['ind'], vid['soi'])
    plain1 = SelfCriticalStep(fs, lambda gen, greedy: np.zeros(gen.shape[0], np.float32))
    dev1 = SelfCriticalStep(fs, RW.CiderDReward(c['sc']))
    plain1(*args, step=False), dev1(*args, refs=packed, step=False)
    torch.cuda.synchronize()
    p_log, p_sync = _host_reads(monkeypatch, lambda: plain1(*args, step=False))
    torch.cuda.synchronize()
    d_log, d_sync = _host_reads(monkeypatch, lambda: dev1(*args, refs=packed, step=False))
    torch.cuda.synchronize()
    print('single step reads, callable: %s\nsingle step reads, CiderDReward: %s' % (p_log, d_log))
    assert p_sync == d_sync == 0 and len(d_log) == len(p_log) + 1
    assert d_log[-1] == (True, (n0,), torch.float32)
    assert [x[1:] for x in d_log[:-1]] == [x[1:] for x in p_log]
    assert all(idle for idle, _, _ in p_log[2:]) and all(idle for idle, _, _ in d_log[2:])          # the two decode reads, then copies


def test_refs_rules_on_the_steps():
    from echr_amd.fused import SelfCriticalBatchStep
    c = _step_case()
    m, fs = _fused(c)
    b = _batch(c['videos'])
    from echr_amd.fused import SelfCriticalStep
    with pytest.raises(ValueError):
        SelfCriticalBatchStep(fs, RW.CiderDReward(c['sc']))(b, step=False)
    with pytest.raises(ValueError):
        SelfCriticalBatchStep(fs, RW.CiderDReward(c['sc'])).handover(b)
    b.refs = c['packed']
    with pytest.raises(TypeError):
        SelfCriticalBatchStep(fs, lambda a, g: np.zeros(a.shape[0]))(b, step=False)
    vid = c['videos'][0]
    args = tuple(torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda')) + (vid['ind'], vid['soi'])
    with pytest.raises(ValueError):
        SelfCriticalStep(fs, RW.CiderDReward(c['sc']))(*args, step=False)
    with pytest.raises(TypeError):
        SelfCriticalStep(fs, lambda a, g: np.zeros(a.shape[0]))(*args, refs=c['sc'].pack_refs(c['docs'][:len(vid['soi'])]), step=False)


def test_ciderd_of_a_caption_videos_result():
    from echr_amd import eval_utils
    c = _step_case()
    m = U.build_gpu_model(c['opt'], c['params'], False)
    b = _batch(c['videos'])
    with torch.no_grad():
        seq, _ = m.forward_batch(b, mode='eval')
    got = eval_utils.ciderd_of({'seq': seq}, c['sc'], c['packed'])
    assert eval_utils.ciderd_of(seq, c['sc'], c['packed']) == got
    empty = eval_utils.ciderd_of({'seq': None}, c['sc'], c['packed'])
    assert abs(empty - float(np.mean(R.score_rows(np.zeros((b.n_events, 0), np.int64), c['seqs'], c['df'], c['n'], c['L'])))) < TOL
    rows = seq.cpu().numpy() if isinstance(seq, torch.Tensor) else np.zeros((b.n_events, 0), np.int64)
    want = float(np.mean(R.score_rows(rows, c['seqs'], c['df'], c['n'], c['L'])))
    assert isinstance(got, float) and abs(got - want) < TOL


@pytest.mark.parametrize('m_batch', [1, 3])
def test_example_driver_runs_with_the_ciderd_reward(m_batch):
    """examples/train_synthetic.py --self_critical --reward ciderd: SelfCriticalStep (m_batch 1) and SelfCriticalBatchStep (V = 3) with the
    corpus built from the synthetic labels; finite losses, the parameters move."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('train_synthetic', os.path.join(os.path.dirname(U.GOLD), '..', 'examples', 'train_synthetic.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist, cg, _ = mod.main(['--self_critical', '--reward', 'ciderd', '--iters', '3', '--m_batch', str(m_batch), '--quiet', '--events', '4',
                            '--segments', '12', '--vocab', '30'])
    assert len(hist) == 3 and np.isfinite(hist).all()
    with pytest.raises(SystemExit):
        mod.main(['--reward', 'ciderd', '--iters', '1', '--quiet'])

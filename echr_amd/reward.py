"""CIDEr-D over token ids on the device: the reward of self-critical training -- score(sampled) - score(greedy)
against the events' ground-truth captions -- and a validation metric that needs nothing installed.

The corpus table is built once on the host (CiderD.from_corpus); scoring is echr_ciderd_score (csrc/reward.hip), one workgroup per
caption, fp64 in a fixed order.  There is no host fallback.

The sequence of a caption row under seq_length L: the l tokens before the row's first 0 (all of them when there is none), then one end
token 0 iff l < L -- whatever width the matrix was cut at.  A reference row is a label row [<bos> = 0 | words | 0 ...], whose first
column is dropped, or a plain token list; a row that starts with 0 and has more than one entry is read as a label row."""
import ctypes as C
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L

MAX_SEQ_LENGTH = 63          # echr_ciderd_score: a sequence's n-grams live in one workgroup's LDS
MAX_V1 = 65535               # token + 1 fills a 16-bit key field
ORDERS = 4


def _sequence(row, seq_length, vocab_size=None):
    """The token sequence (np.int64) of one label row / token list."""
    row = np.asarray(row.cpu() if isinstance(row, torch.Tensor) else row, dtype=np.int64).reshape(-1)
    if row.size > 1 and row[0] == 0:
        row = row[1:]          # the <bos> column
    zeros = np.flatnonzero(row == 0)
    n = int(zeros[0]) if zeros.size else row.size
    if n > seq_length:
        raise ValueError('a reference of %d words does not fit seq_length = %d' % (n, seq_length))
    top = MAX_V1 - 1 if vocab_size is None else int(vocab_size)
    if n and (row[:n].min() < 0 or row[:n].max() > top):
        raise ValueError('token outside the vocabulary [0, %d]: %s' % (top, row[:n].tolist()))
    return np.concatenate([row[:n], np.zeros(1, np.int64)]) if n < seq_length else row[:n].copy()


def pack_keys(seq, n):
    """uint64 keys of the order-n n-grams of a sequence: sum (tok_i + 1) << 16 i."""
    s = np.asarray(seq, dtype=np.uint64) + np.uint64(1)
    m = len(s) - n + 1
    if m <= 0:
        return np.zeros(0, np.uint64)
    k = np.zeros(m, np.uint64)
    for i in range(n):
        k |= s[i:i + m] << np.uint64(16 * i)
    return k


def unpack_key(key):
    """The token tuple of a key (the inverse of pack_keys for one n-gram)."""
    key, out = int(key), []
    while key:
        out.append((key & 0xFFFF) - 1)
        key >>= 16
    return tuple(out)


class PackedRefs(NamedTuple):
    """References in the kernel's form: refs int32 [R_tot, L] (zero-padded sequences), ref_len int32 [R_tot], ref_offset int32 [N + 1]."""
    refs: torch.Tensor
    ref_len: torch.Tensor
    ref_offset: torch.Tensor

    def to(self, device):
        return PackedRefs(*(t.to(device) for t in self))

    def cuda(self, device=None):
        return self.to(torch.device('cuda') if device is None else device)


def pack_refs(label_sets, seq_length, vocab_size=None):
    """label_sets: per caption row (event), the list of its references (label rows or token lists).  Returns PackedRefs (host tensors);
    ValueError for an event without a reference or a token outside the vocabulary ([0, vocab_size], or the key range without one)."""
    seq_length = int(seq_length)
    rows, lens, offs = [], [], [0]
    for n, refs in enumerate(label_sets):
        refs = list(refs)
        if not refs:
            raise ValueError('event %d has no reference' % n)
        for r in refs:
            s = _sequence(r, seq_length, vocab_size)
            rows.append(np.pad(s, (0, seq_length - len(s))))
            lens.append(len(s))
        offs.append(len(rows))
    refs = np.stack(rows).astype(np.int32) if rows else np.zeros((0, seq_length), np.int32)
    return PackedRefs(torch.from_numpy(refs), torch.from_numpy(np.asarray(lens, np.int32)), torch.from_numpy(np.asarray(offs, np.int32)))


class CiderD(object):
    """The corpus table (sorted exact n-gram keys with their document frequencies, n_docs) and the scoring entry points."""

    def __init__(self, keys, df, n_docs, seq_length, vocab_size):
        seq_length, vocab_size = int(seq_length), int(vocab_size)
        if not 1 <= seq_length <= MAX_SEQ_LENGTH:
            raise ValueError('seq_length must be in [1, %d] (got %d)' % (MAX_SEQ_LENGTH, seq_length))
        if vocab_size + 1 > MAX_V1:
            raise ValueError('exact n-gram keys hold token ids up to %d: vocab_size + 1 = %d is refused' % (MAX_V1 - 1, vocab_size + 1))
        keys = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64).reshape(-1))
        df = np.ascontiguousarray(np.asarray(df, dtype=np.int32).reshape(-1))
        if keys.shape != df.shape:
            raise ValueError('keys and df differ in length (%d, %d)' % (keys.size, df.size))
        if keys.size > 1 and not (keys[1:] > keys[:-1]).all():
            raise ValueError('keys must be strictly increasing as uint64')
        if int(n_docs) < 1:
            raise ValueError('n_docs must be at least 1')
        self.keys, self.df, self.n_docs, self.seq_length, self.vocab_size = keys, df, int(n_docs), seq_length, vocab_size
        self.device = torch.device('cpu')
        self._dev = None

    @classmethod
    def from_corpus(cls, ref_sets, seq_length, vocab_size):
        """ref_sets: the documents, each the list of one event's references (label rows or token lists)."""
        seq_length, vocab_size = int(seq_length), int(vocab_size)
        if not 1 <= seq_length <= MAX_SEQ_LENGTH:
            raise ValueError('seq_length must be in [1, %d] (got %d)' % (MAX_SEQ_LENGTH, seq_length))
        if vocab_size + 1 > MAX_V1:
            raise ValueError('exact n-gram keys hold token ids up to %d: vocab_size + 1 = %d is refused' % (MAX_V1 - 1, vocab_size + 1))
        per_doc, n_docs = [], 0
        for d, doc in enumerate(ref_sets):
            doc = list(doc)
            if not doc:
                raise ValueError('document %d has no reference' % d)
            n_docs += 1
            ks = [pack_keys(s, n) for s in (_sequence(r, seq_length, vocab_size) for r in doc) for n in range(1, ORDERS + 1)]
            per_doc.append(np.unique(np.concatenate(ks)))
        if n_docs == 0:
            raise ValueError('the corpus has no document')
        keys, df = np.unique(np.concatenate(per_doc), return_counts=True)
        return cls(keys, df, n_docs, seq_length, vocab_size)

    # ---- the table ----
    def idf(self):
        """float64 [n_keys]: log(n_docs) - log(max(1, df))."""
        return math.log(self.n_docs) - np.log(np.maximum(1, self.df).astype(np.float64))

    def state_dict(self):
        return {'keys': torch.from_numpy(self.keys.view(np.int64).copy()), 'df': torch.from_numpy(self.df.copy()), 'n_docs': self.n_docs,
                'seq_length': self.seq_length, 'vocab_size': self.vocab_size}

    def load_state_dict(self, sd):
        keys = np.asarray(torch.as_tensor(sd['keys']).cpu().numpy(), dtype=np.int64).view(np.uint64)
        self.__init__(keys, torch.as_tensor(sd['df']).cpu().numpy(), sd['n_docs'], sd['seq_length'], sd['vocab_size'])
        return self

    @classmethod
    def from_state_dict(cls, sd):
        return cls.__new__(cls).load_state_dict(sd)

    def to(self, device):
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device != self.device:
            self.device, self._dev = device, None
        if device.type == 'cuda' and self._dev is None:
            self._dev = (torch.from_numpy(self.keys.view(np.int64)).to(device), torch.from_numpy(self.idf()).to(device))
        return self

    def cuda(self, device=None):
        return self.to('cuda' if device is None else device)

    def pack_refs(self, label_sets):
        return pack_refs(label_sets, self.seq_length, self.vocab_size)

    # ---- scoring ----
    def device_refs(self, refs):
        """`refs` (PackedRefs or any (refs, ref_len, ref_offset)) on the table's device, int32 and contiguous; a no-op for PackedRefs.to()'s
        output.  Host references are uploaded here -- a caller inside an iteration does that once, outside it."""
        out = []
        for t in refs:
            t = torch.as_tensor(t)
            if t.device != self.device or t.dtype != torch.int32 or not t.is_contiguous():
                t = t.to(device=self.device, dtype=torch.int32).contiguous()
            out.append(t)
        if len(out) != 3 or out[0].dim() != 2 or out[0].shape[1] != self.seq_length or out[1].numel() != out[0].shape[0]:
            raise ValueError('refs must be (refs [R_tot, %d], ref_len [R_tot], ref_offset [N + 1])' % self.seq_length)
        return PackedRefs(*out)

    def _launch(self, seq, refs, width=None, counts=None, base=None, weight=1.0):
        if not isinstance(seq, torch.Tensor) or not seq.is_cuda:
            raise L.EchrHipError('captions must live on the GPU (got %s); echr_amd has no CPU path'
                                 % (seq.device if isinstance(seq, torch.Tensor) else type(seq).__name__))
        if self.device.type != 'cuda':
            self.to(seq.device)
        if seq.device != self.device:
            raise L.EchrHipError('captions on %s, the corpus table on %s' % (seq.device, self.device))
        if seq.dtype not in (torch.int32, torch.int64) or seq.dim() != 2:
            raise L.EchrHipError('captions must be int32 or int64 [N, T] (got %s %s)' % (seq.dtype, tuple(seq.shape)))
        lib = L.load()
        refs = self.device_refs(refs)
        N = seq.shape[0]
        if refs.ref_offset.numel() != N + 1:
            raise ValueError('ref_offset names %d caption rows, the captions have %d' % (refs.ref_offset.numel() - 1, N))
        T = seq.shape[1] if width is None else int(width)
        if counts is None and not 0 <= T <= min(seq.shape[1], self.seq_length):
            raise ValueError('width %d outside [0, min(%d columns, seq_length = %d)]' % (T, seq.shape[1], self.seq_length))
        if counts is not None and seq.shape[1] < self.seq_length:
            raise ValueError('a decode\'s counts need its uncut [N, %d] captions (got %d columns)' % (self.seq_length, seq.shape[1]))
        keys, idf = self._dev
        out = torch.empty(N, device=self.device, dtype=torch.float32)
        a = L.CiderdArgs(N, self.seq_length, seq.data_ptr(), 1 if seq.dtype == torch.int32 else 0, T, seq.stride(0), seq.stride(1),
                         L.ptr(counts, torch.int32, 'counts') if counts is not None else None,
                         L.ptr(refs.refs, torch.int32), L.ptr(refs.ref_len, torch.int32), L.ptr(refs.ref_offset, torch.int32),
                         refs.refs.shape[0], keys.numel(), L.ptr(keys, torch.int64) if keys.numel() else None,
                         L.ptr(idf, torch.float64) if keys.numel() else None, math.log(self.n_docs),
                         L.ptr(base) if base is not None else None, float(weight), L.ptr(out))
        L.check(lib.echr_ciderd_score(C.byref(a), L.stream_ptr()), 'ciderd_score')
        return out

    def score(self, seq, refs, width=None, counts=None):
        """CIDEr-D fp32 [N] (device) of the caption rows seq [N, T] (int32 / int64, any strides) against `refs`.  `width`: read columns
        < width only; `counts`: a decode's device n_unfinished [seq_length + 1] -- the width is derived on the device as the host cuts
        the decode's output, and seq is the decode's uncut matrix."""
        return self._launch(seq, refs, width, counts)

    def reward(self, gen, greedy, refs, weight=1.0, gen_width=None, gen_counts=None, greedy_width=None, greedy_counts=None):
        """weight * (score(gen) - score(greedy)), fp32 [N] on the device: what RewardCriterion takes as its reward."""
        refs = self.device_refs(refs) if self.device.type == 'cuda' else refs
        base = self._launch(greedy, refs, greedy_width, greedy_counts)
        return self._launch(gen, refs, gen_width, gen_counts, base=base, weight=weight)


class CiderDReward(object):
    """The reward object SelfCriticalStep / SelfCriticalBatchStep accept as reward_fn: with it the step scores both decodes on the device
    (their full-width sequences and device counts) before the iteration's one host read.  The packed references of the call's events, in
    row order, come as SelfCriticalStep's `refs=` and as the batch's `VideoBatch.refs`.  Called directly it is scorer.reward on device
    captions."""

    def __init__(self, scorer, weight=1.0):
        if not isinstance(scorer, CiderD):
            raise TypeError('CiderDReward wraps a CiderD scorer')
        self.scorer, self.weight = scorer, float(weight)

    def __call__(self, gen, greedy, refs, **widths):
        return self.scorer.reward(gen, greedy, refs, self.weight, **widths)


def check_reward_refs(reward_fn, refs, reward=None):
    """The refs= rules of the self-critical steps: a CiderDReward that is going to be called needs refs; refs with a plain callable is a
    TypeError.  Returns True when the device reward runs."""
    device = isinstance(reward_fn, CiderDReward)
    if refs is not None and not device:
        raise TypeError('references (refs= / VideoBatch.refs) go with a CiderDReward reward_fn: a plain callable receives the captions only')
    if device and reward is None and refs is None:
        raise ValueError('a CiderDReward needs the packed references of the call\'s events (echr_amd.reward.pack_refs): refs= / VideoBatch.refs')
    return device and reward is None

"""The dense-caption scoring contract as plain Python over float64 / Python ints: tIoU matching, Recall /
Precision, corpus BLEU-1..4 per video, ROUGE-L and (through a callable) CIDEr-D over the matched pairs.  Shares nothing with the package;
the n-gram key packing of section 4s is restated here."""
import math
from collections import Counter

BETA = 1.2
ORDERS = (1, 2, 3, 4)
SCORES = ('Recall', 'Precision', 'Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L', 'CIDErD')


def words(row):
    """The tokens before the row's first 0, all of them when there is none."""
    out = []
    for t in row:
        if int(t) == 0:
            break
        out.append(int(t))
    return out


def iou(s1, e1, s2, e2):
    s1, e1, s2, e2 = float(s1), float(e1), float(s2), float(e2)
    inter = max(0.0, min(e1, e2) - max(s1, s2))
    union = min(max(e1, e2) - min(s1, s2), (e2 - s2) + (e1 - s1))
    return inter / (union + 1e-8)


def key(gram):
    """sum (tok_i + 1) << 16 i: exact for tokens <= 65534 and orders <= 4."""
    k = 0
    for i, t in enumerate(gram):
        k |= (int(t) + 1) << (16 * i)
    return k


def keys(seq, n):
    return Counter(key(seq[i:i + n]) for i in range(len(seq) - n + 1))


def lcs(a, b):
    row = [0] * (len(b) + 1)
    for x in a:
        prev = 0
        for j, y in enumerate(b):
            cur = row[j + 1]
            row[j + 1] = prev + 1 if x == y else max(row[j + 1], row[j])
            prev = cur
    return row[len(b)]


def pair_stats(cand, ref):
    """(match_1..4, len_c, len_r, lcs) of a candidate's words against a reference's words; ref None is the unmatched pair."""
    if ref is None:
        return (0, 0, 0, 0, len(cand), 1, 0)
    m = []
    for n in ORDERS:
        kc, kr = keys(cand, n), keys(ref, n)
        m.append(sum(min(tf, kr.get(g, 0)) for g, tf in kc.items()))
    return tuple(m) + (len(cand), len(ref), lcs(cand, ref))


def rouge_l(l, len_c, len_r):
    if l <= 0 or len_c <= 0 or len_r <= 0:
        return 0.0
    P, R = l / len_c, l / len_r
    return (1.0 + BETA ** 2) * P * R / (R + BETA ** 2 * P)


def bleu(stats):
    """Bleu_1..4 of a video's pairs (corpus level, one reference each)."""
    c = sum(s[4] for s in stats)
    r = sum(s[5] for s in stats)
    ratio = (c + 1e-15) / (r + 1e-9)
    bp = 1.0 if ratio >= 1.0 else math.exp(1.0 - 1.0 / ratio)
    out, prod = [], 1.0
    for n in ORDERS:
        match = sum(s[n - 1] for s in stats)
        guess = sum(max(s[4] - n + 1, 0) for s in stats)
        prod *= (match + 1e-15) / (guess + 1e-9)
        out.append(prod ** (1.0 / n) * bp)
    return out


def _mean(xs):
    s = 0.0
    for x in xs:          # in order, one rounding per add
        s += x
    return s / len(xs)


def evaluate(pred_stamps, pred_offset, captions, gt_stamps, gt_offset, references, tious, cider=None):
    """captions: one token row per prediction, or None (detection only); references: one token row per ground truth (read up to its first
    0); cider: None or a callable (prediction row, ground-truth row) -> float.  Returns a dict: 'pairs'[k] the (prediction, ground truth or
    -1) list at tious[k], 'stats'[k] the per-pair integers, 'video'[name][k][v], 'n_pairs'[k][v], 'n_unmatched'[k][v], name -> [k] means
    over the videos, and 'f1'[k]."""
    V = len(gt_offset) - 1
    caps = None if captions is None else [words(r) for r in captions]
    refs = [words(r) for r in references]
    out = {'pairs': [], 'stats': [], 'video': {n: [] for n in SCORES}, 'n_pairs': [], 'n_unmatched': []}
    for tau in tious:
        tau = float(tau)
        pairs, stats = [], []
        video = {n: [] for n in SCORES}
        n_pairs, n_unmatched = [], []
        for v in range(V):
            p0, p1, g0, g1 = int(pred_offset[v]), int(pred_offset[v + 1]), int(gt_offset[v]), int(gt_offset[v + 1])
            assert g1 > g0
            m = {(p, g): iou(pred_stamps[p][0], pred_stamps[p][1], gt_stamps[g][0], gt_stamps[g][1]) for p in range(p0, p1) for g in range(g0, g1)}
            video['Precision'].append(sum(any(m[p, g] > tau for g in range(g0, g1)) for p in range(p0, p1)) / (p1 - p0) if p1 > p0 else 0.0)
            video['Recall'].append(sum(any(m[p, g] > tau for p in range(p0, p1)) for g in range(g0, g1)) / (g1 - g0))
            mine = []
            for p in range(p0, p1):
                partners = [g for g in range(g0, g1) if m[p, g] >= tau]
                mine.extend((p, g) for g in (partners or [-1]))
            n_pairs.append(len(mine))
            n_unmatched.append(sum(g < 0 for _, g in mine))
            st = [pair_stats(caps[p], refs[g] if g >= 0 else None) for p, g in mine] if caps is not None else []
            pairs.extend(mine)
            stats.extend(st)
            if caps is None or not mine:
                for n in SCORES[2:]:
                    video[n].append(0.0)
                continue
            for n, b in zip(ORDERS, bleu(st)):
                video['Bleu_%d' % n].append(b)
            video['ROUGE_L'].append(_mean([rouge_l(s[6], s[4], s[5]) for s in st]))
            video['CIDErD'].append(_mean([cider(p, g) if g >= 0 else 0.0 for p, g in mine]) if cider is not None else 0.0)
        out['pairs'].append(pairs)
        out['stats'].append(stats)
        out['n_pairs'].append(n_pairs)
        out['n_unmatched'].append(n_unmatched)
        for n in SCORES:
            out['video'][n].append(video[n])
            out.setdefault(n, []).append(_mean(video[n]))
    out['f1'] = [2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(out['Precision'], out['Recall'])]
    return out

#!/usr/bin/env python3
"""Batched proposal encoder against V sequential single-video calls, in one process (D = 500, H = 512, K = 256).

For V = 1 / 4 / 8 / 16 videos of T = 256 rows and one mixed-length batch (8 videos, lengths spread over 32..256), in the persistent and the
launch-per-step wavefront form: forward, and forward + backward, of SST.forward_batch and of V SST.forward calls (+ one backward each).
Every figure is the median of five timed regions of `--iters` iterations each (device events around the region, one warm-up region first);
`spread` is (max - min) / median of the five.  Prints ONE JSON line; --out writes it to a file as well.

usage: python tools/sst_batch_bench.py [--iters 10] [--out profiles/sst_batch_bench.json] [--stamps]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from echr_amd import _lib, models, synth

D, H, K = 500, 512, 256


def timed(fn, iters, regions=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    med = float(np.median(ms))
    return dict(ms=round(med, 4), spread=round((max(ms) - min(ms)) / med, 4))


def bench_case(m, lengths, iters):
    dev = torch.device('cuda')
    rs = np.random.RandomState(len(lengths))
    xs = [torch.from_numpy(rs.standard_normal((t, D)).astype(np.float32)).to(dev) for t in lengths]
    ro = [0]
    for t in lengths:
        ro.append(ro[-1] + t)
    X = torch.cat(xs, 0)
    WT = torch.from_numpy(rs.standard_normal((ro[-1], H)).astype(np.float32)).to(dev)
    wts = [WT[a:b] for a, b in zip(ro[:-1], ro[1:])]

    def zero():
        for p in m.parameters():
            p.grad = None

    def batch_fwd():
        with torch.no_grad():
            m.forward_batch(X, ro)

    def seq_fwd():
        with torch.no_grad():
            for x in xs:
                m(x)

    def batch_fb():
        zero()
        tap, sc = m.forward_batch(X, ro)
        ((tap * WT).sum() + sc.sum()).backward()

    def seq_fb():
        zero()
        for x, w in zip(xs, wts):
            tap, sc = m(x)
            ((tap * w).sum() + sc.sum()).backward()
    r = dict(batch_fwd=timed(batch_fwd, iters), seq_fwd=timed(seq_fwd, iters), batch_fwd_bwd=timed(batch_fb, iters), seq_fwd_bwd=timed(seq_fb, iters))
    r['speedup_fwd'] = round(r['seq_fwd']['ms'] / r['batch_fwd']['ms'], 3)
    r['speedup_fwd_bwd'] = round(r['seq_fwd_bwd']['ms'] / r['batch_fwd_bwd']['ms'], 3)
    return r


def step_stamps(m, lengths, which):
    """Median per-step time of workgroup 0 (persist_stamps 3 = forward, 4 = reverse kernel of the first group), in microseconds."""
    lib = _lib.load()
    dev = torch.device('cuda')
    X = torch.randn(sum(lengths), D, device=dev)
    ro = [0]
    for t in lengths:
        ro.append(ro[-1] + t)
    lib.echr_config_set(b'persist_stamps', which)
    try:
        tap, sc = m.forward_batch(X, ro)
        if which == 4:
            (tap.sum() + sc.sum()).backward()
        torch.cuda.synchronize()
        buf = np.zeros(4 * 256 * 16, dtype=np.uint64)
        S = lib.echr_persist_read_stamps(buf.ctypes.data, buf.size)
        if S < 8:
            return None
    finally:
        lib.echr_config_set(b'persist_stamps', 0)
    st = buf[:S * 16].reshape(S, 16).astype(np.float64)[4:S - 4]
    tick = 0.01          # s_memrealtime counts at 100 MHz
    if which == 4 and len(lengths) > 1:
        # the batched reverse kernel runs its group as two half-groups per step: half B's rows travel while half A is multiplied
        seg = {'wait_a': st[:, 1] - st[:, 0], 'barrier': st[:, 2] - st[:, 1], 'half_a_products_cell_publish': st[:, 3] - st[:, 2],
               'half_b_wait_products_cell_publish': st[:, 4] - st[:, 3], 'step': np.diff(st[:, 0])}
    else:
        seg = {'wait': st[:, 1] - st[:, 0], 'barrier': st[:, 2] - st[:, 1], 'products': st[:, 3] - st[:, 2], 'cell_publish': st[:, 4] - st[:, 3],
               'step': np.diff(st[:, 0])}
    return {k: round(float(np.median(v)) * tick, 3) for k, v in seg.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', type=str, default='')
    ap.add_argument('--stamps', action='store_true', help='also record per-step stamps of workgroup 0 (V = 1 / 8, T = 256)')
    ap.add_argument('--cases', type=str, default='', help='comma-separated subset of V1,V4,V8,V16,mixed8 (default: all)')
    a = ap.parse_args(argv)
    lib = _lib.load()
    torch.manual_seed(0)
    m = models.setup_tap(synth.default_opt(video_dim=D, hidden_dim=H, K=K)).cuda()
    m.eval()          # timing only: no dropout (the mask costs one hash per element either way)
    cases = [('V1', [256]), ('V4', [256] * 4), ('V8', [256] * 8), ('V16', [256] * 16), ('mixed8', [32, 64, 96, 128, 160, 192, 224, 256])]
    if a.cases:
        cases = [c for c in cases if c[0] in a.cases.split(',')]
    res = dict(tool='sst_batch_bench', D=D, H=H, K=K, iters=a.iters, group=int(lib.echr_sst_batch_group()), device=torch.cuda.get_device_name(0))
    try:
        for persist, name in ((1, 'persistent'), (0, 'wavefront')):
            lib.echr_config_set(b'sst_persist', persist)
            res[name] = {c: bench_case(m, lengths, a.iters if persist else max(2, a.iters // 3)) for c, lengths in cases}
    finally:
        lib.echr_config_set(b'sst_persist', 1)
    if a.stamps:
        res['stamps_us'] = {'fwd_V1': step_stamps(m, [256], 3), 'fwd_V8': step_stamps(m, [256] * 8, 3), 'bwd_V1': step_stamps(m, [256], 4),
                            'bwd_V8': step_stamps(m, [256] * 8, 4)}
    res['check_async'] = int(lib.echr_check_async())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

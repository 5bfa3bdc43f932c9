#!/usr/bin/env python3
"""The data-parallel step over multi-video batches (fused.DataParallelBatchStep) against the plain batch step, on the GPU (one JSON line;
profiles/dp_batch_bench.json).  The shapes of tools/vbatch_bench.py, V = 4 / 16 videos per rank, at most two ranks:

  rccl1  ONE rank on RCCL (backend 'nccl', world size 1), cooperative persistent launches as bench.py's multi-rank runs use:
         (a) FusedTrainStep.batch(b) -- the iteration without a communicator, in the same process --  against
         (b) DataParallelBatchStep(f)(b): step=False with the hand-over callback, four collectives, one wait, clamp + Adam.
         A sum over one rank is the identity and crosses no wire: (b) - (a) is the host-path cost of the exchange, everything but the wire.
         The exposed wait (exchange_report: what the caller's stream waited for the collectives) comes from a pass of its own.
  gloo2  TWO ranks over gloo on one GPU (launch-per-phase recurrences: two persistent grids must not share a device), V videos per rank:
         the same two lines per rank, MAX over ranks.  A rehearsal of the two-rank host path, not a scaling figure: both ranks share the
         device and gloo stages every collective through the host.

Median-of-regions timing: a host clock around `reps` repetitions that end in a device synchronise, (a) and (b) alternating `rounds` times in
one process, min / median / max over the rounds.  No RCCL run with more than one rank exists for this project.

Usage: python tools/dp_batch_bench.py [--reps 30] [--rounds 5] [--out profiles/dp_batch_bench.json]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

VS = (4, 16)
WORKER_TIMEOUT = 420


def stats(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 4), median=round(xs[len(xs) // 2], 4), max=round(xs[-1], 4))


def worker(args):
    import torch
    import torch.distributed as dist
    import echr_amd
    import vbatch_bench as VB
    from echr_amd import _lib, synth
    from echr_amd.batch import VideoBatch
    from echr_amd.fused import DataParallelBatchStep, FusedTrainStep
    from echr_amd.optim import ClampAdam
    if not torch.cuda.is_available():
        raise SystemExit('dp_batch_bench needs the GPU: a timing taken anywhere else says nothing (no fallback)')
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    _lib.check(lib.echr_streams_init(), 'streams_init')          # the library's helper streams ahead of the communicator, as bench.py does
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(args.port)
    if args.worker == 'rccl1':
        fd = os.dup(1)
        os.dup2(2, 1)          # (RCCL prints its version banner to stdout)
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
        dist.barrier()
        os.dup2(fd, 1)
        os.close(fd)
        lib.echr_config_set(b'persist_coop', 1)
    else:
        dist.init_process_group('gloo', rank=args.rank, world_size=2)
        for key in (b'persist', b'persist_bwd'):
            lib.echr_config_set(key, 0)
    opt = synth.default_opt(vocab_size=VB.V1 - 1, seq_length=VB.L - 2)
    params = synth.make_params(opt, 0)
    cases = []
    for V in VS:
        vids = VB.videos(V, seed=4000 + 100 * args.rank)
        m = echr_amd.CaptionGenerator(opt)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        m = m.to(dev).train()
        o = ClampAdam(m.parameters(), lr=opt.lr, arena=m.build_arena())
        f = FusedTrainStep(m, o, grad_clip=opt.grad_clip)
        b = VideoBatch.from_videos(vids, device=dev)
        dp = DataParallelBatchStep(f)
        plain, wrapped = (lambda: f.batch(b)), (lambda: dp(b))
        for _ in range(args.warmup):
            plain()
            wrapped()
        ta, tb = [], []
        for _ in range(args.rounds):          # alternating, in one process; the ranks enter every region together
            dist.barrier()
            ta.append(VB.timed(plain, args.reps))
            dist.barrier()
            tb.append(VB.timed(wrapped, args.reps))
        # the exposed wait, in a pass of its own (its two events per step are not part of the timed regions)
        dp.measure = True
        for _ in range(args.reps):
            wrapped()
        torch.cuda.synchronize()
        dp.measure = False
        ex = dp.exchange_report()
        _lib.check(lib.echr_check_async(), 'dp_batch_bench')
        t = torch.tensor([stats(ta)['median'], stats(tb)['median'], ex['exposed_ms_median'] or 0.0], dtype=torch.float64)
        if args.worker == 'gloo2':
            dist.all_reduce(t, op=dist.ReduceOp.MAX)          # the job's figure: the slower rank
        cases.append(dict(V_per_rank=V, n_events_per_rank=b.n_events, S=b.S, batch_ms=stats(ta), dp_batch_ms=stats(tb),
                          batch_ms_median=round(float(t[0]), 4), dp_batch_ms_median=round(float(t[1]), 4),
                          overhead_ms=round(float(t[1] - t[0]), 4), overhead_ratio=round(float(t[1] / t[0]), 4),
                          exposed_wait_ms_median=round(float(t[2]), 4), exchange=ex))
        del dp, f, o, m
    with open(args.result, 'w') as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), cases=cases), fh)
    dist.destroy_process_group()


def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_leg(name, n_ranks, args, tmp):
    port = free_port()
    outs = [os.path.join(tmp, '%s_%d.json' % (name, r)) for r in range(n_ranks)]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', name, '--rank', str(r), '--port', str(port), '--result', outs[r],
                               '--reps', str(args.reps), '--rounds', str(args.rounds), '--warmup', str(args.warmup)], cwd=ROOT)
             for r in range(n_ranks)]
    try:
        for p in procs:
            if p.wait(timeout=WORKER_TIMEOUT) != 0:
                raise SystemExit('dp_batch_bench: a %s rank exited with %d' % (name, p.returncode))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    with open(outs[0]) as fh:
        return json.load(fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--legs', default='rccl1,gloo2')
    ap.add_argument('--worker', default=None)
    ap.add_argument('--rank', type=int, default=0)
    ap.add_argument('--port', type=int, default=0)
    ap.add_argument('--result', default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    res = dict(tool='dp_batch_bench', events_per_video=4, steps=20, V1=5001, reps=args.reps, rounds=args.rounds,
               note='one rank on RCCL crosses no wire; two ranks over gloo share one GPU: no RCCL run with more than one rank exists')
    with tempfile.TemporaryDirectory() as tmp:
        for leg, n in (('rccl1', 1), ('gloo2', 2)):          # one leg at a time: at most two GPU processes
            if leg in args.legs.split(','):
                out = run_leg(leg, n, args, tmp)
                res['device'] = out['device']
                res[leg] = out['cases']
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()

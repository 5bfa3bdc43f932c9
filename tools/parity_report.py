"""Actual parity errors of the HIP path against the reference-generated fixtures (tests/golden), per GEMM path (GPU box only).

--attsat: the attention-regime variants (synth.make_attsat) instead -- e_ref (float32 oracle vs float64 oracle, runs on the CPU) and, when a GPU is
present, the HIP path against the same float64 oracle beside it, persistent and launch-per-phase (the table of tests/test_gpu_attention_regime.py).

--tsrm: the event encoder's route cases (tests/tsrm_ref.py) -- e_ref per case as the lines of E_REF in tests/test_gpu_tsrm_routes.py and, when a GPU is
present, the HIP path's errors beside them.

--sst: the proposal encoder's trained-regime variants (tests/proposal_regime_ref.py) -- e_ref per variant, mode and one video / batch (the E_REF table
of tests/test_gpu_proposal_regime.py holds the largest of each column) and, when a GPU is present, the HIP path against the same float64 oracle beside
it, persistent and wavefront.

--decsat: the decoder recurrences' trained-regime variants (synth.make_decsat, tests/decoder_regime_ref.py) -- e_ref per variant and mode (log-probs,
loss, worst gradient tensor, worst LSTM gate slice; the E_REF table of tests/test_gpu_decoder_regime.py holds the larger of eval and train) and, when a
GPU is present, the HIP path against the same float64 oracle beside it per route: persistent on fp16 pairs, persistent in exact fp32,
launch-per-phase (70 events: the launch form alone; the batch: forward_batch).

--sat: the one-stream decoder's cases (synth.SAT_CASES, tests/sat_ref.py) -- e_ref per variant and mode and, when a GPU is present, the HIP path
against the same float64 run beside it.

--widths: the decoder-width cases (tests/width_ref.py) -- e_ref per case (log-probs, loss, worst gradient tensor, worst slice of the varied axis),
what the two mutants move, and, when a GPU is present, the HIP path against the same float64 oracle beside it."""
import sys, os; sys.path.insert(0, os.environ.get('GRAFT_REPO_ROOT', '/root/repo')); sys.path.insert(0, os.path.join(os.environ.get('GRAFT_REPO_ROOT', '/root/repo'), 'tests'))
import numpy as np, torch
import util as U
from echr_amd import synth, _lib
from oracle import summary as SM


def _errs(pred, loss, grads, ref):
    rp, rl, rg = ref
    worst = max((U.relerr(grads[k], g, U.GRAD_FLOOR), k) for k, g in rg.items() if g is not None and k not in U.NOISE_ONLY)
    return float(np.abs(pred - rp).max()), abs(loss - rl) / abs(rl), worst[0], worst[1]


def attsat_report():
    gpu = torch.cuda.is_available()
    lib = _lib.load() if gpu else None
    for name in synth.ATTSAT:
        if name == 'pq_cross' and gpu:
            print(name, 'outside the domain of the factored tanh: reported as -EDOM, see test_pq_cross_is_reported_not_hidden')
            continue
        opt, params, vid = synth.make_attsat(name)
        for train in (False, True):
            ref = U.run_oracle(opt, params, vid, train, dtype=torch.float64)
            e = _errs(*U.run_oracle(opt, params, vid, train), ref)
            line = '%-12s %s  e_ref: logp %.1e loss %.1e grad %.1e' % (name, 'train' if train else 'eval ', e[0], e[1], e[2])
            for persist in ((1, 0) if gpu else ()):
                lib.echr_config_set(b'persist', persist); lib.echr_config_set(b'persist_bwd', persist)
                try:
                    h = _errs(*U.run_gpu(opt, params, vid, train)[:3], ref)
                finally:
                    lib.echr_config_set(b'persist', 1); lib.echr_config_set(b'persist_bwd', 1)
                line += ' | HIP %s: logp %.1e loss %.1e grad %.1e' % ('persistent' if persist else 'launch', h[0], h[1], h[2])
            print(line, flush=True)


def tsrm_report():
    """e_ref of every case of tests/tsrm_ref.py (the E_REF table of tests/test_gpu_tsrm_routes.py) and, when a GPU is present, the HIP path against
    the same float64 oracle beside it."""
    from tests import tsrm_ref as R
    gpu = torch.cuda.is_available()
    if gpu:
        from tests import test_gpu_tsrm_routes as T
    for name, spec in R.CASES.items():
        e = R.e_ref(spec)
        line = "    %r: (%.1e, %.1e, %.1e),%s# %s" % (name, e[0], e[1], e[3], ' ' * max(1, 30 - len(name)), e[2].replace(R.PREFIX, ''))
        if gpu:
            b = R.bounds(R.case_inputs(spec)[2]) if spec['inference'] else (0, 0)
            h = T.errors(spec, T.gpu_run(spec, bounds=b), R.reference(spec))
            line += ' | HIP: out %.1e grad %.1e (%s) noise %.1e' % (h[0], h[1], h[2].replace(R.PREFIX, ''), h[3])
        print(line, flush=True)


def sst_report():
    from tests import proposal_regime_ref as P
    gpu = torch.cuda.is_available()
    if gpu:
        from tests import test_gpu_proposal_regime as T
    fmt = 'tap %.1e scores %.1e loss %.1e grad %.1e (%s)'
    for name in P.VARIANTS:
        for batch in (False, True):
            for train in (False, True):
                line = '%-10s %s %s  e_ref: ' % (name, 'batch' if batch else 'video', 'train' if train else 'eval ') + fmt % P.e_ref(name, train, batch)
                for persist in ((1, 0) if gpu and P.VARIANTS[name]['H'] == 512 else (0,) if gpu else ()):
                    line += ' | HIP %s: ' % ('persistent' if persist else 'wavefront') + fmt % P.errors(T._route(name, train, batch, persist), P.oracle64(name, train, batch))
                print(line, flush=True)


def decsat_report():
    from tests import decoder_regime_ref as D
    gpu = torch.cuda.is_available()
    if gpu:
        from tests import test_gpu_decoder_regime as T
    fmt = 'logp %.1e loss %.1e grad %.1e slice %.1e'
    pick = lambda e: (e[0], e[1], e[2], e[4])
    for name in synth.DECSAT:
        for train in (False, True):
            line = '%-14s %s  e_ref: ' % (name, 'train' if train else 'eval ') + fmt % pick(D.e_ref(name, train))
            if gpu:
                ref = D.oracle(name, train)
                if name == 'gates_sat_vb':
                    runs = [('forward_batch', T.batch_module_pass(train))]
                else:
                    runs = [(r, T._module_pass(name, train, r)) for r in (T.ROUTES if name in T.PERSISTENT else ('launch',))]
                for route, got in runs:
                    line += ' | HIP %s: ' % route + fmt % pick(D.errors(got, ref))
            print(line, flush=True)
    line = 'drift, one step from the state of largest |c|  e_ref: logp %.1e h %.1e c %.1e' % D.drift_step_e_ref()
    if gpu:
        line += ' | HIP: logp %.1e h %.1e c %.1e' % tuple(T.drift_step_errors())
    print(line, flush=True)


def sat_report():
    """The one-stream decoder (synth.SAT_CASES, tests/sat_ref.py): e_ref per variant and mode (log-probs and loss relative, worst gradient tensor
    and d tap_feats of their max-norms) and, when a GPU is present, the HIP path against the same float64 run beside it (the gates of
    tests/test_gpu_sat.py are ten times the largest of those columns)."""
    from tests import sat_ref as R
    gpu = torch.cuda.is_available()
    if gpu:
        from tests import test_gpu_sat as T

    def errs(got, ref):
        worst = max((U.relerr(got[2][k], g, U.GRAD_FLOOR), k) for k, g in ref[2].items() if g is not None and k not in R.NOISE_ONLY)
        return U.relerr(got[0], ref[0]), abs(got[1] - ref[1]) / abs(ref[1]), worst[0], U.relerr(got[3], ref[3], U.GRAD_FLOOR), worst[1]
    fmt = 'logp %.1e loss %.1e grad %.1e d tap %.1e (%s)'
    for name in synth.SAT_CASES:
        opt, params, vid = synth.make_sat_case(name)
        for train in (False, True):
            ref = R.run(opt, params, vid, train, dtype=torch.float64)
            line = '%-13s %s  e_ref: ' % (name, 'train' if train else 'eval ') + fmt % errs(R.run(opt, params, vid, train), ref)
            if gpu:
                line += ' | HIP: ' + fmt % errs(T._run(opt, params, vid, train), ref)
            print(line, flush=True)


def widths_report():
    """The decoder-width cases (tests/width_ref.py): e_ref per case in train mode (log-probs, loss, worst gradient tensor, worst width slice --
    the table in the docstring of tests/test_gpu_decoder_widths.py and E_REF of tests/width_ref.py), the movement of the two mutants, and, when
    a GPU is present, the HIP path against the same float64 oracle beside it on the default route."""
    from tests import width_ref as W
    gpu = torch.cuda.is_available()
    if gpu:
        from tests import test_gpu_decoder_widths as T
    fmt = 'logp %.1e loss %.1e grad %.1e slice %.1e'
    pick = lambda e: (e[0], e[1], e[2], e[4])
    for name, c in W.CASES.items():
        e = W.e_ref(name)
        line = '%-20s R %d RD %d  e_ref: ' % ((name,) + W.dispatch(c)) + fmt % pick(e) + ' (%s)' % e[5].replace('lm_model.core.', '')
        if name in W.MUTATED:
            opt, ref = W.case(name)[0], W.oracle(name)
            for which in ('alpha', 'c3d'):
                m = W.errors(W.mutant(name, which), ref, opt)
                line += ' | %s: logp %.1e grad %.1e' % (which, m[0], m[2])
        if gpu:
            line += ' | HIP: ' + fmt % pick(W.errors(T.module_pass(name, ()), W.oracle(name), W.case(name)[0]))
        print(line, flush=True)


if '--widths' in sys.argv:
    widths_report()
    sys.exit(0)
if '--sat' in sys.argv:
    sat_report()
    sys.exit(0)
if '--decsat' in sys.argv:
    decsat_report()
    sys.exit(0)
if '--sst' in sys.argv:
    sst_report()
    sys.exit(0)
if '--tsrm' in sys.argv:
    tsrm_report()
    sys.exit(0)
if '--attsat' in sys.argv:
    attsat_report()
    sys.exit(0)
lib = _lib.load()
for case in ('c2full', 'c1'):
    opt, params, vid = synth.make_case(case)
    g = U.gold('case_%s.npz' % case)
    for h2 in (1, 0):
        lib.echr_config_set(b'gemm_h2', h2)
        pred, loss, grads, _ = U.run_gpu(opt, params, vid, False)
        s = SM.summarize_logp(pred)
        gs = SM.summarize_grads(grads)
        worst = 0.0; wk = ''
        for key, v in gs.items():
            name = key.split('|')[0]
            if name in U.NOISE_ONLY or key.endswith('|l2') or key.endswith('|linf'): continue
            scale = max(float(g['eval|grad|' + name + '|linf']), 1e-30)
            e = float(np.abs(v - g['eval|grad|' + key]).max() / scale)
            if e > worst: worst, wk = e, key
        print(case, 'h2' if h2 else 'bf16x3', 'max|dlogp| %.2e' % np.abs(s['slice'] - g['eval|logp|slice']).max(), 'dloss rel %.2e' % abs(loss / float(g['eval|loss']) - 1), 'worst grad slice rel-to-linf %.2e (%s)' % (worst, wk))
lib.echr_config_set(b'gemm_h2', 1)

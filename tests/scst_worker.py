"""Child process of tests/test_gpu_scst.py: three back-to-back SelfCriticalStep iterations in deterministic mode on the 'c1' case;
writes the parameter arena and the Adam moments to the .npz named on the command line (ECHR_STAGE_AHEAD comes from the environment)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import echr_amd                                          # noqa: E402
from echr_amd import synth                               # noqa: E402
from echr_amd.fused import FusedTrainStep, SelfCriticalStep          # noqa: E402
from echr_amd.optim import ClampAdam                     # noqa: E402
from tests import util as U                              # noqa: E402


def reward_fn(gen, greedy):
    # a fixed host reward: longer sampled captions than the baseline are rewarded, per caption
    lg, lb = (gen > 0).sum(1).float(), (greedy > 0).sum(1).float() if greedy.numel() else torch.zeros(gen.shape[0])
    return (lg - lb) / 4.0 - 0.1


def main(out):
    echr_amd.set_deterministic(True)
    opt, params, vid = synth.make_case('c1')
    m = U.build_gpu_model(opt, params, True)
    o = ClampAdam(m.parameters(), lr=1e-3, arena=m.build_arena())
    sc = SelfCriticalStep(FusedTrainStep(m, o, grad_clip=0.1), reward_fn)
    tap, c3d, lda = (torch.from_numpy(vid[k]).cuda() for k in ('tap', 'c3d', 'lda'))
    losses, gens = [], []
    for _ in range(3):
        loss, gen, greedy, _r = sc(tap, c3d, lda, vid['ind'], vid['soi'])
        losses.append(float(loss))
        gens.append(gen.numpy().ravel())
    torch.cuda.synchronize()
    st = o._flat
    np.savez(out, p=o.arena.flat_p.cpu().numpy(), m=st['m'].cpu().numpy(), v=st['v'].cpu().numpy(), loss=np.array(losses, dtype=np.float32),
             gen=np.concatenate(gens), step=np.int64(st['step']))


if __name__ == '__main__':
    main(sys.argv[1])

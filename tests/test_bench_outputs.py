"""CPU: what `bench.py --dump-outputs` writes -- float32 arrays named after the loss and the parameters, the same ones on every call,
within the size limit of the option."""
import os
import types

import numpy as np
import torch

import bench
import echr_amd


def _workload(kind):
    opt, params, _ = bench.make_workload(0, False)
    model = echr_amd.CaptionGenerator(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return types.SimpleNamespace(kind=kind, model=model)


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_names_sizes_and_repeatability(tmp_path):
    wl = _workload('train')
    n = bench.dump_outputs(wl, torch.tensor(2.5), str(tmp_path / 'a'))
    bench.dump_outputs(wl, torch.tensor(2.5), str(tmp_path / 'b'))
    a, b = _read(str(tmp_path / 'a')), _read(str(tmp_path / 'b'))
    params = dict(wl.model.named_parameters())
    assert set(a) == {'loss'} | {'param.' + k for k in params if k not in bench.DUMP_SKIP}
    assert all(v.dtype == np.float32 for v in a.values())
    assert n == sum(v.nbytes for v in a.values()) <= bench.DUMP_MAX_BYTES
    assert float(a['loss']) == 2.5
    for k, v in a.items():
        assert np.array_equal(v, b[k]), k                  # the same sample every time
        if k == 'loss':
            continue
        p = params[k[len('param.'):]].detach().reshape(-1).numpy()
        if p.size <= bench.DUMP_MAX_ELEMS:
            assert np.array_equal(v, p), k                 # small tensors whole
        else:
            assert v.size == bench.DUMP_MAX_ELEMS and np.isin(v, p).all(), k


def test_dump_outputs_keeps_the_total_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 4 << 20)
    n = bench.dump_outputs(_workload('train'), torch.tensor(1.0), str(tmp_path))
    assert n == sum(v.nbytes for v in _read(str(tmp_path)).values()) <= 4 << 20


def test_dump_outputs_forward_only_is_the_loss(tmp_path):
    bench.dump_outputs(_workload('fwd'), torch.tensor(3.0), str(tmp_path))
    assert sorted(os.listdir(str(tmp_path))) == ['loss.npy']

"""The decoder backward passes of tests/decoder_bwd_runs.py equal the record made BEFORE echr::decoder_bwd_parts was cut into stages over one
plan (tests/golden/decoder_bwd.json, tools/make_golden_decoder_bwd.py; a second process at that commit reproduced the record).

Bits: deterministic mode, a fixed dropout seed -- no kernel and no launch order differs, so any difference is a behaviour change: no
tolerance.  Launch counts: deterministic mode never takes the persistent reverse launch or the replica form of att_post, so the same runs
are repeated with it off and the library's profile on, and the `launches` figure of every profile kind is compared as an integer.  No run
is left out of the launch record."""
import functools
import json
import os

import pytest

from tests import decoder_bwd_runs as D
from tests import util as U

ZERO_F32 = '00000000'


@functools.lru_cache(maxsize=None)
def _record():
    with open(os.path.join(U.GOLD, 'decoder_bwd.json')) as f:
        return json.load(f)


def test_the_record_covers_every_run_and_none_of_it_is_zeros():
    """Needs no GPU: the record names exactly RUNS; no loss is zero; every hash comes with the number of floats behind it and is not the
    hash of that many zeros; the hashes of a run differ."""
    import hashlib
    rec = _record()
    assert sorted(rec) == sorted(D.RUNS)
    for name, r in rec.items():
        bits = r['bits']
        assert set(bits) >= {'loss', 'grads', 'floats'}, name
        assert len(bits['loss']) % 8 == 0 and ZERO_F32 not in [bits['loss'][i:i + 8] for i in range(0, len(bits['loss']), 8)], name
        hashed = {k for k, v in bits.items() if isinstance(v, str) and len(v) == 64 and k != 'loss'}
        assert hashed == set(bits['floats']) and len({bits[k] for k in hashed}) == len(hashed), name
        for k, n in bits['floats'].items():
            assert n > 0 and bits[k] != hashlib.sha256(bytes(4 * n)).hexdigest(), (name, k)
        assert r['launches'] is not None and len(r['launches']) == D.PROF_KINDS and sum(r['launches']) > 0, name


@pytest.mark.gpu
@pytest.mark.parametrize('name', D.RUNS)
def test_run_is_bitwise_the_recorded_one(name):
    import echr_amd
    echr_amd.set_deterministic(True)
    try:
        got = D.run(name)
    finally:
        echr_amd.set_deterministic(False)
    want = _record()[name]['bits']
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize('name', D.RUNS)
def test_run_launches_what_the_recorded_one_launched(name):
    assert D.launches(name) == _record()[name]['launches'], name

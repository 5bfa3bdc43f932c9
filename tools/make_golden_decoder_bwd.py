#!/usr/bin/env python3
"""Record tests/golden/decoder_bwd.json: the decoder backward passes of tests/decoder_bwd_runs.py on the GPU -- their bits in
deterministic mode, and their launch counts per profile kind with deterministic mode off.  Run it at the commit whose behaviour is to be
pinned, twice (a second process must reproduce the first before the record is trusted).  A run whose profiled form fails is recorded with
launches = null and the error beside it.

Usage:  python tools/make_golden_decoder_bwd.py [OUT.json]          (default: tests/golden/decoder_bwd.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import echr_amd                                  # noqa: E402
from tests import decoder_bwd_runs as D          # noqa: E402

if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'decoder_bwd.json')
    rec = {}
    echr_amd.set_deterministic(True)
    try:
        for name in D.RUNS:
            rec[name] = dict(bits=D.run(name))
            print(name, rec[name]['bits'], flush=True)
    finally:
        echr_amd.set_deterministic(False)
    for name in D.RUNS:
        try:
            rec[name]['launches'] = D.launches(name)
        except Exception as e:          # noqa: BLE001
            rec[name]['launches'], rec[name]['launches_error'] = None, '%s: %s' % (type(e).__name__, e)
        print(name, rec[name]['launches'], flush=True)
    with open(out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', out)

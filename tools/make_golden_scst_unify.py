#!/usr/bin/env python3
"""Record tests/golden/scst_unify.json: the six self-critical runs of tests/scst_unify_runs.py on the GPU, bit for bit.  Run it at the
commit whose behaviour is to be pinned, twice (a second process must reproduce the first before the record is trusted):

Usage:  python tools/make_golden_scst_unify.py [OUT.json]          (default: tests/golden/scst_unify.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import scst_unify_runs as S          # noqa: E402

if __name__ == '__main__':
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'scst_unify.json')
    with open(out, 'w') as f:
        json.dump(S.run_all(), f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', out)

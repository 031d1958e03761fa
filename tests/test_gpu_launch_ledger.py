"""The launch ledger recorded at the parent of the executor refactoring (tools/make_launch_ledger.py, tests/golden/
launch_ledger_parent.json) replayed on the code under test: every leg must produce the same output bits through the same kernels,
launched as often, executing the same FLOP and moving the same bytes.  The bit-identity tests of test_gpu_denoise.py compare a
windowed against an unwindowed run of one build, so a launch window that grew would pass them; here it moves the FLOP and bytes.

Digests, names and counts are compared exactly.  FLOP and bytes within 1e-9 relative: both are double-precision sums of at most
tens of thousands of positive products, which regrouping the arithmetic moves by far less than 1e-12, while the smallest real
change -- one row of a window of fewer than 1000 rows -- moves them by more than 1e-3."""
import json
import os

import pytest

from conftest import GOLDEN
from tools import make_launch_ledger as ml

pytestmark = pytest.mark.gpu
RTOL = 1e-9


@pytest.fixture(scope='module')
def ledger():
    with open(os.path.join(GOLDEN, 'launch_ledger_parent.json')) as f:
        return json.load(f)


def _close(a, b):
    return abs(a - b) <= RTOL * max(abs(a), abs(b))


@pytest.mark.parametrize('leg', sorted(ml.LEGS))
def test_leg_matches_the_parent_ledger(gpu_ctx, ledger, leg):
    assert ledger['fold_model'] == ml.FOLD_MODEL
    assert leg in ledger['legs'], f'the ledger file lacks leg {leg}'
    want = ledger['legs'][leg]
    assert list(want) == sorted(ml.RUNS[leg]), f'the ledger file lacks a run of leg {leg}'
    got = ml.record(gpu_ctx, [leg])[leg]
    assert sorted(got) == sorted(want)
    for tag in ml.RUNS[leg]:
        g, w = got[tag], want[tag]
        print(f'{leg}/{tag}: {g["launches"]} launches, {sum(c[1] for c in g["classes"]) / 1e9:.3f} GFLOP '
              f'(parent {w["launches"]}, {sum(c[1] for c in w["classes"]) / 1e9:.3f}), {len(g["kernels"])} kernels')
        assert g['shape'] == w['shape'] and g['digest'] == w['digest'], (leg, tag)
        assert g['launches'] == w['launches'], (leg, tag)
        assert g.get('stats') == w.get('stats'), (leg, tag)
        for c, (gc, wc) in enumerate(zip(g['classes'], w['classes'])):
            assert gc[0] == wc[0] and _close(gc[1], wc[1]), (leg, tag, c, gc, wc)
        assert [k[:2] for k in g['kernels']] == [k[:2] for k in w['kernels']], (leg, tag)
        for gk, wk in zip(g['kernels'], w['kernels']):
            assert _close(gk[2], wk[2]) and _close(gk[3], wk[3]), (leg, tag, gk, wk)

"""GPU: the seven stream wrappers give, bit for bit, what the commit before tcow_attn_temporal_step / tcow_cls_step gave through its eleven entry points:
tests/golden/stream_attn_bits.json was recorded on the MI355X from that commit's package and libraries (tools/make_stream_attn_bits.py) and is not
regenerated.  Cases and inputs: tests/stream_attn_bits.py."""
import json
import os

import pytest

import stream_attn_bits as kit

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stream_attn_bits.json')
GEOMETRIES = ['stream', 'pool', 'ragged', 'paged-P2', 'paged-P8', 'paged-T70-P1', 'bad-stream-t0', 'bad-pool-slot', 'bad-ragged-t0', 'bad-paged-page']
CLS = ['cls-stream-t0=0', 'cls-stream-t0=35', 'cls-pool', 'cls-ragged', 'cls-bad-slot']

@pytest.fixture(scope='module')
def parent_bits():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(parent_bits):
    assert sorted(parent_bits) == sorted([f'{pair}/{g}' for pair in kit.PAIRS for g in GEOMETRIES] + CLS)
    assert len(kit.PAIRS) == 8


@pytest.mark.gpu
@pytest.mark.parametrize('pair', list(kit.PAIRS))
def test_attention_gives_the_parent_commits_bits(cuda, pair, parent_bits):
    got = kit.attention_cases(pair)
    assert sorted(got) == sorted(GEOMETRIES)
    for case, hashes in got.items():
        assert hashes == parent_bits[f'{pair}/{case}'], (pair, case, [t for t in hashes if hashes[t] != parent_bits[f'{pair}/{case}'][t]])
    # the cases are different computations, and a bad row leaves the caches as the inputs were: the hashes tell (same seeds, same caches)
    assert len({h['out'] for h in got.values()}) == len(got)
    assert got['bad-stream-t0']['k_cache'] != got['stream']['k_cache'] and got['bad-paged-page']['k_cache'] != got['paged-P8']['k_cache']


@pytest.mark.gpu
def test_cls_gives_the_parent_commits_bits(cuda, parent_bits):
    got = kit.cls_cases()
    assert sorted(got) == sorted(CLS)
    for case, hashes in got.items():
        assert hashes == parent_bits[case], (case, hashes, parent_bits[case])
    assert got['cls-stream-t0=0']['cls_cache'] != got['cls-stream-t0=35']['cls_cache']      # t0 == 0 keeps the row, t0 > 0 reads it

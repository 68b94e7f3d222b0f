"""GPU: ops.attn_fwd / ops.attn_bwd in mode F32X3 give, bit for bit (a -0 counting as +0), what the commit before the x3 kernels were rewritten on
attention_tiles.h's helpers and forward tile step gave: tests/golden/attn_x3_bits.json was recorded on the MI355X from that commit's package and libraries
(tools/make_attn_x3_bits.py) and is not regenerated.  Cases and inputs: tests/attn_x3_bits.py."""
import json
import os

import pytest

import attn_x3_bits as kit

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'attn_x3_bits.json')


@pytest.fixture(scope='module')
def parent_bits():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(parent_bits):
    assert sorted(parent_bits) == sorted(kit.CASES)
    assert len(kit.CASES) == 8
    for name, hashes in parent_bits.items():
        assert sorted(hashes) == sorted(kit.TENSORS), name
        assert all(len(h) == 64 for h in hashes.values()), name


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(kit.CASES))
def test_x3_attention_gives_the_parent_commits_bits(cuda, name, parent_bits):
    got = kit.case(name)
    assert got == parent_bits[name], (name, [t for t in got if got[t] != parent_bits[name][t]])

"""CPU: the host side of SeekerStreamPool.step_ragged (tcow_amd/stream.py) -- the table builder against a brute-force restatement, the
argument refusals that look at the lists alone, and the ABI entries."""
import pytest
import torch

import stream_abi as abi
from stream_kit import _net
from tcow_amd import _lib, stream
from tcow_amd._lib import TcowError


def _brute(t0s, slots, cs):
    """Every flat frame on its own: walk the sessions, count frames."""
    n = len(cs)
    flat = [(r, j) for r in range(n) for j in range(cs[r])]                     # flat frame f -> (session, frame of its chunk)
    first = [min(f for f, (r, _) in enumerate(flat) if r == q) for q in range(n)]
    return {'t0': list(t0s), 'slot': list(slots), 'first': first, 'c': list(cs), 'row_of_frame': [r for r, _ in flat],
            'frames': [t0s[r] + j for r, j in flat]}


@pytest.mark.parametrize('t0s,slots,cs', [
    ([0], [0], [1]),
    ([7], [3], [1]),
    ([0], [2], [5]),
    ([0, 5, 2], [2, 0, 1], [1, 3, 2]),
    ([26, 0, 29, 3], [1, 3, 0, 2], [4, 1, 1, 9]),
    ([0, 4, 8, 12, 17, 21, 25, 22], [7, 6, 5, 4, 3, 2, 1, 0], [1, 1, 1, 1, 2, 2, 4, 8]),
    ([3, 3, 3], [0, 1, 2], [2, 2, 2]),
])
def test_ragged_tables_vs_brute_force(t0s, slots, cs):
    got = stream.ragged_tables(t0s, slots, cs)
    assert got == _brute(t0s, slots, cs)
    F = sum(cs)
    assert len(got['row_of_frame']) == F and len(got['frames']) == F
    for f in range(F):                                                          # the kernel's reading of the tables: j = f - first inside [0, c), t = t0 + j
        r = got['row_of_frame'][f]
        j = f - got['first'][r]
        assert 0 <= j < got['c'][r] and got['frames'][f] == got['t0'][r] + j
    assert all(type(v) is int for k in got for v in got[k])


def test_ragged_tables_refuse_bad_lists():
    with pytest.raises(TcowError, match='chunk lengths'):
        stream.ragged_tables([0, 1], [0, 1], [1, 0])
    with pytest.raises(TcowError, match='per session'):
        stream.ragged_tables([0, 1], [0], [1, 1])
    with pytest.raises(TcowError, match='per session'):
        stream.ragged_tables([], [], [])


def test_step_ragged_list_refusals():
    open_ids = {3: 0, 5: 1, 6: 2}                               # session id -> slot, as the pool keeps it
    chk = lambda *a: stream.check_sessions('stream_pool.step_ragged', *a)
    assert chk((5, 3), 2, None, 4, open_ids) == [5, 3] and chk([6], 1, 1, 4, open_ids) == [6]
    with pytest.raises(TcowError, match='1 .. capacity'):
        chk([], 0, None, 4, open_ids)
    with pytest.raises(TcowError, match='1 .. capacity'):
        chk([3, 5, 6], 3, None, 2, open_ids)
    with pytest.raises(TcowError, match='lengths must agree'):
        chk([3, 5], 1, None, 4, open_ids)
    with pytest.raises(TcowError, match='lengths must agree'):
        chk([3, 5], 2, 3, 4, open_ids)
    with pytest.raises(TcowError, match='not open'):
        chk([3, 4], 2, None, 4, open_ids)
    with pytest.raises(TcowError, match='duplicate'):
        chk([3, 5, 3], 3, 3, 4, open_ids)


def test_step_ragged_range_refusal_names_the_session():
    stream.check_range('stream_pool.step_ragged', [3, 5], [0, 26], [30, 4], 30)                     # both end exactly at the last frame
    with pytest.raises(TcowError, match='session 5: frames 27..30'):
        stream.check_range('stream_pool.step_ragged', [3, 5], [0, 27], [1, 4], 30)
    with pytest.raises(TcowError, match='session 9'):                            # the offender is the last of the list
        stream.check_range('stream_pool.step_ragged', [3, 5, 9], [0, 1, 30], [1, 1, 1], 30)


def test_step_ragged_input_refusals():
    m = _net(1).eval().seeker
    dev = torch.device('cpu')
    ok = torch.zeros(1, 3, 2, 32, 48)
    who = 'stream_pool.step_ragged: session 7'
    for bad in (torch.zeros(2, 3, 2, 32, 48), torch.zeros(1, 4, 2, 32, 48), torch.zeros(1, 3, 0, 32, 48), torch.zeros(1, 3, 2, 32, 40), torch.zeros(3, 2, 32, 48), None):
        with pytest.raises(TcowError, match='session 7: rgb'):
            stream._check_inputs(who, m, dev, 1, 1, bad, None)
    for bad in (torch.zeros(1, 1, 3, 32, 48), torch.zeros(2, 1, 2, 32, 48), 'x'):
        with pytest.raises(TcowError, match='session 7: query_mask'):
            stream._check_inputs(who, m, dev, 1, 1, ok, bad)
    with pytest.raises(TcowError, match='device'):                              # (a CPU tensor is on no stream device)
        stream._check_inputs(who, m, dev, 1, 1, ok, torch.zeros(1, 1, 2, 32, 48))


def test_ragged_abi_entries():
    """A ragged step is a form of the two step records (n_sessions >= 1; first_rows / c_rows given), not an entry point."""
    assert _lib.ABI_VERSION >= 13
    abi.check_header_and_records()
    for name in abi.RECORDS:
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name) and hasattr(_lib.lib('fp16'), name)
    abi.check_old_symbols_are_gone(['tcow_attn_temporal_ragged_fwd', 'tcow_attn_temporal_ragged_cq_fwd', 'tcow_cls_stream', 'tcow_cls_pool', 'tcow_cls_ragged'])

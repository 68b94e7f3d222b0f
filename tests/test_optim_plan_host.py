"""CPU: tcow_amd/optim_plan.py -- chunk rows, flat rows, tile records, the table key and the step base -- against tables worked out by hand."""
import numpy as np

from tcow_amd import optim_plan as plan

P, G, M, V = 0x10000000, 0x20000000, 0x30000000, 0x40000000           # far apart: a swapped column shows


def _tensor(k, n):
    """Addresses of the k-th tensor of n elements: 16 MiB apart within each array."""
    return (P + (k << 24), G + (k << 24), M + (k << 24), V + (k << 24), n)


def test_record_sizes_are_those_of_the_kernel_structs():
    assert (plan.CHUNK, plan.CHUNK_BYTES, plan.TILE_BYTES, plan.TILE) == (65536, 5 * 8, 7 * 8, 64)


def test_chunk_rows_of_the_edge_sizes():
    sizes = [1, 3, 4, 7, 65536, 65537, 15]
    rows, owner = plan.chunk_rows([_tensor(k, n) for k, n in enumerate(sizes)])
    assert rows.dtype == np.int64 and rows.shape == (8, 5) and owner.tolist() == [0, 1, 2, 3, 4, 5, 5, 6]
    assert rows[:, 4].tolist() == [1, 3, 4, 7, 65536, 65536, 1, 15]                 # one vector plus a tail ... two chunks, the second of one element
    for r, k in zip(rows.tolist(), owner.tolist()):
        off = 4 * 65536 if r == rows[6].tolist() else 0
        assert r[:4] == [a + off for a in _tensor(k, 0)[:4]]
    assert plan.chunk_rows([])[0].shape == (0, 5)


def test_three_chunks_advance_every_column_alike():
    rows, owner = plan.chunk_rows([_tensor(0, 2 * 65536 + 5)])
    assert rows.tolist() == [[P, G, M, V, 65536], [P + 262144, G + 262144, M + 262144, V + 262144, 65536], [P + 524288, G + 524288, M + 524288, V + 524288, 5]]


def test_flat_rows_leave_out_the_tiled_tensors():
    rows, owner = plan.chunk_rows([_tensor(0, 7), _tensor(1, 65537), _tensor(2, 4), _tensor(3, 128 * 192)])
    assert plan.flat_rows(rows, owner, []) is rows                                  # nothing tiled: the chunk table itself
    flat = plan.flat_rows(rows, owner, [1, 3])
    assert flat.tolist() == [rows[0].tolist(), rows[3].tolist()] and flat.dtype == np.int64
    assert plan.flat_rows(rows, owner, [0, 1, 2, 3]).shape == (0, 5)


def test_tile_records_of_a_128_by_192_weight():
    """N = 128, K = 192: two tile rows of three tiles.  K != N: strides that were swapped between W and W^T would show."""
    WC, WT = 0x50000000, 0x60000000
    r = plan.tile_records(P, G, M, V, WC, WT, 128, 192)
    assert r.dtype == np.int64 and r.shape == (6, 7)
    origins = [(0, 0), (0, 64), (0, 128), (64, 0), (64, 64), (64, 128)]             # (n0, k0), row by row
    for rec, (n0, k0) in zip(r.tolist(), origins):
        o, ot = n0 * 192 + k0, k0 * 128 + n0                                       # element offsets in [N, K] and in [K, N]
        assert rec[:4] == [P + 4 * o, G + 4 * o, M + 4 * o, V + 4 * o]
        assert rec[4:6] == [WC + 2 * o, WT + 2 * ot]
        assert (rec[6] & 0xffffffff, rec[6] >> 32) == (192, 128)                   # CastTile {..., int K, N}: K in the low half
    assert r[4].tolist() == [P + 49408, G + 49408, M + 49408, V + 49408, WC + 24704, WT + 16512, 192 | (128 << 32)]      # (64 * 192 + 64) * 4, * 2; (64 * 128 + 64) * 2
    assert np.frombuffer(r[0].tobytes(), dtype=np.int32)[12:].tolist() == [192, 128]


def test_tile_records_of_one_tile():
    assert plan.tile_records(P, G, M, V, 8, 16, 64, 64).tolist() == [[P, G, M, V, 8, 16, 64 | (64 << 32)]]


def test_tables_are_current_for_the_same_key_and_generation():
    key = plan.table_key([11, 12], [G, G + 64], [M, M + 64])
    assert key == ((11, G, M), (12, G + 64, M + 64))
    assert plan.tables_current(key, 3, key, 3, True) and plan.tables_current(key, None, key, None, False)
    assert plan.tables_current(key, 4, key, 3, False) and not plan.tables_current(key, 4, key, 3, True)        # the generation counts with fuse_cast only
    assert not plan.tables_current(key, 3, None, None, True)                                                   # nothing built yet
    for moved in (plan.table_key([11, 13], [G, G + 64], [M, M + 64]), plan.table_key([11, 12], [G, G + 128], [M, M + 64]),
                  plan.table_key([11, 12], [G, G + 64], [M, 0]), key[:1]):
        assert not plan.tables_current(moved, 3, key, 3, False)


def test_step_base_is_the_largest_count():
    assert plan.step_base([0]) == 0 and plan.step_base([0, 7, 3]) == 7 and plan.step_base(iter([2, 2])) == 2

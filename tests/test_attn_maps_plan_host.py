"""CPU: the host arithmetic of Seeker.attention_maps (tcow_amd/attn_maps.py): argument normalisation, the (frame, slot) -> sequence position
maps of the divided and the joint type, every refusal with its message, and the shapes and bytes at BASELINE configs[1]."""
import pytest

from conftest import load_golden
from tcow_amd._lib import TcowError
from tcow_amd import attn_maps as am

C1 = dict(depth=12, B=1, T=30, S=301, heads=12, causal=1, joint=False)          # BASELINE configs[1], one query row


def plan(**kw):
    return am.MapPlan(**dict(C1, **kw))


def test_blocks_normalisation():
    assert am.normalise_blocks(None, 12) == tuple(range(12))
    assert am.normalise_blocks([0, -1, 5], 12) == (0, 11, 5)
    assert am.normalise_blocks(-12, 12) == (0,) and am.normalise_blocks([], 12) == ()
    for bad, text in (([0, 0], 'block 0 is named twice'), ([3, -9], 'block 3 is named twice'), ([12], 'block 12 is out of range'),
                      ([-13], 'block -13 is out of range'), ([1.0], 'blocks must be integers'), ([True], 'blocks must be integers')):
        with pytest.raises(TcowError, match=text):
            am.normalise_blocks(bad, 12)


@pytest.mark.parametrize('ca,want', [(0, [(t, 0) for t in range(4)]), (1, [(0, 0)]), (2, None), (3, None), (-1, None)])
def test_cls_expansion_per_causal_value(ca, want):
    if want is None:
        with pytest.raises(TcowError, match=f"spatial_queries='cls' but slot 0 takes no part in spatial attention with causal_attention={ca}"):
            am.normalise_queries('cls', 4, 7, ca, False)
    else:
        assert am.normalise_queries('cls', 4, 7, ca, False) == want
    assert am.normalise_queries('cls', 4, 7, 0, True) == [(0, 0)]               # a joint sequence has one cls
    assert am.normalise_queries(None, 4, 7, ca, False) == []


@pytest.mark.parametrize('ca', [0, 1, 2, 3, -1])
def test_divided_positions_with_the_cls_in_and_out(ca):
    s0 = 0 if ca in (0, 1) else 1
    queries = [(3, 5), (0, 1), (2, 5), (3, 6)] + ([(1, 0)] if s0 == 0 else [])
    p = am.MapPlan(2, 2, 4, 7, 2, ca, False, blocks=[1], temporal=False, spatial_queries=queries)
    assert p.s0 == s0 and p.queries == queries and p.keys == 7
    assert p.positions == sorted({s - s0 for _, s in queries})                  # each distinct position once: it serves every frame
    for (frame, slot), (f, k) in zip(queries, p.gather):
        assert f == frame and p.positions[k] == slot - s0                       # sequence b * T + frame, position slot - s0
    assert p.spatial_shape == (2, len(queries), 2, 7) and p.launch_shape == (2 * 4, len(p.positions), 2, 7)


def test_joint_positions_are_the_reference_token_map():
    _, g = load_golden('g6_index_maps')
    for key in [k for k in g if k.startswith('token_src_')]:
        B, T, Hp, Wp = map(int, key.split('_')[2:])
        N = Hp * Wp
        src = g[key]                                   # [b, position-1] -> flat (b*T + t)*N + n of the source token
        for t in range(T):
            for n in range(N):
                pos = am.joint_position(t, 1 + n, T)
                assert pos == 1 + n * T + t and src[0, pos - 1] == t * N + n
        rows = am.joint_source_rows(T, N)              # reference position -> position in the engine's frame-major compacted sequence
        assert rows[0] == 0 and sorted(rows) == list(range(1 + N * T))
        assert all(rows[1 + p] == 1 + int(src[0, p]) for p in range(N * T))
        queries = [(0, 0), (T - 1, N), (1 % T, 1)]
        p = am.MapPlan(2, B, T, N + 1, 2, 0, True, temporal=False, spatial_queries=queries)
        assert p.token_positions == [0, 1 + (N - 1) * T + T - 1, 1 + 1 % T] and p.gather is None and p.columns == rows
        assert p.positions == [rows[t] for t in p.token_positions] == [0, 1 + (T - 1) * N + N - 1, 1 + (1 % T) * N]
        assert p.spatial_shape == p.launch_shape == (B, 3, 2, 1 + N * T)
    assert am.joint_position(0, 0, 7) == 0


def test_refusals_and_their_messages():
    for kw, text in ((dict(causal=2, spatial_queries=[(0, 0)]), r'query \(0, 0\): slot 0 takes no part in spatial attention with causal_attention=2'),
                     (dict(causal=-1, spatial_queries=[(4, 0)]), 'slot 0 takes no part'),
                     (dict(spatial_queries=[(30, 1)]), r'query \(30, 1\): frame 30 is out of range 0 .. 29'),
                     (dict(spatial_queries=[(-1, 1)]), 'frame -1 is out of range'),
                     (dict(spatial_queries=[(0, 301)]), r'query \(0, 301\): slot 301 is out of range 0 .. 300'),
                     (dict(spatial_queries=[(0, -1)]), 'slot -1 is out of range'),
                     (dict(spatial_queries=[7]), r'a spatial query must be \(frame, slot\)'),
                     (dict(spatial_queries='all'), "must be None, 'cls' or a list"),
                     (dict(joint=True, causal=0), "temporal=True with attention_type='joint_space_time'"),
                     (dict(joint=True, causal=0, temporal=False, spatial_queries=[(1, 0)]), r'one cls token, addressed as \(0, 0\)'),
                     (dict(blocks=[0, 0]), 'named twice'),
                     (dict(max_bytes=1), r'take 155520000 bytes \(12 block\(s\) x 12960000\), over max_bytes = 1'),
                     (dict(max_bytes=-1), 'must be a non-negative integer')):
        with pytest.raises(TcowError, match='attention_maps: .*' + text):
            plan(**kw)
    assert plan(joint=True, causal=0, temporal=False, spatial_queries='cls').queries == [(0, 0)]


def test_shapes_and_bytes_at_configs_1():
    p = plan()
    assert p.temporal_shape == (1, 300, 12, 30, 30) and p.spatial_shape is None and p.launch_shape is None
    assert p.bytes_per_block == 1 * 300 * 12 * 30 * 30 * 4 and p.bytes == 12 * p.bytes_per_block
    p = plan(B=3, blocks=[-1], spatial_queries='cls')
    assert p.blocks == (11,) and p.queries == [(0, 0)] and p.positions == [0] and p.gather == [(0, 0)]
    assert p.temporal_shape == (3, 300, 12, 30, 30) and p.spatial_shape == (3, 1, 12, 301) and p.launch_shape == (90, 1, 12, 301)
    assert p.bytes == 3 * 300 * 12 * 30 * 30 * 4 + (3 + 90) * 12 * 301 * 4 and p.columns is None and p.token_positions is None
    assert plan(max_bytes=p.bytes, B=3, blocks=[-1], spatial_queries='cls').bytes == p.bytes       # exactly at the budget: served
    assert am.DEFAULT_MAX_BYTES == 4 << 30
    with pytest.raises(TcowError, match='over max_bytes'):                                          # configs[1] x 3 queries, every (frame, patch) query of a frame
        plan(B=3, temporal=True, spatial_queries=[(t, s) for t in range(30) for s in range(1, 301)], max_bytes=am.DEFAULT_MAX_BYTES // 64)

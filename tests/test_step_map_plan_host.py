"""CPU: the host side of step_maps / step_ragged_maps -- attn_maps.StepMapPlan (blocks, slots, shapes, bytes, refusals), the four step objects'
probs_temporal against their attn_temporal (ops replaced by recorders on CPU tensors, the approach of tests/stream_calls.py), and the public
calls on the call-trace kit: a refused call moves no counter and allocates no page, a rollover pool refuses."""
import pytest
import torch

import stream_calls
from tcow_amd import engine, ops, stream
from tcow_amd._lib import TcowError
from tcow_amd.attn_maps import DEFAULT_MAX_BYTES, StepMapPlan, normalise_slots
from tcow_amd.attn_probe import StepAttentionMaps, StepMapProbe

DEPTH, T, S, HEADS = 12, 30, 301, 12


def plan(rows_or_chunks=(2, 3), causal=1, **kw):
    return StepMapPlan(DEPTH, rows_or_chunks, T, S, HEADS, causal, **kw)


# ---------------------------------------------------------------------------------------------- the plan

def test_blocks_are_those_of_attention_maps():
    assert plan().blocks == tuple(range(DEPTH))
    assert plan(blocks=[-1, 0, 3]).blocks == (11, 0, 3) and plan(blocks=5).blocks == (5,)
    for bad, text in (([12], 'block 12 is out of range'), ([0, -12], 'block 0 is named twice'), ([1.5], 'blocks must be integers'), ([True], 'blocks must be integers')):
        with pytest.raises(TcowError, match=text):
            plan(blocks=bad)


def test_slots_and_the_cls_rules():
    assert plan().slots == [] and plan().positions == [] and plan().spatial_shape is None and plan().spatial_launch is None
    assert plan(spatial_slots='cls').slots == [0] and plan(spatial_slots='cls').positions == [0]
    assert plan(spatial_slots=[7, 0, 300]).slots == [7, 0, 300] and plan(spatial_slots=[7, 0, 300]).positions == [7, 0, 300]
    p2 = plan(causal=2, spatial_slots=[7, 300, 1])
    assert p2.slots == [7, 300, 1] and p2.s0 == 1 and p2.positions == [6, 299, 0]                  # the sequences start at slot 1
    assert plan(spatial_slots=4).slots == [4]
    with pytest.raises(TcowError, match="step_maps: spatial_slots='cls' but slot 0 takes no part in spatial attention with causal_attention=2"):
        plan(causal=2, spatial_slots='cls')
    with pytest.raises(TcowError, match='step_maps: slot 0 takes no part in spatial attention with causal_attention=2'):
        plan(causal=2, spatial_slots=[3, 0])
    with pytest.raises(TcowError, match=r"step_maps: slot 3 is named twice in spatial_slots=\[3, 1, 3\]"):
        plan(spatial_slots=[3, 1, 3])
    for bad, text in (([301], 'slot 301 is out of range 0 .. 300'), ([-1], 'slot -1 is out of range'), ([1.0], 'a spatial slot must be an integer'),
                      ([False], 'a spatial slot must be an integer'), ('all', "must be None, 'cls' or a list of slots")):
        with pytest.raises(TcowError, match=text):
            plan(spatial_slots=bad)
    assert normalise_slots('cls', 5, 1, who='stream.step_maps') == [0]
    with pytest.raises(TcowError, match='^stream_pool.step_maps: slot 9'):
        StepMapPlan(DEPTH, (1, 1), T, S, HEADS, 1, spatial_slots=[9, 9], who='stream_pool.step_maps')


def test_shapes_of_a_rows_step():
    p = plan((2, 3), spatial_slots=[0, 5])
    assert (p.ragged, p.F, p.chunks, p.first) == (False, 6, [3, 3], [0, 3])
    assert p.temporal_launch == (6, 300, 12, 30) and p.temporal_shape == (2, 300, 12, 3, 30)
    assert p.spatial_launch == (6, 2, 12, 301) and p.spatial_shape == (2, 3, 2, 12, 301)
    q = plan((2, 3), temporal=False, spatial_slots='cls')
    assert q.temporal_launch is None and q.temporal_shape is None and q.spatial_shape == (2, 3, 1, 12, 301)


def test_shapes_of_a_ragged_step():
    p = plan([1, 2, 1], spatial_slots=[5])
    assert (p.ragged, p.F, p.chunks, p.first) == (True, 4, [1, 2, 1], [0, 1, 3])
    assert p.temporal_launch == (4, 300, 12, 30) and p.temporal_shape == [(1, 300, 12, 1, 30), (1, 300, 12, 2, 30), (1, 300, 12, 1, 30)]
    assert p.spatial_launch == (4, 1, 12, 301) and p.spatial_shape == [(1, 1, 1, 12, 301), (1, 2, 1, 12, 301), (1, 1, 1, 12, 301)]
    for bad in ([], [1, 0], (0, 3), (2, 0)):
        with pytest.raises(TcowError, match='at least one row and every row at least one frame'):
            plan(bad)


def test_bytes_and_the_budget():
    t_bytes, s_bytes = 2 * 4 * 6 * 300 * 12 * 30, 4 * 6 * 2 * 12 * 301
    p = plan((2, 3), spatial_slots=[0, 5], blocks=[0, 1, 2])
    assert p.bytes_per_block == t_bytes + s_bytes and p.bytes == 3 * (t_bytes + s_bytes)
    assert plan((2, 3), temporal=False, spatial_slots=[0, 5], blocks=[4]).bytes == s_bytes and plan((2, 3), blocks=[4]).bytes == t_bytes
    assert plan((2, 3), temporal=False).bytes == 0
    assert plan((2, 3), blocks=[4], max_bytes=t_bytes).bytes == t_bytes                                 # at the budget: served
    with pytest.raises(TcowError, match=rf'step_maps: the maps asked for take {t_bytes} bytes \(1 block\(s\) x {t_bytes}\), over max_bytes = {t_bytes - 1}'):
        plan((2, 3), blocks=[4], max_bytes=t_bytes - 1)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(TcowError, match='max_bytes .* must be a non-negative integer'):
            plan(max_bytes=bad)
    assert DEFAULT_MAX_BYTES == 4 << 30


# ---------------------------------------------------------------------------------------------- the step objects

class _State:
    """What a step object reads of its state, on the CPU."""
    T_total, n_slots, n_pages, P, pos, skinny, cq = 40, 4, 17, 8, None, False, ops.FP8

    def __init__(self):
        self.k_cache = torch.zeros(3, 4, 2, 2, 40, 64, dtype=torch.float8_e4m3fn)
        self.v_cache = torch.zeros(3, 4, 2, 2, 40, 64, dtype=torch.float8_e4m3fn)


def _same(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and (a.data_ptr(), tuple(a.shape), a.dtype, a.stride()) == (b.data_ptr(), tuple(b.shape), b.dtype, b.stride())
    return type(a) is type(b) and a == b


@pytest.mark.parametrize('form', ['stream', 'pool', 'ragged', 'paged'])
def test_probs_temporal_passes_what_attn_temporal_passes(monkeypatch, form):
    calls = []
    wrappers = {'stream': 'attn_temporal_cached', 'pool': 'attn_temporal_pool', 'ragged': 'attn_temporal_ragged', 'paged': 'attn_temporal_ragged_paged'}
    for name in wrappers.values():
        monkeypatch.setattr(ops, name, lambda *a, _name=name, **k: calls.append((_name, a, k)))
    monkeypatch.setattr(ops, 'attn_temporal_step_probs', lambda *a, **k: calls.append(('probs', a, k)))
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    st, time_rows = _State(), torch.zeros(4, 128)
    ragged = (i32(3, 0), i32(2, 1), i32(0, 3), i32(3, 1), i32(0, 0, 0, 1))
    step = {'stream': lambda: stream._StreamStep(st, time_rows, i32(5)), 'pool': lambda: stream._PoolStep(st, time_rows, i32(5, 0), i32(2, 1)),
            'ragged': lambda: stream._RaggedStep(st, time_rows, *ragged),
            'paged': lambda: stream._PagedRaggedStep(st, time_rows, *ragged, torch.zeros(2, 5, dtype=torch.int32))}[form]()
    QKV, O, PR = torch.zeros(12, 384), torch.zeros(12, 128), torch.zeros(4, 2, 2, 40)
    shape = (ops.F32, 2, 2, 3, 128, 2, 1) if form in ('stream', 'pool') else (ops.F32, 1, 4, 3, 128, 2, 1)
    step.attn_temporal(1, *shape, QKV, O)
    step.probs_temporal(1, *shape, QKV, PR)
    (name, a, ka), (tag, p, kp) = calls
    assert name == wrappers[form] and tag == 'probs' and p[0] == form
    assert ka == {} and kp == {'cache_dtype': a[-1]} and a[-1] == st.cq                                # the cache type of the state
    assert a[-2] is O and p[-1] is PR
    assert len(a) - 2 == len(p) - 2 and all(_same(x, y) for x, y in zip(a[:-2], p[1:-1])), (a, p)    # shape, T_total, tables, QKV, caches: the same
    assert _same(a[-4], st.k_cache[1]) and _same(a[-3], st.v_cache[1]) and a[-5] is QKV               # block 1's caches


# ---------------------------------------------------------------------------------------------- the public calls, on the call-trace kit

H, W = stream_calls.H, stream_calls.W
BAD = [dict(blocks=[3]), dict(spatial_slots=[1, 1]), dict(spatial_slots=[7]), dict(max_bytes=0), dict(blocks=[0, 0]), dict(spatial_slots='patches')]


@pytest.fixture
def traced(monkeypatch):
    trace = stream_calls.install(monkeypatch)
    probes = []
    recorded = engine.run_forward
    monkeypatch.setattr(engine, 'run_forward', lambda *a, **k: (probes.append(k.get('probe')), recorded(*a, **k))[1])
    return trace, probes


def test_stream_step_maps_on_the_host(traced):
    trace, probes = traced
    st = stream_calls.make_net().stream(batch_size=2, queries_per_clip=2)
    rgb = torch.zeros(2, 3, 2, H, W)
    for bad in BAD:
        with pytest.raises(TcowError, match='^stream.step_maps: |^attention_maps: block'):
            st.step_maps(rgb, **bad)
        assert st.frames_done == 0 and trace == []
    mask, flags, maps = st.step_maps(rgb, blocks=[0], spatial_slots='cls')
    assert st.frames_done == 2 and len(trace) == 1 and isinstance(probes[0], StepMapProbe) and isinstance(maps, StepAttentionMaps)
    assert (maps.slots, maps.t0) == ([0], 0) and probes[0].plan.temporal_shape == (4, 6, 1, 2, 4)
    m2, f2 = st.step(rgb[:, :, :1])
    assert probes[1] is None and st.frames_done == 3 and m2.shape[2] == 1                              # step() passes no probe
    with pytest.raises(TcowError, match='stream.step_maps: frames 3..4 run past the last frame 3'):
        st.step_maps(rgb)


@pytest.mark.parametrize('paged', [False, True])
def test_a_refused_pool_call_moves_no_counter_and_allocates_no_page(traced, paged):
    trace, probes = traced
    pool = stream_calls.make_net().stream_pool(3, **(dict(page_frames=1, pages=12) if paged else {}))
    a, b = pool.open(), pool.open()
    pool.step([a], torch.zeros(1, 3, 1, H, W))
    d = stream_calls.Driver(trace, pool)
    before, n = d.state(), len(trace)
    rgb = torch.zeros(2, 3, 2, H, W)
    for bad in BAD:
        with pytest.raises(TcowError, match='^stream_pool.step_maps: |^attention_maps: block'):
            pool.step_maps([a, b], rgb, **bad)
        with pytest.raises(TcowError, match='^stream_pool.step_ragged_maps: |^attention_maps: block'):
            pool.step_ragged_maps([b, a], [rgb[:1], rgb[1:, :, :1]], **bad)
        assert d.state() == before and len(trace) == n
    mask, flags, maps = pool.step_maps([b, a], rgb, blocks=[0], spatial_slots=[0, 2])
    assert isinstance(probes[-1], StepMapProbe) and maps.t0 == [0, 1] and maps.slots == [0, 2] and (mask.shape[0], mask.shape[2]) == (2, 2)
    assert [pool.frames_done(i) for i in (a, b)] == [3, 2] and (not paged or pool.pages_free == 7)
    masks, flags, maps = pool.step_ragged_maps([b, a], [rgb[:1], rgb[1:, :, :1]], temporal=False)
    assert maps.t0 == [2, 3] and probes[-1].plan.ragged and probes[-1].plan.chunks == [2, 1] and [m.shape[2] for m in masks] == [2, 1]
    assert [pool.frames_done(i) for i in (a, b)] == [4, 4]
    c = pool.open()                                             # step() and step_ragged() still return two values and pass no probe
    assert len(pool.step([c], rgb[:1])) == 2 and probes[-1] is None and len(pool.step_ragged([c], [rgb[:1, :, :1]])) == 2


@pytest.mark.parametrize('kw', [{}, dict(page_frames=2)])
def test_a_rollover_pool_refuses(traced, kw):
    trace, _ = traced
    pool = stream_calls.make_net().stream_pool(4, rollover=1, **kw)
    a = pool.open()
    d = stream_calls.Driver(trace, pool)
    before = d.state()
    with pytest.raises(TcowError, match='stream_pool.step_maps: a rollover pool .* serves no attention maps'):
        pool.step_maps([a], torch.zeros(1, 3, 1, H, W))
    with pytest.raises(TcowError, match='stream_pool.step_ragged_maps: a rollover pool .* serves no attention maps'):
        pool.step_ragged_maps([a], [torch.zeros(1, 3, 1, H, W)])
    assert d.state() == before and trace == []

"""GPU: step_maps / step_ragged_maps of live sessions -- the step's outputs bit for bit, the right tensors in the public layout (the float64
softmax of the q, own keys and cache lines the launch was given, cloned at call time), the forms, the compact cache's rounding rule, and the
fp32 maps of a clip streamed frame by frame against the oracle and against the clip path.

Nets: test_gpu_attention_maps.py's (depth 2, D = 128, 2 heads, T = 4, 32 x 48 frames, 2 clips x 2 queries = 4 query rows) and
stream_kit._small_net."""
import pytest
import torch

from attn_probs_kit import U32, prob_bound, worst
from stream_kit import PRECISIONS, _small_clips, _small_net
from test_gpu_attention_maps import B, DEPTH, HEADS, N, QS, S, T, build, case, oracle_probs
from test_gpu_stream_cache_dtype import _dec
from test_gpu_stream_probs import _ref64
from tcow_amd import ops

pytestmark = pytest.mark.gpu

ROWS = B * QS
SLOTS = {1: [3, 0, N, 1], 2: [3, N, 1]}                       # unsorted; the cls where it takes part
PAIR = {('fp32', None): 'f32', ('bf16x3', None): 'f32', ('bf16', None): 'bf16', ('fp16', None): 'fp16', ('fp32', 'fp8'): 'f32_fp8', ('bf16x3', 'fp8'): 'f32_fp8',
        ('bf16', 'fp8'): 'bf16_fp8', ('fp16', 'fp8'): 'fp16_fp8', ('fp32', 'bf16'): 'f32_bf16'}


def _feed(st, rgb, qm, t, c, maps=None):
    """The next c frames from frame t into a stream: step(), or step_maps(**maps)."""
    r, q = rgb[:, :, t:t + c].cuda(), qm[:, :, t:t + c].cuda()
    return st.step(r, q) if maps is None else st.step_maps(r, q, **maps)


@pytest.fixture
def captured(monkeypatch):
    """ops.attn_temporal_step_probs and ops.attn_probs wrapped: every call keeps clones of what it was given, then runs."""
    temporal, spatial = [], []
    real_t, real_s = ops.attn_temporal_step_probs, ops.attn_probs

    def wrap_t(form, *a, **k):
        qkv, kc, vc, probs = a[-4:]
        temporal.append(dict(form=form, args=[x.clone() if torch.is_tensor(x) else x for x in a[:-4]], qkv=qkv.clone(), kc=kc.clone(), vc=vc.clone()))
        return real_t(form, *a, **k)

    def wrap_s(shape, spatial_rows, qkv, out, lse=None, pos=None):
        spatial.append(dict(shape=shape, qkv=qkv.clone()))
        return real_s(shape, spatial_rows, qkv, out, lse=lse, pos=pos)

    monkeypatch.setattr(ops, 'attn_temporal_step_probs', wrap_t)
    monkeypatch.setattr(ops, 'attn_probs', wrap_s)
    return temporal, spatial


def _sessions_of(call):
    """Per session of a captured launch: (first flat frame, c, t0, its K block [S-1, heads, >= t0, 64] in frame order)."""
    a, kc = call['args'], call['kc']
    if call['form'] == 'stream':
        n, c, t0 = a[1], a[2], int(a[8][0])
        return [(r * c, c, t0, kc[r]) for r in range(n)]
    if call['form'] == 'pool':
        n, c = a[1], a[2]
        return [(r * c, c, int(a[9][r]), kc[int(a[10][r])]) for r in range(n)]
    if call['form'] == 'ragged':
        return [(int(a[11][r]), int(a[12][r]), int(a[9][r]), kc[int(a[10][r])]) for r in range(a[1])]
    P, out = a[9], []
    for r in range(a[1]):
        t0 = int(a[10][r])
        pages = [int(p) for p in a[11][r][:-(-t0 // P)]]                                    # the pages of frames < t0
        block = torch.cat([kc[p] for p in pages], 2) if pages else kc[0][:, :, :0]
        out.append((int(a[12][r]), int(a[13][r]), t0, block))
    return out


def _check_temporal(call, got_rows, pair, tag):
    """got_rows[r]: session r's map in the public layout (N, heads, c, T) against the f64 softmax of the captured tensors, within prob_bound."""
    Sx, heads, T_total = call['args'][3], call['args'][5], call['args'][7]
    for r, (f0, c, t0, block) in enumerate(_sessions_of(call)):
        ref = _ref64(pair, call['qkv'][f0 * Sx:(f0 + c) * Sx], block, c, t0, Sx, heads, T_total)
        got = got_rows[r].permute(2, 0, 1, 3)                                               # -> [c, N, heads, T]
        idx, g, w, d, b = worst(got, ref['P'], prob_bound(ref))
        assert d <= b, (tag, r, idx, g, w, d, b)


# ---------------------------------------------------------------------------------------------- (1) same outputs

@pytest.mark.parametrize('ca', [1, 2])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_step_maps_returns_the_bits_of_step(cuda, precision, ca):
    cfg, sd, rgb, qm = case(ca)
    net = build(cfg, sd, precision)
    a, b = net.stream(batch_size=B, queries_per_clip=QS), net.stream(batch_size=B, queries_per_clip=QS)
    t = 0
    for c in (1, 2, 1):
        m, f, maps = _feed(a, rgb, qm, t, c, dict(spatial_slots=SLOTS[ca]))
        m0, f0 = _feed(b, rgb, qm, t, c)
        assert torch.equal(m, m0) and torch.equal(f, f0), (precision, ca, t)
        assert maps.t0 == t and maps.slots == SLOTS[ca] and sorted(maps.temporal) == sorted(maps.spatial) == [0, 1]
        for i in range(DEPTH):
            assert maps.temporal[i].shape == (ROWS, N, HEADS, c, T) and maps.spatial[i].shape == (ROWS, c, len(SLOTS[ca]), HEADS, S)
            assert maps.temporal[i].is_contiguous() and bool((maps.temporal[i][..., t + c:] == 0).all())
        t += c
        assert a.frames_done == b.frames_done == t


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_step_maps_leaves_a_graph_stream_alone(cuda, precision):
    cfg, sd, rgb, qm = case(1)
    net = build(cfg, sd, precision)
    g, e = net.stream(batch_size=B, queries_per_clip=QS, graph=True), net.stream(batch_size=B, queries_per_clip=QS)
    outs = [_feed(g, rgb, qm, 0, 1)]                                                           # eager, and captures c = 1
    graphs = dict(g._graphs)
    outs.append(_feed(g, rgb, qm, 1, 1, dict(blocks=[1], spatial_slots='cls'))[:2])            # eager, with maps
    assert g._graphs == graphs and g.frames_done == 2
    outs += [_feed(g, rgb, qm, 2, 1), _feed(g, rgb, qm, 3, 1)]                                 # replays
    for t, (m, f) in enumerate(outs):
        m0, f0 = _feed(e, rgb, qm, t, 1)
        assert torch.equal(m, m0) and torch.equal(f, f0), (precision, t)


# ---------------------------------------------------------------------------------------------- (2) the right tensors

@pytest.mark.parametrize('ca', [1, 2])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_maps_are_the_softmax_of_what_the_step_was_given(cuda, captured, precision, ca):
    temporal, spatial = captured
    cfg, sd, rgb, qm = case(ca)
    net = build(cfg, sd, precision)
    st, twin = net.stream(batch_size=B, queries_per_clip=QS), net.stream(batch_size=B, queries_per_clip=QS)
    slots, s0 = SLOTS[ca], 0 if ca == 1 else 1
    _feed(st, rgb, qm, 0, 1); _feed(twin, rgb, qm, 0, 1)
    assert temporal == [] and spatial == []                                                    # step() asks for no maps
    _, _, maps = _feed(st, rgb, qm, 1, 2, dict(spatial_slots=slots))
    assert [c['form'] for c in temporal] == ['stream'] * DEPTH and len(spatial) == DEPTH
    real_probs = ops.attn_probs
    for i in range(DEPTH):
        _check_temporal(temporal[i], maps.temporal[i], PAIR[precision, None], (precision, ca, i))
        assert bool(((maps.temporal[i].double().sum(-1) - 1).abs() <= (T + 8) * U32).all())
        for k, slot in enumerate(slots):
            one = torch.empty(ROWS * 2, 1, HEADS, S, device=cuda)
            real_probs(spatial[i]['shape'], True, spatial[i]['qkv'], one, pos=torch.tensor([slot - s0], dtype=torch.int32, device=cuda))
            assert torch.equal(maps.spatial[i][:, :, k], one.view(ROWS, 2, HEADS, S)), (precision, ca, i, slot)
    # blocks and halves can be left out: the same bits for what remains
    _, _, part = _feed(twin, rgb, qm, 1, 2, dict(blocks=[-1], temporal=False, spatial_slots=slots[:2]))
    assert part.temporal == {} and list(part.spatial) == [1] and torch.equal(part.spatial[1], maps.spatial[1][:, :, :2])
    twin.reset(); _feed(twin, rgb, qm, 0, 1)
    _, _, part = _feed(twin, rgb, qm, 1, 2, dict(blocks=[0]))
    assert part.spatial == {} and list(part.temporal) == [0] and torch.equal(part.temporal[0], maps.temporal[0]) and part.slots == []


# ---------------------------------------------------------------------------------------------- (3) forms

def _run_forms(net, clip, cache_dtype, maps_kw):
    """The same clip through a stream, a pool, a ragged pool and a paged ragged pool in chunks (1, 2, 1): {form: [maps per step]}."""
    rgb, qm = clip
    out = {}
    st = net.stream(cache_dtype=cache_dtype)
    pools = {'pool': net.stream_pool(2, cache_dtype=cache_dtype), 'ragged': net.stream_pool(2, cache_dtype=cache_dtype),
             'paged': net.stream_pool(2, page_frames=2, cache_dtype=cache_dtype)}
    ids = {k: (p.open(), p.open())[1] for k, p in pools.items()}                                # the second slot
    for form in ('stream', 'pool', 'ragged', 'paged'):
        t, got = 0, []
        for c in (1, 2, 1):
            r, q = rgb[:, :, t:t + c], qm[:, :, t:t + c]
            if form == 'stream':
                m, f, maps = st.step_maps(r, q, **maps_kw)
                got.append((m, maps.temporal, maps.spatial))
            elif form == 'pool':
                m, f, maps = pools[form].step_maps([ids[form]], r, q, **maps_kw)
                got.append((m, maps.temporal, maps.spatial))
            else:
                m, f, maps = pools[form].step_ragged_maps([ids[form]], [r], [q], **maps_kw)
                got.append((m[0], {i: v[0] for i, v in maps.temporal.items()}, {i: v[0] for i, v in maps.spatial.items()}))
            t += c
        out[form] = got
    return out


@pytest.mark.parametrize('precision,cache_dtype', [('bf16', None), ('fp32', None), ('bf16', 'fp8'), ('fp32', 'fp8'), ('fp32', 'bf16')])
def test_every_form_serves_the_maps_of_its_own_step(cuda, captured, precision, cache_dtype):
    """Every form's maps are the float64 softmax of the tensors ITS launch was given (a compact cache: of the ROUNDED keys), within prob_bound;
    the four forms give the same bits, as their step outputs do; rows sum to 1 and masked entries are +0.0."""
    temporal, _ = captured
    net = _small_net(precision)
    clip = _small_clips(1)[0]
    got = _run_forms(net, clip, cache_dtype, dict(spatial_slots='cls'))
    forms = ('stream', 'pool', 'ragged', 'paged')
    assert [c['form'] for c in temporal] == [f for f in forms for _ in range(3 * 2)]            # three steps x two blocks each
    pair, Tn = PAIR[precision, cache_dtype], 4
    for fi, form in enumerate(forms):
        t = 0
        for k, c in enumerate((1, 2, 1)):
            m, tmaps, smaps = got[form][k]
            for i in range(2):
                call = temporal[(fi * 3 + k) * 2 + i]
                assert tmaps[i].shape[0] == 1 and tmaps[i].shape[3:] == (c, Tn) and smaps[i].shape[:3] == (1, c, 1)
                _check_temporal(call, tmaps[i], pair, (precision, cache_dtype, form, k, i))
                assert bool(((tmaps[i].double().sum(-1) - 1).abs() <= (Tn + 8) * U32).all())
                past = torch.arange(Tn, device=cuda)[None, :] > (t + torch.arange(c, device=cuda))[:, None]
                assert bool((tmaps[i].view(torch.int32)[..., past] == 0).all())                  # +0.0, bitwise
            t += c
    for k in range(3):                                                                          # where a key lives does not enter the arithmetic
        assert torch.equal(got['paged'][k][0], got['ragged'][k][0])
        for i in range(2):
            assert torch.equal(got['paged'][k][1][i], got['ragged'][k][1][i]) and torch.equal(got['paged'][k][2][i], got['ragged'][k][2][i])
    # one session and the same chunk lengths: the three contiguous forms run the same GEMM shapes on the same rows and share the per-frame
    # kernel bodies, so their steps -- and with them their maps -- are bit-identical too
    for f in ('pool', 'ragged'):
        for k in range(3):
            assert torch.equal(got['stream'][k][0], got[f][k][0]), (f, k)
            assert all(torch.equal(got['stream'][k][1][i], got[f][k][1][i]) and torch.equal(got['stream'][k][2][i], got[f][k][2][i]) for i in range(2)), (f, k)
    if cache_dtype == 'fp8':
        # the rounding rule: the stream's second step (frames 1, 2 at t0 = 1) attends to its own keys at their ROUNDED values -- its maps, within
        # the bound of the rounded softmax above, are outside the bound of the softmax of the same cache lines and the UNROUNDED own keys
        call = temporal[2]
        Sx, heads = call['args'][3], call['args'][5]
        cached = _dec(call['kc'][0]).to(call['qkv'].dtype)                                      # (fp8 values are exact in every storage type)
        ref_u = _ref64(PAIR[precision, None], call['qkv'], cached, 2, 1, Sx, heads, Tn)
        rows = got['stream'][1][1][0][0].permute(2, 0, 1, 3)
        excess = float(((rows.double() - ref_u['P']).abs() - prob_bound(ref_u)).max())
        print(f'{precision} fp8: largest excess over the bound of the unrounded softmax {excess:.3e}')
        assert excess > 0, 'the maps are the softmax of the unrounded keys'


# ---------------------------------------------------------------------------------------------- (4) fp32 against the clip path and the oracle

def test_fp32_streamed_maps_against_the_oracle_and_the_clip_path(cuda):
    """The clip streamed frame by frame, the steps' maps concatenated along dim 3.  Against the oracle's float64 probabilities the criterion of
    test_fp32_maps_against_the_oracle: 4 x the oracle's own f32-against-f64 spread + 1e-7 (summation orders are all that separates the paths);
    against the clip path's attention_maps the triangle sum of the two, 8 x spread + 2e-7.  Prints the ratios."""
    cfg, sd, rgb, qm = case(1)
    p64 = oracle_probs(sd, cfg, rgb, qm, [(0, 0)], torch.float64)
    p32 = oracle_probs(sd, cfg, rgb, qm, [(0, 0)], torch.float32)
    net = build(cfg, sd, 'fp32')
    _, _, clip_maps = net.attention_maps(rgb.cuda(), qm.cuda())
    st = net.stream(batch_size=B, queries_per_clip=QS)
    steps = [_feed(st, rgb, qm, t, 1, {})[2] for t in range(T)]
    for i in range(DEPTH):
        got = torch.cat([m.temporal[i] for m in steps], 3)
        assert got.shape == (ROWS, N, HEADS, T, T)
        spread = float((p32[i]['temporal'].double() - p64[i]['temporal']).abs().max())
        d = float((got.cpu().double() - p64[i]['temporal']).abs().max())
        dc = float((got - clip_maps.temporal[i]).abs().max())
        print(f'block {i} temporal: streamed vs oracle f64 max|d| {d:.3e} (ratio {d / max(spread, 1e-30):.2f} of the oracle f32 spread {spread:.3e}); '
              f'streamed vs clip path max|d| {dc:.3e} (ratio {dc / max(spread, 1e-30):.2f})')
        assert spread > 0 and d <= 4 * spread + 1e-7, (i, d, spread)
        assert dc <= 8 * spread + 2e-7, (i, dc, spread)

"""GPU: Seeker.attention_maps on tiny nets -- the plumbing bit for bit in all four precisions (the right block, the right half, the right query
row order, the right position map), the fp32 maps against the oracle, and the refusals.

Net: depth 2, D = 128, 2 heads, T = 4, 32 x 48 frames (N = 6 patches), 2 clips with two queries each (4 query rows)."""
import pytest
import torch

from conftest import build_hip_seeker
from tcow_amd import synth
from tcow_amd._lib import TcowError

pytestmark = pytest.mark.gpu

PRECISIONS = ('bf16', 'fp16', 'fp32', 'bf16x3')
T, HP, WP, D, HEADS, DEPTH, B, QS = 4, 2, 3, 128, 2, 2, 2, 2
N, S = HP * WP, HP * WP + 1
QUERIES = [(3, 2), (0, 1), (1, N), (3, 1), (2, 2)]             # unsorted, a repeated frame, a repeated slot; (frame, 0) is added where the cls takes part


def case(ca, joint=False, seed=3):
    cfg = synth.seeker_config(num_total_frames=T, frame_height=16 * HP, frame_width=16 * WP, embed_dim=D, depth=DEPTH, num_heads=HEADS,
                              causal_attention=ca, **(dict(attention_type='joint_space_time') if joint else {}))
    sd = synth.make_state_dict(cfg, 8000 + seed)
    clip = synth.make_clip(B, T, 16 * HP, 16 * WP, seed=8100 + seed)
    rgb = torch.from_numpy(clip['rgb'])
    qm = torch.stack([torch.from_numpy(synth.make_query_mask(clip, q, 0)) for q in range(QS)], 1).reshape(B * QS, 1, T, 16 * HP, 16 * WP)   # clip-major rows
    return cfg, sd, rgb, qm


def build(cfg, sd, precision):
    if cfg['attention_type'] == 'divided_space_time':
        return build_hip_seeker(cfg, sd, precision).cuda().eval()
    from tcow_amd.seeker import Seeker
    net = Seeker(None, num_total_frames=T, frame_height=cfg['frame_height'], frame_width=cfg['frame_width'], tracker_pretrained=False, patch_size=16,
                 causal_attention=0, attention_type='joint_space_time', drop_path_rate=0.0, network_depth=DEPTH, embed_dim=D,
                 norm_embeddings=cfg['norm_embeddings'], track_map_stride=cfg['track_map_stride'], track_map_resize=cfg['track_map_resize'],
                 num_heads=HEADS, precision=precision)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.cuda().eval()


def queries_for(ca, joint):
    return QUERIES + ([(0, 0)] if joint else [(2, 0), (0, 0)] if ca in (0, 1) else [])


def saved_qkv(net, rgb, qm):
    """Every block's own qkv tensors, obtained without the probe: the activations run_forward(save=True) keeps (save decides what is kept,
    never what is computed)."""
    from tcow_amd import engine
    m = net.seeker
    with torch.no_grad():
        _, _, sv = engine.run_forward(m, rgb.cuda().float().contiguous(), qm.cuda().float().contiguous(), m.param_list(), save=True)
    return sv['blocks']


@pytest.mark.parametrize('ca', [0, 1, 2, 3, -1])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_divided_maps_are_attn_probs_of_the_blocks_own_qkv(cuda, precision, ca):
    from tcow_amd import ops
    cfg, sd, rgb, qm = case(ca)
    net = build(cfg, sd, precision)
    queries = queries_for(ca, False)
    om, fl, maps = net.attention_maps(rgb.cuda(), qm.cuda(), spatial_queries=queries)
    with torch.no_grad():
        om0, fl0 = net(rgb.cuda(), qm.cuda())
    assert torch.equal(om, om0) and torch.equal(fl, fl0)
    assert maps.queries == queries and sorted(maps.temporal) == sorted(maps.spatial) == [0, 1]
    m = net.seeker
    rows, s0 = B * QS, 0 if ca in (0, 1) else 1
    shape = ops.attn_shape(ops.F32X3 if precision == 'bf16x3' else m.mode, rows, T, S, D, HEADS, ca)
    for i, st in enumerate(saved_qkv(net, rgb, qm)):
        want = torch.empty(rows, N, HEADS, T, T, device=cuda)
        ops.attn_probs(shape, False, st['QKV_t'], want)
        assert maps.temporal[i].shape == want.shape and torch.equal(maps.temporal[i], want), (precision, ca, i, 'temporal')
        assert maps.spatial[i].shape == (rows, len(queries), HEADS, S)
        for k, (frame, slot) in enumerate(queries):
            one = torch.empty(rows * T, 1, HEADS, S, device=cuda)
            ops.attn_probs(shape, True, st['QKV_s'], one, pos=torch.tensor([slot - s0], dtype=torch.int32, device=cuda))
            assert torch.equal(maps.spatial[i][:, k], one.view(rows, T, HEADS, S)[:, frame]), (precision, ca, i, (frame, slot))
        assert float(maps.temporal[i].sum(-1).sub(1).abs().max()) < 1e-5 and float(maps.spatial[i].sum(-1).sub(1).abs().max()) < 1e-5
    # blocks and halves can be left out: the same bits for what remains
    _, _, part = net.attention_maps(rgb.cuda(), qm.cuda(), blocks=[-1], temporal=False, spatial_queries=queries[:2])
    assert part.temporal == {} and list(part.spatial) == [1] and torch.equal(part.spatial[1], maps.spatial[1][:, :2])
    _, _, part = net.attention_maps(rgb.cuda(), qm.cuda(), blocks=[0])
    assert part.spatial == {} and list(part.temporal) == [0] and torch.equal(part.temporal[0], maps.temporal[0]) and part.queries == []


@pytest.mark.parametrize('precision', PRECISIONS)
def test_joint_maps_are_attn_probs_of_the_compacted_qkv(cuda, precision):
    from tcow_amd import ops
    cfg, sd, rgb, qm = case(0, joint=True)
    net = build(cfg, sd, precision)
    queries = queries_for(0, True)
    om, fl, maps = net.attention_maps(rgb.cuda(), qm.cuda(), temporal=False, spatial_queries=queries)
    with torch.no_grad():
        om0, fl0 = net(rgb.cuda(), qm.cuda())
    assert torch.equal(om, om0) and torch.equal(fl, fl0) and maps.temporal == {} and sorted(maps.spatial) == [0, 1]
    rows, Lj = B * QS, 1 + N * T
    shape = ops.attn_shape(ops.F32X3 if precision == 'bf16x3' else net.seeker.mode, rows, 1, Lj, D, HEADS, 0)
    # the engine's compacted sequence is frame-major ((t, n) at 1 + t N + n); the public key axis is the reference's token order, 1 + n T + t
    cols = torch.tensor([0] + [1 + t * N + n for n in range(N) for t in range(T)], device=cuda)
    for i, st in enumerate(saved_qkv(net, rgb, qm)):
        assert maps.spatial[i].shape == (rows, len(queries), HEADS, Lj)
        for k, (frame, slot) in enumerate(queries):
            at = 0 if slot == 0 else 1 + frame * N + slot - 1
            one = torch.empty(rows, 1, HEADS, Lj, device=cuda)
            ops.attn_probs(shape, True, st['QKV_s'], one, pos=torch.tensor([at], dtype=torch.int32, device=cuda))
            assert torch.equal(maps.spatial[i][:, k], one[:, 0][..., cols]), (precision, i, (frame, slot))


# ------------------------------------------------------------------------------------------------------------------- against the oracle (fp32)

def oracle_probs(sd, cfg, rgb, qm, queries, dtype):
    """Block by block, the probabilities the reference materialises (vit.py:88-101), restated from the oracle's taps in `dtype` on the CPU:
    -> [{'temporal': (rows, N, heads, T, T) or None, 'spatial': (rows, nq, heads, keys)}] in attention_maps' layout."""
    from oracle import seeker_oracle as so
    tsd = so.to_torch_state_dict(sd, dtype)
    taps = {}
    rows = qm.shape[0]
    frames = rgb[:, None].expand(B, QS, *rgb.shape[1:]).reshape(rows, *rgb.shape[1:])
    so.seeker_forward(tsd, cfg, frames.to(dtype), qm.to(dtype), taps=taps)
    ca, joint = cfg['causal_attention'], cfg['attention_type'] == 'joint_space_time'

    def probs(x, w, b, keep):
        L = x.shape[1]
        qkv = (x @ w.t() + b).reshape(x.shape[0], L, 3, HEADS, 64).permute(2, 0, 3, 1, 4)
        a = (qkv[0] @ qkv[1].transpose(-2, -1)) * (64 ** -0.5)
        if keep is not None:
            a = a.masked_fill(~keep, -1e10)
        return a.softmax(dim=-1)                                                     # [Bq, heads, L, L]

    out = []
    for i in range(cfg['depth']):
        X, CLS = (taps['tokens_in'], taps['cls_in']) if i == 0 else (taps[f'block{i - 1}'], taps[f'cls{i - 1}'])
        b = so.PREFIX + f'blocks.{i}.'
        if joint:
            allt = torch.cat([CLS[:, None, :], X.reshape(rows, T * N, D)], dim=1)     # frame-major, as the oracle runs it
            P = probs(so.layer_norm(allt, tsd[b + 'norm1.weight'], tsd[b + 'norm1.bias']), tsd[b + 'attn.qkv.weight'], tsd[b + 'attn.qkv.bias'], None)
            cols = torch.tensor([0] + [1 + t * N + n for n in range(N) for t in range(T)])
            sp = torch.stack([P[:, :, 0 if s == 0 else 1 + f * N + s - 1][..., cols] for f, s in queries], 1)
            out.append(dict(temporal=None, spatial=sp))
            continue
        U = so.layer_norm(X, tsd[b + 'temporal_norm1.weight'], tsd[b + 'temporal_norm1.bias'])
        Ut = U.permute(0, 2, 1, 3).reshape(rows * N, T, D)
        Pt = probs(Ut, tsd[b + 'temporal_attn.qkv.weight'], tsd[b + 'temporal_attn.qkv.bias'], so.causal_keep_mask(T, ca) if ca > 0 else None)
        R = so.attention(Ut, tsd[b + 'temporal_attn.qkv.weight'], tsd[b + 'temporal_attn.qkv.bias'], tsd[b + 'temporal_attn.proj.weight'],
                         tsd[b + 'temporal_attn.proj.bias'], HEADS, ca)
        R = R @ tsd[b + 'temporal_fc.weight'].t() + tsd[b + 'temporal_fc.bias']
        Xt = X + R.reshape(rows, N, T, D).permute(0, 2, 1, 3)
        use_cls = ca in (0, 1)
        Vin = torch.cat([CLS[:, None, None, :].expand(rows, T, 1, D), Xt], dim=2) if use_cls else Xt
        L = Vin.shape[2]
        Ps = probs(so.layer_norm(Vin, tsd[b + 'norm1.weight'], tsd[b + 'norm1.bias']).reshape(rows * T, L, D), tsd[b + 'attn.qkv.weight'],
                   tsd[b + 'attn.qkv.bias'], None).reshape(rows, T, HEADS, L, L)
        s0 = S - L
        sp = torch.stack([torch.nn.functional.pad(Ps[:, f, :, s - s0], (s0, 0)) for f, s in queries], 1)
        out.append(dict(temporal=Pt.reshape(rows, N, HEADS, T, T), spatial=sp))
    return out


@pytest.mark.parametrize('ca,joint', [(1, False), (0, False), (0, True)])
def test_fp32_maps_against_the_oracle(cuda, ca, joint):
    """Bound: 4 x the oracle's own float32-against-float64 spread of the same probabilities + 1e-7 (the factor 4 for the different summation
    orders: MFMA K-chunks in the GEMMs, LayerNorm's reduction tree).  The spread comes from the reference restatement on the CPU, not from the
    code under test.  Prints the measured ratio per block and kind."""
    cfg, sd, rgb, qm = case(ca, joint)
    queries = queries_for(ca, joint)
    p64 = oracle_probs(sd, cfg, rgb, qm, queries, torch.float64)
    p32 = oracle_probs(sd, cfg, rgb, qm, queries, torch.float32)
    net = build(cfg, sd, 'fp32')
    _, _, maps = net.attention_maps(rgb.cuda(), qm.cuda(), temporal=not joint, spatial_queries=queries)
    for i in range(DEPTH):
        for kind, got in (('temporal', maps.temporal.get(i)), ('spatial', maps.spatial[i])):
            if p64[i][kind] is None:
                assert got is None
                continue
            spread = float((p32[i][kind].double() - p64[i][kind]).abs().max())
            d = float((got.cpu().double() - p64[i][kind]).abs().max())
            print(f'ca={ca} joint={joint} block {i} {kind}: max|d| {d:.3e}, oracle f32 spread {spread:.3e}, ratio {d / max(spread, 1e-30):.2f}')
            assert spread > 0 and d <= 4 * spread + 1e-7, (ca, joint, i, kind, d, spread)


# ---------------------------------------------------------------------------------------------------------------------------------- refusals

def test_refusals_launch_nothing(cuda, monkeypatch):
    from tcow_amd import engine, ops
    cfg, sd, rgb, qm = case(2)
    net = build(cfg, sd, 'bf16')
    launched = []
    monkeypatch.setattr(engine, 'run_forward', lambda *a, **k: launched.append('run_forward'))
    monkeypatch.setattr(ops, 'attn_probs', lambda *a, **k: launched.append('attn_probs'))
    r, q = rgb.cuda(), qm.cuda()
    with pytest.raises(TcowError, match='training mode'):
        net.train().attention_maps(r, q)
    net.eval()
    with pytest.raises(TcowError, match='runs on the GPU only'):
        build_hip_seeker(cfg, sd, 'bf16').eval().attention_maps(rgb, qm)           # a CPU module
    with pytest.raises(TcowError, match='runs on the GPU only'):
        net.attention_maps(rgb, qm)                                                # CPU inputs
    with pytest.raises(TcowError, match=r'query \(1, 0\): slot 0 takes no part in spatial attention with causal_attention=2'):
        net.attention_maps(r, q, spatial_queries=[(1, 0)])
    with pytest.raises(TcowError, match=f'frame {T} is out of range'):
        net.attention_maps(r, q, spatial_queries=[(T, 1)])
    with pytest.raises(TcowError, match=r'take \d+ bytes .* over max_bytes = 1'):
        net.attention_maps(r, q, max_bytes=1)
    net.seeker.forced_drop_masks = {}
    with pytest.raises(TcowError, match='forced_drop_masks'):
        net.attention_maps(r, q)
    net.seeker.forced_drop_masks = None
    jcfg, jsd, _, _ = case(0, joint=True)
    with pytest.raises(TcowError, match="temporal=True with attention_type='joint_space_time'"):
        build(jcfg, jsd, 'bf16').attention_maps(r, q)
    assert launched == []

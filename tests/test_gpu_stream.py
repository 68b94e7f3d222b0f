"""GPU: streaming inference (Seeker.stream, tcow_amd/stream.py) -- the cached temporal-attention and cls kernels against torch restatements,
and streamed outputs, for every split of the clip into chunks, against the reference goldens, the clip forward and the oracle."""
import numpy as np
import pytest
import torch

from conftest import build_hip_seeker, golden_inputs, load_golden
from stream_kit import PRECISIONS, _check_vs, _splits, _stream, f64_cached_attention
from test_gpu_seeker import EXACT, TRAINED_REL, bf16_flags_tol, h16, h16f
from test_oracle_golden import summarise
from tcow_amd import ops, synth
from tcow_amd._lib import TcowError

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------- kernels

def _attn_case(mode, B, c, S, heads, T_total, t0, causal, seed):
    dev = torch.device('cuda')
    D = heads * 64
    dt = ops.tdtype(mode)
    g = torch.Generator(device=dev).manual_seed(seed)
    qkv = torch.randn(B * c * S, 3 * D, device=dev, generator=g).to(dt)
    kc = torch.randn(B, S - 1, heads, T_total, 64, device=dev, generator=g).to(dt)
    vc = torch.randn(B, S - 1, heads, T_total, 64, device=dev, generator=g).to(dt)
    kc0, vc0 = kc.clone(), vc.clone()
    out = torch.full((B * c * S, D), float('nan'), device=dev).to(dt)
    t0_dev = torch.tensor([t0], dtype=torch.int32, device=dev)
    ops.attn_temporal_cached(ops.F32X3 if mode == 'x3' else mode, B, c, S, D, heads, causal, T_total, t0_dev, qkv, kc, vc, out)
    ref, V = f64_cached_attention(qkv, kc0, vc0, B, c, S, heads, t0)              # on the same (rounded) inputs
    got = out.view(B, c, S, heads, 64)[:, :, 1:].permute(0, 2, 3, 1, 4).double()
    err = float((got - ref).abs().max())
    if dt == torch.float32:
        assert err <= 2e-6 * float(ref.abs().max()), (B, c, S, heads, T_total, t0, causal, err)
    else:
        vmax = float(V.abs().max())
        assert err <= ((2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11) + 1e-5) * vmax, (mode, B, c, S, heads, T_total, t0, causal, err)
    assert bool((out.view(B, c, S, D)[:, :, 0] == 0).all())                                        # slot-0 rows: exactly zero
    ck = lambda x: x.view(B, c, S, heads, 64)[:, :, 1:].permute(0, 2, 3, 1, 4)
    assert torch.equal(kc[..., t0:t0 + c, :], ck(qkv[:, D:2 * D])) and torch.equal(vc[..., t0:t0 + c, :], ck(qkv[:, 2 * D:]))   # appended bit for bit
    assert torch.equal(kc[..., :t0, :], kc0[..., :t0, :]) and torch.equal(kc[..., t0 + c:, :], kc0[..., t0 + c:, :])              # nothing else touched
    assert torch.equal(vc[..., :t0, :], vc0[..., :t0, :]) and torch.equal(vc[..., t0 + c:, :], vc0[..., t0 + c:, :])


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'fp16'])
def test_cached_temporal_attention_vs_f64(cuda, mode):
    m = {'f32': ops.F32, 'bf16': ops.BF16, 'fp16': ops.FP16}[mode]
    seed = 0
    for T_total in (4, 30, 60, 70):
        for c in (1, 3):
            for t0 in sorted({0, 1, 5, T_total - c}):
                if t0 + c > T_total:
                    continue
                for S in (2, 17, 301):
                    for B in (1, 2):
                        for heads in (1, 12):
                            for causal in (1, 2):
                                seed += 1
                                _attn_case(m, B, c, S, heads, T_total, t0, causal, seed)


def test_cached_temporal_attention_bf16x3_mode_stores_f32(cuda):
    _attn_case('x3', 2, 3, 17, 2, 30, 5, 1, 99)


def test_cached_temporal_attention_refuses_bad_arguments(cuda):
    dev = torch.device('cuda')
    B, c, S, heads, T = 1, 1, 5, 1, 8
    qkv = torch.zeros(B * c * S, 192, device=dev); kc = torch.zeros(B, S - 1, heads, T, 64, device=dev); out = torch.zeros(B * c * S, 64, device=dev)
    t0 = torch.zeros(1, dtype=torch.int32, device=dev)
    for causal in (0, 3, -1):
        with pytest.raises(TcowError, match='causal'):
            ops.attn_temporal_cached(ops.F32, B, c, S, 64, heads, causal, T, t0, qkv, kc, kc.clone(), out)
    with pytest.raises(TcowError, match='T_total'):
        ops.attn_temporal_cached(ops.F32, B, c, S, 64, heads, 1, 4096, t0, qkv, kc, kc.clone(), out)
    with pytest.raises(TcowError, match='head_dim'):
        ops.attn_temporal_cached(ops.F32, B, c, S, 96, heads, 1, T, t0, qkv, kc, kc.clone(), out)


def test_cls_stream_vs_torch(cuda):
    dev = torch.device('cuda')
    B, c, S, D = 3, 2, 5, 128
    x = torch.randn(B * c * S, D, device=dev)
    cache = torch.randn(B, D, device=dev)
    t0 = torch.zeros(1, dtype=torch.int32, device=dev)
    ref = x.clone().view(B, c, S, D)
    ref[:, :, 0] = ref[:, 0:1, 0]
    y = x.clone()
    ops.cls_stream(y, B, c, S, cache, t0)
    assert torch.equal(y.view(B, c, S, D), ref) and torch.equal(cache, ref[:, 0, 0])                # t0 == 0: merge (mode 1) and keep
    cache2 = torch.randn(B, D, device=dev)
    t0.fill_(3)
    y = x.clone()
    ops.cls_stream(y, B, c, S, cache2, t0)
    ref = x.clone().view(B, c, S, D)
    ref[:, :, 0] = cache2[:, None]
    assert torch.equal(y.view(B, c, S, D), ref)                                                          # t0 > 0: broadcast the kept row


# ---------------------------------------------------------------------------------------------- streams vs goldens / clip forward

@pytest.mark.parametrize('name', ['g1_cfg1_d256', 'g2_ca2', 'g2_normemb_nearest', 'g2_stride1_prenorm', 'g2_stride2', 'g11_depth18', 'g11_depth24',
                                  'g17_resize_a'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_stream_vs_reference_golden_and_clip_forward(cuda, name, precision):
    meta, g = load_golden(name)
    cfg, sd, rgb, qm = golden_inputs(meta)
    net = build_hip_seeker(cfg, sd, precision)
    if name.startswith('g17'):
        from test_oracle_golden import resize_tables
        pos, te = resize_tables(meta)
        net.seeker.vit.pos_embed = torch.nn.Parameter(torch.from_numpy(pos.copy()))
        net.seeker.vit.time_embed = torch.nn.Parameter(torch.from_numpy(te.copy()))
    net = net.cuda().eval()
    rgb, qm = rgb.cuda(), qm.cuda()
    T = cfg['num_total_frames']
    with torch.no_grad():
        clip_m, clip_f = net(rgb, qm)
    for split in ([1] * T, _splits(T, [2, 1, 1])):
        om, fl = _stream(net, rgb, qm, split)
        assert om.dtype == torch.float32 and om.shape == clip_m.shape and fl.shape == clip_f.shape
        gm, gf = torch.from_numpy(g['output_mask']).cuda(), torch.from_numpy(g['output_flags']).cuda()
        _check_vs(om, fl, gm, gf, precision, g['output_mask'], g['output_flags'])
        _check_vs(om, fl, clip_m, clip_f, precision, g['output_mask'], g['output_flags'])


@pytest.mark.parametrize('precision', PRECISIONS)
def test_stream_full_size_configs1_frame_by_frame(cuda, precision):
    meta, g = load_golden('g4_cfg2_T30_240x320')
    cfg, sd, rgb, qm = golden_inputs(meta)
    net = build_hip_seeker(cfg, sd, precision).cuda().eval()
    om, fl = _stream(net, rgb.cuda(), qm.cuda(), [1] * 30)
    pooled, fsum, fmax = summarise(om.cpu())
    d = np.abs(pooled - g['pooled']).max(); df = np.abs(fl.cpu().numpy() - g['output_flags']).max()
    if precision in EXACT:
        assert d < EXACT[precision] and df < EXACT[precision] and np.abs(fmax - g['frame_absmax']).max() < EXACT[precision]
        assert np.abs(fsum - g['frame_sum']).max() < 0.5
    else:
        assert d < h16(precision) * 0.05 * float(g['logit_std']) and df < h16f(precision) * bf16_flags_tol(g['output_flags'])
        if precision == 'fp16':
            assert d < 1e-3


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_stream_config3_long_clip_in_chunks_of_4(cuda, precision):
    meta, g = load_golden('g8_cfg3_long')
    cfg, sd, rgb, qm = golden_inputs(meta)
    net = build_hip_seeker(cfg, sd, precision).cuda().eval()
    om, fl = _stream(net, rgb.cuda(), qm.cuda(), [4] * 15)
    assert tuple(om.shape) == (1, 3, 60, 480, 640) and bool(torch.isfinite(om).all())
    pooled, fsum, fmax = summarise(om.cpu())
    pooled = pooled.reshape(60, 3, 120, 160)[g['frames']]
    d = np.abs(pooled - g['pooled_frames']).max(); df = np.abs(fl.cpu().numpy() - g['output_flags']).max()
    if precision in EXACT:
        assert d < EXACT[precision] and df < EXACT[precision] and np.abs(fmax - g['frame_absmax']).max() < EXACT[precision]
    else:
        assert d < h16(precision) * 0.05 * float(g['logit_std']) and df < h16f(precision) * bf16_flags_tol(g['output_flags'])
    assert abs(float((om > 0).float().mean()) - float(g['positive_frac'])) < {'fp32': 1e-5}.get(precision, 5e-3)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_stream_at_trained_checkpoint_logit_scale(cuda, precision):
    from test_gpu_seeker import TRAINED_AGREE
    from test_oracle_golden import mask_bits, trained_scale_inputs
    meta, g = load_golden('g16_cfg2_trained_scale')
    cfg, sd, rgb, qm = trained_scale_inputs(meta)
    net = build_hip_seeker(cfg, sd, precision).cuda().eval()
    om, _ = _stream(net, rgb.cuda(), qm.cuda(), [1] * 30)
    om = om.cpu()
    std = float(g['logit_std'])
    pooled, _, _ = summarise(om)
    d = float(np.abs(pooled - g['pooled']).max())
    agree = 1.0 - float(np.unpackbits(mask_bits(om.numpy(), meta['mask_frames']) ^ g['mask_bits']).mean())
    assert np.isfinite(om.numpy()).all()
    assert d < TRAINED_REL[precision] * std, (d, std)
    assert agree >= TRAINED_AGREE[precision], agree


@pytest.mark.parametrize('seed', list(range(16)))
def test_stream_random_geometries_vs_oracle(cuda, seed):
    """test_random_geometries_vs_oracle with causal_attention in {1, 2} and a random chunk split per seed: single-frame chunks, one-patch
    frames, S = 2 and ragged tiles, streamed."""
    from oracle import seeker_oracle as so
    rng = np.random.default_rng(5000 + seed)
    T = int(rng.integers(1, 10)); Hp = int(rng.integers(1, 6)); Wp = int(rng.integers(1, 7)); D = int(rng.choice([64, 128, 192]))
    st = int(rng.choice([1, 2, 4]))
    cfg = synth.seeker_config(num_total_frames=T, frame_height=16 * Hp, frame_width=16 * Wp, embed_dim=D, depth=int(rng.integers(1, 4)), num_heads=D // 64,
                              causal_attention=int(rng.choice([1, 2])), norm_embeddings=bool(rng.integers(0, 2)), track_map_stride=st,
                              track_map_resize=str(rng.choice(['bilinear', 'nearest'])), pretrained_norm=bool(rng.integers(0, 2)))
    sd = synth.make_state_dict(cfg, 6000 + seed)
    B = int(rng.integers(1, 4))
    clip = synth.make_clip(B, T, 16 * Hp, 16 * Wp, seed=7000 + seed)
    rgb = torch.from_numpy(clip['rgb']); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0))
    if qm.shape[0] != B:
        qm = qm.expand(B, -1, -1, -1, -1).contiguous()
    split, n = [], 0
    while n < T:
        c = int(rng.integers(1, T - n + 1)); split.append(c); n += c
    with torch.no_grad():
        om_r, fl_r = so.seeker_forward(so.to_torch_state_dict(sd), cfg, rgb, qm)
    std = float(om_r.std()) + 1e-6 if om_r.numel() > 1 else 1.0
    fstd = float(fl_r.std()) + 1e-6 if fl_r.numel() > 1 else 1.0
    for precision, tol, ftol in (('fp32', 1e-5, 1e-5), ('fp16', 0.00625 * std + 1e-5, 0.0015 * fstd + 2e-5), ('bf16', 0.05 * std + 1e-4, 0.012 * fstd + 2e-4)):
        net = build_hip_seeker(cfg, sd, precision).cuda().eval()
        om, fl = _stream(net, rgb.cuda(), qm.cuda(), split)
        assert float((om.cpu() - om_r).abs().max()) < tol, (precision, cfg, split)
        assert float((fl.cpu() - fl_r).abs().max()) < ftol, (precision, cfg, split)


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-5), ('bf16', 1.5e-2)])
def test_stream_shared_rgb_and_batched_clips(cuda, precision, tol):
    cfg = synth.seeker_config(num_total_frames=4, frame_height=64, frame_width=96, embed_dim=256, depth=2, num_heads=4, causal_attention=1)
    net = build_hip_seeker(cfg, synth.make_state_dict(cfg, 11), precision).cuda().eval()
    clip = synth.make_clip(2, 4, 64, 96, seed=5)
    rgb = torch.from_numpy(clip['rgb']).cuda()
    qms = [torch.from_numpy(synth.make_query_mask(clip, q, 0)).cuda() for q in range(3)]          # each (2, 1, T, H, W)
    # one clip, three queries sharing its frames == three one-query streams
    qm3 = torch.cat([q[0:1] for q in qms], 0)
    om, fl = _stream(net, rgb[0:1], qm3, [2, 1, 1], Qs=3)
    for k in range(3):
        o1, f1 = _stream(net, rgb[0:1], qms[k][0:1], [1, 1, 1, 1])
        assert float((om[k:k + 1] - o1).abs().max()) < tol and float((fl[k:k + 1] - f1).abs().max()) < tol
    assert float((om[0] - om[1]).abs().max()) > 0
    # two clips in one stream == two one-clip streams
    om2, fl2 = _stream(net, rgb, qms[0], [1, 3])
    for b in range(2):
        o1, f1 = _stream(net, rgb[b:b + 1], qms[0][b:b + 1], [1, 3])
        assert float((om2[b:b + 1] - o1).abs().max()) < tol and float((fl2[b:b + 1] - f1).abs().max()) < tol


@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'fp32'])
def test_stream_graph_mode_is_bit_identical_to_eager(cuda, precision):
    """(the split [1, 2, 1, 2] asks for the longer mask0 while the graph of c = 1 is live; two clips: time rows of B * c rows under capture)"""
    cfg = synth.seeker_config(num_total_frames=6, frame_height=32, frame_width=48, embed_dim=128, depth=2, num_heads=2, causal_attention=1)
    net = build_hip_seeker(cfg, synth.make_state_dict(cfg, 5), precision).cuda().eval()
    for clips, splits in ((1, ([1] * 6, [2, 1, 2, 1], [1, 2, 1, 2])), (2, ([2, 1, 2, 1],))):
        clip = synth.make_clip(clips, 6, 32, 48, seed=2)
        rgb = torch.from_numpy(clip['rgb']).cuda(); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
        for split in splits:
            eager = net.stream(batch_size=clips, graph=False); graph = net.stream(batch_size=clips, graph=True)
            for rep in range(2):                                # the second pass replays every captured chunk length
                eager.reset(); graph.reset()
                t = 0
                for c in split:
                    a = eager.step(rgb[:, :, t:t + c], qm[:, :, t:t + c])
                    b = graph.step(rgb[:, :, t:t + c], qm[:, :, t:t + c])
                    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (clips, split, rep, t)
                    t += c
            held = b[0].clone()
            c = split[-1]
            graph.reset(); graph.step(rgb[:, :, 0:c] * 0.5, qm[:, :, 0:c])
            assert torch.equal(b[0], held)                      # returned tensors are the caller's: the next replay does not overwrite them


def test_stream_lifecycle(cuda):
    cfg = synth.seeker_config(num_total_frames=4, frame_height=32, frame_width=48, embed_dim=128, depth=2, num_heads=2, causal_attention=1)
    net = build_hip_seeker(cfg, synth.make_state_dict(cfg, 9), 'bf16').cuda().eval()
    for p in net.parameters():
        p.requires_grad_(True)
    clip = synth.make_clip(1, 4, 32, 48, seed=4)
    rgb = torch.from_numpy(clip['rgb']).cuda(); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
    st = net.stream()
    first = [st.step(rgb[:, :, t:t + 1], qm[:, :, t:t + 1]) for t in range(4)]
    assert st.frames_done == 4
    assert not first[0][0].requires_grad and not first[0][1].requires_grad                  # grad mode does not leak into the outputs
    with pytest.raises(TcowError, match='past the last frame'):
        st.step(rgb[:, :, 0:1], qm[:, :, 0:1])
    st.reset()
    assert st.frames_done == 0
    again = [st.step(rgb[:, :, t:t + 1], qm[:, :, t:t + 1]) for t in range(4)]
    for (a, fa), (b, fb) in zip(first, again):
        assert torch.equal(a, b) and torch.equal(fa, fb)
    # query_mask=None == explicit zeros
    st.reset(); z = st.step(rgb[:, :, 0:2], None)
    st.reset(); e = st.step(rgb[:, :, 0:2], torch.zeros_like(qm[:, :, 0:2]))
    assert torch.equal(z[0], e[0]) and torch.equal(z[1], e[1])
    # wrong shapes / devices
    with pytest.raises(TcowError, match='rgb'):
        st.step(rgb[:, :2, 0:1], None)
    with pytest.raises(TcowError, match='query_mask'):
        st.step(rgb[:, :, 2:3], qm[:, :, 2:4])
    with pytest.raises(TcowError, match='device'):
        st.step(rgb[:, :, 2:3].cpu(), None)
    # a parameter change mid-stream invalidates the cache
    st.reset(); st.step(rgb[:, :, 0:1], qm[:, :, 0:1])
    with torch.no_grad():
        net.seeker.vit.blocks[0].mlp.fc1.bias.add_(0.01)
    with pytest.raises(TcowError, match='changed'):
        st.step(rgb[:, :, 1:2], qm[:, :, 1:2])
    fresh = net.stream()                                        # a stream opened on the new weights runs
    assert torch.isfinite(fresh.step(rgb[:, :, 0:1], qm[:, :, 0:1])[0]).all()
    net.load_state_dict(net.state_dict())                       # load_state_dict writes every parameter
    with pytest.raises(TcowError, match='changed'):
        fresh.step(rgb[:, :, 1:2], qm[:, :, 1:2])
    # leaving eval mode mid-stream
    st2 = net.stream()
    net.train()
    with pytest.raises(TcowError, match='training'):
        st2.step(rgb[:, :, 0:1], None)
    net.eval()


def _recycle_freed_blocks(net):
    """Allocate NaN-filled tensors of every parameter's size in f32 and 16-bit, so that device blocks the caching allocator got back
    (replaced operand copies) hold garbage if anything still reads them."""
    junk = []
    for p in net.parameters():
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            junk.append(torch.full(p.shape, float('nan'), dtype=dt, device=p.device))
    junk.append(torch.full((1 << 20,), float('nan'), device='cuda'))
    return junk


@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_stream_graph_mode_survives_replaced_operand_copies(cuda, precision):
    """An idempotent .cuda(), set_precision() with the same precision and a train-mode forward replace the module's operand copies without
    changing a parameter, and a longer pool step replaces the mask0 all stream steps share: the stream stays valid, and graph steps after
    each of them still equal the eager stream."""
    cfg = synth.seeker_config(num_total_frames=6, frame_height=32, frame_width=48, embed_dim=128, depth=2, num_heads=2, causal_attention=1)
    net = build_hip_seeker(cfg, synth.make_state_dict(cfg, 8), precision).cuda().eval()
    clip = synth.make_clip(1, 6, 32, 48, seed=3)
    rgb = torch.from_numpy(clip['rgb']).cuda(); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
    eager, graph = net.stream(graph=False), net.stream(graph=True)

    def cuda_again():
        net.cuda()

    def same_precision():
        net.seeker.set_precision(precision)

    def train_forward():
        net.train()
        net(rgb, qm)                                            # gradients enabled: the forward builds operand copies for a backward
        net.eval()

    def longer_pool_step():
        pool = net.stream_pool(1)                               # four frames in one ragged step: a longer shared mask0 replaces the captured one
        pool.step_ragged([pool.open()], [rgb[:, :, 0:4]], [qm[:, :, 0:4]])

    events = {2: cuda_again, 3: same_precision, 4: train_forward, 5: longer_pool_step}
    junk = []
    for t in range(6):
        if t in events:
            events[t]()
            junk += _recycle_freed_blocks(net)
        a = eager.step(rgb[:, :, t:t + 1], qm[:, :, t:t + 1])
        b = graph.step(rgb[:, :, t:t + 1], qm[:, :, t:t + 1])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), t
    graph.reset(); eager.reset()                                # and once more as plain replays
    for t in range(6):
        a = eager.step(rgb[:, :, t:t + 1], qm[:, :, t:t + 1])
        b = graph.step(rgb[:, :, t:t + 1], qm[:, :, t:t + 1])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), t


def test_stream_step_before_clip_forward_leaves_the_clip_path_alone(cuda):
    """A stream step builds the chunk's row vectors (mask0 of B*c*S rows) before any clip forward ran: the clip forward that follows must
    use its own B*T*S rows, bit-identical to a module that never streamed."""
    cfg = synth.seeker_config(num_total_frames=5, frame_height=32, frame_width=48, embed_dim=128, depth=2, num_heads=2, causal_attention=2)
    sd = synth.make_state_dict(cfg, 12)
    clip = synth.make_clip(2, 5, 32, 48, seed=6)
    rgb = torch.from_numpy(clip['rgb']).cuda(); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
    streamed = build_hip_seeker(cfg, sd, 'bf16').cuda().eval()
    fresh = build_hip_seeker(cfg, sd, 'bf16').cuda().eval()
    st = streamed.stream(batch_size=2)
    st.step(rgb[:, :, 0:1], qm[:, :, 0:1])
    with torch.no_grad():
        a, fa = streamed(rgb, qm)
        b, fb = fresh(rgb, qm)
    assert torch.equal(a, b) and torch.equal(fa, fb)

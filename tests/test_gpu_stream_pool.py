"""GPU: a pool of live sessions at different frames (Seeker.stream_pool, tcow_amd/stream.py) -- the pool kernels against the stream kernels
row by row (bit for bit) and against torch restatements, and pooled sessions against the reference goldens, the clip forward, the oracle and
one-session streams."""
import numpy as np
import pytest
import torch

from conftest import build_hip_seeker, golden_inputs, load_golden
from stream_kit import MODES, PRECISIONS, _cat, _check_vs, _pool_step, _small_clips, _small_net, _stream, f64_cached_attention
from tcow_amd import ops, synth
from tcow_amd._lib import TcowError

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------- kernels

def _slots_and_t0(n, c, T_total, n_slots, rng):
    """slot_rows: a non-identity injection of the rows into the slots (where one exists); t0_rows: 0 and T_total - c, distinct values otherwise
    while the range has any left, in a random order."""
    while True:
        slots = [int(v) for v in rng.permutation(n_slots)[:n]]
        if slots != list(range(n)) or n_slots == 1:
            break
    t0 = [0, T_total - c][:n] if n > 1 else [T_total - c]
    rest = [t for t in range(T_total - c + 1) if t not in t0]
    rng.shuffle(rest)
    while len(t0) < n:
        t0.append(int(rest.pop()) if rest else T_total - c)
    order = rng.permutation(n)
    return slots, [t0[i] for i in order]


def _pool_case(mode_name, n, c, S, heads, T_total, n_slots, causal, seed, t0_rows=None):
    dev = torch.device('cuda')
    mode = MODES[mode_name]
    D = heads * 64
    dt = ops.tdtype(ops.F32 if mode == ops.F32X3 else mode)
    rng = np.random.default_rng(seed)
    slots, t0s = _slots_and_t0(n, c, T_total, n_slots, rng)
    if t0_rows is not None:
        t0s = list(t0_rows)
    g = torch.Generator(device=dev).manual_seed(seed)
    qkv = torch.randn(n * c * S, 3 * D, device=dev, generator=g).to(dt)
    kc0 = torch.randn(n_slots, S - 1, heads, T_total, 64, device=dev, generator=g).to(dt)
    vc0 = torch.randn(n_slots, S - 1, heads, T_total, 64, device=dev, generator=g).to(dt)
    kc, vc = kc0.clone(), vc0.clone()
    out = torch.full((n * c * S, D), float('nan'), device=dev).to(dt)
    ops.attn_temporal_pool(mode, n, c, S, D, heads, causal, T_total, n_slots, torch.tensor(t0s, dtype=torch.int32, device=dev),
                           torch.tensor(slots, dtype=torch.int32, device=dev), qkv, kc, vc, out)
    # n launches of the stream kernel: one row's qkv block, the contiguous one-slot view of a copy of the caches, that row's t0
    kc_r, vc_r = kc0.clone(), vc0.clone()
    out_r = torch.full((n * c * S, D), float('nan'), device=dev).to(dt)
    R = c * S
    for r in range(n):
        sl = slots[r]
        ops.attn_temporal_cached(mode, 1, c, S, D, heads, causal, T_total, torch.tensor([t0s[r]], dtype=torch.int32, device=dev), qkv[r * R:(r + 1) * R],
                                 kc_r[sl:sl + 1], vc_r[sl:sl + 1], out_r[r * R:(r + 1) * R])
    tag = (mode_name, n, c, S, heads, T_total, n_slots, causal, slots, t0s)
    assert torch.equal(out, out_r), tag
    assert torch.equal(kc, kc_r) and torch.equal(vc, vc_r), tag                       # the whole tensors: unnamed slots bit-unchanged
    for r in range(n):
        ref, V = (x[0] for x in f64_cached_attention(qkv[r * R:(r + 1) * R], kc0[slots[r]][None], vc0[slots[r]][None], 1, c, S, heads, t0s[r]))
        got = out[r * R:(r + 1) * R].view(c, S, heads, 64)[:, 1:].permute(1, 2, 0, 3).double()
        err = float((got - ref).abs().max())
        print('pool kernel', tag, 'row', r, 'err', err)
        if dt == torch.float32:
            assert err <= 2e-6 * float(ref.abs().max()), (tag, r, err)
        else:
            assert err <= ((2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11) + 1e-5) * float(V.abs().max()), (tag, r, err)


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'fp16'])
def test_pool_attention_equals_the_stream_kernel_row_by_row(cuda, mode):
    seed = 0
    for n in (1, 3):
        for c in (1, 3):
            for S in (2, 17):
                for heads in (1, 2):
                    for T_total in (4, 30):
                        for n_slots in (n, n + 2):
                            seed += 1
                            _pool_case(mode, n, c, S, heads, T_total, n_slots, 1 + seed % 2, seed)
                            if n == 1:                          # one row cannot hold both ends of the range: the other end as a case of its own
                                _pool_case(mode, n, c, S, heads, T_total, n_slots, 1 + seed % 2, seed, t0_rows=[0])


def test_pool_attention_bf16x3_mode_stores_f32(cuda):
    _pool_case('x3', 3, 3, 17, 2, 30, 5, 1, 99)


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_pool_attention_real_grid(cuda, mode):
    _pool_case(mode, 2, 1, 301, 12, 30, 4, 1, 7)


def test_cls_pool_vs_torch(cuda):
    dev = torch.device('cuda')
    n, c, S, D, n_slots = 3, 2, 5, 128, 5
    t0s, slots = (0, 3, 0), (4, 0, 2)
    x = torch.randn(n * c * S, D, device=dev)
    cache0 = torch.randn(n_slots, D, device=dev)
    cache = cache0.clone()
    y = x.clone()
    ops.cls_pool(y, n, c, S, cache, n_slots, torch.tensor(t0s, dtype=torch.int32, device=dev), torch.tensor(slots, dtype=torch.int32, device=dev))
    ref = x.clone().view(n, c, S, D)
    ref_cache = cache0.clone()
    for r in range(n):
        if t0s[r] == 0:
            ref[r, :, 0] = ref[r, 0:1, 0]
            ref_cache[slots[r]] = ref[r, 0, 0]
        else:
            ref[r, :, 0] = cache0[slots[r]][None]
    assert torch.equal(y.view(n, c, S, D), ref)
    assert torch.equal(cache[4], x.view(n, c, S, D)[0, 0, 0]) and torch.equal(cache[2], x.view(n, c, S, D)[2, 0, 0])       # kept rows
    assert torch.equal(cache, ref_cache)                                                                                  # every other row unchanged


def test_pool_kernels_refuse_bad_arguments(cuda):
    dev = torch.device('cuda')
    n, c, S, heads, T, n_slots = 1, 1, 5, 1, 8, 2
    qkv = torch.zeros(n * c * S, 192, device=dev); kc = torch.zeros(n_slots, S - 1, heads, T, 64, device=dev); out = torch.zeros(n * c * S, 64, device=dev)
    t0 = torch.zeros(n, dtype=torch.int32, device=dev); sl = torch.zeros(n, dtype=torch.int32, device=dev)
    for causal in (0, 3, -1):
        with pytest.raises(TcowError, match='causal'):
            ops.attn_temporal_pool(ops.F32, n, c, S, 64, heads, causal, T, n_slots, t0, sl, qkv, kc, kc.clone(), out)
    with pytest.raises(TcowError, match='T_total'):
        ops.attn_temporal_pool(ops.F32, n, c, S, 64, heads, 1, 4096, n_slots, t0, sl, qkv, kc, kc.clone(), out)
    with pytest.raises(TcowError, match='head_dim'):
        ops.attn_temporal_pool(ops.F32, n, c, S, 96, heads, 1, T, n_slots, t0, sl, qkv, kc, kc.clone(), out)
    for bad in (0, -1):
        with pytest.raises(TcowError, match='n_slots'):
            ops.attn_temporal_pool(ops.F32, n, c, S, 64, heads, 1, T, bad, t0, sl, qkv, kc, kc.clone(), out)
        with pytest.raises(TcowError, match='tcow_cls_step: n_slots'):
            ops.cls_pool(torch.zeros(n * c * S, 64, device=dev), n, c, S, torch.zeros(n_slots, 64, device=dev), bad, t0, sl)
    with pytest.raises(TcowError, match='CUDA'):
        ops.attn_temporal_pool(ops.F32, n, c, S, 64, heads, 1, T, n_slots, t0.cpu(), sl, qkv, kc, kc.clone(), out)


# ---------------------------------------------------------------------------------------------- pooled sessions

@pytest.mark.parametrize('name', ['g1_cfg1_d256', 'g2_ca2'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_pool_vs_reference_golden_and_clip_forward(cuda, name, precision):
    meta, g = load_golden(name)
    cfg, sd, rgb, qm = golden_inputs(meta)
    net = build_hip_seeker(cfg, sd, precision).cuda().eval()
    rgb, qm = rgb.cuda(), qm.cuda()
    B, T = rgb.shape[0], cfg['num_total_frames']
    rgb_l, qm_l = rgb[0:1].flip(2).contiguous(), qm[0:1].flip(2).contiguous()             # the lead: row 0's clip, frames in reverse order
    with torch.no_grad():
        clip_m, clip_f = net(rgb, qm)
        lead_m, lead_f = net(rgb_l, qm_l)
    pool = net.stream_pool(B + 1)
    lead = pool.open()
    sess, got = [], {lead: []}
    for step in range(T + 2):
        if step == 2:
            sess = [pool.open() for _ in range(B)]
            got.update({i: [] for i in sess})
        feeds = [(lead, rgb_l, qm_l)] if step < T else []
        if step >= 2:
            feeds += [(i, rgb[b:b + 1], qm[b:b + 1]) for b, i in enumerate(sess)]
        for i, o in (_pool_step(pool, feeds) if feeds else {}).items():
            got[i].append(o)
        if step == T - 1:
            assert pool.frames_done(lead) == T
            pool.close(lead)
    om, fl = (torch.cat(x, 0) for x in zip(*[_cat(got[i]) for i in sess]))
    assert om.shape == clip_m.shape and fl.shape == clip_f.shape
    gm, gf = torch.from_numpy(g['output_mask']).cuda(), torch.from_numpy(g['output_flags']).cuda()
    _check_vs(om, fl, gm, gf, precision, g['output_mask'], g['output_flags'])
    _check_vs(om, fl, clip_m, clip_f, precision, g['output_mask'], g['output_flags'])
    lm, lf = _cat(got[lead])
    _check_vs(lm, lf, lead_m, lead_f, precision, g['output_mask'], g['output_flags'])


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-5), ('bf16', 1.5e-2)])
def test_pool_slot_reuse_reads_nothing_of_the_previous_tenant(cuda, precision, tol):
    net = _small_net(precision)
    clips = _small_clips(4)
    want = [_stream(net, r, q, [1, 1, 1, 1]) for r, q in clips]
    pool = net.stream_pool(3)                                   # three slots: the newcomer can only get the slot the lead leaves
    lead = pool.open()
    got = {lead: []}
    for _ in range(2):
        got[lead].append(_pool_step(pool, [(lead, *clips[0])])[lead])
    a, b = pool.open(), pool.open()
    got.update({a: [], b: []})
    with pytest.raises(TcowError, match='slots are taken'):
        pool.open()
    for _ in range(2):
        for i, o in _pool_step(pool, [(a, *clips[1]), (lead, *clips[0]), (b, *clips[2])]).items():
            got[i].append(o)
    pool.close(lead)
    new = pool.open()                                           # the lead's slot: its K / V rows 0..3 and its cls rows are still there
    got[new] = []
    for _ in range(2):
        for i, o in _pool_step(pool, [(new, *clips[3]), (a, *clips[1]), (b, *clips[2])]).items():
            got[i].append(o)
    pool.close(a); pool.close(b)
    for _ in range(2):
        got[new].append(_pool_step(pool, [(new, *clips[3])])[new])
    for i, k in ((lead, 0), (a, 1), (b, 2), (new, 3)):
        om, fl = _cat(got[i])
        d, df = float((om - want[k][0]).abs().max()), float((fl - want[k][1]).abs().max())
        print('slot reuse', precision, 'clip', k, d, df)
        assert d < tol and df < tol, (k, d, df)
    assert float((want[3][0] - want[0][0]).abs().max()) > tol               # the two tenants' outputs differ by more than the tolerance


@pytest.mark.parametrize('seed', list(range(8)))
def test_pool_random_geometries_vs_oracle(cuda, seed):
    """test_stream_random_geometries_vs_oracle with each clip of the batch a session of its own, delayed by a random number of pool steps, and a
    random common chunk length per step."""
    from oracle import seeker_oracle as so
    rng = np.random.default_rng(5000 + seed)
    T = int(rng.integers(1, 10)); Hp = int(rng.integers(1, 6)); Wp = int(rng.integers(1, 7)); D = int(rng.choice([64, 128, 192]))
    st = int(rng.choice([1, 2, 4]))
    cfg = synth.seeker_config(num_total_frames=T, frame_height=16 * Hp, frame_width=16 * Wp, embed_dim=D, depth=int(rng.integers(1, 4)), num_heads=D // 64,
                              causal_attention=int(rng.choice([1, 2])), norm_embeddings=bool(rng.integers(0, 2)), track_map_stride=st,
                              track_map_resize=str(rng.choice(['bilinear', 'nearest'])), pretrained_norm=bool(rng.integers(0, 2)))
    sd = synth.make_state_dict(cfg, 6000 + seed)
    B = int(rng.integers(2, 4))
    clip = synth.make_clip(B, T, 16 * Hp, 16 * Wp, seed=7000 + seed)
    rgb = torch.from_numpy(clip['rgb']); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0))
    if qm.shape[0] != B:
        qm = qm.expand(B, -1, -1, -1, -1).contiguous()
    delay = [int(rng.integers(0, 4)) for _ in range(B)]
    plan, done, step = [], [0] * B, 0                            # per pool step: (rows that take part, common c)
    while min(done) < T:
        rows = [b for b in range(B) if delay[b] <= step and done[b] < T]
        if rows:
            c = int(rng.integers(1, min(T - done[b] for b in rows) + 1))
            plan.append((rows, c))
            for b in rows:
                done[b] += c
        step += 1
    with torch.no_grad():
        om_r, fl_r = so.seeker_forward(so.to_torch_state_dict(sd), cfg, rgb, qm)
    std = float(om_r.std()) + 1e-6 if om_r.numel() > 1 else 1.0
    fstd = float(fl_r.std()) + 1e-6 if fl_r.numel() > 1 else 1.0
    rgb_d, qm_d = rgb.cuda(), qm.cuda()
    for precision, tol, ftol in (('fp32', 1e-5, 1e-5), ('fp16', 0.00625 * std + 1e-5, 0.0015 * fstd + 2e-5), ('bf16', 0.05 * std + 1e-4, 0.012 * fstd + 2e-4)):
        net = build_hip_seeker(cfg, sd, precision).cuda().eval()
        pool = net.stream_pool(B)
        ids, got = {}, {b: [] for b in range(B)}
        for rows, c in plan:
            for b in rows:
                if b not in ids:
                    ids[b] = pool.open()
            out = _pool_step(pool, [(ids[b], rgb_d[b:b + 1], qm_d[b:b + 1]) for b in rows], c)
            for b in rows:
                got[b].append(out[ids[b]])
        om, fl = (torch.cat(x, 0) for x in zip(*[_cat(got[b]) for b in range(B)]))
        d, df = float((om.cpu() - om_r).abs().max()), float((fl.cpu() - fl_r).abs().max())
        print('pool oracle', seed, precision, d, tol, df, ftol)
        assert d < tol, (precision, cfg, plan, delay)
        assert df < ftol, (precision, cfg, plan, delay)


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-5), ('bf16', 1.5e-2)])
def test_pool_order_and_chunking(cuda, precision, tol):
    net = _small_net(precision)
    clips = _small_clips(3)

    def phased():
        """A pool with three sessions at frames 2, 1, 0."""
        pool = net.stream_pool(4)
        ids = [pool.open() for _ in range(3)]
        _pool_step(pool, [(ids[0], *clips[0])])
        _pool_step(pool, [(ids[0], *clips[0]), (ids[1], *clips[1])])
        return pool, ids

    p1, i1 = phased()
    p2, i2 = phased()
    a = _pool_step(p1, [(i1[k], *clips[k]) for k in (0, 1, 2)])
    b = _pool_step(p2, [(i2[k], *clips[k]) for k in (2, 0, 1)])                 # ids and input rows permuted together
    for k in range(3):
        assert torch.equal(a[i1[k]][0], b[i2[k]][0]) and torch.equal(a[i1[k]][1], b[i2[k]][1]), k
    # one session fed [2, 1, 1] == the same session fed [1, 1, 1, 1], each next to a session at another phase
    outs = []
    for split in ([2, 1, 1], [1, 1, 1, 1]):
        pool = net.stream_pool(2)
        other, me = pool.open(), pool.open()
        _pool_step(pool, [(other, *clips[1])])
        parts = []
        for c in split:
            feeds = [(me, *clips[0])] + ([(other, *clips[1])] if pool.frames_done(other) + c <= 4 else [])
            parts.append(_pool_step(pool, feeds, c)[me])
        outs.append(_cat(parts))
    d, df = float((outs[0][0] - outs[1][0]).abs().max()), float((outs[0][1] - outs[1][1]).abs().max())
    print('pool chunking', precision, d, df)
    assert d < tol and df < tol, (d, df)


def test_pool_lifecycle(cuda):
    cfg = synth.seeker_config(num_total_frames=4, frame_height=32, frame_width=48, embed_dim=128, depth=2, num_heads=2, causal_attention=1)
    net = build_hip_seeker(cfg, synth.make_state_dict(cfg, 9), 'bf16').cuda().eval()
    for p in net.parameters():
        p.requires_grad_(True)
    clip = synth.make_clip(2, 4, 32, 48, seed=4)
    rgb = torch.from_numpy(clip['rgb']).cuda(); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
    pool = net.stream_pool(2)
    assert pool.cache_bytes == 2 * net.stream().cache_bytes and net.seeker.stream_pool(3).cache_bytes == 3 * net.stream().cache_bytes
    a, b = pool.open(), pool.open()
    assert a != b and pool.frames_done(a) == 0 and pool.frames_done(b) == 0
    with pytest.raises(TcowError, match='slots are taken'):
        pool.open()
    m0, f0 = pool.step([a], rgb[0:1, :, 0:1], qm[0:1, :, 0:1])
    assert not m0.requires_grad and not f0.requires_grad                                   # grad mode does not leak into the outputs
    assert pool.frames_done(a) == 1 and pool.frames_done(b) == 0
    # refused steps: nothing is launched, no counter moves
    both = lambda t_a, t_b, c: (torch.cat([rgb[0:1, :, t_a:t_a + c], rgb[1:2, :, t_b:t_b + c]], 0), torch.cat([qm[0:1, :, t_a:t_a + c], qm[1:2, :, t_b:t_b + c]], 0))
    r2, q2 = both(1, 0, 1)
    with pytest.raises(TcowError, match='duplicate'):
        pool.step([a, a], r2, q2)
    with pytest.raises(TcowError, match='not open'):
        pool.step([a, 12345], r2, q2)
    with pytest.raises(TcowError, match='rgb'):
        pool.step([a, b], r2[:, :2], q2)
    with pytest.raises(TcowError, match='rgb'):
        pool.step([a, b], r2[0:1], q2)
    with pytest.raises(TcowError, match='query_mask'):
        pool.step([a, b], r2, q2[0:1])
    with pytest.raises(TcowError, match='device'):
        pool.step([a, b], r2.cpu(), None)
    with pytest.raises(TcowError, match='1 .. capacity'):
        pool.step([], r2, q2)
    # one of two sessions would overrun: a is at frame 1, b at 0, four frames asked
    r4 = torch.cat([rgb[0:1], rgb[1:2]], 0); q4 = torch.cat([qm[0:1], qm[1:2]], 0)
    with pytest.raises(TcowError, match=f'session {a}'):
        pool.step([a, b], r4, q4)
    assert pool.frames_done(a) == 1 and pool.frames_done(b) == 0
    got = pool.step([a, b], r2, q2)
    ref_pool = net.stream_pool(2)                                                           # the same steps, the refused ones never sent
    ra, rb = ref_pool.open(), ref_pool.open()
    ref_pool.step([ra], rgb[0:1, :, 0:1], qm[0:1, :, 0:1])
    want = ref_pool.step([ra, rb], r2, q2)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert pool.frames_done(a) == 2 and pool.frames_done(b) == 1
    # query_mask=None == explicit zeros
    pool.reset(a); pool.reset(b)
    assert pool.frames_done(a) == 0 and pool.frames_done(b) == 0
    z = pool.step([a, b], rgb[:, :, 0:2], None)
    pool.reset(a); pool.reset(b)
    e = pool.step([a, b], rgb[:, :, 0:2], torch.zeros_like(qm[:, :, 0:2]))
    assert torch.equal(z[0], e[0]) and torch.equal(z[1], e[1])
    # reset(id) and close() / open() start at frame 0: the first frame again gives the first outputs again
    pool.reset(a)
    again = pool.step([a], rgb[0:1, :, 0:1], qm[0:1, :, 0:1])
    assert torch.equal(again[0], m0) and torch.equal(again[1], f0)
    pool.close(a)
    with pytest.raises(TcowError, match='not open'):
        pool.step([a], rgb[0:1, :, 1:2], qm[0:1, :, 1:2])
    with pytest.raises(TcowError, match='not open'):
        pool.frames_done(a)
    with pytest.raises(TcowError, match='not open'):
        pool.close(a)
    a2 = pool.open()
    assert a2 != a and pool.frames_done(a2) == 0
    again = pool.step([a2], rgb[0:1, :, 0:1], qm[0:1, :, 0:1])
    assert torch.equal(again[0], m0) and torch.equal(again[1], f0)
    # a parameter change invalidates the caches; leaving eval mode
    with torch.no_grad():
        net.seeker.vit.blocks[0].mlp.fc1.bias.add_(0.01)
    with pytest.raises(TcowError, match='changed'):
        pool.step([a2], rgb[0:1, :, 1:2], qm[0:1, :, 1:2])
    assert pool.frames_done(a2) == 1
    fresh = net.stream_pool(1)
    s = fresh.open()
    assert torch.isfinite(fresh.step([s], rgb[0:1, :, 0:1], qm[0:1, :, 0:1])[0]).all()
    net.train()
    with pytest.raises(TcowError, match='training'):
        fresh.step([s], rgb[0:1, :, 1:2], None)
    net.eval()


def test_pool_steps_leave_the_clip_path_and_streams_alone(cuda):
    """After pool steps on a module, its clip forward and a SeekerStream opened on it are bit-identical to those of a module that never pooled."""
    cfg = synth.seeker_config(num_total_frames=5, frame_height=32, frame_width=48, embed_dim=128, depth=2, num_heads=2, causal_attention=1)
    sd = synth.make_state_dict(cfg, 12)
    clip = synth.make_clip(2, 5, 32, 48, seed=6)
    rgb = torch.from_numpy(clip['rgb']).cuda(); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
    pooled = build_hip_seeker(cfg, sd, 'bf16').cuda().eval()
    fresh = build_hip_seeker(cfg, sd, 'bf16').cuda().eval()
    pool = pooled.stream_pool(2)
    a = pool.open()
    pool.step([a], rgb[0:1, :, 0:1], qm[0:1, :, 0:1])
    b = pool.open()
    pool.step([b, a], torch.cat([rgb[1:2, :, 0:1], rgb[0:1, :, 1:2]], 0), torch.cat([qm[1:2, :, 0:1], qm[0:1, :, 1:2]], 0))
    with torch.no_grad():
        x, fx = pooled(rgb, qm)
        y, fy = fresh(rgb, qm)
    assert torch.equal(x, y) and torch.equal(fx, fy)
    for split in ([1] * 5, [2, 3]):
        s1, f1 = _stream(pooled, rgb, qm, split)
        s2, f2 = _stream(fresh, rgb, qm, split)
        assert torch.equal(s1, s2) and torch.equal(f1, f2), split

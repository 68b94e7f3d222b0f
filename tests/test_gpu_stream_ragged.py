"""GPU: pool steps whose sessions bring different numbers of frames (SeekerStreamPool.step_ragged, tcow_amd/stream.py) -- the ragged kernels
against the pool kernels session by session (bit for bit) and against torch / f64 restatements, and ragged sessions against the reference
goldens, the clip forward, the oracle, pool.step and one-session streams."""
import numpy as np
import pytest
import torch

from conftest import build_hip_seeker, golden_inputs, load_golden
from stream_kit import (CHUNK_LISTS, MODES, PRECISIONS, _cat, _check_vs, _i32, _pool_step, _ragged_launch, _ragged_step, _run_ragged, _small_clips,
                        _small_net, _stream, _t0_sets, _tables, f64_cached_attention)
from tcow_amd import ops, stream, synth
from tcow_amd._lib import TcowError

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- kernels

def _ragged_case(mode_name, cs, S, heads, T_total, n_slots, causal, seed, t0s):
    dev = torch.device('cuda')
    mode = MODES[mode_name]
    n, F, D = len(cs), sum(cs), heads * 64
    dt = ops.tdtype(ops.F32 if mode == ops.F32X3 else mode)
    rng = np.random.default_rng(seed)
    while True:                                                 # a non-identity injection of the sessions into the slots (where one exists)
        slots = [int(v) for v in rng.permutation(n_slots)[:n]]
        if slots != list(range(n)) or n_slots == 1:
            break
    g = torch.Generator(device=dev).manual_seed(seed)
    qkv = torch.randn(F * S, 3 * D, device=dev, generator=g).to(dt)
    kc0 = torch.randn(n_slots, S - 1, heads, T_total, 64, device=dev, generator=g).to(dt)
    vc0 = torch.randn(n_slots, S - 1, heads, T_total, 64, device=dev, generator=g).to(dt)
    kc, vc = kc0.clone(), vc0.clone()
    out = _ragged_launch(mode, cs, S, heads, causal, T_total, n_slots, t0s, slots, qkv, kc, vc)
    # n launches of the pool kernel with one row each: that session's qkv rows, t0 and slot, on copies of the whole caches
    kc_r, vc_r = kc0.clone(), vc0.clone()
    out_r = torch.full((F * S, D), float('nan'), device=dev).to(dt)
    first = stream.ragged_tables(t0s, slots, cs)['first']
    for r in range(n):
        lo, hi = first[r] * S, (first[r] + cs[r]) * S
        ops.attn_temporal_pool(mode, 1, cs[r], S, D, heads, causal, T_total, n_slots, _i32([t0s[r]]), _i32([slots[r]]), qkv[lo:hi], kc_r, vc_r, out_r[lo:hi])
    tag = (mode_name, cs, S, heads, T_total, n_slots, causal, slots, t0s)
    assert torch.equal(out, out_r), tag
    assert torch.equal(kc, kc_r) and torch.equal(vc, vc_r), tag               # the whole tensors: unnamed slots and positions outside [t0, t0 + c) bit-unchanged
    for r in range(n):
        lo, hi = first[r] * S, (first[r] + cs[r]) * S
        ref, V = (x[0] for x in f64_cached_attention(qkv[lo:hi], kc0[slots[r]][None], vc0[slots[r]][None], 1, cs[r], S, heads, t0s[r]))
        got = out[lo:hi].view(cs[r], S, heads, 64)[:, 1:].permute(1, 2, 0, 3).double()
        err = float((got - ref).abs().max())
        print('ragged kernel', tag, 'session', r, 'err', err)
        if dt == torch.float32:
            assert err <= 2e-6 * float(ref.abs().max()), (tag, r, err)
        else:
            assert err <= ((2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11) + 1e-5) * float(V.abs().max()), (tag, r, err)
        assert float(out[lo:hi].view(cs[r], S, D)[:, 0].float().abs().max()) == 0.0, tag       # slot-0 rows: zero


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'fp16'])
def test_ragged_attention_equals_the_pool_kernel_session_by_session(cuda, mode):
    seed = 0
    rng = np.random.default_rng(77)
    for cs, T_total in CHUNK_LISTS:
        n = len(cs)
        for S in (2, 17):
            for heads in (1, 2):
                for n_slots in (n, n + 2):
                    for t0s in _t0_sets(cs, T_total, rng):
                        seed += 1
                        _ragged_case(mode, cs, S, heads, T_total, n_slots, 1 + seed % 2, seed, t0s)


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'fp16'])
def test_ragged_attention_batches_across_the_cache_chunk_boundary(cuda, mode):
    """T_total = 40: a loaded batch of G * ST_U = 32 / 16 keys that straddles the cache / chunk boundary, and a key loop with a second iteration."""
    for S in (2, 17):
        for heads in (1, 2):
            _ragged_case(mode, [36], S, heads, 40, 3, 1, 500 + S + heads, [3])
            _ragged_case(mode, [3, 1], S, heads, 40, 4, 2, 600 + S + heads, [37, 0])


def test_ragged_attention_bf16x3_mode_stores_f32(cuda):
    _ragged_case('x3', [1, 3, 2], 17, 2, 30, 5, 1, 99, [27, 0, 28])


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_ragged_attention_real_grid(cuda, mode):
    _ragged_case(mode, [1, 4], 301, 12, 30, 4, 1, 7, [29, 0])


def test_cls_ragged_vs_torch(cuda):
    dev = torch.device('cuda')
    cs, S, D, n_slots = [2, 1, 3], 5, 128, 5
    t0s, slots = (0, 3, 0), (4, 0, 2)
    n, F = len(cs), sum(cs)
    tb, first = _tables(t0s, slots, cs)
    x = torch.randn(F * S, D, device=dev)
    cache0 = torch.randn(n_slots, D, device=dev)
    cache, y = cache0.clone(), x.clone()
    ops.cls_ragged(y, n, F, S, cache, n_slots, tb['t0'], tb['slot'], tb['first'], tb['c'])
    ref = x.clone().view(F, S, D)
    ref_cache = cache0.clone()
    for r in range(n):
        fr = slice(first[r], first[r] + cs[r])
        if t0s[r] == 0:
            ref[fr, 0] = x.view(F, S, D)[first[r], 0][None]
            ref_cache[slots[r]] = x.view(F, S, D)[first[r], 0]
        else:
            ref[fr, 0] = cache0[slots[r]][None]
    assert torch.equal(y.view(F, S, D), ref)
    assert torch.equal(cache, ref_cache)                                        # the kept rows, and every other row unchanged
    # a slot outside the pool: NaN in that session's slot-0 rows alone, no cache row touched
    cache, y = cache0.clone(), x.clone()
    ops.cls_ragged(y, n, F, S, cache, n_slots, tb['t0'], _i32((4, 5, 2)), tb['first'], tb['c'])
    assert torch.equal(cache, ref_cache)
    assert torch.isnan(y.view(F, S, D)[2, 0]).all()
    ref[2, 0] = 0; y.view(F, S, D)[2, 0] = 0
    assert torch.equal(y.view(F, S, D), ref)


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_ragged_attention_bad_row_among_good_rows(cuda, mode):
    """A session with t0 + c > T_total: its output rows are NaN, both caches are bit-unchanged for its slot, and the other sessions are equal to a
    launch without it."""
    dev = torch.device('cuda')
    m = MODES[mode]
    dt = ops.tdtype(m)
    S, heads, T_total, n_slots = 17, 2, 30, 4
    D = heads * 64
    cs, t0s, slots = [2, 3, 1], [5, 28, 0], [3, 1, 0]                            # the middle session: 28 + 3 > 30
    F = sum(cs)
    g = torch.Generator(device=dev).manual_seed(31)
    qkv = torch.randn(F * S, 3 * D, device=dev, generator=g).to(dt)
    kc0 = torch.randn(n_slots, S - 1, heads, T_total, 64, device=dev, generator=g).to(dt)
    vc0 = torch.randn(n_slots, S - 1, heads, T_total, 64, device=dev, generator=g).to(dt)
    kc, vc = kc0.clone(), vc0.clone()
    out = _ragged_launch(m, cs, S, heads, 1, T_total, n_slots, t0s, slots, qkv, kc, vc, fill=0.0)       # (zeros: the NaN below are the kernel's)
    kc_g, vc_g = kc0.clone(), vc0.clone()
    good = torch.cat([qkv[:2 * S], qkv[5 * S:]], 0).contiguous()
    out_g = _ragged_launch(m, [2, 1], S, heads, 1, T_total, n_slots, [5, 0], [3, 0], good, kc_g, vc_g)
    assert torch.isnan(out[2 * S:5 * S].float()).all()
    assert torch.equal(kc[1], kc0[1]) and torch.equal(vc[1], vc0[1])
    assert torch.equal(torch.cat([out[:2 * S], out[5 * S:]], 0), out_g)
    assert torch.equal(kc, kc_g) and torch.equal(vc, vc_g)
    # a frame whose session does not own it (j outside [0, c)) and a slot outside the pool are bad in the same way
    for bad_tables in ('row_of_frame', 'slot'):
        tb, _ = _tables([5, 20, 0], slots, cs)
        if bad_tables == 'row_of_frame':
            tb['row_of_frame'] = _i32([0, 0, 1, 1, 0, 2])                          # flat frame 4 names session 0, whose frames are 0 and 1
        else:
            tb['slot'] = _i32([3, n_slots, 0])
        kc, vc = kc0.clone(), vc0.clone()
        out = torch.zeros(F * S, D, device=dev).to(dt)
        ops.attn_temporal_ragged(m, 3, F, S, D, heads, 1, T_total, n_slots, tb['t0'], tb['slot'], tb['first'], tb['c'], tb['row_of_frame'], qkv, kc, vc, out)
        nan_frames = [4] if bad_tables == 'row_of_frame' else [2, 3, 4]
        for f in range(F):
            assert bool(torch.isnan(out[f * S:(f + 1) * S].float()).all()) == (f in nan_frames), (bad_tables, f)
        if bad_tables == 'slot':
            assert torch.equal(kc[1], kc0[1]) and torch.equal(vc[1], vc0[1]) and torch.equal(kc[2], kc0[2])
        else:
            assert torch.equal(kc[1, :, :, 22:], kc0[1, :, :, 22:]) and torch.equal(vc[1, :, :, 22:], vc0[1, :, :, 22:])   # session 1 wrote positions 20 and 21 only: the bad frame appended nothing
            assert torch.equal(kc[3, :, :, 7:], kc0[3, :, :, 7:])                                                       # session 0 wrote positions 5 and 6 only


def test_ragged_kernels_refuse_bad_arguments(cuda):
    dev = torch.device('cuda')
    cs, S, heads, T, n_slots = [1, 2], 5, 1, 8, 2
    n, F = 2, 3
    qkv = torch.zeros(F * S, 192, device=dev); kc = torch.zeros(n_slots, S - 1, heads, T, 64, device=dev); out = torch.zeros(F * S, 64, device=dev)
    tb, _ = _tables([0, 3], [1, 0], cs)
    args = lambda **kw: [kw.get(k, tb[k]) for k in ('t0', 'slot', 'first', 'c', 'row_of_frame')]
    run = lambda causal=1, T_total=T, D=64, slots=n_slots, n=n, F=F, qkv=qkv, out=out, **kw: ops.attn_temporal_ragged(
        ops.F32, n, F, S, D, heads, causal, T_total, slots, *args(**kw), qkv, kc, kc.clone(), out)
    run()
    for causal in (0, 3, -1):
        with pytest.raises(TcowError, match='causal'):
            run(causal=causal)
    with pytest.raises(TcowError, match='T_total'):
        run(T_total=4096)
    with pytest.raises(TcowError, match='head_dim'):
        run(D=96)
    x = torch.zeros(F * S, 64, device=dev); cc = torch.zeros(n_slots, 64, device=dev)
    ops.cls_ragged(x, n, F, S, cc, n_slots, tb['t0'], tb['slot'], tb['first'], tb['c'])
    for bad in (0, -1):
        with pytest.raises(TcowError, match='n_slots'):
            run(slots=bad)
        with pytest.raises(TcowError, match='tcow_cls_step: n_slots'):
            ops.cls_ragged(x, n, F, S, cc, bad, tb['t0'], tb['slot'], tb['first'], tb['c'])
    for name in ('t0', 'slot', 'first', 'c', 'row_of_frame'):
        with pytest.raises(TcowError, match='CUDA'):
            run(**{name: tb[name].cpu()})
        with pytest.raises(TcowError, match='int32'):
            run(**{name: tb[name].long()})
        with pytest.raises(TcowError, match='entries'):                         # a table length that disagrees with n (per session) or F (per frame)
            run(**{name: torch.cat([tb[name], tb[name][:1]])})
    with pytest.raises(TcowError, match='entries'):
        run(n=3)
    with pytest.raises(TcowError, match='entries'):
        run(F=4, qkv=torch.zeros(4 * S, 192, device=dev), out=torch.zeros(4 * S, 64, device=dev))
    with pytest.raises(TcowError, match='rows'):
        run(qkv=torch.zeros(F * S + 1, 192, device=dev))
    with pytest.raises(TcowError, match='rows'):
        run(out=torch.zeros(F * S - 1, 64, device=dev))
    with pytest.raises(TcowError, match='CUDA'):
        ops.cls_ragged(x, n, F, S, cc, n_slots, tb['t0'].cpu(), tb['slot'], tb['first'], tb['c'])
    with pytest.raises(TcowError, match='entries'):
        ops.cls_ragged(x, n, F, S, cc, n_slots, tb['t0'], tb['slot'][:1], tb['first'], tb['c'])
    with pytest.raises(TcowError, match='rows'):
        ops.cls_ragged(x[:S], n, F, S, cc, n_slots, tb['t0'], tb['slot'], tb['first'], tb['c'])


# ---------------------------------------------------------------------------------------------- ragged sessions

@pytest.mark.parametrize('name', ['g1_cfg1_d256', 'g2_ca2'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_ragged_vs_reference_golden_and_clip_forward(cuda, name, precision):
    meta, g = load_golden(name)
    cfg, sd, rgb, qm = golden_inputs(meta)
    net = build_hip_seeker(cfg, sd, precision).cuda().eval()
    rgb, qm = rgb.cuda(), qm.cuda()
    B, T = rgb.shape[0], cfg['num_total_frames']
    rgb_l, qm_l = rgb[0:1].flip(2).contiguous(), qm[0:1].flip(2).contiguous()             # one more session: row 0's clip, frames in reverse order
    with torch.no_grad():
        clip_m, clip_f = net(rgb, qm)
        lead_m, lead_f = net(rgb_l, qm_l)
    clips = [(rgb_l, qm_l)] + [(rgb[b:b + 1], qm[b:b + 1]) for b in range(B)]
    outs = _run_ragged(net.stream_pool(B + 1), clips, T, opens=[0] + [1 + b % 2 for b in range(B)])
    om, fl = (torch.cat(x, 0) for x in zip(*outs[1:]))
    assert om.shape == clip_m.shape and fl.shape == clip_f.shape
    gm, gf = torch.from_numpy(g['output_mask']).cuda(), torch.from_numpy(g['output_flags']).cuda()
    _check_vs(om, fl, gm, gf, precision, g['output_mask'], g['output_flags'])
    _check_vs(om, fl, clip_m, clip_f, precision, g['output_mask'], g['output_flags'])
    _check_vs(outs[0][0], outs[0][1], lead_m, lead_f, precision, g['output_mask'], g['output_flags'])


def _phased(net, clips):
    """A pool of 4 slots with three sessions at frames 2, 1, 0 (by pool.step)."""
    pool = net.stream_pool(4)
    ids = [pool.open() for _ in range(3)]
    _pool_step(pool, [(ids[0], *clips[0])])
    _pool_step(pool, [(ids[0], *clips[0]), (ids[1], *clips[1])])
    return pool, ids


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'bf16x3', 'fp16'])
@pytest.mark.parametrize('c', [1, 2])
def test_ragged_equal_chunk_lengths_are_bit_equal_to_pool_step(cuda, precision, c):
    """With every c_i = c a ragged step runs the GEMMs of pool.step on the same shapes, and every other kernel but the two ragged ones -- which
    are bit-equal to the pool kernels -- sees the same rows: twin pools give the same bits."""
    net = _small_net(precision)
    clips = _small_clips(3)
    p1, i1 = _phased(net, clips)
    p2, i2 = _phased(net, clips)
    order = (2, 0, 1)
    a = _pool_step(p1, [(i1[k], *clips[k]) for k in order], c)
    b = _ragged_step(p2, [(i2[k], *clips[k]) for k in order], [c] * 3)
    for k in range(3):
        assert torch.equal(a[i1[k]][0], b[i2[k]][0]) and torch.equal(a[i1[k]][1], b[i2[k]][1]), k


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-5), ('bf16', 1.5e-2)])
def test_ragged_mixed_chunk_lengths_vs_per_length_pool_steps(cuda, precision, tol):
    """The same tick served by one ragged step and by one pool.step per distinct chunk length (what a caller had to do before).  The GEMM tile
    choice depends on the row count, so the two agree to the precision's rounding, not bit for bit."""
    net = _small_net(precision)
    clips = _small_clips(3)
    p1, i1 = _phased(net, clips)                                # frames done: 2, 1, 0
    p2, i2 = _phased(net, clips)
    cs = [1, 3, 3]
    a = _ragged_step(p1, [(i1[k], *clips[k]) for k in range(3)], cs)
    b = _pool_step(p2, [(i2[0], *clips[0])], 1)
    b.update(_pool_step(p2, [(i2[1], *clips[1]), (i2[2], *clips[2])], 3))
    cs2 = [1, 1]                                                 # a second tick: sessions 0 and 2 have one frame left each, session 1 is done
    a2 = _ragged_step(p1, [(i1[2], *clips[2]), (i1[0], *clips[0])], cs2)
    b2 = _pool_step(p2, [(i2[2], *clips[2]), (i2[0], *clips[0])], 1)
    for x, y, ia, ib in ((a, b, i1, i2), (a2, b2, i1, i2)):
        for k in range(3):
            if ia[k] in x:
                d, df = float((x[ia[k]][0] - y[ib[k]][0]).abs().max()), float((x[ia[k]][1] - y[ib[k]][1]).abs().max())
                print('ragged vs per-length pool steps', precision, k, d, df)
                assert d < tol and df < tol, (k, d, df)
    assert [p1.frames_done(i) for i in i1] == [4, 4, 4] == [p2.frames_done(i) for i in i2]


@pytest.mark.parametrize('seed', list(range(4)))
def test_ragged_random_geometries_vs_oracle(cuda, seed):
    """test_pool_random_geometries_vs_oracle with a random chunk length per session and step."""
    from oracle import seeker_oracle as so
    rng = np.random.default_rng(8000 + seed)
    T = int(rng.integers(2, 10)); Hp = int(rng.integers(1, 6)); Wp = int(rng.integers(1, 7)); D = int(rng.choice([64, 128, 192]))
    st = int(rng.choice([1, 2, 4]))
    cfg = synth.seeker_config(num_total_frames=T, frame_height=16 * Hp, frame_width=16 * Wp, embed_dim=D, depth=int(rng.integers(1, 4)), num_heads=D // 64,
                              causal_attention=int(rng.choice([1, 2])), norm_embeddings=bool(rng.integers(0, 2)), track_map_stride=st,
                              track_map_resize=str(rng.choice(['bilinear', 'nearest'])), pretrained_norm=bool(rng.integers(0, 2)))
    sd = synth.make_state_dict(cfg, 9000 + seed)
    B = int(rng.integers(2, 4))
    clip = synth.make_clip(B, T, 16 * Hp, 16 * Wp, seed=9500 + seed)
    rgb = torch.from_numpy(clip['rgb']); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0))
    if qm.shape[0] != B:
        qm = qm.expand(B, -1, -1, -1, -1).contiguous()
    delay = [int(rng.integers(0, 4)) for _ in range(B)]
    plan, done, step = [], [0] * B, 0                            # per step: (sessions that take part, a chunk length each)
    while min(done) < T:
        rows = [b for b in range(B) if delay[b] <= step and done[b] < T]
        if rows:
            cs = [int(rng.integers(1, T - done[b] + 1)) for b in rows]
            plan.append((rows, cs))
            for b, c in zip(rows, cs):
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
        for rows, cs in plan:
            for b in rows:
                if b not in ids:
                    ids[b] = pool.open()
            out = _ragged_step(pool, [(ids[b], rgb_d[b:b + 1], qm_d[b:b + 1]) for b in rows], cs)
            for b in rows:
                got[b].append(out[ids[b]])
        om, fl = (torch.cat(x, 0) for x in zip(*[_cat(got[b]) for b in range(B)]))
        d, df = float((om.cpu() - om_r).abs().max()), float((fl.cpu() - fl_r).abs().max())
        print('ragged oracle', seed, precision, d, tol, df, ftol)
        assert d < tol, (precision, cfg, plan, delay)
        assert df < ftol, (precision, cfg, plan, delay)


@pytest.mark.parametrize('precision,tol', [('fp32', 2e-5), ('bf16', 1.5e-2)])
def test_ragged_mixes_with_step_and_slot_reuse_reads_nothing_of_the_previous_tenant(cuda, precision, tol):
    net = _small_net(precision)
    clips = _small_clips(4)
    want = [_stream(net, r, q, [1, 1, 1, 1]) for r, q in clips]
    pool = net.stream_pool(3)                                   # three slots: the newcomer can only get the slot the lead leaves
    lead = pool.open()
    got = {lead: [_ragged_step(pool, [(lead, *clips[0])], [2])[lead]]}
    a, b = pool.open(), pool.open()
    got.update({a: [], b: []})
    for i, o in _pool_step(pool, [(a, *clips[1]), (lead, *clips[0]), (b, *clips[2])]).items():            # step and step_ragged on the same sessions
        got[i].append(o)
    for i, o in _ragged_step(pool, [(b, *clips[2]), (lead, *clips[0]), (a, *clips[1])], [2, 1, 1]).items():
        got[i].append(o)
    assert pool.frames_done(lead) == 4
    pool.close(lead)
    new = pool.open()                                           # the lead's slot: its K / V rows 0..3 and its cls rows are still there
    got[new] = []
    for i, o in _ragged_step(pool, [(new, *clips[3]), (a, *clips[1]), (b, *clips[2])], [3, 2, 1]).items():
        got[i].append(o)
    pool.close(a); pool.close(b)
    got[new].append(_pool_step(pool, [(new, *clips[3])])[new])
    for i, k in ((lead, 0), (a, 1), (b, 2), (new, 3)):
        om, fl = _cat(got[i])
        assert om.shape == want[k][0].shape
        d, df = float((om - want[k][0]).abs().max()), float((fl - want[k][1]).abs().max())
        print('ragged slot reuse', precision, 'clip', k, d, df)
        assert d < tol and df < tol, (k, d, df)
    assert float((want[3][0] - want[0][0]).abs().max()) > tol               # the two tenants' outputs differ by more than the tolerance


def test_ragged_lifecycle(cuda):
    cfg = synth.seeker_config(num_total_frames=4, frame_height=32, frame_width=48, embed_dim=128, depth=2, num_heads=2, causal_attention=1)
    net = build_hip_seeker(cfg, synth.make_state_dict(cfg, 9), 'bf16').cuda().eval()
    for p in net.parameters():
        p.requires_grad_(True)
    clip = synth.make_clip(2, 4, 32, 48, seed=4)
    rgb = torch.from_numpy(clip['rgb']).cuda(); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
    pool = net.seeker.stream_pool(2)                            # (the QueryMaskTracker's pool: the same class)
    a, b = pool.open(), pool.open()
    ms, fls = pool.step_ragged([a], [rgb[0:1, :, 0:1]], [qm[0:1, :, 0:1]])
    m0, f0 = ms[0].clone(), fls[0].clone()
    assert not ms[0].requires_grad and not fls[0].requires_grad
    assert pool.frames_done(a) == 1 and pool.frames_done(b) == 0
    # refused steps: nothing is launched, no counter moves.  a is at frame 1, b at 0
    ra, qa, rb, qb = rgb[0:1, :, 1:2], qm[0:1, :, 1:2], rgb[1:2, :, 0:3], qm[1:2, :, 0:3]
    refusals = [
        ('duplicate', ([a, a], [ra, ra], [qa, qa])),
        ('not open', ([a, 12345], [ra, rb], [qa, qb])),
        ('1 .. capacity', ([], [], None)),
        ('lengths must agree', ([a, b], [ra], [qa, qb])),
        ('lengths must agree', ([a, b], [ra, rb], [qa])),
        (f'session {b}: rgb', ([a, b], [ra, rb[:, :2]], [qa, qb])),
        (f'session {b}: rgb', ([a, b], [ra, rgb[:, :, 0:3]], [qa, qb])),
        (f'session {b}: rgb', ([a, b], [ra, rb[:, :, 0:0]], [qa, None])),
        (f'session {b}: query_mask', ([a, b], [ra, rb], [qa, qb[:, :, 0:2]])),
        (f'session {b}: inputs must be on', ([a, b], [ra, rb.cpu()], None)),
        (f'session {b}: frames 0..4', ([a, b], [ra, torch.cat([rb, rb[:, :, :2]], 2)], None)),          # the offender is the last of the list
        (f'session {a}: frames 1..4', ([a, b], [rgb[0:1], rb], None)),
    ]
    for match, (ids, rgbs, qms) in refusals:
        k0, v0, c0 = pool._st.k_cache.clone(), pool._st.v_cache.clone(), pool._st.cls_cache.clone()
        with pytest.raises(TcowError, match=match):
            pool.step_ragged(ids, rgbs, qms)
        assert pool.frames_done(a) == 1 and pool.frames_done(b) == 0, match
        for x, y in ((k0, pool._st.k_cache), (v0, pool._st.v_cache), (c0, pool._st.cls_cache)):       # nothing was launched on the caches (bits, NaN-safe)
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), match
    got = pool.step_ragged([a, b], [ra, rb], [qa, qb])
    ref_pool = net.stream_pool(2)                                                           # the same steps, the refused ones never sent
    r_a, r_b = ref_pool.open(), ref_pool.open()
    ref_pool.step_ragged([r_a], [rgb[0:1, :, 0:1]], [qm[0:1, :, 0:1]])
    want = ref_pool.step_ragged([r_a, r_b], [ra, rb], [qa, qb])
    for k in range(2):
        assert torch.equal(got[0][k], want[0][k]) and torch.equal(got[1][k], want[1][k])
    assert pool.frames_done(a) == 2 and pool.frames_done(b) == 3
    # the outputs are the caller's: a later step does not write into them
    keep = [t.clone() for t in got[0]]
    pool.step_ragged([b, a], [rgb[1:2, :, 3:4], rgb[0:1, :, 2:4]], None)
    assert all(torch.equal(x, y) for x, y in zip(keep, got[0]))
    # query_masks=None == a list of None == explicit zeros, entry by entry
    outs = []
    for qms in (None, [None, None], [torch.zeros_like(qm[0:1, :, 0:2]), None], [torch.zeros_like(qm[0:1, :, 0:2]), torch.zeros_like(qm[1:2, :, 0:1])]):
        pool.reset(a); pool.reset(b)
        outs.append(pool.step_ragged([a, b], [rgb[0:1, :, 0:2], rgb[1:2, :, 0:1]], qms))
    for o in outs[1:]:
        for k in range(2):
            assert torch.equal(o[0][k], outs[0][0][k]) and torch.equal(o[1][k], outs[0][1][k])
    # reset(id) and close() / open() start at frame 0: the first frame again gives the first outputs again
    pool.reset(a)
    again = pool.step_ragged([a], [rgb[0:1, :, 0:1]], [qm[0:1, :, 0:1]])
    assert torch.equal(again[0][0], m0) and torch.equal(again[1][0], f0)
    pool.close(a)
    with pytest.raises(TcowError, match='not open'):
        pool.step_ragged([a], [rgb[0:1, :, 1:2]], None)
    # a parameter change invalidates the caches; leaving eval mode
    with torch.no_grad():
        net.seeker.vit.blocks[0].mlp.fc1.bias.add_(0.01)
    with pytest.raises(TcowError, match='changed'):
        pool.step_ragged([b], [rgb[1:2, :, 1:2]], None)
    assert pool.frames_done(b) == 1
    fresh = net.stream_pool(1)
    s = fresh.open()
    assert torch.isfinite(fresh.step_ragged([s], [rgb[0:1, :, 0:1]], None)[0][0]).all()
    net.train()
    with pytest.raises(TcowError, match='training'):
        fresh.step_ragged([s], [rgb[0:1, :, 1:2]], None)
    net.eval()


def test_ragged_steps_leave_the_clip_path_and_streams_alone(cuda):
    """After ragged steps on a module, its clip forward and a SeekerStream opened on it are bit-identical to those of a module that never pooled."""
    cfg = synth.seeker_config(num_total_frames=5, frame_height=32, frame_width=48, embed_dim=128, depth=2, num_heads=2, causal_attention=1)
    sd = synth.make_state_dict(cfg, 12)
    clip = synth.make_clip(2, 5, 32, 48, seed=6)
    rgb = torch.from_numpy(clip['rgb']).cuda(); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
    pooled = build_hip_seeker(cfg, sd, 'bf16').cuda().eval()
    fresh = build_hip_seeker(cfg, sd, 'bf16').cuda().eval()
    with torch.no_grad():
        x0, fx0 = pooled(rgb, qm)
    s0 = _stream(pooled, rgb, qm, [2, 3])
    pool = pooled.stream_pool(2)
    a = pool.open()
    pool.step_ragged([a], [rgb[0:1, :, 0:1]], [qm[0:1, :, 0:1]])
    b = pool.open()
    pool.step_ragged([b, a], [rgb[1:2, :, 0:3], rgb[0:1, :, 1:2]], [qm[1:2, :, 0:3], qm[0:1, :, 1:2]])
    pool.step_ragged([a, b], [rgb[0:1, :, 2:5], rgb[1:2, :, 3:5]], None)
    with torch.no_grad():
        x, fx = pooled(rgb, qm)
        y, fy = fresh(rgb, qm)
    assert torch.equal(x, y) and torch.equal(fx, fy) and torch.equal(x, x0) and torch.equal(fx, fx0)
    for split in ([1] * 5, [2, 3]):
        s1, f1 = _stream(pooled, rgb, qm, split)
        s2, f2 = _stream(fresh, rgb, qm, split)
        assert torch.equal(s1, s2) and torch.equal(f1, f2), split
    assert torch.equal(s0[0], s1) and torch.equal(s0[1], f1)

"""GPU: a stream pool whose K / V caches are a heap of pages (stream_pool(page_frames=P, pages=N), tcow_amd/stream.py).  Where a key lives does
not enter the arithmetic of temporal attention, so everything here is exact: the paged kernel against the contiguous ragged kernel bit for bit
(outputs, and the pages gathered back), a paged pool against a contiguous pool on the same feed schedule bit for bit, and the page accounting."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import build_hip_seeker, golden_inputs, load_golden
from stream_kit import (CHUNK_LISTS, MODES, PRECISIONS, _check_vs, _i32, _pool_step, _ragged_launch, _ragged_step, _run_ragged, _small_clips,
                        _small_net, _t0_sets, _tables, _to_pages as _pages_filled)
from tcow_amd import _lib, ops, stream, synth
from tcow_amd._lib import TcowError

pytestmark = pytest.mark.gpu

SENTINEL = 7.0                                                  # what unowned pages (and the tail of a session's last page) hold: finite, exact in every type
_to_pages = functools.partial(_pages_filled, fill=SENTINEL)     # (caches, page_of, n_pages, P) -> page arrays; everything else SENTINEL


# ---------------------------------------------------------------------------------------------- kernel

def _page_table(n, T_total, P, extra, rng):
    """A non-identity injection of the (session, page index) pairs into n * pps + extra page ids."""
    pps = -(-T_total // P)
    n_pages = n * pps + extra
    while True:
        ids = [int(v) for v in rng.permutation(n_pages)[:n * pps]]
        if ids != list(range(n * pps)):
            break
    return [ids[r * pps:(r + 1) * pps] for r in range(n)], n_pages


def _paged_launch(mode, cs, S, heads, causal, T_total, n_pages, P, t0s, page_rows, qkv, kp, vp, fill=float('nan')):
    F, D = sum(cs), heads * 64
    tb, _ = _tables(t0s, list(range(len(cs))), cs)
    out = torch.full((F * S, D), fill, device=qkv.device).to(qkv.dtype)
    ops.attn_temporal_ragged_paged(mode, len(cs), F, S, D, heads, causal, T_total, n_pages, P, tb['t0'], page_rows, tb['first'], tb['c'], tb['row_of_frame'],
                                   qkv, kp, vp, out)
    return out


def _case_inputs(mode_name, cs, S, heads, T_total, seed):
    dev = torch.device('cuda')
    mode = MODES[mode_name]
    n, F, D = len(cs), sum(cs), heads * 64
    dt = ops.tdtype(ops.F32 if mode == ops.F32X3 else mode)
    g = torch.Generator(device=dev).manual_seed(seed)
    qkv = torch.randn(F * S, 3 * D, device=dev, generator=g).to(dt)
    kc0 = torch.randn(n, S - 1, heads, T_total, 64, device=dev, generator=g).to(dt)
    vc0 = torch.randn(n, S - 1, heads, T_total, 64, device=dev, generator=g).to(dt)
    return mode, qkv, kc0, vc0


def _paged_case(mode_name, cs, S, heads, T_total, P, causal, seed, t0s, extra=3):
    """The contiguous ragged kernel (session r on slot r) and the paged kernel on the same contents: equal outputs, and the page arrays after the
    launch equal the contiguous caches after the launch scattered the same way -- owned pages gathered back, every unowned page, the tail of a last
    page and every position outside [t0, t0 + c) in one comparison."""
    n = len(cs)
    mode, qkv, kc0, vc0 = _case_inputs(mode_name, cs, S, heads, T_total, seed)
    page_of, n_pages = _page_table(n, T_total, P, extra, np.random.default_rng(seed))
    kc, vc = kc0.clone(), vc0.clone()
    out_c = _ragged_launch(mode, cs, S, heads, causal, T_total, n, t0s, list(range(n)), qkv, kc, vc)
    kp, vp = _to_pages(kc0, page_of, n_pages, P), _to_pages(vc0, page_of, n_pages, P)
    out_p = _paged_launch(mode, cs, S, heads, causal, T_total, n_pages, P, t0s, _i32(sum(page_of, [])).view(n, -1), qkv, kp, vp)
    tag = (mode_name, cs, S, heads, T_total, P, causal, t0s, page_of)
    assert not torch.isnan(out_c.float()).any(), tag            # (every row of the poisoned output was written: torch.equal below compares numbers)
    assert torch.equal(out_p, out_c), tag
    assert not torch.equal(kc, kc0), tag                        # (the launch did append)
    assert torch.equal(kp, _to_pages(kc, page_of, n_pages, P)) and torch.equal(vp, _to_pages(vc, page_of, n_pages, P)), tag


P_LIST = (1, 2, 8, 32)                                          # 32 >= T_total of every case below but the T_total = 40 ones


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'fp16'])
def test_paged_attention_equals_the_ragged_kernel(cuda, mode):
    seed = 0
    rng = np.random.default_rng(78)
    for cs, T_total in CHUNK_LISTS:
        for S in (2, 17):
            for heads in (1, 2):
                for t0s in _t0_sets(cs, T_total, rng):
                    for P in P_LIST:
                        seed += 1
                        _paged_case(mode, cs, S, heads, T_total, P, 1 + seed % 2, seed, t0s)


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'fp16'])
def test_paged_attention_odd_t0_on_two_frame_pages(cuda, mode):
    """P = 2 with t0 odd (the append lands in the second line of a page that the same wave reads the first line of) and P = 1, every t0 of a short stream."""
    for t0 in range(0, 7):
        for P in (1, 2):
            _paged_case(mode, [1, 2], 3, 1, 9, P, 1, 300 + 10 * t0 + P, [t0, 7 - t0], extra=1)


@pytest.mark.parametrize('mode', ['f32', 'bf16', 'fp16'])
def test_paged_attention_batches_across_the_cache_chunk_boundary(cuda, mode):
    """T_total = 40: a loaded batch of G * ST_U = 32 / 16 keys that straddles the cache / chunk boundary and several pages, and a key loop with a second iteration."""
    for S in (2, 17):
        for heads in (1, 2):
            for P in P_LIST + (64,):
                _paged_case(mode, [36], S, heads, 40, P, 1, 500 + S + heads + P, [3])
                _paged_case(mode, [3, 1], S, heads, 40, P, 2, 600 + S + heads + P, [37, 0])


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_paged_attention_more_table_entries_than_lanes(cuda, mode):
    """A wave whose keys reach table entries >= 64 looks its pages up in memory, one below takes them from the entries its check loaded (a lane
    shuffle): sessions on either side in one launch, a chunk whose frames cross from one to the other, and a key loop of several iterations."""
    for S, heads in ((2, 1), (5, 2)):
        _paged_case(mode, [5, 1, 2], S, heads, 70, 1, 1, 700 + S, [62, 0, 68])          # entries 62 .. 66: frames on both sides of 64
        _paged_case(mode, [5, 1, 2], S, heads, 140, 2, 2, 710 + S, [125, 3, 138])       # pages 62 .. 64 of two frames
        _paged_case(mode, [1, 1], S, heads, 200, 1, 1, 720 + S, [199, 63])              # the last entry of a long table; the last narrow wave
    # an entry outside the heap beyond lane 63's is seen by the check; one beyond (t0 + c - 1) / P is not read
    S, heads, T_total, P = 3, 1, 70, 1
    cs, t0s = [1, 1], [66, 2]
    _, qkv, kc0, vc0 = _case_inputs(mode, cs, S, heads, T_total, 41)
    page_of, n_pages = _page_table(2, T_total, P, 2, np.random.default_rng(41))
    kp0, vp0 = _to_pages(kc0, page_of, n_pages, P), _to_pages(vc0, page_of, n_pages, P)
    rows = lambda table: _i32(sum(table, [])).view(len(table), -1)
    kp_c, vp_c = kp0.clone(), vp0.clone()
    clean = _paged_launch(MODES[mode], cs, S, heads, 1, T_total, n_pages, P, t0s, rows(page_of), qkv, kp_c, vp_c)
    for q, read in ((1, True), (64, True), (66, True), (67, False), (69, False)):
        bad = [list(p) for p in page_of]
        bad[0][q] = n_pages
        kp, vp = kp0.clone(), vp0.clone()
        out = _paged_launch(MODES[mode], cs, S, heads, 1, T_total, n_pages, P, t0s, rows(bad), qkv, kp, vp, fill=0.0)
        assert bool(torch.isnan(out[:S].float()).all()) == read, q
        assert torch.equal(out[S:], clean[S:]), q
        if read:
            assert torch.equal(kp[page_of[0][66]], kp0[page_of[0][66]]) and torch.equal(vp[page_of[0][66]], vp0[page_of[0][66]]), q        # nothing appended
        else:
            assert torch.equal(out, clean) and torch.equal(kp, kp_c) and torch.equal(vp, vp_c), q


def test_paged_attention_bf16x3_mode_stores_f32(cuda):
    _paged_case('x3', [1, 3, 2], 17, 2, 30, 8, 1, 99, [27, 0, 28])


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_paged_attention_real_grid(cuda, mode):
    _paged_case(mode, [1, 4], 301, 12, 30, 8, 1, 7, [29, 0])


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_paged_attention_bad_page_among_good_rows(cuda, mode):
    """Session 1 (t0 = 20, c = 3, P = 4: its frames read entries 0 .. 5) with an entry outside the heap in a page all its frames reach: its rows are
    NaN, the other sessions' rows and every page equal a launch without it.  The same entry beyond (t0 + c - 1) / P is never read."""
    m = MODES[mode]
    S, heads, T_total, P = 17, 2, 30, 4
    cs, t0s = [2, 3, 1], [5, 20, 0]
    _, qkv, kc0, vc0 = _case_inputs(mode, cs, S, heads, T_total, 31)
    page_of, n_pages = _page_table(3, T_total, P, 2, np.random.default_rng(31))
    kp0, vp0 = _to_pages(kc0, page_of, n_pages, P), _to_pages(vc0, page_of, n_pages, P)
    rows = lambda table: _i32(sum(table, [])).view(len(table), -1)
    kp_c, vp_c = kp0.clone(), vp0.clone()
    clean = _paged_launch(m, cs, S, heads, 1, T_total, n_pages, P, t0s, rows(page_of), qkv, kp_c, vp_c)
    kp_g, vp_g = kp0.clone(), vp0.clone()                       # the launch without session 1
    good = torch.cat([qkv[:2 * S], qkv[5 * S:]], 0).contiguous()
    out_g = _paged_launch(m, [2, 1], S, heads, 1, T_total, n_pages, P, [5, 0], rows([page_of[0], page_of[2]]), good, kp_g, vp_g)
    assert torch.equal(torch.cat([clean[:2 * S], clean[5 * S:]], 0), out_g)
    for entry in (-1, n_pages):
        for q in (0, 3, 5):                                     # 5 = (t0 + 0) / P: the page of the session's own frames
            bad = [list(p) for p in page_of]
            bad[1][q] = entry
            kp, vp = kp0.clone(), vp0.clone()
            out = _paged_launch(m, cs, S, heads, 1, T_total, n_pages, P, t0s, rows(bad), qkv, kp, vp, fill=0.0)      # (zeros: the NaN below are the kernel's)
            assert torch.isnan(out[2 * S:5 * S].float()).all(), (entry, q)
            assert torch.equal(torch.cat([out[:2 * S], out[5 * S:]], 0), out_g), (entry, q)
            assert torch.equal(kp, kp_g) and torch.equal(vp, vp_g), (entry, q)      # session 1 appended nothing; the others as without it
        for q in (6, 7):                                        # beyond (t0 + c - 1) / P = 5: not read
            bad = [list(p) for p in page_of]
            bad[1][q] = entry
            kp, vp = kp0.clone(), vp0.clone()
            out = _paged_launch(m, cs, S, heads, 1, T_total, n_pages, P, t0s, rows(bad), qkv, kp, vp)
            assert torch.equal(out, clean) and torch.equal(kp, kp_c) and torch.equal(vp, vp_c), (entry, q)
    # the rows the ragged kernel refuses are refused here too: t0 + c > T_total, and a frame that its session does not own
    kp, vp = kp0.clone(), vp0.clone()
    out = _paged_launch(m, cs, S, heads, 1, T_total, n_pages, P, [5, 28, 0], rows(page_of), qkv, kp, vp, fill=0.0)
    assert torch.isnan(out[2 * S:5 * S].float()).all() and torch.equal(torch.cat([out[:2 * S], out[5 * S:]], 0), out_g)
    assert torch.equal(kp, kp_g) and torch.equal(vp, vp_g)
    tb, _ = _tables(t0s, [0, 1, 2], cs)
    kp, vp = kp0.clone(), vp0.clone()
    out = torch.zeros(6 * S, heads * 64, device='cuda').to(qkv.dtype)
    ops.attn_temporal_ragged_paged(m, 3, 6, S, heads * 64, heads, 1, T_total, n_pages, P, tb['t0'], rows(page_of), tb['first'], tb['c'], _i32([0, 0, 1, 1, 0, 2]),
                                   qkv, kp, vp, out)                # flat frame 4 names session 0, whose frames are 0 and 1
    for f in range(6):
        assert bool(torch.isnan(out[f * S:(f + 1) * S].float()).all()) == (f == 4), f


def test_paged_kernel_refuses_bad_arguments(cuda):
    """Every refusal of the launcher names its argument and launches nothing: the output stays as it was."""
    dev = torch.device('cuda')
    cs, S, heads, T, P, n_pages = [1, 2], 5, 1, 8, 4, 5
    n, F = 2, 3
    qkv = torch.zeros(F * S, 192, device=dev); kp = torch.zeros(n_pages, S - 1, heads, P, 64, device=dev)
    out = torch.full((F * S, 64), 5.0, device=dev)
    tb, _ = _tables([0, 3], [0, 1], cs)
    pages = _i32([3, 0, 4, 1]).view(2, 2)
    args = lambda **kw: [kw.get(k, tb[k]) for k in ('first', 'c', 'row_of_frame')]
    run = lambda causal=1, T_total=T, D=64, n_pages=n_pages, P=P, pages=pages, n=n, F=F, qkv=qkv, out=out, **kw: ops.attn_temporal_ragged_paged(
        ops.F32, n, F, S, D, heads, causal, T_total, n_pages, P, kw.get('t0', tb['t0']), pages, *args(**kw), qkv, kp, kp.clone(), out)
    refusals = [('causal', dict(causal=0)), ('causal', dict(causal=3)), ('causal', dict(causal=-1)), ('T_total', dict(T_total=4096, pages=_i32(range(2048)).view(2, -1))),
                ('head_dim', dict(D=96)), ('page_frames', dict(P=3)), ('page_frames', dict(P=0)), ('page_frames', dict(P=-4)), ('page_frames', dict(P=2048)),
                ('n_pages', dict(n_pages=0)), ('n_pages', dict(n_pages=-1)), ('does not cover T_total', dict(pages=_i32([3, 0]).view(2, 1))),
                ('does not cover T_total', dict(P=2)), ('page_rows', dict(pages=pages.long())), ('page_rows', dict(pages=pages.view(-1))),
                ('page_rows', dict(pages=_i32([3, 0, 4, 1, 2, 2]).view(3, 2))), ('CUDA', dict(pages=pages.cpu())),
                ('entries', dict(n=3)), ('rows', dict(qkv=torch.zeros(F * S + 1, 192, device=dev)))]
    for name in ('t0', 'first', 'c', 'row_of_frame'):
        refusals += [('CUDA', {name: tb[name].cpu()}), ('int32', {name: tb[name].long()}), ('entries', {name: torch.cat([tb[name], tb[name][:1]])})]
    for match, kw in refusals:
        with pytest.raises(TcowError, match=match):
            run(**kw)
        assert bool((out == 5.0).all()), (match, kw)
    # null pointers cannot come through ops: the entry point itself
    ptrs = dict(t0_rows=tb['t0'], page_rows=pages, first_rows=tb['first'], c_rows=tb['c'], row_of_frame=tb['row_of_frame'], qkv=qkv, k_cache=kp, v_cache=kp.clone(),
                out=out)
    fn = _lib.lib().tcow_attn_temporal_step
    for k in ptrs:                                                              # each pointer field of a paged ragged record in turn
        rec = _lib.StreamAttnArgs(shape=_lib.AttnShape(1, F, S, 64, heads, 1, _lib.TCOW_F32), cache_dtype=_lib.TCOW_F32, T_total=T, n_sessions=n, page_frames=P,
                                  n_pages=n_pages, pages_per_session=2, **{name: None if name == k else t.data_ptr() for name, t in ptrs.items()})
        assert fn(None, ctypes.byref(rec)) != 0 and b'null pointer' in _lib.lib().tcow_last_error()
        assert bool((out == 5.0).all()), k
    assert fn(None, None) != 0 and b'null args' in _lib.lib().tcow_last_error()
    run()
    assert not bool((out == 5.0).any())


# ---------------------------------------------------------------------------------------------- paged pools

def _schedule(pool, clips):
    """Sessions opened at different ticks, a close and a re-open in between, step and step_ragged mixed (T = 4) -> every output in order."""
    outs = []
    keep = lambda d, order: outs.extend(d[i] for i in order)
    a = pool.open()
    keep(_ragged_step(pool, [(a, *clips[0])], [2]), [a])
    b, c = pool.open(), pool.open()
    keep(_pool_step(pool, [(b, *clips[1]), (a, *clips[0]), (c, *clips[2])]), [a, b, c])
    keep(_ragged_step(pool, [(c, *clips[2]), (a, *clips[0]), (b, *clips[1])], [2, 1, 1]), [a, b, c])
    assert pool.frames_done(a) == 4
    pool.close(a)
    d = pool.open()                                             # a's slot, and in a paged pool pages a held
    keep(_ragged_step(pool, [(d, *clips[3]), (b, *clips[1]), (c, *clips[2])], [3, 2, 1]), [d, b, c])
    pool.close(b); pool.close(c)
    keep(_pool_step(pool, [(d, *clips[3])]), [d])
    assert pool.frames_done(d) == 4
    return outs


@functools.lru_cache(maxsize=None)
def _contiguous_schedule(precision):
    """The schedule through a contiguous pool, once per precision: the reference of the paged pools (never written to afterwards)."""
    return _schedule(_small_net(precision).stream_pool(3), _small_clips(4))


@pytest.mark.parametrize('P', [1, 4])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_paged_pool_is_bit_equal_to_the_contiguous_pool(cuda, precision, P):
    want = _contiguous_schedule(precision)
    pool = _small_net(precision).stream_pool(3, page_frames=P)
    assert pool.pages_total == 3 * (4 // P) == pool.pages_free
    got = _schedule(pool, _small_clips(4))
    assert len(got) == len(want)
    for k, ((m, f), (wm, wf)) in enumerate(zip(got, want)):
        assert m.shape == wm.shape and torch.equal(m, wm) and torch.equal(f, wf), (precision, P, k)


@pytest.mark.parametrize('name', ['g1_cfg1_d256', 'g2_ca2'])
@pytest.mark.parametrize('precision', PRECISIONS)
def test_paged_pool_vs_reference_golden(cuda, name, precision):
    meta, g = load_golden(name)
    cfg, sd, rgb, qm = golden_inputs(meta)
    net = build_hip_seeker(cfg, sd, precision).cuda().eval()
    rgb, qm = rgb.cuda(), qm.cuda()
    B, T = rgb.shape[0], cfg['num_total_frames']
    clips = [(rgb[b:b + 1], qm[b:b + 1]) for b in range(B)]
    pool = net.stream_pool(B, page_frames=2, pages=B * -(-T // 2))
    outs = _run_ragged(pool, clips, T, opens=[b % 2 for b in range(B)])
    assert pool.pages_free == 0                                 # every session ran to T: the default number of pages is exactly enough
    om, fl = (torch.cat(x, 0) for x in zip(*outs))
    gm, gf = torch.from_numpy(g['output_mask']).cuda(), torch.from_numpy(g['output_flags']).cuda()
    _check_vs(om, fl, gm, gf, precision, g['output_mask'], g['output_flags'])


def _tiny(T=6):
    cfg = synth.seeker_config(num_total_frames=T, frame_height=32, frame_width=48, embed_dim=128, depth=2, num_heads=2, causal_attention=1)
    net = build_hip_seeker(cfg, synth.make_state_dict(cfg, 9), 'bf16').cuda().eval()
    clip = synth.make_clip(2, T, 32, 48, seed=4)
    return net, torch.from_numpy(clip['rgb']).cuda(), torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()


def test_paged_pool_lifecycle_and_exhaustion(cuda):
    net, rgb, qm = _tiny()
    fr = lambda x, b, t0, c=1: x[b:b + 1, :, t0:t0 + c]
    pool = net.stream_pool(2, page_frames=2, pages=4)
    twin = net.seeker.stream_pool(2)                            # contiguous, fed every step but the refused one
    st = pool._st
    assert type(st) is stream._PagedState and tuple(st.k_cache.shape) == (2, 4, 6, 2, 2, 64) and st.k_cache.dtype == torch.bfloat16
    assert pool.cache_bytes == 2 * (2 * 4 * 6 * 2 * 2 * 64 * 2) + 2 * 2 * 128 * 4          # K and V page arrays + the f32 cls rows [depth, capacity, D]
    assert (pool.pages_total, pool.pages_free) == (4, 4)
    a, b = pool.open(), pool.open()
    ta, tb = twin.open(), twin.open()
    assert pool.pages_of(a) == () and pool.pages_free == 4      # an open session that has seen no frame holds nothing
    same = lambda x, y: all(torch.equal(p, q) for p, q in zip(x, y))
    got = pool.step_ragged([a], [fr(rgb, 0, 0)], [fr(qm, 0, 0)]); want = twin.step_ragged([ta], [fr(rgb, 0, 0)], [fr(qm, 0, 0)])
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert pool.pages_of(a) == (0,) and pool.pages_free == 3
    both = lambda ta_, tb_: (torch.cat([fr(rgb, 0, ta_), fr(rgb, 1, tb_)], 0), torch.cat([fr(qm, 0, ta_), fr(qm, 1, tb_)], 0))
    assert same(pool.step([a, b], *both(1, 0)), twin.step([ta, tb], *both(1, 0)))
    assert pool.pages_of(a) == (0,) and pool.pages_of(b) == (1,) and pool.pages_free == 2  # a's frame 1 fits its page; b's frame 0 takes one
    assert same(pool.step([a, b], *both(2, 1)), twin.step([ta, tb], *both(2, 1)))
    assert pool.pages_of(a) == (0, 2) and pool.pages_of(b) == (1,) and pool.pages_free == 1
    # a: frames 3, 4 -> a third page; b: frame 2 -> a second page: 2 needed, 1 free
    k0, v0, c0 = st.k_cache.clone(), st.v_cache.clone(), st.cls_cache.clone()
    with pytest.raises(TcowError, match=r'needs 2 more page\(s\) of 2 frame\(s\), 1 of 4 are free'):
        pool.step_ragged([a, b], [fr(rgb, 0, 3, 2), fr(rgb, 1, 2)], None)
    with pytest.raises(TcowError, match='out of pages'):
        pool.step([a, b], torch.cat([fr(rgb, 0, 3, 2), fr(rgb, 1, 2, 2)], 0), None)
    assert pool.frames_done(a) == 3 and pool.frames_done(b) == 2
    assert pool.pages_of(a) == (0, 2) and pool.pages_of(b) == (1,) and pool.pages_free == 1
    for x, y in ((k0, st.k_cache), (v0, st.v_cache), (c0, st.cls_cache)):                   # nothing was launched (bits, NaN-safe)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert same(pool.step([b, a], *[t.flip(0) for t in both(3, 2)]), twin.step([tb, ta], *[t.flip(0) for t in both(3, 2)]))      # the next step: as if never refused
    assert pool.pages_of(a) == (0, 2) and pool.pages_of(b) == (1, 3) and pool.pages_free == 0
    # reset and close give the pages back; the lowest free page is the next one out
    pool.reset(b); twin.reset(tb)
    assert pool.pages_of(b) == () and pool.pages_free == 2 and pool.frames_done(b) == 0
    got = pool.step_ragged([b, a], [fr(rgb, 1, 0, 2), fr(rgb, 0, 4)], None); want = twin.step_ragged([tb, ta], [fr(rgb, 1, 0, 2), fr(rgb, 0, 4)], None)
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert pool.pages_of(b) == (1,) and pool.pages_of(a) == (0, 2, 3) and pool.pages_free == 0     # in the order of the ids: b first
    pool.close(a)
    assert pool.pages_free == 3 and pool.pages_of(b) == (1,)
    with pytest.raises(TcowError, match='not open'):
        pool.pages_of(a)
    with pytest.raises(TcowError, match='contiguous'):
        twin.pages_free
    with pytest.raises(TcowError, match='contiguous'):
        twin.pages_of(tb)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_paged_pool_page_reuse_reads_nothing_of_the_previous_tenant(cuda, precision):
    """The pool has exactly the pages of one session: the newcomer gets the pages the lead leaves, poisoned with NaN in between."""
    net = _small_net(precision)
    clips = _small_clips(2)
    twin = net.stream_pool(1)
    pool = net.stream_pool(1, page_frames=2, pages=2)
    outs = []
    for p in (twin, pool):
        lead = p.open()
        got = [_pool_step(p, [(lead, *clips[0])], 2)[lead], _ragged_step(p, [(lead, *clips[0])], [2])[lead]]
        if p is pool:
            held = pool.pages_of(lead)
            assert sorted(held) == [0, 1] and pool.pages_free == 0
        p.close(lead)
        if p is pool:
            assert pool.pages_free == 2
            pool._st.k_cache[:, list(held)] = float('nan')
            pool._st.v_cache[:, list(held)] = float('nan')
        new = p.open()
        got += [_ragged_step(p, [(new, *clips[1])], [1])[new], _pool_step(p, [(new, *clips[1])], 1)[new], _ragged_step(p, [(new, *clips[1])], [2])[new]]
        if p is pool:
            assert sorted(pool.pages_of(new)) == [0, 1]
        outs.append(got)
    for k, ((m, f), (wm, wf)) in enumerate(zip(outs[1], outs[0])):
        assert torch.isfinite(m).all() and torch.isfinite(f).all(), k
        assert torch.equal(m, wm) and torch.equal(f, wf), k
    assert not torch.equal(outs[0][0][0], torch.cat([outs[0][2][0], outs[0][3][0]], 2))     # the two tenants' outputs differ


def test_default_pool_is_untouched_by_paged_pools(cuda):
    """stream_pool(capacity) without the keywords still builds the contiguous state, and gives the same bits before and after a paged pool ran."""
    net = _small_net('bf16')
    clips = _small_clips(4)
    pool = net.stream_pool(3)
    assert type(pool._st) is stream._State and pool.page_frames is None
    assert tuple(pool._st.k_cache.shape[1:]) == (3, pool._st.k_cache.shape[2], 4, 4, 64)
    before = _schedule(pool, clips)
    _schedule(net.stream_pool(3, page_frames=2), clips)
    after = _schedule(net.stream_pool(3), clips)
    for (m, f), (wm, wf) in zip(after, before):
        assert torch.equal(m, wm) and torch.equal(f, wf)

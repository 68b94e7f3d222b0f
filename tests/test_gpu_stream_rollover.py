"""GPU: a stream pool whose sessions run past the last frame (stream_pool(rollover=k), tcow_amd/stream.py) -- the re-query kernel against torch,
the chain of windows against forward() of every window, the bit-exact twins (step / step_ragged, contiguous / paged, fp8 cache), chunks that
cross hand-offs, the number of Seeker steps per call, and the page and slot lifecycle.

The chain tests build every window's query from the pool's OWN hand-off masks: logits within 1e-6 of zero occur at every hand-off of this input
(CPU oracle: the per-plane min |logit| is 5e-9 .. 7e-6), so two correct implementations may disagree on a pixel; what is exact is that the mask
is the threshold of the logits the pool returned.  Sensitivity (CPU oracle, max |d| of the window's logits): one flipped mask pixel 3.5e-3, the
neighbouring frame's mask 3.1e-2 .. 3.4e-2, a zero mask 5.8e-2 .. 6.0e-2 (flags 0.16 .. 0.18) -- the fp32 leg (2e-5) sees one wrong pixel, the bf16
leg (1.5e-2) a wrong frame or a missing mask."""
import functools

import pytest
import torch

from stream_kit import _small_net
from tcow_amd import engine, ops, synth
from tcow_amd._lib import TcowError

pytestmark = pytest.mark.gpu

T = 4                                                           # of _small_net
TOL = {'fp32': 2e-5, 'bf16': 1.5e-2}                            # that config's stream-vs-forward tolerances


# ---------------------------------------------------------------------------------------------- kernel

def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize('thr', [0.0, 0.25])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('plane', [1, 3, 4, 63, 64, 65, 4097, 6144])
def test_requery_kernel_vs_torch(cuda, plane, n, thr):
    dev = torch.device('cuda')
    g = torch.Generator(device=dev).manual_seed(plane * 7 + n)
    logits = torch.randn(n * plane + 5, device=dev, generator=g)
    t = torch.tensor(thr, dtype=torch.float32)
    special = torch.stack([torch.tensor(v, dtype=torch.float32) for v in (0.0, -0.0, thr, float('nan'), float('inf'), float('-inf'), 1e-40, -1e-40)]
                          + [torch.nextafter(t, torch.tensor(float('inf'))), torch.nextafter(t, torch.tensor(float('-inf')))]).to(dev)
    for i in range(n):                                          # at the start and at the end of every plane (the vector body and the scalar tail)
        m = min(plane, special.numel())
        logits[i * plane:i * plane + m] = special[:m]
        logits[(i + 1) * plane - m:(i + 1) * plane] = special[:m].flip(0)
    n_dst = n + 2
    rows = [int(v) for v in torch.randperm(n_dst, generator=torch.Generator().manual_seed(n + plane))[:n]]
    # n hand-offs (plane i starts at i * plane: an odd plane makes the later ones misaligned), then three that must write nothing: a row past
    # the end, a negative row, and a plane that does not lie inside logits
    spare = next(r for r in range(n_dst) if r not in rows)
    src = [i * plane for i in range(n)] + [0, 0, logits.numel() - plane + 1, -1]
    dst = rows + [n_dst, -1, spare, spare]
    mask = torch.full((n_dst, plane), float('nan'), device=dev)
    pixels = torch.full((n_dst,), -1, dtype=torch.int32, device=dev)
    want_m, want_p = mask.clone(), pixels.clone()
    for i, r in enumerate(rows):
        b = logits[i * plane:(i + 1) * plane] > thr
        want_m[r] = b.float()
        want_p[r] = int(b.sum())
    ops.requery_mask(logits, torch.tensor(src, dtype=torch.int64, device=dev), thr, mask, torch.tensor(dst, dtype=torch.int32, device=dev), pixels)
    assert torch.equal(_bits(mask), _bits(want_m)), (plane, n, thr, rows)          # bits: the unnamed rows are still NaN
    assert torch.equal(pixels, want_p), (plane, n, thr, rows, pixels.tolist(), want_p.tolist())
    # overwritten, not accumulated: the same launch again gives the same counts
    ops.requery_mask(logits, torch.tensor(src, dtype=torch.int64, device=dev), thr, mask, torch.tensor(dst, dtype=torch.int32, device=dev), pixels)
    assert torch.equal(pixels, want_p) and torch.equal(_bits(mask), _bits(want_m))


def test_requery_kernel_refuses_bad_arguments(cuda):
    dev = torch.device('cuda')
    logits = torch.zeros(64, device=dev); mask = torch.zeros(2, 16, device=dev); pixels = torch.zeros(2, dtype=torch.int32, device=dev)
    src = torch.zeros(1, dtype=torch.int64, device=dev); dst = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.requery_mask(logits, src, 0.0, mask, dst, pixels)
    for bad in (float('nan'), float('inf'), float('-inf')):
        with pytest.raises(TcowError, match='finite'):
            ops.requery_mask(logits, src, bad, mask, dst, pixels)
    with pytest.raises(TcowError, match='n=0'):
        ops.requery_mask(logits, src[:0], 0.0, mask, dst[:0], pixels)
    with pytest.raises(TcowError, match='plane'):
        ops.requery_mask(logits, src, 0.0, mask[:, :0].contiguous(), dst, pixels)
    with pytest.raises(TcowError, match='logits_len'):
        ops.requery_mask(logits[:8], src, 0.0, mask, dst, pixels)
    with pytest.raises(TcowError, match='CUDA'):
        ops.requery_mask(logits.cpu(), src, 0.0, mask, dst, pixels)
    for a in ((logits.double(), src, 0.0, mask, dst, pixels), (logits, src.int(), 0.0, mask, dst, pixels), (logits, src, 0.0, mask, dst.long(), pixels),
              (logits, src, 0.0, mask, dst, pixels.long()), (logits, src, 0.0, mask, dst, pixels[:1]), (logits, src, 0.0, mask.view(-1), dst, pixels)):
        with pytest.raises(TcowError, match='requery_mask'):
            ops.requery_mask(*a)
    # the library's own refusals, with pointers that are not null
    from tcow_amd import _lib
    lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    args = lambda **kw: [kw.get(k, v) for k, v in (('stream', st), ('n', 1), ('plane', 16), ('logits', logits.data_ptr()), ('len', 64), ('src', src.data_ptr()),
                                                   ('thr', 0.0), ('mask', mask.data_ptr()), ('dst', dst.data_ptr()), ('n_dst', 2), ('pixels', pixels.data_ptr()))]
    assert lib.tcow_requery_mask(*args()) == 0
    for kw, text in (({'n': 0}, 'n=0'), ({'n': -1}, 'n=-1'), ({'plane': 0}, 'plane=0'), ({'n_dst': 0}, 'n_dst=0'), ({'len': 15}, 'logits_len=15'),
                     ({'thr': float('nan')}, 'finite'), ({'logits': None}, 'null'), ({'src': None}, 'null'), ({'mask': None}, 'null'), ({'dst': None}, 'null'),
                     ({'pixels': None}, 'null')):
        assert lib.tcow_requery_mask(*args(**kw)) != 0 and text in lib.tcow_last_error().decode(), kw
    torch.cuda.synchronize()
    assert int(pixels.sum()) == 0 and float(mask.sum()) == 0.0


# ---------------------------------------------------------------------------------------------- the chain of windows

@functools.lru_cache(maxsize=None)
def _clip():
    """Two clips of 10 frames with their frame-0 query masks, on the device; shared and never written."""
    clip = synth.make_clip(2, 10, 64, 96, seed=5)
    return torch.from_numpy(clip['rgb']).cuda(), torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()


def _frames(k):
    """Three windows: k = 1 -> windows at 0, 3, 6 (10 frames), k = 2 -> 0, 2, 4 (8 frames)."""
    return 2 * (T - k) + T


def _feed(pool, feeds, chunks, ragged=False):
    """feeds: [(session, rgb (1,3,G,H,W), qm (1,1,G,H,W))], all at the frame pool.frames_done says; chunks: [c per session] -> per session
    (mask logits, flags) of those frames, and {hand-off frame: (requery mask, pixels)} for the hand-offs this call made."""
    ids = [f[0] for f in feeds]
    g0 = [pool.frames_done(i) for i in ids]
    cut = lambda x, g, c: x[:, :, g:g + c]
    if ragged:
        ms, fs = pool.step_ragged(ids, [cut(f[1], g, c) for f, g, c in zip(feeds, g0, chunks)], [cut(f[2], g, c) for f, g, c in zip(feeds, g0, chunks)])
    else:
        assert len(set(chunks)) == 1
        m, fl = pool.step(ids, torch.cat([cut(f[1], g, chunks[0]) for f, g in zip(feeds, g0)], 0), torch.cat([cut(f[2], g, chunks[0]) for f, g in zip(feeds, g0)], 0))
        ms, fs = [m[i:i + 1] for i in range(len(ids))], [fl[i:i + 1] for i in range(len(ids))]
    out, s = {}, T - pool.rollover
    for i, g, c, m, fl in zip(ids, g0, chunks, ms, fs):
        assert tuple(m.shape) == (1, 3, c, 64, 96) and tuple(fl.shape[:2]) == (1, c) and m.dtype == torch.float32
        assert pool.frames_done(i) == g + c and pool.window(i) == pool.plan.window(g + c)
        hand = {h: (pool.requery_mask(i), pool.requery_pixels(i)) for h in range(g, g + c) if h >= s and h % s == 0}
        out[i] = (m, fl, hand)
    return out


def _session(pool, sid, rgb, qm, chunks, ragged=False):
    """One session alone: (mask logits, flags, {hand-off frame: (mask, pixels)}) of sum(chunks) frames."""
    ms, fs, hand = [], [], {}
    for c in chunks:
        m, fl, h = _feed(pool, [(sid, rgb, qm)], [c], ragged)[sid]
        ms.append(m); fs.append(fl); hand.update(h)
    return torch.cat(ms, 2), torch.cat(fs, 1), hand


def _check_handoffs(om, hand, k, frames):
    """(a): every hand-off's mask is the threshold of the logits the pool itself returned for that frame, bit for bit, and the count is its sum.
    First the precondition of the whole chain test: a mask that is neither empty nor full (the original query covers 4 .. 6 %)."""
    s = T - k
    assert sorted(hand) == [h for h in range(s, frames) if h % s == 0]
    for h, (mask, pixels) in hand.items():
        assert tuple(mask.shape) == (1, 1, 1, 64, 96) and mask.dtype == torch.float32 and mask.is_cuda and pixels.dtype == torch.int32 and pixels.is_cuda
        frac = float(mask.mean())
        print('hand-off', h, 'ones', frac)
        assert 0.05 <= frac <= 0.95, (h, frac)
    for h, (mask, pixels) in hand.items():
        assert torch.equal(mask, (om[:, 0:1, h:h + 1] > 0).float()[:, :, None].reshape(1, 1, 1, 64, 96)), h
        assert int(pixels) == int(mask.sum()), h


def _check_chain(net, rgb, qm, om, fl, hand, k, tol, tag):
    """(b): the reported outputs are forward() of every window -- its frames, the caller's query frames, local frame 0 replaced by the pool's own
    hand-off mask -- window 0 whole, a later window from its local frame k on."""
    s, frames = T - k, om.shape[2]
    g = 0
    with torch.no_grad():
        for w in range((frames - T) // s + 1):
            q = qm[:, :, w * s:w * s + T].clone()
            if w:
                q[:, :, 0:1] = hand[w * s][0][:, :, 0]
            rm, rf = net(rgb[:, :, w * s:w * s + T], q)
            lo = k if w else 0
            n = T - lo
            d, df = float((om[:, :, g:g + n] - rm[:, :, lo:]).abs().max()), float((fl[:, g:g + n] - rf[:, lo:]).abs().max())
            print('chain', tag, 'window', w, 'frames', g, '..', g + n - 1, d, df)
            assert d < tol and df < tol, (tag, w, d, df)
            g += n
    assert g == frames


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('ca', [1, 2])
@pytest.mark.parametrize('k', [1, 2])
def test_chain_frame_by_frame_equals_forward_of_every_window(cuda, k, ca, precision):
    net = _small_net(precision, ca)
    rgb, qm = _clip()
    frames = _frames(k)
    pool = net.stream_pool(4, rollover=k)
    a, b = pool.open(), pool.open()
    got = {a: ([], [], {}), b: ([], [], {})}
    for _ in range(frames):                                     # both sessions in every step, one frame per call
        for i, (m, fl, h) in _feed(pool, [(a, rgb[0:1], qm[0:1]), (b, rgb[1:2], qm[1:2])], [1, 1]).items():
            got[i][0].append(m); got[i][1].append(fl); got[i][2].update(h)
    for row, i in enumerate((a, b)):
        om, fl, hand = torch.cat(got[i][0], 2), torch.cat(got[i][1], 1), got[i][2]
        _check_handoffs(om, hand, k, frames)
        _check_chain(net, rgb[row:row + 1], qm[row:row + 1], om, fl, hand, k, TOL[precision], (k, ca, precision, row))


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_chunks_that_cross_hand_offs_and_a_session_that_joins_later(cuda, precision):
    k, frames = 1, 10
    net = _small_net(precision)
    rgb, qm = _clip()
    pool = net.stream_pool(4, rollover=k)
    a = pool.open()
    plan = {0: [3], 1: [1], 2: [2, 2], 3: [3, 2], 4: [1, 3], 5: [None, 3]}      # call -> [frames of a, frames of b]; b opens two calls later
    got, b = {a: ([], [], {})}, None
    for call in range(6):
        if call == 2:
            b = pool.open()
            got[b] = ([], [], {})
        feeds = [(i, rgb[r:r + 1], qm[r:r + 1], c) for r, (i, c) in enumerate(zip((a, b), plan[call] + [None])) if i is not None and c is not None]
        for i, (m, fl, h) in _feed(pool, [f[:3] for f in feeds], [f[3] for f in feeds], ragged=True).items():
            got[i][0].append(m); got[i][1].append(fl); got[i][2].update(h)
    for row, i in enumerate((a, b)):
        om, fl, hand = torch.cat(got[i][0], 2), torch.cat(got[i][1], 1), got[i][2]
        assert om.shape[2] == frames
        _check_handoffs(om, hand, k, frames)
        _check_chain(net, rgb[row:row + 1], qm[row:row + 1], om, fl, hand, k, TOL[precision], ('chunked', precision, row))


# ---------------------------------------------------------------------------------------------- bit-exact twins

def _two_sessions(net, chunks, ragged, **kw):
    """Both clips as two sessions of a fresh pool, fed `chunks` together -> everything the pool gave, in one list."""
    rgb, qm = _clip()
    pool = net.stream_pool(4, rollover=1, **kw)
    a, b = pool.open(), pool.open()
    out = []
    for c in chunks:
        r = _feed(pool, [(a, rgb[0:1], qm[0:1]), (b, rgb[1:2], qm[1:2])], [c, c], ragged)
        for i in (a, b):
            out += [r[i][0], r[i][1]] + [t for h in sorted(r[i][2]) for t in r[i][2][h]]
    return out


def _same(x, y):
    assert len(x) == len(y) and len(x) > 20
    for i, (p, q) in enumerate(zip(x, y)):
        assert torch.equal(p, q), i


def test_twins_step_ragged_and_paged_are_bit_identical(cuda):
    net = _small_net('bf16')
    chunks = [2, 2, 3, 1, 2]                                    # hand-offs 3 and 6: each ends a chunk, and the retained frame opens the next call
    base = _two_sessions(net, chunks, False)
    _same(base, _two_sessions(net, chunks, True))
    _same(base, _two_sessions(net, chunks, False, page_frames=1))
    _same(base, _two_sessions(net, chunks, True, page_frames=2))
    other = [3, 3, 3, 1]                                        # hand-off 3 opens a chunk, hand-off 6 too: two Seeker steps each
    base = _two_sessions(net, other, False)
    _same(base, _two_sessions(net, other, True, page_frames=2))
    _same(base, _two_sessions(net, other, False, page_frames=1))


def test_twins_fp8_cache_paged_and_contiguous(cuda):
    net = _small_net('bf16')
    chunks = [3, 1, 2, 3, 1]
    _same(_two_sessions(net, chunks, True, cache_dtype='fp8'), _two_sessions(net, chunks, True, cache_dtype='fp8', page_frames=2))


# ---------------------------------------------------------------------------------------------- scheduling

def test_one_seeker_step_unless_a_chunk_goes_on_after_its_hand_off_frame(cuda, monkeypatch):
    net = _small_net('bf16')
    rgb, qm = _clip()
    calls = []
    real = engine.run_forward

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(engine, 'run_forward', counted)

    def steps(pool, feeds, chunks):
        del calls[:]
        _feed(pool, feeds, chunks, ragged=True)
        return len(calls)

    for k in (1, 2):
        pool = net.stream_pool(4, rollover=k)
        a, b = pool.open(), pool.open()
        for g in range(_frames(k)):                             # a camera: one frame per call, hand-off frames included
            assert steps(pool, [(a, rgb[0:1], qm[0:1]), (b, rgb[1:2], qm[1:2])], [1, 1]) == 1, (k, g)
    pool = net.stream_pool(4, rollover=1)                       # hand-offs at 3 and 6
    a, b = pool.open(), pool.open()
    A, B = (a, rgb[0:1], qm[0:1]), (b, rgb[1:2], qm[1:2])
    assert steps(pool, [A, B], [2, 3]) == 1                     # a: 0-1; b: 0-2
    assert steps(pool, [A, B], [2, 1]) == 1                     # a: 2-3, the hand-off frame ends the chunk; b: 3, the same
    assert steps(pool, [A, B], [1, 2]) == 1                     # both start with the retained frame
    assert steps(pool, [A, B], [3, 1]) == 2                     # a: 5-7 goes on after hand-off frame 6; b: 6 alone
    assert steps(pool, [A], [2]) == 1                           # a: 8-9
    assert steps(pool, [B], [3]) == 1                           # b: 7-9, the retained frame first
    assert pool.frames_done(a) == 10 and pool.frames_done(b) == 10
    pool.reset(a)
    assert steps(pool, [A], [3]) == 1 and steps(pool, [A], [3]) == 2          # 0-2; 3-5: hand-off frame 3 opens the chunk
    with pytest.raises(TcowError, match='chunk'):
        pool.step_ragged([a], [rgb[0:1, :, 0:4]], [qm[0:1, :, 0:4]])            # c = 4 > T - k = 3: refused before anything moves
    assert pool.frames_done(a) == 6


# ---------------------------------------------------------------------------------------------- pages and slots

@pytest.mark.parametrize('P', [1, 2])
def test_pages_follow_the_windows(cuda, P):
    k = 2
    net = _small_net('bf16')
    rgb, qm = _clip()
    ceil = lambda x, y: -(-x // y)
    peak = ceil(T, P) + ceil(k, P)
    pool = net.stream_pool(4, rollover=k, page_frames=P)
    assert pool.pages_total == 2 * peak                         # capacity / 2 sessions at their peak
    a = pool.open()
    most = 0
    for g in range(_frames(k)):
        _feed(pool, [(a, rgb[0:1], qm[0:1])], [1])
        own = pool.pages_of(a)
        assert len(set(own)) == len(own) and pool.pages_free + len(own) == pool.pages_total
        # after the call of frame g: the windows that have not ended, by what they have been given (window w + 1 starts with the call after its
        # hand-off frame)
        want = sum(ceil(min(g, w * 2 + T - 1) - w * 2 + 1, P) for w in range(5) if g > w * 2 - (w == 0) and g < w * 2 + T - 1)
        assert len(own) == want, (g, own, want)
        most = max(most, len(own) + (ceil(T, P) if g >= T - 1 and (g - k) % 2 == 1 else 0))      # + the window that this call ended
    assert most == peak
    pool.close(a)
    assert pool.pages_free == pool.pages_total


def test_a_call_short_of_pages_moves_nothing(cuda):
    k, P = 2, 1
    net = _small_net('bf16')
    rgb, qm = _clip()
    A = lambda i: (i, rgb[0:1], qm[0:1])
    B = lambda i: (i, rgb[1:2], qm[1:2])
    pool, twin = net.stream_pool(4, rollover=k, page_frames=P, pages=8), net.stream_pool(4, rollover=k, page_frames=P)
    a, b = pool.open(), pool.open()
    ta, tb = twin.open(), twin.open()
    for _ in range(3):                                          # frames 0 .. 2: three pages each
        _feed(pool, [A(a), B(b)], [1, 1]); _feed(twin, [A(ta), B(tb)], [1, 1])
    assert pool.pages_free == 2
    # frame 3: window 0 needs its fourth page and window 1 starts with the retained frame 2 and frame 3: three pages each, two are free
    before = (pool.frames_done(a), pool.frames_done(b), pool.pages_free, pool.window(a), pool.pages_of(a), pool.pages_of(b))
    with pytest.raises(TcowError, match='out of pages'):
        _feed(pool, [A(a), B(b)], [1, 1])
    assert before == (pool.frames_done(a), pool.frames_done(b), pool.pages_free, pool.window(a), pool.pages_of(a), pool.pages_of(b))
    with pytest.raises(TcowError, match='out of pages'):
        _feed(pool, [A(a)], [1])
    pool.close(b); twin.close(tb)
    assert pool.pages_free == 5
    for _ in range(4):                                          # the same call now succeeds, and the session runs on as in a pool that never ran short
        x, y = _feed(pool, [A(a)], [1])[a], _feed(twin, [A(ta)], [1])[ta]
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and sorted(x[2]) == sorted(y[2])
        for h in x[2]:
            assert torch.equal(x[2][h][0], y[2][h][0]) and torch.equal(x[2][h][1], y[2][h][1])


@pytest.mark.parametrize('how', ['close', 'reset'])
@pytest.mark.parametrize('P', [None, 2])
def test_reset_and_close_mid_overlap_free_both_windows(cuda, how, P):
    """The pattern of test_pool_slot_reuse_reads_nothing_of_the_previous_tenant: the new tenant of the two slots equals a fresh pool bit for bit."""
    k = 2
    net = _small_net('bf16')
    rgb, qm = _clip()
    kw = {} if P is None else {'page_frames': P}
    fresh = net.stream_pool(2, rollover=k, **kw)
    want = _session(fresh, fresh.open(), rgb[1:2], qm[1:2], [1] * 8)
    pool = net.stream_pool(2, rollover=k, **kw)                 # two slots: one session
    a = pool.open()
    with pytest.raises(TcowError, match='takes two'):
        pool.open()
    _session(pool, a, rgb[0:1], qm[0:1], [1] * 5)               # frames 0 .. 4: window 1 is live, window 2 waits with its mask and the retained frame 4
    assert pool.window(a) == 1 and int(pool.requery_pixels(a)) > 0
    if how == 'close':
        pool.close(a)
        with pytest.raises(TcowError, match='not open'):
            pool.requery_mask(a)
        a = pool.open()                                         # both slots were free again
    else:
        pool.reset(a)
    assert pool.frames_done(a) == 0 and pool.window(a) == 0
    with pytest.raises(TcowError, match='no hand-off'):
        pool.requery_mask(a)
    if P is not None:
        assert pool.pages_free == pool.pages_total
    got = _session(pool, a, rgb[1:2], qm[1:2], [1] * 8)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and sorted(got[2]) == sorted(want[2]) == [2, 4, 6]
    for h in got[2]:
        assert torch.equal(got[2][h][0], want[2][h][0]) and torch.equal(got[2][h][1], want[2][h][1])


def test_a_pool_without_the_keyword_ends_at_the_last_frame(cuda):
    net = _small_net('bf16')
    rgb, qm = _clip()
    pool = net.stream_pool(2)
    assert type(pool).__name__ == 'SeekerStreamPool' and not hasattr(pool, 'requery_mask')
    a = pool.open()
    pool.step([a], rgb[0:1, :, 0:4], qm[0:1, :, 0:4])
    with pytest.raises(TcowError, match=r'stream_pool\.step: session 0: frames 4\.\.4 run past the last frame 3 of the stream \(num_total_frames = 4\); '
                                        r'reset\(\) or close\(\) it'):
        pool.step([a], rgb[0:1, :, 4:5], qm[0:1, :, 4:5])
    assert pool.frames_done(a) == 4
    st = net.stream()
    st.step(rgb[0:1, :, 0:4], qm[0:1, :, 0:4])
    with pytest.raises(TcowError, match=r'run past the last frame 3 .*stream_pool\(capacity, rollover=k\)'):
        st.step(rgb[0:1, :, 4:5], qm[0:1, :, 4:5])

"""CPU: the host side of a rollover stream pool (stream_pool(rollover=k), tcow_amd/stream.py) -- the window arithmetic of RolloverPlan by brute
force, the split of a chunk into Seeker steps, the keyword refusals, the page default, and the ABI entry of the re-query kernel."""
import os
import re

import pytest

from stream_kit import _net
from tcow_amd import _lib, stream
from tcow_amd._lib import TcowError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(T, k) for T in (4, 5, 30) for k in range(1, T // 2 + 1)]


def _spans(T, k, G):
    """Window w covers w*s .. w*s + T - 1, stated apart from the plan: {g: [w, ...]} for g < G."""
    s = T - k
    return {g: [w for w in range(G // s + 2) if w * s <= g <= w * s + T - 1] for g in range(G)}


@pytest.mark.parametrize('T,k', CASES)
def test_every_frame_is_reported_once_and_never_from_a_warm_up_frame(T, k):
    plan, s, G = stream.RolloverPlan(T, k), T - k, 4 * T
    spans = _spans(T, k, G)
    for g in range(G):
        # reported exactly once: one window of those that cover g has it outside its warm-up frames (window 0 has none)
        reporters = [w for w in spans[g] if w == 0 or g - w * s >= k]
        assert reporters == [plan.window(g)], (g, spans[g])
        w = plan.window(g)
        assert w == 0 or g - w * s >= k
        assert 0 <= g - w * s < T
        live = plan.live(g)
        assert list(live) == spans[g] and 1 <= len(live) <= 2
        assert plan.is_handoff(g) == (g >= s and g % s == 0)
        if plan.is_handoff(g):                                  # the older window reports the hand-off frame; the newer starts there
            assert plan.window(g) == g // s - 1 and live == (g // s - 1, g // s)


@pytest.mark.parametrize('T,k', CASES)
def test_chunk_splits(T, k):
    """Every start and every allowed chunk length: one part unless a frame follows the hand-off frame, never three; every window gets each frame
    of its span exactly once, in order, over consecutive calls; the report runs are the chunk's frames from their reporting windows."""
    plan, s, G = stream.RolloverPlan(T, k), T - k, 4 * T
    for g0 in range(G):
        for c in range(1, s + 1):
            sp = plan.split(g0, c)
            hs = [g for g in range(g0, g0 + c) if g >= s and g % s == 0]
            assert len(hs) <= 1 and sp['handoff'] == (hs[0] if hs else None)
            follows = bool(hs) and hs[0] < g0 + c - 1
            assert len(sp['parts']) == (2 if follows else 1)
            assert sp['keep'] == (bool(hs) and not follows)
            want = [(plan.window(g), g) for g in range(g0, g0 + c)]
            got = [(w, g + j) for p, w, g, n in sp['report'] for j in range(n)]
            assert got == want
            for p, w, g, n in sp['report']:                     # the run lies inside a row of that window in that part
                row = [r for r in sp['parts'][p] if r[0] == w]
                assert len(row) == 1 and row[0][3] <= g and g + n <= row[0][3] + row[0][2]
            for part in sp['parts']:
                assert len({r[0] for r in part}) == len(part) <= 2
                for w, t0, n, g in part:
                    assert n >= 1 and t0 == g - w * s and 0 <= t0 and t0 + n <= T
    for c in sorted({1, 2, s} & set(range(1, s + 1))):           # a session fed in chunks of c: what each window has been given
        fed, g0 = {}, 0
        while g0 < G:
            sp = plan.split(g0, c)
            for p, part in enumerate(sp['parts']):
                for w, t0, n, g in part:
                    assert len(fed.setdefault(w, [])) == t0, (c, g0, w)       # appended in order, nothing twice, nothing skipped
                    fed[w] += range(g, g + n)
                    if w >= 1 and t0 == 0:                      # a window starts only after its hand-off frame has been through the older one
                        assert g == w * s and (p == 1 or g == g0 - 1)
            g0 += c
        for w, frames in fed.items():
            assert frames == list(range(w * s, w * s + len(frames))) and len(frames) <= T
            if (w + 1) * s + k <= g0 - c:                       # windows that must have ended by now are complete
                assert len(frames) == T


def _call(plan, g0s, cs, keep, fed, handed):
    """One call of a rollover pool as SeekerRolloverPool._roll runs a RolloverCall, with lists of frame ids in place of tensors and a stand-in
    forward that returns (session, window, local frame) per flat frame.  Session i stands at g0s[i] and brings cs[i] frames; keep[i]: the frame
    it retained or None, fed[i]: {window: frames given so far}, handed[i]: the windows whose hand-off mask has been made -- all updated."""
    s, n = plan.s, len(g0s)
    call = stream.RolloverCall(plan, g0s, cs)
    chunks = [list(range(g0, g0 + c)) for g0, c in zip(g0s, cs)]
    outs = []
    for p, rows in enumerate(call.parts):
        first = stream.ragged_tables([r.t0 for r in rows], [0] * len(rows), [r.c for r in rows])['first']
        out = []
        for r, f0 in zip(rows, first):
            assert r.first == f0 == len(out) and r.t0 == r.g - r.w * s
            frames = ([keep[r.k]] if r.kept else []) + chunks[r.k][r.lo:r.hi]
            assert frames == list(range(r.g, r.g + r.c))        # exactly its frames, in order, the retained frame included
            assert fed[r.k].get(r.w, 0) == r.t0                 # nothing twice, nothing skipped
            fed[r.k][r.w] = r.t0 + r.c
            queries = (['hand-off'] if r.handed else []) + [('caller', g) for g in chunks[r.k][r.qlo:r.hi]]
            want = [('caller', g) for g in frames]
            if r.w >= 1 and r.t0 == 0:                          # a window >= 1: the hand-off mask at its local frame 0, made before this part
                want[0] = 'hand-off'
                assert r.w in handed[r.k]
            assert queries == want
            out += [(r.k, r.w, r.t0 + j) for j in range(r.c)]
        outs.append(out)
        if p == 0:
            for i, born, f in call.handoffs:                    # the source: where window born - 1 processed the hand-off frame
                assert born * s in chunks[i] and out[f] == (i, born - 1, born * s - (born - 1) * s)
                handed[i].add(born)
    assert [i for i, _, _ in call.handoffs] == [i for i in range(n) if any(plan.is_handoff(g) for g in chunks[i])]
    follows = any(plan.is_handoff(g) for ch in chunks for g in ch[:-1])
    assert len(call.parts) == (2 if follows else 1)
    for i in range(n):
        assert call.keep[i] == plan.is_handoff(chunks[i][-1])
        keep[i] = chunks[i][-1] if call.keep[i] else None
        reported = [outs[p][f + j] for p, f, c in call.report[i] for j in range(c)]
        assert reported == [(i, plan.window(g), g - plan.window(g) * s) for g in chunks[i]]
    return call


@pytest.mark.parametrize('T,k', CASES)
def test_a_call_feeds_every_window_and_reports_every_frame(T, k):
    """RolloverCall by brute force (_call above holds the assertions): every start g0 < 4T with every allowed c, beside a second session out of
    phase, from the state that one frame per call leaves; then two sessions fed in chunks of 1, 2 and s, the second a call behind."""
    plan, s, G = stream.RolloverPlan(T, k), T - k, 4 * T
    keep, fed, handed, snap = [None], [{}], [set()], []
    for g in range(G):
        snap.append((keep[0], dict(fed[0]), set(handed[0])))
        _call(plan, [g], [1], keep, fed, handed)
    for g0 in range(G):
        for c in range(1, s + 1):
            g1, c1 = (g0 + 2) % G, 1 + (g0 + c) % s
            _call(plan, [g0, g1], [c, c1], [snap[g0][0], snap[g1][0]], [dict(snap[g0][1]), dict(snap[g1][1])], [set(snap[g0][2]), set(snap[g1][2])])
    for c in sorted({1, 2, s}):
        keep, fed, handed, done = [None, None], [{}, {}], [set(), set()], [0, 0]
        for call_no in range(G // c):
            live = [0] if call_no == 0 else [1, 0]
            kp = [keep[i] for i in live]
            _call(plan, [done[i] for i in live], [c] * len(live), kp, [fed[i] for i in live], [handed[i] for i in live])
            for j, i in enumerate(live):
                keep[i], done[i] = kp[j], done[i] + c
        for i in (0, 1):
            assert sorted(fed[i]) == list(range(len(fed[i]))) and len(fed[i]) >= 3
            for w, count in fed[i].items():
                assert count <= T
                if (w + 1) * s + k <= done[i] - c:              # windows that must have ended by now are complete
                    assert count == T


def test_refusals():
    for T in (4, 5, 30):
        for k in (0, -1, T // 2 + 1, T, 1.5, True):
            with pytest.raises(TcowError, match='rollover'):
                stream.RolloverPlan(T, k)
    plan = stream.RolloverPlan(5, 2)
    for c in (0, 4, 9):
        with pytest.raises(TcowError, match='chunk'):
            plan.split(0, c)
    plan.split(7, 3)
    net = _net().eval()
    with pytest.raises(TcowError, match='rollover'):
        net.stream_pool(2, rollover=0)
    with pytest.raises(TcowError, match='rollover'):
        net.stream_pool(2, rollover=3)                          # T = 4: k <= 2
    with pytest.raises(TcowError, match='capacity'):
        net.stream_pool(1, rollover=1)
    for bad in (float('nan'), float('inf'), float('-inf'), 'x', None):
        with pytest.raises(TcowError, match='requery_threshold'):
            net.stream_pool(2, rollover=1, requery_threshold=bad)
    with pytest.raises(TcowError, match='page_frames'):
        net.stream_pool(2, rollover=1, page_frames=3)
    with pytest.raises(TcowError, match='CPU'):                 # every keyword accepted: what is left is that streams run on the GPU
        net.stream_pool(2, rollover=2, requery_threshold=0.25, page_frames=2)
    with pytest.raises(TcowError, match='CPU'):                 # without the keyword: the pool as it was
        net.stream_pool(1)


def test_page_default_and_peak():
    ceil = lambda a, b: -(-a // b)
    for T, k in CASES:
        for P in (1, 2, 8):
            for capacity in (2, 3, 8):
                peak = ceil(T, P) + ceil(k, P)
                assert stream.rollover_pages(capacity, T, k, P, None) == (P, ceil(capacity * peak, 2))
                assert stream.rollover_pages(capacity, T, k, P, 7) == (P, 7)
            # one frame per call: the pages a session holds while a call runs, from the plan alone (a window's pages return after the call
            # that brings its last frame).  k = 1: the next window starts only with the call after its hand-off frame, which is the older
            # window's last, so the two never hold pages together and the formula is an upper bound.
            plan, held, most = stream.RolloverPlan(T, k), {}, 0
            for g0 in range(4 * T):
                sp = plan.split(g0, 1)
                assert len(sp['parts']) == 1
                for w, t0, n, _ in sp['parts'][0]:
                    held[w] = ceil(t0 + n, P)
                most = max(most, sum(held.values()))
                for w, t0, n, _ in sp['parts'][0]:
                    if t0 + n == T:
                        del held[w]
            assert most == (peak if k >= 2 else ceil(T, P)), (T, k, P)
    assert stream.rollover_pages(4, 30, 3, None, None) == (None, None)


def test_requery_abi_entry():
    hdr = open(os.path.join(ROOT, 'include', 'tcow_hip.h')).read()
    assert int(re.search(r'#define\s+TCOW_ABI_VERSION\s+(\d+)', hdr).group(1)) == 16 and _lib.ABI_VERSION == 16
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    decl = re.search(r'\bint\s+tcow_requery_mask\s*\(([^;]*)\)\s*;', code)
    assert decl, 'tcow_requery_mask is not declared in tcow_hip.h'
    assert len(decl.group(1).split(',')) == len(_lib.SIGNATURES['tcow_requery_mask'][1]) == 11
    for fmt in ('bf16', 'fp16'):
        lib = _lib.lib(fmt)
        assert lib.tcow_version() == 16
        assert hasattr(lib, 'tcow_requery_mask'), f'tcow_requery_mask is not exported by the {fmt} build'
        assert lib.tcow_requery_mask.argtypes == _lib.SIGNATURES['tcow_requery_mask'][1]

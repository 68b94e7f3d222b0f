"""CPU: the host side of a paged stream pool (stream_pool(page_frames=P, pages=N), tcow_amd/stream.py) -- the page allocator against a set-based
model, the page moves of a rollover call against the accounting they replaced, the keyword checks, and the ABI entry of the paged attention kernel."""
import ctypes
import os
import re

import numpy as np
import pytest

import stream_abi as abi
from stream_kit import _net
from tcow_amd import _lib, stream
from tcow_amd._lib import TcowError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- allocator

def test_allocator_hands_out_the_lowest_free_page_first_in_frame_order():
    a = stream.PageAllocator(8, 4)
    assert a.free == 8 and a.pages_of('x') == ()
    assert a.grow(['x', 'y'], [1, 9]) == [(0,), (1, 2, 3)]                      # session by session in the order given, lowest page first
    assert a.grow(['y', 'x'], [12, 8]) == [(1, 2, 3), (0, 4)]                   # y has room for frames 9..11; x's second page holds its frames 4..7
    assert a.pages_of('x') == (0, 4) and a.pages_of('y') == (1, 2, 3) and a.free == 3
    a.release('y')
    assert a.free == 6 and a.pages_of('y') == ()
    assert a.grow(['z'], [5]) == [(1, 2)]                                       # the freed pages are the lowest again
    assert a.grow(['x'], [9]) == [(0, 4, 3)]
    a.release('nobody')                                                         # a session without pages: nothing happens
    assert a.free == 3


@pytest.mark.parametrize('P', [1, 2, 4, 8, 32])
def test_allocator_grows_only_at_page_boundaries(P):
    """One frame at a time, and chunks of 3: a page is taken exactly when t0 + c passes q * P."""
    for c in (1, 3):
        a = stream.PageAllocator(64, P)
        t0 = 0
        while t0 + c <= 40:
            before = len(a.pages_of('s'))
            assert a.missing('s', t0 + c) == -(-(t0 + c) // P) - before
            a.grow(['s'], [t0 + c])
            t0 += c
            after = len(a.pages_of('s'))
            assert after == -(-t0 // P)                                         # ceil(frames / P) pages: every frame 0 .. t0-1 has a page, none beyond
            crossed = (t0 - 1) // P != (t0 - c - 1) // P if t0 > c else True    # the chunk's last frame lies in a later page than the frame before the chunk
            assert (after > before) == crossed, (P, c, t0)
        assert a.free == 64 - len(a.pages_of('s'))


def test_allocator_reports_exhaustion_before_anything_moves():
    a = stream.PageAllocator(4, 2)
    a.grow(['x', 'y'], [2, 3])                                                  # x: (0,), y: (1, 2); one page free
    with pytest.raises(TcowError, match=r'needs 2 more page\(s\).*1 of 4 are free'):
        a.grow(['x', 'y'], [4, 5])                                              # x alone would fit: nothing is handed out all the same
    assert a.pages_of('x') == (0,) and a.pages_of('y') == (1, 2) and a.free == 1
    assert a.grow(['x'], [4]) == [(0, 3)] and a.free == 0
    with pytest.raises(TcowError, match='out of pages'):
        a.grow(['new'], [1])
    assert a.pages_of('new') == () and a.free == 0
    a.grow(['x', 'y'], [4, 4])                                                  # nothing missing: no page needed, none free, no refusal


@pytest.mark.parametrize('seed', list(range(6)))
def test_allocator_never_hands_one_page_to_two_sessions(seed):
    """Random open / step / reset / close sequences against a set-based model: the owners' pages and the free pages partition the heap."""
    rng = np.random.default_rng(100 + seed)
    P = int(rng.choice([1, 2, 4, 8]))
    T = 30
    n_pages = int(rng.integers(3, 40))
    a = stream.PageAllocator(n_pages, P)
    frames, model, next_id = {}, {}, 0                                          # model: session -> set of pages
    for _ in range(300):
        op = rng.integers(0, 10)
        if op < 2 or not frames:
            frames[next_id], model[next_id] = 0, set()
            next_id += 1
        elif op < 8:
            ids = [int(i) for i in rng.permutation(list(frames))[:int(rng.integers(1, len(frames) + 1))]]
            ids = [i for i in ids if frames[i] < T]
            if not ids:
                continue
            to = [int(rng.integers(frames[i] + 1, min(T, frames[i] + 9) + 1)) for i in ids]
            need = sum(max(0, -(-t // P) - len(model[i])) for i, t in zip(ids, to))
            free_before = set(range(n_pages)) - set().union(*model.values())
            if need > len(free_before):
                snapshot = {i: a.pages_of(i) for i in frames}
                with pytest.raises(TcowError, match=f'needs {need} more'):
                    a.grow(ids, to)
                assert {i: a.pages_of(i) for i in frames} == snapshot and a.free == len(free_before)
                continue
            lowest = sorted(free_before)[:need]
            got = a.grow(ids, to)
            handed = []
            for i, t, pages in zip(ids, to, got):
                new = set(pages) - model[i]
                assert new <= free_before and len(pages) == len(set(pages)) == -(-t // P)
                assert pages[:len(model[i])] == tuple(p for p in pages if p in model[i])       # the old pages first, in the order they had
                handed += pages[len(model[i]):]
                free_before -= new
                model[i] |= new
                frames[i] = t
            assert handed == lowest                                             # the lowest free pages, ascending, session by session
        else:
            i = int(rng.choice(list(frames)))
            a.release(i)
            if op == 8:
                frames[i], model[i] = 0, set()                                  # reset
            else:
                del frames[i], model[i]                                         # close
        owned = [p for i in frames for p in a.pages_of(i)]
        assert len(owned) == len(set(owned))                                    # no page in two sessions (or twice in one)
        assert all(set(a.pages_of(i)) == model[i] for i in frames)
        assert a.free == n_pages - len(owned) and all(0 <= p < n_pages for p in owned)


def test_allocator_lowest_free_first_after_random_releases():
    a = stream.PageAllocator(10, 1)
    a.grow(list('abcde'), [2] * 5)
    a.release('d'); a.release('b')                                              # pages 6, 7 and 2, 3 come back
    assert a.grow(['f'], [3]) == [(2, 3, 6)]
    assert a.grow(['g'], [1]) == [(7,)] and a.free == 0


def test_allocator_copy_is_independent():
    a = stream.PageAllocator(6, 2)
    a.grow(['x', 'y'], [3, 1])
    b = a.copy()
    assert (b.n_pages, b.P, b.free, b.pages_of('x'), b.pages_of('y')) == (6, 2, 3, (0, 1), (2,))
    b.grow(['y', 'z'], [4, 2]); b.release('x')
    assert (a.free, a.pages_of('x'), a.pages_of('y'), a.pages_of('z')) == (3, (0, 1), (2,), ())
    assert (b.free, b.pages_of('x'), b.pages_of('y'), b.pages_of('z')) == (3, (), (2, 3), (4,))
    a.release('y')
    assert b.pages_of('y') == (2, 3)


def _old_page_check(a, T, ids, splits):
    """The page accounting a rollover call used to do with counters of its own before anything was launched, restated as the oracle: part by
    part, what the rows lack against what is free, a window that ends in a part giving its pages back to the next.  -> None, or (needed, free)
    of the part that is refused."""
    free, held = a.free, {}
    for p in range(2):
        need, ended = 0, []
        for sid, sp in zip(ids, splits):
            for w, t0, c, _ in (sp['parts'][p] if p < len(sp['parts']) else ()):
                key = (sid, w & 1)
                have = held.setdefault(key, len(a.pages_of(key)))
                want = max(have, -(-(t0 + c) // a.P))
                need += want - have
                held[key] = want
                if t0 + c == T:
                    ended.append(key)
        if need > free:
            return need, free
        free += sum(held[key] for key in ended) - need
        held.update((key, 0) for key in ended)
    return None


@pytest.mark.parametrize('T', [4, 5, 8, 30])
def test_rollover_page_moves_decide_as_the_old_accounting_did(T):
    """Random calls of 1 .. 4 sessions on pools from a third of the peak to above it, every k, P in 1, 2, 4, 8: a run of rollover_page_moves on a
    copy of the allocator refuses exactly the calls the old accounting refused, with the same message, and moves nothing; the real run then
    leaves every window's pages as growing per part and releasing the ended windows afterwards did."""
    rng = np.random.default_rng(7 + T)
    calls = refused = 0
    for k in range(1, T // 2 + 1):
        plan = stream.RolloverPlan(T, k)
        for P in (1, 2, 4, 8):
            for _ in range(3):
                n_sessions = int(rng.integers(1, 5))
                peak = n_sessions * (-(-T // P) + -(-k // P))
                a = stream.PageAllocator(int(rng.integers(max(1, peak // 3), peak + 3)), P)
                done = [0] * n_sessions
                for _ in range(40):
                    ids = [int(i) for i in rng.permutation(n_sessions)[:int(rng.integers(1, n_sessions + 1))]]
                    cs = [int(rng.integers(1, plan.s + 1)) for _ in ids]
                    g0s = [done[i] for i in ids]
                    old = _old_page_check(a, T, ids, [plan.split(g0, c) for g0, c in zip(g0s, cs)])
                    call = stream.RolloverCall(plan, g0s, cs)
                    before = (a.free, {key: a.pages_of(key) for i in range(n_sessions) for key in ((i, 0), (i, 1))})
                    calls += 1
                    try:
                        trial = a.copy()
                        for rows in call.parts:
                            stream.rollover_page_moves(trial, T, ids, rows)
                    except TcowError as e:
                        refused += 1
                        assert old is not None and str(e) == (f'stream_pool: out of pages: this step needs {old[0]} more page(s) of {P} frame(s), {old[1]} of '
                                                              f'{a.n_pages} are free; close() or reset() a session, or open the pool with more pages')
                        assert before == (a.free, {key: a.pages_of(key) for key in before[1]})
                        i = ids[int(rng.integers(len(ids)))]                    # the caller makes room: reset() of one of the sessions
                        a.release((i, 0)); a.release((i, 1))
                        done[i] = 0
                        continue
                    assert old is None and before == (a.free, {key: a.pages_of(key) for key in before[1]})
                    ref = a.copy()
                    for rows in call.parts:                                    # as the pool used to: grow, launch, then release
                        keys = [(ids[r.k], r.w & 1) for r in rows]
                        want = ref.grow(keys, [r.t0 + r.c for r in rows])
                        assert stream.rollover_page_moves(a, T, ids, rows) == want
                        for key, r in zip(keys, rows):
                            if r.t0 + r.c == T:
                                ref.release(key)
                        assert a.free == ref.free
                    assert (trial.free, trial._pages) == (a.free, a._pages) == (ref.free, ref._pages)
                    for i, c in zip(ids, cs):
                        done[i] += c
    assert calls >= 400 and refused >= calls // 20, (calls, refused)


# ---------------------------------------------------------------------------------------------- keywords

def test_page_plan_defaults_and_refusals():
    assert stream.page_plan(3, 30, None, None) == (None, None)                  # the contiguous pool
    for cap, T, P in ((1, 30, 1), (3, 30, 8), (8, 60, 16), (2, 4, 32), (5, 30, 32), (4, 1024, 1024)):
        assert stream.page_plan(cap, T, P, None) == (P, cap * -(-T // P))       # capacity * ceil(T / P): cannot run out
    assert stream.page_plan(32, 60, 8, 100) == (8, 100)
    assert stream.page_plan(2, 30, 4, 1) == (4, 1)
    for P in (0, -1, 3, 6, 12, 2048, 2.5):
        with pytest.raises(TcowError, match='page_frames'):
            stream.page_plan(2, 30, P, None)
    for pages in (0, -3, 1.5):
        with pytest.raises(TcowError, match='pages'):
            stream.page_plan(2, 30, 4, pages)
    with pytest.raises(TcowError, match='without page_frames'):
        stream.page_plan(2, 30, None, 16)


def test_stream_pool_refuses_bad_page_keywords_before_anything_else():
    """On both classes that carry stream_pool, and ahead of the check that the module is on the GPU (these modules are not)."""
    net = _net(1).eval()
    for obj in (net, net.seeker):
        with pytest.raises(TcowError, match='page_frames'):
            obj.stream_pool(2, page_frames=3)
        with pytest.raises(TcowError, match='pages'):
            obj.stream_pool(2, page_frames=2, pages=0)
        with pytest.raises(TcowError, match='without page_frames'):
            obj.stream_pool(2, pages=4)
        with pytest.raises(TcowError, match='CPU'):                             # valid keywords: the usual refusal of a CPU module
            obj.stream_pool(2, page_frames=2, pages=3)


# ---------------------------------------------------------------------------------------------- ABI

def test_paged_abi_entry():
    """The paged layout is three ints and a table of the step record (page_frames == 0: contiguous), not an entry point."""
    abi.check_version()
    abi.check_header_and_records()
    fields = abi.header_fields(abi.header()[1], 'tcow_stream_attn_args')
    assert [f for f in fields if 'page' in f[0]] == [('page_frames', ctypes.c_int), ('n_pages', ctypes.c_int), ('pages_per_session', ctypes.c_int),
                                                     ('page_rows', ctypes.c_void_p)]
    assert len(_lib.SIGNATURES['tcow_attn_temporal_step'][1]) == 2
    abi.check_builds_export()
    abi.check_old_symbols_are_gone(['tcow_attn_temporal_ragged_paged_fwd', 'tcow_attn_temporal_ragged_paged_cq_fwd'])

"""The host arithmetic of streaming inference (tcow_amd/stream.py): everything that needs no device, no module and no tensor, so all of it runs
and is tested on the CPU.  stream.py imports these names and owns what is left: tensors, graphs and launches.

  cache_plan       the cache_dtype keyword -> the element type of the K / V caches.
  ragged_tables    n sessions with c_i new frames each -> the tables of ONE step over the F = sum of the c_i frames, flat in session order.
  check_sessions, check_range    the refusals of a pool step that look at the lists alone.
  page_plan, PageAllocator       a paged pool: its keywords, and which pages each session owns (lowest free page first, all or nothing).
  RolloverPlan     a session as a chain of windows of T frames that start every s = T - k frames; split(g0, c): the one or two Seeker steps a
                   chunk takes part in, its hand-off frame, and where its frames are reported.
  RolloverCall     the splits of all sessions of one call, put together: the rows of each part, which slice of the caller's chunk and query
                   mask each row takes, the hand-offs, and the runs that make up every session's outputs.
  rollover_page_moves            the page moves of one part of a rollover call; the pool runs them on a copy of its allocator for every part
                   before anything is launched (the refusal is PageAllocator.grow's), then on the allocator itself.
"""
from collections import namedtuple

import torch

from . import ops
from ._lib import TcowError

MAX_FRAMES = 1024       # TCOW_STREAM_MAX_FRAMES of include/tcow_hip.h


def cache_plan(mode, cache_dtype):
    """THE decision of the cache_dtype keyword (host arithmetic only): (torch dtype of the K / V caches, cache_dtype argument of the
    ops.attn_temporal_* wrappers) for a module of ops mode `mode` (F32, BF16, FP16; bf16x3 stores F32).  None -> (the storage type, None): the
    entry points without a cache type.  'fp8' -> torch.float8_e4m3fn in any mode.  'bf16' -> torch.bfloat16 under f32 storage; under bf16
    storage it is what None gives; binary16 storage refuses it (bfloat16 is no narrower, and the binary16 build has no such kernel)."""
    if cache_dtype is None:
        return ops.tdtype(mode), None
    if cache_dtype == 'fp8':
        return torch.float8_e4m3fn, ops.FP8
    if cache_dtype == 'bf16':
        if mode == ops.FP16:
            raise TcowError("stream: cache_dtype='bf16' with precision='fp16': the cache would be no smaller than the binary16 storage; "
                            "use None or 'fp8'")
        return (torch.bfloat16, None) if mode == ops.BF16 else (torch.bfloat16, ops.BF16)
    raise TcowError(f"stream: cache_dtype={cache_dtype!r} must be None, 'bf16' or 'fp8'")


def ragged_tables(t0s, slots, cs):
    """The tables of a ragged step, as lists of ints: n sessions, session r at frame t0s[r] on cache slot slots[r] with cs[r] >= 1 new frames.
    The F = sum(cs) frames lie flat in session order.  Returns a dictionary with, per session, 't0', 'slot', 'first' (its first flat frame: the
    exclusive prefix sum of cs) and 'c', and per flat frame 'row_of_frame' (its session) and 'frames' (its index in the stream, t0 + j: the row
    of the time table it takes)."""
    t0s, slots, cs = [int(v) for v in t0s], [int(v) for v in slots], [int(v) for v in cs]
    if not (len(t0s) == len(slots) == len(cs)) or not cs:
        raise TcowError(f'ragged_tables: {len(t0s)} t0 / {len(slots)} slots / {len(cs)} chunk lengths: one of each per session, at least one session')
    if min(cs) < 1:
        raise TcowError(f'ragged_tables: chunk lengths must be >= 1, got {cs}')
    first, row_of_frame, frames, f = [], [], [], 0
    for r, (t0, c) in enumerate(zip(t0s, cs)):
        first.append(f)
        row_of_frame += [r] * c
        frames += range(t0, t0 + c)
        f += c
    return {'t0': t0s, 'slot': slots, 'first': first, 'c': cs, 'row_of_frame': row_of_frame, 'frames': frames}


def check_sessions(who, ids, n_rgbs, n_masks, capacity, open_ids):
    """The checks of a pool step (`who`) that look at the lists alone: 1 .. capacity sessions, every id open, none twice, and for a list of rgb
    entries (n_rgbs not None) one entry per session, the same for a list of query masks (n_masks not None).  Returns the ids as a list."""
    ids = list(ids)
    n = len(ids)
    if n < 1 or n > capacity:
        raise TcowError(f'{who}: {n} sessions given; a step takes 1 .. capacity = {capacity}')
    if n_rgbs is not None and (n_rgbs != n or (n_masks is not None and n_masks != n)):
        raise TcowError(f'{who}: {n} ids, {n_rgbs} rgb entries' + ('' if n_masks is None else f', {n_masks} query_masks entries')
                        + ': the lengths must agree (one entry per session)')
    seen = set()
    for sid in ids:
        if sid not in open_ids:
            raise TcowError(f'stream_pool: session {sid!r} is not open (unknown or closed id)')
        if sid in seen:
            raise TcowError(f'{who}: duplicate session {sid!r}: a session is one run of frames of a step')
        seen.add(sid)
    return ids


def check_range(who, ids, t0s, cs, T):
    """No session runs past the last frame: frames_done + c_i <= T for every session, the offender named."""
    for sid, t0, c in zip(ids, t0s, cs):
        if t0 + c > T:
            raise TcowError(f'{who}: session {sid}: frames {t0}..{t0 + c - 1} run past the last frame {T - 1} of the stream '
                            f'(num_total_frames = {T}); reset() or close() it')


def page_plan(capacity, T, page_frames, pages):
    """The page_frames / pages keywords of stream_pool for a pool of `capacity` sessions of T frames -> (P, n_pages), or (None, None) for the
    contiguous pool (page_frames None).  P must be a power of two in 1 .. TCOW_STREAM_MAX_FRAMES; pages defaults to capacity * ceil(T / P), with
    which no step can run out of pages."""
    if page_frames is None:
        if pages is not None:
            raise TcowError(f'stream_pool: pages ({pages}) given without page_frames: only a paged pool is sized in pages')
        return None, None
    P = int(page_frames)
    if P != page_frames or P < 1 or P > MAX_FRAMES or P & (P - 1):
        raise TcowError(f'stream_pool: page_frames ({page_frames}) must be a power of two in 1 .. {MAX_FRAMES}')
    n_pages = capacity * -(-T // P) if pages is None else int(pages)
    if n_pages < 1 or (pages is not None and n_pages != pages):
        raise TcowError(f'stream_pool: pages ({pages}) must be an integer >= 1')
    return P, n_pages


class RolloverPlan:
    """THE host arithmetic of a rollover pool (stream_pool(rollover=k)): plain Python, no device.  A session of a model of T frames is a chain of
    windows of T frames that start every s = T - k frames: window w covers the global frames w*s .. w*s + T - 1, frame g is its local frame
    g - w*s.  Window w + 1 starts at the hand-off frame (w + 1)*s, which window w reports and whose thresholded mask logits are the query mask
    of window w + 1.  1 <= k <= T // 2, so at most two windows are live at a frame and a hand-off frame is never a warm-up frame of the older."""

    def __init__(self, T, k):
        T = int(T)
        if isinstance(k, bool) or int(k) != k or k < 1 or k > T // 2:
            raise TcowError(f'stream_pool: rollover ({k!r}) must be an integer in 1 .. num_total_frames // 2 = {T // 2}: the frames two consecutive '
                            'windows share')
        self.T, self.k, self.s = T, int(k), T - int(k)

    def window(self, g):
        """The window that reports global frame g: window 0 its whole span, a later window its local frames k .. T - 1 (the first k warm it up)."""
        return 0 if g < self.T else (g - self.k) // self.s

    def live(self, g):
        """The windows that frame g belongs to, oldest first: the reporting one, and the next once its first frame has come."""
        w = self.window(g)
        return (w, w + 1) if g >= (w + 1) * self.s else (w,)

    def is_handoff(self, g):
        """Frame g is the first frame of a window w >= 1 (g = w*s)."""
        return g >= self.s and g % self.s == 0

    def split(self, g0, c):
        """A session at global frame g0 brings c <= s frames -> the Seeker steps they take part in and where their outputs come from.
        'parts': one or two lists of rows (window, t0, c, g): the window takes its local frames t0 .. t0 + c - 1 = the global frames g .. g + c - 1
        in that step.  Part 1 holds the frames up to and including the chunk's hand-off frame h, if it has one, else all; part 2, only if frames
        follow h, holds those, and the new window from h on (t0 = 0), after the hand-off has made its query mask.  When h is the chunk's last
        frame ('keep') the caller retains that frame, and the next call's part 1 gives it to the new window: a row that starts at g0 - 1.
        'handoff': h or None.  'report': runs (part, window, g, count) in frame order, together the chunk's c frames: where each is reported."""
        g0, c, s = int(g0), int(c), self.s
        if c < 1 or c > s:
            raise TcowError(f'stream_pool: a chunk of {c} frames: a rollover pool takes 1 .. num_total_frames - rollover = {s} frames of a session '
                            'per call (at most one hand-off frame)')
        end = g0 + c
        h = next((g for g in range(g0, end) if self.is_handoff(g)), None)
        cut = end if h is None else h + 1
        born = None if h is None else h // s
        parts = []
        for p, (lo, hi) in enumerate(((g0, cut), (cut, end))):
            if lo >= hi:
                continue
            rows = {}                                           # window -> [first global frame, frames]
            for g in range(lo, hi):
                for w in self.live(g):
                    if not (p == 0 and w == born):              # the new window waits for its query mask
                        rows.setdefault(w, [g, 0])[1] += 1
            if p == 0 and g0 >= 1 and self.is_handoff(g0 - 1):  # the frame the call before retained
                r = rows[(g0 - 1) // s]
                r[0], r[1] = g0 - 1, r[1] + 1
            if p == 1:
                r = rows[born]
                r[0], r[1] = h, r[1] + 1
            parts.append([(w, g - w * s, n, g) for w, (g, n) in sorted(rows.items())])
        report = []
        for g in range(g0, end):
            p, w = int(g >= cut), self.window(g)
            if report and report[-1][:2] == (p, w):
                report[-1] = (p, w, report[-1][2], report[-1][3] + 1)
            else:
                report.append((p, w, g, 1))
        return {'parts': parts, 'handoff': h, 'keep': h == end - 1, 'report': report}


# A row of one part of a rollover call.  k: the session's index in the call; w, t0, c, g: window w takes its local frames t0 .. t0 + c - 1 = the
# global frames g .. g + c - 1; first: its first flat frame in the part's step (ragged_tables' 'first').  Its frames are the slice [lo:hi] of
# the caller's chunk, after the frame the call before retained if `kept`; its query masks the hand-off mask for its first frame if `handed`
# (local frame 0 of a window >= 1), then the slice [qlo:hi] of the caller's query mask (or zeros), which may be empty.
RolloverRow = namedtuple('RolloverRow', 'k w t0 c g first lo hi kept handed qlo')


class RolloverCall:
    """One call of a rollover pool: sessions 0 .. n-1 at global frames g0s bring cs frames.  Plain ints, no tensors, no slots, no pages.
    parts: one or two lists of RolloverRow, the Seeker steps of the call, rows in session order.
    handoffs: (session index, newborn window, flat frame of part 1 at which the window before it reports the hand-off frame).
    keep: per session, whether the chunk ends on its hand-off frame (the pool retains that frame for the next call).
    report: per session the runs (part, flat first frame, count) that make up its outputs, in frame order."""

    def __init__(self, plan, g0s, cs):
        splits = [plan.split(g0, c) for g0, c in zip(g0s, cs)]
        self.keep = [sp['keep'] for sp in splits]
        self.parts, where = [], []                              # where[p][k, w] + g: the flat frame of global frame g in window w's row of part p
        for p in range(max(len(sp['parts']) for sp in splits)):
            rows, at, f = [], {}, 0
            for k, sp in enumerate(splits):
                for w, t0, c, g in (sp['parts'][p] if p < len(sp['parts']) else ()):
                    j, handed = g - g0s[k], w >= 1 and t0 == 0  # j = -1: the row starts at the frame the call before retained
                    rows.append(RolloverRow(k, w, t0, c, g, f, max(j, 0), j + c, j < 0, handed, j + handed))
                    at[k, w] = f - g
                    f += c
            self.parts.append(rows)
            where.append(at)
        born = [None if sp['handoff'] is None else sp['handoff'] // plan.s for sp in splits]
        self.handoffs = [(k, b, where[0][k, b - 1] + sp['handoff']) for k, (sp, b) in enumerate(zip(splits, born)) if b is not None]
        self.report = [[(p, where[p][k, w] + g, n) for p, w, g, n in sp['report']] for k, sp in enumerate(splits)]


def rollover_threshold(threshold):
    """The requery_threshold keyword as a float; a threshold that is not finite is refused."""
    try:
        t = float(threshold)
    except (TypeError, ValueError):
        t = float('nan')
    if t != t or t in (float('inf'), float('-inf')):
        raise TcowError(f'stream_pool: requery_threshold ({threshold!r}) must be a finite number')
    return t


def rollover_capacity(capacity):
    """A session of a rollover pool owns two cache slots, one per live window."""
    if int(capacity) < 2:
        raise TcowError(f'stream_pool: capacity ({capacity}) must be >= 2 with rollover: a session owns two cache slots, one per live window')
    return int(capacity)


def rollover_pages(capacity, T, k, page_frames, pages):
    """page_plan for a rollover pool: a session holds at most ceil(T / P) + ceil(k / P) pages after a call (the window that ends and the k
    warm-up frames of the next), and capacity // 2 sessions fit, so that is what pages defaults to, rounded up."""
    P, n_pages = page_plan(capacity, T, page_frames, pages)
    if P is not None and pages is None:
        n_pages = -(-capacity * (-(-T // P) + -(-k // P)) // 2)
    return P, n_pages


class PageAllocator:
    """Which pages of a paged pool each session owns: plain Python, no device.  Pages 0 .. n_pages-1 hold P frames each; a session that has
    `frames` frames owns ceil(frames / P) pages, in frame order (entry q holds its frames q*P .. q*P+P-1).  Deterministic: grow() hands out the
    lowest free page first, session by session in the order given, as open() takes the lowest free slot."""

    def __init__(self, n_pages, page_frames):
        self.n_pages, self.P = int(n_pages), int(page_frames)
        self._free = list(range(self.n_pages))                  # ascending
        self._pages = {}                                        # session -> its pages in frame order

    @property
    def free(self):
        return len(self._free)

    def pages_of(self, sid):
        return tuple(self._pages.get(sid, ()))

    def missing(self, sid, frames):
        """Pages the session lacks to hold `frames` frames: more than 0 only when the frames cross a page boundary."""
        return max(0, -(-int(frames) // self.P) - len(self._pages.get(sid, ())))

    def grow(self, sids, frames):
        """Every session sids[k] gets the pages it lacks to hold frames[k] frames.  All or nothing: if the free pages do not cover the sum, raises
        TcowError (pages needed and free named) and nothing has moved.  Returns each session's pages."""
        need = sum(self.missing(sid, f) for sid, f in zip(sids, frames))
        if need > len(self._free):
            raise TcowError(f'stream_pool: out of pages: this step needs {need} more page(s) of {self.P} frame(s), {len(self._free)} of '
                            f'{self.n_pages} are free; close() or reset() a session, or open the pool with more pages')
        for sid, f in zip(sids, frames):
            k = self.missing(sid, f)
            if k:
                self._pages.setdefault(sid, []).extend(self._free[:k])
                del self._free[:k]
        return [self.pages_of(sid) for sid in sids]

    def release(self, sid):
        """The session's pages are free again (a session without pages: nothing happens)."""
        self._free = sorted(self._free + self._pages.pop(sid, []))

    def copy(self):
        """An independent allocator in the same state: what a sequence of moves would do, tried without moving anything."""
        a = PageAllocator(0, self.P)
        a.n_pages, a._free, a._pages = self.n_pages, list(self._free), {sid: list(pages) for sid, pages in self._pages.items()}
        return a


def rollover_page_moves(alloc, T, sids, rows):
    """The page moves of one part of a rollover call on `alloc`, whose keys are (session, window parity): every row's window grows to hold its
    frames up to t0 + c (all or nothing: PageAllocator.grow refuses, and nothing has moved), then a window that has produced its last frame
    (t0 + c == T) gives its pages back -- to the next part or call; the pages stay as they are until someone writes them.  Returns the pages
    each row's window had for this part, which is what the part's step reads."""
    keys = [(sids[r.k], r.w & 1) for r in rows]
    pages = alloc.grow(keys, [r.t0 + r.c for r in rows])
    for key, r in zip(keys, rows):
        if r.t0 + r.c == T:
            alloc.release(key)
    return pages

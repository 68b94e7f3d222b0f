"""Streaming inference: the Seeker one chunk of frames at a time, for callers that receive frames live (a camera, a decoder).

With causal_attention 1 or 2 the model is causal along time: frame t's mask logits and flags depend on frames 0..t only (the tril() mask of
vit.py:93-99, the cls row taken from frame 0, vit.py:192-198; everything else works per token or per frame).  A stream step therefore runs
the eval schedule of engine.run_forward on its new frames alone, with three substitutions: the frames' rows of the time table, temporal
attention against a per-block K / V cache of the earlier frames (which the same launch extends by the new frames' K / V), and for
causal_attention == 1 the cls row of frame 0 kept per block.  For any split of 0..T-1 into chunks the concatenated outputs equal forward() of
the whole clip, to the precision mode's rounding.

What lives as long as a stream or a pool is a _State: per block a K and a V cache [rows, S-1, heads, T, 64] in the mode's storage type (16-bit
modes: bf16 / binary16; fp32 and bf16x3: f32), one f32 cls row per row and block, and the effective pos / time tables.  A stream has rows =
clips x queries (the query mask changes every token's K / V), a pool rows = capacity.  At BASELINE configs[1] (T = 30, 240x320, depth 12)
that is 332 MB per row in the 16-bit modes; at configs[3] (T = 60, 480x640) 2.65 GB; f32 twice that.

cache_dtype (net.stream / net.stream_pool; cache_plan below is the one place that decides): the element type of the K / V caches, apart from
the precision mode -- the kernel computes in f32 and only loads and stores cache lines.  None: the storage type, as above.  'bf16': halves the
caches of 'fp32' and 'bf16x3' (the same as None in 'bf16'; refused in 'fp16').  'fp8' (OCP e4m3fn, saturating at +-448, no scales): any
precision, a quarter of an f32 cache and half of a 16-bit one -- 166 MB per row at configs[1].  With a compact cache every key and value of
the temporal attention, the step's own included, enters at its value rounded to that type (q does not), so the outputs still do not depend
on how the frames were split into chunks, and the four step forms below still agree bit for bit; they differ from the None stream's by the
rounding ("Compact cache": accuracy and time, measured).  cls rows, tables, graphs, pages and GEMMs are untouched.

What belongs to one step is a _Step, and it is all run_forward sees (its `stream` argument): pos, time_rows [B*T, D] (one row of the time table
per (row, frame) of the step), attn_temporal(i, ...) and cls_row(i, ...) for block i, and skinny: whether the step's GEMMs take the
skinny-M entry points where ops.skinny_plan (16-bit modes) / ops.skinny_plan_x3 (bf16x3) route them (the skinny_gemm keyword of net.stream /
net.stream_pool).  There are three forms (a fourth for paged pools, below), each a _Step subclass that holds
its device tables and calls its own pair of ops entry points; step(), pool.step() and pool.step_ragged() each build the tables and construct
their form, and nothing else asks which form a step has:

  _StreamStep (SeekerStream.step): every row stands at the same frame t0, a device scalar, and row b uses cache slot b
  (tcow_attn_temporal_cached_fwd, tcow_cls_stream).
  _PoolStep (SeekerStreamPool.step): live sessions that started at different moments, stepped together with one chunk length: a t0 and a
  cache slot per row (tcow_attn_temporal_pool_fwd, tcow_cls_pool -- the stream's kernels, of which the stream is the case "one t0, slot = row").
  _RaggedStep (SeekerStreamPool.step_ragged): the sessions bring different numbers of frames (cameras at different rates, a decoder's GOP, a
  session that catches up while its neighbours advance by one).  The F = sum of the c_i frames lie flat in session order and run as ONE row
  of F frames; ragged_tables() gives every session its t0, slot, first flat frame and chunk length and every frame its session
  (tcow_attn_temporal_ragged_fwd, one wave per frame, not per session, and tcow_cls_ragged).

A paged pool (net.stream_pool(capacity, page_frames=P, pages=N)): a contiguous pool reserves a whole stream's cache per slot, whether its session
is at frame 2, at frame 59 or closed.  With page_frames the K / V caches of a block are a heap of N pages of P frames (_PagedState:
[N, S-1, heads, P, 64], a page id valid in every block alike), a session owns only the pages its frames so far have filled (PageAllocator: host
side, lowest free page first, grows when t0 + c crosses a multiple of P), and close() / reset() give them back; the cls rows stay per slot.  The
pool is then sized in memory (pages), and `capacity` only bounds the number of open sessions.  pages defaults to capacity * ceil(T / P), which
cannot run out; with fewer, a step that needs more pages than are free raises TcowError before anything is launched or any counter or page
moves.  Both step() and step_ragged() of a paged pool run a fourth form:

  _PagedRaggedStep: the _RaggedStep tables plus page_rows [n, ceil(T / P)], the sessions' pages in frame order, sent in the same host-to-device
  copy (tcow_attn_temporal_ragged_paged_fwd: the ragged kernel with "page page_rows[r][kt / P], line kt % P" for "slot, line kt"; tcow_cls_ragged).

Where a key lives does not enter the arithmetic, so a paged pool gives the bits of the contiguous pool.  A one-frame step costs between nothing measurable
and 0.13 ms more than on the contiguous pool (profiles/stream_paged_latency.json; P = 8 is the recommendation, P = 1 the
dearest): the keywords are off by default.  SeekerStream stays contiguous.

A rollover pool (net.stream_pool(capacity, rollover=k, requery_threshold=0.0) -> SeekerRolloverPool): a stream or a pool session ends at frame
T - 1, because the time table has T rows and the query belongs to frame 0.  With rollover a session is a chain of windows of T frames that
start every T - k frames (RolloverPlan: all of the host arithmetic); each later window is queried with the thresholded mask logits the window
before it returned for the frame where it starts (ops.requery_mask, tcow_requery_mask: on the device, nothing is read back), its first k frames
only fill its cache, and the reported outputs are forward() of every window built that way.  A session owns two cache slots, a call is one
Seeker step unless a chunk goes on after a hand-off frame (then two), and the steps are the ragged forms above, unchanged.  Without the keyword
a pool is what it was.

graph=True (SeekerStream): the first step of each chunk length c runs eagerly and captures the step as a torch.cuda.CUDAGraph; later steps copy
their inputs into the graph's static buffers, write t0 and the time rows (the stream keeps one _StreamStep with static time rows per chunk
length, and one t0 scalar: the graph points into both) and replay.  No step synchronises the host except the one capture per chunk length.  A
graph keeps the module's operand copies it was captured with alive; when the module replaces them (.cuda() / .to() on the same device,
set_precision() with the same precision, a train-mode forward) the graphs are dropped and captured again.  Pool steps run eagerly and build a
fresh step object per call.  With skinny_gemm the captured launches also point into the split-K workspace of ops.gemm_nt_skinny / ops.gemm_nt_skinny_x3 (one tag): the capture
runs on the workspace that the eager step before it sized, and the graph's entry keeps that tensor (ops.workspace replaces, never resizes).
"""
import torch

from . import engine, ops
from ._lib import TcowError

MAX_FRAMES = 1024       # TCOW_STREAM_MAX_FRAMES of include/tcow_hip.h

# Default of the skinny_gemm keyword.  True: measured (profiles/stream_skinny_latency.json) -- a one-frame bf16 step takes
# 1.42 ms instead of 2.41 at configs[1] B = 1, 2.41 instead of 3.35 at configs[3] B = 1 and 2.60 instead of 3.24 at configs[1] B = 8, on / off
# alternating in one run, each difference several times the off leg's own max - min.  False runs the steps on tcow_gemm_nt alone.
SKINNY_GEMM_DEFAULT = True
# The same keyword's default when the module's precision is 'bf16x3' (ops.gemm_nt_skinny_x3 where ops.skinny_plan_x3 routes).  True: measured
# (profiles/stream_skinny_x3_latency.json) -- a one-frame bf16x3 step takes 1.94 ms instead of 4.28 at configs[1] B = 1,
# 4.45 instead of 5.88 at configs[3] B = 1 and 5.17 instead of 6.06 at configs[1] B = 8, each difference above the off leg's own max - min.
SKINNY_GEMM_X3_DEFAULT = True


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


def _skinny_default(module):
    return SKINNY_GEMM_X3_DEFAULT if module.gemm_mode == ops.F32X3 else SKINNY_GEMM_DEFAULT


class _State:
    """What lives as long as a stream or a pool of `rows` query rows: per block the K / V caches [rows, S-1, heads, T, 64] in the element type of
    cache_plan (the mode's storage type unless cache_dtype says otherwise) and one f32 cls row per query row, and the effective pos table and
    time table [T, D].  cq: the cache_dtype argument every step built on this state passes to its ops.attn_temporal_* wrapper."""

    def _kv_shape(self, depth, rows, g):
        return (depth, rows, g['S'] - 1, g['heads'], self.T_total, 64)

    def __init__(self, module, rows, skinny=False, cache_dtype=None):
        self.skinny = bool(skinny)                              # every step built on this state carries it (_Step.skinny)
        g = module.geometry(rows)
        dev = module.vit.pos_embed.device
        cdt, self.cq = cache_plan(module.mode, cache_dtype)     # (None: the storage type -- bf16x3 stores f32, like fp32)
        self.T_total, self.n_slots, self.D = module.num_total_frames, rows, g['D']
        shape = self._kv_shape(module.network_depth, rows, g)
        self.k_cache = torch.empty(shape, dtype=cdt, device=dev)
        self.v_cache = torch.empty(shape, dtype=cdt, device=dev)
        self.cls_cache = torch.empty(module.network_depth, rows, g['D'], dtype=torch.float32, device=dev)
        with torch.no_grad():
            self.pos, self.time, _, _ = engine._effective_embeddings(module, g)     # (nearest-resized when the stored tables differ)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.k_cache, self.v_cache, self.cls_cache))


class _PagedState(_State):
    """The state of a paged pool: per block the K / V caches are a heap of n_pages pages of P frames, [n_pages, S-1, heads, P, 64], of which a
    session owns those its frames so far have filled (PageAllocator; a page id is valid in every block's arrays alike); the cls rows stay one per
    slot [rows, D], and `rows` = capacity only bounds the number of open sessions.  A session's row of the page table has pps = ceil(T / P) entries."""

    def __init__(self, module, rows, skinny, page_frames, n_pages, cache_dtype=None):
        self.P, self.n_pages = page_frames, n_pages
        self.pps = -(-module.num_total_frames // page_frames)
        super().__init__(module, rows, skinny, cache_dtype)

    def _kv_shape(self, depth, rows, g):
        return (depth, self.n_pages, g['S'] - 1, g['heads'], self.P, 64)


class _Step:
    """What engine.run_forward asks of one stream step: pos, time_rows [B*T, D] (one row of the time table per (row, chunk frame)) and the two
    substitutions of block i, attn_temporal and cls_row.  A form is its tables and its two ops entry points; it is chosen by constructing one of
    the three classes below, where the tables are built, and nowhere else."""

    def __init__(self, state, time_rows, *tables):
        self.state, self.pos, self.time_rows, self.tables = state, state.pos, time_rows, tables
        self.skinny = state.skinny


class _StreamStep(_Step):
    """tables: t0_dev, the one frame index of all rows (a device scalar: a captured graph reads it); row b works on cache slot b."""

    def attn_temporal(self, i, amode, B, T, S, D, heads, ca, QKV, O):
        st = self.state
        ops.attn_temporal_cached(amode, B, T, S, D, heads, ca, st.T_total, *self.tables, QKV, st.k_cache[i], st.v_cache[i], O, st.cq)

    def cls_row(self, i, R2, B, T, S):
        ops.cls_stream(R2, B, T, S, self.state.cls_cache[i], *self.tables)


class _PoolStep(_Step):
    """tables: t0_rows, slot_rows (device int32 [B]): a frame index and a cache slot per row."""

    def attn_temporal(self, i, amode, B, T, S, D, heads, ca, QKV, O):
        st = self.state
        ops.attn_temporal_pool(amode, B, T, S, D, heads, ca, st.T_total, st.n_slots, *self.tables, QKV, st.k_cache[i], st.v_cache[i], O, st.cq)

    def cls_row(self, i, R2, B, T, S):
        ops.cls_pool(R2, B, T, S, self.state.cls_cache[i], self.state.n_slots, *self.tables)


class _RaggedStep(_Step):
    """tables: t0_rows, slot_rows, first_rows, c_rows (device int32 [n], per session) and row_of_frame ([F], per flat frame); the step is ONE row
    of F = T frames."""

    def attn_temporal(self, i, amode, B, T, S, D, heads, ca, QKV, O):
        st = self.state
        ops.attn_temporal_ragged(amode, self.tables[0].numel(), T, S, D, heads, ca, st.T_total, st.n_slots, *self.tables, QKV, st.k_cache[i],
                                 st.v_cache[i], O, st.cq)

    def cls_row(self, i, R2, B, T, S):
        ops.cls_ragged(R2, self.tables[0].numel(), T, S, self.state.cls_cache[i], self.state.n_slots, *self.tables[:4])


class _PagedRaggedStep(_RaggedStep):
    """A ragged step on a _PagedState.  tables: those of _RaggedStep (the slot still names the session's cls row) and page_rows (device int32
    [n, pps]): the pages of every session in frame order, -1 where it owns none yet (the kernel reads only the entries of frames <= t)."""

    def attn_temporal(self, i, amode, B, T, S, D, heads, ca, QKV, O):
        st = self.state
        t0_rows, _, first_rows, c_rows, row_of_frame, page_rows = self.tables
        ops.attn_temporal_ragged_paged(amode, t0_rows.numel(), T, S, D, heads, ca, st.T_total, st.n_pages, st.P, t0_rows, page_rows, first_rows, c_rows,
                                       row_of_frame, QKV, st.k_cache[i], st.v_cache[i], O, st.cq)


def check_streamable(module):
    """Raise TcowError unless `module` (a QueryMaskTracker) can be streamed in its present state."""
    if module.attention_type != 'divided_space_time':
        raise TcowError(f"stream: attention_type={module.attention_type!r} is not supported: joint space-time attention lets every frame see every "
                        "other frame; only 'divided_space_time' streams")
    if module.causal_attention not in (1, 2):
        raise TcowError(f'stream: causal_attention={module.causal_attention} is not causal along time (0: mean cls over all frames; -1: no mask; '
                        '>= 3: look-ahead compounded over the blocks); a stream needs causal_attention 1 or 2')
    if module.training:
        raise TcowError('stream: the module is in training mode (DropPath draws one value per temporal row across all frames): call .eval() first')
    if module.forced_drop_masks is not None:
        raise TcowError('stream: forced_drop_masks is set; DropPath cannot be streamed')
    if not module.vit.pos_embed.is_cuda:
        raise TcowError('stream: the module is on the CPU; streams run on the GPU only (move the module to cuda)')


def _signature(module):
    """Changes whenever a parameter (or the precision) changes: load_state_dict / optimizer steps bump _version, FusedAdamWClip bumps the operand epoch."""
    return (module.mode, module.gemm_mode, module._operands.epoch) + tuple((id(p), p._version, p.data_ptr()) for p in module.param_list())


def _check_module(module, sig):
    """The module can still be streamed and is the one the caches were filled by."""
    check_streamable(module)
    if _signature(module) != sig:
        raise TcowError('stream: a parameter (or the precision) changed since the stream was opened; the cached keys / values belong to the old '
                        'weights -- open a new stream')


def _check_inputs(who, m, device, clips, rows, rgb, query_mask):
    """Shapes and devices of a step's frames (rgb of `clips` clips, query masks of `rows` query rows); returns the chunk length c."""
    if not torch.is_tensor(rgb) or rgb.dim() != 5 or rgb.shape[0] != clips or rgb.shape[1] != 3 or rgb.shape[2] < 1 \
            or rgb.shape[3] != m.frame_height or rgb.shape[4] != m.frame_width:
        raise TcowError(f'{who}: rgb must be ({clips}, 3, c >= 1, {m.frame_height}, {m.frame_width}), got '
                        f'{tuple(rgb.shape) if torch.is_tensor(rgb) else type(rgb).__name__}')
    c = int(rgb.shape[2])
    if query_mask is not None and (not torch.is_tensor(query_mask) or tuple(query_mask.shape) != (rows, 1, c, m.frame_height, m.frame_width)):
        raise TcowError(f'{who}: query_mask must be ({rows}, 1, {c}, {m.frame_height}, {m.frame_width}) or None, got '
                        f'{tuple(query_mask.shape) if torch.is_tensor(query_mask) else type(query_mask).__name__}')
    for t in (rgb, query_mask):
        if t is not None and (not t.is_cuda or t.device != device):
            raise TcowError(f'{who}: inputs must be on the stream device {device}, got {t.device}')
    return c


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


def _zero_mask(rows, rgb):
    """The query mask of a step that was given none: all zeros, (rows, 1, c, H, W) for rgb (clips, 3, c, H, W)."""
    return torch.zeros(rows, 1, *rgb.shape[2:], dtype=torch.float32, device=rgb.device)


class SeekerStream:
    """net.stream(batch_size, queries_per_clip, graph, skinny_gemm, cache_dtype) of Seeker / QueryMaskTracker; see the module docstring.  A stream
    ends at frame num_total_frames - 1; a session without a last frame is net.stream_pool(capacity, rollover=k) (SeekerRolloverPool)."""

    def __init__(self, module, batch_size=1, queries_per_clip=1, graph=False, skinny_gemm=None, cache_dtype=None):
        module = getattr(module, 'seeker', module)
        check_streamable(module)
        Bc, Qs = int(batch_size), int(queries_per_clip)
        if Bc < 1 or Qs < 1:
            raise TcowError(f'stream: batch_size ({Bc}) and queries_per_clip ({Qs}) must be >= 1')
        self.module = module
        self.Bc, self.Qs, self.B = Bc, Qs, Bc * Qs
        self.T = module.num_total_frames
        self.graph = bool(graph)
        self.skinny_gemm = _skinny_default(module) if skinny_gemm is None else bool(skinny_gemm)
        self.cache_dtype = cache_dtype
        self._st = _State(module, self.B, self.skinny_gemm, cache_dtype)
        self.device = self._st.pos.device
        self._t0_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._steps = {}                # c -> the step of chunk length c; its time_rows [B*c, D] f32 are static: a captured graph points into both
        self._graphs = {}               # c -> (graph, static rgb, static query mask, output mask, flags)
        self._sig = _signature(module)
        self.frames_done = 0

    @property
    def cache_bytes(self):
        """Device bytes of the K / V caches and the cls rows."""
        return self._st.nbytes

    def reset(self):
        """Start again at frame 0 (the buffers, and any captured graphs, are kept)."""
        self.frames_done = 0

    def step(self, rgb, query_mask=None):
        """rgb (Bc, 3, c, H, W), query_mask (Bc*Qs, 1, c, H, W) or None (all zeros) for the next c >= 1 frames ->
        (mask logits (Bc*Qs, Co, c, H, W) f32, flags (Bc*Qs, c, F) or None) of exactly those frames, owned by the caller."""
        _check_module(self.module, self._sig)
        c = _check_inputs('stream.step', self.module, self.device, self.Bc, self.B, rgb, query_mask)
        t0 = self.frames_done
        if t0 + c > self.T:
            raise TcowError(f'stream.step: frames {t0}..{t0 + c - 1} run past the last frame {self.T - 1} of the stream (num_total_frames = {self.T}); '
                            'reset() to start again, or run the camera on net.stream_pool(capacity, rollover=k), whose sessions have no last frame')
        with torch.no_grad(), torch.cuda.device(self.device):
            step = self._steps.get(c)
            if step is None:
                step = self._steps[c] = _StreamStep(self._st, torch.empty(self.B * c, self._st.D, dtype=torch.float32, device=self.device), self._t0_dev)
            step.time_rows.view(self.B, c, -1).copy_(self._st.time[t0:t0 + c])      # row b*c + j = time row t0 + j, for every b
            self._t0_dev.fill_(t0)
            rgb32 = rgb.to(torch.float32).contiguous()
            qm32 = None if query_mask is None else query_mask.to(torch.float32).contiguous()
            out = self._graph_step(step, rgb32, qm32) if self.graph else self._run(step, rgb32, qm32)
        self.frames_done = t0 + c
        return out

    def _run(self, step, rgb, qm):
        m = self.module
        out_mask, flags, _ = engine.run_forward(m, rgb, _zero_mask(self.B, rgb) if qm is None else qm, m.param_list(), save=False, stream=step)
        return out_mask, (flags if m.flag_channels > 0 else None)

    def _operand_generation(self):
        """Identifies the module's operand caches (16-bit weight copies, folded projection, row vectors in module._operands).  .cuda() / .to()
        on the same device, set_precision() with the same precision and train-mode forwards replace them without changing a parameter."""
        m = self.module
        return (m._operands.generation, m.mode)

    def _graph_step(self, step, rgb, qm):
        c = rgb.shape[2]
        gen = self._operand_generation()
        if any(e['gen'] != gen for e in self._graphs.values()):
            self._graphs.clear()                # captured against replaced operand copies: capture again (the pool of a dropped graph is stream-ordered)
        ent = self._graphs.get(c)
        if ent is None:
            out = self._run(step, rgb, qm)      # this step's result; it also creates every lazily built operand the capture needs
            s_rgb = rgb.clone()
            s_qm = qm.clone() if qm is not None else _zero_mask(self.B, rgb)
            graph = torch.cuda.CUDAGraph()
            # the split-K workspace as the eager step above left it (current stream; the capture runs on a side stream): large enough for this
            # chunk length, so the capture allocates none, and this entry owns the tensor its launches point into
            ws = ops.workspace(0, self.device, 'nt_skinny') if step.skinny else None
            with torch.cuda.graph(graph):
                if ws is None:
                    g_mask, g_flags = self._run(step, s_rgb, s_qm)
                else:
                    with ops.pinned_workspace('nt_skinny', ws):
                        g_mask, g_flags = self._run(step, s_rgb, s_qm)
            # The graph holds raw pointers into tensors that only module._operands owns (operand copies, folded W' / b', mask0): a shallow copy
            # of the dictionary keeps them alive as long as the graph, whatever later replaces the dictionary or its entries.
            keep = self.module._operands.keep_alive()
            self._graphs[c] = dict(graph=graph, rgb=s_rgb, qm=s_qm, mask=g_mask, flags=g_flags, gen=self._operand_generation(), keep=keep, ws=ws)
            return out
        graph, s_rgb, s_qm, g_mask, g_flags = ent['graph'], ent['rgb'], ent['qm'], ent['mask'], ent['flags']
        s_rgb.copy_(rgb)
        if qm is None:
            s_qm.zero_()
        else:
            s_qm.copy_(qm)
        graph.replay()
        return g_mask.clone(), (g_flags.clone() if g_flags is not None else None)


class SeekerStreamPool:
    """net.stream_pool(capacity, skinny_gemm, page_frames, pages, cache_dtype) of Seeker / QueryMaskTracker: up to `capacity` live sessions (one clip and one query
    mask each) that stand at different frames, stepped together; see the module docstring.  open() -> id, step(ids, rgb, query_mask) (one chunk
    length for all) or step_ragged(ids, rgbs, query_masks) (a chunk length per session), close(id).  page_frames=P: a paged pool, whose K / V
    memory is `pages` pages of P frames shared by the sessions (pages_total, pages_free, pages_of(id)); its outputs are bit-identical to the
    contiguous pool's."""

    def __init__(self, module, capacity, skinny_gemm=None, page_frames=None, pages=None, cache_dtype=None):
        module = getattr(module, 'seeker', module)
        capacity = int(capacity)
        if capacity < 1:
            raise TcowError(f'stream_pool: capacity ({capacity}) must be >= 1')
        self.page_frames, n_pages = page_plan(capacity, module.num_total_frames, page_frames, pages)
        check_streamable(module)
        self.module = module
        self.capacity = capacity
        self.T = module.num_total_frames
        self.skinny_gemm = _skinny_default(module) if skinny_gemm is None else bool(skinny_gemm)
        self.cache_dtype = cache_dtype
        if self.page_frames is None:
            self._st, self._alloc = _State(module, capacity, self.skinny_gemm, cache_dtype), None
        else:
            self._st = _PagedState(module, capacity, self.skinny_gemm, self.page_frames, n_pages, cache_dtype)
            self._alloc = PageAllocator(n_pages, self.page_frames)
        self.device = self._st.pos.device
        self._sig = _signature(module)
        self._slot = {}                 # open session id -> cache slot
        self._done = {}                 # open session id -> frames consumed
        self._next_id = 0

    @property
    def cache_bytes(self):
        """Device bytes of the K / V caches and the cls rows of all `capacity` slots (a paged pool: of all its pages and the cls rows)."""
        return self._st.nbytes

    def _paged(self):
        if self._alloc is None:
            raise TcowError('stream_pool: this pool is contiguous (opened without page_frames): it has no pages')
        return self._alloc

    @property
    def pages_total(self):
        """Pages of a paged pool."""
        return self._paged().n_pages

    @property
    def pages_free(self):
        """Pages of a paged pool that no session owns."""
        return self._paged().free

    def pages_of(self, sid):
        """The pages the session owns, in frame order: ceil(frames it was stepped to / page_frames) of them."""
        return self._paged().pages_of(self._known(sid))

    def _known(self, sid):
        if sid not in self._slot:
            raise TcowError(f'stream_pool: session {sid!r} is not open (unknown or closed id)')
        return sid

    def open(self):
        """A new session at frame 0 in the smallest free slot; returns its id (ids are never reused)."""
        taken = set(self._slot.values())
        free = [s for s in range(self.capacity) if s not in taken]
        if not free:
            raise TcowError(f'stream_pool.open: all {self.capacity} slots are taken; close() a session first')
        sid = self._next_id
        self._next_id += 1
        self._slot[sid], self._done[sid] = free[0], 0
        return sid

    def close(self, sid):
        """End the session; its slot is free for the next open() (and in a paged pool its pages for any session)."""
        self._known(sid)
        del self._slot[sid], self._done[sid]
        if self._alloc is not None:
            self._alloc.release(sid)

    def frames_done(self, sid):
        return self._done[self._known(sid)]

    def reset(self, sid):
        """Put the session back at frame 0 (it keeps its slot; in a paged pool it gives its pages back)."""
        self._done[self._known(sid)] = 0
        if self._alloc is not None:
            self._alloc.release(sid)

    def _checked(self, who, ids, rgbs, qms, per):
        """Every check of a step (`who`), before anything is launched or any counter moves.  rgbs / qms: one tensor of all sessions, or (per) a list
        with an entry per session.  Returns (ids, the frame every session stands at, the chunk length of every session)."""
        m = self.module
        ids = check_sessions(who, ids, len(rgbs) if per else None, len(qms) if per and qms is not None else None, self.capacity, self._slot)
        _check_module(m, self._sig)
        if per:
            cs = [_check_inputs(f'{who}: session {sid}', m, self.device, 1, 1, rgbs[k], None if qms is None else qms[k]) for k, sid in enumerate(ids)]
        else:
            cs = [_check_inputs(who, m, self.device, len(ids), len(ids), rgbs, qms)] * len(ids)
        t0s = [self._done[sid] for sid in ids]
        check_range(who, ids, t0s, cs, self.T)
        if self._alloc is not None:
            # the last check, and the only thing of a refused step that could have moved: the pages of frames up to t0 + c_i - 1 (all or nothing)
            self._alloc.grow(ids, [t0 + c for t0, c in zip(t0s, cs)])
        return ids, t0s, cs

    def _forward(self, step, rgb, qm):
        """One Seeker step (qm None: all zeros)."""
        m = self.module
        out_mask, flags, _ = engine.run_forward(m, rgb, _zero_mask(rgb.shape[0], rgb) if qm is None else qm, m.param_list(), save=False, stream=step)
        return out_mask, (flags if m.flag_channels > 0 else None)

    def _run(self, step, ids, cs, rgb, qm):
        """One Seeker step, after which every session has moved on by its chunk length."""
        out = self._forward(step, rgb, qm)
        for sid, c in zip(ids, cs):
            self._done[sid] += c
        return out

    def step(self, ids, rgb, query_mask=None):
        """ids: n distinct open sessions, at any phases; rgb (n, 3, c, H, W), query_mask (n, 1, c, H, W) or None (all zeros): the next c >= 1
        frames of each -> (mask logits (n, Co, c, H, W) f32, flags (n, c, F) or None) in the order of `ids`, owned by the caller.  Every check
        runs before anything is launched: a refused step leaves every session where it was."""
        ids, t0s, cs = self._checked('stream_pool.step', ids, rgb, query_mask, False)
        if self._alloc is not None:
            return self._step_paged(ids, t0s, cs, rgb, query_mask)
        st, c = self._st, cs[0]
        with torch.no_grad(), torch.cuda.device(self.device):
            t0_rows = torch.tensor(t0s, dtype=torch.int32, device=self.device)
            slot_rows = torch.tensor([self._slot[sid] for sid in ids], dtype=torch.int32, device=self.device)
            frames = (t0_rows[:, None] + torch.arange(c, dtype=torch.int32, device=self.device)[None, :]).reshape(-1)
            step = _PoolStep(st, st.time.index_select(0, frames), t0_rows, slot_rows)         # [n*c, D]: row r*c + j = time row t0_rows[r] + j
            return self._run(step, ids, cs, rgb.to(torch.float32).contiguous(), None if query_mask is None else query_mask.to(torch.float32).contiguous())

    def _ragged_form(self, ids, t0s, cs, slots=None):
        """The step object of a ragged step (inside no_grad on the pool's device) and every session's first flat frame.  A paged pool sends the
        sessions' page rows in the same host-to-device copy as the other tables.  ids: what the page allocator knows the rows by; slots: their
        cache slots (None: those of the sessions `ids`)."""
        n, st = len(ids), self._st
        tab = ragged_tables(t0s, [self._slot[sid] for sid in ids] if slots is None else slots, cs)
        F = len(tab['frames'])
        # all tables in one host-to-device copy: [t0 | slot | first | c] per session, [row_of_frame | frames] per flat frame, [pages] per session
        flat = tab['t0'] + tab['slot'] + tab['first'] + tab['c'] + tab['row_of_frame'] + tab['frames']
        if self._alloc is not None:
            for sid in ids:
                own = self._alloc.pages_of(sid)
                flat += list(own) + [-1] * (st.pps - len(own))
        dev = torch.tensor(flat, dtype=torch.int32).to(self.device)
        time_rows = st.time.index_select(0, dev[4 * n + F:4 * n + 2 * F])               # [F, D]: flat frame f = time row t0 + j of its session
        tables = (dev[0:n], dev[n:2 * n], dev[2 * n:3 * n], dev[3 * n:4 * n], dev[4 * n:4 * n + F])
        if self._alloc is None:
            return _RaggedStep(st, time_rows, *tables), tab['first']
        return _PagedRaggedStep(st, time_rows, *tables, dev[4 * n + 2 * F:].view(n, st.pps)), tab['first']

    def _step_paged(self, ids, t0s, cs, rgb, query_mask):
        """step() of a paged pool: the ragged form with equal chunk lengths (bit-equal to the pool form), in and out in step()'s shapes."""
        n, c = len(ids), cs[0]
        # (n, C, c, H, W) -> (1, C, n*c, H, W): the frames flat in session order
        flat = lambda x: x.to(torch.float32).transpose(0, 1).reshape(1, x.shape[1], n * c, *x.shape[3:]).contiguous()
        with torch.no_grad(), torch.cuda.device(self.device):
            step, _ = self._ragged_form(ids, t0s, cs)
            out_mask, flags = self._run(step, ids, cs, flat(rgb), None if query_mask is None else flat(query_mask))
            out_mask = out_mask.view(out_mask.shape[1], n, c, *out_mask.shape[3:]).transpose(0, 1).contiguous()
        return out_mask, (None if flags is None else flags.reshape(n, c, -1))

    def step_ragged(self, ids, rgbs, query_masks=None):
        """ids: n distinct open sessions, at any phases; rgbs: n tensors (1, 3, c_i, H, W), the next c_i >= 1 frames of each session (the c_i need
        not be equal); query_masks: None, or n entries, each None (all zeros) or (1, 1, c_i, H, W) -> (a list of n mask-logit tensors
        (1, Co, c_i, H, W) f32, a list of n flag tensors (1, c_i, F) or None), in the order of `ids`.  The outputs are slices of buffers allocated
        for this step and owned by the caller.  The whole step is ONE Seeker step over the sum of the c_i frames.  Every check runs before anything
        is launched: a refused step leaves every session where it was."""
        rgbs = list(rgbs)
        qms = None if query_masks is None else list(query_masks)
        ids, t0s, cs = self._checked('stream_pool.step_ragged', ids, rgbs, qms, True)
        n = len(ids)
        with torch.no_grad(), torch.cuda.device(self.device):
            step, first = self._ragged_form(ids, t0s, cs)
            rgb32 = rgbs[0].to(torch.float32).contiguous() if n == 1 else torch.cat([r.to(torch.float32) for r in rgbs], 2)
            if qms is not None and all(q is not None for q in qms):
                qm32 = qms[0].to(torch.float32).contiguous() if n == 1 else torch.cat([q.to(torch.float32) for q in qms], 2)
            else:
                qm32 = _zero_mask(1, rgb32)
                for q, f0, c in zip(qms or (), first, cs):
                    if q is not None:
                        qm32[:, :, f0:f0 + c] = q
            out_mask, flags = self._run(step, ids, cs, rgb32, qm32)
        masks = [out_mask[:, :, f0:f0 + c] for f0, c in zip(first, cs)]
        return masks, (None if flags is None else [flags[:, f0:f0 + c] for f0, c in zip(first, cs)])


class SeekerRolloverPool(SeekerStreamPool):
    """net.stream_pool(capacity, ..., rollover=k, requery_threshold=0.0): a pool whose sessions run past the last frame of the model.  A session
    is a chain of windows of T frames that overlap by k (RolloverPlan); window w + 1 is queried with the thresholded mask logits that window w
    returned for the frame where it starts (ops.requery_mask: on the device, nothing is read back), its first k frames only fill its cache, and
    the caller sees one unbroken run of frames.  The reported outputs are forward() of each window, built that way, sliced by the reporting
    rule.  A session owns two cache slots (the current and the next window, alternating; cls rows per slot), so capacity // 2 sessions fit.

    Every call becomes ragged steps over (session, window) rows.  Part 1: every session's frames up to and including its hand-off frame, if
    its chunk holds one, for each window live at them; then the one re-query launch; part 2, only if some chunk has frames after its hand-off
    frame: those frames, and the new window from the hand-off frame on.  When the hand-off frame ends the chunk, the pool keeps that RGB frame
    and the next call gives it to the new window with its own frames.  So a call in which no chunk continues past a hand-off frame is exactly
    one Seeker step -- every call of a camera that sends one frame per call -- and any other call exactly two.

    Paged: pages are owned per (session, window); everything both parts need is checked before anything is launched (a refused call moves no
    counter, page or retained frame), and a window's pages return after the step that brings its last frame.  Fed one frame per call a session
    holds at most ceil(T / P) + ceil(k / P) pages (the window that ends and the k warm-up frames of the next), which is what `pages` defaults
    to for capacity // 2 sessions.  A chunk that runs past a window's last frame keeps that window's pages through the step in which the next
    one grows past k frames: up to ceil((k + c - 1) / P) for it; with pages at the default and every session in that phase at once such a
    call can be refused, and feeding it in two calls is always enough."""

    def __init__(self, module, capacity, skinny_gemm=None, page_frames=None, pages=None, cache_dtype=None, rollover=1, requery_threshold=0.0):
        m = getattr(module, 'seeker', module)
        self.plan = RolloverPlan(m.num_total_frames, rollover)
        self.rollover = self.plan.k
        self.requery_threshold = rollover_threshold(requery_threshold)
        capacity = rollover_capacity(capacity)
        _, n_pages = rollover_pages(capacity, m.num_total_frames, self.plan.k, page_frames, pages)
        super().__init__(m, capacity, skinny_gemm, page_frames, n_pages, cache_dtype)       # _slot: session -> its two slots, window w on w & 1
        self._hw = (m.frame_height, m.frame_width)
        self._masks = torch.zeros(capacity, self._hw[0] * self._hw[1], dtype=torch.float32, device=self.device)      # row = the slot of the window it queries
        self._pixels = torch.zeros(capacity, dtype=torch.int32, device=self.device)
        self._keep = {}                 # session -> the hand-off frame (1, 3, 1, H, W) f32 that ended its last chunk
        self._last = {}                 # session -> the row of _masks / _pixels of its last hand-off

    def open(self):
        """A new session at frame 0 on the two smallest free slots; returns its id (ids are never reused)."""
        taken = {s for pair in self._slot.values() for s in pair}
        free = [s for s in range(self.capacity) if s not in taken]
        if len(free) < 2:
            raise TcowError(f'stream_pool.open: {len(free)} of {self.capacity} slots are free and a rollover session takes two; close() a session first')
        sid = self._next_id
        self._next_id += 1
        self._slot[sid], self._done[sid] = (free[0], free[1]), 0
        return sid

    def _forget(self, sid):
        self._keep.pop(sid, None)
        self._last.pop(sid, None)
        if self._alloc is not None:
            self._alloc.release((sid, 0))
            self._alloc.release((sid, 1))

    def close(self, sid):
        """End the session: both slots, the pages of both windows, the retained frame and the pending mask are released."""
        self._known(sid)
        self._forget(sid)
        del self._slot[sid], self._done[sid]

    def reset(self, sid):
        """Put the session back at frame 0 (it keeps its slots; the pages of both windows, the retained frame and the pending mask go)."""
        self._done[self._known(sid)] = 0
        self._forget(sid)

    def window(self, sid):
        """The window that reports the session's next frame."""
        return self.plan.window(self._done[self._known(sid)])

    def pages_of(self, sid):
        """The pages the session owns: those of its older live window in frame order, then those of the newer."""
        a, w = self._paged(), self.plan.window(max(self._done[self._known(sid)] - 1, 0))
        return a.pages_of((sid, w & 1)) + a.pages_of((sid, (w + 1) & 1))

    def _handed(self, sid):
        if self._known(sid) not in self._last:
            raise TcowError(f'stream_pool: session {sid} has had no hand-off yet (the first is frame {self.plan.s})')
        return self._last[sid]

    def requery_mask(self, sid):
        """(1, 1, 1, H, W) f32 on the device: the query mask the session's last hand-off made, returned logits > requery_threshold as 0.0 / 1.0."""
        return self._masks[self._handed(sid)].view(1, 1, 1, *self._hw).clone()

    def requery_pixels(self, sid):
        """A device int32 scalar: the number of ones of requery_mask(sid).  An empty mask is used as it is; this is where the caller sees it."""
        return self._pixels[self._handed(sid)].clone()

    def _check_pages(self, ids, splits):
        """The all-or-nothing page check of a call: part by part, what the rows lack against what is free, a window that ends in a part giving
        its pages back to the next.  Nothing moves."""
        a = self._alloc
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
                    if t0 + c == self.T:
                        ended.append(key)
            if need > free:
                raise TcowError(f'stream_pool: out of pages: this step needs {need} more page(s) of {a.P} frame(s), {free} of {a.n_pages} are free; '
                                'close() or reset() a session, or open the pool with more pages')
            free += sum(held[key] for key in ended) - need
            held.update((key, 0) for key in ended)

    def _roll(self, who, ids, rgbs, qms, per):
        """step() and step_ragged(): every check, then part 1, the re-query launch, part 2 if any chunk goes on after its hand-off frame.  Returns
        per session (mask logits (1, Co, c, H, W), flags (1, c, F) or None) of its c frames."""
        m, plan = self.module, self.plan
        ids = check_sessions(who, ids, len(rgbs) if per else None, len(qms) if per and qms is not None else None, self.capacity, self._slot)
        _check_module(m, self._sig)
        if per:
            cs = [_check_inputs(f'{who}: session {sid}', m, self.device, 1, 1, rgbs[k], None if qms is None else qms[k]) for k, sid in enumerate(ids)]
        else:
            cs = [_check_inputs(who, m, self.device, len(ids), len(ids), rgbs, qms)] * len(ids)
            rgbs, qms = [rgbs[k:k + 1] for k in range(len(ids))], (None if qms is None else [qms[k:k + 1] for k in range(len(ids))])
        g0s = [self._done[sid] for sid in ids]
        splits = [plan.split(g0, c) for g0, c in zip(g0s, cs)]
        if self._alloc is not None:
            self._check_pages(ids, splits)
        HW = self._hw[0] * self._hw[1]
        outs = []                                               # per part: (mask logits, flags, {(session index, window): (first flat frame, its global frame)})
        with torch.no_grad(), torch.cuda.device(self.device):
            rgbs = [r.to(torch.float32) for r in rgbs]
            qms = [None] * len(ids) if qms is None else [None if q is None else q.to(torch.float32) for q in qms]
            for p in range(max(len(sp['parts']) for sp in splits)):
                rows = [(k, *row) for k, sp in enumerate(splits) if p < len(sp['parts']) for row in sp['parts'][p]]
                keys = [(ids[k], w & 1) for k, w, _, _, _ in rows]
                slots = [self._slot[ids[k]][w & 1] for k, w, _, _, _ in rows]
                if self._alloc is not None:
                    self._alloc.grow(keys, [t0 + c for _, _, t0, c, _ in rows])
                step, first = self._ragged_form(keys, [r[2] for r in rows], [r[3] for r in rows], slots)
                rgb_p, qm_p = [], []
                for (k, w, t0, c, g), slot in zip(rows, slots):
                    j = g - g0s[k]                              # -1: the row starts at the frame the call before retained
                    if j < 0:
                        rgb_p.append(self._keep[ids[k]])
                    rgb_p.append(rgbs[k][:, :, max(j, 0):j + c])
                    if w >= 1 and t0 == 0:                      # the window's query: the mask of its hand-off in place of the caller's frame
                        qm_p.append(self._masks[slot].view(1, 1, 1, *self._hw))
                        j, c = j + 1, c - 1
                    if c:
                        qm_p.append(_zero_mask(1, rgbs[k][:, :, j:j + c]) if qms[k] is None else qms[k][:, :, j:j + c])
                rgb_p, qm_p = [t for t in rgb_p if t.shape[2]], [t for t in qm_p if t.shape[2]]
                rgb32 = rgb_p[0].contiguous() if len(rgb_p) == 1 else torch.cat(rgb_p, 2)
                qm32 = qm_p[0].contiguous() if len(qm_p) == 1 else torch.cat(qm_p, 2)
                out_mask, flags = self._forward(step, rgb32, qm32)
                where = {(k, w): (f, g) for (k, w, _, _, g), f in zip(rows, first)}
                outs.append((out_mask, flags, where))
                if p == 0:
                    hand = [(k, sp['handoff']) for k, sp in enumerate(splits) if sp['handoff'] is not None]
                    if hand:
                        src, dst = [], []
                        for k, h in hand:
                            born = h // plan.s
                            f, g = where[(k, born - 1)]          # the older window reports the hand-off frame: channel 0 of flat frame f + h - g
                            src.append((f + h - g) * HW)
                            dst.append(self._slot[ids[k]][born & 1])
                            self._last[ids[k]] = dst[-1]
                        tab = torch.cat([torch.tensor(src, dtype=torch.int64).view(torch.int32), torch.tensor(dst, dtype=torch.int32)]).to(self.device)
                        ops.requery_mask(out_mask, tab[:2 * len(src)].view(torch.int64), self.requery_threshold, self._masks, tab[2 * len(src):], self._pixels)
                if self._alloc is not None:
                    for key, (_, _, t0, c, _) in zip(keys, rows):
                        if t0 + c == self.T:                    # the window has produced its last frame
                            self._alloc.release(key)
            for k, (sid, sp) in enumerate(zip(ids, splits)):
                if sp['keep']:
                    self._keep[sid] = rgbs[k][:, :, -1:].clone()
                else:
                    self._keep.pop(sid, None)
                self._done[sid] += cs[k]
            res = []
            for k, sp in enumerate(splits):
                ms, fs = [], []
                for p, w, g, n in sp['report']:
                    out_mask, flags, where = outs[p]
                    f = where[(k, w)][0] + g - where[(k, w)][1]
                    ms.append(out_mask[:, :, f:f + n])
                    fs.append(None if flags is None else flags[:, f:f + n])
                res.append((ms[0] if len(ms) == 1 else torch.cat(ms, 2), None if fs[0] is None else fs[0] if len(fs) == 1 else torch.cat(fs, 1)))
        return res

    def step(self, ids, rgb, query_mask=None):
        """SeekerStreamPool.step with c <= T - rollover frames per session, at any global frame."""
        res = self._roll('stream_pool.step', ids, rgb, query_mask, False)
        masks = torch.cat([r[0] for r in res], 0) if len(res) > 1 else res[0][0].contiguous()
        return masks, (None if res[0][1] is None else torch.cat([r[1] for r in res], 0))

    def step_ragged(self, ids, rgbs, query_masks=None):
        """SeekerStreamPool.step_ragged with c_i <= T - rollover frames of session i, at any global frame."""
        res = self._roll('stream_pool.step_ragged', ids, list(rgbs), None if query_masks is None else list(query_masks), True)
        return [r[0] for r in res], (None if res[0][1] is None else [r[1] for r in res])

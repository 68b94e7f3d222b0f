"""Streaming inference: the Seeker one chunk of frames at a time, for callers that receive frames live (a camera, a decoder).  This module owns
the tensors, graphs and launches; what is arithmetic on plain ints (tables, refusals, pages, rollover windows) lives in stream_plan.py, runs on
the CPU, and is imported here by name.

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

cache_dtype (net.stream / net.stream_pool; stream_plan.cache_plan is the one place that decides): the element type of the K / V caches, apart from
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
  (the rows form of tcow_attn_temporal_step / tcow_cls_step without a slot table).
  _PoolStep (SeekerStreamPool.step): live sessions that started at different moments, stepped together with one chunk length: a t0 and a
  cache slot per row (the rows form with t0_rows and slot_rows -- the stream's kernels, of which the stream is the case "one t0, slot = row").
  _RaggedStep (SeekerStreamPool.step_ragged): the sessions bring different numbers of frames (cameras at different rates, a decoder's GOP, a
  session that catches up while its neighbours advance by one).  The F = sum of the c_i frames lie flat in session order and run as ONE row
  of F frames; ragged_tables() gives every session its t0, slot, first flat frame and chunk length and every frame its session
  (the ragged form of both entry points: one wave per frame, not per session).

A paged pool (net.stream_pool(capacity, page_frames=P, pages=N)): a contiguous pool reserves a whole stream's cache per slot, whether its session
is at frame 2, at frame 59 or closed.  With page_frames the K / V caches of a block are a heap of N pages of P frames (_PagedState:
[N, S-1, heads, P, 64], a page id valid in every block alike), a session owns only the pages its frames so far have filled (PageAllocator: host
side, lowest free page first, grows when t0 + c crosses a multiple of P), and close() / reset() give them back; the cls rows stay per slot.  The
pool is then sized in memory (pages), and `capacity` only bounds the number of open sessions.  pages defaults to capacity * ceil(T / P), which
cannot run out; with fewer, a step that needs more pages than are free raises TcowError before anything is launched or any counter or page
moves.  Both step() and step_ragged() of a paged pool run a fourth form:

  _PagedRaggedStep: the _RaggedStep tables plus page_rows [n, ceil(T / P)], the sessions' pages in frame order, sent in the same host-to-device
  copy (the paged layout of tcow_attn_temporal_step: the ragged kernel with "page page_rows[r][kt / P], line kt % P" for "slot, line kt"; cls as ragged).

Where a key lives does not enter the arithmetic, so a paged pool gives the bits of the contiguous pool.  A one-frame step costs between nothing measurable
and 0.13 ms more than on the contiguous pool (profiles/stream_paged_latency.json; P = 8 is the recommendation, P = 1 the
dearest): the keywords are off by default.  SeekerStream stays contiguous.

A rollover pool (net.stream_pool(capacity, rollover=k, requery_threshold=0.0) -> SeekerRolloverPool): a stream or a pool session ends at frame
T - 1, because the time table has T rows and the query belongs to frame 0.  With rollover a session is a chain of windows of T frames that
start every T - k frames (stream_plan.RolloverPlan and RolloverCall: all of the host arithmetic); each later window is queried with the thresholded mask logits the window
before it returned for the frame where it starts (ops.requery_mask, tcow_requery_mask: on the device, nothing is read back), its first k frames
only fill its cache, and the reported outputs are forward() of every window built that way.  A session owns two cache slots, a call is one
Seeker step unless a chunk goes on after a hand-off frame (then two), and the steps are the ragged forms above, unchanged.  Without the keyword
a pool is what it was.

Attention maps (step_maps of a stream or pool, step_ragged_maps): the step, run eagerly with a probe (attn_probe.StepMapProbe; attn_maps.StepMapPlan
has the host rules and refusals) that asks the step object for probs_temporal(i, ...) right before attn_temporal -- the softmax rows of the
step's frames against the block's K cache (ops.attn_temporal_step_probs: the caches are only read) -- and launches ops.attn_probs on the
step's own spatial qkv.  The outputs are step()'s, bit for bit; a rollover pool refuses.

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
from .attn_maps import DEFAULT_MAX_BYTES, StepMapPlan
from .attn_probe import StepMapProbe
from .stream_plan import (MAX_FRAMES, PageAllocator, RolloverCall, RolloverPlan, cache_plan, check_range, check_sessions, page_plan,  # noqa: F401
                          ragged_tables, rollover_capacity, rollover_page_moves, rollover_pages, rollover_threshold)

# Default of the skinny_gemm keyword.  True: measured (profiles/stream_skinny_latency.json) -- a one-frame bf16 step takes
# 1.42 ms instead of 2.41 at configs[1] B = 1, 2.41 instead of 3.35 at configs[3] B = 1 and 2.60 instead of 3.24 at configs[1] B = 8, on / off
# alternating in one run, each difference several times the off leg's own max - min.  False runs the steps on tcow_gemm_nt alone.
SKINNY_GEMM_DEFAULT = True
# The same keyword's default when the module's precision is 'bf16x3' (ops.gemm_nt_skinny_x3 where ops.skinny_plan_x3 routes).  True: measured
# (profiles/stream_skinny_x3_latency.json) -- a one-frame bf16x3 step takes 1.94 ms instead of 4.28 at configs[1] B = 1,
# 4.45 instead of 5.88 at configs[3] B = 1 and 5.17 instead of 6.06 at configs[1] B = 8, each difference above the off leg's own max - min.
SKINNY_GEMM_X3_DEFAULT = True


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
    substitutions of block i, attn_temporal and cls_row; a step_maps call also asks probs_temporal, the attention maps of the step's frames
    against the same tables and caches (right before attn_temporal: the caches are only read).  A form is its tables and its ops entry points; it is chosen by constructing one of
    the three classes below, where the tables are built, and nowhere else."""

    def __init__(self, state, time_rows, *tables):
        self.state, self.pos, self.time_rows, self.tables = state, state.pos, time_rows, tables
        self.skinny = state.skinny


class _StreamStep(_Step):
    """tables: t0_dev, the one frame index of all rows (a device scalar: a captured graph reads it); row b works on cache slot b."""

    def attn_temporal(self, i, amode, B, T, S, D, heads, ca, QKV, O):
        st = self.state
        ops.attn_temporal_cached(amode, B, T, S, D, heads, ca, st.T_total, *self.tables, QKV, st.k_cache[i], st.v_cache[i], O, st.cq)

    def probs_temporal(self, i, amode, B, T, S, D, heads, ca, QKV, probs):
        st = self.state
        ops.attn_temporal_step_probs('stream', amode, B, T, S, D, heads, ca, st.T_total, *self.tables, QKV, st.k_cache[i], st.v_cache[i], probs, cache_dtype=st.cq)

    def cls_row(self, i, R2, B, T, S):
        ops.cls_stream(R2, B, T, S, self.state.cls_cache[i], *self.tables)


class _PoolStep(_Step):
    """tables: t0_rows, slot_rows (device int32 [B]): a frame index and a cache slot per row."""

    def attn_temporal(self, i, amode, B, T, S, D, heads, ca, QKV, O):
        st = self.state
        ops.attn_temporal_pool(amode, B, T, S, D, heads, ca, st.T_total, st.n_slots, *self.tables, QKV, st.k_cache[i], st.v_cache[i], O, st.cq)

    def probs_temporal(self, i, amode, B, T, S, D, heads, ca, QKV, probs):
        st = self.state
        ops.attn_temporal_step_probs('pool', amode, B, T, S, D, heads, ca, st.T_total, st.n_slots, *self.tables, QKV, st.k_cache[i], st.v_cache[i], probs,
                                     cache_dtype=st.cq)

    def cls_row(self, i, R2, B, T, S):
        ops.cls_pool(R2, B, T, S, self.state.cls_cache[i], self.state.n_slots, *self.tables)


class _RaggedStep(_Step):
    """tables: t0_rows, slot_rows, first_rows, c_rows (device int32 [n], per session) and row_of_frame ([F], per flat frame); the step is ONE row
    of F = T frames."""

    def attn_temporal(self, i, amode, B, T, S, D, heads, ca, QKV, O):
        st = self.state
        ops.attn_temporal_ragged(amode, self.tables[0].numel(), T, S, D, heads, ca, st.T_total, st.n_slots, *self.tables, QKV, st.k_cache[i],
                                 st.v_cache[i], O, st.cq)

    def probs_temporal(self, i, amode, B, T, S, D, heads, ca, QKV, probs):
        st = self.state
        ops.attn_temporal_step_probs('ragged', amode, self.tables[0].numel(), T, S, D, heads, ca, st.T_total, st.n_slots, *self.tables, QKV, st.k_cache[i],
                                     st.v_cache[i], probs, cache_dtype=st.cq)

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

    def probs_temporal(self, i, amode, B, T, S, D, heads, ca, QKV, probs):
        st = self.state
        t0_rows, _, first_rows, c_rows, row_of_frame, page_rows = self.tables
        ops.attn_temporal_step_probs('paged', amode, t0_rows.numel(), T, S, D, heads, ca, st.T_total, st.n_pages, st.P, t0_rows, page_rows, first_rows, c_rows,
                                     row_of_frame, QKV, st.k_cache[i], st.v_cache[i], probs, cache_dtype=st.cq)


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


def _zero_mask(rows, rgb):
    """The query mask of a step that was given none: all zeros, (rows, 1, c, H, W) for rgb (clips, 3, c, H, W)."""
    return torch.zeros(rows, 1, *rgb.shape[2:], dtype=torch.float32, device=rgb.device)


def _f32(x):
    """An input of a step as the kernels take it: f32 and contiguous (None stays None)."""
    return None if x is None else x.to(torch.float32).contiguous()


def _cat_f32(chunks):
    """Chunks (rows, C, c_i, H, W) as one run of frames, f32 and contiguous."""
    return _f32(chunks[0]) if len(chunks) == 1 else torch.cat([x.to(torch.float32) for x in chunks], 2)


def _seeker_step(module, step, rgb, qm, rows, probe=None):
    """One Seeker step of `rows` query rows (qm None: all zeros) -> (mask logits, flags or None).  probe: the StepMapProbe of a step_maps call."""
    kw = {} if probe is None else {'probe': probe}
    out_mask, flags, _ = engine.run_forward(module, rgb, _zero_mask(rows, rgb) if qm is None else qm, module.param_list(), save=False, stream=step, **kw)
    return out_mask, (flags if module.flag_channels > 0 else None)


def _map_plan(who, module, rows_or_chunks, maps):
    """The StepMapPlan of a step_maps call (`maps`: its blocks, temporal, spatial_slots, max_bytes): every refusal of those arguments, on the host."""
    g = module.geometry(1, T=1)
    blocks, temporal, spatial_slots, max_bytes = maps
    return StepMapPlan(module.network_depth, rows_or_chunks, module.num_total_frames, g['S'], g['heads'], module.causal_attention, blocks, temporal,
                       spatial_slots, DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, who)


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
        return self._step('stream.step', rgb, query_mask, None)[:2]

    def step_maps(self, rgb, query_mask=None, blocks=None, temporal=True, spatial_slots=None, max_bytes=None):
        """step() that also returns what the step's frames look at: (mask logits, flags, maps), the two outputs with the bits of step() on the
        same frames, maps an attn_probe.StepAttentionMaps of this step:
          maps.temporal[i] (rows, N, heads, c, T): block i, how much frame t0 + j of a patch pulls from every frame 0 .. t0 + j of the stream,
                                                   the earlier ones as the K cache holds them (a compact cache: the rounded keys the model attends
                                                   to); later frames +0.0.  Concatenated along dim 3 over the steps: the clip's causal map;
          maps.spatial[i]  (rows, c, nq, heads, S): block i, which slots of its own frame each of spatial_slots looks at -- None: no spatial maps,
                                                   'cls' (causal_attention == 1 only), or a list of slots, 0 = cls, 1 + n = patch n;
          maps.slots, maps.t0: the normalised slots, the step's first frame.
        blocks: None = all, or block indices (negative from the top); max_bytes: budget of the maps (default 4 GiB); tcow_amd/attn_maps.py,
        StepMapPlan, has every rule, and a refused call moves nothing.  On a graph=True stream the call runs eagerly and leaves the captured
        graphs alone: later step() calls replay as before."""
        return self._step('stream.step_maps', rgb, query_mask, (blocks, temporal, spatial_slots, max_bytes))

    def _step(self, who, rgb, query_mask, maps):
        _check_module(self.module, self._sig)
        c = _check_inputs(who, self.module, self.device, self.Bc, self.B, rgb, query_mask)
        t0 = self.frames_done
        if t0 + c > self.T:
            raise TcowError(f'{who}: frames {t0}..{t0 + c - 1} run past the last frame {self.T - 1} of the stream (num_total_frames = {self.T}); '
                            'reset() to start again, or run the camera on net.stream_pool(capacity, rollover=k), whose sessions have no last frame')
        plan = None if maps is None else _map_plan(who, self.module, (self.B, c), maps)
        with torch.no_grad(), torch.cuda.device(self.device):
            step = self._steps.get(c)
            if step is None:
                step = self._steps[c] = _StreamStep(self._st, torch.empty(self.B * c, self._st.D, dtype=torch.float32, device=self.device), self._t0_dev)
            step.time_rows.view(self.B, c, -1).copy_(self._st.time[t0:t0 + c])      # row b*c + j = time row t0 + j, for every b
            self._t0_dev.fill_(t0)
            rgb32, qm32 = _f32(rgb), _f32(query_mask)
            if plan is not None:                    # (eager also on a graph stream: the graphs hold no probe launches and stay as they are)
                probe = StepMapProbe(plan, self.device, t0)
                out = _seeker_step(self.module, step, rgb32, qm32, self.B, probe) + (probe.maps,)
            else:
                out = self._graph_step(step, rgb32, qm32) if self.graph else _seeker_step(self.module, step, rgb32, qm32, self.B)
        self.frames_done = t0 + c
        return out

    def _operand_generation(self):
        """Identifies the module's operand caches (16-bit weight copies, folded projection, row vectors in module._operands).  .cuda() / .to()
        on the same device, set_precision() with the same precision and train-mode forwards replace them without changing a parameter."""
        m = self.module
        return (m._operands.generation, m.mode)

    def _graph_step(self, step, rgb, qm):
        c = rgb.shape[2]
        run = lambda r, q: _seeker_step(self.module, step, r, q, self.B)
        gen = self._operand_generation()
        if any(e['gen'] != gen for e in self._graphs.values()):
            self._graphs.clear()                # captured against replaced operand copies: capture again (the pool of a dropped graph is stream-ordered)
        ent = self._graphs.get(c)
        if ent is None:
            out = run(rgb, qm)                  # this step's result; it also creates every lazily built operand the capture needs
            s_rgb = rgb.clone()
            s_qm = qm.clone() if qm is not None else _zero_mask(self.B, rgb)
            graph = torch.cuda.CUDAGraph()
            # the split-K workspace as the eager step above left it (current stream; the capture runs on a side stream): large enough for this
            # chunk length, so the capture allocates none, and this entry owns the tensor its launches point into
            ws = ops.workspace(0, self.device, 'nt_skinny') if step.skinny else None
            with torch.cuda.graph(graph):
                if ws is None:
                    g_mask, g_flags = run(s_rgb, s_qm)
                else:
                    with ops.pinned_workspace('nt_skinny', ws):
                        g_mask, g_flags = run(s_rgb, s_qm)
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

    def _checked(self, who, ids, rgbs, qms, per, maps=None):
        """Every check of a step (`who`), before anything is launched or any counter moves.  rgbs / qms: one tensor of all sessions, or (per) a list
        with an entry per session.  Returns (ids, the frame every session stands at, the chunk length of every session, in a paged pool the pages
        of every session, grown to hold the step's frames; else None, and the StepMapProbe of a step_maps call -- `maps`: its arguments -- or None)."""
        ids, cs = self._prologue(who, ids, rgbs, qms, per)
        t0s = [self._done[sid] for sid in ids]
        check_range(who, ids, t0s, cs, self.T)
        plan = None if maps is None else _map_plan(who, self.module, list(cs) if per else (len(ids), cs[0]), maps)
        # the last check, and the only thing of a refused step that could have moved: the pages of frames up to t0 + c_i - 1 (all or nothing)
        pages = None if self._alloc is None else self._alloc.grow(ids, [t0 + c for t0, c in zip(t0s, cs)])
        return ids, t0s, cs, pages, (None if plan is None else StepMapProbe(plan, self.device, list(t0s)))

    def _prologue(self, who, ids, rgbs, qms, per):
        """What every pool call (`who`) checks first, in this order: the sessions, the module, the inputs.  Returns (ids, every session's chunk length)."""
        m = self.module
        ids = check_sessions(who, ids, len(rgbs) if per else None, len(qms) if per and qms is not None else None, self.capacity, self._slot)
        _check_module(m, self._sig)
        if per:
            return ids, [_check_inputs(f'{who}: session {sid}', m, self.device, 1, 1, rgbs[k], None if qms is None else qms[k]) for k, sid in enumerate(ids)]
        return ids, [_check_inputs(who, m, self.device, len(ids), len(ids), rgbs, qms)] * len(ids)

    def _run(self, step, ids, cs, rgb, qm, probe=None):
        """One Seeker step, after which every session has moved on by its chunk length."""
        out = _seeker_step(self.module, step, rgb, qm, rgb.shape[0], probe)
        for sid, c in zip(ids, cs):
            self._done[sid] += c
        return out

    def step(self, ids, rgb, query_mask=None):
        """ids: n distinct open sessions, at any phases; rgb (n, 3, c, H, W), query_mask (n, 1, c, H, W) or None (all zeros): the next c >= 1
        frames of each -> (mask logits (n, Co, c, H, W) f32, flags (n, c, F) or None) in the order of `ids`, owned by the caller.  Every check
        runs before anything is launched: a refused step leaves every session where it was."""
        return self._step('stream_pool.step', ids, rgb, query_mask, None)

    def step_maps(self, ids, rgb, query_mask=None, blocks=None, temporal=True, spatial_slots=None, max_bytes=None):
        """step() that also returns the attention maps of the step's frames against the sessions' caches: (mask logits, flags, maps) -- the
        keywords, shapes and rules of SeekerStream.step_maps, rows in the order of `ids`, maps.t0 the frame every session stood at.  A paged pool
        and any cache_dtype are served alike; a refused call moves no counter and allocates no page."""
        return self._step('stream_pool.step_maps', ids, rgb, query_mask, (blocks, temporal, spatial_slots, max_bytes))

    def _step(self, who, ids, rgb, query_mask, maps):
        ids, t0s, cs, pages, probe = self._checked(who, ids, rgb, query_mask, False, maps)
        more = () if probe is None else (probe.maps,)
        if pages is not None:
            return self._step_paged(ids, t0s, cs, pages, rgb, query_mask, probe) + more
        st, c = self._st, cs[0]
        with torch.no_grad(), torch.cuda.device(self.device):
            t0_rows = torch.tensor(t0s, dtype=torch.int32, device=self.device)
            slot_rows = torch.tensor([self._slot[sid] for sid in ids], dtype=torch.int32, device=self.device)
            frames = (t0_rows[:, None] + torch.arange(c, dtype=torch.int32, device=self.device)[None, :]).reshape(-1)
            step = _PoolStep(st, st.time.index_select(0, frames), t0_rows, slot_rows)         # [n*c, D]: row r*c + j = time row t0_rows[r] + j
            return self._run(step, ids, cs, _f32(rgb), _f32(query_mask), probe) + more

    def _ragged_form(self, t0s, slots, cs, pages):
        """The step object of a ragged step (inside no_grad on the pool's device) and every row's first flat frame.  pages: None, or in a paged
        pool every row's pages (PageAllocator.grow's), sent in the same host-to-device copy as the other tables."""
        n, st = len(t0s), self._st
        tab = ragged_tables(t0s, slots, cs)
        F = len(tab['frames'])
        # all tables in one host-to-device copy: [t0 | slot | first | c] per session, [row_of_frame | frames] per flat frame, [pages] per session
        flat = tab['t0'] + tab['slot'] + tab['first'] + tab['c'] + tab['row_of_frame'] + tab['frames']
        for own in pages or ():
            flat += list(own) + [-1] * (st.pps - len(own))
        dev = torch.tensor(flat, dtype=torch.int32).to(self.device)
        time_rows = st.time.index_select(0, dev[4 * n + F:4 * n + 2 * F])               # [F, D]: flat frame f = time row t0 + j of its session
        tables = (dev[0:n], dev[n:2 * n], dev[2 * n:3 * n], dev[3 * n:4 * n], dev[4 * n:4 * n + F])
        if pages is None:
            return _RaggedStep(st, time_rows, *tables), tab['first']
        return _PagedRaggedStep(st, time_rows, *tables, dev[4 * n + 2 * F:].view(n, st.pps)), tab['first']

    def _step_paged(self, ids, t0s, cs, pages, rgb, query_mask, probe=None):
        """step() of a paged pool: the ragged form with equal chunk lengths (bit-equal to the pool form), in and out in step()'s shapes."""
        n, c = len(ids), cs[0]
        # (n, C, c, H, W) -> (1, C, n*c, H, W): the frames flat in session order
        flat = lambda x: x.to(torch.float32).transpose(0, 1).reshape(1, x.shape[1], n * c, *x.shape[3:]).contiguous()
        with torch.no_grad(), torch.cuda.device(self.device):
            step, _ = self._ragged_form(t0s, [self._slot[sid] for sid in ids], cs, pages)
            out_mask, flags = self._run(step, ids, cs, flat(rgb), None if query_mask is None else flat(query_mask), probe)
            out_mask = out_mask.view(out_mask.shape[1], n, c, *out_mask.shape[3:]).transpose(0, 1).contiguous()
        return out_mask, (None if flags is None else flags.reshape(n, c, -1))

    def step_ragged(self, ids, rgbs, query_masks=None):
        """ids: n distinct open sessions, at any phases; rgbs: n tensors (1, 3, c_i, H, W), the next c_i >= 1 frames of each session (the c_i need
        not be equal); query_masks: None, or n entries, each None (all zeros) or (1, 1, c_i, H, W) -> (a list of n mask-logit tensors
        (1, Co, c_i, H, W) f32, a list of n flag tensors (1, c_i, F) or None), in the order of `ids`.  The outputs are slices of buffers allocated
        for this step and owned by the caller.  The whole step is ONE Seeker step over the sum of the c_i frames.  Every check runs before anything
        is launched: a refused step leaves every session where it was."""
        return self._step_ragged('stream_pool.step_ragged', ids, rgbs, query_masks, None)

    def step_ragged_maps(self, ids, rgbs, query_masks=None, blocks=None, temporal=True, spatial_slots=None, max_bytes=None):
        """step_ragged() that also returns the attention maps, per session: (masks, flags, maps) with maps.temporal[i][k] (1, N, heads, c_k, T)
        and maps.spatial[i][k] (1, c_k, nq, heads, S) of session ids[k]; the keywords and rules of SeekerStream.step_maps."""
        return self._step_ragged('stream_pool.step_ragged_maps', ids, rgbs, query_masks, (blocks, temporal, spatial_slots, max_bytes))

    def _step_ragged(self, who, ids, rgbs, query_masks, maps):
        rgbs = list(rgbs)
        qms = None if query_masks is None else list(query_masks)
        ids, t0s, cs, pages, probe = self._checked(who, ids, rgbs, qms, True, maps)
        with torch.no_grad(), torch.cuda.device(self.device):
            step, first = self._ragged_form(t0s, [self._slot[sid] for sid in ids], cs, pages)
            rgb32 = _cat_f32(rgbs)
            if qms is not None and all(q is not None for q in qms):
                qm32 = _cat_f32(qms)
            else:
                qm32 = _zero_mask(1, rgb32)
                for q, f0, c in zip(qms or (), first, cs):
                    if q is not None:
                        qm32[:, :, f0:f0 + c] = q
            out_mask, flags = self._run(step, ids, cs, rgb32, qm32, probe)
        masks = [out_mask[:, :, f0:f0 + c] for f0, c in zip(first, cs)]
        return (masks, (None if flags is None else [flags[:, f0:f0 + c] for f0, c in zip(first, cs)])) + (() if probe is None else (probe.maps,))


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

    def _roll(self, who, ids, rgbs, qms, per):
        """step() and step_ragged(): every check, then part 1, the re-query launch, part 2 if any chunk goes on after its hand-off frame.  Returns
        per session (mask logits (1, Co, c, H, W), flags (1, c, F) or None) of its c frames."""
        ids, cs = self._prologue(who, ids, rgbs, qms, per)
        n = len(ids)
        if not per:
            rgbs, qms = [rgbs[k:k + 1] for k in range(n)], (None if qms is None else [qms[k:k + 1] for k in range(n)])
        call = RolloverCall(self.plan, [self._done[sid] for sid in ids], cs)
        if self._alloc is not None:                             # all or nothing: both parts' page moves on a copy, before anything is launched
            trial = self._alloc.copy()
            for rows in call.parts:
                rollover_page_moves(trial, self.T, ids, rows)
        HW = self._hw[0] * self._hw[1]
        outs = []                                               # per part: (mask logits, flags)
        with torch.no_grad(), torch.cuda.device(self.device):
            rgbs = [r.to(torch.float32) for r in rgbs]
            qms = [None] * n if qms is None else [None if q is None else q.to(torch.float32) for q in qms]
            for p, rows in enumerate(call.parts):
                slots = [self._slot[ids[r.k]][r.w & 1] for r in rows]
                pages = None if self._alloc is None else rollover_page_moves(self._alloc, self.T, ids, rows)
                step, _ = self._ragged_form([r.t0 for r in rows], slots, [r.c for r in rows], pages)
                rgb_p, qm_p = [], []
                for r, slot in zip(rows, slots):
                    if r.kept:
                        rgb_p.append(self._keep[ids[r.k]])
                    rgb_p.append(rgbs[r.k][:, :, r.lo:r.hi])
                    if r.handed:                                # the window's query: the mask of its hand-off in place of the caller's frame
                        qm_p.append(self._masks[slot].view(1, 1, 1, *self._hw))
                    if r.qlo < r.hi:
                        qm_p.append(_zero_mask(1, rgbs[r.k][:, :, r.qlo:r.hi]) if qms[r.k] is None else qms[r.k][:, :, r.qlo:r.hi])
                outs.append(_seeker_step(self.module, step, _cat_f32(rgb_p), _cat_f32(qm_p), 1))
                if p == 0 and call.handoffs:                    # channel 0 of the flat frame at which the older window reports the hand-off frame
                    src = [f * HW for _, _, f in call.handoffs]
                    dst = [self._slot[ids[k]][born & 1] for k, born, _ in call.handoffs]
                    self._last.update((ids[k], d) for (k, _, _), d in zip(call.handoffs, dst))
                    tab = torch.cat([torch.tensor(src, dtype=torch.int64).view(torch.int32), torch.tensor(dst, dtype=torch.int32)]).to(self.device)
                    ops.requery_mask(outs[0][0], tab[:2 * len(src)].view(torch.int64), self.requery_threshold, self._masks, tab[2 * len(src):], self._pixels)
            for k, sid in enumerate(ids):
                if call.keep[k]:
                    self._keep[sid] = rgbs[k][:, :, -1:].clone()
                else:
                    self._keep.pop(sid, None)
                self._done[sid] += cs[k]
            res = []
            for runs in call.report:
                ms = [outs[p][0][:, :, f:f + c] for p, f, c in runs]
                fs = [None if outs[p][1] is None else outs[p][1][:, f:f + c] for p, f, c in runs]
                res.append((ms[0] if len(ms) == 1 else torch.cat(ms, 2), None if fs[0] is None else fs[0] if len(fs) == 1 else torch.cat(fs, 1)))
        return res

    def step(self, ids, rgb, query_mask=None):
        """SeekerStreamPool.step with c <= T - rollover frames per session, at any global frame."""
        res = self._roll('stream_pool.step', ids, rgb, query_mask, False)
        masks = torch.cat([r[0] for r in res], 0) if len(res) > 1 else res[0][0].contiguous()
        return masks, (None if res[0][1] is None else torch.cat([r[1] for r in res], 0))

    def step_maps(self, *args, **kwargs):
        """Refused: a rollover session's frames are window-relative and a hand-off step runs two windows; maps of it need a design of their own."""
        raise TcowError('stream_pool.step_maps: a rollover pool (rollover=k) serves no attention maps: frame indices are relative to a window and a '
                        'hand-off frame belongs to two; use a pool without rollover')

    def step_ragged_maps(self, *args, **kwargs):
        """Refused, as step_maps."""
        raise TcowError('stream_pool.step_ragged_maps: a rollover pool (rollover=k) serves no attention maps: frame indices are relative to a window '
                        'and a hand-off frame belongs to two; use a pool without rollover')

    def step_ragged(self, ids, rgbs, query_masks=None):
        """SeekerStreamPool.step_ragged with c_i <= T - rollover frames of session i, at any global frame."""
        res = self._roll('stream_pool.step_ragged', ids, list(rgbs), None if query_masks is None else list(query_masks), True)
        return [r[0] for r in res], (None if res[0][1] is None else [r[1] for r in res])

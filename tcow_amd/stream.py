"""Streaming inference: the Seeker one chunk of frames at a time, for callers that receive frames live (a camera, a decoder).

With causal_attention 1 or 2 the model is causal along time: frame t's mask logits and flags depend on frames 0..t only (the tril() mask of
vit.py:93-99, the cls row taken from frame 0, vit.py:192-198; everything else works per token or per frame).  A SeekerStream therefore runs
the eval schedule of engine.run_forward on the c new frames of a step alone, with three substitutions (see run_forward's `stream`): the
chunk's rows of the time table, temporal attention against a per-block K / V cache of the earlier frames (tcow_attn_temporal_cached_fwd, which
also appends the chunk's K / V), and for causal_attention == 1 the cls row of frame 0 kept per block (tcow_cls_stream).  For any split of
0..T-1 into chunks the concatenated outputs equal forward() of the whole clip, to the precision mode's rounding.

State, allocated once by stream(): per block a K and a V cache [B, S-1, heads, T, 64] in the mode's storage type (16-bit modes: bf16 / binary16;
fp32 and bf16x3: f32) with B = clips x queries (the query mask changes every token's K / V), and one f32 cls row per query row.  At BASELINE
configs[1] (T = 30, 240x320, depth 12) that is 332 MB per query row in the 16-bit modes; at configs[3] (T = 60, 480x640) 2.65 GB; f32 twice that.

graph=True: the first step of each chunk length c runs eagerly and captures the step as a torch.cuda.CUDAGraph; later steps copy their inputs
into the graph's static buffers, write t0 (a device scalar the kernels read) and replay.  No step synchronises the host except the one capture
per chunk length.  A graph keeps the module's operand copies it was captured with alive; when the module replaces them (.cuda() / .to() on
the same device, set_precision() with the same precision, a train-mode forward) the graphs are dropped and captured again.

SeekerStreamPool (net.stream_pool(capacity)): live sessions that started at different moments, stepped together.  The three substitutions
depend on a row's own frame index only, so a pool step is one Seeker step whose rows each carry their own t0 and their own cache slot
(tcow_attn_temporal_pool_fwd, tcow_cls_pool; the time rows are gathered per row).  The pool holds the state of `capacity` one-row streams:
per block K / V caches [capacity, S-1, heads, T, 64] and one cls row per slot.  Pool steps run eagerly.

pool.step_ragged(ids, rgbs, query_masks): the sessions of one step bring different numbers of frames (cameras at different rates, a decoder's
GOP, a session that catches up or prefills its history while its neighbours advance by one).  The step's F = sum of the c_i frames lie flat
in session order and run as ONE row of F frames; ragged_tables() gives every session its t0, slot, first flat frame and chunk length and every
frame its session, and the two substitutions are tcow_attn_temporal_ragged_fwd (one wave per frame, not per session) and tcow_cls_ragged.
"""
import torch

from . import engine, ops
from ._lib import TcowError


class _StepState:
    """What engine.run_forward substitutes for a stream step."""
    __slots__ = ('T_total', 't0_dev', 'pos', 'time_rows', 'k_cache', 'v_cache', 'cls_cache', 't0_rows', 'slot_rows', 'n_slots', 'first_rows', 'c_rows',
                 'row_of_frame')

    def __init__(self):
        self.t0_rows = self.slot_rows = self.n_slots = None       # set by a pool step only: a frame index and a cache slot per row
        self.first_rows = self.c_rows = self.row_of_frame = None  # set by a ragged pool step only: a first flat frame and a chunk length per session, a session per frame


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


def _new_state(module, rows):
    """(state with the caches of `rows` rows allocated, effective time table [T, D], geometry) -- what a stream and a pool both start from."""
    g = module.geometry(rows)
    dev = module.vit.pos_embed.device
    cdt = ops.tdtype(module.mode)                           # (bf16x3 stores f32, like fp32)
    T = module.num_total_frames
    shape = (module.network_depth, rows, g['S'] - 1, g['heads'], T, 64)
    st = _StepState()
    st.T_total = T
    st.k_cache = torch.empty(shape, dtype=cdt, device=dev)
    st.v_cache = torch.empty(shape, dtype=cdt, device=dev)
    st.cls_cache = torch.empty(module.network_depth, rows, g['D'], dtype=torch.float32, device=dev)
    with torch.no_grad():
        st.pos, time, _, _ = engine._effective_embeddings(module, g)            # (nearest-resized when the stored tables differ)
    st.time_rows = None
    return st, time, g


def _cache_bytes(st):
    return sum(t.numel() * t.element_size() for t in (st.k_cache, st.v_cache, st.cls_cache))


def _check_module(module, sig):
    """The module can still be streamed and is the one the caches were filled by."""
    check_streamable(module)
    if _signature(module) != sig:
        raise TcowError('stream: a parameter (or the precision) changed since the stream was opened; the cached keys / values belong to the old '
                        'weights -- open a new stream')


def _check_step(who, module, sig, device, clips, rows, rgb, query_mask):
    """The checks of a step that do not depend on where its rows stand; returns the chunk length c."""
    _check_module(module, sig)
    return _check_inputs(who, module, device, clips, rows, rgb, query_mask)


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


def check_ragged_sessions(ids, n_rgbs, n_masks, capacity, open_ids):
    """The checks of step_ragged that look at the lists alone: 1 .. capacity sessions, one rgb entry (and one query-mask entry, unless the list
    is None: n_masks None) per session, every id open, none twice.  Returns the ids as a list."""
    ids = list(ids)
    n = len(ids)
    if n < 1 or n > capacity:
        raise TcowError(f'stream_pool.step_ragged: {n} sessions given; a step takes 1 .. capacity = {capacity}')
    if n_rgbs != n or (n_masks is not None and n_masks != n):
        raise TcowError(f'stream_pool.step_ragged: {n} ids, {n_rgbs} rgb entries' + ('' if n_masks is None else f', {n_masks} query_masks entries')
                        + ': the lengths must agree (one entry per session)')
    seen = set()
    for sid in ids:
        if sid not in open_ids:
            raise TcowError(f'stream_pool: session {sid!r} is not open (unknown or closed id)')
        if sid in seen:
            raise TcowError(f'stream_pool.step_ragged: duplicate session {sid!r}: a session is one run of frames of a step')
        seen.add(sid)
    return ids


def check_ragged_range(ids, t0s, cs, T):
    """No session runs past the last frame: frames_done + c_i <= T for every session, the offender named."""
    for sid, t0, c in zip(ids, t0s, cs):
        if t0 + c > T:
            raise TcowError(f'stream_pool.step_ragged: session {sid}: frames {t0}..{t0 + c - 1} run past the last frame {T - 1} of the stream '
                            f'(num_total_frames = {T}); reset() or close() it')


class SeekerStream:
    """net.stream(batch_size, queries_per_clip, graph) of Seeker / QueryMaskTracker; see the module docstring."""

    def __init__(self, module, batch_size=1, queries_per_clip=1, graph=False):
        module = getattr(module, 'seeker', module)
        check_streamable(module)
        Bc, Qs = int(batch_size), int(queries_per_clip)
        if Bc < 1 or Qs < 1:
            raise TcowError(f'stream: batch_size ({Bc}) and queries_per_clip ({Qs}) must be >= 1')
        self.module = module
        self.Bc, self.Qs, self.B = Bc, Qs, Bc * Qs
        self.T = module.num_total_frames
        self.graph = bool(graph)
        st, self._time, g = _new_state(module, self.B)
        self._S, self._D = g['S'], g['D']
        self.device = st.pos.device
        st.t0_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._st = st
        self._time_rows = {}            # c -> static [c, D] f32 time rows of the step
        self._graphs = {}               # c -> (graph, static rgb, static query mask, output mask, flags)
        self._sig = _signature(module)
        self.frames_done = 0

    @property
    def cache_bytes(self):
        """Device bytes of the K / V caches and the cls rows."""
        return _cache_bytes(self._st)

    def reset(self):
        """Start again at frame 0 (the buffers, and any captured graphs, are kept)."""
        self.frames_done = 0

    def step(self, rgb, query_mask=None):
        """rgb (Bc, 3, c, H, W), query_mask (Bc*Qs, 1, c, H, W) or None (all zeros) for the next c >= 1 frames ->
        (mask logits (Bc*Qs, Co, c, H, W) f32, flags (Bc*Qs, c, F) or None) of exactly those frames, owned by the caller."""
        c = _check_step('stream.step', self.module, self._sig, self.device, self.Bc, self.B, rgb, query_mask)
        t0 = self.frames_done
        if t0 + c > self.T:
            raise TcowError(f'stream.step: frames {t0}..{t0 + c - 1} run past the last frame {self.T - 1} of the stream (num_total_frames = {self.T}); '
                            'reset() to start again')
        with torch.no_grad(), torch.cuda.device(self.device):
            tr = self._time_rows.get(c)
            if tr is None:
                tr = self._time_rows[c] = torch.empty(c, self._D, dtype=torch.float32, device=self.device)
            tr.copy_(self._time[t0:t0 + c])
            self._st.t0_dev.fill_(t0)
            self._st.time_rows = tr
            rgb32 = rgb.to(torch.float32).contiguous()
            qm32 = None if query_mask is None else query_mask.to(torch.float32).contiguous()
            out = self._graph_step(c, rgb32, qm32) if self.graph else self._run(rgb32, qm32)
        self.frames_done = t0 + c
        return out

    def _run(self, rgb, qm):
        m = self.module
        if qm is None:
            qm = torch.zeros(self.B, 1, rgb.shape[2], rgb.shape[3], rgb.shape[4], dtype=torch.float32, device=rgb.device)
        out_mask, flags, _ = engine.run_forward(m, rgb, qm, m.param_list(), save=False, stream=self._st)
        return out_mask, (flags if m.flag_channels > 0 else None)

    def _operand_generation(self):
        """Identifies the module's operand caches (16-bit weight copies, folded projection, row vectors in module._operands).  .cuda() / .to()
        on the same device, set_precision() with the same precision and train-mode forwards replace them without changing a parameter."""
        m = self.module
        return (m._operands.generation, m.mode)

    def _graph_step(self, c, rgb, qm):
        gen = self._operand_generation()
        if any(e['gen'] != gen for e in self._graphs.values()):
            self._graphs.clear()                # captured against replaced operand copies: capture again (the pool of a dropped graph is stream-ordered)
        ent = self._graphs.get(c)
        if ent is None:
            out = self._run(rgb, qm)            # this step's result; it also creates every lazily built operand the capture needs
            s_rgb = rgb.clone()
            s_qm = qm.clone() if qm is not None else torch.zeros(self.B, 1, *rgb.shape[2:], dtype=torch.float32, device=rgb.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                g_mask, g_flags = self._run(s_rgb, s_qm)
            # The graph holds raw pointers into tensors that only module._operands owns (operand copies, folded W' / b', mask0): a shallow copy
            # of the dictionary keeps them alive as long as the graph, whatever later replaces the dictionary or its entries.
            keep = self.module._operands.keep_alive()
            self._graphs[c] = dict(graph=graph, rgb=s_rgb, qm=s_qm, mask=g_mask, flags=g_flags, gen=self._operand_generation(), keep=keep)
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
    """net.stream_pool(capacity) of Seeker / QueryMaskTracker: up to `capacity` live sessions (one clip and one query mask each) that stand at
    different frames, stepped together; see the module docstring.  open() -> id, step(ids, rgb, query_mask) (one chunk length for all) or
    step_ragged(ids, rgbs, query_masks) (a chunk length per session), close(id)."""

    def __init__(self, module, capacity):
        module = getattr(module, 'seeker', module)
        capacity = int(capacity)
        if capacity < 1:
            raise TcowError(f'stream_pool: capacity ({capacity}) must be >= 1')
        check_streamable(module)
        self.module = module
        self.capacity = capacity
        self.T = module.num_total_frames
        st, self._time, g = _new_state(module, capacity)
        st.n_slots = capacity
        self._st = st
        rg = self._st_ragged = _StepState()        # the state of a ragged step: the same caches, its own tables (step() never sees them)
        rg.T_total, rg.n_slots, rg.pos, rg.k_cache, rg.v_cache, rg.cls_cache = st.T_total, st.n_slots, st.pos, st.k_cache, st.v_cache, st.cls_cache
        self.device = st.pos.device
        self._sig = _signature(module)
        self._slot = {}                 # open session id -> cache slot
        self._done = {}                 # open session id -> frames consumed
        self._next_id = 0

    @property
    def cache_bytes(self):
        """Device bytes of the K / V caches and the cls rows of all `capacity` slots."""
        return _cache_bytes(self._st)

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
        """End the session; its slot is free for the next open()."""
        self._known(sid)
        del self._slot[sid], self._done[sid]

    def frames_done(self, sid):
        return self._done[self._known(sid)]

    def reset(self, sid):
        """Put the session back at frame 0 (it keeps its slot)."""
        self._done[self._known(sid)] = 0

    def step(self, ids, rgb, query_mask=None):
        """ids: n distinct open sessions, at any phases; rgb (n, 3, c, H, W), query_mask (n, 1, c, H, W) or None (all zeros): the next c >= 1
        frames of each -> (mask logits (n, Co, c, H, W) f32, flags (n, c, F) or None) in the order of `ids`, owned by the caller.  Every check
        runs before anything is launched: a refused step leaves every session where it was."""
        m = self.module
        ids = list(ids)
        n = len(ids)
        if n < 1 or n > self.capacity:
            raise TcowError(f'stream_pool.step: {n} sessions given; a step takes 1 .. capacity = {self.capacity}')
        seen = set()
        for sid in ids:
            if sid in seen:
                raise TcowError(f'stream_pool.step: duplicate session {sid!r}: a session is one row of a step')
            seen.add(self._known(sid))
        c = _check_step('stream_pool.step', m, self._sig, self.device, n, n, rgb, query_mask)
        t0s = [self._done[sid] for sid in ids]
        for sid, t0 in zip(ids, t0s):
            if t0 + c > self.T:
                raise TcowError(f'stream_pool.step: session {sid}: frames {t0}..{t0 + c - 1} run past the last frame {self.T - 1} of the stream '
                                f'(num_total_frames = {self.T}); reset() or close() it')
        st = self._st
        with torch.no_grad(), torch.cuda.device(self.device):
            st.t0_rows = torch.tensor(t0s, dtype=torch.int32, device=self.device)
            st.slot_rows = torch.tensor([self._slot[sid] for sid in ids], dtype=torch.int32, device=self.device)
            frames = (st.t0_rows[:, None] + torch.arange(c, dtype=torch.int32, device=self.device)[None, :]).reshape(-1)
            st.time_rows = self._time.index_select(0, frames)                   # [n*c, D]: row r*c + j = time row t0_rows[r] + j
            rgb32 = rgb.to(torch.float32).contiguous()
            if query_mask is None:
                qm32 = torch.zeros(n, 1, c, rgb.shape[3], rgb.shape[4], dtype=torch.float32, device=self.device)
            else:
                qm32 = query_mask.to(torch.float32).contiguous()
            out_mask, flags, _ = engine.run_forward(m, rgb32, qm32, m.param_list(), save=False, stream=st)
        for sid in ids:
            self._done[sid] += c
        return out_mask, (flags if m.flag_channels > 0 else None)

    def step_ragged(self, ids, rgbs, query_masks=None):
        """ids: n distinct open sessions, at any phases; rgbs: n tensors (1, 3, c_i, H, W), the next c_i >= 1 frames of each session (the c_i need
        not be equal); query_masks: None, or n entries, each None (all zeros) or (1, 1, c_i, H, W) -> (a list of n mask-logit tensors
        (1, Co, c_i, H, W) f32, a list of n flag tensors (1, c_i, F) or None), in the order of `ids`.  The outputs are slices of buffers allocated
        for this step and owned by the caller.  The whole step is ONE Seeker step over the sum of the c_i frames.  Every check runs before anything
        is launched: a refused step leaves every session where it was."""
        m = self.module
        rgbs = list(rgbs)
        qms = None if query_masks is None else list(query_masks)
        ids = check_ragged_sessions(ids, len(rgbs), None if qms is None else len(qms), self.capacity, self._slot)
        n = len(ids)
        _check_module(m, self._sig)
        cs = [_check_inputs(f'stream_pool.step_ragged: session {sid}', m, self.device, 1, 1, rgbs[k], None if qms is None else qms[k])
              for k, sid in enumerate(ids)]
        t0s = [self._done[sid] for sid in ids]
        check_ragged_range(ids, t0s, cs, self.T)
        tab = ragged_tables(t0s, [self._slot[sid] for sid in ids], cs)
        F = len(tab['frames'])
        st = self._st_ragged
        with torch.no_grad(), torch.cuda.device(self.device):
            # all six tables in one host-to-device copy: [t0 | slot | first | c] per session, [row_of_frame | frames] per flat frame
            dev = torch.tensor(tab['t0'] + tab['slot'] + tab['first'] + tab['c'] + tab['row_of_frame'] + tab['frames'], dtype=torch.int32).to(self.device)
            st.t0_rows, st.slot_rows, st.first_rows, st.c_rows = dev[0:n], dev[n:2 * n], dev[2 * n:3 * n], dev[3 * n:4 * n]
            st.row_of_frame = dev[4 * n:4 * n + F]
            st.time_rows = self._time.index_select(0, dev[4 * n + F:])             # [F, D]: flat frame f = time row t0 + j of its session
            H, W = m.frame_height, m.frame_width
            rgb32 = rgbs[0].to(torch.float32).contiguous() if n == 1 else torch.cat([r.to(torch.float32) for r in rgbs], 2)
            if qms is not None and all(q is not None for q in qms):
                qm32 = qms[0].to(torch.float32).contiguous() if n == 1 else torch.cat([q.to(torch.float32) for q in qms], 2)
            else:
                qm32 = torch.zeros(1, 1, F, H, W, dtype=torch.float32, device=self.device)
                for q, f0, c in zip(qms or (), tab['first'], cs):
                    if q is not None:
                        qm32[:, :, f0:f0 + c] = q
            out_mask, flags, _ = engine.run_forward(m, rgb32, qm32, m.param_list(), save=False, stream=st)
        for sid, c in zip(ids, cs):
            self._done[sid] += c
        masks = [out_mask[:, :, f0:f0 + c] for f0, c in zip(tab['first'], cs)]
        return masks, ([flags[:, f0:f0 + c] for f0, c in zip(tab['first'], cs)] if m.flag_channels > 0 else None)

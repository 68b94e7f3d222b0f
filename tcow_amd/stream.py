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
"""
import torch

from . import engine, ops
from ._lib import TcowError


class _StepState:
    """What engine.run_forward substitutes for a stream step."""
    __slots__ = ('T_total', 't0_dev', 'pos', 'time_rows', 'k_cache', 'v_cache', 'cls_cache')


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
        g = module.geometry(self.B)
        self._S, self._D = g['S'], g['D']
        dev = module.vit.pos_embed.device
        self.device = dev
        cdt = ops.tdtype(module.mode)                       # (bf16x3 stores f32, like fp32)
        shape = (module.network_depth, self.B, g['S'] - 1, g['heads'], self.T, 64)
        st = _StepState()
        st.T_total = self.T
        st.k_cache = torch.empty(shape, dtype=cdt, device=dev)
        st.v_cache = torch.empty(shape, dtype=cdt, device=dev)
        st.cls_cache = torch.empty(module.network_depth, self.B, g['D'], dtype=torch.float32, device=dev)
        st.t0_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.no_grad():
            st.pos, self._time, _, _ = engine._effective_embeddings(module, g)        # (nearest-resized when the stored tables differ)
        st.time_rows = None
        self._st = st
        self._time_rows = {}            # c -> static [c, D] f32 time rows of the step
        self._graphs = {}               # c -> (graph, static rgb, static query mask, output mask, flags)
        self._sig = _signature(module)
        self.frames_done = 0

    @property
    def cache_bytes(self):
        """Device bytes of the K / V caches and the cls rows."""
        st = self._st
        return sum(t.numel() * t.element_size() for t in (st.k_cache, st.v_cache, st.cls_cache))

    def reset(self):
        """Start again at frame 0 (the buffers, and any captured graphs, are kept)."""
        self.frames_done = 0

    def step(self, rgb, query_mask=None):
        """rgb (Bc, 3, c, H, W), query_mask (Bc*Qs, 1, c, H, W) or None (all zeros) for the next c >= 1 frames ->
        (mask logits (Bc*Qs, Co, c, H, W) f32, flags (Bc*Qs, c, F) or None) of exactly those frames, owned by the caller."""
        m = self.module
        check_streamable(m)
        if _signature(m) != self._sig:
            raise TcowError('stream: a parameter (or the precision) changed since the stream was opened; the cached keys / values belong to the old '
                            'weights -- open a new stream')
        if not torch.is_tensor(rgb) or rgb.dim() != 5 or rgb.shape[0] != self.Bc or rgb.shape[1] != 3 or rgb.shape[2] < 1 \
                or rgb.shape[3] != m.frame_height or rgb.shape[4] != m.frame_width:
            raise TcowError(f'stream.step: rgb must be ({self.Bc}, 3, c >= 1, {m.frame_height}, {m.frame_width}), got '
                            f'{tuple(rgb.shape) if torch.is_tensor(rgb) else type(rgb).__name__}')
        c = int(rgb.shape[2])
        if query_mask is not None and (not torch.is_tensor(query_mask) or tuple(query_mask.shape) != (self.B, 1, c, m.frame_height, m.frame_width)):
            raise TcowError(f'stream.step: query_mask must be ({self.B}, 1, {c}, {m.frame_height}, {m.frame_width}) or None, got '
                            f'{tuple(query_mask.shape) if torch.is_tensor(query_mask) else type(query_mask).__name__}')
        for t in (rgb, query_mask):
            if t is not None and (not t.is_cuda or t.device != self.device):
                raise TcowError(f'stream.step: inputs must be on the stream device {self.device}, got {t.device}')
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

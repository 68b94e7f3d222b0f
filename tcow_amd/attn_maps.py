"""Host arithmetic of Seeker.attention_maps: what the arguments mean, where a (frame, slot) query sits in the sequences the attention kernels run
over, the shapes and bytes of the maps, and every refusal -- all of it before a launch.  No device, module or tensor in here (the probe that
launches ops.attn_probs is tcow_amd/attn_probe.py); tests/test_attn_maps_plan_host.py pins it on the CPU.  The same for the maps of a live
stream or pool step against its cache (StepMapPlan, at the end; tests/test_step_map_plan_host.py).

A query is (frame, slot): slot 0 is the cls token, slot 1 + n patch n = h' * W' + w' of that frame.
  divided_space_time: the spatial sequences are those of tcow_attn_spatial_fwd, one per (clip, frame) over slots s0 .. S-1, s0 = 0 when
      causal_attention is 0 or 1 (the cls takes part, vit.py:180-186) and 1 otherwise (vit.py:202-208).  (frame, slot) is position slot - s0
      of sequence b * T + frame of every query row b.
  joint_space_time: one sequence of 1 + N * T tokens per query row, in the reference's token order (vision_tf.py:137): the cls at 0,
      addressed as (0, 0) only, and (frame t, patch n) at 1 + n * T + t.  The key axis of a joint map has the same order.  The engine keeps
      its compacted sequences frame-major ((t, n) at 1 + t * N + n; attention without a mask does not care), so the kernel is launched with
      that position and the map's columns are gathered into the reference's order afterwards (joint_source_rows)."""
from ._lib import TcowError

DEFAULT_MAX_BYTES = 4 << 30


def cls_takes_part(causal):
    """The cls slot is part of the spatial sequences iff causal_attention is 0 or 1."""
    return causal in (0, 1)


def joint_position(frame, slot, T):
    """Reference token index of (frame, slot) in a joint sequence: 0 for the cls, else 1 + (slot - 1) * T + frame."""
    return 0 if slot == 0 else 1 + (slot - 1) * T + frame


def joint_engine_position(frame, slot, N):
    """Position of (frame, slot) in the engine's compacted joint sequence: 0 for the cls, else 1 + frame * N + (slot - 1)."""
    return 0 if slot == 0 else 1 + frame * N + (slot - 1)


def joint_source_rows(T, N):
    """Reference-order gather of one clip's compacted joint sequence as the engine keeps it (the cls, then frame-major patches: frame t, patch n
    at 1 + t * N + n): entry p is the engine position of reference token p."""
    src = [0] * (1 + N * T)
    for n in range(N):
        for t in range(T):
            src[1 + n * T + t] = 1 + t * N + n
    return src


def normalise_blocks(blocks, depth):
    """None = all; ints, negative ones counted from the top, in the order given; a block named twice is refused."""
    if blocks is None:
        return tuple(range(depth))
    if isinstance(blocks, int):
        blocks = [blocks]
    out = []
    for b in blocks:
        if isinstance(b, bool) or not isinstance(b, int):
            raise TcowError(f'attention_maps: blocks must be integers, got {b!r}')
        if not -depth <= b < depth:
            raise TcowError(f'attention_maps: block {b} is out of range for a network of depth {depth}')
        i = b % depth
        if i in out:
            raise TcowError(f'attention_maps: block {i} is named twice in blocks={list(blocks)!r}')
        out.append(i)
    return tuple(out)


def normalise_queries(spatial_queries, T, S, causal, joint):
    """None -> []; 'cls' -> the cls queries that matter for this causal_attention; a list of (frame, slot) -> itself, checked."""
    if spatial_queries is None:
        return []
    if isinstance(spatial_queries, str):
        if spatial_queries != 'cls':
            raise TcowError(f"attention_maps: spatial_queries={spatial_queries!r} must be None, 'cls' or a list of (frame, slot)")
        if joint:
            return [(0, 0)]
        if not cls_takes_part(causal):
            raise TcowError(f"attention_maps: spatial_queries='cls' but slot 0 takes no part in spatial attention with causal_attention={causal}")
        # causal_attention == 1 keeps frame 0's cls row only (vit.py:193-198); 0 averages the T rows, so each of them matters
        return [(0, 0)] if causal == 1 else [(t, 0) for t in range(T)]
    out = []
    for q in spatial_queries:
        try:
            frame, slot = q
            frame, slot = int(frame), int(slot)
        except (TypeError, ValueError):
            raise TcowError(f'attention_maps: a spatial query must be (frame, slot), got {q!r}') from None
        if not 0 <= frame < T:
            raise TcowError(f'attention_maps: query {(frame, slot)}: frame {frame} is out of range 0 .. {T - 1}')
        if not 0 <= slot < S:
            raise TcowError(f'attention_maps: query {(frame, slot)}: slot {slot} is out of range 0 .. {S - 1}')
        if slot == 0 and joint and frame != 0:
            raise TcowError(f'attention_maps: query {(frame, slot)}: a joint sequence has one cls token, addressed as (0, 0)')
        if slot == 0 and not joint and not cls_takes_part(causal):
            raise TcowError(f'attention_maps: query {(frame, slot)}: slot 0 takes no part in spatial attention with causal_attention={causal}')
        out.append((frame, slot))
    return out


class MapPlan:
    """What one attention_maps call computes.  blocks, temporal, queries: the normalised arguments.  joint, s0.
    positions: the table the rows form is launched with -- divided: the DISTINCT positions slot - s0 of the queries (the kernel serves every
        sequence with every entry, so a position is computed once for all frames), joint: the engine position of each query.
    token_positions: joint only, the reference token index of each query (joint_position); columns: joint only, joint_source_rows -- column p
        of a map is launch column columns[p].
    gather: divided only, per query (frame, index into positions): map row (b, i) is launch row (b * T + frame, index).
    temporal_shape (B, N, heads, T, T) or None; spatial_shape (B, nq, heads, keys) or None; launch_shape of the rows form's own output.
    bytes: everything the call allocates for maps -- per block the temporal map, the spatial map and the launch output it is gathered from."""

    def __init__(self, depth, B, T, S, heads, causal, joint, blocks=None, temporal=True, spatial_queries=None, max_bytes=DEFAULT_MAX_BYTES):
        self.joint, self.s0 = bool(joint), 0 if (joint or cls_takes_part(causal)) else 1
        self.blocks = normalise_blocks(blocks, depth)
        self.temporal = bool(temporal)
        if self.temporal and joint:
            raise TcowError("attention_maps: temporal=True with attention_type='joint_space_time': a joint block has no temporal attention "
                            '(pass temporal=False)')
        self.queries = normalise_queries(spatial_queries, T, S, causal, joint)
        N, nq = S - 1, len(self.queries)
        self.keys = 1 + N * T if joint else S
        self.gather = self.token_positions = self.columns = None
        if joint:
            self.positions = [joint_engine_position(f, s, N) for f, s in self.queries]
            self.token_positions = [joint_position(f, s, T) for f, s in self.queries]
            self.columns = joint_source_rows(T, N)
        else:
            self.positions = sorted({s - self.s0 for _, s in self.queries})
            self.gather = [(f, self.positions.index(s - self.s0)) for f, s in self.queries]
        self.temporal_shape = (B, N, heads, T, T) if self.temporal else None
        self.spatial_shape = (B, nq, heads, self.keys) if nq else None
        self.launch_shape = None if not nq else (B, nq, heads, self.keys) if joint else (B * T, len(self.positions), heads, S)
        per_block = 0
        for shape in (self.temporal_shape, self.spatial_shape, self.launch_shape):
            if shape is not None:
                n = 4
                for d in shape:
                    n *= d
                per_block += n
        self.bytes_per_block, self.bytes = per_block, per_block * len(self.blocks)
        if isinstance(max_bytes, bool) or not isinstance(max_bytes, int) or max_bytes < 0:
            raise TcowError(f'attention_maps: max_bytes ({max_bytes!r}) must be a non-negative integer')
        if self.bytes > max_bytes:
            raise TcowError(f'attention_maps: the maps asked for take {self.bytes} bytes ({len(self.blocks)} block(s) x {per_block}), over '
                            f'max_bytes = {max_bytes}: name fewer blocks or queries, or raise the budget')


# ---------------------------------------------------------------------------------------------------------------------------- live sessions

def normalise_slots(spatial_slots, S, causal, who='step_maps'):
    """The spatial queries of a step: every frame of a step asks the same slots, so a query is a slot.  None -> []; 'cls' -> [0], where slot 0
    takes part in spatial attention (a stream has causal_attention 1 or 2: with 1 only); a list of slots in 0 .. S-1, slot 0 under the same
    rule, a slot named twice refused."""
    if spatial_slots is None:
        return []
    if isinstance(spatial_slots, str):
        if spatial_slots != 'cls':
            raise TcowError(f"{who}: spatial_slots={spatial_slots!r} must be None, 'cls' or a list of slots")
        if not cls_takes_part(causal):
            raise TcowError(f"{who}: spatial_slots='cls' but slot 0 takes no part in spatial attention with causal_attention={causal}")
        return [0]
    if isinstance(spatial_slots, int) and not isinstance(spatial_slots, bool):
        spatial_slots = [spatial_slots]
    out = []
    for s in spatial_slots:
        if isinstance(s, bool) or not isinstance(s, int):
            raise TcowError(f'{who}: a spatial slot must be an integer, got {s!r}')
        if not 0 <= s < S:
            raise TcowError(f'{who}: slot {s} is out of range 0 .. {S - 1}')
        if s == 0 and not cls_takes_part(causal):
            raise TcowError(f'{who}: slot 0 takes no part in spatial attention with causal_attention={causal}')
        if s in out:
            raise TcowError(f'{who}: slot {s} is named twice in spatial_slots={list(spatial_slots)!r}')
        out.append(s)
    return out


class StepMapPlan:
    """What one step_maps / step_ragged_maps call of a live stream or pool computes, beside the step.  rows_or_chunks: a tuple (rows, c) -- a
    stream or pool step of `rows` query rows with c frames each -- or a list of chunk lengths, one per session of a ragged step.
    blocks, temporal, slots: the normalised arguments; s0 and positions (slot - s0, the table of ops.attn_probs' rows form) as in MapPlan.
    F: flat frames of the step; first: every session's first flat frame (rows form: r * c); chunks: its frames.
    temporal_launch (F, S-1, heads, T_total): tcow_attn_temporal_step_probs' output; temporal_shape: the public layout -- (rows, N, heads, c, T),
        ragged a list of (1, N, heads, c_k, T) -- or None.
    spatial_launch (F, nq, heads, S): the rows form's output, of which the public maps are views -- (rows, c, nq, heads, S), ragged a list of
        (1, c_k, nq, heads, S) -- or None.
    bytes: everything the call allocates for maps: per block the temporal launch output and its permuted copy, and the spatial launch output."""

    def __init__(self, depth, rows_or_chunks, T_total, S, heads, causal, blocks=None, temporal=True, spatial_slots=None, max_bytes=DEFAULT_MAX_BYTES,
                 who='step_maps'):
        self.ragged = not isinstance(rows_or_chunks, tuple)
        if self.ragged:
            self.chunks = [int(c) for c in rows_or_chunks]
        else:
            rows, c = rows_or_chunks
            self.chunks = [int(c)] * int(rows)
        if not self.chunks or min(self.chunks) < 1:
            raise TcowError(f'{who}: a step has at least one row and every row at least one frame, got {rows_or_chunks!r}')
        self.first = [sum(self.chunks[:k]) for k in range(len(self.chunks))]
        self.F = F = sum(self.chunks)
        self.blocks = normalise_blocks(blocks, depth)
        self.temporal = bool(temporal)
        self.slots = normalise_slots(spatial_slots, S, causal, who)
        self.s0 = 0 if cls_takes_part(causal) else 1
        self.positions = [s - self.s0 for s in self.slots]
        N, nq, n = S - 1, len(self.slots), len(self.chunks)
        self.temporal_launch = (F, N, heads, T_total) if self.temporal else None
        self.spatial_launch = (F, nq, heads, S) if nq else None
        if self.ragged:
            self.temporal_shape = [(1, N, heads, c, T_total) for c in self.chunks] if self.temporal else None
            self.spatial_shape = [(1, c, nq, heads, S) for c in self.chunks] if nq else None
        else:
            self.temporal_shape = (n, N, heads, self.chunks[0], T_total) if self.temporal else None
            self.spatial_shape = (n, self.chunks[0], nq, heads, S) if nq else None
        per_block = (2 * 4 * F * N * heads * T_total if self.temporal else 0) + (4 * F * nq * heads * S if nq else 0)
        self.bytes_per_block, self.bytes = per_block, per_block * len(self.blocks)
        if isinstance(max_bytes, bool) or not isinstance(max_bytes, int) or max_bytes < 0:
            raise TcowError(f'{who}: max_bytes ({max_bytes!r}) must be a non-negative integer')
        if self.bytes > max_bytes:
            raise TcowError(f'{who}: the maps asked for take {self.bytes} bytes ({len(self.blocks)} block(s) x {per_block}), over '
                            f'max_bytes = {max_bytes}: name fewer blocks or slots, or raise the budget')

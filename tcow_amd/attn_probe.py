"""The probe that engine.run_forward(..., probe=) calls for the blocks of an attention_maps call: it launches ops.attn_probs on the block's qkv
tensor, on the forward's stream, into tensors of its own.  It keeps no activation alive: what it holds after a call are the maps.  StepMapProbe is
the probe of a step_maps call of a live stream or pool: its temporal maps come from the step object (c.stream.probs_temporal, against the K cache)."""
import torch

from . import ops


class AttentionMaps:
    """What Seeker.attention_maps returns beside the model's outputs.
    temporal: {block: (B, N, heads, T, T) f32} -- [b, n, h, tq, tk] = how much frame tq of patch n looks at frame tk (masked entries +0.0);
    spatial:  {block: (B, nq, heads, S) f32}, joint type (B, nq, heads, 1 + N*T) -- [b, i, h, :] = the softmax row of queries[i] over the slots of
              its frame (column 0 the cls, +0.0 where it takes no part; column 1 + n patch n), joint: over the clip's tokens in the reference's
              order (cls, then 1 + n*T + t);
    queries:  the normalised list of (frame, slot).  B counts query rows (clips x queries per clip)."""

    def __init__(self, queries):
        self.temporal, self.spatial, self.queries = {}, {}, list(queries)


class MapProbe:
    def __init__(self, plan, dev):
        self.plan, self.maps = plan, AttentionMaps(plan.queries)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        self.pos = i32(plan.positions) if plan.positions else None
        self.columns = torch.tensor(plan.columns, dtype=torch.long, device=dev) if plan.columns is not None else None
        if plan.gather is not None and plan.queries:
            self.frames = torch.tensor([f for f, _ in plan.gather], dtype=torch.long, device=dev)
            self.index = torch.tensor([k for _, k in plan.gather], dtype=torch.long, device=dev)

    def wants(self, i):
        return i in self.plan.blocks

    def temporal(self, i, c, QKV):
        if not (self.plan.temporal and self.wants(i)):
            return
        out = torch.empty(self.plan.temporal_shape, dtype=torch.float32, device=c.dev)
        ops.attn_probs(c.shape_attn, False, QKV, out)
        self.maps.temporal[i] = out

    def spatial(self, i, c, QKV):
        if self.pos is None or not self.wants(i):
            return
        plan = self.plan
        out = torch.empty(plan.launch_shape, dtype=torch.float32, device=c.dev)
        if plan.joint:
            ops.attn_probs(c.shape_joint, True, QKV, out, pos=self.pos)           # (QKV: the compacted sequences, frame-major)
            self.maps.spatial[i] = out.index_select(3, self.columns)              # key axis into the reference's token order
        else:
            ops.attn_probs(c.shape_attn, True, QKV, out, pos=self.pos)
            B, T = c.g['B'], c.g['T']
            full = out.view(B, T, len(plan.positions), out.shape[2], out.shape[3])
            self.maps.spatial[i] = full[:, self.frames, self.index].contiguous()


class StepAttentionMaps:
    """What step_maps / step_ragged_maps of a live stream or pool return beside the step's outputs.
    temporal: {block: (rows, N, heads, c, T) f32} -- [r, n, h, j, k] = how much frame t0 + j of patch n of row r looks at frame k of its session,
              keys < t0 as the K cache holds them (a compact cache: at their rounded values, which is what the model attends to); entries
              k > t0 + j are +0.0.  The steps' maps concatenated along dim 3 are the clip's (rows, N, heads, T, T) causal map.
    spatial:  {block: (rows, c, nq, heads, S) f32} -- the softmax row of slot slots[i] of every frame of the step over the slots of that frame.
    A ragged step: lists with an entry per session, (1, N, heads, c_k, T) and (1, c_k, nq, heads, S).
    slots: the normalised slot list; t0: the step's first frame (a pool: a list, one per session, in the order of the ids)."""

    def __init__(self, slots, t0):
        self.temporal, self.spatial, self.slots, self.t0 = {}, {}, list(slots), t0


class StepMapProbe:
    """The probe of a stream step (engine.run_forward calls it as it calls MapProbe; c.stream is the step): the temporal maps come from the
    step object's probs_temporal, right before its attn_temporal appends the step's keys, the spatial ones from ops.attn_probs on the step's
    own spatial qkv (a step's spatial sequences are per frame, as in a clip).  It keeps no activation alive."""

    def __init__(self, plan, dev, t0):
        self.plan, self.maps = plan, StepAttentionMaps(plan.slots, t0)
        self.pos = torch.tensor(plan.positions, dtype=torch.int32, device=dev) if plan.positions else None

    def wants(self, i):
        return i in self.plan.blocks

    def _per_session(self, launch, public):
        """launch [F, ...] -> the public layout: `public` maps a session's frames [c, ...] to its tensor; rows form: all rows at once."""
        plan = self.plan
        if plan.ragged:
            return [public(launch[f0:f0 + c].unsqueeze(0)) for f0, c in zip(plan.first, plan.chunks)]
        return public(launch.view(len(plan.chunks), plan.chunks[0], *launch.shape[1:]))

    def temporal(self, i, c, QKV):
        if not (self.plan.temporal and self.wants(i)):
            return
        g = c.g
        out = torch.empty(self.plan.temporal_launch, dtype=torch.float32, device=c.dev)
        c.stream.probs_temporal(i, c.amode, g['B'], g['T'], g['S'], g['D'], g['heads'], c.ca, QKV, out)
        self.maps.temporal[i] = self._per_session(out, lambda x: x.permute(0, 2, 3, 1, 4).contiguous())      # (rows, c, N, heads, T) -> (rows, N, heads, c, T)

    def spatial(self, i, c, QKV):
        if self.pos is None or not self.wants(i):
            return
        out = torch.empty(self.plan.spatial_launch, dtype=torch.float32, device=c.dev)
        ops.attn_probs(c.shape_attn, True, QKV, out, pos=self.pos)
        self.maps.spatial[i] = self._per_session(out, lambda x: x)

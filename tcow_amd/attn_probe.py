"""The probe that engine.run_forward(..., probe=) calls for the blocks of an attention_maps call: it launches ops.attn_probs on the block's qkv
tensor, on the forward's stream, into tensors of its own.  It keeps no activation alive: what it holds after a call are the maps."""
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

"""Drop-in `Seeker` / `QueryMaskTracker` for the TCOW hot path, running on libtcow_hip (gfx950).

Mirrors the nn.Module surface of the reference (model/seeker.py:17-25, model/mask_tracker.py:24-142):
same constructor keywords, `forward(input_frames, query_mask) -> (output_mask, output_flags)`, and the same
251 state-dict keys / shapes (seeker.tracker_backbone.timesformer.model.*, seeker.tracker_post_linear.*,
seeker.flag_post_linear.*), so checkpoints (`net_seeker`, train.py:281 / eval/inference.py:52) load with
strict=True.  The stock nn.Linear / nn.Conv2d / nn.LayerNorm objects below are parameter containers only:
their forward is never called; all arithmetic runs in the HIP kernels through one autograd.Function whose
backward is hand-written (no autograd graph inside the model).

precision:
  'bf16' (default)  bf16 GEMM/attention operands, f32 accumulation, f32 residual stream / LayerNorm / softmax.
  'fp16'            the bf16 mode's kernels built for IEEE binary16 storage (libtcow_hip_fp16.so: 11 instead of 8 significand bits,
                    same speed): mask logits within 1e-3 of the fp32 reference (measured ~6e-4 at BASELINE configs[1]); the backward
                    runs on gradients scaled by a power of two (exact; `loss_scale`, chosen per backward on the device) to stay inside binary16's range.
  'fp32'            everything f32 on the exact-f32 MFMA/FMA kernels: the parity mode (mask logits within 1e-3
                    of the fp32 reference; measured ~1e-6).
  'bf16x3'          the fp32 mode with its GEMMs on the bf16 matrix cores: every f32 operand is split into two bf16
                    terms in registers and a product is three MFMAs (hi*hi + hi*lo + lo*hi, csrc/gemm_x3.hip) --
                    ~1e-5 relative per product; mask logits within ~1e-5 of the reference at twice the fp32 mode's rate.
"""
import math
from functools import partial

import torch
import torch.nn as nn

from . import ops
from ._lib import TcowError
from .operands import OperandCache

TIMESFORMER_MEAN = 0.45
TIMESFORMER_STD = 0.225


# ----------------------------------------------------------------------------------------------- containers

def _trunc_normal_(t, std=.02):
    with torch.no_grad():
        return nn.init.trunc_normal_(t, mean=0., std=std, a=-2., b=2.)   # vit_utils.py:25-76 defaults a=-2,b=2


class _Attention(nn.Module):                     # vit.py:64-76
    def __init__(self, dim):
        super().__init__()
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.proj = nn.Linear(dim, dim)


class _Mlp(nn.Module):                           # vit.py:45-53
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _Block(nn.Module):                         # vit.py:126-153
    def __init__(self, dim, mlp_ratio, divided=True):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attention(dim)
        if divided:                              # temporal parameters exist only for divided_space_time (vit.py:140-146)
            self.temporal_norm1 = nn.LayerNorm(dim, eps=1e-6)
            self.temporal_attn = _Attention(dim)
            self.temporal_fc = nn.Linear(dim, dim)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))


class _PatchEmbed(nn.Module):                    # vit.py:220-233
    def __init__(self, patch, in_chans, dim):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, dim, kernel_size=patch, stride=patch)


class _VisionTransformer(nn.Module):             # vit.py:244-306
    def __init__(self, img_size, patch, in_chans, dim, depth, mlp_ratio, num_frames, divided=True):
        super().__init__()
        self.embed_dim = dim
        self.patch_embed = _PatchEmbed(patch, in_chans, dim)
        n_patches = (img_size[0] // patch) * (img_size[1] // patch)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, n_patches + 1, dim))
        self.time_embed = nn.Parameter(torch.zeros(1, num_frames, dim))      # stays zero at init (vit.py:268)
        self.blocks = nn.ModuleList([_Block(dim, mlp_ratio, divided) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        _trunc_normal_(self.pos_embed)
        _trunc_normal_(self.cls_token)
        for m in self.modules():                                             # vit.py:299-306
            if isinstance(m, nn.Linear):
                _trunc_normal_(m.weight)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)
        # vit.py:289-297: the loop counts the ModuleList itself as "Block 0", so every real block is zeroed.
        for blk in self.blocks if divided else []:
            nn.init.constant_(blk.temporal_fc.weight, 0)
            nn.init.constant_(blk.temporal_fc.bias, 0)


class _TimeSformer(nn.Module):                   # vit.py:416-459
    def __init__(self, **kw):
        super().__init__()
        self.model = _VisionTransformer(**kw)


class _Backbone(nn.Module):                      # vision_tf.py:27-66
    def __init__(self, **kw):
        super().__init__()
        self.timesformer = _TimeSformer(**kw)
        self.output_feature_dim = self.timesformer.model.embed_dim


_DEPTH_GEOMETRY = {12: (768, 12), 18: (896, 14), 24: (1024, 16)}      # vit.py:424-449


class ParamLayout:
    """THE order of QueryMaskTracker.param_list(), by name: the list is built from it and the engine indexes the list through it.

        cls, pos, time, patch_w, patch_b | depth x block | norm_w, norm_b, head_w, head_b [, flags_w, flags_b]

    A block is (weight, bias) of each of `subs` in order; ix[name] is the weight's offset inside the block (bias: + 1), at(i, name) its index
    in the whole list, block(i) the block's slice, blocks(lo, hi) the indices of blocks lo .. hi-1, embed those in front of the blocks."""
    cls, pos, time, patch_w, patch_b = embed = range(5)
    # sub-module of a _Block behind each name; a joint_space_time block has no temporal half (vit.py:135-153)
    MODULES = dict(tn=lambda b: b.temporal_norm1, tqkv=lambda b: b.temporal_attn.qkv, tproj=lambda b: b.temporal_attn.proj, tfc=lambda b: b.temporal_fc,
                   n1=lambda b: b.norm1, qkv=lambda b: b.attn.qkv, proj=lambda b: b.attn.proj, n2=lambda b: b.norm2, fc1=lambda b: b.mlp.fc1,
                   fc2=lambda b: b.mlp.fc2)

    def __init__(self, divided, depth, flags):
        self.subs = (('tn', 'tqkv', 'tproj', 'tfc') if divided else ()) + ('n1', 'qkv', 'proj', 'n2', 'fc1', 'fc2')
        self.ix = {name: 2 * k for k, name in enumerate(self.subs)}
        self.per_block, self.depth = 2 * len(self.subs), depth
        end = 5 + depth * self.per_block
        self.norm_w, self.norm_b, self.head_w, self.head_b, self.flags_w, self.flags_b = range(end, end + 6)
        self.count = end + (6 if flags else 4)

    def at(self, i, name, bias=0):
        return 5 + i * self.per_block + self.ix[name] + bias

    def blocks(self, lo, hi):
        return range(5 + lo * self.per_block, 5 + hi * self.per_block)

    def block(self, i):
        return slice(5 + i * self.per_block, 5 + (i + 1) * self.per_block)


# ----------------------------------------------------------------------------------------------- the module

class QueryMaskTracker(nn.Module):
    """mask_tracker.py:24-142.  Extra keywords (not in the reference): `embed_dim`, `num_heads` to build
    geometries other than depth 12/18/24 (the reference raises for those, vit.py:449), `precision`."""

    def __init__(self, logger, num_total_frames=24, num_visible_frames=16, frame_height=224, frame_width=288,
                 tracker_pretrained=False, attention_type='divided_space_time', patch_size=16, causal_attention=False,
                 norm_embeddings=False, drop_path_rate=0.1, network_depth=12, track_map_stride=4,
                 track_map_resize='bilinear', query_channels=1, output_channels=3, flag_channels=3,
                 embed_dim=None, num_heads=None, precision='bf16'):
        super().__init__()
        self.logger = logger
        self.num_total_frames = num_total_frames
        self.num_visible_frames = num_visible_frames
        self.frame_height = frame_height
        self.frame_width = frame_width
        self.attention_type = attention_type
        self.patch_size = patch_size
        self.causal_attention = int(causal_attention)
        self.norm_embeddings = bool(norm_embeddings)
        self.drop_path_rate = drop_path_rate
        self.network_depth = network_depth
        self.track_map_stride = track_map_stride
        self.track_map_resize = track_map_resize
        self.query_channels = query_channels
        self.output_channels = output_channels
        self.flag_channels = flag_channels
        self.input_channels = 3 + query_channels
        self._operands = OperandCache()   # every derived copy of the parameters and the persistent gradient buckets (tcow_amd/operands.py)
        self.set_precision(precision)

        from .checkpoint import parse_tracker_pretrained
        self.tracker_pretrained, self.pretrained_path = parse_tracker_pretrained(tracker_pretrained)   # mask_tracker.py:55-67
        if logger is not None:
            logger.info(f'(QueryMaskTracker) tracker_pretrained: {self.tracker_pretrained} '
                        f'pretrained_path: {self.pretrained_path}')

        assert attention_type in ['divided_space_time', 'space_only', 'joint_space_time']      # vit.py:133
        if attention_type == 'space_only':
            # the reference cannot run this setting either: DenseTimeSformer.forward reads model.time_embed (vision_tf.py:127-132), which a
            # space_only VisionTransformer does not create (vit.py:263-265) -> AttributeError on the first forward
            raise TcowError("attention_type='space_only' is not runnable through Seeker (vision_tf.py:127 needs time_embed, vit.py:263-265)")
        if query_channels != 1:
            raise TcowError('query_channels must be 1 (mask_tracker.py:105)')
        if embed_dim is None or num_heads is None:
            if network_depth not in _DEPTH_GEOMETRY:
                raise ValueError(f'Invalid network depth {network_depth}, must be one of 12, 18, 24.')  # vit.py:449
            embed_dim, num_heads = _DEPTH_GEOMETRY[network_depth]
        if embed_dim != num_heads * 64:
            raise TcowError(f'head_dim must be 64 (embed_dim={embed_dim}, num_heads={num_heads})')
        self.embed_dim, self.num_heads = embed_dim, num_heads
        assert frame_height % patch_size == 0                             # mask_tracker.py:89-90
        assert frame_width % patch_size == 0
        if track_map_stride > 1 and patch_size % track_map_stride != 0:
            raise TcowError('track_map_stride must divide patch_size')
        if track_map_resize not in ('bilinear', 'nearest'):
            raise TcowError(f'unsupported track_map_resize {track_map_resize}')

        self.tracker_backbone = _Backbone(img_size=(frame_height, frame_width), patch=patch_size,
                                          in_chans=self.input_channels, dim=embed_dim, depth=network_depth,
                                          mlp_ratio=4, num_frames=num_total_frames, divided=(attention_type == 'divided_space_time'))
        self.layout = ParamLayout(attention_type == 'divided_space_time', network_depth, flag_channels > 0)
        self.use_feature_dim = embed_dim
        self.tracker_post_linear = nn.Linear(embed_dim, output_channels * patch_size * patch_size)
        if flag_channels > 0:
            self.flag_post_linear = nn.Linear(embed_dim, flag_channels)
        if self.tracker_pretrained:
            from .checkpoint import load_pretrained_vit
            load_pretrained_vit(self, self.pretrained_path, logger)
        # dynamic loss scale of precision='fp16' (engine.run_backward): log2 of the target magnitude of the largest gradient seed element.  A
        # NON-persistent buffer: it follows .to() / DataParallel replication like any buffer, stays out of the 251-key state dict, and
        # save_tcow_checkpoint / resume_tcow_checkpoint carry it beside the optimizer state.
        self.register_buffer('ls_log2', torch.full((), -2.0, dtype=torch.float32), persistent=False)
        # persistent_grads=True: the backward writes parameter gradients into flat per-bucket buffers that live across steps and
        # hands them to p.grad directly (same pointers every step: no autograd copies, the fused optimizer's pointer table stays
        # valid).  Gradients are then OVERWRITTEN, not accumulated, by each backward -- use only with one backward per step.
        self.persistent_grads = False
        self.forced_drop_masks = None     # tests can inject explicit DropPath keep masks
        self.grad_hook = None             # optional callable(bucket_name, tensors) fired during backward (DDP)
        # ---- loss-scale / optimizer hand-off (engine.run_backward <-> optim.FusedAdamWClip)
        self._optim_ref = None            # weakref to the attached FusedAdamWClip(module=net): set by its constructor, cleared by its detach(); dead once it is collected
        self.pending_inv_scale = None     # device scalar 1 / loss scale while param.grad is loss-scaled: written by every backward, cleared by unscale_(); valid until the next backward
        self._defer_unscale = True        # tests switch the deferral off to compare the two paths; never written by the product
        self._warned_ls = False           # run_backward has warned once that nothing lowers the dynamic fp16 loss scale

    # ---- configuration helpers
    def set_precision(self, precision):
        if precision not in ('bf16', 'fp16', 'fp32', 'bf16x3'):
            raise ValueError("precision must be 'bf16', 'fp16', 'fp32' or 'bf16x3'")
        self.precision = precision
        self.mode = ops.BF16 if precision == 'bf16' else ops.FP16 if precision == 'fp16' else ops.F32
        if 'ls_log2' in self._buffers:
            with torch.no_grad():
                self.ls_log2.fill_(-2.0)
        self.loss_scale = 'dynamic'                                             # fp16 only: power-of-two factor on the backward's gradients (engine.run_backward); a number = static
        self.gemm_mode = ops.F32X3 if precision == 'bf16x3' else self.mode     # GEMM arithmetic; storage / every other kernel follow `mode`
        self._operands.drop(buckets=False)
        return self

    def invalidate_weight_cache(self):
        """Call after updating parameters through raw pointers (tcow_amd.optim.FusedAdamWClip does): in-place torch ops bump the
        parameters' autograd version counters, which the operand cache checks on its own."""
        self._operands.invalidate(self.mode)

    def _live_optim(self):
        """The FusedAdamWClip attached to this module (FusedAdamWClip(..., module=net)), or None when there is none or it has been garbage-collected."""
        return self._optim_ref() if self._optim_ref is not None else None

    def _apply(self, fn, *a, **kw):
        # .to() / .cuda() / .half() swap the parameters' .data (neither id() nor ._version changes): every cache that holds device
        # pointers or copies of the old storage must go, and so must the cached parameter list
        self._operands.drop()
        self.invalidate_param_cache()
        return super()._apply(fn, *a, **kw)

    @property
    def vit(self):
        return self.tracker_backbone.timesformer.model

    def geometry(self, B, T=None):
        """T: frames per row block (default num_total_frames; a stream step passes its chunk length)."""
        P = self.patch_size
        Hp, Wp = self.frame_height // P, self.frame_width // P
        N = Hp * Wp
        T = self.num_total_frames if T is None else T
        return dict(B=B, T=T, Hp=Hp, Wp=Wp, N=N, S=N + 1, D=self.embed_dim, heads=self.num_heads, P=P, M=B * T * (N + 1))

    def stream(self, batch_size=1, queries_per_clip=1, graph=False, skinny_gemm=None, cache_dtype=None):
        """Streaming inference (causal_attention 1 or 2, eval, CUDA): a SeekerStream of at most num_total_frames frames for `batch_size` clips with
        `queries_per_clip` query masks each; stream.step(rgb, query_mask) takes the next frames and returns their outputs (tcow_amd/stream.py).
        skinny_gemm: the steps' GEMMs of a few hundred rows run on 64 x 64 tiles with a split over K -- the 16-bit modes where ops.skinny_plan
        routes them, 'bf16x3' where ops.skinny_plan_x3 does; exact 'fp32' has no such kernel.  None = the measured default of the precision,
        stream.SKINNY_GEMM_DEFAULT (16-bit) / stream.SKINNY_GEMM_X3_DEFAULT (bf16x3).
        cache_dtype: the element type of the temporal K / V cache, apart from the precision (stream.cache_plan): None = the storage type;
        'bf16' halves the cache of 'fp32' / 'bf16x3'; 'fp8' (OCP e4m3fn) in any precision, a quarter of an f32 cache.  Keys and values are then
        used at their rounded values: the outputs differ from the None stream's by that rounding and still do not depend on the chunking."""
        from .stream import SeekerStream
        return SeekerStream(self, batch_size, queries_per_clip, graph, skinny_gemm, cache_dtype)

    def stream_pool(self, capacity, skinny_gemm=None, page_frames=None, pages=None, cache_dtype=None, rollover=None, requery_threshold=0.0):
        """Streaming inference for up to `capacity` live sessions that started at different moments: a SeekerStreamPool whose step(ids, rgb,
        query_mask) advances any subset of the open sessions, each at its own frame, in one Seeker step (tcow_amd/stream.py).
        page_frames=P (a power of two): a paged pool -- the K / V caches are `pages` pages of P frames (default capacity * ceil(T / P), which cannot
        run out; lower it to the memory budget), a session holds only the pages its frames so far have filled and close() / reset() return them;
        a step that would need more pages than are free raises TcowError and moves nothing.  Same outputs, bit for bit.  None: one full cache per slot.
        cache_dtype: as in stream(); a pool gives the bits of a stream with the same cache_dtype.
        rollover=k (1 .. num_total_frames // 2): a SeekerRolloverPool, whose sessions have no last frame.  A session is a chain of windows of
        num_total_frames frames that overlap by k; each later window is queried with the model's own output at its first frame, thresholded on
        the device (mask logits > requery_threshold), and its first k frames only warm it up.  The outputs are forward() of every such window.
        A session takes two cache slots and at most num_total_frames - k frames per call; frames_done() counts on, window(), requery_mask() and
        requery_pixels() show the chain.  None: sessions end at frame num_total_frames - 1, as above."""
        from .stream import SeekerRolloverPool, SeekerStreamPool
        if rollover is not None:
            return SeekerRolloverPool(self, capacity, skinny_gemm, page_frames, pages, cache_dtype, rollover, requery_threshold)
        return SeekerStreamPool(self, capacity, skinny_gemm, page_frames, pages, cache_dtype)

    def param_list(self):
        """Fixed order of the parameters the autograd.Function sees.  Cached: walking ~250 module attributes costs 0.4 ms per call.  .to() /
        load_state_dict keep the Parameter objects; code that ASSIGNS a new Parameter inside the module tree must call invalidate_param_cache()
        (the first and last entries are re-checked on every call, which catches wholesale replacement)."""
        cached = self.__dict__.get('_param_list_cache')
        if cached is not None and cached[0] is self.vit.cls_token and cached[-1] is (self.flag_post_linear if self.flag_channels > 0 else self.tracker_post_linear).bias:
            return cached
        ps = self._param_list_uncached()
        self.__dict__['_param_list_cache'] = ps
        return ps

    def invalidate_param_cache(self):
        self.__dict__.pop('_param_list_cache', None)

    def _param_list_uncached(self):
        v, lay = self.vit, self.layout                 # (the order is ParamLayout's: its docstring states it)
        ps = [v.cls_token, v.pos_embed, v.time_embed, v.patch_embed.proj.weight, v.patch_embed.proj.bias]
        for b in v.blocks:
            for name in lay.subs:
                sub = lay.MODULES[name](b)
                ps += [sub.weight, sub.bias]
        ps += [v.norm.weight, v.norm.bias, self.tracker_post_linear.weight, self.tracker_post_linear.bias]
        if self.flag_channels > 0:
            ps += [self.flag_post_linear.weight, self.flag_post_linear.bias]
        assert len(ps) == lay.count
        return ps

    # ---- forward
    def forward(self, input_frames, query_mask):
        """mask_tracker.py:92-142: (B,3,T,Hf,Wf), (B,1,T,Hf,Wf) -> (B,C,T,Hf,Wf) logits, (B,T,F) flags.
        Extension: query_mask may carry Qs masks per clip, (B*Qs,1,T,Hf,Wf) with clip b's queries at rows b*Qs..b*Qs+Qs-1;
        the outputs then have B*Qs rows and equal Qs separate calls with the same frames (pipeline.py:134-158), but the rgb part of the
        patch embedding is computed once per clip."""
        (B, _, T, Hf, Wf) = input_frames.shape
        assert query_mask.shape[1] == 1                                   # mask_tracker.py:105
        assert query_mask.shape[0] % B == 0 and query_mask.shape[2:] == input_frames.shape[2:]
        assert T == self.num_total_frames                                 # vision_tf.py:96
        assert Hf == self.frame_height and Wf == self.frame_width         # vision_tf.py:97 (W' check)
        assert self.attention_type == 'divided_space_time' or self.causal_attention == 0   # vit.py:160
        if not input_frames.is_cuda:
            raise TcowError('Seeker (tcow_amd) runs on the GPU only: move inputs and module to cuda')
        if query_mask.device != input_frames.device or self.vit.pos_embed.device != input_frames.device:
            raise TcowError(f'Seeker (tcow_amd): inputs ({input_frames.device}, {query_mask.device}) and parameters ({self.vit.pos_embed.device}) must share one device')
        if getattr(self, '_is_replica', False):
            # torch.nn.DataParallel (train.py:222-223) re-creates shallow replicas every forward: their dicts alias the original's, so give
            # each replica private operand / gradient caches for this call instead of growing the shared ones with dead entries
            self._operands = self._operands.fresh()
        rgb = input_frames.to(torch.float32).contiguous()                 # mask_tracker.py:103-104 (inputs not mutated)
        qm = query_mask.to(torch.float32).contiguous()
        from .engine import SeekerFunction
        with torch.cuda.device(input_frames.device):                      # kernels launch on the tensors' device and its current stream
            out_mask, out_flags = SeekerFunction.apply(self, rgb, qm, *self.param_list())
        if self.flag_channels <= 0:
            out_flags = None
        return (out_mask, out_flags)

    def attention_maps(self, input_frames, query_mask, blocks=None, temporal=True, spatial_queries=None, max_bytes=None):
        """forward() that also returns attention weights: (output_mask, output_flags, maps), the two outputs with the bits of forward() on the
        same inputs, maps an attn_probe.AttentionMaps:
          maps.temporal[i] (B, N, heads, T, T): block i, which earlier frames a patch pulls from (temporal=True; divided_space_time only);
          maps.spatial[i]  (B, nq, heads, S):   block i, which slots the tokens of spatial_queries look at -- None: no spatial maps, 'cls', or a
                                                list of (frame, slot), slot 0 = cls, 1 + n = patch n; joint_space_time: (B, nq, heads, 1 + N*T)
                                                over the clip's tokens in the reference's order (cls, 1 + n*T + t);
          maps.queries: the normalised (frame, slot) list.  B counts query rows (clips x queries per clip).
        blocks: None = all, or block indices (negative from the top).  max_bytes: budget of the maps (default 4 GiB); what is asked for is
        computed and refused, in bytes, before anything runs (tcow_amd/attn_maps.py has every rule).
        The maps are the f32 softmax of the q and k the model computed and stored (include/tcow_hip.h, tcow_attn_probs), not a replay of the
        flash kernels' own score rounding.  Eval mode only (DropPath draws would make a map a sample), no forced_drop_masks, under
        torch.no_grad().  This is the clip path; a live stream or pool session serves the maps of a step against its cache through
        SeekerStream.step_maps / SeekerStreamPool.step_maps / step_ragged_maps."""
        from .attn_maps import DEFAULT_MAX_BYTES, MapPlan
        from .attn_probe import MapProbe
        from .engine import run_forward
        if self.training:
            raise TcowError('attention_maps: the module is in training mode: DropPath draws would make a map a sample (call .eval())')
        if self.forced_drop_masks is not None:
            raise TcowError('attention_maps: forced_drop_masks is set: the maps are defined for the eval forward only')
        if not input_frames.is_cuda or not query_mask.is_cuda or not self.vit.pos_embed.is_cuda:
            raise TcowError('attention_maps: Seeker (tcow_amd) runs on the GPU only: move inputs and module to cuda')
        if query_mask.device != input_frames.device or self.vit.pos_embed.device != input_frames.device:
            raise TcowError(f'attention_maps: inputs ({input_frames.device}, {query_mask.device}) and parameters ({self.vit.pos_embed.device}) must share one device')
        (B, _, T, Hf, Wf) = input_frames.shape
        assert query_mask.shape[1] == 1 and query_mask.shape[0] % B == 0 and query_mask.shape[2:] == input_frames.shape[2:]
        assert T == self.num_total_frames and Hf == self.frame_height and Wf == self.frame_width
        assert self.attention_type == 'divided_space_time' or self.causal_attention == 0
        g = self.geometry(query_mask.shape[0])
        plan = MapPlan(self.network_depth, g['B'], g['T'], g['S'], g['heads'], self.causal_attention, self.attention_type != 'divided_space_time',
                       blocks, temporal, spatial_queries, DEFAULT_MAX_BYTES if max_bytes is None else max_bytes)
        rgb = input_frames.to(torch.float32).contiguous()
        qm = query_mask.to(torch.float32).contiguous()
        with torch.no_grad(), torch.cuda.device(input_frames.device):
            probe = MapProbe(plan, input_frames.device)
            out_mask, out_flags, _ = run_forward(self, rgb, qm, self.param_list(), save=False, probe=probe)
        return (out_mask, out_flags if self.flag_channels > 0 else None, probe.maps)


class Seeker(nn.Module):
    """model/seeker.py:17-25."""

    shares_rgb = True          # forward accepts (B, ...) frames with (B * Qs, ...) query masks (see QueryMaskTracker.forward)

    def __init__(self, logger, **kwargs):
        super().__init__()
        self.logger = logger
        self.seeker_args = {k: v for k, v in kwargs.items() if k != 'precision'}     # what train.py:186-205 stores as checkpoint['seeker_args']
        self.seeker = QueryMaskTracker(logger, **kwargs)

    def forward(self, *args):
        return self.seeker(*args)

    def attention_maps(self, input_frames, query_mask, blocks=None, temporal=True, spatial_queries=None, max_bytes=None):
        """See QueryMaskTracker.attention_maps."""
        return self.seeker.attention_maps(input_frames, query_mask, blocks, temporal, spatial_queries, max_bytes)

    def stream(self, batch_size=1, queries_per_clip=1, graph=False, skinny_gemm=None, cache_dtype=None):
        """See QueryMaskTracker.stream."""
        return self.seeker.stream(batch_size, queries_per_clip, graph, skinny_gemm, cache_dtype)

    def stream_pool(self, capacity, skinny_gemm=None, page_frames=None, pages=None, cache_dtype=None, rollover=None, requery_threshold=0.0):
        """See QueryMaskTracker.stream_pool."""
        return self.seeker.stream_pool(capacity, skinny_gemm, page_frames, pages, cache_dtype, rollover, requery_threshold)

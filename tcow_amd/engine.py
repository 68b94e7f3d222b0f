"""Forward / backward schedule of the Seeker hot path on libtcow_hip, as one autograd.Function.

Layout: residual stream R [M, D] f32 with M = B*T*S rows, row(b,t,s) = (b*T+t)*S + s, slot 0 = cls replica
(see include/tcow_hip.h).  Per block (vit.py:155-217), with the reference lines each launch replaces:

    U   = LN_t(R0)                                  temporal_norm1            vit.py:172
    QKV = U Wqkv_t^T + b                            temporal_attn.qkv         vit.py:81
    O   = attn_temporal(QKV)          causal mask   vit.py:88-109
    Pj  = dp_t * (O Wproj_t^T + b)                  temporal_attn.proj + DropPath   vit.py:111,172
    R1  = R0 + [s>=1] * (Pj Wfc^T + b)              temporal_fc + residual    vit.py:174-176
    V   = LN_1(R1);  QKV = V Wqkv^T + b;  O = attn_spatial(QKV)               vit.py:184-186 / 206-208
    R2  = R1 + dp_s * (O Wproj^T + b);  cls merge                             vit.py:189-215
    H   = GELU(LN_2(R2) W1^T + b1);  R3 = R2 + dp_m * (H W2^T + b2)           vit.py:216, 55-61

The backward below is the hand-derived adjoint of exactly this schedule; nothing goes through torch autograd.

16-bit modes FOLD the temporal projection: temporal_attn.proj -> DropPath -> temporal_fc (vit.py:111,172-176) are two Linear layers
with only a per-row scale dp_t between them, so

    R1 = R0 + [s>=1] * (dp_t * (O W'^T + b') + b_fc),      W' = Wfc Wproj,  b' = Wfc b_proj

is ONE [M,768] x [768,768] GEMM instead of two (forward, input gradient and weight gradient: 36 of them per step at depth 12).  The
state dict keeps both Linear layers: W', b' are recomputed from the f32 masters after every optimizer step (one batched launch of small
f32 products, ops.sgemm_batched), and the backward turns dW' = dY'^T O, db' into dWfc = dW' Wproj^T, dWproj = Wfc^T dW',
db_proj = Wfc^T db' the same way; b_fc's gradient is the row-masked column sum of dR1, taken in f32 inside the LayerNorm backward
that produces dR1.  (The f32 parity modes keep the reference's op order.)

How the file reads.  run_forward and run_backward are drivers.  Both build a _Ctx (the step's modes, geometry, attention shapes, allocation
and operand look-ups) and address the parameters through module.layout (seeker.ParamLayout), never by position.  The forward walks
_patch_embed, _embed, one _block_forward_* per block and _heads_forward; the backward walks _heads_backward (which chooses the binary16 loss
scale, _loss_scale), one _block_backward_* per block, _embed_backward and -- when the frames or the query mask require grad -- _input_backward.  Where a parameter gradient lands, when its weight-gradient GEMM is
launched and when its bucket goes to the data-parallel hook is all in _GradBuckets, whose docstring states the ordering rules, rule 5 what
requires_grad_(False) takes out of the backward (lowest_block: where the chain stops; tests/test_frozen_host.py);
tests/test_ddp_gloo.py and tests/test_engine_host.py check them, and the launch schedule call for call, on the CPU.
"""
import os
import warnings

import torch

from . import ops
from .ops import ACT_GELU, ACT_GELU_DSAVE, ACT_MUL_AUX
from .operands import fold_on

f32 = torch.float32


def _joint_rows(module, g, dev):
    """Row indices [B * (1 + T*N)] of the joint-attention sequences inside the [B*T*S] token matrix: per clip its cls row (frame 0's
    slot 0) followed by every patch row.  The reference's sequence is (cls, patches in n-major order) (vision_tf.py:137); attention
    without a mask is invariant to the order of its keys / queries, so the frame-major order of our layout is used as is."""
    def build():
        B, T, S = g['B'], g['T'], g['S']
        r = torch.arange(B * T * S, device=dev).reshape(B, T * S)
        keep = torch.ones(T * S, dtype=torch.bool, device=dev)
        keep[torch.arange(1, T, device=dev) * S] = False                      # cls replicas of frames 1..T-1 take no part
        return r[:, keep].reshape(-1).contiguous()
    return module._operands.constant(('jrows', g['B'], str(dev)), build)


def group_sizes(depth, spec=None):
    """Blocks per gradient group, TOP group first (the order the backward finishes them): TCOW_DDP_GROUP = one number (every group that
    size, the bottom one takes the remainder) or a comma list 'a,b,c' (top group a blocks, the next b, ...; the last entry repeats until the
    blocks are used up, the bottom group is cut to what is left).  Default '5,5,2' at depth 12: the bottom group's gradients only exist
    when the backward is over, so its all-reduce cannot overlap anything -- it is kept small (2 blocks + embeddings = 76 MB instead of the
    190 MB of an even 4/4/4 split), and the weight-gradient launches of the 5-block groups fill three whole rounds of the chip with ONE
    token slice (765 tiles of 256 x 256 on 256 CUs).  Other depths default to groups of four."""
    if spec is None:
        spec = os.environ.get('TCOW_DDP_GROUP') or ('5,5,2' if depth == 12 else '4')
    want = [max(1, int(x)) for x in str(spec).split(',') if x.strip()] or [4]
    sizes, left, k = [], depth, 0
    while left > 0:
        gs = min(want[min(k, len(want) - 1)], left)
        sizes.append(gs); left -= gs; k += 1
    return sizes


def _mask0(module, g, dev, stream_step):
    """mask0 [M]: 0 on slot 0, 1 elsewhere.
    stream_step: B * T takes many values from one stream step to the next, and mask0 of fewer frames is a prefix of mask0 of more frames (the
    same S entries per frame, whatever B and T), so one vector -- the longest asked for so far -- serves them all instead of one cache entry
    per distinct (B, T)."""
    B, T, S = g['B'], g['T'], g['S']
    def build(frames):
        m = torch.ones(frames, S, dtype=f32, device=dev)
        m[:, 0] = 0
        return m.reshape(-1).contiguous()
    if stream_step:
        return module._operands.longest(('mask0_frames', S, str(dev)), B * T * S, lambda n: build(-(-n // S)))
    return module._operands.constant(('mask0', B, T, str(dev)), lambda: build(B * T))


def _dp_draw(module, i, name, rate, shape, train, dev):
    """keep / (1 - rate) of block i's DropPath `name` (vit_utils.py:150-152: keep = floor(rand + 1 - r), x / (1 - r) * keep), one entry per
    element of `shape`; None when that DropPath does nothing.  forced_drop_masks replaces the draw for the keys it holds and switches the rest off."""
    forced = module.forced_drop_masks
    if forced is not None:
        if (i, name) not in forced:
            return None
        keep, rate = forced[(i, name)]
        return keep.to(dev, f32).reshape(shape) / (1.0 - rate)
    if not (train and rate > 0.):
        return None
    keep = (torch.rand(shape, device=dev) + (1.0 - rate)).floor_()
    return keep / (1.0 - rate)


def _dp_joint(module, g, rates, train, dev):
    """joint_space_time block (vit.py:161-162): both DropPath calls see x of shape (B, 1+N*T, D) -> one draw per sample each."""
    B, T, S = g['B'], g['T'], g['S']
    scales = []
    for i, r in enumerate(rates):
        ent = {'t': None, 's': None, 'm': None}
        for kind, name in (('s', 'spatial'), ('m', 'mlp')):
            k = _dp_draw(module, i, name, r, B, train, dev)
            if k is not None:
                ent[kind] = k[:, None].expand(B, T * S).reshape(-1).contiguous()
        scales.append(ent)
    return scales


def _dp_batched(module, g, rates, mask0, dev):
    """All DropPath draws of a divided_space_time training step in one batch: one rand and three broadcasts (one launch on the device,
    ops.droppath_rows) instead of ~15 tiny launches per block."""
    B, T, S, N, depth = g['B'], g['T'], g['S'], g['N'], len(rates)
    keep_p = module._operands.constant(('keep_p', tuple(rates), str(dev)), lambda: (1.0 - torch.tensor(rates, dtype=f32)).to(dev))
    u = torch.rand(depth, B * N + B * T + B, device=dev)
    if u.is_cuda and N == S - 1:
        rt, rsp, rml, rt0 = ops.droppath_rows(u, keep_p, mask0, B, T, S)
    else:
        kp = keep_p[:, None]
        sc = (u + kp).floor_() / kp
        kt = sc[:, :B * N].reshape(depth, B, 1, N); ks = sc[:, B * N:B * N + B * T].reshape(depth, B, T, 1); km = sc[:, B * N + B * T:].reshape(depth, B, 1)
        rt = torch.ones(depth, B, T, S, dtype=f32, device=dev)
        rt[:, :, :, 1:] = kt
        rt = rt.reshape(depth, -1)
        rsp = ks.expand(depth, B, T, S).reshape(depth, -1)
        rml = km.expand(depth, B, T * S).reshape(depth, -1)
        rt0 = rt * mask0[None, :]               # mask0 * dp_t: row scale of the folded temporal projection
    live = [r > 0. for r in rates]
    return [{'t': rt[i] if live[i] else None, 's': rsp[i] if live[i] else None, 'm': rml[i] if live[i] else None, 't0': rt0[i] if live[i] else mask0}
            for i in range(depth)]


def _dp_per_block(module, g, rates, train, mask0, dev):
    """divided_space_time, draw by draw: forced masks, eval, or a rate of zero.  Temporal: one draw per (clip, patch), spatial: per (clip,
    frame), MLP: per clip (the shapes DropPath sees at vit.py:172, 189, 216)."""
    B, T, S, N = g['B'], g['T'], g['S'], g['N']
    scales = []
    for i, r in enumerate(rates):
        ent = {'t': None, 's': None, 'm': None}
        if module.forced_drop_masks is not None or (train and r > 0.):       # (an eval step, a stream step among them, draws nothing)
            kt = _dp_draw(module, i, 'temporal', r, (B, N), train, dev)
            if kt is not None:
                rs = torch.ones(B, T, S, dtype=f32, device=dev)
                rs[:, :, 1:] = kt[:, None, :]
                ent['t'] = rs.reshape(-1).contiguous()
            ks = _dp_draw(module, i, 'spatial', r, (B, T), train, dev)
            if ks is not None:
                ent['s'] = ks[:, :, None].expand(B, T, S).reshape(-1).contiguous()
            km = _dp_draw(module, i, 'mlp', r, (B,), train, dev)
            if km is not None:
                ent['m'] = km[:, None].expand(B, T * S).reshape(-1).contiguous()
        ent['t0'] = mask0 if ent['t'] is None else ent['t'] * mask0
        scales.append(ent)
    return scales


def _row_vectors(module, g, train, stream_step=False):
    """mask0 [M] (0 on slot 0) and the DropPath row scales of every block: per block a dict of [M] vectors 't', 's', 'm' (None where that
    DropPath does nothing) and, for a divided block, 't0' = 't' * mask0."""
    dev = module.vit.pos_embed.device
    mask0 = _mask0(module, g, dev, stream_step)
    depth = module.network_depth
    rates = torch.linspace(0, module.drop_path_rate, depth).tolist() if depth > 1 else [0.0]   # vit.py:272
    if module.attention_type != 'divided_space_time':
        return mask0, _dp_joint(module, g, rates, train, dev)
    if module.forced_drop_masks is None and train and max(rates) > 0.:
        return mask0, _dp_batched(module, g, rates, mask0, dev)
    return mask0, _dp_per_block(module, g, rates, train, mask0, dev)


def _effective_embeddings(module, g):
    """pos [S,D] / time [T,D] as used by the forward, with the nearest-neighbour resize of vision_tf.py:103-115,
    127-132 when the stored tables do not match the clip; returns index maps for the backward."""
    v = module.vit
    pos = v.pos_embed.detach()[0]
    S, T = g['S'], g['T']
    pos_idx = None
    if pos.shape[0] != S:
        n_old = pos.shape[0] - 1
        Pold = int(n_old ** 0.5)
        Hn = S // g['Wp']                       # vision_tf.py:108: H = x.size(1) // W
        ys = (torch.arange(Hn, device=pos.device).float() * (Pold / Hn)).floor().long().clamp_(max=Pold - 1)
        xs = (torch.arange(g['Wp'], device=pos.device).float() * (Pold / g['Wp'])).floor().long().clamp_(max=Pold - 1)
        grid = (ys[:, None] * Pold + xs[None, :]).reshape(-1) + 1
        pos_idx = torch.cat([torch.zeros(1, dtype=torch.long, device=pos.device), grid])
        pos = pos[pos_idx].contiguous()
    te = v.time_embed.detach()[0]
    time_idx = None
    if te.shape[0] != T:
        time_idx = (torch.arange(T, device=te.device).float() * (te.shape[0] / T)).floor().long().clamp_(max=te.shape[0] - 1)
        te = te[time_idx].contiguous()
    return pos.contiguous(), te.contiguous(), pos_idx, time_idx


class _Ctx:
    """What one step's forward and backward both need and build the same way: the module, its modes (mode: storage and every kernel but the
    GEMMs; gmode: the GEMM entry points' arithmetic -- `mode`, or F32X3 for precision='bf16x3'; amode: the attention's, on split-bf16 MFMAs too
    in bf16x3, csrc/attention_x3.hip), the geometry g, the attention shapes, the parameter layout, and `save`: whether activations are kept
    for a backward (the forward of a training step, and the backward itself)."""

    def __init__(self, module, g, dev, save, stream=None, probe=None):
        self.module, self.g, self.dev, self.save, self.stream = module, g, dev, save, stream
        self.probe = probe                  # attention_maps only (attn_probe.MapProbe); None: nothing is called
        self.mode, self.gmode = module.mode, module.gemm_mode
        self.amode = self.gmode if self.gmode == ops.F32X3 else self.mode
        self.dt = ops.tdtype(self.mode)
        self.lay, self.opnd = module.layout, module._operands
        self.joint, self.fold = module.attention_type != 'divided_space_time', fold_on(module)
        self.ca = module.causal_attention
        self.use_cls = self.ca in (0, 1)
        self.sk = {} if stream is None else {'skinny': stream.skinny}        # GEMM routing of a stream step (ops.gemm_nt); the clip path never passes the keyword
        B, T, S, D, heads = g['B'], g['T'], g['S'], g['D'], g['heads']
        self.shape_attn = ops.attn_shape(self.amode, B, T, S, D, heads, self.ca)
        if self.joint:
            self.jrows = _joint_rows(module, g, dev)
            self.Lj = 1 + T * (S - 1)
            self.shape_joint = ops.attn_shape(self.amode, B, 1, self.Lj, D, heads, 0)     # one sequence of 1 + N*T tokens per clip, cls included, no mask (vit.py:159-161)

    def E(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=self.dt if dtype is None else dtype, device=self.dev)

    def W(self, p):
        """Operand copy [N,K] of a GEMM weight (the forward's)."""
        return self.opnd.weight(self.mode, p, self.save)[0]

    def Wt(self, p):
        """Transposed operand copy [K,N] (the input-gradient GEMMs')."""
        return self.opnd.weight(self.mode, p, True)[1]

    def ln_fwd(self, x, w, b):
        """LayerNorm of x [M,D] in the step's mode -> (out, mean, rstd); the statistics only when activations are saved."""
        M = x.shape[0]
        out = self.E(M, x.shape[1]); mean = self.E(M, dtype=f32) if self.save else None; rstd = self.E(M, dtype=f32) if self.save else None
        ops.layernorm_fwd(self.mode, x, w, b, out, mean, rstd)
        return out, mean, rstd


# ---------------------------------------------------------------------------------------------------------------------------------- forward

def _patch_embed(c, rgb, qm, params, sv):
    """Patch embedding (vit.py:233-241) -> X [M,D] f32; the im2col operand(s) are kept for the weight gradient (sv None: nobody wants them)."""
    module, g, lay = c.module, c.g, c.lay
    T, S, D, M, P = g['T'], g['S'], g['D'], g['M'], g['P']
    Kpe = module.input_channels * P * P
    bias = params[lay.patch_b].detach()
    X = c.E(M, D, dtype=f32)
    B, Bc = qm.shape[0], rgb.shape[0]        # query rows, clips; B = Bc * Qs
    if B == Bc:
        A_pe = c.E(M, Kpe)
        ops.im2col(c.mode, rgb, qm, P, module.tracker_pretrained, A_pe)
        ops.gemm_nt(c.gmode, A_pe, c.W(params[lay.patch_w]), X, bias=bias, **c.sk)
        if sv is not None:
            sv['A_pe'] = A_pe
        return X
    # shared rgb: the Qs queries of a clip see the same frames (pipeline.py:134-158), only the mask channel differs:
    # conv(cat[rgb, mask]) = W[:, :3] * rgb + W[:, 3] * mask -> one K = 3 P^2 GEMM per clip + one K = P^2 GEMM per query, the
    # latter taking the clip's rgb part as its residual operand
    Krgb, Qs, TS = 3 * P * P, B // Bc, T * S
    Wc = c.W(params[lay.patch_w])                                    # [D, 4 P^2], channel-major columns (vit.py:233)
    A_rgb = c.E(Bc * TS, Krgb); A_m = c.E(M, Kpe - Krgb)
    ops.im2col_channels(c.mode, rgb, P, module.tracker_pretrained, A_rgb)
    ops.im2col_channels(c.mode, qm, P, False, A_m)
    Xrgb = c.E(Bc * TS, D, dtype=f32)
    ops.gemm_nt(c.gmode, A_rgb, Wc[:, :Krgb], Xrgb, bias=bias, **c.sk)
    for bq in range(B):
        b = bq // Qs
        ops.gemm_nt(c.gmode, A_m[bq * TS:(bq + 1) * TS], Wc[:, Krgb:], X[bq * TS:(bq + 1) * TS], resid=Xrgb[b * TS:(b + 1) * TS], **c.sk)
    if sv is not None:
        sv['A_pe'] = (A_rgb, A_m)
    return X


def _embed(c, X, params, sv):
    """cls token, position and time embeddings onto X in place (vision_tf.py:99-138)."""
    g = c.g
    cls = params[c.lay.cls].detach().reshape(-1)
    if c.stream is None:
        pos, te, pos_idx, time_idx = _effective_embeddings(c.module, g)
        ops.embed_fwd(X, g['B'], g['T'], g['S'], cls, pos, te)
        if sv is not None:
            sv.update(pos_idx=pos_idx, time_idx=time_idx)
    else:
        # every row has its own frames: the table [B*T, D] holds the time row of (b, j) at b*T + j, which tcow_embed_fwd indexes by (row / S) % (B*T)
        ops.embed_fwd(X, 1, g['B'] * g['T'], g['S'], cls, c.stream.pos, c.stream.time_rows)


def _mlp_forward(c, q, R2, dp, st):
    """R3 = R2 + dp_m * (GELU(LN_2(R2) W1^T + b1) W2^T + b2)   (vit.py:216, 55-61)"""
    ix, E, W, gmode, save = c.lay.ix, c.E, c.W, c.gmode, c.save       # (locals: this runs per block of a launch-bound stream step)
    M, D = R2.shape
    Wn, mu2, rs2 = c.ln_fwd(R2, q[ix['n2']].detach(), q[ix['n2'] + 1].detach())
    Hd = q[ix['fc1']].shape[0]
    pre = E(M, Hd) if save else None
    H = E(M, Hd)
    # training saves GELU'(pre-activation) instead of the pre-activation: the backward is then one multiply per element
    ops.gemm_nt(gmode, Wn, W(q[ix['fc1']]), H, bias=q[ix['fc1'] + 1].detach(), act=ACT_GELU_DSAVE if save else ACT_GELU, aux=pre, **c.sk)
    R3 = E(M, D, dtype=f32) if save else R2
    ops.gemm_nt(gmode, H, W(q[ix['fc2']]), R3, bias=q[ix['fc2'] + 1].detach(), row_scale=dp['m'], resid=R2, **c.sk)
    if save:
        st.update(R2=R2, mu2=mu2, rs2=rs2, Wn=Wn, pre=pre, H=H)
    return R3


def _block_forward_joint(c, i, q, R0, dp, mask0, st):
    """joint_space_time block (vit.py:159-162): x = x + drop_path(attn(norm1(x))) over all 1 + N*T tokens of a clip, then the MLP."""
    g, ix = c.g, c.lay.ix
    B, D, M, heads = g['B'], g['D'], g['M'], g['heads']
    V, mu1, rs1 = c.ln_fwd(R0, q[ix['n1']].detach(), q[ix['n1'] + 1].detach())
    QKV2 = c.E(M, 3 * D)
    ops.gemm_nt(c.gmode, V, c.W(q[ix['qkv']]), QKV2, bias=q[ix['qkv'] + 1].detach(), **c.sk)
    QJ = QKV2.index_select(0, c.jrows)                                # compact (cls, patches) sequences: the kernels take contiguous ones
    if c.probe is not None:
        c.probe.spatial(i, c, QJ)
    OJ = c.E(B * c.Lj, D); lse_s = c.E(B * c.Lj, heads, dtype=f32) if c.save else None
    ops.attn_fwd(c.shape_joint, True, QJ, OJ, lse_s)
    O2 = torch.zeros(M, D, dtype=c.dt, device=c.dev)
    O2.index_copy_(0, c.jrows, OJ)                                    # (the unused cls replicas of frames 1.. get a zero attention output)
    R2 = c.E(M, D, dtype=f32) if c.save else R0
    ops.gemm_nt(c.gmode, O2, c.W(q[ix['proj']]), R2, bias=q[ix['proj'] + 1].detach(), row_scale=dp['s'], resid=R0, **c.sk)
    if c.save:
        st.update(R1=R0, mu1=mu1, rs1=rs1, V=V, QKV_s=QJ, O_s=O2, OJ=OJ, lse_s=lse_s, rs_s=dp['s'])
    return _mlp_forward(c, q, R2, dp, st)


def _block_forward_divided(c, i, q, R0, dp, mask0, st):
    """divided_space_time block (vit.py:163-217): temporal attention + temporal_fc, spatial attention + cls merge, MLP; the lines of the
    module docstring.  A stream step substitutes the temporal attention and, for causal_attention == 1, the cls row."""
    g, ix, sk, stream, E, W, gmode, save = c.g, c.lay.ix, c.sk, c.stream, c.E, c.W, c.gmode, c.save
    B, T, S, D, M, heads = g['B'], g['T'], g['S'], g['D'], g['M'], g['heads']
    P_ = lambda name, k=0: q[ix[name] + k].detach()                     # weight (k = 0) / bias (k = 1) of a sub-module of this block
    # temporal
    U, mu0, rs0 = c.ln_fwd(R0, P_('tn'), P_('tn', 1))
    QKV = E(M, 3 * D)
    ops.gemm_nt(gmode, U, W(q[ix['tqkv']]), QKV, bias=P_('tqkv', 1), **sk)
    if c.probe is not None:
        c.probe.temporal(i, c, QKV)
    O = E(M, D); lse_t = E(M, heads, dtype=f32) if save else None
    if stream is None:
        ops.attn_fwd(c.shape_attn, False, QKV, O, lse_t)
    else:
        stream.attn_temporal(i, c.amode, B, T, S, D, heads, c.ca, QKV, O)
    R1 = E(M, D, dtype=f32) if save else R0
    if c.fold:
        Wf, _, bprime = c.opnd.folded(c.mode, i, q, ix, save)
        ops.gemm_nt(gmode, O, Wf, R1, bias=bprime, row_scale=dp['t0'], resid=R0, bias2=P_('tfc', 1), row_scale2=mask0, **sk)
        Pj = None
    else:
        Pj = E(M, D)
        ops.gemm_nt(gmode, O, W(q[ix['tproj']]), Pj, bias=P_('tproj', 1), row_scale=dp['t'], **sk)
        ops.gemm_nt(gmode, Pj, W(q[ix['tfc']]), R1, bias=P_('tfc', 1), row_scale=mask0, resid=R0, **sk)
    if save:
        st.update(R0=R0, mu0=mu0, rs0=rs0, U=U, QKV_t=QKV, O_t=O, lse_t=lse_t, Pj=Pj)
    # spatial
    V, mu1, rs1 = c.ln_fwd(R1, P_('n1'), P_('n1', 1))
    QKV2 = E(M, 3 * D)
    ops.gemm_nt(gmode, V, W(q[ix['qkv']]), QKV2, bias=P_('qkv', 1), **sk)
    if c.probe is not None:
        c.probe.spatial(i, c, QKV2)
    O2 = E(M, D); lse_s = E(M, heads, dtype=f32) if save else None
    ops.attn_fwd(c.shape_attn, True, QKV2, O2, lse_s)
    rs_s = dp['s']
    if not c.use_cls:
        rs_s = mask0 if rs_s is None else rs_s * mask0
    R2 = E(M, D, dtype=f32) if save else R1
    ops.gemm_nt(gmode, O2, W(q[ix['proj']]), R2, bias=P_('proj', 1), row_scale=rs_s, resid=R1, **sk)
    if c.use_cls and stream is not None:
        stream.cls_row(i, R2, B, T, S)                                       # (a stream has causal_attention 1 or 2)
    elif c.use_cls:
        ops.cls_merge(R2, B, T, S, 1 if c.ca == 1 else 0)
    if save:
        st.update(R1=R1, mu1=mu1, rs1=rs1, V=V, QKV_s=QKV2, O_s=O2, lse_s=lse_s, rs_s=rs_s)
    return _mlp_forward(c, q, R2, dp, st)


def _heads_forward(c, X, params, sv):
    """Final norm (vision_tf.py:152-153), mask head (mask_tracker.py:113-132) and flags head (mask_tracker.py:135-137) -> (mask logits, flags)."""
    module, g, lay, mode = c.module, c.g, c.lay, c.mode
    B, T, S, D, M, P = g['B'], g['T'], g['S'], g['D'], g['M'], g['P']
    norm_w, norm_b = params[lay.norm_w].detach(), params[lay.norm_b].detach()
    feat32 = X
    if module.norm_embeddings:
        Fm, muf, rsf = c.ln_fwd(X, norm_w, norm_b)
        if module.flag_channels > 0 and mode != ops.F32:
            feat32 = c.E(M, D, dtype=f32)
            ops.layernorm_fwd(ops.F32, X, norm_w, norm_b, feat32)
        elif mode == ops.F32:
            feat32 = Fm
        if c.save:
            sv.update(muf=muf, rsf=rsf)
    elif mode == ops.F32:
        Fm = X
    else:
        Fm = c.E(M, D)
        ops.scale_cast(mode, X, None, Fm)
    Co = module.output_channels
    Pm = c.E(M, Co * P * P)
    ops.gemm_nt(c.gmode, Fm, c.W(params[lay.head_w]), Pm, bias=params[lay.head_b].detach(), **c.sk)
    stp = module.track_map_stride if module.track_map_stride > 1 else 1
    h, w = module.frame_height // stp, module.frame_width // stp
    pooled = c.E(B * T, Co, h, w, dtype=f32)
    ops.unpatchify_pool_fwd(mode, Pm, B * T, g['Hp'], g['Wp'], P, Co, stp, pooled)
    out_mask = c.E(B, Co, T, module.frame_height, module.frame_width, dtype=f32)
    bilinear = (module.track_map_resize == 'bilinear') and stp > 1
    ops.upsample_fwd(pooled, B, T, Co, h, w, stp, bilinear, out_mask)
    if module.flag_channels > 0:
        flags = c.E(B, T, module.flag_channels, dtype=f32)
        ops.flags_fwd(feat32, B * T, S, params[lay.flags_w].detach(), params[lay.flags_b].detach(), flags)
    else:
        flags = torch.zeros(0, device=c.dev)
    if c.save:
        sv.update(X_final=X, Fm=Fm, feat32=feat32, stp=stp, bilinear=bilinear, h=h, w=w)
    return out_mask, flags


def lowest_block(lay, frozen, want_inputs):
    """The stopping rule of a backward with frozen parameters: k, the lowest block that holds a wanted parameter -- 0 when an embedding parameter
    or an input gradient is wanted, lay.depth when nothing at or below the top block is.  The backward runs blocks depth-1 .. k and nothing below;
    the forward keeps no activations of the blocks below k."""
    if any(want_inputs) or any(j not in frozen for j in lay.embed):
        return 0
    for i in range(lay.depth):
        if any(j not in frozen for j in lay.blocks(i, i + 1)):
            return i
    return lay.depth


def run_forward(module, rgb, qm, params, save, stream=None, frozen=frozenset(), want_inputs=(False, False), probe=None):
    """-> (mask logits, flags, saved activations or None).
    frozen, want_inputs (training): the indices of the parameters whose gradient is NOT wanted and which input gradients (frames, query mask) are,
    as SeekerFunction.forward reads them; they hold for this forward's backward (sv['frozen'], sv['want_inputs'], sv['k'] = lowest_block()) and
    decide what is saved, never what is computed.
    stream (inference only): one stream step, built by tcow_amd/stream.py -- rgb / qm then hold the step's T = rgb.shape[2] frames
    per row, and the schedule differs in three places: the embeddings (stream.pos, and stream.time_rows [B*T, D], one row of the time table per
    (row, frame)), the temporal attention (stream.attn_temporal: against the block's K / V cache, which it extends) and, for
    causal_attention == 1, the cls row (stream.cls_row: frame 0's, kept per block).  A fifth thing is asked of the step: stream.skinny, whether its
    GEMMs may take the skinny-M entry point (ops.gemm_nt(..., skinny=)); the clip path never passes the keyword.
    probe (Seeker.attention_maps; None: nothing changes): every block calls probe.temporal(i, c, QKV) right after its temporal qkv GEMM and
    probe.spatial(i, c, QKV2 -- joint: the compacted QJ) right after its spatial one; the probe launches ops.attn_probs on the same stream into
    tensors of its own and decides which blocks it serves.  It reads the tensor during the call only: no activation is kept alive for it."""
    B = qm.shape[0]                          # query rows (== clips unless the rgb frames are shared between a clip's queries)
    g = module.geometry(B) if stream is None else module.geometry(B, T=rgb.shape[2])
    c = _Ctx(module, g, rgb.device, save, stream, probe)
    mask0, dps = _row_vectors(module, g, module.training, stream_step=stream is not None)
    sv = {'g': g, 'blocks': [], 'mask0': mask0, 'dps': dps} if save else None
    k = lowest_block(c.lay, frozen, want_inputs) if save else 0
    if save:
        sv.update(frozen=frozen, want_inputs=tuple(want_inputs), k=k)
    X = _patch_embed(c, rgb, qm, params, sv if save and (c.lay.patch_w not in frozen or any(want_inputs)) else None)
    _embed(c, X, params, sv)
    block_forward = _block_forward_joint if c.joint else _block_forward_divided
    below = _Ctx(module, g, rgb.device, False, stream, probe) if k > 0 else None      # the blocks under the lowest wanted parameter run as in inference
    for i in range(module.network_depth):
        keep = save and i >= k
        st = {} if keep else None
        X = block_forward(c if keep or not save else below, i, params[c.lay.block(i)], X, dps[i], mask0, st)
        if save:
            sv['blocks'].append(st)
    out_mask, flags = _heads_forward(c, X, params, sv)
    return out_mask, flags, sv


# --------------------------------------------------------------------------------------------------------------------------------- backward

def _loss_scale(module, ls_mode, mask_amax, d_flags, dev):
    """The binary16 loss scale of one backward -> (gscale, 1 / gscale), device scalars, or (None, None).  ls_mode: module.loss_scale in fp16,
    None in the other modes; mask_amax: max |d_mask| (device scalar or None)."""
    # binary16: gradients of a mean-reduced loss (~1e-9 per element at BASELINE configs[1]) sit far below fp16's normal range (6.1e-5), so the
    # whole backward runs on gradients multiplied by a power of two and every finished gradient bucket is multiplied back (exact) before anyone
    # sees it (_GradBuckets.publish) -- everything in between is linear in the seed.  'dynamic' (default): the scale is chosen on the device, per
    # backward and without a host sync, so that the largest seed element lands in [2^t / 2, 2^t) with t = module.ls_log2 (a device scalar, -2 to
    # start with).  Measured over 300 training steps (tools/dev_fp16_amp.py): the 16-bit gradient operands peak at 3 ... 12 000 times the seed
    # maximum (median 240), i.e. at <= 6 000 of binary16's 65 504, with their median near 1e-3 (normal range).  An overflow all the same shows up
    # as a non-finite gradient norm: FusedAdamWClip then skips the update and lowers t by 4 (optim.py).  A number instead of 'dynamic' = static.
    # Where it is applied (_heads_backward): the mask head's first two steps (bilinear x4 adjoint, un-patchify) are f32 and linear, so the scale
    # goes onto the POOLED gradient (5 MB) behind them, not onto d_mask (83 MB) -- bit-identical, a power of two commutes with the sums -- and
    # max |d_mask| comes out of the adjoint's own pass over d_mask (tcow_upsample_bwd_amax) instead of an abs + amax pair of passes.
    if ls_mode is None:
        return None, None
    if ls_mode == 'dynamic':
        amax = mask_amax if mask_amax is not None else torch.zeros((), dtype=f32, device=dev)
        if d_flags is not None and d_flags.numel():
            amax = torch.maximum(amax, d_flags.detach().abs().amax().to(f32))
        gs = torch.exp2(torch.floor(module.ls_log2 - torch.log2(amax.clamp_min(1e-37)))).clamp(2.0 ** -20, 2.0 ** 60)
    elif float(ls_mode) != 1.0:
        gs = torch.tensor(float(ls_mode), dtype=f32, device=dev)
    else:
        return None, None
    return gs, 1.0 / gs


class _GradBuckets:
    """Where the parameter gradients of one backward land, when their launches are issued and when they are handed out.  The ordering rules:

    1. A bucket is one flat f32 buffer; views of it are the parameters' gradients (`grads`), the flat buffer is what the data-parallel
       all-reduce moves.  Buckets are the groups of blocks of group_sizes(), the top group with the output heads, the bottom one with the
       embeddings; `flat` is the bucket of the group being differentiated (start_block opens the next at a group's top block).  With the
       folded projection there is one more, the LATE bucket: tproj.weight, tproj.bias and tfc.weight of every block.
    2. linear_bwd(defer=True) and queue_fold() only QUEUE a weight-gradient GEMM (`pending`), layernorm_bwd(defer=ln_jobs) only queues the
       fold of its dgamma / dbeta table.  end_block() issues both queues (flush) at a group's bottom block -- the bottom group's too --, or
       earlier when one more block would not fit into a grouped launch.  The queued operands stay alive until then.
    3. publish(tag, flat) hands a FINISHED bucket to module.grad_hook: no launch writes into it afterwards.  The order is 'g<bottom block>'
       of every group above the bottom one, straight behind its flush; 'fold', behind the four batched products of finish_late(); 'g0',
       behind the embedding gradients (run_backward); then the hook's finish(), and nothing after it.
    4. The loss scale (inv_gscale, set by _heads_backward) is undone by publish(), unless defer_unscale leaves it to the optimizer.
    5. Frozen parameters (`frozen`: the indices whose gradient is not wanted; k = lowest_block()).  A bucket holds views for wanted parameters
       only, grads[j] stays None for the others, and a bucket without a wanted parameter is neither allocated nor published.  The chain stops
       below block k, so block k is the bottom block of its group: its bucket goes out as 'g<k>' (k = depth, heads only: 'g<depth>'), and the
       groups wholly below k never appear.  linear_bwd queues a Linear's weight-gradient GEMM only when its weight is wanted (bias frozen: without a
       bias gradient) and a column sum (`colsums`, one tcow_colsum_grouped call per flush) when only its bias is; a LayerNorm with both
       parameters frozen computes neither (ln_targets), one with one of them wanted sends the other to scratch -- the kernel has no form for one.
       Scratch is c.E(...), never a bucket.  Nothing here looks at the frozen set to choose the loss scale or who undoes it."""

    def __init__(self, c, params, have_flags, frozen=frozenset(), k=0):
        module, lay = c.module, c.lay
        self.c, self.params, self.hook = c, params, module.grad_hook
        self.grads = [None] * len(params)
        self.want, self.k = [j not in frozen for j in range(len(params))], k
        self.colsums = []                                               # (dY, db): bias gradients of Linear layers whose weight is frozen
        self.inv_gscale = None
        # Who undoes the loss scale.  With a data-parallel hook every finished bucket is multiplied back before the hook sees it (ranks choose their
        # own scales).  Without one (or with one that says it is not `active`: a GradSync of one rank), and with a live FusedAdamWClip(module=net)
        # attached, the buckets stay scaled and the optimizer's clip-coefficient kernel folds the inverse scale into the update
        # (grad_inv_scale of tcow_adamw_clip_step): 488 MB less read and written per step.  param.grad then holds SCALED gradients (as under
        # torch.cuda.amp.GradScaler before unscale_); module.pending_inv_scale (device scalar, valid until the next backward) is the factor the
        # optimizer applies on the fly.  The deferral needs ONE backward per optimizer step -- several backwards into the same param.grad (the
        # reference's per-query model loop, gradient accumulation, DataParallel replicas) would make autograd add buckets that carry different
        # scales -- so it is tied to `persistent_grads` (whose contract is exactly that: each backward OVERWRITES the gradients), never taken by
        # a DataParallel replica, and only while the attached optimizer is still alive (a weak reference: a discarded or replaced FusedAdamWClip
        # must not leave param.grad scaled for torch.optim.AdamW or clip_grad_norm_).
        self.defer_unscale = ((self.hook is None or getattr(self.hook, 'active', True) is False) and module._live_optim() is not None
                              and bool(getattr(module, 'persistent_grads', False)) and not getattr(module, '_is_replica', False)
                              and module._defer_unscale)                 # (tests switch the deferral off to compare the two paths)
        self.pending, self.ln_jobs, self.fold_jobs = [], [], []         # weight-gradient GEMMs (dY, X, dW, db); LayerNorm folds; (block, dW' [D,D], db' [D])
        self.tn_group_max = ops.tn_group_max()
        # Groups of blocks (TCOW_DDP_GROUP, default 5 / 5 / 2 from the top at depth 12): 3 all-reduces of ~75-190 MB at depth 12 instead of 14 of
        # ~38 MB -- each collective is a window in which resident RCCL workgroups push the one-workgroup-per-CU GEMMs into an extra round
        # (profiles/r02_cu_contention.txt), so fewer, larger ones.  The WEIGHT-GRADIENT GEMMs of a group are issued together at its end as well
        # (one grouped launch over 28 problems = 612 tiles of 256 x 256 at ViT-B): so many tiles fill whole rounds of the chip with TWO token
        # slices instead of five, i.e. 60 % less f32 partial-sum traffic in the GEMM and in the fold (tcow_tn_group_slices); nothing in the
        # backward chain waits for a weight gradient, and the bucket is not published before the group's end anyway.
        self.group_lo = {}                                              # block index -> first block of its group
        hi = lay.depth
        for gs in group_sizes(lay.depth):
            for j in range(hi - gs, hi):
                self.group_lo[j] = max(hi - gs, k)
            hi -= gs
        # The folded projection's three gradients per block come out of small products that are worth batching over ALL blocks (a launch of three
        # 768^3 problems is pure latency: 35 us whether it carries 3 problems or 12): the late bucket (57 MB at ViT-B), finished once after block 0.
        self.late = set()
        if c.fold:
            for j in range(lay.depth):
                self.late.update((lay.at(j, 'tproj'), lay.at(j, 'tproj', 1), lay.at(j, 'tfc')))
        self.late_flat = self.bucket(sorted(self.late)) if self.late else None
        heads = ([lay.norm_w, lay.norm_b] if module.norm_embeddings else []) + [lay.head_w, lay.head_b] + ([lay.flags_w, lay.flags_b] if have_flags else [])
        self.flat = self.group_bucket(self.group_lo[lay.depth - 1], lay.depth, heads)

    def bucket(self, indices):
        """A flat buffer for those of the given parameters that are wanted, None when none is; persistent_grads: the same storage every step (see
        QueryMaskTracker.persistent_grads)."""
        params, dev = self.params, self.c.dev
        indices = [j for j in indices if self.want[j]]
        if not indices:
            return None
        total = sum(params[j].numel() for j in indices)
        alloc = lambda: torch.empty(total, dtype=f32, device=dev)
        flat = self.c.opnd.buffer(('gbuf', indices[0], total, str(dev)), alloc) if getattr(self.c.module, 'persistent_grads', False) else alloc()
        off = 0
        for j in indices:
            n = params[j].numel()
            self.grads[j] = flat[off:off + n].view(params[j].shape)
            off += n
        return flat

    def group_bucket(self, lo, hi, heads=()):
        """The bucket of blocks lo .. hi-1 without their late entries (+ the embeddings for the bottom group, + the given head entries)."""
        lay = self.c.lay
        return self.bucket((list(lay.embed) if lo == 0 else []) + [j for j in lay.blocks(lo, hi) if j not in self.late] + list(heads))

    def publish(self, tag, flat):
        if flat is None:                                                # (no wanted parameter in this bucket: it does not exist)
            return
        if self.inv_gscale is not None and not self.defer_unscale:
            flat.mul_(self.inv_gscale)
        if self.hook is not None:
            self.hook(tag, flat)

    def wants(self, *indices):
        return any(self.want[j] for j in indices)

    def linear_bwd(self, idx_w, dY, Xin, defer=False):
        """dW, db of the Linear at params[idx_w], [idx_w + 1] whose output-gradient operand is dY [M,N] and input operand Xin [M,K]; a frozen one
        is None and not computed: without the weight there is no GEMM, its bias gradient is a column sum of dY."""
        dW, db = self.grads[idx_w], self.grads[idx_w + 1]
        if dW is None:
            if db is not None and defer:
                self.colsums.append((dY, db))
            elif db is not None:
                ops.colsum_grouped(self.c.mode, [(dY, db)])
        elif defer:
            self.pending.append((dY, Xin, dW.reshape(dW.shape[0], -1), db))
        else:
            ops.gemm_tn(self.c.gmode, dY, Xin, dW.reshape(dW.shape[0], -1), bias_grad=db)

    def ln_targets(self, idx_w):
        """(dgamma, dbeta) to pass to the backward of the LayerNorm at params[idx_w], [idx_w + 1]: (None, None) when both are frozen (no partial table,
        no fold); with one of them wanted the other is scratch."""
        dg, db = self.grads[idx_w], self.grads[idx_w + 1]
        if dg is None and db is None:
            return None, None
        D = self.params[idx_w].numel()
        return dg if dg is not None else self.c.E(D, dtype=f32), db if db is not None else self.c.E(D, dtype=f32)

    def queue_fold(self, i, dY, O):
        """Block i's folded projection: dW' = dY'^T O, db' into persistent temporaries, turned into the three real gradients by finish_late();
        nothing when none of the three is wanted."""
        c, D, lay = self.c, self.c.g['D'], self.c.lay
        if not self.wants(lay.at(i, 'tproj'), lay.at(i, 'tproj', 1), lay.at(i, 'tfc')):
            return
        tW, tb = c.opnd.buffer(('foldtmp', i, str(c.dev)), lambda: (torch.empty(D, D, dtype=f32, device=c.dev), torch.empty(D, dtype=f32, device=c.dev)))
        self.pending.append((dY, O, tW, tb))
        self.fold_jobs.append((i, tW, tb))

    def flush(self):
        if self.pending:
            ops.gemm_tn_grouped(self.c.gmode, self.pending)
            self.pending.clear()
        if self.colsums:
            ops.colsum_grouped(self.c.mode, self.colsums)
            self.colsums.clear()
        if self.ln_jobs:
            ops.layernorm_fold(self.ln_jobs)

    def start_block(self, i):
        if i != self.c.lay.depth - 1 and self.group_lo[i] != self.group_lo[i + 1]:      # first (top) block of the next group: its bucket
            self.flat = self.group_bucket(self.group_lo[i], i + 1)

    def end_block(self, i, sv):
        if self.group_lo[i] == i or len(self.pending) + 8 > self.tn_group_max:
            self.flush()             # the group's weight-gradient GEMMs (six or seven per block; joint: four) as one grouped launch
        sv['blocks'][i] = None       # free this block's activations (the queued weight-gradient operands keep theirs)
        if i > 0 and self.group_lo[i] == i:                               # last (bottom) block of a group that is not the bottom group: done
            self.publish('g%d' % i, self.flat)

    def finish_late(self):
        """Z = P Wfc^T + b_fc with P = dp_t (O Wproj^T + b_proj) and dY' = dp_t dZ:  dWfc = dZ^T P = dW' Wproj^T + db' b_proj^T,
        dWproj = Wfc^T dW', db_proj = Wfc^T db' for all blocks: four batched launches (<= 24 problems each); then the late bucket goes out."""
        lay, params, grads = self.c.lay, self.params, self.grads
        nt_, r1_, tn_, gv_ = [], [], [], []
        for (i, tW, tb) in self.fold_jobs:
            fc, pw, pb = lay.at(i, 'tfc'), lay.at(i, 'tproj'), lay.at(i, 'tproj', 1)
            wfc, wp, bp = params[fc].detach(), params[pw].detach(), params[pb].detach()
            if grads[fc] is not None:
                nt_.append((tW, wp.t(), grads[fc]))
                r1_.append((tb.view(-1, 1), bp.view(1, -1), grads[fc]))
            if grads[pw] is not None:
                tn_.append((wfc.t(), tW, grads[pw]))
            if grads[pb] is not None:
                gv_.append((wfc.t(), tb.view(-1, 1), grads[pb].view(-1, 1)))
        for c0 in range(0, max(len(nt_), len(tn_), len(gv_)), 24):       # (wanted outputs only: a list may be shorter than the others, or empty)
            for lst, acc in ((nt_, False), (r1_, True), (tn_, False), (gv_, False)):
                if lst[c0:c0 + 24]:
                    ops.sgemm_batched(lst[c0:c0 + 24], accumulate=acc)
        self.fold_jobs.clear()
        if self.late_flat is not None:
            self.publish('fold', self.late_flat)


def _heads_backward(c, bk, sv, params, d_mask, d_flags, have_flags):
    """Mask head (mask_tracker.py:113-132), flags head and final norm, from the seeds to dX [M,D] f32; chooses the loss scale on the way.
    -> None when only head parameters are wanted: then nothing is launched behind the wanted head products."""
    module, g, lay, mode, dev = c.module, c.g, c.lay, c.mode, c.dev
    B, T, S, D, M, P = g['B'], g['T'], g['S'], g['D'], g['M'], g['P']
    Co = module.output_channels
    ls_mode = getattr(module, 'loss_scale', 'dynamic') if mode == ops.FP16 else None
    if ls_mode == 'dynamic' and module._live_optim() is None and not module._warned_ls:
        module._warned_ls = True
        warnings.warn("precision='fp16' with the dynamic loss scale but no FusedAdamWClip(..., module=net) attached: nothing lowers the scale "
                      "after an overflow or skips the poisoned step -- pass module= to the optimizer or set net.seeker.loss_scale to a number")
    if d_mask is None:
        d_mask = torch.zeros(B, Co, T, module.frame_height, module.frame_width, dtype=f32, device=dev)
    d_mask = d_mask.to(f32).contiguous()
    dpooled = c.E(B * T, Co, sv['h'], sv['w'], dtype=f32)
    mask_amax = None
    if ls_mode == 'dynamic' and sv['bilinear'] and sv['stp'] == 4 and sv['h'] > 4 and sv['w'] > 4:
        _, mask_amax = ops.upsample_bwd_amax(d_mask, B, T, Co, sv['h'], sv['w'], sv['stp'], dpooled)
    else:
        if ls_mode == 'dynamic' and d_mask.numel():
            mask_amax = d_mask.abs().amax()
        ops.upsample_bwd(d_mask, B, T, Co, sv['h'], sv['w'], sv['stp'], sv['bilinear'], dpooled)
    gscale, bk.inv_gscale = _loss_scale(module, ls_mode, mask_amax, d_flags, dev)
    if gscale is not None:
        dpooled.mul_(gscale)
        d_flags = None if d_flags is None else d_flags * gscale
    dPm = c.E(M, Co * P * P)
    ops.unpatchify_pool_bwd(mode, dpooled, B * T, g['Hp'], g['Wp'], P, Co, sv['stp'], dPm)
    bk.linear_bwd(lay.head_w, dPm, sv['Fm'])
    # heads only: no block runs (bk.k == depth) and the final norm, where it takes part, is frozen too -- nothing below the head products is wanted
    below = bk.k < lay.depth or (module.norm_embeddings and bk.wants(lay.norm_w, lay.norm_b))
    dFeat = None
    if below:
        # gradient w.r.t. the features that feed both heads, always f32: dFeat = dPm . Whead (+ flags adjoint)
        dFeat = c.E(M, D, dtype=f32)
        ops.gemm_nt(c.gmode, dPm, c.Wt(params[lay.head_w]), dFeat)
    if have_flags:
        # flags head adjoint (F x D, once per step; only the plugin path ever asks for it, pipeline.py:238)
        df = d_flags.to(f32).reshape(B * T, -1).contiguous()
        if bk.grads[lay.flags_w] is not None:
            meanf = sv['feat32'].reshape(B * T, S, D)[:, 1:, :].float().mean(dim=1)
            ops.sgemm_batched([(df.t(), meanf, bk.grads[lay.flags_w])])         # dWf = df^T mean(features)   (library kernel: no vendor BLAS on the path)
        if below:
            dmean = torch.empty(B * T, D, dtype=f32, device=dev)
            ops.sgemm_batched([(df, params[lay.flags_w].detach(), dmean)])
        if bk.grads[lay.flags_b] is not None:
            bk.grads[lay.flags_b].copy_(df.sum(0))
        if below:
            dFeat.reshape(B * T, S, D)[:, 1:, :] += (dmean / float(S - 1))[:, None, :]
    # (without a flags gradient flag_post_linear.* keep grad None, like the reference where pipeline.py:157 drops them)
    if not below or not module.norm_embeddings:
        return dFeat     # model.norm takes no part when norm_embeddings is False (vision_tf.py:152): its grads stay None
    dX = c.E(M, D, dtype=f32)
    dgamma, dbeta = bk.ln_targets(lay.norm_w)
    ops.layernorm_bwd(ops.F32, dFeat, sv['X_final'], sv['muf'], sv['rsf'], params[lay.norm_w].detach(), None, dX, dgamma, dbeta)
    return dX


def _mlp_backward(c, bk, i, q, st, dp, dR3, G3):
    """Adjoint of _mlp_forward -> (dR2 [M,D] f32, G2 = its operand copy * the spatial row scale).  G3: the operand copy of dR3 * dp_m when
    the LayerNorm backward of the block above produced it (fused cast), else None."""
    lay, ix = c.lay, c.lay.ix
    M, D = dR3.shape
    if G3 is None:
        G3 = c.E(M, D)
        ops.scale_cast(c.mode, dR3, dp['m'], G3)
    dpre = c.E(M, q[ix['fc1']].shape[0])
    ops.gemm_nt(c.gmode, G3, c.Wt(q[ix['fc2']]), dpre, act=ACT_MUL_AUX, aux=st['pre'])
    bk.linear_bwd(lay.at(i, 'fc2'), G3, st['H'], defer=True)
    dWn = c.E(M, D)
    ops.gemm_nt(c.gmode, dpre, c.Wt(q[ix['fc1']]), dWn)
    bk.linear_bwd(lay.at(i, 'fc1'), dpre, st['Wn'], defer=True)
    dR2 = c.E(M, D, dtype=f32)
    G2 = c.E(M, D)                           # operand copy of dR2 * row scale: written by the LayerNorm backward, its slot-0 rows redone by the cls adjoint
    dgamma, dbeta = bk.ln_targets(lay.at(i, 'n2'))
    ops.layernorm_bwd(c.mode, dWn, st['R2'], st['mu2'], st['rs2'], q[ix['n2']].detach(), dR3, dR2, dgamma, dbeta,
                      dx_cast=G2, cast_scale=st['rs_s'], defer=bk.ln_jobs)
    return dR2, G2


def _attn_backward(c, bk, i, q, st, dp, mask0, next_scale, dR2, G2):
    """Adjoint of the spatial (divided block) or joint attention -> (dR1 [M,D] f32, G1 = its operand copy * a row scale: a divided block's is
    the output-gradient operand of its temporal projection, a joint block's (no temporal half) that of the block below, scaled by next_scale)."""
    g, lay, ix = c.g, c.lay, c.lay.ix
    B, T, S, D, M = g['B'], g['T'], g['S'], g['D'], g['M']
    if c.use_cls and not c.joint:
        ops.cls_merge(dR2, B, T, S, 1 if c.ca == 1 else 0, backward=True, cast_mode=c.mode, cast_out=G2, cast_scale=st['rs_s'])
    dO2 = c.E(M, D)
    ops.gemm_nt(c.gmode, G2, c.Wt(q[ix['proj']]), dO2)
    bk.linear_bwd(lay.at(i, 'proj'), G2, st['O_s'], defer=True)
    if c.joint:
        dQJ = c.E(B * c.Lj, 3 * D)
        ops.attn_bwd(c.shape_joint, True, st['QKV_s'], st['OJ'], dO2.index_select(0, c.jrows), st['lse_s'], dQJ)
        dQKV2 = torch.zeros(M, 3 * D, dtype=c.dt, device=c.dev)       # the unused cls replicas receive no gradient
        dQKV2.index_copy_(0, c.jrows, dQJ)
    else:
        dQKV2 = c.E(M, 3 * D)
        ops.attn_bwd(c.shape_attn, True, st['QKV_s'], st['O_s'], dO2, st['lse_s'], dQKV2)
    dV = c.E(M, D)
    ops.gemm_nt(c.gmode, dQKV2, c.Wt(q[ix['qkv']]), dV)
    bk.linear_bwd(lay.at(i, 'qkv'), dQKV2, st['V'], defer=True)
    dR1 = c.E(M, D, dtype=f32)
    G1 = c.E(M, D)                           # bf16(dR1 * row scale), written by the same LayerNorm backward pass
    # folded: G1 = bf16(dR1 * mask0 * dp_t) = dY' of the folded projection; its bias b_fc sees dR1 * mask0: summed here, in f32
    extra = dict(cast_scale=dp['t0']) if c.fold else dict(cast_scale=next_scale if c.joint else mask0)
    dgamma, dbeta = bk.ln_targets(lay.at(i, 'n1'))
    if c.fold and bk.grads[lay.at(i, 'tfc', 1)] is not None:
        extra.update(colsum_out=bk.grads[lay.at(i, 'tfc', 1)], colsum_scale=mask0)
        if dgamma is None:           # the column sum rides on the parameter-gradient pass: with n1 frozen that pass writes to scratch
            dgamma, dbeta = c.E(D, dtype=f32), c.E(D, dtype=f32)
    ops.layernorm_bwd(c.mode, dV, st['R1'], st['mu1'], st['rs1'], q[ix['n1']].detach(), dR2, dR1, dgamma, dbeta,
                      dx_cast=G1, defer=bk.ln_jobs, **extra)
    return dR1, G1


def _block_backward_joint(c, bk, i, q, st, dp, mask0, next_scale, dR3, G3):
    """-> (gradient of the block's input [M,D] f32, its operand copy * next_scale): next_scale is the row scale of the operand the block
    below (or the patch embedding) consumes."""
    dR2, G2 = _mlp_backward(c, bk, i, q, st, dp, dR3, G3)
    return _attn_backward(c, bk, i, q, st, dp, mask0, next_scale, dR2, G2)


def _block_backward_divided(c, bk, i, q, st, dp, mask0, next_scale, dR3, G3):
    """-> (dR0, G0), as _block_backward_joint."""
    lay, ix = c.lay, c.lay.ix
    M, D = dR3.shape
    dR2, G2 = _mlp_backward(c, bk, i, q, st, dp, dR3, G3)
    dR1, G1 = _attn_backward(c, bk, i, q, st, dp, mask0, next_scale, dR2, G2)
    # temporal
    dO = c.E(M, D)
    if c.fold:
        ops.gemm_nt(c.gmode, G1, c.opnd.folded(c.mode, i, q, ix, True)[1], dO)
        bk.queue_fold(i, G1, st['O_t'])
    else:
        dPj = c.E(M, D)
        ops.gemm_nt(c.gmode, G1, c.Wt(q[ix['tfc']]), dPj, row_scale=dp['t'])
        bk.linear_bwd(lay.at(i, 'tfc'), G1, st['Pj'], defer=True)
        ops.gemm_nt(c.gmode, dPj, c.Wt(q[ix['tproj']]), dO)
        bk.linear_bwd(lay.at(i, 'tproj'), dPj, st['O_t'], defer=True)
    dQKV = c.E(M, 3 * D)
    ops.attn_bwd(c.shape_attn, False, st['QKV_t'], st['O_t'], dO, st['lse_t'], dQKV)
    dU = c.E(M, D)
    ops.gemm_nt(c.gmode, dQKV, c.Wt(q[ix['tqkv']]), dU)
    bk.linear_bwd(lay.at(i, 'tqkv'), dQKV, st['U'], defer=True)
    dR0 = c.E(M, D, dtype=f32)
    G0 = c.E(M, D)                           # operand of the next (lower) block's MLP backward, or of the patch-embed weight gradient
    dgamma, dbeta = bk.ln_targets(lay.at(i, 'tn'))
    ops.layernorm_bwd(c.mode, dU, st['R0'], st['mu0'], st['rs0'], q[ix['tn']].detach(), dR1, dR0, dgamma, dbeta,
                      dx_cast=G0, cast_scale=next_scale, defer=bk.ln_jobs)
    return dR0, G0


def _embed_backward(c, bk, sv, gX, Gpe):
    """Embeddings (cls, pos, time) and patch embedding from gX [M,D] f32; Gpe = its operand copy * mask0 from block 0's LayerNorm backward.
    -> Gsum, the operand copy of gX summed over each clip's queries (shared rgb; None otherwise), which _input_backward takes as well."""
    Gsum = None
    g, lay, grads = c.g, c.lay, bk.grads
    B, T, S, D = g['B'], g['T'], g['S'], g['D']
    if bk.wants(lay.cls, lay.pos, lay.time, lay.patch_b):
        # (tcow_embed_bwd writes the pos | time pair in one pass, and cls and the patch bias are read off them: a frozen table's half goes to scratch)
        dpos_eff = grads[lay.pos][0] if sv['pos_idx'] is None and grads[lay.pos] is not None else c.E(S, D, dtype=f32)
        dtime_eff = grads[lay.time][0] if sv['time_idx'] is None and grads[lay.time] is not None else c.E(T, D, dtype=f32)
        ops.embed_bwd(gX, B, T, S, dpos_eff, dtime_eff)
        if grads[lay.cls] is not None:
            grads[lay.cls].copy_(dpos_eff[0].reshape(1, 1, D))
        if sv['pos_idx'] is not None and grads[lay.pos] is not None:        # nearest-resized tables (vision_tf.py:103-115): scatter back to the stored rows
            grads[lay.pos].zero_()
            grads[lay.pos][0].index_add_(0, sv['pos_idx'], dpos_eff)
        if sv['time_idx'] is not None and grads[lay.time] is not None:
            grads[lay.time].zero_()
            grads[lay.time][0].index_add_(0, sv['time_idx'], dtime_eff)
    if grads[lay.patch_w] is not None:
        dWpe = grads[lay.patch_w].reshape(D, -1)
        if isinstance(sv['A_pe'], tuple):                               # shared rgb: dW[:, :3 P^2] = (sum over the clip's queries of G)^T A_rgb
            A_rgb, A_m = sv['A_pe']
            Krgb = A_rgb.shape[1]
            Gsum = _query_sum(c, sv, gX)
            ops.gemm_tn(c.gmode, Gsum, A_rgb, dWpe[:, :Krgb])
            ops.gemm_tn(c.gmode, Gpe, A_m, dWpe[:, Krgb:])
        else:
            ops.gemm_tn(c.gmode, Gpe, sv['A_pe'], dWpe)
    if grads[lay.patch_b] is not None:
        grads[lay.patch_b].copy_(dtime_eff.sum(0))       # bias gradient = sum over all patch rows
    return Gsum


def _query_sum(c, sv, gX):
    """Shared rgb: the operand copy of gX [M,D] * mask0 summed over each clip's queries, [Bc*T*S, D]."""
    g = c.g
    B, TS, D = g['B'], g['T'] * g['S'], g['D']
    Bc = sv['A_pe'][0].shape[0] // TS
    Gsum = c.E(Bc * TS, D)
    ops.scale_cast(c.mode, gX.reshape(Bc, B // Bc, TS, D).sum(dim=1).reshape(Bc * TS, D), sv['mask0'][:Bc * TS], Gsum)
    return Gsum


def _input_backward(c, bk, sv, G, want_rgb, want_qm, Gsum=None):
    """Gradients of the frames and of the query mask -> (d_rgb or None, d_qm or None), f32 in the shapes of the inputs.  The patch embedding is
    X = A W_pe^T with A = im2col(cat[rgb, mask]), so dA = G W_pe with the operand G of the patch-embed weight gradient (dR0 * mask0: the cls rows take
    no part) and the transposed operand copy of W_pe the forward already made; col2im, the adjoint of im2col, is a permutation (ops.col2im).  Only
    the rows of W_pe^T whose channels are wanted are multiplied.  G carries the binary16 loss scale, so dA does: col2im multiplies it out (exact, a
    power of two, read on the device) whether or not the parameter buckets stay scaled for the optimizer -- these gradients go back through autograd
    at once.  Runs behind publish('g0'): no bucket is touched, and a data-parallel all-reduce of the last bucket overlaps the two launches."""
    module, g = c.module, c.g
    B, T, S, M, P = g['B'], g['T'], g['S'], g['M'], g['P']
    H, W, PP = g['Hp'] * P, g['Wp'] * P, P * P
    Wt = c.Wt(bk.params[c.lay.patch_w])                                 # [4 P^2, D], channel-major rows (vit.py:233)
    norm, inv = module.tracker_pretrained, bk.inv_gscale
    if not isinstance(sv['A_pe'], tuple):
        dA = c.E(M, 4 * PP, dtype=f32)
        lo, hi = (0 if want_rgb else 3) * PP, (4 if want_qm else 3) * PP
        ops.gemm_nt(c.gmode, G, Wt[lo:hi], dA[:, lo:hi])
        d_rgb = c.E(B, 3, T, H, W, dtype=f32) if want_rgb else None
        d_qm = c.E(B, 1, T, H, W, dtype=f32) if want_qm else None
        ops.col2im(dA, B, T, H, W, P, norm, d_rgb, d_qm, inv_scale=inv)
        return d_rgb, d_qm
    # shared rgb: a clip's frames feed all its queries, so their gradient is the sum over the queries -- taken on the operand (Gsum), before the product
    d_rgb = d_qm = None
    if want_rgb:
        Bc = Gsum.shape[0] // (T * S)
        dA_rgb = c.E(Bc * T * S, 3 * PP, dtype=f32)
        ops.gemm_nt(c.gmode, Gsum, Wt[:3 * PP], dA_rgb)
        d_rgb = ops.col2im_channels(dA_rgb, P, norm, c.E(Bc, 3, T, H, W, dtype=f32), inv_scale=inv)
    if want_qm:
        dA_m = c.E(M, PP, dtype=f32)
        ops.gemm_nt(c.gmode, G, Wt[3 * PP:], dA_m)
        d_qm = ops.col2im_channels(dA_m, P, False, c.E(B, 1, T, H, W, dtype=f32), inv_scale=inv)
    return d_rgb, d_qm


def run_backward(module, sv, params, d_mask, d_flags):
    """-> the parameter gradients, in the order of `params` (None where a parameter takes no part or is frozen), every bucket published.
    Frozen parameters (sv['frozen']) cost nothing: no launch whose only products are their gradients, and the chain runs blocks depth-1 .. sv['k']
    only -- no block below, the embeddings only when one of their parameters is wanted, the inputs only when asked for (_GradBuckets, rule 5).
    sv['want_inputs'] = (frames, query mask), set by SeekerFunction.forward: which input gradients are wanted as well; they are left in
    sv['d_inputs'] (None where not wanted)."""
    c = _Ctx(module, sv['g'], sv['X_final'].device, True)
    have_flags = module.flag_channels > 0 and d_flags is not None and d_flags.numel() > 0
    lay, depth = c.lay, module.network_depth
    k = sv.get('k', 0)                             # the chain stops below block k (lowest_block(), fixed by the forward with sv['frozen'])
    bk = _GradBuckets(c, params, have_flags, sv.get('frozen', frozenset()), k)
    dR, G = _heads_backward(c, bk, sv, params, d_mask, d_flags, have_flags), None
    block_backward = _block_backward_joint if c.joint else _block_backward_divided
    for i in reversed(range(k, depth)):
        bk.start_block(i)
        next_scale = sv['dps'][i - 1]['m'] if i > 0 else sv['mask0']
        dR, G = block_backward(c, bk, i, params[lay.block(i)], sv['blocks'][i], sv['dps'][i], sv['mask0'], next_scale, dR, G)
        bk.end_block(i, sv)
    bk.finish_late()
    Gsum = _embed_backward(c, bk, sv, dR, G) if bk.wants(*lay.embed) else None
    if k == 0 or k == depth:                       # (0 < k < depth: end_block(k) has published the last bucket, as 'g<k>')
        bk.publish('g%d' % k, bk.flat)
    module.pending_inv_scale = bk.inv_gscale if bk.defer_unscale else None
    want_rgb, want_qm = sv.get('want_inputs', (False, False))
    if want_rgb and Gsum is None and isinstance(sv['A_pe'], tuple):
        Gsum = _query_sum(c, sv, dR)                # (shared rgb with a frozen patch weight: the frames' gradient needs the sum all the same)
    sv['d_inputs'] = _input_backward(c, bk, sv, G, want_rgb, want_qm, Gsum) if want_rgb or want_qm else (None, None)
    if bk.hook is not None and hasattr(bk.hook, 'finish'):
        # The collectives launched above were overlapped with the remaining backward compute; they must be complete (in
        # stream order) before autograd copies the bucket views into param.grad, so the hook is drained here.
        bk.hook.finish()
    return bk.grads


class SeekerFunction(torch.autograd.Function):
    """(module, rgb, query_mask, *params) -> (output_mask, output_flags)."""

    @staticmethod
    def forward(ctx, module, rgb, qm, *params):
        need = any(ctx.needs_input_grad[1:])      # a parameter, the frames (1) or the query mask (2)
        ctx.set_materialize_grads(False)      # an unused output (e.g. output_flags in Kubric training) arrives as None, not zeros
        # the frozen set is read here, once, and holds for this forward's backward: requires_grad_() between the two changes nothing
        frozen = frozenset(j for j, wanted in enumerate(ctx.needs_input_grad[3:]) if not wanted)
        out_mask, flags, sv = run_forward(module, rgb, qm, params, save=need, frozen=frozen, want_inputs=(ctx.needs_input_grad[1], ctx.needs_input_grad[2]))
        ctx.module = module
        ctx.sv = sv
        ctx.params = params
        return out_mask, flags

    @staticmethod
    def backward(ctx, d_mask, d_flags):
        if ctx.sv is None:
            raise ops.L.TcowError('backward called on a forward that did not save activations')
        grads = run_backward(ctx.module, ctx.sv, ctx.params, d_mask, d_flags)
        d_rgb, d_qm = ctx.sv['d_inputs']
        ctx.sv = None
        out = []
        persistent = getattr(ctx.module, 'persistent_grads', False)
        for p, gr, need in zip(ctx.params, grads, ctx.needs_input_grad[3:]):
            if not need or gr is None:
                out.append(None)
                continue
            gr = gr.reshape(p.shape)
            if persistent and (p.grad is None or p.grad.data_ptr() == gr.data_ptr()):
                p.grad = gr          # delivered out of band: the same storage every step, no autograd copy
                out.append(None)
            else:
                out.append(gr)
        return (None, d_rgb, d_qm, *out)

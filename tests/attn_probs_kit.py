"""What the attention-map tests share: the float64 softmax of the SAME stored q and k that tcow_attn_probs reads, laid out as the entry point's
outputs, and the derived bound.  The sequences (seq_rows) and the 'exact' score model (_scores) are tests/test_gpu_attention.py's, by name."""
import math

import torch

from test_gpu_attention import _scores, seq_rows

U32 = 2.0 ** -24


def storage(ops, mname):
    """(ops mode, torch dtype) of a storage type; 'f32x3' stores f32 and takes the f32 kernel."""
    return {'f32': (ops.F32, torch.float32), 'f32x3': (ops.F32X3, torch.float32), 'bf16': (ops.BF16, torch.bfloat16),
            'fp16': (ops.FP16, torch.float16)}[mname]


def draw_qkv(B, T, S, heads, dtype, dev, seed=0, zero_q=False):
    """N(0, 1) q, k, v rounded to the storage type before either side sees them."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    x = torch.randn(B * T * S, 3, heads * 64, generator=g)
    if zero_q:
        x[:, 0] = 0
    return x.reshape(B * T * S, 3 * heads * 64).to(dtype).to(dev)


def ref64(qkv, B, T, S, heads, ca, spatial, pos=None):
    """-> dict: P float64 in the entry point's layout (temporal [B, S-1, heads, T, T]; rows [G, nq, heads, S], column 0 zero when the cls is
    out), keep (bool, same shape: the entries the mask allows), lse float64 ([N, heads, T] temporal / [G, nq, heads] rows), delta = 66 u
    max_ij sum_c |q_c k_c| / 8, n_keys, rows [N, L] and v [N, heads, L, 64]."""
    M, dev = qkv.shape[0], qkv.device
    rows, diag = seq_rows(B, T, S, spatial, ca)
    rows = rows.to(dev)
    N, L = rows.shape
    x = qkv.double().view(M, 3, heads, 64)[rows]                                # [N, L, 3, H, 64]
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))               # [N, H, L, 64]
    if pos is not None:
        q = q[:, :, torch.as_tensor(pos, device=dev, dtype=torch.long)]
    Lq = q.shape[2]
    s = _scores(q.reshape(N * heads, Lq, 64), k.reshape(N * heads, L, 64), 'exact').view(N, heads, Lq, L)
    mag = (q.abs().reshape(N * heads, Lq, 64) @ k.abs().reshape(N * heads, L, 64).transpose(1, 2)).max() / 8
    delta = 66 * U32 * float(mag)
    kpos = torch.arange(L, device=dev)
    qpos = kpos if pos is None else torch.as_tensor(pos, device=dev, dtype=torch.long)
    keep = (kpos[None, :] <= qpos[:, None] + diag).expand(N, heads, Lq, L)
    s = s.masked_fill(~keep, float('-inf'))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    if spatial:
        s0 = S - L
        P = torch.nn.functional.pad(P, (s0, 0)).permute(0, 2, 1, 3).contiguous()          # [G, nq, H, S]
        keep = torch.nn.functional.pad(keep, (s0, 0)).permute(0, 2, 1, 3).contiguous()
        lse = lse.permute(0, 2, 1).contiguous()
    return dict(P=P, keep=keep, lse=lse, delta=delta, n_keys=L, rows=rows, v=v, L=L)


def prob_bound(ref):
    """|P - P64| <= P64 (expm1(2 delta) + (n_keys + 8) u) + 1e-30: the score error enters through the numerator and through Z, n_keys additions
    in Z, a few ulp for exp, subtract and divide, the floor for flushed denormals."""
    return ref['P'] * (math.expm1(2 * ref['delta']) + (ref['n_keys'] + 8) * U32) + 1e-30


def lse_bound(ref):
    return 2 * ref['delta'] + 4 * U32 * ref['lse'].abs()


def worst(got, want, bound):
    """(index of the worst excess, got, want, |d|, bound there); excess <= 0 everywhere = pass.  A NaN in got fails."""
    d = (got.double() - want).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float('inf')), d)
    i = int((d - bound).argmax())
    idx = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), d.shape))
    return idx, float(got.reshape(-1)[i]), float(want.reshape(-1)[i]), float(d.reshape(-1)[i]), float(bound.reshape(-1)[i])

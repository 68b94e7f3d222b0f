"""Dev: time the attention kernels one by one (HIP events around single launches) at the benchmark shape + check EVERY (sequence, head) vs torch.
Environment: B (3), S (301), T (30), FWD_ONLY=1; MODE=bf16 (default) | f32x3 (f32 tensors, the split-bf16 kernels of attention_x3.hip);
TEMPORAL=1: temporal attention (one sequence of T frames per patch slot) instead of spatial, CAUSAL (1) its causal_attention; JSON=1 adds a line
{"kind", "mode", "fwd_us", "bwd_us", ...} for drivers.  (TCOW_LIB=<another build> compares builds on one box; under `rocprofv3 --kernel-trace --stats`
the per-kernel durations come from the trace, tools/prof_attn.sh.)"""
import json, os, sys, torch
sys.path.insert(0, '.')
from tcow_amd import ops
dev = 'cuda'
B, T, S, heads = int(os.environ.get('B', '3')), int(os.environ.get('T', '30')), int(os.environ.get('S', '301')), 12; D = heads * 64; M = B * T * S
mname = os.environ.get('MODE', 'bf16'); mode, dt = {'bf16': (ops.BF16, torch.bfloat16), 'f32x3': (ops.F32X3, torch.float32)}[mname]
temporal = bool(os.environ.get('TEMPORAL')); causal = int(os.environ.get('CAUSAL', '1')) if temporal else 1; kind = 'temporal' if temporal else 'spatial'
torch.manual_seed(0)
qkv = torch.randn(M, 3 * D, device=dev).to(dt); out = torch.empty(M, D, device=dev, dtype=dt); lse = torch.empty(M, heads, device=dev)
dout = torch.randn(M, D, device=dev).to(dt); dqkv = torch.empty(M, 3 * D, device=dev, dtype=dt)
shape = ops.attn_shape(mode, B, T, S, D, heads, causal)
def bench(f, n=20, w=5):
    for _ in range(w): f()
    torch.cuda.synchronize(); e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True); e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize(); return e0.elapsed_time(e1) / n * 1e3
def seqs(x, w):
    """[M, w] -> (sequences, L, w): spatial = the S slots of a frame, temporal = the T frames of a patch slot (slot 0 takes no part)"""
    x = x.float().reshape(B, T, S, w)
    return x.permute(0, 2, 1, 3)[:, 1:].reshape(B * (S - 1), T, w) if temporal else x.reshape(B * T, S, w)
def attend(x):
    """x (sequences, L, 3, h, 64) f32 -> out (sequences, L, h, 64), lse (sequences, L, h)"""
    q, k, v = [x[:, :, i].permute(0, 2, 1, 3) for i in range(3)]                   # (n, h, L, 64)
    sc = (q @ k.transpose(-1, -2)) * 0.125
    if temporal and causal > 0:
        L = sc.shape[-1]; sc = sc.masked_fill(~torch.ones(L, L, dtype=torch.bool, device=x.device).tril(0 if causal <= 2 else causal - 2), float('-inf'))
    return (sc.softmax(-1) @ v).permute(0, 2, 1, 3), torch.logsumexp(sc, -1).permute(0, 2, 1)
out.fill_(float('nan')); lse.fill_(float('nan'))
ops.attn_fwd(shape, not temporal, qkv, out, lse); torch.cuda.synchronize()
# correctness of the forward on every sequence / head against torch f32 (+ log-sum-exp)
x = seqs(qkv, 3 * D); x = x.reshape(x.shape[0], x.shape[1], 3, heads, 64)
ref, ref_lse = attend(x)
got, got_lse = seqs(out, D), seqs(lse, heads)
ef = (got - ref.reshape(got.shape)).abs().max().item(); el = (got_lse - ref_lse).abs().max().item()
bad = (~torch.isfinite(got)).sum().item()
tf = bench(lambda: ops.attn_fwd(shape, not temporal, qkv, out, lse))
res = {'kind': kind, 'mode': mname, 'B': B, 'T': T, 'S': S, 'fwd_us': tf, 'fwd_max_abs_d': ef, 'lse_max_abs_d': el, 'non_finite': bad}
msg = f'S={S} B={B} T={T} {mname}: {kind} fwd {tf:.1f} us | max|d| out {ef:.2e} lse {el:.2e} non-finite {bad} (ref max {ref.abs().max().item():.2f})'
if not os.environ.get('FWD_ONLY'):
    tb = bench(lambda: ops.attn_bwd(shape, not temporal, qkv, out, dout, lse, dqkv))
    xg = x[:1].clone().requires_grad_(True)                                          # the first sequence: L,3,h,64
    (attend(xg)[0] * seqs(dout, D)[:1].reshape(1, -1, heads, 64)).sum().backward()
    eb = (seqs(dqkv, 3 * D)[:1].reshape(xg.shape) - xg.grad).abs().max().item()
    res.update(bwd_us=tb, bwd_max_abs_d=eb)
    msg += f' | bwd {tb:.1f} us max|d| {eb:.2e} (ref max {xg.grad.abs().max().item():.2f})'
print(msg, flush=True)
if os.environ.get('JSON'): print('JSON ' + json.dumps(res), flush=True)

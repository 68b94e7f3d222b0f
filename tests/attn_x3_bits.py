"""GPU kit: ops.attn_fwd and ops.attn_bwd in mode F32X3 (csrc/attention_x3.hip) on fixed inputs, every result hashed.  run() -> {case: {tensor: sha256}};
tests/golden/attn_x3_bits.json holds it as recorded on the MI355X from the package and libraries of the commit BEFORE the x3 kernels were rewritten on
attention_tiles.h's helpers and forward tile step (tools/make_attn_x3_bits.py; never recorded from the tree it holds to those bits),
tests/test_gpu_attn_x3_bits.py recomputes it.  ops.attn_fwd / attn_bwd are the same on both sides, so this file runs on both.

Inputs: fixed-seed normal qkv and dout from numpy's generator on the host.  out, lse and dqkv start at 0.0, so rows of no sequence (the slot-0 rows
of temporal attention, whose lse no kernel writes) are pinned too.  Each tensor is hashed as t + 0.0: a -0 counts as +0 (masking a score before the
exp2 can turn a masked dS of +0 into -0, and nothing else).

B = 1, heads = 3; two patch slots (temporal) or two frames (spatial): 6 (sequence, head) pairs, so the second SOLO workgroup is half filled and the
chunked kernels' grid of 8 has two workgroups with no pair.  The shapes are the smallest at which each path of the kernels can go wrong:
  temporal, one tile (SOLO kernels)   L = 5 causal 1 (padded tile, causal mask inside it), L = 32 no mask (a full tile), L = 30 causal 3 (look-ahead diagonal)
  temporal, two tiles (chunked)       L = 40 causal 1 and 3 (causal_key_tiles / causal_first_query_tile, a partial last tile)
  spatial                             L = 33 (nt = 2: one forward chunk of CH = 2, one partial backward chunk of CH = 4), L = 130 (nt = 5: a second workgroup
                                      with one live wave, 3 forward / 2 backward chunks, a last tile of 2 rows), L = 257 (nt = 9: three workgroups per pair, a
                                      last tile of 1 row, a chunk boundary inside a workgroup's range)"""
import hashlib

import numpy as np
import torch

from tcow_amd import ops

HEADS, D = 3, 192
# case: (spatial, T, S, causal_attention)
CASES = {'temporal-L5-causal1': (False, 5, 3, 1), 'temporal-L32-causal0': (False, 32, 3, 0), 'temporal-L30-causal3': (False, 30, 3, 3),
         'temporal-L40-causal1': (False, 40, 3, 1), 'temporal-L40-causal3': (False, 40, 3, 3),
         'spatial-L33': (True, 2, 33, 0), 'spatial-L130': (True, 2, 130, 0), 'spatial-L257': (True, 2, 257, 0)}
TENSORS = ('out', 'lse', 'dqkv')


def _sha(t):
    return hashlib.sha256((t.detach() + 0.0).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _randn(seed, shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).cuda()


def case(name):
    """{tensor: sha256} of one case."""
    spatial, T, S, causal = CASES[name]
    rows = T * S
    shape = ops.attn_shape(ops.F32X3, 1, T, S, D, HEADS, causal)
    qkv, dout = _randn(1, (rows, 3 * D)), _randn(2, (rows, D))
    out, lse, dqkv = torch.zeros(rows, D, device='cuda'), torch.zeros(rows, HEADS, device='cuda'), torch.zeros(rows, 3 * D, device='cuda')
    ops.attn_fwd(shape, spatial, qkv, out, lse)
    ops.attn_bwd(shape, spatial, qkv, out, dout, lse, dqkv)
    torch.cuda.synchronize()
    return {'out': _sha(out), 'lse': _sha(lse), 'dqkv': _sha(dqkv)}


def run():
    return {name: case(name) for name in CASES}

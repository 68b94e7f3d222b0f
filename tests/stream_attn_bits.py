"""GPU kit: the seven stream wrappers of tcow_amd.ops (attn_temporal_cached / _pool / _ragged / _ragged_paged, cls_stream / _pool / _ragged) on fixed
inputs, every result hashed.  run() -> {case: {tensor: sha256}}; tests/golden/stream_attn_bits.json holds it as recorded on the MI355X from the package
and libraries of the commit BEFORE the stream step's entry points became one (tools/make_stream_attn_bits.py; never recorded from the tree it holds
to those bits), tests/test_gpu_stream_attn_bits.py recomputes it.  The wrappers' signatures are the same on both sides, so this file runs on both.

Inputs come from numpy's generator on the host.  S = 3, heads = 2, T_total = 40: the smallest at which every branch of the host code and both key
loops of the kernels run (16-bit storage: 32 keys per batch, so t0 = 35 leaves one whole batch below t0 for the compact cache's branch-free loop
and a second, partial one; f32: 16 per batch).  Geometries: the stream (B = 2, c = 3, t0 = 35), the pool (t0 = [35, 0], slots permuted), a ragged
step (c = [3, 1, 2], t0 = [35, 0, 17]), that step on pages of P = 2 and P = 8 through a shuffled table, and T_total = 70 on pages of one frame
(c = [5, 1], t0 = [62, 0]: table entries on both sides of lane 64); one bad row per form (t0, slot, t0, page outside its range: NaN rows, caches
untouched).  Each under every (storage, cache) pair of PAIRS.  cls: the three wrappers at D = 128, rows at t0 = 0 and t0 > 0."""
import hashlib

import numpy as np
import torch

from tcow_amd import ops

S, HEADS, D = 3, 2, 128
PAIRS = {'bf16/None': (ops.BF16, None), 'bf16/fp8': (ops.BF16, ops.FP8), 'fp16/None': (ops.FP16, None), 'fp16/fp8': (ops.FP16, ops.FP8),
         'f32/None': (ops.F32, None), 'f32/bf16': (ops.F32, ops.BF16), 'f32/fp8': (ops.F32, ops.FP8), 'f32x3/None': (ops.F32X3, None)}


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device='cuda')


def _randn(seed, shape, dtype):
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))
    return (x.clamp(-448, 448) if dtype == torch.float8_e4m3fn else x).to(dtype).cuda()


def _cache_type(mode, cq):
    return torch.float8_e4m3fn if cq == ops.FP8 else torch.bfloat16 if cq == ops.BF16 else ops.tdtype(mode)


def _tables(cs):
    first = [sum(cs[:r]) for r in range(len(cs))]
    return first, [r for r, c in enumerate(cs) for _ in range(c)]


def _attn(mode, cq, frames, cache_shape, seed, launch):
    """launch(qkv, k, v, out, cache_dtype) on random rows and random caches (every position: an untouched one keeps its bits)."""
    dt, cdt = ops.tdtype(mode), _cache_type(mode, cq)
    qkv = _randn(seed, (frames * S, 3 * D), dt)
    k, v = _randn(seed + 1, cache_shape, cdt), _randn(seed + 2, cache_shape, cdt)
    out = torch.full((frames * S, D), 7.0, device='cuda', dtype=dt)
    launch(qkv, k, v, out, cq)
    torch.cuda.synchronize()
    return {'out': _sha(out), 'k_cache': _sha(k), 'v_cache': _sha(v)}


def attention_cases(pair):
    """{case: hashes} of every geometry under one (storage, cache) pair."""
    mode, cq = PAIRS[pair]
    T, res = 40, {}

    def stream(t0):
        return _attn(mode, cq, 2 * 3, (2, S - 1, HEADS, T, 64), 10, lambda qkv, k, v, out, cd: ops.attn_temporal_cached(
            mode, 2, 3, S, D, HEADS, 1, T, _i32([t0]), qkv, k, v, out, cache_dtype=cd))

    def pool(slots):
        return _attn(mode, cq, 2 * 3, (3, S - 1, HEADS, T, 64), 20, lambda qkv, k, v, out, cd: ops.attn_temporal_pool(
            mode, 2, 3, S, D, HEADS, 1, T, 3, _i32([35, 0]), _i32(slots), qkv, k, v, out, cache_dtype=cd))

    def ragged(t0s):
        cs = [3, 1, 2]
        first, rof = _tables(cs)
        return _attn(mode, cq, 6, (4, S - 1, HEADS, T, 64), 30, lambda qkv, k, v, out, cd: ops.attn_temporal_ragged(
            mode, 3, 6, S, D, HEADS, 1, T, 4, _i32(t0s), _i32([2, 0, 3]), _i32(first), _i32(cs), _i32(rof), qkv, k, v, out, cache_dtype=cd))

    def paged(T_total, P, cs, t0s, seed, spoil=None):
        n, pps = len(cs), -(-T_total // P)
        n_pages = n * pps + 3
        table = np.random.default_rng(seed).permutation(n_pages)[:n * pps].reshape(n, pps).astype(np.int64)
        assert (np.diff(table[0]) < 0).any()                        # (not the identity)
        if spoil is not None:
            table[spoil] = n_pages
        first, rof = _tables(cs)
        return _attn(mode, cq, sum(cs), (n_pages, S - 1, HEADS, P, 64), seed, lambda qkv, k, v, out, cd: ops.attn_temporal_ragged_paged(
            mode, n, sum(cs), S, D, HEADS, 1, T_total, n_pages, P, _i32(t0s), _i32(table.tolist()), _i32(first), _i32(cs), _i32(rof), qkv, k, v, out,
            cache_dtype=cd))

    res['stream'] = stream(35)
    res['pool'] = pool([2, 0])
    res['ragged'] = ragged([35, 0, 17])
    res['paged-P2'] = paged(T, 2, [3, 1, 2], [35, 0, 17], 40)
    res['paged-P8'] = paged(T, 8, [3, 1, 2], [35, 0, 17], 50)
    res['paged-T70-P1'] = paged(70, 1, [5, 1], [62, 0], 60)
    res['bad-stream-t0'] = stream(38)                               # t0 + c > T_total: every row
    res['bad-pool-slot'] = pool([3, 0])                             # row 0 names slot 3 of 3
    res['bad-ragged-t0'] = ragged([35, -1, 17])                     # session 1
    res['bad-paged-page'] = paged(T, 8, [3, 1, 2], [35, 0, 17], 50, spoil=(0, 2))      # session 0 reads pages 0 .. 4 of its row
    return res


def cls_cases():
    def run(seed, frames, n_slots, launch):
        x, cache = _randn(seed, (frames * S, D), torch.float32), _randn(seed + 1, (n_slots, D), torch.float32)
        launch(x, cache)
        torch.cuda.synchronize()
        return {'x': _sha(x), 'cls_cache': _sha(cache)}

    first, _ = _tables([3, 1, 2])
    return {'cls-stream-t0=0': run(70, 6, 2, lambda x, cache: ops.cls_stream(x, 2, 3, S, cache, _i32([0]))),
            'cls-stream-t0=35': run(70, 6, 2, lambda x, cache: ops.cls_stream(x, 2, 3, S, cache, _i32([35]))),
            'cls-pool': run(80, 6, 3, lambda x, cache: ops.cls_pool(x, 2, 3, S, cache, 3, _i32([35, 0]), _i32([2, 0]))),
            'cls-ragged': run(90, 6, 4, lambda x, cache: ops.cls_ragged(x, 3, 6, S, cache, 4, _i32([35, 0, 17]), _i32([2, 0, 3]), _i32(first), _i32([3, 1, 2]))),
            'cls-bad-slot': run(80, 6, 3, lambda x, cache: ops.cls_pool(x, 2, 3, S, cache, 3, _i32([35, 0]), _i32([3, 0])))}


def run():
    doc = {f'{pair}/{case}': h for pair in PAIRS for case, h in attention_cases(pair).items()}
    doc.update(cls_cases())
    return doc

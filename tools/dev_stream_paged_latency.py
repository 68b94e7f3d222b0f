"""Dev: what a paged K / V cache costs a pool step (stream_pool(page_frames=P), tcow_amd/stream.py), on the GPU.

    python tools/dev_stream_paged_latency.py --out profiles/stream_paged_latency.json
                                        # one-frame pool.step at t0 = T - 1 (the longest key loop) on a contiguous pool and on paged pools of
                                        # P = 1, 4, 8, 16, 32, the six legs alternating in one run: configs[1] with 8 sessions and configs[3] with 1
                                        # session, in bf16 and bf16x3
    --only configs1_n8_bf16,configs3_n1_bf16x3      a subset of the four runs
    python tools/dev_stream_paged_latency.py --kernel --out profiles/stream_paged_kernel.json
                                        # the attention launch alone at the same grids (one block's launch of such a step): the pool kernel, the
                                        # ragged kernel and the paged kernel at P = 1, 8, 32, alternating, ten launches between a pair of events

The protocol of tools/dev_stream_latency.py: device events around each call after warm-up, profiler off, the legs taken in turn `--reps` times so
that drift of the machine hits all alike.  The yardstick of a paged leg is the contiguous leg of the same run: its median, and its own max - min as
the spread a difference has to exceed.  recommended_P is the smallest P whose median lies within that spread of the contiguous median (None if
there is none).  Every pool is warmed up with the whole clip, so each session owns all its pages; the step's work depends on t0, not on what the
cache holds.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dev_stream_latency import CONFIGS, build, ev_time, inputs       # noqa: E402
from tcow_amd import ops                                             # noqa: E402

PAGE_FRAMES = [1, 4, 8, 16, 32]
RUNS = [('configs1', 8, 'bf16'), ('configs1', 8, 'bf16x3'), ('configs3', 1, 'bf16'), ('configs3', 1, 'bf16x3')]


def page_bytes(H, W, P, elem, depth=12, heads=12):
    """Device bytes of one page: K and V lines of P frames for every block, token slot and head -- 2 * depth * (S-1) * heads * P * 64 * elem."""
    return 2 * depth * (H // 16) * (W // 16) * heads * P * 64 * elem


def paged_leg(name, n, precision, reps):
    T, H, W = CONFIGS[name]
    net = build(T, H, W, precision)
    rgb, qm = inputs(n, T, H, W)
    f = lambda x, t: x[:, :, t:t + 1]
    with torch.no_grad():
        pools = {'contiguous': net.stream_pool(n)}
        for P in PAGE_FRAMES:
            pools[f'P{P}'] = net.stream_pool(n, page_frames=P)
        ids = {k: [p.open() for _ in range(n)] for k, p in pools.items()}
        for k, p in pools.items():                              # warm-up: the whole clip once (every cache row and page is filled)
            for t in range(T):
                p.step(ids[k], f(rgb, t), f(qm, t))
        r1, q1 = f(rgb, T - 1).contiguous(), f(qm, T - 1).contiguous()

        def leg(k):
            p = pools[k]

            def one():
                for sid in ids[k]:
                    p._done[sid] = T - 1
                p.step(ids[k], r1, q1)
            return one

        legs = {k: leg(k) for k in pools}
        for fn in legs.values():
            for _ in range(3):
                fn()
        samples = {k: [] for k in legs}
        for _ in range(reps):
            for k, fn in legs.items():
                samples[k].append(ev_time(fn, 1))
    elem = 2 if precision in ('bf16', 'fp16') else 4
    res = {'config': name, 'T': T, 'H': H, 'W': W, 'sessions': n, 'precision': precision, 't0': T - 1, 'reps': reps,
           'cache_bytes': {k: p.cache_bytes for k, p in pools.items()}, 'page_bytes': {f'P{P}': page_bytes(H, W, P, elem) for P in PAGE_FRAMES}}
    for k, v in samples.items():
        v = sorted(v)
        res[k + '_step_ms'] = {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}
    c = res['contiguous_step_ms']
    spread = c['max'] - c['min']
    res['contiguous_spread_ms'] = spread
    res['paged_over_contiguous'] = {f'P{P}': res[f'P{P}_step_ms']['median'] / c['median'] for P in PAGE_FRAMES}
    res['paged_minus_contiguous_ms'] = {f'P{P}': res[f'P{P}_step_ms']['median'] - c['median'] for P in PAGE_FRAMES}
    within = [P for P in PAGE_FRAMES if res[f'P{P}_step_ms']['median'] - c['median'] <= spread]
    res['within_contiguous_spread'] = within
    res['recommended_P'] = within[0] if within else None
    del pools, legs, net
    torch.cuda.empty_cache()
    return res


def kernel_leg(name, n, storage, reps, heads=12, D=768):
    """One block's temporal-attention launch of the one-frame step at t0 = T - 1 (n sessions, random contents and a random page table), in us per
    launch: tcow_attn_temporal_step in its pool (rows), ragged and paged ragged forms at P = 1, 8, 32."""
    T, H, W = CONFIGS[name]
    S = (H // 16) * (W // 16) + 1
    mode, dt = (ops.BF16, torch.bfloat16) if storage == 'bf16' else (ops.F32, torch.float32)
    dev = torch.device('cuda')
    i32 = lambda v: torch.tensor(list(v), dtype=torch.int32, device=dev)
    qkv = torch.randn(n * S, 3 * D, device=dev).to(dt)
    kc = torch.randn(n, S - 1, heads, T, 64, device=dev).to(dt)
    vc = torch.randn_like(kc)
    out = torch.empty(n * S, D, device=dev, dtype=dt)
    t0, slot, first, c, rof = i32([T - 1] * n), i32(range(n)), i32(range(n)), i32([1] * n), i32(range(n))
    legs = {'pool': lambda: ops.attn_temporal_pool(mode, n, 1, S, D, heads, 1, T, n, t0, slot, qkv, kc, vc, out),
            'ragged': lambda: ops.attn_temporal_ragged(mode, n, n, S, D, heads, 1, T, n, t0, slot, first, c, rof, qkv, kc, vc, out)}
    for P in (1, 8, 32):
        pps = -(-T // P)
        kp = torch.randn(n * pps, S - 1, heads, P, 64, device=dev).to(dt)
        vp = torch.randn_like(kp)
        pages = torch.randperm(n * pps, device=dev).to(torch.int32).view(n, pps).contiguous()
        legs[f'paged_P{P}'] = (lambda P=P, kp=kp, vp=vp, pages=pages: ops.attn_temporal_ragged_paged(
            mode, n, n, S, D, heads, 1, T, kp.shape[0], P, t0, pages, first, c, rof, qkv, kp, vp, out))

    def ten(fn):
        for _ in range(10):
            fn()
    for fn in legs.values():
        ten(fn)
    samples = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            samples[k].append(ev_time(lambda: ten(fn), 1) * 100)       # us per launch
    res = {'config': name, 'sessions': n, 'storage': storage, 'S': S, 'T': T, 't0': T - 1, 'reps': reps}
    for k, v in samples.items():
        v = sorted(v)
        res[k + '_us'] = {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--kernel', action='store_true', help='the attention launch alone: pool, ragged and paged kernels at the grids of the four runs')
    ap.add_argument('--only', default=None, help='comma list of configs1_n8_bf16, configs1_n8_bf16x3, configs3_n1_bf16, configs3_n1_bf16x3')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dev_stream_paged_latency.py needs a GPU')
    if a.kernel:
        out = {'device': torch.cuda.get_device_name(0), 'kernel': []}
        for name, n, storage in (('configs1', 8, 'bf16'), ('configs1', 8, 'f32'), ('configs3', 1, 'bf16'), ('configs3', 1, 'f32')):
            out['kernel'].append(kernel_leg(name, n, storage, a.reps))
            print(json.dumps(out['kernel'][-1]), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                json.dump(out, fh, indent=1)
        return
    runs = RUNS
    if a.only:
        keep = set(a.only.split(','))
        runs = [r for r in runs if f'{r[0]}_n{r[1]}_{r[2]}' in keep]
    out = {'device': torch.cuda.get_device_name(0), 'page_frames': PAGE_FRAMES, 'runs': []}
    for name, n, precision in runs:
        r = paged_leg(name, n, precision, a.reps)
        print(json.dumps(r), flush=True)
        out['runs'].append(r)
        if a.out:                                               # (after every run: a later run that fails keeps the earlier ones)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()

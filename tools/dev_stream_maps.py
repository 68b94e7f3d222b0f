"""Dev: what the attention maps of a live session cost (SeekerStream.step_maps / SeekerStreamPool.step_maps, tcow_attn_temporal_step_probs), on the GPU.

    python tools/dev_stream_maps.py --out profiles/stream_maps.json
                                        # configs[1], B = 1, bf16: a one-frame step() against step_maps() with all 12 blocks, temporal maps and 'cls',
                                        # at t0 = 0, 15, 29, the two legs alternating in one process, median of --reps (10); the same for one step of
                                        # a pool of eight sessions at spread t0; and the new kernel alone (us per launch, algorithmic bytes)
    python tools/dev_stream_maps.py --plain --out plain.json
                                        # plain step() only: one-frame eager at t0 = 29, graph replay, the pool of eight -- run once on this tree and
                                        # once on the parent commit's tree (the tool itself needs nothing of this change in that mode)
    python tools/dev_stream_maps.py --out profiles/stream_maps.json --plain-change c1.json,c2.json,... --plain-parent p1.json,p2.json,...
                                        # the full run, with the --plain runs of both sides folded in (comma lists, the sides run alternately): each
                                        # leg of the change must lie inside the parent leg's own max - min spread (the criterion of
                                        # profiles/stream_plan_refactor.json)

Times are device events around each call after warm-up, profiler off; a step at a given t0 is timed by setting the host frame counter, as in
tools/dev_stream_latency.py (the work of a step depends on t0, not on what the cache holds).  Synthetic weights / clips; depth 12 ViT-B."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dev_stream_latency import CONFIGS, build, ev_time, inputs      # noqa: E402

POOL_SESSIONS = 8
MAPS = dict(blocks=None, temporal=True, spatial_slots='cls')


def _mmm(v):
    v = sorted(v)
    return {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}


def alternate(legs, reps):
    """Every leg three times to warm up, then the legs in turn `reps` times (drift of the machine hits all alike) -> {leg: median / min / max ms}."""
    samples = {k: [] for k in legs}
    for fn in legs.values():
        for _ in range(3):
            fn()
    for _ in range(reps):
        for k, fn in legs.items():
            samples[k].append(ev_time(fn, 1))
    return {k: _mmm(v) for k, v in samples.items()}


def _pool(net, rgb, qm, T):
    n = POOL_SESSIONS
    pool = net.stream_pool(n)
    ids = [pool.open() for _ in range(n)]
    for t in range(T):                                          # warm-up: the whole clip once (fills every cache row)
        pool.step(ids, rgb[:, :, t:t + 1], qm[:, :, t:t + 1])
    t0s = [round(k * (T - 1) / (n - 1)) for k in range(n)]
    rgb_a = torch.cat([rgb[k:k + 1, :, t0:t0 + 1] for k, t0 in enumerate(t0s)], 0)
    qm_a = torch.cat([qm[k:k + 1, :, t0:t0 + 1] for k, t0 in enumerate(t0s)], 0)

    def at_t0s():
        for sid, t0 in zip(ids, t0s):
            pool._done[sid] = t0
    return pool, ids, t0s, rgb_a, qm_a, at_t0s


def plain_legs(reps):
    """step() alone: one-frame eager and graph replay at t0 = T - 1 (B = 1) and one step of the pool of eight, alternating."""
    T, H, W = CONFIGS['configs1']
    net = build(T, H, W, 'bf16')
    rgb, qm = inputs(POOL_SESSIONS, T, H, W)
    f = lambda x, t: x[0:1, :, t:t + 1]
    with torch.no_grad():
        eager, graph = net.stream(batch_size=1), net.stream(batch_size=1, graph=True)
        for t in range(T):
            eager.step(f(rgb, t), f(qm, t)); graph.step(f(rgb, t), f(qm, t))
        pool, ids, t0s, rgb_a, qm_a, at_t0s = _pool(net, rgb, qm, T)

        def one(st):
            st.frames_done = T - 1
            st.step(f(rgb, T - 1), f(qm, T - 1))

        def pool_step():
            at_t0s()
            pool.step(ids, rgb_a, qm_a)
        res = alternate({'eager_step_ms': lambda: one(eager), 'graph_step_ms': lambda: one(graph), 'pool8_step_ms': pool_step}, reps)
    return {'config': 'configs1', 'precision': 'bf16', 'reps': reps, 't0': T - 1, 'pool_t0_rows': t0s, **res}


def kernel_bytes(F_t, S, heads, T, e, ce):
    """Algorithmic bytes of one tcow_attn_temporal_step_probs launch: per (frame at t, slot >= 1, head) the q line and the frame's own key line
    in the storage type (e bytes an element), t cached key lines (ce bytes an element), and the row of T floats written once.  F_t: the t of
    every flat frame of a one-frame-per-session step."""
    per = sum(64 * e * 2 + t * 64 * ce + 4 * T for t in F_t)
    return per * (S - 1) * heads


def kernel_alone(net, T, batch=20):
    """The launch alone at the shapes of a one-frame configs[1] step: B = 1 at t0 = 0, 15, 29 (the stream form) and the eight sessions of the pool
    (the pool form); `batch` launches between one pair of events."""
    from tcow_amd import ops
    m = net.seeker
    g = m.geometry(1, T=1)
    S, D, heads = g['S'], g['D'], g['heads']
    dev = m.vit.pos_embed.device
    out = {}
    n = POOL_SESSIONS
    kc = torch.randn(n, S - 1, heads, T, 64, device=dev).to(torch.bfloat16)
    for name, rows, t0s in [(f'b1_t0_{t0}', 1, [t0]) for t0 in (0, T // 2, T - 1)] + [('pool8', n, [round(k * (T - 1) / (n - 1)) for k in range(n)])]:
        qkv = torch.randn(rows * S, 3 * D, device=dev).to(torch.bfloat16)
        probs = torch.empty(rows, S - 1, heads, T, device=dev)
        t0_rows = torch.tensor(t0s, dtype=torch.int32, device=dev)
        slots = torch.arange(rows, dtype=torch.int32, device=dev)
        if rows == 1:
            call = lambda: ops.attn_temporal_step_probs('stream', ops.BF16, 1, 1, S, D, heads, 1, T, t0_rows, qkv, kc[:1], kc[:1], probs)
        else:
            call = lambda: ops.attn_temporal_step_probs('pool', ops.BF16, rows, 1, S, D, heads, 1, T, n, t0_rows, slots, qkv, kc, kc, probs)
        call()

        def many():
            for _ in range(batch):
                call()
        ms = _mmm([ev_time(many, 1) / batch for _ in range(10)])
        by = kernel_bytes(t0s, S, heads, T, 2, 2)
        out[name] = {'us_per_launch': {k: 1e3 * v for k, v in ms.items()}, 'algorithmic_bytes': by, 'GBps_at_median': by / (ms['median'] * 1e-3) / 1e9,
                     'waves': rows * (S - 1) * heads}
    return out


def maps_legs(reps):
    T, H, W = CONFIGS['configs1']
    net = build(T, H, W, 'bf16')
    rgb, qm = inputs(POOL_SESSIONS, T, H, W)
    f = lambda x, t: x[0:1, :, t:t + 1]
    res = {'config': 'configs1', 'T': T, 'H': H, 'W': W, 'precision': 'bf16', 'reps': reps, 'maps': {k: ('all' if v is None else v) for k, v in MAPS.items()}}
    with torch.no_grad():
        st = net.stream(batch_size=1)
        for t in range(T):
            st.step(f(rgb, t), f(qm, t))
        res['b1'] = {}
        for t0 in (0, T // 2, T - 1):
            def step(t0=t0):
                st.frames_done = t0
                st.step(f(rgb, t0), f(qm, t0))

            def step_maps(t0=t0):
                st.frames_done = t0
                st.step_maps(f(rgb, t0), f(qm, t0), **MAPS)
            r = alternate({'step_ms': step, 'step_maps_ms': step_maps}, reps)
            r['maps_minus_step_ms'] = r['step_maps_ms']['median'] - r['step_ms']['median']
            res['b1'][f't0_{t0}'] = r
        st.frames_done = T - 1
        maps = st.step_maps(f(rgb, T - 1), f(qm, T - 1), **MAPS)[2]
        res['b1']['map_bytes'] = sum(v.numel() * 4 for d in (maps.temporal, maps.spatial) for v in d.values())
        pool, ids, t0s, rgb_a, qm_a, at_t0s = _pool(net, rgb, qm, T)
        r = alternate({'step_ms': lambda: (at_t0s(), pool.step(ids, rgb_a, qm_a)), 'step_maps_ms': lambda: (at_t0s(), pool.step_maps(ids, rgb_a, qm_a, **MAPS))}, reps)
        r['maps_minus_step_ms'] = r['step_maps_ms']['median'] - r['step_ms']['median']
        res['pool8'] = dict(r, t0_rows=t0s)
        res['kernel'] = kernel_alone(net, T)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--plain', action='store_true', help='plain step() legs only (also runs on the parent commit)')
    ap.add_argument('--plain-change', default=None, help='a --plain result of this tree, folded into the full result')
    ap.add_argument('--plain-parent', default=None, help='a --plain result of the parent commit, folded into the full result')
    ap.add_argument('--fold', default=None, help='an existing full result: only fold the --plain runs into it and write --out (no GPU)')
    a = ap.parse_args()
    if a.fold:                                                  # no GPU: fold --plain runs into an existing result
        res = json.load(open(a.fold))
    else:
        assert torch.cuda.is_available(), 'needs a GPU'
        res = plain_legs(a.reps) if a.plain else maps_legs(a.reps)
    if a.plain_change and a.plain_parent:
        # runs of each side (comma lists, taken alternately process by process): a side's figure is the median of its run medians, the parent's
        # spread max - min over all its samples -- and, the narrower reading, over its run medians
        change, parent = ([json.load(open(f)) for f in arg.split(',')] for arg in (a.plain_change, a.plain_parent))
        legs = {}
        for k in ('eager_step_ms', 'graph_step_ms', 'pool8_step_ms'):
            med = lambda runs: sorted(r[k]['median'] for r in runs)
            pm, cm = med(parent), med(change)
            p, c = pm[len(pm) // 2], cm[len(cm) // 2]
            lo, hi = min(r[k]['min'] for r in parent), max(r[k]['max'] for r in parent)
            legs[k] = {'parent_runs': [r[k] for r in parent], 'change_runs': [r[k] for r in change], 'parent_ms': p, 'change_ms': c, 'change_minus_parent_ms': c - p,
                       'parent_samples': [lo, hi], 'parent_run_medians': [pm[0], pm[-1]], 'inside_parent_spread': bool(abs(c - p) <= hi - lo),
                       'inside_parent_run_medians': bool(pm[0] <= c <= pm[-1])}
        res['plain_step_parent_vs_change'] = legs
    if not a.fold:
        res['device'] = torch.cuda.get_device_name(0)
    with open(a.out, 'w') as fo:
        json.dump(res, fo, indent=1)
        fo.write('\n')
    print(json.dumps(res)[:2000])


if __name__ == '__main__':
    main()

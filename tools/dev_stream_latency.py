"""Dev: latency of streaming inference (Seeker.stream, tcow_amd/stream.py) against the clip forward, on the GPU.

    python tools/dev_stream_latency.py --out profiles/stream_latency.json       # step latencies, whole-clip sums, clip forwards (one JSON file)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/dev_stream_latency.py --kprof
                                        # one-frame bf16 steps at configs[3], t0 = 59: KPROF_WARMUP warm-up steps, then KPROF_STEPS profiled ones
    python tools/dev_stream_latency.py --kstats DIR/run_kernel_trace.csv --out profiles/stream_step_kernel_stats.txt
                                        # per-step kernel breakdown of the profiled steps only (the warm-up steps' dispatches are dropped)
    python tools/dev_stream_latency.py --pool --out profiles/stream_pool_latency.json
                                        # eight live sessions at configs[1]: one pool step at eight different t0 against the in-phase B = 8 stream
                                        # step and against eight one-session steps, the three legs alternating in one run
    python tools/dev_stream_latency.py --ragged --out profiles/stream_ragged_latency.json
                                        # the same eight sessions with chunk lengths 1, 1, 1, 1, 2, 2, 4, 8 in one tick: one step_ragged against one
                                        # pool.step per distinct length, and step_ragged with every length 1 against pool.step
    python tools/dev_stream_latency.py --skinny --out profiles/stream_skinny_latency.json
                                        # one-frame steps at t0 = T - 1 with skinny_gemm=True against skinny_gemm=False (the code as it was before the
                                        # keyword existed), alternating in one run: configs[1] B = 1 and B = 8, configs[3] B = 1, eager and graph
    python tools/dev_stream_latency.py --skinny --precision bf16x3 --reps 30 --out profiles/stream_skinny_x3_latency.json
                                        # the same legs in precision='bf16x3' (ops.gemm_nt_skinny_x3 against tcow_gemm_nt with TCOW_F32X3)
    --kprof / --kstats take --precision and --skinny-gemm on|off as well: the breakdown of a bf16x3 step with and without the flag
    python tools/dev_stream_latency.py --cache-dtype fp8 --out lat_bf16.json
    python tools/dev_stream_latency.py --cache-dtype bf16,fp8 --precision fp32 --out lat_fp32.json
                                        # one-frame steps with cache_dtype=None against the listed compact caches, the legs alternating in one run:
                                        # configs[1] B = 1 and B = 8, configs[3] B = 1 at t0 = 0, T/2, T-1, and a long stream (configs[1] geometry,
                                        # num_total_frames = 240) at t0 = 239; the two files' runs are the 'latency' list of profiles/stream_cache_dtype.json
    --kprof / --kstats take one --cache-dtype as well (the temporal kernel's own time and bytes with a compact cache)
    python tools/dev_stream_latency.py --rollover 10 --out profiles/stream_rollover_latency.json
                                        # one session of a rollover pool (stream_pool(2, rollover=K)) at configs[1], B = 1, bf16, one frame per call over
                                        # three windows: plain, overlap and hand-off ticks, each followed by the one-frame step of a pool without the
                                        # keyword at the same local frame; and the re-query launch alone at the configs[1] / configs[3] plane sizes

Times are device events around each call after warm-up, profiler off.  A step at a given t0 is timed by setting the stream's host frame counter
(the kernels then read t0 from the device scalar the step writes): the work of a step depends on t0, not on what the cache holds.  Synthetic
weights / clips (tcow_amd.synth); depth 12 ViT-B; one query per clip.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcow_amd import synth                      # noqa: E402
from tcow_amd.seeker import Seeker              # noqa: E402

CONFIGS = {'configs1': (30, 240, 320), 'configs3': (60, 480, 640)}


def build(T, H, W, precision):
    cfg = synth.seeker_config(num_total_frames=T, frame_height=H, frame_width=W, causal_attention=1)
    net = Seeker(None, num_total_frames=T, frame_height=H, frame_width=W, causal_attention=1, drop_path_rate=0.0, precision=precision)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, 900).items()})
    return net.cuda().eval()


def inputs(B, T, H, W):
    clip = synth.make_clip(1, T, H, W, seed=900)
    rgb = torch.from_numpy(clip['rgb']).cuda().expand(B, -1, -1, -1, -1).contiguous()
    qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda().expand(B, -1, -1, -1, -1).contiguous()
    return rgb, qm


def ev_time(fn, reps):
    """Median device time (ms) of fn() over `reps` calls, each bracketed by events on the current stream."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2]


def measure(name, B, precision, reps):
    T, H, W = CONFIGS[name]
    net = build(T, H, W, precision)
    rgb, qm = inputs(B, T, H, W)
    res = {'config': name, 'T': T, 'H': H, 'W': W, 'B': B, 'precision': precision}
    with torch.no_grad():
        for _ in range(3):
            net(rgb, qm)
        res['clip_forward_ms'] = ev_time(lambda: net(rgb, qm), reps)
        for graph in (False, True):
            st = net.stream(batch_size=B, graph=graph)
            tag = 'graph' if graph else 'eager'
            for t in range(T):                                    # warm-up: the whole clip once (captures the c = 1 graph)
                st.step(rgb[:, :, t:t + 1], qm[:, :, t:t + 1])
            lat = {}
            for t0 in (0, T // 2, T - 1):
                def one(t0=t0):
                    st.frames_done = t0
                    st.step(rgb[:, :, t0:t0 + 1], qm[:, :, t0:t0 + 1])
                one()
                lat[str(t0)] = ev_time(one, reps)
            res[f'{tag}_step_ms'] = lat

            def whole():
                st.reset()
                for t in range(T):
                    st.step(rgb[:, :, t:t + 1], qm[:, :, t:t + 1])
            res[f'{tag}_clip_sum_ms'] = ev_time(whole, max(3, reps // 5))
        res['cache_bytes'] = st.cache_bytes
        del st
    del net
    torch.cuda.empty_cache()
    return res


POOL_SESSIONS = 8


def pool_leg(reps):
    """Eight sessions at configs[1], bf16, one-frame steps, the three legs taken in turn `reps` times (so drift of the machine hits all alike):
    (a) one SeekerStreamPool step with t0 spread evenly over 0 .. T-1, (b) the in-phase batch_size = 8 SeekerStream step at t0 = T-1 (it reads
    at least as much cache as (a)), (c) eight one-session SeekerStream steps at the eight t0 of (a), one after the other.  The spread (b) is
    judged against is max - min of (b)'s own samples in this run."""
    name, n = 'configs1', POOL_SESSIONS
    T, H, W = CONFIGS[name]
    net = build(T, H, W, 'bf16')
    rgb, qm = inputs(n, T, H, W)
    t0s = [round(k * (T - 1) / (n - 1)) for k in range(n)]
    f = lambda x, t0: x[:, :, t0:t0 + 1]
    with torch.no_grad():
        pool = net.stream_pool(n)
        ids = [pool.open() for _ in range(n)]
        inphase = net.stream(batch_size=n)
        single = net.stream(batch_size=1)
        for t in range(T):                                    # warm-up: the whole clip once through each (fills every cache row)
            pool.step(ids, f(rgb, t), f(qm, t))
            inphase.step(f(rgb, t), f(qm, t))
            single.step(f(rgb[0:1], t), f(qm[0:1], t))
        rgb_a = torch.cat([f(rgb[k:k + 1], t0) for k, t0 in enumerate(t0s)], 0)
        qm_a = torch.cat([f(qm[k:k + 1], t0) for k, t0 in enumerate(t0s)], 0)

        def leg_a():
            for sid, t0 in zip(ids, t0s):
                pool._done[sid] = t0                         # (the step's work depends on t0, not on what the cache holds)
            pool.step(ids, rgb_a, qm_a)

        def leg_b():
            inphase.frames_done = T - 1
            inphase.step(f(rgb, T - 1), f(qm, T - 1))

        def leg_c():
            for t0 in t0s:
                single.frames_done = t0
                single.step(f(rgb[0:1], t0), f(qm[0:1], t0))

        legs = {'a_pool_step_ms': leg_a, 'b_inphase_b8_step_ms': leg_b, 'c_eight_single_steps_ms': leg_c}
        samples = {k: [] for k in legs}
        for fn in legs.values():
            for _ in range(3):
                fn()
        for _ in range(reps):
            for k, fn in legs.items():
                samples[k].append(ev_time(fn, 1))
    res = {'config': name, 'T': T, 'H': H, 'W': W, 'sessions': n, 'precision': 'bf16', 'reps': reps, 't0_rows': t0s, 'pool_cache_bytes': pool.cache_bytes}
    for k, v in samples.items():
        v = sorted(v)
        res[k] = {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}
    a, b, c = (res[k]['median'] for k in legs)
    spread = res['b_inphase_b8_step_ms']['max'] - res['b_inphase_b8_step_ms']['min']
    res.update(b_spread_ms=spread, a_minus_b_ms=a - b, a_within_b_plus_spread=bool(a <= b + spread), a_over_c=a / c)
    return res


RAGGED_CHUNKS = [1, 1, 1, 1, 2, 2, 4, 8]


def ragged_leg(reps):
    """Eight sessions at configs[1], bf16, at the spread t0 of pool_leg, the four legs taken in turn `reps` times: (a) one step_ragged with chunk
    lengths RAGGED_CHUNKS (a t0 is moved back where t0 + c would pass the last frame), (b) the same tick as one pool.step per distinct chunk
    length (four calls), (c) one step_ragged with every chunk length 1, (d) pool.step on the same eight sessions.  Spreads are max - min of a
    leg's own samples in this run."""
    name, n = 'configs1', POOL_SESSIONS
    T, H, W = CONFIGS[name]
    net = build(T, H, W, 'bf16')
    rgb, qm = inputs(n, T, H, W)
    t0s = [round(k * (T - 1) / (n - 1)) for k in range(n)]
    cs = RAGGED_CHUNKS
    t0s_a = [min(t0, T - c) for t0, c in zip(t0s, cs)]
    f = lambda x, t0, c=1: x[:, :, t0:t0 + c]
    with torch.no_grad():
        pool = net.stream_pool(n)
        ids = [pool.open() for _ in range(n)]
        for t in range(T):                                    # warm-up: the whole clip once (fills every cache row)
            pool.step(ids, f(rgb, t), f(qm, t))
        rgbs_a = [f(rgb[k:k + 1], t0, c).contiguous() for k, (t0, c) in enumerate(zip(t0s_a, cs))]
        qms_a = [f(qm[k:k + 1], t0, c).contiguous() for k, (t0, c) in enumerate(zip(t0s_a, cs))]
        groups = [(c, [k for k in range(n) if cs[k] == c]) for c in sorted(set(cs))]
        rgb_b = [torch.cat([rgbs_a[k] for k in ks], 0) for _, ks in groups]
        qm_b = [torch.cat([qms_a[k] for k in ks], 0) for _, ks in groups]
        rgbs_c = [f(rgb[k:k + 1], t0).contiguous() for k, t0 in enumerate(t0s)]
        qms_c = [f(qm[k:k + 1], t0).contiguous() for k, t0 in enumerate(t0s)]
        rgb_d, qm_d = torch.cat(rgbs_c, 0), torch.cat(qms_c, 0)

        def at(t0_list):
            for sid, t0 in zip(ids, t0_list):
                pool._done[sid] = t0                         # (the step's work depends on t0, not on what the cache holds)

        def leg_a():
            at(t0s_a)
            pool.step_ragged(ids, rgbs_a, qms_a)

        def leg_b():
            at(t0s_a)
            for (c, ks), r, q in zip(groups, rgb_b, qm_b):
                pool.step([ids[k] for k in ks], r, q)

        def leg_c():
            at(t0s)
            pool.step_ragged(ids, rgbs_c, qms_c)

        def leg_d():
            at(t0s)
            pool.step(ids, rgb_d, qm_d)

        legs = {'a_ragged_step_ms': leg_a, 'b_pool_step_per_length_ms': leg_b, 'c_ragged_step_all_one_ms': leg_c, 'd_pool_step_ms': leg_d}
        samples = {k: [] for k in legs}
        for fn in legs.values():
            for _ in range(3):
                fn()
        for _ in range(reps):
            for k, fn in legs.items():
                samples[k].append(ev_time(fn, 1))
    res = {'config': name, 'T': T, 'H': H, 'W': W, 'sessions': n, 'precision': 'bf16', 'reps': reps, 'chunk_lengths': cs, 't0_rows_a_b': t0s_a,
           't0_rows_c_d': t0s, 'pool_steps_in_b': len(groups)}
    for k, v in samples.items():
        v = sorted(v)
        res[k] = {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}
    a, b, c, d = (res[k]['median'] for k in legs)
    b_spread = res['b_pool_step_per_length_ms']['max'] - res['b_pool_step_per_length_ms']['min']
    d_spread = res['d_pool_step_ms']['max'] - res['d_pool_step_ms']['min']
    res.update(b_spread_ms=b_spread, b_minus_a_ms=b - a, a_below_b_by_more_than_b_spread=bool(b - a > b_spread), a_over_b=a / b,
               d_spread_ms=d_spread, c_minus_d_ms=c - d, c_not_above_d_by_more_than_d_spread=bool(c - d <= d_spread))
    return res


def skinny_leg(reps, precision='bf16'):
    """One-frame steps (bf16, or `precision`) at t0 = T - 1, skinny_gemm on / off, eager and graph: the four streams of a config are stepped in turn `reps` times, one
    sample (one step between a pair of events) each per round.  The verdict of DESIGN.md section 9: the eager medians at configs[1] B = 1 and
    configs[3] B = 1 are lower with the flag by more than the off-leg's own max - min, and the B = 8 leg is not slower by more than that spread."""
    runs = []
    for name, B in (('configs1', 1), ('configs1', 8), ('configs3', 1)):
        T, H, W = CONFIGS[name]
        net = build(T, H, W, precision)
        rgb, qm = inputs(B, T, H, W)
        f = lambda x, t: x[:, :, t:t + 1]
        with torch.no_grad():
            legs = {}
            for graph in (False, True):
                for flag in (False, True):
                    st = net.stream(batch_size=B, graph=graph, skinny_gemm=flag)
                    for t in (0, T - 1, T - 1, T - 1):          # warm-up: operand copies, the c = 1 graph, the workspace
                        st.frames_done = t
                        st.step(f(rgb, t), f(qm, t))

                    def one(st=st):
                        st.frames_done = T - 1
                        st.step(f(rgb, T - 1), f(qm, T - 1))
                    legs[f"{'graph' if graph else 'eager'}_{'on' if flag else 'off'}"] = one
            samples = {k: [] for k in legs}
            for _ in range(reps):
                for k, fn in legs.items():
                    samples[k].append(ev_time(fn, 1))
        r = {'config': name, 'T': T, 'H': H, 'W': W, 'B': B, 'precision': precision, 't0': T - 1, 'reps': reps}
        for k, v in samples.items():
            v = sorted(v)
            r[k + '_step_ms'] = {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}
        for mode in ('eager', 'graph'):
            off, on = r[mode + '_off_step_ms'], r[mode + '_on_step_ms']
            r[mode + '_off_spread_ms'] = off['max'] - off['min']
            r[mode + '_off_minus_on_ms'] = off['median'] - on['median']
            r[mode + '_on_lower_by_more_than_off_spread'] = bool(off['median'] - on['median'] > off['max'] - off['min'])
            r[mode + '_on_not_slower_by_more_than_off_spread'] = bool(on['median'] - off['median'] <= off['max'] - off['min'])
        runs.append(r)
        del legs, net
        torch.cuda.empty_cache()
    by = {(r['config'], r['B']): r for r in runs}
    verdict = bool(by[('configs1', 1)]['eager_on_lower_by_more_than_off_spread'] and by[('configs3', 1)]['eager_on_lower_by_more_than_off_spread']
                   and by[('configs1', 8)]['eager_on_not_slower_by_more_than_off_spread'])
    return {'runs': runs, 'verdict_default_true': verdict}


LONG_T = 240


def cache_leg(reps, precision, keywords, only=None):
    """One-frame eager steps with cache_dtype=None and each of `keywords`, the streams of a shape stepped in turn `reps` times (one sample, one
    step between a pair of events, each per round) at every t0: median, min, max per leg and t0, and None's median minus the leg's next to None's
    own max - min.  The long stream has configs[1]'s frame size and LONG_T frames; its steps are fed the clip's first frame (the work of a step
    depends on t0 alone)."""
    runs = []
    shapes = [('configs1', 1, None), ('configs1', 8, None), ('configs3', 1, None), ('configs1', 1, LONG_T)]
    for name, B, T_long in shapes:
        tag = f'{name}_b{B}' + ('_long' if T_long else '')
        if only and tag not in only:
            continue
        T, H, W = CONFIGS[name]
        rgb, qm = inputs(B, 2 if T_long else T, H, W)
        T = T_long or T
        net = build(T, H, W, precision)
        frame = (lambda x, t: x[:, :, 0:1]) if T_long else (lambda x, t: x[:, :, t:t + 1])
        t0s = [T - 1] if T_long else [0, T // 2, T - 1]
        r = {'shape': tag, 'config': name, 'T': T, 'H': H, 'W': W, 'B': B, 'precision': precision, 'reps': reps, 'cache_bytes': {}, 'step_ms': {}}
        with torch.no_grad():
            streams = {}
            for kw in [None] + list(keywords):
                st = streams[str(kw)] = net.stream(batch_size=B, cache_dtype=kw)
                r['cache_bytes'][str(kw)] = st.cache_bytes
                for t in (0, T - 1, T - 1):                     # warm-up: operand copies, the workspace
                    st.frames_done = t
                    st.step(frame(rgb, t), frame(qm, t))
            for t0 in t0s:
                samples = {k: [] for k in streams}

                def one(st, t0=t0):
                    st.frames_done = t0
                    st.step(frame(rgb, t0), frame(qm, t0))
                for st in streams.values():
                    one(st)
                for _ in range(reps):
                    for k, st in streams.items():
                        samples[k].append(ev_time(lambda: one(st), 1))
                row = {}
                for k, v in samples.items():
                    v = sorted(v)
                    row[k] = {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}
                base = row['None']
                for k in row:
                    if k != 'None':
                        row[k]['none_minus_this_ms'] = base['median'] - row[k]['median']
                        row[k]['lower_by_more_than_none_spread'] = bool(base['median'] - row[k]['median'] > base['max'] - base['min'])
                r['step_ms'][str(t0)] = row
        print(json.dumps(r), flush=True)
        runs.append(r)
        del streams, net
        torch.cuda.empty_cache()
    return runs


KPROF_WARMUP, KPROF_STEPS = 3, 20
STEP_LAST_KERNEL = 'flags_fwd_kernel'      # the last launch of every step (the flags head, engine.run_forward)


def _mmm(v):
    v = sorted(v)
    return {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1], 'samples': len(v)}


def rollover_leg(reps, k):
    """One session of net.stream_pool(2, rollover=k) at configs[1], bf16, fed one frame per call over three windows (2 * (T - k) + T frames), `reps`
    times.  Every tick is followed by the tick the code took before the keyword existed: the one-frame step of a pool opened without it, one
    session, at the local frame of the window that reports the tick -- so the two legs alternate tick by tick and drift hits both alike.  Ticks by
    kind: 'plain' (one window live: one frame-row), 'overlap' (two windows live; the tick after a hand-off frame also carries the retained frame),
    'handoff' (the tick of a hand-off frame: the re-query launch and the copy of the retained frame ride on it).  Also the re-query launch alone,
    one plane per launch, at the plane sizes of configs[1] and configs[3]."""
    from tcow_amd import ops
    name = 'configs1'
    T, H, W = CONFIGS[name]
    s, frames = T - k, 2 * (T - k) + T
    net = build(T, H, W, 'bf16')
    rgb, qm = inputs(1, T, H, W)
    f = lambda x, g: x[:, :, g % T:g % T + 1]
    with torch.no_grad():
        roll = net.stream_pool(2, rollover=k)
        sid = roll.open()
        old = net.stream_pool(1)
        oid = old.open()
        plan = roll.plan
        kinds, rows = [], []
        for g in range(frames):
            sp = plan.split(g, 1)
            kinds.append('handoff' if sp['handoff'] is not None else 'overlap' if len(sp['parts'][0]) == 2 else 'plain')
            rows.append(sum(r[2] for r in sp['parts'][0]))

        def tick(g):
            roll.step([sid], f(rgb, g), f(qm, g))

        def old_tick(g):
            old._done[oid] = g - plan.window(g) * s         # (the step's work depends on t0, not on what the cache holds)
            old.step([oid], f(rgb, g), f(qm, g))

        for g in range(frames):                             # warm-up: the three windows once through each
            tick(g); old_tick(g)
        samples = {leg: {kd: [] for kd in ('plain', 'overlap', 'handoff')} for leg in ('rollover_ms', 'without_keyword_ms')}
        for _ in range(reps):
            roll.reset(sid)
            for g in range(frames):
                samples['rollover_ms'][kinds[g]].append(ev_time(lambda: tick(g), 1))
                samples['without_keyword_ms'][kinds[g]].append(ev_time(lambda: old_tick(g), 1))
        res = {'config': name, 'T': T, 'H': H, 'W': W, 'B': 1, 'precision': 'bf16', 'rollover': k, 'frames_per_round': frames, 'rounds': reps,
               'ticks_per_round': {kd: kinds.count(kd) for kd in ('plain', 'overlap', 'handoff')},
               'frame_rows_per_tick': {kd: sorted({r for r, q in zip(rows, kinds) if q == kd}) for kd in ('plain', 'overlap', 'handoff')},
               'mean_frame_rows_per_frame': sum(rows[T:]) / len(rows[T:]), 'cache_bytes': roll.cache_bytes}
        for leg, by in samples.items():
            res[leg] = {kd: _mmm(v) for kd, v in by.items() if v}
        sp = res['without_keyword_ms']['plain']
        res['plain_inside_parent_spread'] = bool(sp['min'] <= res['rollover_ms']['plain']['median'] <= sp['max'])
        res['requery_launch_us'] = {}
        for cfg, (_, h, w) in CONFIGS.items():
            plane, n = h * w, 50
            logits = torch.randn(3 * plane, device='cuda')
            mask = torch.zeros(2, plane, device='cuda'); pixels = torch.zeros(2, dtype=torch.int32, device='cuda')
            src = torch.tensor([plane], dtype=torch.int64, device='cuda'); dst = torch.tensor([1], dtype=torch.int32, device='cuda')

            def many():
                for _ in range(n):
                    ops.requery_mask(logits, src, 0.0, mask, dst, pixels)
            many()
            res['requery_launch_us'][cfg] = {'plane': plane, **{q: v * 1e3 / n for q, v in _mmm([ev_time(many, 1) for _ in range(reps)]).items() if q != 'samples'}}
    return res


def cached_kernel_bytes(T, H, W, e=2, heads=12, D=768, ce=None):
    """Algorithmic bytes of one tcow_attn_temporal_step launch (the stream form) of a one-frame step at t0 = T - 1 (B = 1, element size e, cache element
    size ce: e unless the cache is compact)."""
    S, t0 = (H // 16) * (W // 16) + 1, T - 1
    ce = e if ce is None else ce
    alg = {'cache_read': (S - 1) * heads * t0 * 64 * 2 * ce, 'chunk_qkv_read': S * 3 * D * e, 'out_write': S * D * e,
           'cache_append': (S - 1) * heads * 64 * 2 * ce}
    alg['total'] = sum(alg.values())
    return alg


def kprof(precision='bf16', skinny_gemm=None, cache_dtype=None):
    """One-frame steps (bf16, or `precision`) at configs[3], t0 = 59, for a rocprofv3 kernel trace: KPROF_WARMUP steps that build the operand
    copies, then KPROF_STEPS steady ones (--kstats keeps only those)."""
    T, H, W = CONFIGS['configs3']
    net = build(T, H, W, precision)
    rgb, qm = inputs(1, T, H, W)
    with torch.no_grad():
        st = net.stream(batch_size=1, graph=False, skinny_gemm=skinny_gemm, cache_dtype=cache_dtype)
        for _ in range(KPROF_WARMUP + KPROF_STEPS):
            st.frames_done = T - 1
            st.step(rgb[:, :, T - 1:T], qm[:, :, T - 1:T])
        torch.cuda.synchronize()


def kstats(trace_csv, out, precision='bf16', skinny_gemm=None, cache_dtype=None):
    """Per-step kernel breakdown of the KPROF_STEPS profiled steps from rocprofv3's kernel-trace CSV: dispatches in start order, everything up to
    and including the KPROF_WARMUP-th STEP_LAST_KERNEL dropped, per-kernel totals divided by KPROF_STEPS."""
    import csv
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    ends = [i for i, r in enumerate(rows) if STEP_LAST_KERNEL in r['Kernel_Name']]
    assert len(ends) == KPROF_WARMUP + KPROF_STEPS, f'{len(ends)} steps in the trace, expected {KPROF_WARMUP + KPROF_STEPS}'
    rows = rows[ends[KPROF_WARMUP - 1] + 1:]
    per = {}
    for r in rows:
        d = int(r['End_Timestamp']) - int(r['Start_Timestamp'])
        n, tot, mn = per.get(r['Kernel_Name'], (0, 0, None))
        per[r['Kernel_Name']] = (n + 1, tot + d, d if mn is None else min(mn, d))
    T, H, W = CONFIGS['configs3']
    alg = cached_kernel_bytes(T, H, W, e=2 if precision in ('bf16', 'fp16') else 4, ce={None: None, 'bf16': 2, 'fp8': 1}[cache_dtype])
    flag = ('' if skinny_gemm is None else f", skinny_gemm={'on' if skinny_gemm else 'off'}") + ('' if cache_dtype is None else f', cache_dtype={cache_dtype}')
    lines = [f'# {KPROF_STEPS} one-frame {precision} stream steps at BASELINE configs[3] (T=60, 480x640, B=1), t0 = 59{flag}, after {KPROF_WARMUP} warm-up steps',
             '# (rocprofv3 --kernel-trace; tools/dev_stream_latency.py --kprof, then --kstats on the kernel-trace CSV: the warm-up dispatches are dropped)',
             '#   us/step  launches/step   avg us   min us  kernel']
    total = 0
    for name, (n, tot, mn) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        total += tot
        lines.append(f'{tot / KPROF_STEPS / 1e3:10.1f}  {n / KPROF_STEPS:13.1f} {tot / n / 1e3:8.1f} {mn / 1e3:8.1f}  {name[:110]}')
    lines.append(f'total kernel time per step: {total / KPROF_STEPS / 1e3:.1f} us')
    ck = [(n, tot) for name, (n, tot, _) in per.items() if 'temporal_cached_kernel' in name]
    if ck:
        avg = ck[0][1] / ck[0][0] / 1e9
        lines.append('temporal_cached_kernel algorithmic bytes per launch: ' + ', '.join(f'{k} {v}' for k, v in alg.items()))
        lines.append(f'-> {alg["total"] / avg / 1e12:.2f} TB/s at the {avg * 1e6:.1f} us average = {alg["total"] / avg / 8e12:.2f} of the 8 TB/s HBM peak')
    txt = '\n'.join(lines) + '\n'
    print(txt)
    if out:
        with open(out, 'w') as f:
            f.write(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--kprof', action='store_true')
    ap.add_argument('--pool', action='store_true', help='the stream-pool leg (eight sessions at configs1)')
    ap.add_argument('--ragged', action='store_true', help='the ragged-step leg (eight sessions at configs1, chunk lengths 1, 1, 1, 1, 2, 2, 4, 8)')
    ap.add_argument('--skinny', action='store_true', help='skinny_gemm=True against False, one-frame steps at configs1 B = 1 / 8 and configs3 B = 1')
    ap.add_argument('--kstats', default=None, metavar='KERNEL_TRACE_CSV')
    ap.add_argument('--precision', default='bf16', help="precision of the --skinny, --kprof and --kstats legs ('bf16' or 'bf16x3')")
    ap.add_argument('--skinny-gemm', default=None, choices=['on', 'off'], help='the skinny_gemm keyword of the --kprof steps (default: the stream default)')
    ap.add_argument('--cache-dtype', default=None, help="comma list of 'bf16' / 'fp8': the compact-cache leg against cache_dtype=None; one value with "
                                                        '--kprof / --kstats')
    ap.add_argument('--rollover', type=int, default=None, metavar='K', help='the rollover-pool leg: one session at configs1 over three windows that overlap by K')
    ap.add_argument('--only', default=None, help='comma list of configs1_b1, configs1_b8, configs3_b1 (--cache-dtype: also configs1_b1_long)')
    a = ap.parse_args()
    flag = None if a.skinny_gemm is None else a.skinny_gemm == 'on'
    if a.kstats:
        kstats(a.kstats, a.out, a.precision, flag, a.cache_dtype)
        return
    if not torch.cuda.is_available():
        raise SystemExit('dev_stream_latency.py needs a GPU')
    if a.kprof:
        kprof(a.precision, flag, a.cache_dtype)
        return
    if a.cache_dtype:
        out = {'device': torch.cuda.get_device_name(0),
               'cache_dtype': cache_leg(a.reps, a.precision, a.cache_dtype.split(','), set(a.only.split(',')) if a.only else None)}
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                json.dump(out, f, indent=1)
        return
    if a.rollover is not None:
        out = {'device': torch.cuda.get_device_name(0), 'rollover': rollover_leg(a.reps, a.rollover)}
        print(json.dumps(out['rollover']), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                json.dump(out, f, indent=1)
        return
    if a.pool:
        out = {'device': torch.cuda.get_device_name(0), 'pool': pool_leg(a.reps)}
        print(json.dumps(out['pool']), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                json.dump(out, f, indent=1)
        return
    if a.ragged:
        out = {'device': torch.cuda.get_device_name(0), 'ragged': ragged_leg(a.reps)}
        print(json.dumps(out['ragged']), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                json.dump(out, f, indent=1)
        return
    if a.skinny:
        out = {'device': torch.cuda.get_device_name(0), 'skinny': skinny_leg(a.reps, a.precision)}
        print(json.dumps(out['skinny']), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                json.dump(out, f, indent=1)
        return
    runs = [('configs1', 1), ('configs1', 8), ('configs3', 1)]
    if a.only:
        keep = set(a.only.split(','))
        runs = [r for r in runs if f'{r[0]}_b{r[1]}' in keep]
    out = {'device': torch.cuda.get_device_name(0), 'runs': []}
    for name, B in runs:
        r = measure(name, B, 'bf16', a.reps)
        print(json.dumps(r), flush=True)
        out['runs'].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()

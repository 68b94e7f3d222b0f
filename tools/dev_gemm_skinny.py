"""Dev: the skinny-M NT GEMM (ops.gemm_nt_skinny) against tcow_gemm_nt as routed today, at the shapes of a one-frame stream step, on the GPU.

    python tools/dev_gemm_skinny.py --out profiles/gemm_skinny.json

Shapes: the four weight shapes of a ViT-B block with the epilogue the forward issues for each (qkv: bias, 16-bit output; proj / temporal fc: bias +
f32 residual; fc1: bias + GELU; fc2: bias + f32 residual) at M = 301 (configs[1], B = 1), 1 201 (configs[3], B = 1) and 2 408 (configs[1], B = 8).
Legs: tcow_gemm_nt (tile = 0), and the skinny entry point at S in {1, 2, 3, 4, 6, 8}.  All legs of a shape alternate in one process for
--rounds rounds after warm-up; one sample is --batch launches between one pair of device events (a window of milliseconds), reported per launch.
The launches of a batch walk over WEIGHT_COPIES copies of W, as the blocks of a step do: no launch finds its weights in the L2 the one before
left them in.

Per shape the JSON states what the measurement asks of ops.skinny_plan: 'route' = the best split's median is below today's by more than
today's own max - min; 'accept' = the splits whose median lies within the best one's max - min of it; 'plan' = what the committed rule returns.
tests/test_gemm_skinny_host.py::test_plan_reproduces_the_measured_table holds the rule to it.

    python tools/dev_gemm_skinny.py --x3 --out profiles/gemm_skinny_x3.json

--x3: the same harness for precision='bf16x3' -- f32 operands and outputs, tcow_gemm_nt with TCOW_F32X3 against ops.gemm_nt_skinny_x3, the rule
ops.skinny_plan_x3 (tests/test_gemm_skinny_host.py::test_plan_x3_reproduces_the_measured_table).

    python tools/dev_gemm_skinny.py --x3 --rows 14,30 --out profiles/gemm_skinny_x3_small.json

--rows: other row counts than the three above (the steps of small nets: one 64-row tile per column of tiles).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcow_amd import ops                        # noqa: E402

WEIGHTS = [('qkv', 2304, 768), ('proj', 768, 768), ('fc1', 3072, 768), ('fc2', 768, 3072)]
ROWS = [301, 1201, 2408]
SPLITS = [1, 2, 3, 4, 6, 8]
WEIGHT_COPIES = 12


def make(name, M, N, K, x3=False):
    g = torch.Generator(device='cuda').manual_seed(M + N + K)
    bf = torch.float32 if x3 else torch.bfloat16
    A = torch.randn(M, K, device='cuda', generator=g).to(bf)
    Ws = [(torch.randn(N, K, device='cuda', generator=g) * 0.05).to(bf) for _ in range(WEIGHT_COPIES)]
    bias = torch.randn(N, device='cuda', generator=g)
    if name in ('proj', 'fc2'):
        out, kw = torch.empty(M, N, device='cuda'), dict(bias=bias, resid=torch.randn(M, N, device='cuda', generator=g))
    elif name == 'fc1':
        out, kw = torch.empty(M, N, device='cuda', dtype=bf), dict(bias=bias, act=ops.ACT_GELU)
    else:
        out, kw = torch.empty(M, N, device='cuda', dtype=bf), dict(bias=bias)
    return A, Ws, out, kw


def sample(fn, Ws, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(batch):
        fn(Ws[i % len(Ws)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / batch          # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--batch', type=int, default=120)
    ap.add_argument('--x3', action='store_true', help="the bf16 x 3 leg: f32 tensors, TCOW_F32X3 against ops.gemm_nt_skinny_x3")
    ap.add_argument('--rows', default=None, help="comma-separated row counts M instead of 301,1201,2408")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dev_gemm_skinny.py needs a GPU')
    shapes = []
    for name, N, K in WEIGHTS:
        for M in ([int(m) for m in a.rows.split(',')] if a.rows else ROWS):
            A, Ws, out, kw = make(name, M, N, K, a.x3)
            mode = ops.F32X3 if a.x3 else ops.BF16
            legs = {'nt': lambda W: ops.gemm_nt(mode, A, W, out, **kw)}
            for S in SPLITS:
                if S <= K // 64:
                    legs[f'S{S}'] = (lambda W, S=S: ops.gemm_nt_skinny_x3(A, W, out, split=S, **kw)) if a.x3 else (lambda W, S=S: ops.gemm_nt_skinny(ops.BF16, A, W, out, split=S, **kw))
            # the legs agree on the product before they are timed
            want = ops.gemm_nt(mode, A, Ws[0], torch.empty_like(out), **kw).float()
            for k, fn in legs.items():
                err = float((fn(Ws[0]).float() - want).abs().max() / want.abs().max())
                assert err < 1e-2, (name, M, k, err)
            for fn in legs.values():
                sample(fn, Ws, a.batch)
            samples = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, fn in legs.items():
                    samples[k].append(sample(fn, Ws, a.batch))
            r = {'name': name, 'M': M, 'N': N, 'K': K, 'tiles_128': -(-M // 128) * -(-N // 128), 'tiles_64': -(-M // 64) * -(-N // 64), 'legs_us': {}}
            for k, v in samples.items():
                v = sorted(v)
                r['legs_us'][k] = {'median': round(v[len(v) // 2], 3), 'min': round(v[0], 3), 'max': round(v[-1], 3)}
            nt = r['legs_us']['nt']
            sk = {int(k[1:]): v for k, v in r['legs_us'].items() if k != 'nt'}
            best = min(sk, key=lambda s: sk[s]['median'])
            r['best_split'] = best
            r['nt_spread_us'] = round(nt['max'] - nt['min'], 3)
            r['route'] = bool(nt['median'] - sk[best]['median'] > nt['max'] - nt['min'])
            r['accept'] = sorted(s for s in sk if sk[s]['median'] - sk[best]['median'] <= sk[best]['max'] - sk[best]['min'])
            r['plan'] = (ops.skinny_plan_x3 if a.x3 else ops.skinny_plan)(M, N, K)
            r['plan_ok'] = bool(r['plan'] in r['accept'] if r['route'] else r['plan'] == 0)
            print(json.dumps(r), flush=True)
            shapes.append(r)
            del A, Ws, out, kw, legs
    res = {'device': torch.cuda.get_device_name(0), 'rounds': a.rounds, 'batch': a.batch, 'weight_copies': WEIGHT_COPIES,
           'shapes': shapes}
    if a.x3:
        res['mode'] = 'bf16x3'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

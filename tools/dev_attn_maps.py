"""Dev: what Seeker.attention_maps costs, at BASELINE configs[1] (T = 30, 240 x 320) and configs[3] (T = 60, 480 x 640), B = 1, precision 'bf16'.

    python tools/dev_attn_maps.py --out profiles/attention_maps.json

Two measurements per geometry, timed with device events, the legs alternating in one process after warm-up:

  * forward() against attention_maps() with all 12 blocks, temporal maps on and the 'cls' spatial queries (eval, no_grad);
  * the two kernels of tcow_attn_probs alone, --batch launches between one pair of events, each on the next of COPIES sets of buffers: us per
    launch and achieved bytes/s over the algorithmic bytes -- the K and Q columns of the rows the sequences cover read once, plus the output.

No pass mark: nobody had measured these kernels.  The numbers say whether the write stream runs near LayerNorm's rate or not.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcow_amd import ops                        # noqa: E402
from tcow_amd.seeker import Seeker              # noqa: E402

GEOMETRIES = {'configs[1]': dict(T=30, H=240, W=320), 'configs[3]': dict(T=60, H=480, W=640)}
P, D, HEADS, CA = 16, 768, 12, 1
COPIES = 3


def stats(v):
    v = sorted(v)
    return {'median': round(v[len(v) // 2], 3), 'min': round(v[0], 3), 'max': round(v[-1], 3)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)                     # ms


def module_legs(geo, rounds, warmup):
    """ms of forward() and of attention_maps(all blocks, temporal, 'cls')."""
    T, H, W = geo['T'], geo['H'], geo['W']
    torch.manual_seed(0)
    net = Seeker(None, num_total_frames=T, frame_height=H, frame_width=W, causal_attention=CA, drop_path_rate=0.0, precision='bf16').cuda().eval()
    rgb = torch.rand(1, 3, T, H, W, device='cuda')
    qm = torch.zeros(1, 1, T, H, W, device='cuda'); qm[:, :, 0, H // 4:H // 2, W // 4:W // 2] = 1

    def forward():
        with torch.no_grad():
            net(rgb, qm)

    held = {}

    def maps():
        held['maps'] = net.attention_maps(rgb, qm, spatial_queries='cls')[2]

    for _ in range(warmup):
        forward(); maps()
    samples = {'forward': [], 'attention_maps': []}
    for _ in range(rounds):
        samples['forward'].append(timed(forward)); samples['attention_maps'].append(timed(maps))
    res = {k: stats(v) for k, v in samples.items()}
    m = held['maps']
    res['maps_bytes'] = sum(t.numel() * 4 for t in list(m.temporal.values()) + list(m.spatial.values()))
    res['extra_ms'] = round(res['attention_maps']['median'] - res['forward']['median'], 3)
    return res


def kernel_legs(geo, rounds, batch):
    """us per launch of the temporal form and of the rows form with one query position (the 'cls' table of causal_attention 1)."""
    T, S = geo['T'], (geo['H'] // P) * (geo['W'] // P) + 1
    M = T * S
    g = torch.Generator(device='cuda').manual_seed(1)
    qkv = [torch.randn(M, 3 * D, device='cuda', generator=g).to(torch.bfloat16) for _ in range(COPIES)]
    out_t = [torch.empty(1, S - 1, HEADS, T, T, device='cuda') for _ in range(COPIES)]
    out_r = [torch.empty(T, 1, HEADS, S, device='cuda') for _ in range(COPIES)]
    pos = torch.zeros(1, dtype=torch.int32, device='cuda')
    shape = ops.attn_shape(ops.BF16, 1, T, S, D, HEADS, CA)
    legs = {'temporal': lambda i: ops.attn_probs(shape, False, qkv[i], out_t[i]),
            'rows': lambda i: ops.attn_probs(shape, True, qkv[i], out_r[i], pos=pos)}

    def sample(fn):
        def run():
            for k in range(batch):
                fn(k % COPIES)
        return timed(run) * 1e3 / batch

    for fn in legs.values():
        sample(fn)
    samples = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            samples[k].append(sample(fn))
    res = {k: stats(v) for k, v in samples.items()}
    nbytes = {'temporal': {'read': 2 * T * (S - 1) * D * 2, 'written': out_t[0].numel() * 4},
              'rows': {'read': (T * S + T) * D * 2, 'written': out_r[0].numel() * 4}}
    for k, nb in nbytes.items():
        res[k].update(bytes_read=nb['read'], bytes_written=nb['written'], gbytes_per_s=round((nb['read'] + nb['written']) / (res[k]['median'] * 1e-6) / 1e9, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dev_attn_maps.py needs a GPU')
    res = {'device': torch.cuda.get_device_name(0), 'precision': 'bf16', 'B': 1, 'blocks': 12, 'spatial_queries': 'cls', 'causal_attention': CA, 'rounds': a.rounds,
           'batch': a.batch, 'copies': COPIES, 'speed_target': None, 'geometries': {}}
    for name, geo in GEOMETRIES.items():
        kernels = kernel_legs(geo, a.rounds, a.batch)
        print(name, json.dumps(kernels), flush=True)
        module = module_legs(geo, a.rounds, a.warmup)
        print(name, json.dumps(module), flush=True)
        res['geometries'][name] = dict(geo, S=(geo['H'] // P) * (geo['W'] // P) + 1, module_ms=module, kernels_us=kernels)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

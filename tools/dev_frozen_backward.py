"""Dev: what frozen parameters save in forward + backward at BASELINE configs[1], on the GPU.

    python tools/dev_frozen_backward.py --out profiles/frozen_backward.json

One clip of T = 30 frames at 240 x 320 with its 3 queries as a plain batch (M = 27 090 token rows, the benchmark's), ViT-B, precision 'bf16', train mode,
drop_path_rate 0.  Three legs alternate in one process after warm-up; each sample is one forward + backward between a pair of device events:

  a  the inputs require grad, every parameter trainable (what the backward did before it looked at requires_grad: the baseline);
  b  the same with every parameter frozen (a saliency / adversarial-probe iteration);
  c  no input gradients, only the heads and the top two blocks trainable (fine-tuning a loaded checkpoint): the chain stops below block depth - 2
     and the forward keeps no activations of the blocks under it.

Reported: median of the rounds with each leg's own min / max, the differences to leg a, and the peak allocated memory of a and c (the allocator's
high-water mark over one forward + backward, reset before it).  A fourth measurement is the new launch alone: tcow_colsum_grouped on the seven output
gradients of a block's Linear layers (--batch calls between one pair of events, on COPIES sets of operands), with the bytes it reads.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tcow_amd import ops, synth                 # noqa: E402
from tcow_amd.seeker import Seeker              # noqa: E402

T, H, W, P, D, QUERIES = 30, 240, 320, 16, 768, 3
COPIES = 3


def stats(v):
    v = sorted(v)
    return {'median': round(v[len(v) // 2], 3), 'min': round(v[0], 3), 'max': round(v[-1], 3), 'spread': round(v[-1] - v[0], 3)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)                     # ms


def step_legs(rounds, warmup):
    torch.manual_seed(0)
    net = Seeker(None, num_total_frames=T, frame_height=H, frame_width=W, causal_attention=1, drop_path_rate=0.0, precision='bf16').cuda().train()
    depth = net.seeker.network_depth
    clip = synth.make_clip(1, T, H, W, seed=900)
    rgb = torch.from_numpy(clip['rgb']).cuda().expand(QUERIES, -1, -1, -1, -1).contiguous()
    qm = torch.cat([torch.from_numpy(synth.make_query_mask(clip, q, 0)) for q in range(QUERIES)], 0).cuda()
    top = tuple('.blocks.%d.' % j for j in (depth - 2, depth - 1))
    trainable = {'a': lambda n: True, 'b': lambda n: False, 'c': lambda n: 'post_linear' in n or '.model.norm.' in n or any(t in n for t in top)}
    inputs = {'a': True, 'b': True, 'c': False}
    peak = {}

    def leg(name):
        for n, p in net.named_parameters():
            p.requires_grad_(trainable[name](n))
        net.zero_grad(set_to_none=True)
        r, q = rgb.clone().requires_grad_(inputs[name]), qm.clone().requires_grad_(inputs[name])
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()

        def step():
            om, fl = net(r, q)
            (om.square().mean() + fl.square().mean()).backward()
        ms = timed(step)
        peak[name] = {'peak_allocated_mb': round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), 'allocated_before_mb': round(base / 2 ** 20, 1)}
        assert (r.grad is not None) == inputs[name]
        got = sum(p.grad is not None for p in net.parameters())
        assert (got == 0) == (name == 'b') and (name != 'a' or got > 200)
        return ms

    for _ in range(warmup):
        for name in 'abc':
            leg(name)
    samples = {name: [] for name in 'abc'}
    for _ in range(rounds):
        for name in 'abc':
            samples[name].append(leg(name))
    res = {name: dict(stats(v), **peak[name]) for name, v in samples.items()}
    for name in 'bc':
        res[name]['saved_vs_a_ms'] = round(res['a']['median'] - res[name]['median'], 3)
    return res


def colsum_leg(rounds, batch):
    """us per tcow_colsum_grouped call over the seven Linear output gradients of a divided space-time block, 16-bit storage."""
    M = QUERIES * T * ((H // P) * (W // P) + 1)
    widths = [D, 4 * D, D, 3 * D, D, D, 3 * D]                       # fc2, fc1, proj, qkv, tfc, tproj, tqkv
    g = torch.Generator(device='cuda').manual_seed(1)
    sets = [[(torch.randn(M, N, device='cuda', generator=g).to(torch.bfloat16), torch.empty(N, device='cuda')) for N in widths] for _ in range(COPIES)]

    def sample():
        def run():
            for k in range(batch):
                ops.colsum_grouped(ops.BF16, sets[k % COPIES])
        return timed(run) * 1e3 / batch

    sample()
    res = stats([sample() for _ in range(rounds)])
    nbytes = M * sum(widths) * 2
    res.update(M=M, widths=widths, bytes_read=nbytes, gbytes_per_s=round(nbytes / (res['median'] * 1e-6) / 1e9, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dev_frozen_backward.py needs a GPU')
    colsum = colsum_leg(a.rounds, a.batch)
    print(json.dumps(colsum), flush=True)
    legs = step_legs(a.rounds, a.warmup)
    print(json.dumps(legs), flush=True)
    res = {'device': torch.cuda.get_device_name(0), 'precision': 'bf16', 'geometry': dict(T=T, H=H, W=W, P=P, D=D, query_rows=QUERIES), 'rounds': a.rounds,
           'legs': {'a': 'inputs require grad, every parameter trainable', 'b': 'inputs require grad, every parameter frozen',
                    'c': 'no input gradients, heads and the top two blocks trainable'},
           'forward_backward_ms': legs, 'colsum_grouped_block_us': colsum}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

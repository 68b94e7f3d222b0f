"""Dev: what the backward to the inputs (engine._input_backward) costs at BASELINE configs[1], on the GPU.

    python tools/dev_input_grad.py --out profiles/input_grad.json

One clip of T = 30 frames at 240 x 320 with its 3 queries as a plain batch (M = 27 090 token rows, the benchmark's), ViT-B, precision 'bf16', train mode.
Two measurements, each with its legs alternating in one process after warm-up, timed with device events:

  * the whole backward with and without the frames and the query mask requiring grad (the forward in front of each is not timed);
  * the launches alone, --batch of them between one pair of events: the product dA = G W_pe (M = 27 090, N = 1024, K = 768, f32 output), tcow_col2im, and
    tcow_im2col at the same geometry -- the yardstick: both move the same pixels.  Every launch of a batch works on the next of COPIES sets of buffers
    (COPIES x 111 MB of matrix: more than the 256 MiB Infinity Cache), so none finds its data where the launch before left it.

Bytes are the algorithm's, computed from the shapes: col2im reads the patch rows of the f32 matrix and writes the f32 images (a permutation: the same count
both ways), im2col reads the f32 images and writes the whole 16-bit matrix, slot-0 rows included.
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
COPIES = 4


def stats(v):
    v = sorted(v)
    return {'median': round(v[len(v) // 2], 3), 'min': round(v[0], 3), 'max': round(v[-1], 3)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)                     # ms


def backward_legs(rounds, warmup):
    """ms per backward, inputs requiring grad or not."""
    torch.manual_seed(0)
    net = Seeker(None, num_total_frames=T, frame_height=H, frame_width=W, causal_attention=1, drop_path_rate=0.0, precision='bf16').cuda().train()
    clip = synth.make_clip(1, T, H, W, seed=900)
    rgb = torch.from_numpy(clip['rgb']).cuda().expand(QUERIES, -1, -1, -1, -1).contiguous()
    qm = torch.cat([torch.from_numpy(synth.make_query_mask(clip, q, 0)) for q in range(QUERIES)], 0).cuda()

    def leg(inputs):
        net.zero_grad(set_to_none=True)
        r, q = rgb.clone().requires_grad_(inputs), qm.clone().requires_grad_(inputs)
        om, fl = net(r, q)
        loss = om.square().mean() + fl.square().mean()
        ms = timed(loss.backward)
        assert (r.grad is not None) == inputs and (q.grad is not None) == inputs
        return ms

    for _ in range(warmup):
        leg(False); leg(True)
    samples = {'without': [], 'with': []}
    for _ in range(rounds):
        samples['without'].append(leg(False)); samples['with'].append(leg(True))
    return {k: stats(v) for k, v in samples.items()}


def launch_legs(rounds, batch):
    """us per launch of the product, col2im and im2col at B = 3 query rows."""
    B, S, PP = QUERIES, (H // P) * (W // P) + 1, P * P
    M = B * T * S
    g = torch.Generator(device='cuda').manual_seed(1)
    G = [torch.randn(M, D, device='cuda', generator=g).to(torch.bfloat16) for _ in range(COPIES)]
    Wt = [(torch.randn(4 * PP, D, device='cuda', generator=g) * 0.05).to(torch.bfloat16) for _ in range(COPIES)]
    dA = [torch.randn(M, 4 * PP, device='cuda', generator=g) for _ in range(COPIES)]
    d_rgb = [torch.empty(B, 3, T, H, W, device='cuda') for _ in range(COPIES)]
    d_qm = [torch.empty(B, 1, T, H, W, device='cuda') for _ in range(COPIES)]
    rgb = [torch.rand(B, 3, T, H, W, device='cuda', generator=g) for _ in range(COPIES)]
    qm = [torch.rand(B, 1, T, H, W, device='cuda', generator=g) for _ in range(COPIES)]
    A = [torch.empty(M, 4 * PP, device='cuda', dtype=torch.bfloat16) for _ in range(COPIES)]
    out = torch.empty(M, 4 * PP, device='cuda')
    legs = {'gemm_nt': lambda i: ops.gemm_nt(ops.BF16, G[i], Wt[i], out),
            'col2im': lambda i: ops.col2im(dA[i], B, T, H, W, P, False, d_rgb[i], d_qm[i]),
            'im2col': lambda i: ops.im2col(ops.BF16, rgb[i], qm[i], P, False, A[i])}

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
    pixels = B * 4 * T * H * W
    nbytes = {'col2im': {'read': pixels * 4, 'written': pixels * 4}, 'im2col': {'read': pixels * 4, 'written': M * 4 * PP * 2}}
    for k, nb in nbytes.items():
        res[k].update(bytes_read=nb['read'], bytes_written=nb['written'], gbytes_per_s=round((nb['read'] + nb['written']) / (res[k]['median'] * 1e-6) / 1e9, 1))
    res['gemm_nt'].update(M=M, N=4 * PP, K=D, gflop=round(2.0 * M * 4 * PP * D / 1e9, 2), tflops=round(2.0 * M * 4 * PP * D / (res['gemm_nt']['median'] * 1e-6) / 1e12, 1))
    res['col2im_over_im2col_rate'] = round(res['col2im']['gbytes_per_s'] / res['im2col']['gbytes_per_s'], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dev_input_grad.py needs a GPU')
    launches = launch_legs(a.rounds, a.batch)
    print(json.dumps(launches), flush=True)
    backward = backward_legs(a.rounds, a.warmup)
    backward['with_minus_without_ms'] = round(backward['with']['median'] - backward['without']['median'], 3)
    backward['launches_sum_ms'] = round((launches['gemm_nt']['median'] + launches['col2im']['median']) * 1e-3, 3)
    print(json.dumps(backward), flush=True)
    res = {'device': torch.cuda.get_device_name(0), 'precision': 'bf16', 'geometry': dict(T=T, H=H, W=W, P=P, D=D, query_rows=QUERIES), 'rounds': a.rounds, 'batch': a.batch,
           'copies': COPIES, 'backward_ms': backward, 'launches_us': launches}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

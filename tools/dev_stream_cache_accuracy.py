"""Dev: what a compact K / V cache (net.stream(cache_dtype=...), tcow_amd/stream.py) costs in accuracy, on the GPU.

    python tools/dev_stream_cache_accuracy.py --out accuracy.json        # its rows are the 'accuracy' list of profiles/stream_cache_dtype.json

For every (precision, cache_dtype) pair, None included, the clip of a reference golden (tests/golden) is streamed frame by frame and the mask
logits are compared with the REFERENCE's, not with the None stream's: max |d| of the logits (the small goldens g1_cfg1_d256 and g2_ca2, whose
files hold the full output, with the flags' max |d| next to it) or of the 4x4-pooled logits (g4: BASELINE configs[1] at full size; g16: the same
geometry at the logit scale of a trained checkpoint, parity modes only, with the fraction of mask bits that agree).  The result is a fixed
function of the inputs: one run, no repetitions.  --only g1,g2 for the two small ones (the bounds of tests/test_gpu_stream_cache_dtype.py).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from conftest import build_hip_seeker, golden_inputs, load_golden                    # noqa: E402
from test_oracle_golden import mask_bits, summarise, trained_scale_inputs           # noqa: E402

GOLDENS = {'g1': 'g1_cfg1_d256', 'g2': 'g2_ca2', 'g4': 'g4_cfg2_T30_240x320', 'g16': 'g16_cfg2_trained_scale'}
KEYWORDS = {'fp32': (None, 'bf16', 'fp8'), 'bf16x3': (None, 'bf16', 'fp8'), 'bf16': (None, 'fp8'), 'fp16': (None, 'fp8')}


def stream_clip(net, rgb, qm, keyword):
    st = net.stream(batch_size=rgb.shape[0], cache_dtype=keyword)
    outs = [st.step(rgb[:, :, t:t + 1], qm[:, :, t:t + 1]) for t in range(rgb.shape[2])]
    return torch.cat([m for m, _ in outs], 2), torch.cat([f for _, f in outs], 1), st.cache_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--only', default='g1,g2,g4,g16')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dev_stream_cache_accuracy.py needs a GPU')
    rows = []
    for tag in a.only.split(','):
        meta, g = load_golden(GOLDENS[tag])
        cfg, sd, rgb, qm = trained_scale_inputs(meta) if tag == 'g16' else golden_inputs(meta)
        rgb, qm = rgb.cuda(), qm.cuda()
        for precision in (('fp32', 'bf16x3') if tag == 'g16' else KEYWORDS):
            net = build_hip_seeker(cfg, sd, precision).cuda().eval()
            for keyword in KEYWORDS[precision]:
                om, fl, nbytes = stream_clip(net, rgb, qm, keyword)
                row = {'golden': GOLDENS[tag], 'precision': precision, 'cache_dtype': keyword, 'cache_bytes': nbytes, 'finite': bool(torch.isfinite(om).all())}
                if 'output_mask' in g:
                    row['mask_logits_max_abs_d'] = float((om.cpu() - torch.from_numpy(g['output_mask'])).abs().max())
                    row['flags_max_abs_d'] = float((fl.cpu() - torch.from_numpy(g['output_flags'])).abs().max())
                else:
                    pooled, _, _ = summarise(om.cpu())
                    row['pooled_logits_max_abs_d'] = float(np.abs(pooled - g['pooled']).max())
                    row['logit_std'] = float(g['logit_std'])
                    if 'mask_bits' in g:
                        row['mask_bits_agree'] = 1.0 - float(np.unpackbits(mask_bits(om.cpu().numpy(), meta['mask_frames']) ^ g['mask_bits']).mean())
                print(json.dumps(row), flush=True)
                rows.append(row)
            del net
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()

"""GPU: the gradients of the frames and of the query mask (engine._input_backward) against the oracle.

oracle.seeker_oracle.seeker_forward is plain torch and differentiable in its inputs; it runs on the CPU with requires_grad inputs, once per case.
Bounds: the ones the project holds for its PARAMETER gradients on the same inputs -- gtol * max|ref| + 1e-7 with gtol 2e-4 (fp32), 5e-3 (fp16), 4e-2
(bf16) from test_random_geometries_vs_oracle and 2e-4 (bf16x3) from test_gradients_vs_reference_golden.  The input gradient is the sibling of the
patch-embed weight gradient: the same operand G and one more rounding of W_pe to the mode's 16 bits.  Each case prints its max|d| / max|ref|."""
import numpy as np
import pytest
import torch

from conftest import build_hip_seeker
from tcow_amd import synth

pytestmark = pytest.mark.gpu

GTOL = {'fp32': 2e-4, 'fp16': 5e-3, 'bf16': 4e-2, 'bf16x3': 2e-4}
PRECISIONS = ('fp32', 'fp16', 'bf16', 'bf16x3')


def oracle_run(cfg, sd, rgb, qm, Gm=None, Gf=None, rng=None, drop_masks=None, params_grad=True, seed_scale=1.0):
    """The oracle's outputs and gradients for the loss <om, Gm> + <fl, Gf> -> (om, fl, d_rgb, d_qm, {name: param grad}, Gm, Gf); Gm, Gf: given, or
    standard normal draws of rng times seed_scale."""
    from oracle import seeker_oracle as so
    tsd = so.to_torch_state_dict(sd)
    for v in tsd.values():
        v.requires_grad_(params_grad)
    rgb = rgb.clone().requires_grad_(True); qm = qm.clone().requires_grad_(True)
    om, fl = so.seeker_forward(tsd, cfg, rgb, qm, drop_masks=drop_masks)
    if Gm is None:
        Gm = torch.from_numpy(rng.standard_normal(size=tuple(om.shape)).astype(np.float32)) * seed_scale
        Gf = torch.from_numpy(rng.standard_normal(size=tuple(fl.shape)).astype(np.float32)) * seed_scale
    ((om * Gm).sum() + (fl * Gf).sum()).backward()
    return om.detach(), fl.detach(), rgb.grad, qm.grad, {k: v.grad for k, v in tsd.items()}, Gm, Gf


def hip_run(net, rgb, qm, Gm, Gf, rgb_grad=True, qm_grad=True):
    """One forward + backward of the module -> (om, fl, rgb.grad, qm.grad)."""
    net.zero_grad(set_to_none=True)
    r = rgb.cuda().requires_grad_(rgb_grad); q = qm.cuda().requires_grad_(qm_grad)
    om, fl = net(r, q)
    ((om * Gm.cuda()).sum() + (fl * Gf.cuda()).sum()).backward()
    return om.detach(), fl.detach(), r.grad, q.grad


def close(got, ref, precision, what):
    assert got is not None and got.shape == ref.shape and got.dtype == ref.dtype, (precision, what)
    d, scale = float((got.cpu() - ref).abs().max()), float(ref.abs().max())
    print(f'{what} {precision}: max|d| / max|ref| = {d / max(scale, 1e-30):.3e}  (bound {GTOL[precision]:.0e})')
    assert d <= GTOL[precision] * scale + 1e-7, (precision, what, d, scale)


def param_grads(net):
    return [None if p.grad is None else p.grad.detach().clone() for p in net.parameters()]


def same_grads(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and torch.equal(x, y)) for x, y in zip(a, b))


def small_case(seed, B=2, T=3, Hp=2, Wp=3, D=64, depth=2, queries=1, **kw):
    cfg = synth.seeker_config(num_total_frames=T, frame_height=16 * Hp, frame_width=16 * Wp, embed_dim=D, depth=depth, num_heads=D // 64, **kw)
    sd = synth.make_state_dict(cfg, 7000 + seed)
    clip = synth.make_clip(B, T, 16 * Hp, 16 * Wp, seed=7100 + seed)
    rgb = torch.from_numpy(clip['rgb'])
    qm = torch.stack([torch.from_numpy(synth.make_query_mask(clip, q, 0)) for q in range(queries)], 1).reshape(B * queries, 1, T, 16 * Hp, 16 * Wp)   # clip-major rows
    return cfg, sd, rgb, qm


@pytest.mark.parametrize('seed', list(range(8)))
def test_random_geometries_vs_oracle(cuda, seed):
    """Eight random small geometries from the generator ranges of test_gpu_seeker.py::test_random_geometries_vs_oracle; in the same runs, the outputs and
    the parameter gradients with the inputs requiring grad are bit for bit those without."""
    rng = np.random.default_rng(4000 + seed)
    T = int(rng.integers(1, 10)); Hp = int(rng.integers(1, 6)); Wp = int(rng.integers(1, 7)); D = int(rng.choice([64, 128, 192]))
    cfg = synth.seeker_config(num_total_frames=T, frame_height=16 * Hp, frame_width=16 * Wp, embed_dim=D, depth=int(rng.integers(1, 4)), num_heads=D // 64,
                              causal_attention=[-1, 0, 1, 2, 3, 4][seed % 6], norm_embeddings=bool(rng.integers(0, 2)), track_map_stride=int(rng.choice([1, 2, 4])),
                              track_map_resize=['bilinear', 'nearest'][seed % 2], pretrained_norm=bool((seed // 2) % 2))
    sd = synth.make_state_dict(cfg, 5000 + seed)
    B = int(rng.integers(1, 4))
    clip = synth.make_clip(B, T, 16 * Hp, 16 * Wp, seed=6000 + seed)
    rgb = torch.from_numpy(clip['rgb']); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0))
    om_r, fl_r, drgb_r, dqm_r, _, Gm, Gf = oracle_run(cfg, sd, rgb, qm, rng=rng)
    assert float(drgb_r.abs().max()) > 0 and float(dqm_r.abs().max()) > 0
    for precision in PRECISIONS:
        net = build_hip_seeker(cfg, sd, precision).cuda().train()           # drop_path_rate 0: train mode only to get gradients
        om0, fl0, none_r, none_q = hip_run(net, rgb, qm, Gm, Gf, False, False)
        assert none_r is None and none_q is None
        plain = param_grads(net)
        om, fl, d_rgb, d_qm = hip_run(net, rgb, qm, Gm, Gf)
        assert torch.equal(om, om0) and torch.equal(fl, fl0), (precision, cfg)
        assert same_grads(param_grads(net), plain), (precision, cfg)
        close(d_rgb, drgb_r, precision, 'd_rgb'); close(d_qm, dqm_r, precision, 'd_qm')


@pytest.mark.parametrize('precision', PRECISIONS)
def test_shared_rgb_sums_the_queries(cuda, precision):
    """Qs = 2 queries on each of 2 clips, the frames passed once: d_rgb (Bc, 3, T, H, W) is the oracle's on the expanded batch summed over each clip's
    queries, d_qm matches row by row."""
    cfg, sd, rgb, qm = small_case(1, queries=2, causal_attention=1)
    expanded = rgb[:, None].expand(2, 2, -1, -1, -1, -1).reshape(4, *rgb.shape[1:]).contiguous()
    _, _, drgb_r, dqm_r, _, Gm, Gf = oracle_run(cfg, sd, expanded, qm, rng=np.random.default_rng(11))
    net = build_hip_seeker(cfg, sd, precision).cuda().train()
    _, _, d_rgb, d_qm = hip_run(net, rgb, qm, Gm, Gf)
    assert tuple(d_rgb.shape) == tuple(rgb.shape)
    close(d_rgb, drgb_r.reshape(2, 2, *rgb.shape[1:]).sum(1), precision, 'shared d_rgb'); close(d_qm, dqm_r, precision, 'shared d_qm')
    _, _, only_rgb, no_qm = hip_run(net, rgb, qm, Gm, Gf, qm_grad=False)
    assert no_qm is None and torch.equal(only_rgb, d_rgb)
    _, _, no_rgb, only_qm = hip_run(net, rgb, qm, Gm, Gf, rgb_grad=False)
    assert no_rgb is None and torch.equal(only_qm, d_qm)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_joint_attention(cuda, precision):
    cfg, sd, rgb, qm = small_case(2, causal_attention=0, attention_type='joint_space_time')
    _, _, drgb_r, dqm_r, _, Gm, Gf = oracle_run(cfg, sd, rgb, qm, rng=np.random.default_rng(12))
    from tcow_amd.seeker import Seeker
    net = Seeker(None, num_total_frames=cfg['num_total_frames'], frame_height=cfg['frame_height'], frame_width=cfg['frame_width'], tracker_pretrained=False,
                 patch_size=16, causal_attention=0, attention_type='joint_space_time', drop_path_rate=0.0, network_depth=cfg['depth'], embed_dim=cfg['embed_dim'],
                 norm_embeddings=cfg['norm_embeddings'], track_map_stride=cfg['track_map_stride'], track_map_resize=cfg['track_map_resize'],
                 num_heads=cfg['num_heads'], precision=precision)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    _, _, d_rgb, d_qm = hip_run(net.cuda().train(), rgb, qm, Gm, Gf)
    close(d_rgb, drgb_r, precision, 'joint d_rgb'); close(d_qm, dqm_r, precision, 'joint d_qm')


@pytest.mark.parametrize('precision', PRECISIONS)
def test_forced_droppath(cuda, precision):
    """Train mode with forced keep masks that drop one temporal row (a patch site of clip 0), one spatial row (a frame of clip 1) and clip 1's whole MLP
    branch in the last block: the input gradients are the oracle's under the same masks, the dropped clip's among them."""
    cfg, sd, rgb, qm = small_case(3, causal_attention=1)
    B, T, N = 2, 3, 6
    kt = torch.ones(B, N); kt[0, 2] = 0
    ks = torch.ones(B, T); ks[1, 1] = 0
    km = torch.ones(B); km[1] = 0
    masks = {(0, 'temporal'): (kt, 0.1), (0, 'spatial'): (ks, 0.1), (1, 'mlp'): (km, 0.2), (0, 'mlp'): (torch.ones(B), 0.1)}
    _, _, drgb_r, dqm_r, _, Gm, Gf = oracle_run(cfg, sd, rgb, qm, rng=np.random.default_rng(13), drop_masks=masks)
    _, _, drgb_e, _, _, _, _ = oracle_run(cfg, sd, rgb, qm, Gm=Gm, Gf=Gf)
    assert float((drgb_r[1] - drgb_e[1]).abs().max()) > 1e-3 * float(drgb_e.abs().max())          # the masks matter to the dropped clip's gradient
    net = build_hip_seeker(cfg, sd, precision, drop_path_rate=0.2).cuda().train()
    net.seeker.forced_drop_masks = masks
    _, _, d_rgb, d_qm = hip_run(net, rgb, qm, Gm, Gf)
    close(d_rgb, drgb_r, precision, 'droppath d_rgb'); close(d_qm, dqm_r, precision, 'droppath d_qm')
    close(d_rgb[1:], drgb_r[1:], precision, 'droppath d_rgb, dropped clip')


@pytest.mark.parametrize('loss_scale', ['dynamic', 1024.0])
def test_fp16_input_grads_are_unscaled_while_the_buckets_stay_scaled(cuda, loss_scale):
    """fp16 with FusedAdamWClip(module=net) and persistent_grads: the parameter buckets stay loss-scaled for the optimizer (pending_inv_scale is set), the
    input gradients come back unscaled all the same -- bit for bit those of the step that unscales in the backward.  The seeds are 2^-12 x standard normal
    (the size of a mean-reduced loss's, where a static scale of 1024 is a sensible choice: 1024 x seeds of order one would overflow binary16)."""
    from tcow_amd.optim import FusedAdamWClip
    cfg, sd, rgb, qm = small_case(4, causal_attention=1)
    _, _, drgb_r, dqm_r, _, Gm, Gf = oracle_run(cfg, sd, rgb, qm, rng=np.random.default_rng(14), seed_scale=2.0 ** -12)
    got = {}
    for defer in (True, False):
        net = build_hip_seeker(cfg, sd, 'fp16').cuda().train()
        net.seeker.persistent_grads, net.seeker.loss_scale, net.seeker._defer_unscale = True, loss_scale, defer
        opt = FusedAdamWClip(list(net.parameters()), lr=1e-3, max_norm=0.3, module=net)
        _, _, d_rgb, d_qm = hip_run(net, rgb, qm, Gm, Gf)
        inv = net.seeker.pending_inv_scale
        if defer:
            assert inv is not None and float(inv) != 1.0                    # param.grad is still scaled
            if loss_scale != 'dynamic':
                assert float(inv) == 1.0 / 1024.0
        else:
            assert inv is None
        got[defer] = (d_rgb, d_qm, net.seeker.tracker_post_linear.weight.grad.detach().clone(), inv)
        del opt
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])
    assert torch.equal(got[True][2] * got[True][3], got[False][2])          # (and the deferred bucket differs from the unscaled one by exactly the scale)
    close(got[True][0], drgb_r, 'fp16', f'deferred ({loss_scale}) d_rgb'); close(got[True][1], dqm_r, 'fp16', f'deferred ({loss_scale}) d_qm')


@pytest.mark.parametrize('precision', PRECISIONS)
def test_frozen_parameters_in_eval_mode(cuda, precision):
    cfg, sd, rgb, qm = small_case(5, causal_attention=1, pretrained_norm=True)
    _, _, drgb_r, dqm_r, _, Gm, Gf = oracle_run(cfg, sd, rgb, qm, rng=np.random.default_rng(15), params_grad=False)
    net = build_hip_seeker(cfg, sd, precision).cuda().eval()
    for p in net.parameters():
        p.requires_grad_(False)
    _, _, d_rgb, d_qm = hip_run(net, rgb, qm, Gm, Gf)
    close(d_rgb, drgb_r, precision, 'frozen d_rgb'); close(d_qm, dqm_r, precision, 'frozen d_qm')
    assert all(p.grad is None for p in net.parameters())


def test_one_input_only_and_half_precision_inputs(cuda):
    cfg, sd, rgb, qm = small_case(6, causal_attention=2)
    _, _, drgb_r, dqm_r, _, Gm, Gf = oracle_run(cfg, sd, rgb, qm, rng=np.random.default_rng(16))
    net = build_hip_seeker(cfg, sd, 'fp32').cuda().train()
    _, _, d_rgb, d_qm = hip_run(net, rgb, qm, Gm, Gf)
    _, _, only_rgb, no_qm = hip_run(net, rgb, qm, Gm, Gf, qm_grad=False)
    assert no_qm is None and torch.equal(only_rgb, d_rgb)
    _, _, no_rgb, only_qm = hip_run(net, rgb, qm, Gm, Gf, rgb_grad=False)
    assert no_rgb is None and torch.equal(only_qm, d_qm)
    close(d_rgb, drgb_r, 'fp32', 'd_rgb'); close(d_qm, dqm_r, 'fp32', 'd_qm')
    # inputs given in torch.float16: Seeker.forward casts them with .to(float32), which autograd differentiates -- the gradient arrives in float16
    _, _, h_rgb, h_qm = hip_run(net, rgb.half(), qm.half(), Gm, Gf)
    assert h_rgb.dtype == torch.float16 and h_qm.dtype == torch.float16 and h_rgb.shape == rgb.shape and h_qm.shape == qm.shape
    assert bool(torch.isfinite(h_rgb).all()) and float(h_rgb.float().abs().max()) > 0

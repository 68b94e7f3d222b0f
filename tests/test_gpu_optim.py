"""GPU: FusedAdamWClip on libtcow_hip -- against torch's clip_grad_norm_ + AdamW to a tolerance, against itself bit for bit across its
paths (fused operand copies, deferred unscale), and against the bits of the commit before the library's optimizer entry points became one
(tests/golden/optim_step_bits.json, tools/make_optim_bits.py).  The host side of every step is pinned on the CPU: test_optim_calls_host.py."""
import json
import math

import numpy as np
import pytest
import torch

import optim_calls as kit
from conftest import build_hip_seeker
from tcow_amd import synth

pytestmark = pytest.mark.gpu


def test_fused_adamw_clip_matches_torch(cuda):
    """tcow_adamw_clip_step == torch.nn.utils.clip_grad_norm_(0.3) + torch.optim.AdamW (train.py:99-102), incl. params without grad."""
    from tcow_amd.optim import FusedAdamWClip
    g = torch.Generator(device='cuda').manual_seed(0)
    shapes = [(768, 768), (3, 5), (70001,), (1, 1, 768), (2304,)]
    pa = [torch.nn.Parameter(torch.randn(s, device=cuda, generator=g)) for s in shapes] + [torch.nn.Parameter(torch.zeros(7, device=cuda))]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ref = torch.optim.AdamW(pb, lr=1e-3)
    opt = FusedAdamWClip(pa, lr=1e-3, max_norm=0.3)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, [1, 2], gamma=0.3); sched_ref = torch.optim.lr_scheduler.MultiStepLR(ref, [1, 2], gamma=0.3)   # train.py:236-243 attaches unchanged
    for it in range(3):
        for a, b in zip(pa[:-1], pb[:-1]):                      # the last parameter never gets a gradient
            gr = torch.randn(a.shape, device=cuda, generator=g) * (10.0 if it == 0 else 0.001)   # clipped on step 0, not afterwards
            a.grad = gr.clone(); b.grad = gr.clone()
        n_ref = torch.nn.utils.clip_grad_norm_(pb, 0.3)
        v0 = pa[0]._version
        ref.step(); opt.step(); sched.step(); sched_ref.step()
        assert pa[0]._version > v0                              # raw-pointer update made visible to version-keyed caches
        assert abs(float(opt.grad_norm()) - float(n_ref)) <= 1e-4 * float(n_ref)
        for a, b in zip(pa, pb):
            assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(b.abs().max()))
    # state in torch.optim.AdamW's layout: it loads into AdamW and back (train.py:246-257 resumes 'optim_seeker' this way)
    ref2 = torch.optim.AdamW(pb, lr=1e-3); ref2.load_state_dict(opt.state_dict())
    assert all(torch.equal(ref2.state[b]['exp_avg'], opt.state[a]['exp_avg']) for a, b in zip(pa[:-1], pb[:-1]))
    opt.load_state_dict(ref.state_dict())
    assert opt.step_count == 3


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_optimizer_writes_the_operand_copies_itself(cuda, precision):
    """FusedAdamWClip(module=net) in the 16-bit modes: the update kernel of the GEMM weights (64 x 64 tiles, the tile table of tcow_adamw_clip_step) also writes their 16-bit
    W / W^T operand copies, and the module's batched re-cast only covers the folded products.  Bit-identical training against fuse_cast=False (the separate
    re-cast of rounds 1-5); after a step every cached copy equals a cast of its f32 master weight and its transpose."""
    from tcow_amd.optim import FusedAdamWClip
    cfg = synth.seeker_config(num_total_frames=4, frame_height=64, frame_width=64, embed_dim=128, depth=2, num_heads=2, causal_attention=1)
    sd = synth.make_state_dict(cfg, 7)
    clip = synth.make_clip(2, 4, 64, 64, seed=3)
    rgb = torch.from_numpy(clip['rgb']).cuda(); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
    dt = torch.bfloat16 if precision == 'bf16' else torch.float16
    res = {}
    for fuse in (True, False):
        net = build_hip_seeker(cfg, sd, precision, drop_path_rate=0.0).cuda().train()
        net.seeker.persistent_grads = True
        opt = FusedAdamWClip(list(net.parameters()), lr=1e-3, max_norm=0.3, module=net, fuse_cast=fuse)
        losses = []
        for it in range(4):
            om, fl = net(rgb, qm)
            loss = om.square().mean() * 1e-2 + fl.square().mean() * 1e-2
            loss.backward(); opt.step()
            losses.append(float(loss.detach()))
        assert (opt._tiles is not None) == fuse
        if fuse:
            n_tiles = sum((p.shape[0] // 64) * (p.reshape(p.shape[0], -1).shape[1] // 64) for p in net.parameters() if id(p) in opt._cast_keys)
            assert opt._tiles.shape[0] == n_tiles and n_tiles > 0
            reg = net.seeker._operands.registry
            for k, (p, Wc, Wt, N, K) in reg.items():
                if isinstance(k, int):                                           # plain GEMM weights (fold entries: W' = Wfc Wproj, cast by the module)
                    w = p.detach().reshape(N, K).to(dt)
                    assert torch.equal(Wc, w) and torch.equal(Wt, w.t().contiguous()), (N, K, id(p) in opt._cast_keys)
        res[fuse] = (losses, [p.detach().clone() for p in net.parameters()], float(opt.grad_norm()))
    assert res[True][0] == res[False][0] and res[True][2] == res[False][2]
    assert all(torch.equal(a, b) for a, b in zip(res[True][1], res[False][1]))


def test_fp16_overflow_skips_the_step_and_lowers_the_loss_scale(cuda):
    """precision='fp16': a non-finite gradient (an overflow of the scaled binary16 backward) must not poison the weights: the fused
    clip + AdamW kernels skip the update (parameters and moments untouched) and the module's loss-scale exponent drops by 4, on the device;
    the next good step applies normally and the exponent creeps back."""
    from tcow_amd.optim import FusedAdamWClip
    cfg = synth.seeker_config(num_total_frames=4, frame_height=32, frame_width=32, embed_dim=128, depth=2, num_heads=2, causal_attention=1)
    net = build_hip_seeker(cfg, synth.make_state_dict(cfg, 5), 'fp16').cuda().train()
    opt = FusedAdamWClip(list(net.parameters()), lr=1e-3, max_norm=0.3, module=net)
    clip = synth.make_clip(1, 4, 32, 32, seed=2)
    rgb = torch.from_numpy(clip['rgb']).cuda(); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
    opt.zero_grad(set_to_none=True); om, fl = net(rgb, qm); (om.square().mean() + fl.square().mean()).backward(); opt.step()          # a normal step creates the scale state
    assert float(net.seeker.ls_log2) == -2.0 and all(bool(torch.isfinite(p).all()) for p in net.parameters())
    before = [p.detach().clone() for p in net.parameters()]
    m_before = opt.state[next(iter(net.parameters()))]['exp_avg'].clone()
    opt.zero_grad(set_to_none=True); om, fl = net(rgb, qm); (om.square().mean() + fl.square().mean()).backward()
    next(p for p in net.parameters() if p.grad is not None).grad.view(-1)[0] = float('inf')        # what an overflow looks like to the optimizer
    opt.step()
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))                # skipped
    assert torch.equal(m_before, opt.state[next(iter(net.parameters()))]['exp_avg'])
    assert float(net.seeker.ls_log2) == -6.0
    opt.zero_grad(set_to_none=True); om, fl = net(rgb, qm); (om.square().mean() + fl.square().mean()).backward(); opt.step()          # scale 2^-4 of before: still a good step
    assert not all(torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters()) and -6.0 < float(net.seeker.ls_log2) < -5.9


def test_fp16_deferred_unscale_only_with_one_backward_per_step(cuda):
    """ADVICE r5 (engine.py deferred unscale): the loss scale is chosen per backward, so leaving gradients scaled for the optimizer is only sound when ONE
    backward feeds a step.  (a) default module (persistent_grads False) + FusedAdamWClip(module=): two model calls in one graph (the reference's per-query
    loop, pipeline.py:134-174) -- nothing is deferred, param.grad = the sum of the two calls' TRUE gradients; (b) persistent_grads: deferred, and
    unscale_() turns param.grad into the true gradient, after which step() gives bit-identical parameters; (c) a discarded optimizer no longer leaves
    gradients scaled; (d) a DataParallel-style replica never defers."""
    import gc
    from tcow_amd.optim import FusedAdamWClip
    cfg = synth.seeker_config(num_total_frames=4, frame_height=32, frame_width=32, embed_dim=128, depth=2, num_heads=2, causal_attention=1)
    sd = synth.make_state_dict(cfg, 5)
    clip = synth.make_clip(2, 4, 32, 32, seed=2)
    rgb = torch.from_numpy(clip['rgb']).cuda()
    qms = [torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda(), torch.from_numpy(synth.make_query_mask(clip, 1, 1)).cuda()]
    loss_of = lambda om, fl, k: om.square().mean() * (1e-4 * (1 + 300 * k)) + fl.square().mean() * 1e-4      # very different seed magnitudes -> different scales

    def grads(net):
        return [None if p.grad is None else p.grad.detach().clone().float() for p in net.parameters()]

    # (a) two calls, one graph
    net = build_hip_seeker(cfg, sd, 'fp16').cuda().train()
    opt = FusedAdamWClip(list(net.parameters()), lr=1e-3, max_norm=0.3, module=net)
    singles = []
    for k in range(2):
        opt.zero_grad(set_to_none=True)
        om, fl = net(rgb, qms[k]); loss_of(om, fl, k).backward()
        assert net.seeker.__dict__.get('pending_inv_scale') is None
        singles.append(grads(net))
    opt.zero_grad(set_to_none=True)
    (om0, fl0), (om1, fl1) = net(rgb, qms[0]), net(rgb, qms[1])
    (loss_of(om0, fl0, 0) + loss_of(om1, fl1, 1)).backward()
    assert net.seeker.__dict__.get('pending_inv_scale') is None
    both = grads(net)
    for g, a, b in zip(both, singles[0], singles[1]):
        if g is not None:
            assert torch.allclose(g, a + b, rtol=1e-5, atol=1e-9 + 1e-6 * float((a + b).abs().max()))
    opt.step()
    assert math.isfinite(float(opt.grad_norm())) and float(opt.skipped_steps) == 0

    # (b) persistent_grads: deferred; unscale_() -> true gradients; step after unscale_ == step without it, bit for bit
    res = {}
    for use_unscale in (False, True):
        net = build_hip_seeker(cfg, sd, 'fp16').cuda().train(); net.seeker.persistent_grads = True
        opt = FusedAdamWClip(list(net.parameters()), lr=1e-3, max_norm=0.3, module=net)
        om, fl = net(rgb, qms[0]); loss_of(om, fl, 0).backward()
        inv = net.seeker.__dict__.get('pending_inv_scale')
        assert inv is not None and float(inv) != 1.0
        scaled = grads(net)
        if use_unscale:
            opt.unscale_()
            assert net.seeker.__dict__.get('pending_inv_scale') is None
            for g, s_ in zip(grads(net), scaled):
                if g is not None:
                    assert torch.equal(g, s_ * float(inv))
            n = float(torch.nn.utils.clip_grad_norm_(net.parameters(), 1e9))      # what INTEGRATION.md's isfinite(clip_grad_norm_) check sees: the true norm
        opt.step()
        if use_unscale:
            assert abs(n - float(opt.grad_norm())) <= 1e-4 * n
        res[use_unscale] = [p.detach().clone() for p in net.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(res[False], res[True]))

    # (c) the optimizer is gone: the next backward unscales itself again
    del opt; gc.collect()
    om, fl = net(rgb, qms[0])
    with pytest.warns(UserWarning, match='no FusedAdamWClip'):
        loss_of(om, fl, 0).backward()
    assert net.seeker.__dict__.get('pending_inv_scale') is None
    true0 = grads(net)
    # (d) a replica (torch.nn.DataParallel's shallow copy, flagged by torch) never defers, whatever its dict inherited
    opt = FusedAdamWClip(list(net.parameters()), lr=1e-3, max_norm=0.3, module=net)
    net.seeker._is_replica = True
    net.zero_grad(set_to_none=True)
    try:
        om, fl = net(rgb, qms[0]); loss_of(om, fl, 0).backward()
        assert net.seeker.__dict__.get('pending_inv_scale') is None
    finally:
        del net.seeker._is_replica
    for g, t in zip(grads(net), true0):
        if g is not None:
            assert torch.equal(g, t)


def test_fp16_unscaling_inside_the_optimizer_is_bit_identical(cuda):
    """precision='fp16' with FusedAdamWClip(module=net) and no data-parallel hook: the backward leaves the gradient buckets loss-scaled and the
    optimizer folds the inverse scale (a power of two) into its clip coefficient (grad_inv_scale of tcow_adamw_clip_step) instead of a multiplication pass
    over every bucket.  Same parameters, moments and gradient norm, bit for bit, as the path that unscales in the backward; param.grad of the
    deferred path = scaled gradient, pending_inv_scale = the factor."""
    from tcow_amd.optim import FusedAdamWClip
    cfg = synth.seeker_config(num_total_frames=4, frame_height=32, frame_width=32, embed_dim=128, depth=2, num_heads=2, causal_attention=1)
    sd = synth.make_state_dict(cfg, 5)
    clip = synth.make_clip(1, 4, 32, 32, seed=2)
    rgb = torch.from_numpy(clip['rgb']).cuda(); qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
    out = {}
    for deferred in (True, False):
        net = build_hip_seeker(cfg, sd, 'fp16').cuda().train()
        net.seeker.persistent_grads = True
        opt = FusedAdamWClip(list(net.parameters()), lr=1e-3, max_norm=0.3, module=net)
        if not deferred:
            net.seeker.__dict__['_defer_unscale'] = False
        norms = []
        for it in range(3):
            om, fl = net(rgb, qm)
            (om.square().mean() * 1e-4 + fl.square().mean() * 1e-4).backward()
            inv = net.seeker.__dict__.get('pending_inv_scale')
            assert (inv is not None) == deferred
            if it == 0:
                g0 = [p.grad.clone() * (inv if deferred else 1.0) for p in net.parameters() if p.grad is not None]
            opt.step()
            norms.append(float(opt.grad_norm()))
        assert not torch.equal(net.seeker.tracker_post_linear.weight.detach().cpu().float(), torch.as_tensor(np.asarray(sd['seeker.tracker_post_linear.weight'])).float())      # the steps did move the parameters
        out[deferred] = ([p.detach().clone() for p in net.parameters()], [opt.state[p]['exp_avg_sq'].clone() for p in net.parameters() if p in opt.state and 'exp_avg_sq' in opt.state[p]], norms, g0)
    (pa, va, na, ga), (pb, vb, nb, gb) = out[True], out[False]
    assert na == nb and all(math.isfinite(x) and x > 0 for x in na)
    assert all(torch.equal(a, b) for a, b in zip(ga, gb))                 # scaled gradient x inverse scale == the unscaled gradient (power of two)
    assert all(torch.equal(a, b) for a, b in zip(pa, pb)) and all(torch.equal(a, b) for a, b in zip(va, vb))


@pytest.fixture(scope='module')
def parent_bits():
    with open(kit.BITS_FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('precision', ['bf16', 'fp16', 'fp32'])
def test_four_steps_give_the_parent_commits_bits(cuda, precision, parent_bits):
    """kit.bits_run -- a clipped step, a loss-scaled unclipped one, a skipped one, one whose bias correction runs with step - skipped, all but the first
    on the fast path -- leaves every parameter, moment and operand copy with the sha256, and the gradient norm, skip count and loss-scale exponent with
    the exact value, recorded on the MI355X from the package and libraries of the commit before tcow_adamw_clip_step took an argument structure."""
    want, got = parent_bits[precision], kit.bits_run(precision)
    assert [s['tiles'] for s in want] == ([43] * 4 if precision != 'fp32' else [0] * 4)                     # the tile kernel ran iff the mode is 16-bit
    assert [float.fromhex(s['skipped_steps']) for s in want] == [0.0, 0.0, 1.0, 1.0]
    assert want[2]['params'] == want[1]['params'] and want[2]['exp_avg'] == want[1]['exp_avg'] and want[3]['params'] != want[2]['params']
    assert [float.fromhex(s['ls_log2']) for s in want] == ([-2.0, -2.0, -6.0, -6.0 + 1 / 256] if precision == 'fp16' else [-2.0] * 4)
    for k, (w, g) in enumerate(zip(want, got)):
        for field in w:
            assert w[field] == g[field], (precision, f'step {k + 1}', field, [i for i, (a, b) in enumerate(zip(w[field], g[field])) if a != b] if isinstance(w[field], list) else (w[field], g[field]))
    assert len(got) == len(want) == 4

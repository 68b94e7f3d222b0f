"""CPU: what requires_grad_(False) takes out of the backward's launch schedule (engine.lowest_block, _GradBuckets rule 5), on the trace kit
tests/engine_trace.py with its geometry (T = 4, 32 x 48, D = 64, depth 3, 2 clips, S = 7).

A frozen parameter costs nothing: no launch whose only products are its gradient, no bucket view, and the chain stops below the lowest block that
holds a wanted parameter.  The schedule with every parameter trainable is pinned elsewhere (tests/test_engine_host.py, tests/test_input_grad_host.py,
tests/test_ddp_gloo.py); here every frozen schedule is compared with the all-trainable one of the same net, recorded in the same test."""
import json
import os
import re

import pytest
import torch

import engine_trace as kit
from conftest import ROOT
from tcow_amd import _lib, engine

S = (kit.H // 16) * (kit.W // 16) + 1
ROWS = kit.CLIPS * kit.T * S
ATTN_BWD = ('tcow_attn_temporal_bwd', 'tcow_attn_spatial_bwd')
TN = ('tcow_gemm_tn', 'tcow_gemm_tn_grouped', 'tcow_gemm_tn_grouped_workspace_bytes')
LN_DGAMMA, LN_DBETA, LN_COLSUM = 16, 17, 25                            # positions in a normalised tcow_layernorm_bwd call
BLK = 'seeker.tracker_backbone.timesformer.model.blocks.%d.'
NETS = [('bf16', {}), ('fp32', {}), ('bf16', dict(ca=0, attention_type='joint_space_time')), ('fp32', dict(ca=0, attention_type='joint_space_time'))]
DIVIDED = NETS[:2]
IDS = lambda v: '%s-%s' % (v[0], 'joint' if v[1] else 'divided')


def name_of(net, p):
    return next(n for n, q in net.named_parameters() if q is p)


def freeze(net, frozen):
    """requires_grad_(not frozen(name)) on every parameter; returns the names left trainable."""
    left = []
    for n, p in net.named_parameters():
        p.requires_grad_(not frozen(n))
        if p.requires_grad:
            left.append(n)
    return left


class Run:
    """One forward + backward through SeekerFunction: fwd / bwd = the normalised calls of each half, events = the backward's raw events (with the hook's
    publishes and finish), blocks = which of sv['blocks'] were None right behind the forward."""

    def __init__(self, net, monkeypatch, frozen=None, rgb_grad=False, qm_grad=False, hook=True, persistent=True, flags_grad=True, groups=None):
        monkeypatch.delenv('TCOW_DDP_GROUP', raising=False)
        if groups is not None:
            monkeypatch.setenv('TCOW_DDP_GROUP', groups)
        trace = kit.install(monkeypatch)
        torch.manual_seed(0)
        self.net, self.m = net, net.train().seeker
        self.trainable = freeze(net, frozen or (lambda n: False))
        self.m.grad_hook = kit.RecordingHook(trace) if hook else None
        self.m.persistent_grads = persistent
        for p in net.parameters():
            p.grad = None
        self.rgb, self.qm = kit.clip_inputs()
        self.rgb.requires_grad_(rgb_grad); self.qm.requires_grad_(qm_grad)
        om, fl = engine.SeekerFunction.apply(self.m, self.rgb, self.qm, *self.m.param_list())
        self.blocks = [st is None for st in om.grad_fn.sv['blocks']]
        self.saved_A_pe = 'A_pe' in om.grad_fn.sv
        self.fwd = json.loads(json.dumps(trace.calls))
        trace.clear()
        (om.sum() + fl.sum() if flags_grad else om.sum()).backward()
        self.bwd, self.events = json.loads(json.dumps(trace.calls)), list(trace.events)

    def named(self, *names):
        return [c for c in self.bwd if c[0] in names]

    def publishes(self):
        return [e for e in self.events if e[0] == 'publish']

    def grouped(self):
        """The problem lists of the grouped weight-gradient launches."""
        return [c[4] for c in self.bwd if c[0] == 'tcow_gemm_tn_grouped']

    def grad_names(self):
        return sorted(n for n, p in self.net.named_parameters() if p.grad is not None)


def make(spec):
    precision, kw = spec
    return kit.make_net(precision, **kw)


def without(calls, *names):
    return [c for c in calls if c[0] not in names]


@pytest.mark.parametrize('spec', NETS, ids=IDS)
def test_all_frozen_with_input_grads(spec, monkeypatch):
    full = Run(make(spec), monkeypatch, rgb_grad=True, qm_grad=True)
    r = Run(make(spec), monkeypatch, frozen=lambda n: True, rgb_grad=True, qm_grad=True)
    assert r.fwd == full.fwd                                            # freezing changes the backward, never what the forward computes
    assert not r.named(*TN, 'tcow_colsum_grouped', 'tcow_layernorm_fold', 'tcow_embed_bwd')
    assert full.named('tcow_gemm_tn_grouped') and full.named('tcow_layernorm_fold') and full.named('tcow_embed_bwd')       # (they are there without the freeze)
    # the one small f32 product left is the flags head's adjoint towards the features; finish_late launches none
    assert len(r.named('tcow_sgemm_x3_batched')) == 1 and len(full.named('tcow_sgemm_x3_batched')) == (6 if spec[0] == 'bf16' and not spec[1] else 2)
    ln = r.named('tcow_layernorm_bwd')
    assert len(ln) == len(full.named('tcow_layernorm_bwd')) > 0
    assert all(c[LN_DGAMMA] is None and c[LN_DBETA] is None and c[LN_COLSUM] is None for c in ln)
    assert r.publishes() == [] and r.events.count(('finish',)) == 1 and r.events[-1] == ('finish',)
    chain = ('tcow_gemm_nt',) + ATTN_BWD
    assert r.named(*chain) == full.named(*chain)                          # the input-gradient chain, call for call
    assert r.bwd[-1][0] == 'tcow_col2im' and r.rgb.grad is not None and r.qm.grad is not None
    assert r.grad_names() == [] and r.blocks == [False] * kit.DEPTH and r.saved_A_pe


@pytest.mark.parametrize('k', [1, kit.DEPTH - 1])
@pytest.mark.parametrize('spec', NETS, ids=IDS)
def test_prefix_frozen_stops_the_chain(spec, k, monkeypatch):
    below = tuple(BLK % j for j in range(k))
    frozen = lambda n: n.startswith(below) or '.blocks.' not in n and 'post_linear' not in n and '.norm.' not in n      # embeddings and blocks < k
    full = Run(make(spec), monkeypatch)
    r = Run(make(spec), monkeypatch, frozen=frozen)
    assert r.fwd[-6:] == full.fwd[-6:] and r.blocks == [j < k for j in range(kit.DEPTH)] and not r.saved_A_pe
    per_block = lambda name: (len(full.named(name)) - (name == 'tcow_gemm_nt')) // kit.DEPTH      # (one gemm_nt, dFeat, belongs to the heads)
    for name in ('tcow_gemm_nt',) + ATTN_BWD:
        assert len(r.named(name)) == (name == 'tcow_gemm_nt') + (kit.DEPTH - k) * per_block(name), name
    assert not r.named('tcow_embed_bwd', 'tcow_col2im', 'tcow_col2im_channels')
    tags = [e[1] for e in r.publishes()]
    assert tags == (['g%d' % k, 'fold'] if spec[0] == 'bf16' and not spec[1] else ['g%d' % k]) and 'g0' not in tags
    wanted = [p for n, p in r.net.named_parameters() if p.requires_grad and '.model.norm.' not in n]      # (model.norm takes no part: norm_embeddings is off)
    assert sum(hi - lo for _, _, (lo, hi) in r.publishes()) == 4 * sum(p.numel() for p in wanted)
    assert r.grad_names() == sorted(name_of(r.net, p) for p in wanted)
    assert r.events[-1] == ('finish',) and r.events.count(('finish',)) == 1


@pytest.mark.parametrize('groups, k, tags', [('1', 1, ['g2', 'g1', 'fold']), ('1', 2, ['g2', 'fold']), ('2,1', 1, ['g1', 'fold']), ('1', 0, ['g2', 'g1', 'fold', 'g0'])])
def test_groups_below_the_lowest_block_never_appear(groups, k, tags, monkeypatch):
    """Several gradient groups (TCOW_DDP_GROUP): block k is the bottom block of its group, the groups wholly below it are not opened; k = 0 with frozen
    embeddings keeps the parent's tags."""
    below = tuple(BLK % j for j in range(k))
    frozen = lambda n: n.startswith(below) or '.blocks.' not in n and 'post_linear' not in n and '.norm.' not in n
    r = Run(kit.make_net('bf16'), monkeypatch, frozen=frozen, groups=groups)
    assert [e[1] for e in r.publishes()] == tags
    wanted = [p for n, p in r.net.named_parameters() if p.requires_grad and '.model.norm.' not in n]
    assert sum(hi - lo for _, _, (lo, hi) in r.publishes()) == 4 * sum(p.numel() for p in wanted)
    ranges = sorted(e[2] for e in r.publishes())
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))          # distinct buffers
    assert len(r.named('tcow_gemm_tn_grouped')) == sum(t.startswith('g') for t in tags)      # one flush per group that runs
    assert r.events[-1] == ('finish',)


@pytest.mark.parametrize('flags', [False, True])
@pytest.mark.parametrize('spec', DIVIDED, ids=IDS)
def test_heads_only_stops_behind_the_head_products(spec, flags, monkeypatch):
    r = Run(make(spec), monkeypatch, frozen=lambda n: 'post_linear' not in n, flags_grad=flags)
    assert r.blocks == [True] * kit.DEPTH
    names = [c[0] for c in r.bwd]
    tail = names[names.index('tcow_gemm_tn') + 1:]                       # behind the mask head's weight gradient: the flags head's, when it has a seed
    assert tail == (['tcow_sgemm_x3_batched'] if flags else [])
    assert not r.named('tcow_gemm_nt', 'tcow_layernorm_bwd', *ATTN_BWD)
    assert [e[1] for e in r.publishes()] == ['g%d' % kit.DEPTH] and r.events[-1] == ('finish',)
    assert len(r.grad_names()) == (4 if flags else 2)


def test_final_norm_alone_keeps_the_feature_gradient(monkeypatch):
    r = Run(kit.make_net('bf16', norm_embeddings=True), monkeypatch, frozen=lambda n: '.model.norm.bias' not in n)
    ln = r.named('tcow_layernorm_bwd')
    assert len(ln) == 1 and ln[0][LN_DGAMMA] == ln[0][LN_DBETA] == 'ptr' and not r.named(*ATTN_BWD, *TN)
    assert r.grad_names() == ['seeker.tracker_backbone.timesformer.model.norm.bias']


def tn_index(spec, block, name):
    """Position of a Linear's problem in the kit's one grouped launch: blocks from the top, each in the order the backward queues them."""
    if spec[1]:
        order = ['fc2', 'fc1', 'proj', 'qkv']
    else:
        order = ['fc2', 'fc1', 'proj', 'qkv'] + (['fold'] if spec[0] == 'bf16' else ['tfc', 'tproj']) + ['tqkv']
    return (kit.DEPTH - 1 - block) * len(order) + order.index(name)


def same_but_grouped(r, full):
    """Every call outside the grouped weight-gradient launch (and its size query) equals the all-trainable run's."""
    skip = ('tcow_gemm_tn_grouped', 'tcow_gemm_tn_grouped_workspace_bytes')
    return r.fwd == full.fwd and without(r.bwd, *skip) == without(full.bwd, *skip)


@pytest.mark.parametrize('spec', NETS, ids=IDS)
def test_one_linear_frozen_in_the_middle(spec, monkeypatch):
    full = Run(make(spec), monkeypatch)
    r = Run(make(spec), monkeypatch, frozen=lambda n: n.startswith(BLK % 1 + 'mlp.fc1.'))
    (want,), (got,) = full.grouped(), r.grouped()
    i = tn_index(spec, 1, 'fc1')
    assert (want[i]['N'], want[i]['K']) == (4 * kit.D, kit.D)
    assert got == want[:i] + want[i + 1:]
    assert same_but_grouped(r, full) and not r.named('tcow_colsum_grouped')
    assert len(r.grad_names()) == len(full.grad_names()) - 2


@pytest.mark.parametrize('spec', NETS, ids=IDS)
def test_weight_frozen_bias_trainable_is_a_column_sum(spec, monkeypatch):
    full = Run(make(spec), monkeypatch)
    r = Run(make(spec), monkeypatch, frozen=lambda n: n == BLK % 1 + 'attn.qkv.weight')
    (want,), (got,) = full.grouped(), r.grouped()
    i = tn_index(spec, 1, 'qkv')
    assert got == want[:i] + want[i + 1:]                                # in no TnProblem
    (call,) = r.named('tcow_colsum_grouped')
    assert call[2:5] == [_lib.TCOW_F32 if spec[0] == 'fp32' else _lib.TCOW_BF16, 1, [dict(M=ROWS, N=3 * kit.D, dY='ptr', lddy=3 * kit.D, out='ptr', accumulate=0)]]
    bias = dict(r.net.named_parameters())[BLK % 1 + 'attn.qkv.bias']
    (ev,) = [e for e in r.events if e[:2] == ('call', 'tcow_colsum_grouped')]
    assert bias.grad.data_ptr() in ev[2]                                 # the sum lands in the bias's bucket view
    names = [c[0] for c in r.bwd]
    at = names.index('tcow_gemm_tn_grouped')                             # it flushes with the GEMMs of its group
    assert names[at + 1:at + 4] == ['tcow_colsum_grouped_workspace_bytes', 'tcow_colsum_grouped', 'tcow_layernorm_fold']
    skip = ('tcow_gemm_tn_grouped', 'tcow_gemm_tn_grouped_workspace_bytes', 'tcow_colsum_grouped', 'tcow_colsum_grouped_workspace_bytes')
    assert r.fwd == full.fwd and without(r.bwd, *skip) == without(full.bwd, *skip)
    assert dict(r.net.named_parameters())[BLK % 1 + 'attn.qkv.weight'].grad is None


@pytest.mark.parametrize('spec', NETS, ids=IDS)
def test_weight_trainable_bias_frozen_has_no_bias_gradient(spec, monkeypatch):
    full = Run(make(spec), monkeypatch)
    r = Run(make(spec), monkeypatch, frozen=lambda n: n == BLK % 1 + 'attn.qkv.bias')
    (want,), (got,) = full.grouped(), r.grouped()
    i = tn_index(spec, 1, 'qkv')
    assert want[i]['bias_grad'] == 'ptr' and got[i] == dict(want[i], bias_grad=None)
    assert got[:i] + got[i + 1:] == want[:i] + want[i + 1:]
    assert same_but_grouped(r, full) and not r.named('tcow_colsum_grouped')


def test_layernorm_with_one_parameter_frozen_writes_the_other_to_scratch(monkeypatch):
    full = Run(kit.make_net('bf16'), monkeypatch)
    r = Run(kit.make_net('bf16'), monkeypatch, frozen=lambda n: n == BLK % 1 + 'norm2.bias')
    assert r.fwd == full.fwd and r.bwd == full.bwd                       # the pair is computed as before ...
    folds = [p for e in r.events if e[:2] == ('call', 'tcow_layernorm_fold') for p in e[2]]
    w = dict(r.net.named_parameters())[BLK % 1 + 'norm2.weight']
    assert w.grad.data_ptr() in folds and dict(r.net.named_parameters())[BLK % 1 + 'norm2.bias'].grad is None
    published = sum(hi - lo for _, _, (lo, hi) in r.publishes())
    assert published == sum(hi - lo for _, _, (lo, hi) in full.publishes()) - 4 * kit.D      # ... and the frozen half lies in no bucket


def late_launches(r):
    """Problem counts of finish_late's small f32 products (the flags head's two come first)."""
    return [c[2] for c in r.named('tcow_sgemm_x3_batched')][2:]


def test_fold_triple_frozen_leaves_the_late_launches(monkeypatch):
    triple = (BLK % 1 + 'temporal_attn.proj.weight', BLK % 1 + 'temporal_attn.proj.bias', BLK % 1 + 'temporal_fc.weight')
    full = Run(kit.make_net('bf16'), monkeypatch)
    r = Run(kit.make_net('bf16'), monkeypatch, frozen=lambda n: n in triple)
    assert late_launches(full) == [kit.DEPTH] * 4 and late_launches(r) == [kit.DEPTH - 1] * 4
    (want,), (got,) = full.grouped(), r.grouped()
    i = tn_index(('bf16', {}), 1, 'fold')
    assert got == want[:i] + want[i + 1:]                                # block 1 queues no dW' product
    skip = ('tcow_gemm_tn_grouped', 'tcow_gemm_tn_grouped_workspace_bytes', 'tcow_sgemm_x3_batched')
    assert without(r.bwd, *skip) == without(full.bwd, *skip)
    # one of the three wanted: the product is queued, and only that output's launch carries block 1
    r = Run(kit.make_net('bf16'), monkeypatch, frozen=lambda n: n in triple[:2])
    assert r.grouped() == full.grouped() and late_launches(r) == [kit.DEPTH, kit.DEPTH, kit.DEPTH - 1, kit.DEPTH - 1]


def test_tfc_bias_alone_rides_on_a_scratch_layernorm_pass(monkeypatch):
    r = Run(kit.make_net('bf16'), monkeypatch, frozen=lambda n: n != BLK % 1 + 'temporal_fc.bias')
    assert r.blocks == [True, False, False]
    ln = r.named('tcow_layernorm_bwd')                                   # blocks 2 and 1: n2, n1, tn each
    assert len(ln) == 6
    for j, c in enumerate(ln):
        if j == 4:                                                       # block 1's n1: the column sum needs the parameter-gradient pass
            assert c[LN_DGAMMA] == c[LN_DBETA] == c[LN_COLSUM] == 'ptr'
        else:
            assert c[LN_DGAMMA] is c[LN_DBETA] is c[LN_COLSUM] is None
    (fold,) = r.named('tcow_layernorm_fold')
    assert fold[2] == 1 and fold[3][0]['colsum_out'] == 'ptr'
    bias = dict(r.net.named_parameters())[BLK % 1 + 'temporal_fc.bias']
    (ev,) = [e for e in r.events if e[:2] == ('call', 'tcow_layernorm_fold')]
    (lo, hi), = [e[2] for e in r.publishes()]
    assert bias.grad.data_ptr() == lo and hi - lo == 4 * kit.D           # the bucket is that bias alone: dgamma / dbeta went to scratch
    assert sum(lo <= p < hi for p in ev[2]) == 1
    assert not r.named(*TN, 'tcow_colsum_grouped') and r.grad_names() == [BLK % 1 + 'temporal_fc.bias']


@pytest.mark.parametrize('persistent', [False, True])
@pytest.mark.parametrize('spec', DIVIDED, ids=IDS)
def test_grad_is_none_exactly_for_frozen_parameters(spec, persistent, monkeypatch):
    net = make(spec)
    frozen = lambda n: n.startswith(BLK % 0) or n.endswith('mlp.fc2.weight') or n.endswith('norm1.bias') or 'pos_embed' in n
    r = Run(net, monkeypatch, frozen=frozen, hook=False, persistent=persistent)
    for n, p in net.named_parameters():
        if '.model.norm.' in n:
            continue                                                     # (takes no part: norm_embeddings is off)
        assert (p.grad is None) == frozen(n), n
        if p.grad is not None:
            assert p.grad.shape == p.shape and p.grad.dtype == torch.float32
    # a gradient a frozen parameter already had is what it was
    p0 = dict(net.named_parameters())[BLK % 0 + 'mlp.fc1.bias']
    keep = torch.full_like(p0, 7.0)
    p0.grad = keep.clone()
    om, fl = engine.SeekerFunction.apply(r.m, r.rgb.detach(), r.qm.detach(), *r.m.param_list())
    (om.sum() + fl.sum()).backward()
    assert torch.equal(p0.grad, keep)


def test_the_frozen_set_is_read_by_the_forward(monkeypatch):
    net = kit.make_net('bf16')
    trace = kit.install(monkeypatch)
    m = net.train().seeker
    freeze(net, lambda n: n.startswith(BLK % 0))
    om, fl = engine.SeekerFunction.apply(m, *kit.clip_inputs(), *m.param_list())
    for p in net.parameters():
        p.requires_grad_(True)                                           # thawed between forward and backward: this backward does not see it
    (om.sum() + fl.sum()).backward()
    assert all((p.grad is None) == n.startswith(BLK % 0) for n, p in net.named_parameters() if '.model.norm.' not in n and '.blocks.' in n)


def test_lowest_block():
    lay = kit.make_net('fp32').seeker.layout
    every = frozenset(range(lay.count))
    assert engine.lowest_block(lay, every, (False, False)) == lay.depth
    assert engine.lowest_block(lay, every, (False, True)) == 0 and engine.lowest_block(lay, every - {lay.pos}, (False, False)) == 0
    assert engine.lowest_block(lay, every - {lay.at(2, 'fc2', 1), lay.at(1, 'tn')}, (False, False)) == 1
    assert engine.lowest_block(lay, every - {lay.head_w, lay.norm_b}, (False, False)) == lay.depth


def test_abi_has_the_grouped_column_sum():
    hdr = open(os.path.join(ROOT, 'include', 'tcow_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+tcow_colsum_grouped\s*\(\s*void\*\s*stream,\s*int\s+dtype,\s*int\s+n,\s*const\s+tcow_colsum_problem\*', code)
    assert re.search(r'\blong\s+tcow_colsum_grouped_workspace_bytes\s*\(', code)
    assert {'tcow_colsum_grouped', 'tcow_colsum_grouped_workspace_bytes'} <= set(_lib.SIGNATURES)
    assert [f for f, _ in _lib.ColsumProblem._fields_] == ['M', 'N', 'dY', 'lddy', 'out', 'accumulate']
    assert _lib.ABI_VERSION == 16 and int(re.search(r'#define\s+TCOW_ABI_VERSION\s+(\d+)', hdr).group(1)) == 16      # (14 when this symbol arrived, no signature changed; 15: the optimizer step became one entry point; 16: the stream step did)
    for fmt in ('bf16', 'fp16'):
        lib = _lib.lib(fmt)
        assert lib.tcow_version() == 16 and lib.tcow_colsum_group_max() == 16

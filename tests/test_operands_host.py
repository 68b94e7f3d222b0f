"""CPU: the bookkeeping of tcow_amd.operands.OperandCache (what is current, epoch, generation, consumed-once, keep-alive, the re-cast table) on CPU
tensors, with the three launches the cache makes replaced by recording stand-ins.  The built library is needed for tcow_cast_desc_bytes only."""
import struct

import pytest
import torch

from tcow_amd import _lib, ops
from tcow_amd.operands import OperandCache

BF16 = ops.BF16
REC = '<QQQiiii'          # tcow_cast_desc: source, Wc, Wt pointers; N, K, first tile, tile edge


@pytest.fixture
def log(monkeypatch):
    """The launches, in order: ('cast', N, K) / ('batched', decoded records, n, tiles) / ('sgemm', problems)."""
    out = []

    def cast_transpose(mode, W, Wc=None, Wt=None):
        out.append(('cast',) + tuple(W.shape))
        if Wc is not None:
            Wc.copy_(W.to(ops.tdtype(mode)))
        if Wt is not None:
            Wt.copy_(W.to(ops.tdtype(mode)).t())

    def cast_transpose_batched(mode, table, n, total_tiles):
        raw = bytes(table.numpy().tobytes())
        assert len(raw) == n * struct.calcsize(REC)
        out.append(('batched', [struct.unpack_from(REC, raw, i * struct.calcsize(REC)) for i in range(n)], n, total_tiles))

    def sgemm_batched(problems, accumulate=False):
        out.append(('sgemm', len(problems)))
        for A, B, C in problems:
            C.copy_(C + A @ B if accumulate else A @ B)

    monkeypatch.setattr(ops, 'cast_transpose', cast_transpose)
    monkeypatch.setattr(ops, 'cast_transpose_batched', cast_transpose_batched)
    monkeypatch.setattr(ops, 'sgemm_batched', sgemm_batched)
    return out


def _param(n, k, seed=0):
    return torch.nn.Parameter(torch.randn(n, k, generator=torch.Generator().manual_seed(seed)))


def _bump(p):
    with torch.no_grad():
        p.mul_(1.5)               # in place: the version counter moves


def test_record_layout_matches_the_library():
    assert struct.calcsize(REC) == int(_lib.lib().tcow_cast_desc_bytes())


def test_a_copy_is_current_until_version_epoch_or_mode_moves(log):
    c, p = OperandCache(), _param(64, 128)
    Wc, Wt = c.weight(BF16, p, False)
    assert log == [('cast', 64, 128)] and Wt is None and torch.equal(Wc, p.detach().to(torch.bfloat16))
    assert c.weight(BF16, p, False)[0] is Wc and len(log) == 1                 # unchanged weight: a hit, no launch
    _bump(p)
    Wc2, _ = c.weight(BF16, p, False)
    assert len(log) == 2 and torch.equal(Wc2, p.detach().to(torch.bfloat16))   # version bump: ONE launch
    assert c.weight(BF16, p, False)[0] is Wc2 and len(log) == 2
    with torch.no_grad():
        p.data.mul_(2.0)                                                        # .data: no version bump, only the epoch tells the cache
    assert c.weight(BF16, p, False)[0] is Wc2 and len(log) == 2
    c.invalidate(BF16)                                                          # nothing registered: no batched launch, but every copy is stale
    assert len(log) == 2 and c.epoch == 1
    Wc3, _ = c.weight(BF16, p, False)
    assert len(log) == 3 and torch.equal(Wc3, p.detach().to(torch.bfloat16))
    Wh, _ = c.weight(ops.FP16, p, False)                                        # another mode: not current
    assert len(log) == 4 and Wh.dtype == torch.float16
    assert c.generation == 0 and not c.registry                                # eval lookups register nothing and move nothing


def test_f32_mode_serves_the_master_and_casts_only_the_transpose(log):
    c, p = OperandCache(), _param(64, 64)
    Wc, Wt = c.weight(ops.F32, p, False)
    assert log == [] and Wt is None and Wc.data_ptr() == p.data_ptr()
    Wc, Wt = c.weight(ops.F32, p, True)
    assert len(log) == 1 and torch.equal(Wt, p.detach().t()) and c.registry[id(p)][1] is None      # (no Wc record: refresh writes W^T only)


def test_eval_then_training_lookup_allocates_wt_and_registers(log):
    c, p = OperandCache(), _param(64, 128)
    assert c.weight(BF16, p, False)[1] is None and not c.registry and c.generation == 0
    Wc, Wt = c.weight(BF16, p, True)
    assert len(log) == 2 and Wt.shape == (128, 64) and torch.equal(Wt, Wc.t())
    src, rWc, rWt, N, K = c.registry[id(p)]
    assert src is p and rWc is Wc and rWt is Wt and (N, K) == (64, 128) and c.generation == 1
    assert c.weight(BF16, p, False) == (Wc, Wt) and c.weight(BF16, p, True)[1] is Wt and len(log) == 2 and c.generation == 1


def _fold_q(D, seed=0):
    torch.manual_seed(seed)
    proj, fc = torch.nn.Linear(D, D), torch.nn.Linear(D, D)
    return [proj.weight, proj.bias, fc.weight], dict(tproj=0, tfc=2)


def test_generation_moves_on_registration_and_drop_only(log):
    c, p, p2 = OperandCache(), _param(64, 64), _param(64, 64, 1)
    q, ix = _fold_q(64)
    seen = [c.generation]
    step = lambda: seen.append(c.generation) or seen[-1] - seen[-2]
    c.weight(BF16, p, False); assert step() == 0                 # eval lookup
    c.weight(BF16, p, True); assert step() == 1                  # training registration
    c.weight(BF16, p, True); assert step() == 0                  # hit
    c.weight(BF16, p2, True); assert step() == 1                 # another weight registers
    c.folded(BF16, 0, q, ix, True); assert step() == 0           # (the fold registers buffers of its own: not a plain weight)
    c.constant(('mask0', 1, 2, 'cpu'), lambda: torch.ones(3)); assert step() == 0
    c.buffer(('gbuf', 0, 4, 'cpu'), lambda: torch.empty(4)); assert step() == 0
    c.optimizer_wrote(frozenset([id(p)])); c.invalidate(BF16); c.refresh(BF16); c.keep_alive(); assert step() == 0
    _bump(p); c.weight(BF16, p, True); assert step() == 1        # re-allocated copies register again
    c.drop(buckets=False); assert step() == 1
    c.drop(); assert step() == 1


def test_refresh_skips_what_the_optimizer_wrote_exactly_once(log):
    c = OperandCache()
    ps = [_param(64, 64, i) for i in range(3)]
    copies = [c.weight(BF16, p, True) for p in ps]
    del log[:]
    c.optimizer_wrote(frozenset(id(p) for p in ps[:2]))
    for p in ps:
        _bump(p)
    c.invalidate(BF16)
    (kind, recs, n, tiles), = log
    assert kind == 'batched' and n == 1 and tiles == 1 and recs[0][:3] == (ps[2].data_ptr(), copies[2][0].data_ptr(), copies[2][1].data_ptr())
    for p, (Wc, Wt) in zip(ps, copies):                         # every registered copy is stamped current, the skipped ones included: hits, no launch
        assert c.weight(BF16, p, True) == (Wc, Wt)
    assert len(log) == 1
    c.invalidate(BF16)                                          # the declared set was consumed: nothing is skipped now
    assert len(log) == 2 and log[1][2] == 3 and [r[0] for r in log[1][1]] == [p.data_ptr() for p in ps]
    c.optimizer_wrote(frozenset(id(p) for p in ps))             # everything written by the optimizer: no launch at all, stamps refreshed
    _bump(ps[0]); c.invalidate(BF16)
    assert len(log) == 2 and c.weight(BF16, ps[0], True) == copies[0] and len(log) == 2


@pytest.mark.parametrize('shapes, edge, tiles', [([(128, 64), (64, 192)], 64, [2, 3]), ([(128, 64), (64, 192), (96, 32)], 32, [8, 12, 3])])
def test_table_records_and_tile_total(log, shapes, edge, tiles):
    c = OperandCache()
    ps = [_param(n, k, i) for i, (n, k) in enumerate(shapes)]
    copies = [c.weight(BF16, p, True) for p in ps]
    del log[:]
    c.refresh(BF16)
    (kind, recs, n, total), = log
    assert kind == 'batched' and n == len(shapes) == c.table[2] and total == sum(tiles) == c.table[3]
    first = 0
    for p, (Wc, Wt), (N, K), t, rec in zip(ps, copies, shapes, tiles, recs):
        assert rec == (p.data_ptr(), Wc.data_ptr(), Wt.data_ptr(), N, K, first, edge)
        first += t


def test_table_is_reused_until_a_buffer_moves(log):
    c = OperandCache()
    ps = [_param(64, 64, i) for i in range(2)]
    for p in ps:
        c.weight(BF16, p, True)
    c.refresh(BF16)
    tab = c.table
    c.invalidate(BF16)
    assert c.table is tab and c.table[1] is tab[1]                 # same pointers: the device records are not rebuilt
    keep = c.keep_alive()                                          # holds the old copies: the new ones cannot land on their addresses
    old = c.weight(BF16, ps[0], True)
    _bump(ps[0])
    new = c.weight(BF16, ps[0], True)
    assert new[0].data_ptr() != old[0].data_ptr() and keep[id(ps[0])][2] is old[0] and keep[id(ps[0])][3] is old[1]
    c.refresh(BF16)
    assert c.table is not tab and log[-1][1][0][1:3] == (new[0].data_ptr(), new[1].data_ptr())
    tab2 = c.table
    c.refresh(ops.FP16)                                            # the mode is part of the signature
    assert c.table is not tab2


def test_folded_projection_products_registration_and_chunks(log):
    c = OperandCache()
    q, ix = _fold_q(64)
    Wc, Wt, b = c.folded(BF16, 0, q, ix, False)
    W32 = q[2].detach() @ q[0].detach()
    assert log == [('sgemm', 1), ('sgemm', 1), ('cast', 64, 64)] and Wt is None and not c.registry and not c.folds
    assert torch.equal(Wc, W32.to(torch.bfloat16)) and torch.allclose(b, q[2].detach() @ q[1].detach())
    assert c.folded(BF16, 0, q, ix, False)[0] is Wc and len(log) == 3
    Wc2, Wt2, _ = c.folded(BF16, 0, q, ix, True)                  # training: W^T appears in the SAME entry, registered with W32 as the re-cast's source
    ent = c.folds[('fold', 0)]
    assert Wc2 is Wc and Wt2 is not None and len(log) == 6 and c.registry[('fold', 0)] == (ent['W32'], Wc, Wt2, 64, 64) and c.copies[('fold', 0)] is ent
    _bump(q[2])
    for i in range(1, 25):                                         # 25 live folds: the products go in chunks of 24
        c.folded(BF16, i, *_fold_q(8, i), True)
    del log[:]
    c.invalidate(BF16)
    assert [e[:2] for e in log[:4]] == [('sgemm', 24), ('sgemm', 24), ('sgemm', 1), ('sgemm', 1)] and log[4][0] == 'batched' and len(log) == 5
    assert log[4][2] == 25 and log[4][1][0][0] == ent['W32'].data_ptr() and log[4][1][0][6] == 32
    assert torch.allclose(ent['W32'], q[2].detach() @ q[0].detach())
    assert c.folded(BF16, 0, q, ix, True)[0] is Wc and len(log) == 5         # stamped: a hit


def test_drop_empties_everything_and_buckets_false_keeps_the_buckets(log):
    c, p = OperandCache(), _param(64, 64)
    q, ix = _fold_q(64)
    c.weight(BF16, p, True); c.folded(BF16, 0, q, ix, True); c.refresh(BF16)
    c.constant(('mask0', 1, 2, 'cpu'), lambda: torch.ones(3))
    buf = c.buffer(('gbuf', 0, 4, 'cpu'), lambda: torch.empty(4))
    assert c.buffer(('gbuf', 0, 4, 'cpu'), lambda: torch.empty(4)) is buf
    c.optimizer_wrote(frozenset([id(p)]))
    assert c.copies and c.registry and c.folds and c.table is not None and c.buckets
    gen = c.generation
    c.drop(buckets=False)
    assert not c.copies and not c.registry and not c.folds and c.table is None and c.buckets == {('gbuf', 0, 4, 'cpu'): buf} and c.generation == gen + 1
    del log[:]
    c.weight(BF16, p, True); c.invalidate(BF16)
    assert log[-1][0] == 'batched' and log[-1][2] == 1             # (the declared set went with the drop: the weight is re-cast)
    c.drop()
    assert not c.copies and not c.registry and not c.folds and c.table is None and not c.buckets and c.generation == gen + 3


def test_a_replica_private_instance_leaves_the_original_untouched(log):
    c, p = OperandCache(), _param(64, 64)
    c.weight(BF16, p, True); c.buffer('b', lambda: torch.empty(1)); c.invalidate(BF16)
    before = (dict(c.copies), dict(c.registry), dict(c.buckets), c.table, c.generation, c.epoch)
    r = c.fresh()
    assert r is not c and r.generation == c.generation + 1 and r.epoch == c.epoch and not r.copies and not r.registry and not r.buckets
    r.weight(BF16, p, True); r.buffer('b', lambda: torch.empty(1)); r.buffer('c', lambda: torch.empty(1)); r.invalidate(BF16); r.drop()
    assert (c.copies, c.registry, c.buckets, c.table, c.generation, c.epoch) == before


def _net():
    from tcow_amd.seeker import Seeker
    return Seeker(None, num_total_frames=4, frame_height=32, frame_width=48, network_depth=1, embed_dim=64, num_heads=1, causal_attention=1,
                  drop_path_rate=0.0, precision='fp32')


def test_module_owns_one_cache_and_set_precision_keeps_the_gradient_buckets():
    sk = _net().seeker
    od = sk._operands
    assert isinstance(od, OperandCache)
    assert sk._replicate_for_data_parallel()._operands is od        # a replica's __dict__ aliases the original's: why forward() binds a fresh() one
    od.constant(('mask0', 1, 4, 'cpu'), lambda: torch.ones(3))
    buf = od.buffer(('gbuf', 0, 4, 'cpu'), lambda: torch.empty(4))
    gen = od.generation
    sk.set_precision('bf16')
    assert sk._operands is od and not od.copies and od.buckets == {('gbuf', 0, 4, 'cpu'): buf} and od.generation == gen + 1
    sk.invalidate_weight_cache()
    assert od.epoch == 1 and od.generation == gen + 1
    sk.float()                                                      # Module._apply: everything goes, the buckets too
    assert sk._operands is od and not od.buckets and od.generation == gen + 2 and sk.__dict__.get('_param_list_cache') is None


def test_handoff_attributes_are_declared():
    sk = _net().seeker
    assert {k: sk.__dict__[k] for k in ('_optim_ref', 'pending_inv_scale', '_defer_unscale', '_warned_ls')} == \
        dict(_optim_ref=None, pending_inv_scale=None, _defer_unscale=True, _warned_ls=False)
    assert sk._live_optim() is None

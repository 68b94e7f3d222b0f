"""tcow_attn_probs (csrc/attention_probs.hip) through ops.attn_probs, against a float64 softmax of the same stored q and k (attn_probs_kit.py).

The tolerance is derived, not chosen: delta = 66 u max_ij sum_c |q_c k_c| / 8 (u = 2^-24) covers the f32 dot product of 64 terms and the scale;
|P - P64| <= P64 (expm1(2 delta) + (n_keys + 8) u) + 1e-30.  Storage types: bf16 and f32 from the main library, binary16 from the fp16 build;
q and k are drawn N(0, 1) and rounded to the storage type before both sides see them.

Shapes are (B, T, S, heads, causal).  The temporal kernel walks the keys in trips of TEMPORAL_TRIP = 64 (one key per lane, AP_TKEYS); the rows
kernel in batches of ROWS_BATCH[storage] = G * AP_U keys (G = 8 lane groups for 16-bit lines, 4 for f32, AP_U = 4 batches in flight)."""
import pytest
import torch

import attn_probs_kit as kit
from test_gpu_attention import TOL

STORAGES = ['f32', 'bf16', 'fp16']
TEMPORAL_TRIP = 64
ROWS_BATCH = {'f32': 16, 'bf16': 32, 'fp16': 32}

TEMPORAL = [
    (1, 1, 2, 1, 1), (1, 2, 2, 1, 1),                                           # single key, trivial softmax
    *[(2, 30, 5, 2, ca) for ca in (-1, 0, 1, 2, 3, 5, 40)],                     # non-power-of-two T, every mask kind; 40 = look-ahead past the end
    (1, 64, 3, 1, 1), (1, 65, 3, 2, 1),                                         # one wave's lanes, exactly and one over
    (1, 130, 2, 1, 3), (1, 130, 2, 1, 0),                                       # multi-trip key loop, masked and not
    (2, 7, 3, 3, 1),                                                            # addressing across clips, slots and heads at once
    # one, two and three trips of TEMPORAL_TRIP keys with and without a remainder (64 and 65 above: one trip, one trip + 1); 128 % 4 == 0 takes
    # the 16-byte stores in the two-pass path, 129 / 193 the scalar ones
    (1, 2 * TEMPORAL_TRIP, 2, 1, 1), (1, 2 * TEMPORAL_TRIP + 1, 2, 1, 1), (1, 3 * TEMPORAL_TRIP, 2, 1, 0), (1, 3 * TEMPORAL_TRIP + 1, 2, 1, 2),
    (1, 63, 2, 1, 1), (1, 60, 2, 2, 1),                                         # a remainder inside the single trip: scalar and 16-byte stores
]
ROWS = [
    (1, 1, 2, 1, 0), (1, 2, 2, 1, 2),                                           # cls in / out at the smallest S; S = 2, ca = 2: a single key
    (2, 3, 5, 2, 1),                                                            # generic
    (1, 2, 65, 2, 0), (1, 2, 66, 1, 2),                                         # around one wave of keys
    (1, 1, 301, 2, 1),                                                          # the workload's S
    (1, 1, 1025, 1, 0),                                                         # a joint-like long sequence, many loop trips
    (1, 2, 33, 1, 1), (1, 2, 34, 1, 2), (1, 1, 17, 1, 0), (1, 1, 18, 1, 2),     # L = 33 / 33 / 17 / 17: one ROWS_BATCH plus one key, both storages
]
_tid = lambda s: 'B%d_T%d_S%d_h%d_c%d' % s


@pytest.fixture(scope='module')
def ops(cuda):
    from tcow_amd import ops as o
    return o


def tables(L):
    """Query tables of a sequence of L positions: a single entry, every position, repeated entries, unsorted entries."""
    every = list(range(L)) if L <= 130 else list(range(0, L, 37)) + [L - 1]
    return {'single': [L // 2], 'every': every, 'repeated': [0, L - 1, 0, 0, L - 1], 'unsorted': [L - 1, 0, L // 3, L // 2, 1 % L]}


class Run:
    def __init__(self, ops, dev, mname, shape, seed=0, zero_q=False):
        self.ops, self.dev, self.mname = ops, dev, mname
        self.B, self.T, self.S, self.H, self.ca = shape
        mode, self.dt = kit.storage(ops, mname)
        self.shape = ops.attn_shape(mode, self.B, self.T, self.S, self.H * 64, self.H, self.ca)
        self.qkv = kit.draw_qkv(self.B, self.T, self.S, self.H, self.dt, dev, seed, zero_q)
        self.M = self.B * self.T * self.S
        self.s0 = 0 if self.ca in (0, 1) else 1

    def temporal(self, with_lse=True):
        out = torch.full((self.B, self.S - 1, self.H, self.T, self.T), float('nan'), device=self.dev)
        lse = torch.full((self.M, self.H), float('nan'), device=self.dev) if with_lse else None
        self.ops.attn_probs(self.shape, False, self.qkv, out, lse)
        return out, lse

    def rows(self, pos, with_lse=True):
        p = torch.tensor(pos, dtype=torch.int32, device=self.dev)
        out = torch.full((self.B * self.T, len(pos), self.H, self.S), float('nan'), device=self.dev)
        lse = torch.full((self.B * self.T, len(pos), self.H), float('nan'), device=self.dev) if with_lse else None
        self.ops.attn_probs(self.shape, True, self.qkv, out, lse, p)
        return out, lse

    def ref(self, spatial, pos=None):
        return kit.ref64(self.qkv, self.B, self.T, self.S, self.H, self.ca, spatial, pos)


def check(label, got, want, bound):
    idx, g, w, d, b = kit.worst(got, want, bound)
    print(f'{label}: worst |d| {d:.3e} against bound {b:.3e} at {idx}')
    assert d <= b, f'{label}: at {idx} got {g!r}, want {w!r}, |d| {d:.3e} > bound {b:.3e}'


def temporal_lse_rows(r, ref, lse):
    """The kernel's [M, heads] table read at the sequences' rows -> [N, heads, T]; every other row must be untouched (NaN here)."""
    touched = torch.zeros(r.M, dtype=torch.bool, device=r.dev)
    touched[ref['rows'].reshape(-1)] = True
    assert torch.isnan(lse[~touched]).all(), 'lse of a slot-0 row was written'
    return lse[ref['rows']].permute(0, 2, 1)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', TEMPORAL, ids=_tid)
@pytest.mark.parametrize('mname', STORAGES)
def test_temporal_against_float64(ops, cuda, mname, shape):
    r = Run(ops, cuda, mname, shape)
    out, lse = r.temporal()
    ref = r.ref(False)
    P, keep = ref['P'].view_as(out), ref['keep'].reshape(out.shape)
    check(f'{mname} {_tid(shape)} P', out, P, kit.prob_bound(ref).view_as(out))
    # every masked entry is bit-equal to +0.0
    assert (out[~keep].view(torch.int32) == 0).all()
    check(f'{mname} {_tid(shape)} lse', temporal_lse_rows(r, ref, lse), ref['lse'], kit.lse_bound(ref))
    # two calls give bit-identical outputs; lse = None changes nothing
    out2, _ = r.temporal(with_lse=False)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', ROWS, ids=_tid)
@pytest.mark.parametrize('mname', STORAGES)
def test_rows_against_float64(ops, cuda, mname, shape):
    r = Run(ops, cuda, mname, shape)
    L = r.S - r.s0
    for name, pos in tables(L).items():
        out, lse = r.rows(pos)
        ref = r.ref(True, pos)
        check(f'{mname} {_tid(shape)} {name} P', out, ref['P'], kit.prob_bound(ref))
        if r.s0:
            assert (out[..., 0].view(torch.int32) == 0).all()                   # column 0 is +0.0 when the cls is out
        check(f'{mname} {_tid(shape)} {name} lse', lse, ref['lse'], kit.lse_bound(ref))
        out2, _ = r.rows(pos, with_lse=False)
        assert torch.equal(out.view(torch.int32), out2.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize('mname', STORAGES + ['f32x3'])
def test_zero_queries_give_uniform_rows(ops, cuda, mname):
    """q = 0: every allowed entry is 1 / n_visible to one f32 rounding, in both forms and in the two-pass paths."""
    for shape in [(2, 30, 5, 2, 1), (1, 130, 2, 1, 3), (1, 65, 3, 2, 0)]:
        r = Run(ops, cuda, mname, shape, zero_q=True)
        out, _ = r.temporal()
        keep = r.ref(False)['keep'].reshape(out.shape)
        want = 1.0 / keep.sum(-1, keepdim=True).double().expand_as(out)
        assert ((out.double() - want).abs()[keep] <= kit.U32 * want[keep]).all() and (out[~keep].view(torch.int32) == 0).all()
    for shape in [(2, 3, 5, 2, 1), (1, 2, 66, 1, 2), (1, 1, 301, 2, 1)]:
        r = Run(ops, cuda, mname, shape, zero_q=True)
        L = r.S - r.s0
        out, _ = r.rows([0, L - 1])
        assert ((out[..., r.s0:].double() - 1.0 / L).abs() <= kit.U32 / L).all()
        assert (out[..., :r.s0].view(torch.int32) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('mname', STORAGES)
def test_a_position_outside_the_sequence_gives_nan_in_its_own_rows(ops, cuda, mname):
    for shape in [(2, 3, 5, 2, 1), (1, 2, 66, 1, 2)]:
        r = Run(ops, cuda, mname, shape)
        L = r.S - r.s0
        good = [L - 1, 0, 2]
        bad = [L - 1, L, 0, -1, 2, 1 << 30]
        at = [0, 2, 4]                                                           # where the good entries stand in `bad`
        out_g, lse_g = r.rows(good)
        out_b, lse_b = r.rows(bad)
        assert torch.equal(out_b[:, at].view(torch.int32), out_g.view(torch.int32)) and torch.equal(lse_b[:, at].view(torch.int32), lse_g.view(torch.int32))
        assert torch.isnan(out_b[:, [1, 3, 5]]).all() and torch.isnan(lse_b[:, [1, 3, 5]]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('mname', STORAGES)
def test_maps_times_v_is_the_shipped_forward(ops, cuda, mname):
    """P @ V (float64, the new P with the stored V) against ops.attn_fwd on the same qkv, within the project's own bound of that forward."""
    for spatial, shape in [(False, (2, 30, 5, 2, 1)), (True, (1, 2, 66, 2, 2))]:
        r = Run(ops, cuda, mname, shape)
        ref = r.ref(spatial)
        out = torch.full((r.M, r.H * 64), float('nan'), device=cuda, dtype=r.dt)
        ops.attn_fwd(r.shape, spatial, r.qkv, out)
        if spatial:
            P = r.rows(list(range(ref['L'])), with_lse=False)[0][..., r.s0:].permute(0, 2, 1, 3)       # [G, H, L, L]
        else:
            P = r.temporal(with_lse=False)[0].reshape(-1, r.H, r.T, r.T)
        o = (P.double() @ ref['v']).permute(0, 2, 1, 3)                                                 # [N, L, H, 64]
        got = out.double().view(r.M, r.H, 64)[ref['rows']]
        d, scale = float((got - o).abs().max()), float(o.abs().max())
        print(f'{mname} spatial={spatial}: max |P V - attn_fwd| {d:.3e}, bound {TOL[mname] * scale:.3e}')
        assert d <= TOL[mname] * scale


@pytest.mark.gpu
def test_bf16x3_takes_the_f32_kernel(ops, cuda):
    shape = (2, 7, 3, 3, 1)
    a, b = Run(ops, cuda, 'f32', shape), Run(ops, cuda, 'f32x3', shape)
    assert torch.equal(a.temporal()[0].view(torch.int32), b.temporal()[0].view(torch.int32))
    assert torch.equal(a.rows([1, 0])[0].view(torch.int32), b.rows([1, 0])[0].view(torch.int32))


@pytest.mark.gpu
def test_the_wrapper_refuses_before_a_launch(ops, cuda):
    r = Run(ops, cuda, 'bf16', (1, 2, 3, 1, 1))
    out = torch.empty(1, 2, 1, 2, 2, device=cuda)
    with pytest.raises(ops.L.TcowError, match='pos must be a contiguous int32 vector'):
        ops.attn_probs(r.shape, True, r.qkv, out, pos=torch.zeros(1, dtype=torch.int64, device=cuda))
    with pytest.raises(ops.L.TcowError, match='out must hold'):
        ops.attn_probs(r.shape, False, r.qkv, out[:, :1])
    with pytest.raises(ops.L.TcowError, match='tcow_attn_probs failed .*nq = 1, must be 0 in the temporal form'):
        ops.attn_probs(r.shape, False, r.qkv, out, pos=torch.zeros(1, dtype=torch.int32, device=cuda))

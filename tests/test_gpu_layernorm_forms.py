"""GPU: every compiled form of LayerNorm (csrc/layernorm.hip) and of the row fold behind it (csrc/reduce.hip), every row stride, every loop trip.

test_gpu_kernels.py runs LayerNorm at D = 64 / 256 / 768 / 1024 with dense tensors and at most 9030 rows.  Here: all nine (NV, FULL) forms of
ln_fwd_kernel / ln_bwd_kernel, the second and third trips of their row loops, `dres` absent, every combination of the optional outputs, strided views
of all six tensors, and partial tables whose 16-column fold workgroups straddle the dgamma | dbeta | colsum boundaries.

Every case compares with F.layer_norm in float64 and its autograd; copies and casts are compared bit for bit.  Bounds (of the tensor's maximum, rel()):
y 2e-5 / 2e-2 / 2.5e-3 (f32 / bf16 / fp16 storage), mean 1e-5, dx dgamma dbeta 1e-4, colsum 1e-5 against the float64 column sum of the dx the kernel
wrote -- all as in test_gpu_kernels.py -- and 1e-4 against the all-float64 colsum (it inherits dx's error).  rstd has no bound there: 1e-5 here, the
bound of mean (both are one f32 tree sum over D <= 2048 values, at most ~12 roundings of 2^-24 each = 7e-7, then a division / a square root and
a division).  The same formulas in plain float32 torch ops, at these shapes and inputs, stay more than a factor 30 inside every one of these bounds
(largest over all shapes of this module, D = 4 and the 6150-row sums included: y 1.7e-7, mean 1.6e-7, rstd 1.5e-7, dx 1.6e-7, dgamma 2.7e-7, dbeta 1.9e-7,
colsum 2.1e-7, all-float64 colsum 2.4e-7), so no bound is widened for any shape.

Outputs are [:rows, :D] views of NaN-filled buffers with pad columns and a spare row (kernel_forms.py): a dead lane of a non-FULL form or a last trip
that runs past `rows` shows as a changed sentinel, an unwritten element as a NaN inside the view."""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from kernel_forms import assert_guarded, bits, guarded
from test_gpu_kernels import MODES, _mode, rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops(cuda):
    from tcow_amd import ops as o
    return o


# D -> (NV, FULL) as tcow_layernorm_fwd / _bwd dispatch:  nvl = ceil(D / 256) float4 passes per lane;  FULL = (D == 256 * nvl and nvl <= 4);
# NV = nvl for nvl <= 4, else the NV = 8 form (never FULL).  All nine compiled forms appear:
FORMS = {
    4: (1, False), 252: (1, False), 256: (1, True),
    260: (2, False), 512: (2, True),
    516: (3, False), 764: (3, False), 768: (3, True),
    1000: (4, False), 1024: (4, True),
    1028: (8, False), 1536: (8, False), 2044: (8, False), 2048: (8, False),
}
ROWS = [1, 5, 37]              # one wave; two workgroups, three waves of the second idle (they still join the LDS fold); ten workgroups, a ragged last one


def test_form_table_matches_the_dispatch():
    def dispatch(D):
        nvl = (D // 4 + 63) // 64
        return (nvl if nvl <= 4 else 8), (D == 256 * nvl and nvl <= 4)
    assert all(dispatch(D) == form for D, form in FORMS.items())
    assert set(FORMS.values()) == {(1, False), (1, True), (2, False), (2, True), (3, False), (3, True), (4, False), (4, True), (8, False)}


@functools.lru_cache(maxsize=2)
def case(rows, D, device):
    """Inputs (the generators of test_gpu_kernels.py) and the float64 forward of one shape, shared by the three storages and left unchanged."""
    g = torch.Generator(device=device).manual_seed(rows * 4099 + D)
    c = SimpleNamespace(rows=rows, D=D)
    c.x = torch.randn(rows, D, device=device, generator=g) * 2 + 0.5
    c.w = torch.rand(D, device=device, generator=g) + 0.5; c.b = torch.randn(D, device=device, generator=g)
    c.dy32 = torch.randn(rows, D, device=device, generator=g); c.dres = torch.randn(rows, D, device=device, generator=g)
    c.sc = torch.rand(rows, device=device, generator=g) + 0.5
    c.dg0 = torch.randn(D, device=device, generator=g); c.db0 = torch.randn(D, device=device, generator=g); c.cs0 = torch.randn(D, device=device, generator=g)
    c.xd = c.x.double().requires_grad_(True); c.wd = c.w.double().requires_grad_(True); c.bd = c.b.double().requires_grad_(True)
    c.ref = F.layer_norm(c.xd, (D,), c.wd, c.bd, 1e-6)
    c.mean = c.x.double().mean(1); c.rstd = (c.x.double().var(1, unbiased=False) + 1e-6).rsqrt()
    return c


def bwd_ref(c, dy):
    """float64 (dx without the residual term, dgamma, dbeta) for this storage's dy."""
    return torch.autograd.grad((c.ref * dy.double()).sum(), [c.xd, c.wd, c.bd], retain_graph=True)


def run_fwd(ops, mode, dt, c, tol, x=None, pitch=4):
    """layernorm_fwd into guarded buffers; checks y, mean, rstd against float64 and the sentinels.  Returns (y, mean, rstd) views."""
    rows, D, dev = c.rows, c.D, c.x.device
    ybuf, y = guarded(rows, D, D + pitch, dt, dev)
    mbuf, mu = guarded(1, rows, rows + 3, torch.float32, dev); rbuf, rs = guarded(1, rows, rows + 3, torch.float32, dev)
    mu, rs = mu[0], rs[0]
    ops.layernorm_fwd(mode, c.x if x is None else x, c.w, c.b, y, mu, rs)
    assert_guarded(ybuf, rows, D, 'y'); assert_guarded(mbuf, 1, rows, 'mean'); assert_guarded(rbuf, 1, rows, 'rstd')
    e = rel(y, c.ref), rel(mu, c.mean), rel(rs, c.rstd)
    assert e[0] < tol and e[1] < 1e-5 and e[2] < 1e-5, f'y {e[0]:.3e} mean {e[1]:.3e} rstd {e[2]:.3e}'
    return y, mu, rs


def run_bwd(ops, mode, dt, c, dy, mu, rs, dres=True, params=None, cast=None, colsum=None, pitches=(4, 8)):
    """One layernorm_bwd call with every output in a guarded buffer.  params: None | 'plain' | 'acc' (dgamma / dbeta / colsum start from dg0 / db0 / cs0);
    cast, colsum: None | 'plain' | 'scaled'.  Checks the sentinels and returns the outputs."""
    rows, D, dev = c.rows, c.D, c.x.device
    o = SimpleNamespace(dg=None, db=None, cs=None, dxc=None)
    dxbuf, o.dx = guarded(rows, D, D + pitches[0], torch.float32, dev)
    kw = {}
    bufs = []
    if params:
        for name, init in (('dg', c.dg0), ('db', c.db0)) + ((('cs', c.cs0),) if colsum else ()):
            buf, v = guarded(1, D, D + 5, torch.float32, dev)
            if params == 'acc':
                v.copy_(init)
            setattr(o, name, v[0]); bufs.append((name, buf))
        kw.update(dgamma=o.dg, dbeta=o.db, accumulate=params == 'acc')
        if colsum:
            kw.update(colsum_out=o.cs, colsum_scale=c.sc if colsum == 'scaled' else None)
    if cast:
        cbuf, o.dxc = guarded(rows, D, D + pitches[1], dt, dev)
        kw.update(dx_cast=o.dxc, cast_scale=c.sc if cast == 'scaled' else None)
    ops.layernorm_bwd(mode, dy, c.x, mu, rs, c.w, c.dres if dres else None, o.dx, **kw)
    assert_guarded(dxbuf, rows, D, 'dx')
    for name, buf in bufs:
        assert_guarded(buf, 1, D, name)
    if cast:
        assert_guarded(cbuf, rows, D, 'dx_cast')
    return o


def check_bwd(c, o, gx, gw, gb, dres=True, params=None, cast=None, colsum=None):
    """The outputs of run_bwd against float64 (dx, dgamma, dbeta: 1e-4; colsum: 1e-5 on the kernel's dx, 1e-4 all-float64) and the cast bit for bit."""
    want_dx = gx + c.dres.double() if dres else gx
    e = rel(o.dx, want_dx)
    assert e < 1e-4, f'dx {e:.3e}'
    acc = params == 'acc'
    if params:
        eg, eb = rel(o.dg, gw + c.dg0.double() if acc else gw), rel(o.db, gb + c.db0.double() if acc else gb)
        assert eg < 1e-4 and eb < 1e-4, f'dgamma {eg:.3e} dbeta {eb:.3e}'
    if colsum:
        s = c.sc.double()[:, None] if colsum == 'scaled' else 1.0
        base = c.cs0.double() if acc else 0.0
        e1, e2 = rel(o.cs, (o.dx.double() * s).sum(0) + base), rel(o.cs, (want_dx * s).sum(0) + base)
        assert e1 < 1e-5 and e2 < 1e-4, f'colsum {e1:.3e} (sum of the kernel dx) {e2:.3e} (float64)'
    if cast:
        want = o.dx * c.sc[:, None] if cast == 'scaled' else o.dx
        assert torch.equal(o.dxc, want.to(o.dxc.dtype)), 'dx_cast is not dtype(dx * scale)'


@pytest.mark.parametrize('mname,tol', MODES)
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('D', sorted(FORMS))
def test_layernorm_every_form(ops, cuda, mname, tol, rows, D):
    """Forward (y, mean, rstd) and every argument combination of the backward, for every (NV, FULL) form of FORMS at rows = 1, 5, 37."""
    mode, dt = _mode(ops, mname)
    c = case(rows, D, cuda)
    y, mu, rs = run_fwd(ops, mode, dt, c, tol)
    dy = c.dy32.to(dt)
    ref = bwd_ref(c, dy)
    base = None
    for kw in (dict(dres=True, params='plain'),                                             # dres given, plain parameter gradients
               dict(dres=True),                                                             # parameter gradients absent (no partial table, no LDS)
               dict(dres=True, params='acc'),                                               # accumulating into nonzero dgamma / dbeta
               dict(dres=True, cast='scaled'), dict(dres=True, cast='plain'),               # dx_cast with and without cast_scale
               dict(dres=True, params='plain', colsum='scaled'), dict(dres=True, params='plain', colsum='plain'),
               dict(dres=True, params='acc', colsum='scaled', cast='scaled'),               # everything at once
               dict(dres=False), dict(dres=False, params='plain'),                          # dres = None
               dict(dres=False, params='acc', colsum='plain', cast='plain')):
        o = run_bwd(ops, mode, dt, c, dy, mu, rs, **kw)
        check_bwd(c, o, *ref, **kw)
        if kw == dict(dres=True, params='plain'):
            base = o
        elif kw['dres']:
            assert torch.equal(o.dx, base.dx), f'{kw}: dx differs from the plain call'
            if kw.get('params') == 'plain':                                                 # (the colsum form folds the same dgamma / dbeta partials)
                assert rel(o.dg, base.dg) < 1e-5 and rel(o.db, base.db) < 1e-5


@pytest.mark.parametrize('mname,tol', MODES)
@pytest.mark.parametrize('rows,D', [(16389, 64), (32771, 64), (16389, 260)])
def test_layernorm_fwd_row_loop(ops, cuda, mname, tol, rows, D):
    """The forward visits rows in steps of 4096 workgroups x 4 waves = 16384 with the next row's loads issued early: 16389 rows = five waves make a second
    trip (and nothing is prefetched for a third), 32771 = three rows of a third trip; D = 260 takes the loop in a guarded (2, no) form."""
    mode, dt = _mode(ops, mname)
    run_fwd(ops, mode, dt, case(rows, D, cuda), tol)


@pytest.mark.parametrize('mname,tol', MODES)
@pytest.mark.parametrize('D', [260, 1028])
@pytest.mark.parametrize('rows,colsum', [(3073, None), (6150, None), (2049, 'scaled'), (4100, 'scaled')])
def test_layernorm_bwd_row_loop(ops, cuda, mname, tol, D, rows, colsum):
    """The backward runs 768 workgroups x 4 waves = 3072 rows per trip (512 x 4 = 2048 with the column sum): one row / six rows past one and two trips, in the
    (2, no) and the NV = 8 forms; the fold then reads 768 / 512 partial rows (the 8-deep unrolled loop of row_reduce_body and its tail)."""
    mode, dt = _mode(ops, mname)
    c = case(rows, D, cuda)
    _, mu, rs = run_fwd(ops, mode, dt, c, tol)
    dy = c.dy32.to(dt)
    ref = bwd_ref(c, dy)
    for kw in (dict(dres=True, params='plain', colsum=colsum, cast='scaled'), dict(dres=False, params='acc', colsum=colsum)):
        check_bwd(c, run_bwd(ops, mode, dt, c, dy, mu, rs, **kw), *ref, **kw)


@pytest.mark.parametrize('mname,tol', MODES)
@pytest.mark.parametrize('D', [260, 768, 1028])
def test_layernorm_strided_views_equal_dense(ops, cuda, mname, tol, D):
    """x, y, dy, dres, dx and dx_cast as [:rows, :D] views of buffers with row pitch D + 4 or D + 8 (different pitches in one call, pads NaN): every result
    equals the dense call's bit for bit and no pad changes, the inputs' included."""
    mode, dt = _mode(ops, mname)
    rows = 37
    c = case(rows, D, cuda)
    dy = c.dy32.to(dt)
    dense = lambda t: torch.empty(rows, D, device=cuda, dtype=t)
    y0, mu0, rs0 = dense(dt), torch.empty(rows, device=cuda), torch.empty(rows, device=cuda)
    ops.layernorm_fwd(mode, c.x, c.w, c.b, y0, mu0, rs0)
    dx0, dxc0 = dense(torch.float32), dense(dt)
    dg0, db0, cs0 = (torch.empty(D, device=cuda) for _ in range(3))
    ops.layernorm_bwd(mode, dy, c.x, mu0, rs0, c.w, c.dres, dx0, dg0, db0, dx_cast=dxc0, cast_scale=c.sc, colsum_out=cs0, colsum_scale=c.sc)
    check_bwd(c, SimpleNamespace(dx=dx0, dg=dg0, db=db0, cs=cs0, dxc=dxc0), *bwd_ref(c, dy), dres=True, params='plain', cast='scaled', colsum='scaled')

    def strided(src, pitch):
        buf, v = guarded(rows, D, D + pitch, src.dtype, cuda)
        v.copy_(src)
        return buf, v
    xb, xs = strided(c.x, 4); dyb, dys = strided(dy, 8); drb, drs = strided(c.dres, 4)
    inputs = [(b, b.clone()) for b in (xb, dyb, drb)]
    yb, ys = guarded(rows, D, D + 8, dt, cuda); dxb, dxs = guarded(rows, D, D + 8, torch.float32, cuda); cb, cs_ = guarded(rows, D, D + 4, dt, cuda)
    mu1, rs1 = torch.empty(rows, device=cuda), torch.empty(rows, device=cuda)
    ops.layernorm_fwd(mode, xs, c.w, c.b, ys, mu1, rs1)
    dg1, db1, cs1 = (torch.empty(D, device=cuda) for _ in range(3))
    ops.layernorm_bwd(mode, dys, xs, mu1, rs1, c.w, drs, dxs, dg1, db1, dx_cast=cs_, cast_scale=c.sc, colsum_out=cs1, colsum_scale=c.sc)
    assert_guarded(yb, rows, D, 'y'); assert_guarded(dxb, rows, D, 'dx'); assert_guarded(cb, rows, D, 'dx_cast')
    for got, want in ((ys, y0), (mu1, mu0), (rs1, rs0), (dxs, dx0), (cs_, dxc0), (dg1, dg0), (db1, db0), (cs1, cs0)):
        assert torch.equal(got, want)
    for buf, before in inputs:
        assert torch.equal(bits(buf), bits(before)), 'an input buffer was written'
    # dres absent and no optional output: still the strided dx only
    dxb2, dxs2 = guarded(rows, D, D + 4, torch.float32, cuda); dx2 = dense(torch.float32)
    ops.layernorm_bwd(mode, dys, xs, mu1, rs1, c.w, None, dxs2)
    ops.layernorm_bwd(mode, dy, c.x, mu0, rs0, c.w, None, dx2)
    assert_guarded(dxb2, rows, D, 'dx'); assert torch.equal(dxs2, dx2)


@pytest.mark.parametrize('mname', ['f32', 'bf16', 'fp16'])
@pytest.mark.parametrize('D', [516, 1028])
def test_layernorm_deferred_fold_off_the_fold_tile(ops, cuda, mname, D):
    """test_layernorm_deferred_fold_is_bit_identical at D = 516 and 1028: 2 D and 3 D are no multiples of the fold's 16 columns, so one workgroup of
    row_reduce_body holds the end of dgamma and the start of dbeta (and of colsum) and the last one is ragged.  600 rows = 150 partial rows: thread rows
    that take the 8-deep loop and thread rows that take only its tail.  layernorm_bwd(defer=) + layernorm_fold equals the immediate fold bit for bit, with
    and without the third table, with and without accumulation; the tables' pad elements keep their sentinel."""
    mode, dt = _mode(ops, mname)
    rows = 600
    g = torch.Generator(device=cuda).manual_seed(D)
    jobs, want = [], []
    for k in range(3):
        x = torch.randn(rows, D, device=cuda, generator=g) * 2 + 0.5; dy = torch.randn(rows, D, device=cuda, generator=g).to(dt)
        w = torch.rand(D, device=cuda, generator=g) + 0.5; dres = torch.randn(rows, D, device=cuda, generator=g)
        mu = x.mean(1); rs = (x.var(1, unbiased=False) + 1e-6).rsqrt(); sc = torch.rand(rows, device=cuda, generator=g)
        acc = k == 2
        outs = []
        for defer in (None, jobs):
            tabs = [guarded(1, D, D + 5, torch.float32, cuda) for _ in range(3)]
            for (_, v), init in zip(tabs, (0.5, -0.25, 0.0)):
                v.fill_(init)
            dg, db, cs = tabs[0][1][0], tabs[1][1][0], (tabs[2][1][0] if k != 1 else None)
            dx = torch.empty(rows, D, device=cuda)
            ops.layernorm_bwd(mode, dy, x, mu, rs, w, dres, dx, dg, db, accumulate=acc, colsum_out=cs, colsum_scale=sc if cs is not None else None, defer=defer)
            outs.append((tabs, dx))
        want.append(outs)
    assert len(jobs) == 3
    ops.layernorm_fold(jobs)
    assert not jobs
    for (now_tabs, now_dx), (later_tabs, later_dx) in want:
        assert torch.equal(now_dx, later_dx)
        for (a, _), (b, _) in zip(now_tabs, later_tabs):
            assert_guarded(a, 1, D, 'immediate fold'); assert_guarded(b, 1, D, 'deferred fold')
            assert torch.equal(bits(a), bits(b))
    # and the immediate fold is right per element (float64 column sums of the same products)
    xh = (x.double() - mu.double()[:, None]) * rs.double()[:, None]
    (tabs, dx) = want[2][0]
    assert rel(tabs[0][1][0], 0.5 + (dy.double() * xh).sum(0)) < 1e-4 and rel(tabs[1][1][0], -0.25 + dy.double().sum(0)) < 1e-4
    assert rel(tabs[2][1][0], (dx.double() * sc.double()[:, None]).sum(0)) < 1e-5

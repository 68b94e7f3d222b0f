"""GPU: the skinny-M NT GEMMs in every arithmetic that has one: the two 16-bit storage formats (tcow_gemm_nt_skinny, csrc/gemm_nt_skinny.hip) and
bf16 x 3 on f32 tensors (tcow_gemm_nt_skinny_x3, csrc/gemm_nt_skinny_x3.hip).  split == 1 against the 128 x 128 tile bit for bit; split > 1
exactly on operands whose product is known (small integers; hi / lo planes for bf16 x 3), in its fixed summation order, and through every epilogue
against an f64 product; the refusals.  16-bit operands are made as in test_gpu_kernels.py and the tolerances are that file's: bf16 outputs 4e-3,
binary16 5e-4, f32 outputs 2e-5 of the reference's maximum; bf16 x 3 (operands, outputs and aux all f32) 4e-5, its 'f32x3' entry of GEMM_MODES."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

from kernel_forms import hi_lo_operand, want_hi_lo
from test_gpu_kernels import GEMM_MODES

pytestmark = pytest.mark.gpu

SENT = 7.0
TOL16 = {'bf16': 4e-3, 'fp16': 5e-4}
TOL32 = 2e-5
TOLX3 = dict(GEMM_MODES)['f32x3']
assert TOLX3 == 4e-5
FMTS16 = ['bf16', 'fp16']
FMTS = FMTS16 + ['bf16x3']


@pytest.fixture(scope='module', autouse=True)
def _leave_no_scratch():
    """ops.workspace keeps a thread's grow-only buffers for as long as the thread lives, and other tests look at them: this module leaves none of
    its split-K scratch behind."""
    yield
    from tcow_amd import ops as o
    o.workspace_drop('nt_skinny')


@pytest.fixture(scope='module')
def ops(cuda):
    from tcow_amd import ops as o
    return o


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def _integers(gen, shape, device):
    """Elements in {-3 .. 3}: every sum stays below 2^24, so the f32 output is the integer product exactly, whatever the order."""
    return torch.randint(-3, 4, shape, device=device, generator=gen).float()


def _want_integers(c):
    return c.ref0


def _want_hi_lo(c):
    """Operands of kernel_forms.hi_lo_operand: the f32 output is hi_A hi_W^T + hi_A lo_W^T + lo_A hi_W^T exactly, in any order (want_hi_lo)."""
    return want_hi_lo(c.A, c.W)


def _arith(ops, fmt):
    """One arithmetic: its mode and storage dtype, its entry point (C name, wrapper), the 128-tile call split == 1 is compared with, the tolerance
    of an output in the storage dtype / in f32, the operands whose product is known exactly with that product, and what the entry point refuses
    beyond the split, K and workspace cases they all share."""
    from tcow_amd import _lib as L
    a = types.SimpleNamespace(fmt=fmt, x3=fmt == 'bf16x3')
    if a.x3:
        a.mode, a.dt, a.entry = ops.F32X3, torch.float32, 'tcow_gemm_nt_skinny_x3'
        a.skinny = lambda A, W, out, **kw: ops.gemm_nt_skinny_x3(A, W, out, **kw)
        a.tile128 = lambda A, W, out, **kw: ops.gemm_nt(ops.F32X3, A, W, out, **kw)
        a.tol = a.tol32 = TOLX3
        a.exact, a.exact_want = hi_lo_operand, _want_hi_lo
        a.refused = [(dict(ws_off=4), 'workspace'), (dict(dtype=L.TCOW_BF16), 'dtype'), (dict(dtype=L.TCOW_F32), 'dtype'), (dict(ldc_extra=-2), 'ldc')]
    else:
        a.mode, a.dt, a.entry = {'bf16': (ops.BF16, torch.bfloat16), 'fp16': (ops.FP16, torch.float16)}[fmt] + ('tcow_gemm_nt_skinny',)
        a.skinny = lambda A, W, out, **kw: ops.gemm_nt_skinny(a.mode, A, W, out, **kw)
        a.tile128 = lambda A, W, out, **kw: ops.gemm_nt(a.mode, A, W, out, tile=128, **kw)
        a.tol, a.tol32 = TOL16[fmt], TOL32
        a.exact, a.exact_want = _integers, _want_integers
        a.refused = [(dict(dtype=L.TCOW_F32), 'dtype')]
    return a


def _case(cuda, a, M, N, K, seed, exact=False):
    """Operands of one product.  A and the GELU' / multiplier tile are column slices of wider tensors (lda > K, ldaux > N).
    exact: the arithmetic's exactly representable operands (a.exact), integer bias and residual."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    c = types.SimpleNamespace(M=M, N=N, K=K, dt=a.dt)
    if exact:
        ri = lambda *s: torch.randint(-3, 4, s, device=cuda, generator=g).float()
        x = lambda *s: a.exact(g, s, cuda)
        c.A = x(M, K + 8).to(a.dt)[:, 8:]; c.W = x(N, K).to(a.dt)
        c.bias = ri(N); c.resid = ri(M, N)
    else:
        c.A = torch.randn(M, K + 8, device=cuda, generator=g).to(a.dt)[:, 8:]; c.W = (torch.randn(N, K, device=cuda, generator=g) * 0.05).to(a.dt)
        c.bias = torch.randn(N, device=cuda, generator=g); c.resid = torch.randn(M, N, device=cuda, generator=g)
    c.rs = torch.rand(M, device=cuda, generator=g) + 0.5; c.rs[::7] = 0.0
    c.pre = torch.randn(M, N + 8, device=cuda, generator=g).to(a.dt)[:, 4:4 + N]
    c.b2 = torch.randn(N, device=cuda, generator=g); c.rs2 = (torch.rand(M, device=cuda, generator=g) > 0.3).float()
    c.ref0 = c.A.double() @ c.W.double().t()                          # computed once per case, never modified
    return c


def _forms(ops, c):
    """Every epilogue combination of test_gemm_nt_epilogues and test_gemm_nt_every_tile_kernel_at_bench_size:
    (name, f32 output, residual aliases the output, aux role, keywords).  f32 storage: every output is f32 (the flag says nothing), and 'plain32'
    would repeat 'plain16': the row scale alone takes its place."""
    b, rs, res, b2, rs2 = dict(bias=c.bias), dict(row_scale=c.rs), dict(resid=c.resid), dict(bias2=c.b2), dict(row_scale2=c.rs2)
    forms = [
        ('plain16', False, False, None, {}),
        ('bias16', False, False, None, {**b}),
        ('plain32', True, False, None, {}),
        ('bias_rs16', False, False, None, {**b, **rs}),
        ('bias_res32', True, False, None, {**b, **res}),
        ('bias_rs_res32', True, False, None, {**b, **rs, **res}),
        ('alias_bias_res', True, True, None, {**b}),
        ('alias_bias_rs_res', True, True, None, {**b, **rs}),
        ('fold7', True, False, None, {**b, **rs, **res, **b2, **rs2}),
        ('alias_fold7', True, True, None, {**b, **rs, **b2, **rs2}),
        ('bias_b2_16', False, False, None, {**b, **b2}),
        ('gelu_aux', False, False, 'out', {**b, 'act': ops.ACT_GELU}),
        ('gelu', False, False, None, {**b, 'act': ops.ACT_GELU}),
        ('dgelu', False, False, 'in', {'act': ops.ACT_DGELU}),
        ('gelu_dsave', False, False, 'out', {**b, 'act': ops.ACT_GELU_DSAVE}),
        ('mul_aux', False, False, 'in', {'act': ops.ACT_MUL_AUX}),
    ]
    if c.dt == torch.float32:
        forms[2] = ('rs', False, False, None, {**rs})
        forms = [(name, False, alias, auxrole, kw) for name, _, alias, auxrole, kw in forms]
    assert len(forms) == 16
    return forms


def _dgelu(x):
    x = x.clone().requires_grad_(True)
    return torch.autograd.grad(F.gelu(x).sum(), x)[0]


def _reference(ops, c, alias, kw):
    """(f64 output, f64 aux output or None) of one form."""
    v = c.ref0
    if 'bias' in kw:
        v = v + c.bias.double()
    if 'row_scale' in kw:
        v = v * c.rs.double()[:, None]
    act, aux = kw.get('act', ops.ACT_NONE), None
    if act == ops.ACT_GELU:
        aux, v = v, F.gelu(v)
    elif act == ops.ACT_GELU_DSAVE:
        aux, v = _dgelu(v), F.gelu(v)
    elif act == ops.ACT_DGELU:
        v = v * _dgelu(c.pre.double())
    elif act == ops.ACT_MUL_AUX:
        v = v * c.pre.double()
    if 'bias2' in kw:
        v = v + (c.rs2.double()[:, None] if 'row_scale2' in kw else 1.0) * c.b2.double()
    if alias or 'resid' in kw:
        v = v + c.resid.double()
    return v, aux


def _run(call, cuda, c, f32, alias, auxrole, kw):
    """One call into sentinel buffers [M + 1, N + 8]: (output buffer, aux buffer or None)."""
    M, N = c.M, c.N
    ob = torch.full((M + 1, N + 8), SENT, device=cuda, dtype=torch.float32 if f32 else c.dt)
    kw = dict(kw)
    if alias:
        ob[:M, :N] = c.resid
        kw['resid'] = ob[:M, :N]
    ab = None
    if auxrole == 'out':
        ab = torch.full((M + 1, N + 8), SENT, device=cuda, dtype=c.dt)
        kw['aux'] = ab[:M, :N]
    elif auxrole == 'in':
        kw['aux'] = c.pre
    call(c.A, c.W, ob[:M, :N], **kw)
    return ob, ab


def _guards_ok(buf, M, N):
    return buf is None or (bool((buf[M] == SENT).all()) and bool((buf[:, N:] == SENT).all()))


# one partial tile, a ragged N, nk = 1, 2, 3 (nk = 1: a ring shorter than its stages) and 9; the last: 24 x 24 = 576 workgroups, more than one round
# (and, in the 16-bit kernel, the two-stage ring of more than 512 workgroups)
@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('M,N,K', [(1, 4, 64), (63, 60, 128), (64, 64, 64), (65, 68, 192), (301, 264, 576), (1480, 1536, 128)])
def test_split_1_equals_the_128_tile_bit_for_bit(ops, cuda, fmt, M, N, K):
    a = _arith(ops, fmt)
    c = _case(cuda, a, M, N, K, M + N + K)
    skinny = lambda A, W, out, **kw: a.skinny(A, W, out, split=1, **kw)
    for name, f32, alias, auxrole, kw in _forms(ops, c):
        o1, a1 = _run(skinny, cuda, c, f32, alias, auxrole, kw)
        o0, a0 = _run(a.tile128, cuda, c, f32, alias, auxrole, kw)
        assert torch.equal(o1, o0), (name, rel(o1[:M, :N], o0[:M, :N]))
        assert a1 is None or torch.equal(a1, a0), name
        assert _guards_ok(o1, M, N) and _guards_ok(a1, M, N), name


def _split_exact(ops, cuda, fmt, M, N, K, splits):
    """The f32 output is the arithmetic's exact product (a.exact_want), alone and with an integer bias and residual -- every k-slice is covered once
    and none twice (nk = 5: uneven slices, and S = nk)."""
    a = _arith(ops, fmt)
    c = _case(cuda, a, M, N, K, 3 * M + K, exact=True)
    want = a.exact_want(c)
    for S in splits:
        call = lambda A, W, out, **kw: a.skinny(A, W, out, split=S, **kw)
        ob, _ = _run(call, cuda, c, True, False, None, {})
        assert torch.equal(ob[:M, :N].double(), want) and _guards_ok(ob, M, N), S
        ob, _ = _run(call, cuda, c, True, False, None, dict(bias=c.bias, resid=c.resid))
        assert torch.equal(ob[:M, :N].double(), want + c.bias.double() + c.resid.double()) and _guards_ok(ob, M, N), S


@pytest.mark.parametrize('fmt', FMTS16)
@pytest.mark.parametrize('M,N,K,splits', [(65, 68, 320, (2, 3, 5)), (301, 72, 1024, (4, 8, 16))])
def test_split_exact_on_small_integers(ops, cuda, fmt, M, N, K, splits):
    """Operands in {-3 .. 3}, integer bias and residual: the f32 output is the integer product exactly whatever the order."""
    _split_exact(ops, cuda, fmt, M, N, K, splits)


@pytest.mark.parametrize('fmt', ['bf16x3'])
@pytest.mark.parametrize('M,N,K,splits', [(65, 68, 320, (1, 2, 3, 5)), (301, 72, 1024, (4, 8, 16))])
def test_split_exact_on_hi_lo_operands(ops, cuda, fmt, M, N, K, splits):
    """x = h + l with bf16(x) = h and bf16(x - h) = l exactly (_want_hi_lo).  A kernel that drops, doubles or swaps a plane, skips a k-slice or
    covers one twice differs."""
    _split_exact(ops, cuda, fmt, M, N, K, splits)


@pytest.mark.parametrize('fmt', FMTS)
@pytest.mark.parametrize('M,N,K,splits', [(65, 68, 320, (2, 3, 5)), (301, 72, 1024, (4, 8, 16))])
def test_split_adds_the_slices_in_order(ops, cuda, fmt, M, N, K, splits):
    """No epilogue operands, f32 output: the result is p_0 + p_1 + ... + p_{S-1} added in that order in f32, p_s = the split == 1 product over the
    columns of slice s; a second call gives the same bits."""
    a = _arith(ops, fmt)
    c = _case(cuda, a, M, N, K, M + 5 * K)
    nk = K // 64
    for S in splits:
        want = None
        for s in range(S):
            k0, k1 = 64 * (s * nk // S), 64 * ((s + 1) * nk // S)
            p = a.skinny(c.A[:, k0:k1], c.W[:, k0:k1], torch.empty(M, N, device=cuda), split=1)
            want = p if want is None else want + p
        got = a.skinny(c.A, c.W, torch.empty(M, N, device=cuda), split=S)
        assert torch.equal(got, want), (S, rel(got, want))
        again = a.skinny(c.A, c.W, torch.empty(M, N, device=cuda), split=S)
        assert torch.equal(again, got), S


@pytest.mark.parametrize('fmt', FMTS)
def test_split_every_epilogue_vs_f64(ops, cuda, fmt):
    """Two shapes of different sizes back to back on one workspace, filled with NaN before each pair of calls: a slab element that no workgroup
    wrote, or one left by the other call, would show."""
    a = _arith(ops, fmt)
    cases = [(_case(cuda, a, 301, 264, 576, 11), 3), (_case(cuda, a, 130, 768, 3072, 12), 8)]
    lib, _ = ops._sel(a.mode)
    need = max(lib.tcow_gemm_nt_skinny_workspace_bytes(c.M, c.N, S) for c, S in cases)
    ws = ops.workspace(need, cuda, 'nt_skinny')
    forms = [_forms(ops, c) for c, _ in cases]
    for i in range(len(forms[0])):
        ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(float('nan'))
        ran = []
        for (c, S), fs in zip(cases, forms):
            name, f32, alias, auxrole, kw = fs[i]
            call = lambda A, W, out, **k: a.skinny(A, W, out, split=S, **k)
            ran.append((c, S, name, f32, alias, kw) + _run(call, cuda, c, f32, alias, auxrole, kw))
        assert ops.workspace(need, cuda, 'nt_skinny') is ws
        for c, S, name, f32, alias, kw, ob, ab in ran:
            want, want_aux = _reference(ops, c, alias, kw)
            err = rel(ob[:c.M, :c.N], want)
            assert err < (a.tol32 if f32 else a.tol), (name, S, err)
            assert ab is None or rel(ab[:c.M, :c.N], want_aux) < a.tol, (name, S)
            assert _guards_ok(ob, c.M, c.N) and _guards_ok(ab, c.M, c.N), (name, S)


@pytest.mark.parametrize('fmt', FMTS)
def test_refusals_name_the_argument_and_launch_nothing(ops, cuda, fmt):
    from tcow_amd import _lib as L
    a = _arith(ops, fmt)
    lib, dm = ops._sel(a.mode)
    M, N = 40, 64
    A = torch.randn(M, 256, device=cuda).to(a.dt); W = torch.randn(N, 256, device=cuda).to(a.dt)
    ws = torch.empty(8 * M * N * 4 + 16, dtype=torch.uint8, device=cuda)

    def call(K=256, split=2, ws_off=0, nbytes=None, dtype=dm, ldc_extra=0):
        buf = torch.full((M, N + 8), SENT, device=cuda)
        out = buf[:, :N]
        g = L.GemmArgs(M, N, K, dtype, A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0), out.data_ptr(), out.stride(0) + ldc_extra, 1, None, None, None, 0,
                       L.ACT_NONE, None, 0, 0, None, None)
        need = lib.tcow_gemm_nt_skinny_workspace_bytes(M, N, split)
        rc = getattr(lib, a.entry)(ops._stream(), ctypes.byref(g), split, ws.data_ptr() + ws_off if ws_off is not None else None, need if nbytes is None else nbytes)
        torch.cuda.synchronize()
        return rc, lib.tcow_last_error().decode(), bool((buf == SENT).all())

    rc, _, untouched = call()
    assert rc == 0 and not untouched                                              # the accepted call these are variations of
    assert lib.tcow_gemm_nt_skinny_workspace_bytes(M, N, 1) == 0 and lib.tcow_gemm_nt_skinny_workspace_bytes(M, N, 2) == 2 * M * N * 4
    need2 = 2 * M * N * 4
    assert ws.data_ptr() % 16 == 0
    for kw, word in [(dict(split=0), 'split'), (dict(split=17), 'split'), (dict(split=5), 'split'), (dict(K=96, split=1), 'K=96'),
                     (dict(ws_off=None), 'workspace'), (dict(nbytes=need2 - 1), 'workspace')] + a.refused:
        rc, msg, untouched = call(**kw)
        assert rc != 0 and msg.startswith(a.entry + ':') and word in msg and untouched, (kw, rc, msg)
    with pytest.raises(L.TcowError, match='split'):
        a.skinny(A, W, torch.empty(M, N, device=cuda), split=5)
    for mode in (ops.F32, ops.F32X3):                                             # the 16-bit entry point refuses these modes
        with pytest.raises(L.TcowError):
            ops.gemm_nt_skinny(mode, A.float(), W.float(), torch.empty(M, N, device=cuda), split=1)


def test_gemm_nt_routes_only_what_the_entry_point_accepts(ops, cuda, monkeypatch):
    """ops.gemm_nt(F32X3, skinny=True): a product whose N is no multiple of 4, or whose output pitch is not whole 16 bytes, stays on tcow_gemm_nt
    (the 128 tile has a scalar path) instead of raising in the entry point; the aligned product next to it is routed.  Same bits either way."""
    calls = []
    real = ops.gemm_nt_skinny_x3
    monkeypatch.setattr(ops, 'gemm_nt_skinny_x3', lambda *a, **kw: (calls.append(kw.get('split')), real(*a, **kw))[1])
    M, K = 65, 128
    for N, pitch, routed in [(68, 76, True), (68, 74, False), (70, 78, False)]:
        c = _case(cuda, _arith(ops, 'bf16x3'), M, N, K, N + pitch)
        outs = []
        for skinny in (False, True):
            buf = torch.full((M + 1, pitch), SENT, device=cuda)
            ops.gemm_nt(ops.F32X3, c.A, c.W, buf[:M, :N], bias=c.bias, resid=c.resid, skinny=skinny)
            outs.append(buf)
        assert calls == ([1] if routed else []), (N, pitch, calls)
        del calls[:]
        assert torch.equal(outs[0], outs[1]) and _guards_ok(outs[1], M, N)
        assert rel(outs[1][:M, :N], c.ref0 + c.bias.double() + c.resid.double()) < TOLX3

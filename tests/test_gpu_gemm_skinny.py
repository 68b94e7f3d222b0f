"""GPU: the skinny-M NT GEMM (tcow_gemm_nt_skinny, csrc/gemm_nt_skinny.hip) in both 16-bit storage formats.  split == 1 against the 128 x 128 tile
bit for bit; split > 1 exactly on small integers (every k-slice once), in its fixed summation order, and through every epilogue against an f64
product; the refusals.  Operands are 16-bit values made as in test_gpu_kernels.py and the tolerances are that file's: bf16 outputs 4e-3,
binary16 5e-4, f32 outputs 2e-5 of the reference's maximum."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = 7.0
TOL16 = {'bf16': 4e-3, 'fp16': 5e-4}
TOL32 = 2e-5


@pytest.fixture(scope='module', autouse=True)
def _leave_no_scratch():
    """ops.workspace is a process-wide, grow-only cache that other tests look at: this module leaves none of its split-K scratch in it."""
    yield
    from tcow_amd import ops as o
    for k in [k for k in o._ws_cache if k[2] == 'nt_skinny']:
        del o._ws_cache[k]


@pytest.fixture(scope='module')
def ops(cuda):
    from tcow_amd import ops as o
    return o


def _mode(ops, fmt):
    return {'bf16': (ops.BF16, torch.bfloat16), 'fp16': (ops.FP16, torch.float16)}[fmt]


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def _case(cuda, dt, M, N, K, seed, integer=False):
    """Operands of one product.  A and the GELU' / multiplier tile are column slices of wider tensors (lda > K, ldaux > N)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    c = types.SimpleNamespace(M=M, N=N, K=K, dt=dt)
    if integer:
        ri = lambda *s: torch.randint(-3, 4, s, device=cuda, generator=g).float()
        c.A = ri(M, K + 8).to(dt)[:, 8:]; c.W = ri(N, K).to(dt)
        c.bias = ri(N); c.resid = ri(M, N)
    else:
        c.A = torch.randn(M, K + 8, device=cuda, generator=g).to(dt)[:, 8:]; c.W = (torch.randn(N, K, device=cuda, generator=g) * 0.05).to(dt)
        c.bias = torch.randn(N, device=cuda, generator=g); c.resid = torch.randn(M, N, device=cuda, generator=g)
    c.rs = torch.rand(M, device=cuda, generator=g) + 0.5; c.rs[::7] = 0.0
    c.pre = torch.randn(M, N + 8, device=cuda, generator=g).to(dt)[:, 4:4 + N]
    c.b2 = torch.randn(N, device=cuda, generator=g); c.rs2 = (torch.rand(M, device=cuda, generator=g) > 0.3).float()
    c.ref0 = c.A.double() @ c.W.double().t()                          # computed once per case, never modified
    return c


def _forms(ops, c):
    """Every epilogue combination of test_gemm_nt_epilogues and test_gemm_nt_every_tile_kernel_at_bench_size:
    (name, f32 output, residual aliases the output, aux role, keywords)."""
    b, rs, res, b2, rs2 = dict(bias=c.bias), dict(row_scale=c.rs), dict(resid=c.resid), dict(bias2=c.b2), dict(row_scale2=c.rs2)
    return [
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


@pytest.mark.parametrize('fmt', ['bf16', 'fp16'])
@pytest.mark.parametrize('M,N,K', [(1, 4, 64), (63, 60, 128), (64, 64, 64), (65, 68, 192), (301, 264, 576)])
def test_split_1_equals_the_128_tile_bit_for_bit(ops, cuda, fmt, M, N, K):
    mode, dt = _mode(ops, fmt)
    c = _case(cuda, dt, M, N, K, M + N + K)
    skinny = lambda A, W, out, **kw: ops.gemm_nt_skinny(mode, A, W, out, split=1, **kw)
    tile128 = lambda A, W, out, **kw: ops.gemm_nt(mode, A, W, out, tile=128, **kw)
    for name, f32, alias, auxrole, kw in _forms(ops, c):
        o1, a1 = _run(skinny, cuda, c, f32, alias, auxrole, kw)
        o0, a0 = _run(tile128, cuda, c, f32, alias, auxrole, kw)
        assert torch.equal(o1, o0), (name, rel(o1[:M, :N], o0[:M, :N]))
        assert a1 is None or torch.equal(a1, a0), name
        assert _guards_ok(o1, M, N) and _guards_ok(a1, M, N), name


@pytest.mark.parametrize('fmt', ['bf16', 'fp16'])
@pytest.mark.parametrize('M,N,K,splits', [(65, 68, 320, (2, 3, 5)), (301, 72, 1024, (4, 8, 16))])
def test_split_exact_on_small_integers(ops, cuda, fmt, M, N, K, splits):
    """Operands in {-3 .. 3}, integer bias and residual: every sum stays below 2^24, so the f32 output is the integer product exactly whatever the
    order -- every k-slice is covered once and none twice (nk = 5: uneven slices, and S = nk)."""
    mode, dt = _mode(ops, fmt)
    c = _case(cuda, dt, M, N, K, 3 * M + K, integer=True)
    for S in splits:
        call = lambda A, W, out, **kw: ops.gemm_nt_skinny(mode, A, W, out, split=S, **kw)
        ob, _ = _run(call, cuda, c, True, False, None, {})
        assert torch.equal(ob[:M, :N].double(), c.ref0) and _guards_ok(ob, M, N), S
        ob, _ = _run(call, cuda, c, True, False, None, dict(bias=c.bias, resid=c.resid))
        assert torch.equal(ob[:M, :N].double(), c.ref0 + c.bias.double() + c.resid.double()) and _guards_ok(ob, M, N), S


@pytest.mark.parametrize('fmt', ['bf16', 'fp16'])
@pytest.mark.parametrize('M,N,K,splits', [(65, 68, 320, (2, 3, 5)), (301, 72, 1024, (4, 8, 16))])
def test_split_adds_the_slices_in_order(ops, cuda, fmt, M, N, K, splits):
    """No epilogue operands, f32 output: the result is p_0 + p_1 + ... + p_{S-1} added in that order in f32, p_s = the split == 1 product over the
    columns of slice s; a second call gives the same bits."""
    mode, dt = _mode(ops, fmt)
    c = _case(cuda, dt, M, N, K, M + 5 * K)
    nk = K // 64
    for S in splits:
        want = None
        for s in range(S):
            k0, k1 = 64 * (s * nk // S), 64 * ((s + 1) * nk // S)
            p = ops.gemm_nt_skinny(mode, c.A[:, k0:k1], c.W[:, k0:k1], torch.empty(M, N, device=cuda), split=1)
            want = p if want is None else want + p
        got = ops.gemm_nt_skinny(mode, c.A, c.W, torch.empty(M, N, device=cuda), split=S)
        assert torch.equal(got, want), (S, rel(got, want))
        again = ops.gemm_nt_skinny(mode, c.A, c.W, torch.empty(M, N, device=cuda), split=S)
        assert torch.equal(again, got), S


@pytest.mark.parametrize('fmt', ['bf16', 'fp16'])
def test_split_every_epilogue_vs_f64(ops, cuda, fmt):
    """Two shapes of different sizes back to back on one workspace, filled with NaN before each pair of calls: a slab element that no workgroup
    wrote, or one left by the other call, would show."""
    mode, dt = _mode(ops, fmt)
    cases = [(_case(cuda, dt, 301, 264, 576, 11), 3), (_case(cuda, dt, 130, 768, 3072, 12), 8)]
    lib, _ = ops._sel(mode)
    need = max(lib.tcow_gemm_nt_skinny_workspace_bytes(c.M, c.N, S) for c, S in cases)
    ws = ops.workspace(need, cuda, 'nt_skinny')
    forms = [_forms(ops, c) for c, _ in cases]
    for i in range(len(forms[0])):
        ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(float('nan'))
        ran = []
        for (c, S), fs in zip(cases, forms):
            name, f32, alias, auxrole, kw = fs[i]
            call = lambda A, W, out, **k: ops.gemm_nt_skinny(mode, A, W, out, split=S, **k)
            ran.append((c, S, name, f32, alias, kw) + _run(call, cuda, c, f32, alias, auxrole, kw))
        assert ops.workspace(need, cuda, 'nt_skinny') is ws
        for c, S, name, f32, alias, kw, ob, ab in ran:
            want, want_aux = _reference(ops, c, alias, kw)
            err = rel(ob[:c.M, :c.N], want)
            assert err < (TOL32 if f32 else TOL16[fmt]), (name, S, err)
            assert ab is None or rel(ab[:c.M, :c.N], want_aux) < TOL16[fmt], (name, S)
            assert _guards_ok(ob, c.M, c.N) and _guards_ok(ab, c.M, c.N), (name, S)


@pytest.mark.parametrize('fmt', ['bf16', 'fp16'])
def test_refusals_name_the_argument_and_launch_nothing(ops, cuda, fmt):
    from tcow_amd import _lib as L
    mode, dt = _mode(ops, fmt)
    lib, dm = ops._sel(mode)
    M, N = 40, 64
    A = torch.randn(M, 256, device=cuda).to(dt); W = torch.randn(N, 256, device=cuda).to(dt)
    ws = torch.empty(8 * M * N * 4, dtype=torch.uint8, device=cuda)

    def call(K=256, split=2, wsp=ws, nbytes=None, dtype=dm):
        out = torch.full((M, N), SENT, device=cuda)
        a = L.GemmArgs(M, N, K, dtype, A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0), out.data_ptr(), out.stride(0), 1, None, None, None, 0,
                       L.ACT_NONE, None, 0, 0, None, None)
        need = lib.tcow_gemm_nt_skinny_workspace_bytes(M, N, split)
        rc = lib.tcow_gemm_nt_skinny(ops._stream(), ctypes.byref(a), split, wsp.data_ptr() if wsp is not None else None, need if nbytes is None else nbytes)
        torch.cuda.synchronize()
        return rc, lib.tcow_last_error().decode(), bool((out == SENT).all())

    rc, _, untouched = call()
    assert rc == 0 and not untouched                                              # the accepted call these are variations of
    assert lib.tcow_gemm_nt_skinny_workspace_bytes(M, N, 1) == 0 and lib.tcow_gemm_nt_skinny_workspace_bytes(M, N, 2) == 2 * M * N * 4
    need2 = 2 * M * N * 4
    for kw, word in [(dict(split=0), 'split'), (dict(split=17), 'split'), (dict(split=5), 'split'), (dict(K=96, split=1), 'K=96'),
                     (dict(nbytes=need2 - 1), 'workspace'), (dict(wsp=None), 'workspace'), (dict(dtype=L.TCOW_F32), 'dtype')]:
        rc, msg, untouched = call(**kw)
        assert rc != 0 and word in msg and untouched, (kw, rc, msg)
    with pytest.raises(L.TcowError, match='split'):
        ops.gemm_nt_skinny(mode, A, W, torch.empty(M, N, device=cuda), split=5)
    with pytest.raises(L.TcowError):
        ops.gemm_nt_skinny(ops.F32, A.float(), W.float(), torch.empty(M, N, device=cuda), split=1)

"""The 256-tile weight-gradient GEMM on 16x16x32 MFMAs: 32 token rows per MFMA step, two steps per 64-row stage.

GPU tests (exact integers, the kit of test_gpu_gemm_tn.py: operands in {-3 ... 3} behind a NaN tail, f64 reference, torch.equal):
  1. 32-token tails: M = 4096 + r, the rows at which a half-filled MFMA step or a half-filled stage first appears;
  2. the general path (SCHED = 1): an edge tile in n, and strided operands with an edge tile in k;
  3. the grouped launch, through the slab + fold path and through the in-place (one slice) path;
  4. full-range operands against the derived accumulation bound.
That every shape here reaches the kernel form it was chosen for is asserted on the CPU by tests/test_gemm_tn_plan_host.py, which also holds the
check of the LDS image (tools/tn_layout_check.cpp)."""
import pytest
import torch

from test_gpu_gemm_tn import Out, _mode, _operands, _reference

MODES16 = ['bf16', 'fp16']
TAILS = [1, 15, 16, 17, 31, 32, 33, 48, 63]


@pytest.fixture(scope='module')
def ops(cuda):
    from tcow_amd import ops as o
    return o


@pytest.fixture(scope='module')
def refs():
    cache = {}
    yield cache
    cache.clear()


# ---- 1
@pytest.mark.gpu
@pytest.mark.parametrize('mname', MODES16)
def test_32_token_tails(ops, cuda, mname):
    """N = K = 768: 9 whole tiles, gemm_tn_bf16_256_kernel<2>.  M = 4096 + r asks for 16 slices: mps = 320, nz = 13, the last slice has 256 + r
    rows = 4 stages and r rows of a fifth: r < 32 leaves its first MFMA step part-filled and its second empty, r = 32 fills one step exactly,
    32 < r < 64 part-fills the second.  Every M is a prefix of one master buffer, so the rows behind M hold real integers up to the last M and
    NaN behind that: a row past M that does not act as zero changes an integer or makes a NaN."""
    mode, dt = _mode(ops, mname)
    N = K = 768
    Ms = [4096 + r for r in TAILS]
    dY, X = _operands(cuda, dt, Ms[-1], N, K)
    dYd, Xd = dY.double(), X.double()
    cur, w, b = Ms[0], dYd[:Ms[0]].t() @ Xd[:Ms[0]], dYd[:Ms[0]].sum(0)
    for M in Ms:
        if M > cur:
            w += dYd[cur:M].t() @ Xd[cur:M]
            b += dYd[cur:M].sum(0)
            cur = M
        out = Out(cuda, N, K)
        ops.gemm_tn(mode, dY[:M], X[:M], out.dW, bias_grad=out.db)
        out.check((w, b), f'{mname} M={M} N={N} K={K}')


# ---- 2
@pytest.mark.gpu
@pytest.mark.parametrize('mname', MODES16)
@pytest.mark.parametrize('r', [17, 33])
@pytest.mark.parametrize('form', ['edge_n', 'strided_edge_k'])
def test_general_path(ops, cuda, refs, mname, r, form):
    """SCHED = 1.  edge_n: N = 776, K = 768 (4 x 3 tiles, the last tile row has 8 columns of dY: guarded loads, guarded stores).
    strided_edge_k: N = 768, K = 776 with ld = N + 8, K + 8 and NaN in the pad columns (3 x 4 tiles, the last tile column has 8 columns of X)."""
    mode, dt = _mode(ops, mname)
    M = 4096 + r
    N, K, strided = (776, 768, False) if form == 'edge_n' else (768, 776, True)
    dY, X = _operands(cuda, dt, M, N, K, strided=strided)
    if strided:
        assert dY.stride(0) == N + 8 and X.stride(0) == K + 8
    out = Out(cuda, N, K)
    ops.gemm_tn(mode, dY, X, out.dW, bias_grad=out.db)
    out.check(_reference(refs, dY, X), f'{mname} {form} M={M} N={N} K={K}')


# ---- 3
GM = 4096 + 17
PAIR = [(768, 768), (2304, 768)]


def _group(ops, dev, refs, mname, copies):
    mode, dt = _mode(ops, mname)
    operands = {nk: _operands(dev, dt, GM, nk[0], nk[1]) for nk in PAIR}
    probs, outs, want = [], [], []
    for _ in range(copies):
        for N, K in PAIR:
            dY, X = operands[(N, K)]
            o = Out(dev, N, K)
            probs.append((dY, X, o.dW, o.db, 0))
            outs.append(o)
            want.append(_reference(refs, dY, X))
    ops.gemm_tn_grouped(mode, probs)
    for i, (o, w) in enumerate(zip(outs, want)):
        o.check(w, f'{mname} group of {len(probs)}, problem {i} {tuple(o.dW.shape)}')


@pytest.mark.gpu
@pytest.mark.parametrize('mname', MODES16)
def test_grouped_slab_and_fold(ops, cuda, refs, mname):
    """768 x 768 and 2304 x 768 at M = 4113: 9 + 27 = 36 tiles; the group plan (tcow_tn_group_slices, gemm_tn_plan.h) picks 7 slices (252 workgroups, cost 1.016 + 0.308):
    mps = 640, the last slice has 273 rows = 4 stages + 17 rows; seven slabs per weight, folded by the group fold launch."""
    _group(ops, cuda, refs, mname, 1)


@pytest.mark.gpu
@pytest.mark.parametrize('mname', MODES16)
def test_grouped_one_slice_in_place(ops, cuda, refs, mname):
    """One slice.  The C ABI has no slice argument, so the group is filled until the library's own rule asks for one: seven copies of the pair,
    each with outputs of its own, are 252 tiles -- cost(1) = 256 / 252 + 0.044 = 1.060 against cost(2) = 512 / 504 + 0.088 = 1.104.  Every
    workgroup then walks all 4113 rows (64 stages + 17 rows) and stores its accumulators straight into the dense dW: no slab, no fold."""
    assert 14 <= ops.tn_group_max()
    _group(ops, cuda, refs, mname, 7)


# ---- 4
@pytest.mark.gpu
@pytest.mark.parametrize('mname', MODES16)
def test_full_range_operands(ops, cuda, mname):
    """Standard-normal operands rounded to the mode's dtype, M = 4096 + 33, N = K = 768.  A product of two 16-bit operands (8 or 11 significand
    bits each) is exact in f32, so the only error is that of adding M numbers in f32 in some order: |got - want| <= gamma * (|dY|^T |X|)
    elementwise with gamma = M u / (1 - M u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: any order).
    The bias gradient is a sum of M operands: the same bound on sum |dY|.  The integers of the other tests never set the low significand
    bits of an operand; these do."""
    mode, dt = _mode(ops, mname)
    M, N, K = 4096 + 33, 768, 768
    g = torch.Generator(device=cuda).manual_seed(20241)
    dY = torch.randn(M, N, device=cuda, generator=g).to(dt)
    X = torch.randn(M, K, device=cuda, generator=g).to(dt)
    out = Out(cuda, N, K)
    ops.gemm_tn(mode, dY, X, out.dW, bias_grad=out.db)
    dYd, Xd = dY.double(), X.double()
    u = 2.0 ** -24
    gamma = M * u / (1 - M * u)
    err_w = (out.dW.double() - dYd.t() @ Xd).abs()
    bound_w = gamma * (dYd.abs().t() @ Xd.abs())
    err_b = (out.db.double() - dYd.sum(0)).abs()
    bound_b = gamma * dYd.abs().sum(0)
    print(f'{mname}: dW max err / bound {float((err_w / bound_w).max()):.3f}, bias {float((err_b / bound_b).max()):.3f}')
    assert not bool(out.dW.isnan().any()) and bool((err_w <= bound_w).all()), f'dW: {int((err_w > bound_w).sum())} entries beyond the bound, worst ratio {float((err_w / bound_w).max())}'
    assert bool((err_b <= bound_b).all()), f'bias_grad: worst ratio {float((err_b / bound_b).max())}'
    assert out.guards_ok()

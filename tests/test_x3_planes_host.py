"""CPU: the oracle of the exact bf16 x 3 GEMM checks (kernel_forms.hi_lo_operand / planes / want_hi_lo; used by test_gpu_gemm_x3_planes.py and
test_gpu_gemm_skinny.py), proved at the longest contraction those modules may use, X3_MAX_CONTRACTION = 1800.

The kernels split every f32 operand x into hi = bf16(x) and lo = bf16(x - hi) and accumulate lo hi + hi lo + hi hi in f32, in an order that depends on
the k-slices, the split-K slabs and their fold.  The GPU tests compare with hi_A hi_B^T + hi_A lo_B^T + lo_A hi_B^T taken in f64 and allow no
tolerance; that is sound only if (1) the generator's planes are what the split gives, (2) every partial sum of kept terms is exactly representable
in f32 and (3) a kernel that drops, doubles or mixes up a plane gives another number.  Each is asserted here, without a GPU."""
import torch

from kernel_forms import X3_MAX_CONTRACTION, hi_lo_operand, planes, want_hi_lo

K = X3_MAX_CONTRACTION
M, N = 6, 5


def _pair(seed=1800):
    g = torch.Generator().manual_seed(seed)
    return hi_lo_operand(g, (M, K), 'cpu'), hi_lo_operand(g, (N, K), 'cpu')


def test_the_limit_is_the_one_the_bound_gives():
    """Per k the kept terms are at most 3 x 3 + 2 x 3 x 3 / 1024 < 9.02 in magnitude, in units of 2^-10."""
    assert 9 + 18 / 1024 < 9.02 and 9.02 * 1024 * X3_MAX_CONTRACTION < 2 ** 24
    assert 9.02 * 1024 * (X3_MAX_CONTRACTION + 20) > 2 ** 24          # (the limit is not slack: no case may quietly grow past it)


def test_generator_gives_its_planes():
    A, B = _pair()
    for x in (A, B):
        assert x.dtype == torch.float32
        h = torch.round(x)                                             # (|l| <= 3 / 1024: h is the nearest integer)
        l = (x - h) * 1024
        assert set(h.unique().tolist()) == {-3.0, -2.0, 2.0, 3.0} and set(l.unique().tolist()) == {float(v) for v in range(-3, 4)}
        hi, lo = planes(x)
        assert torch.equal(hi, x.bfloat16().double()) and torch.equal(lo, (x - x.bfloat16().float()).bfloat16().double())
        assert torch.equal(hi, h.double()) and torch.equal(lo * 1024, l.double())
        assert torch.equal(hi + lo, x.double()) and bool((lo != 0).any())


def test_want_is_exact_in_f32():
    A, B = _pair()
    want = want_hi_lo(A, B)
    assert float(want.abs().max()) * 1024 < 2 ** 24
    assert torch.equal((want * 1024).round(), want * 1024)
    assert torch.equal(want.float().double(), want)
    # the sum of the magnitudes of all kept terms bounds every partial sum in every order
    (ah, al), (bh, bl) = planes(A), planes(B)
    mags = ah.abs() @ bh.abs().t() + ah.abs() @ bl.abs().t() + al.abs() @ bh.abs().t()
    assert float(mags.max()) * 1024 < 2 ** 24


def test_f32_chain_in_random_order_equals_want():
    """All 3 K terms of every output element, added one at a time in f32 in one random order (the three kinds interleaved): the bits of `want`."""
    A, B = _pair()
    want = want_hi_lo(A, B)
    (ah, al), (bh, bl) = (tuple(p.float() for p in planes(x)) for x in (A, B))
    # terms[t] is the [M, N] outer product of term t: kind 0 = lo hi, 1 = hi lo, 2 = hi hi at k = t // 3
    terms = torch.stack([al[:, None, :] * bh[None, :, :], ah[:, None, :] * bl[None, :, :], ah[:, None, :] * bh[None, :, :]], -1).reshape(M, N, 3 * K)
    assert terms.dtype == torch.float32
    for seed in (0, 1):
        order = torch.randperm(3 * K, generator=torch.Generator().manual_seed(seed)).tolist()
        acc = torch.zeros(M, N, dtype=torch.float32)
        for t in order:
            acc = acc + terms[:, :, t]
        assert acc.dtype == torch.float32 and torch.equal(acc.double(), want), seed
    # and as the kernel does it: slices of 32 k, three terms per k, then a fold of split-K slabs of 288 k
    slabs = []
    for k0 in range(0, K, 288):
        acc = torch.zeros(M, N, dtype=torch.float32)
        for k in range(k0, min(k0 + 288, K)):
            for kind in range(3):
                acc = acc + terms[:, :, 3 * k + kind]
        slabs.append(acc)
    total = slabs[0]
    for s in slabs[1:]:
        total = total + s
    assert torch.equal(total.double(), want)


def test_a_wrong_plane_changes_want():
    """What makes the GPU assertions discriminating: each cross term and the dropped lo lo term are visible, and so is lo taken for hi."""
    A, B = _pair()
    want = want_hi_lo(A, B)
    (ah, al), (bh, bl) = planes(A), planes(B)
    hh, hl, lh, ll = ah @ bh.t(), ah @ bl.t(), al @ bh.t(), al @ bl.t()
    assert torch.equal(want, hh + hl + lh)
    for name, other in (('hi lo dropped', hh + lh), ('lo hi dropped', hh + hl), ('lo lo added', hh + hl + lh + ll), ('hi hi twice for lo hi', 2 * hh + hl),
                        ('lo lo for hi lo', hh + ll + lh), ('the full product', A.double() @ B.double().t())):
        assert not torch.equal(want, other), name
    # confined to one 32-wide k-slice, one row of one operand: still another number
    al2 = al.clone(); al2[0, 64:96] = 0
    assert not torch.equal(want, hh + hl + al2 @ bh.t())

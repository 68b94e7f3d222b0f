"""Helpers shared by test_gpu_layernorm_forms.py, test_gpu_glue_forms.py and test_gpu_gemm_nt.py: outputs that live inside larger buffers pre-filled with a sentinel, so
that a kernel form which writes a dead lane, a pad column or a row past the end is seen (NaN for floats: it also poisons any result that read it).
And the exact hi / lo oracle of the bf16 x 3 GEMM tests (hi_lo_operand, planes, want_hi_lo), shared by test_gpu_gemm_skinny.py, test_gpu_gemm_x3_planes.py
and test_x3_planes_host.py."""
import torch

NAN = float('nan')


def bits(t):
    """The tensor's storage bits as integers of the same width (NaN sentinels compare equal bit for bit, any stride)."""
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def guarded(rows, cols, pitch, dtype, device):
    """([rows + 1, pitch] buffer of NaN, its [:rows, :cols] view): pitch - cols pad columns (none for a dense pitch) and one spare row."""
    assert pitch >= cols
    buf = torch.full((rows + 1, pitch), NAN, dtype=dtype, device=device)
    return buf, buf[:rows, :cols]


def guarded_flat(n, dtype, device, spare=8):
    """([n + spare] buffer of NaN, its [:n] view) for dense outputs: the spare elements stand behind the last one."""
    buf = torch.full((n + spare,), NAN, dtype=dtype, device=device)
    return buf, buf[:n]


def assert_guarded(buf, rows, cols, what=''):
    """Everything outside buf[:rows, :cols] is still the sentinel bit for bit, everything inside is finite."""
    want = bits(torch.full_like(buf, NAN))
    got = bits(buf)
    assert torch.equal(got[rows:], want[rows:]), f'{what}: wrote a row past the end'
    assert torch.equal(got[:rows, cols:], want[:rows, cols:]), f'{what}: wrote a pad column'
    assert bool(torch.isfinite(buf[:rows, :cols].float()).all()), f'{what}: an element inside the view was not written (or is not finite)'


def assert_guarded_flat(buf, n, what=''):
    want = bits(torch.full_like(buf, NAN))
    assert torch.equal(bits(buf)[n:], want[n:]), f'{what}: wrote past the end'
    assert bool(torch.isfinite(buf[:n].float()).all()), f'{what}: an element was not written (or is not finite)'


def assert_untouched(buf, what=''):
    """An output that was not asked for: the whole buffer keeps its sentinel."""
    assert torch.equal(bits(buf), bits(torch.full_like(buf, NAN))), f'{what}: an absent output was written'


# ---- the exact oracle of the bf16 x 3 GEMMs (test_gpu_gemm_skinny.py, test_gpu_gemm_x3_planes.py; proved on the CPU by test_x3_planes_host.py)
X3_MAX_CONTRACTION = 1800       # 9.02 x 1024 x 1800 < 2^24: up to this contraction length every partial sum of kept terms is exact in f32 (want_hi_lo)


def hi_lo_operand(gen, shape, device):
    """x = h + l with h uniform in {+-2, +-3} and l uniform in {-3 .. 3} 2^-10: bf16(x) = h and bf16(x - h) = l exactly (the half ulp of bf16
    in 2 .. 4 is 2^-8 or more).  Drawn on the generator's device, returned on `device`."""
    r = lambda lo, hi: torch.randint(lo, hi, tuple(shape), device=gen.device, generator=gen).float()
    x = r(2, 4) * (r(0, 2) * 2 - 1) + r(-3, 4) / 1024.0
    return x.to(device)


def planes(x):
    """(hi, lo) of an f32 tensor in f64, taken with torch's own bf16 cast (round to nearest even), not the library's."""
    h = x.bfloat16().float()
    return h.double(), (x - h).bfloat16().double()


def want_hi_lo(A, B):
    """What a bf16 x 3 kernel must give for A [M, K] and B [N, K] made by hi_lo_operand, in f64:
        hi_A hi_B^T + hi_A lo_B^T + lo_A hi_B^T
    Every kept term is a multiple of 2^-10 and at most 9.02 per k (9 + 2 x 9 / 1024), so every partial sum stays below 2^24 of those units up to
    K = X3_MAX_CONTRACTION: the f32 output is this value exactly, in any order.  Asserts what makes the comparison discriminating: hi + lo is the
    operand, both lo planes are non-zero, and the dropped lo lo term is visible."""
    assert A.shape[1] == B.shape[1] <= X3_MAX_CONTRACTION
    (ah, al), (bh, bl) = planes(A), planes(B)
    assert torch.equal(ah + al, A.double()) and torch.equal(bh + bl, B.double()) and bool((al != 0).any()) and bool((bl != 0).any())
    want = ah @ bh.t() + ah @ bl.t() + al @ bh.t()
    assert not torch.equal(want, A.double() @ B.double().t())
    return want

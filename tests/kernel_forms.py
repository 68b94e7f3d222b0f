"""Helpers shared by test_gpu_layernorm_forms.py, test_gpu_glue_forms.py and test_gpu_gemm_nt.py: outputs that live inside larger buffers pre-filled with a sentinel, so
that a kernel form which writes a dead lane, a pad column or a row past the end is seen (NaN for floats: it also poisons any result that read it)."""
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

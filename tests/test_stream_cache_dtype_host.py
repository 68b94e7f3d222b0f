"""CPU: the host side of the compact K / V cache of a stream (net.stream(cache_dtype=...), tcow_amd/stream.py) -- the one function that decides
the cache's element type, for every (precision, keyword) pair with its refusals, and the ABI of the step record that carries it (tests/stream_abi.py)."""
import ctypes
import re

import pytest
import torch

import stream_abi as abi
from tcow_amd import _lib, ops, stream
from tcow_amd._lib import TcowError

# precision -> the ops mode a module of that precision stores in (seeker.py: bf16x3 stores f32)
MODES = {'fp32': ops.F32, 'bf16x3': ops.F32, 'bf16': ops.BF16, 'fp16': ops.FP16}


@pytest.mark.parametrize('precision,keyword,want', [
    ('fp32', None, (torch.float32, None)), ('bf16x3', None, (torch.float32, None)),
    ('bf16', None, (torch.bfloat16, None)), ('fp16', None, (torch.float16, None)),                      # None: the storage type, the old symbols
    ('fp32', 'bf16', (torch.bfloat16, _lib.TCOW_BF16)), ('bf16x3', 'bf16', (torch.bfloat16, _lib.TCOW_BF16)),
    ('bf16', 'bf16', (torch.bfloat16, None)),                                                          # the storage type already: equals None
    ('fp32', 'fp8', (torch.float8_e4m3fn, _lib.TCOW_FP8E4M3)), ('bf16x3', 'fp8', (torch.float8_e4m3fn, _lib.TCOW_FP8E4M3)),
    ('bf16', 'fp8', (torch.float8_e4m3fn, _lib.TCOW_FP8E4M3)), ('fp16', 'fp8', (torch.float8_e4m3fn, _lib.TCOW_FP8E4M3)),
])
def test_cache_plan_of_every_precision_and_keyword(precision, keyword, want):
    assert stream.cache_plan(MODES[precision], keyword) == want


def test_cache_plan_refusals():
    with pytest.raises(TcowError, match=r"cache_dtype='bf16' with precision='fp16'"):
        stream.cache_plan(ops.FP16, 'bf16')
    for bad in ('fp16', 'e5m2', 'FP8', 8, torch.float8_e4m3fn, ''):
        for mode in set(MODES.values()):
            with pytest.raises(TcowError, match=r"must be None, 'bf16' or 'fp8'"):
                stream.cache_plan(mode, bad)


def test_cache_bytes_formula_at_configs1():
    """The figures of DESIGN.md section 9, from the shapes alone: per query row at configs[1] (T = 30, 240x320: S - 1 = 300 patches; depth 12,
    D = 768) K and V caches of depth x (S - 1) x D x T elements each and depth f32 cls rows."""
    def nbytes(elem):
        return 2 * 12 * 300 * 768 * 30 * elem + 12 * 768 * 4
    assert nbytes(1) == 165_924_864 and nbytes(2) == 331_812_864 and nbytes(4) == 663_588_864
    assert torch.empty(0, dtype=torch.float8_e4m3fn).element_size() == 1


def test_the_cq_entry_points_are_new_symbols_of_abi_14():
    """Since ABI 16 the cache element type is a field of the one step record, always present: no entry point of its own."""
    hdr, code = abi.header()
    abi.check_version()
    assert int(re.search(r'#define\s+TCOW_FP8E4M3\s+(\d+)', hdr).group(1)) == _lib.TCOW_FP8E4M3 == ops.FP8 == 3
    assert len({_lib.TCOW_F32, _lib.TCOW_BF16, _lib.TCOW_F32X3, _lib.TCOW_FP8E4M3}) == 4
    abi.check_header_and_records()
    assert ('cache_dtype', ctypes.c_int) in abi.header_fields(code, 'tcow_stream_attn_args')
    assert not any('_cq' in name for name in _lib.SIGNATURES) and '_cq_fwd' not in code


def test_both_builds_export_the_cq_entry_points():
    """Both builds export the step's two entry points with the declared argument types, and none of the eight attention symbols they replaced."""
    abi.check_builds_export()
    abi.check_old_symbols_are_gone([n for n in abi.OLD if 'attn' in n])

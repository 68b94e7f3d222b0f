"""CPU: the routing rules of the skinny-M NT GEMMs (ops.skinny_plan for the 16-bit modes, ops.skinny_plan_x3 for bf16 x 3; host arithmetic
only), their entry points in the C ABI and the Python surface around them."""
import ctypes
import inspect
import json
import os
import re

import pytest

from conftest import ROOT

WEIGHTS = [(768, 768), (2304, 768), (3072, 768), (768, 3072)]          # (N, K) of a ViT-B block: qkv, proj / temporal fc, fc1, fc2
STREAM_M = [301, 1201, 2408]                                           # one-frame steps: configs[1] B = 1, configs[3] B = 1, configs[1] B = 8


def _plan():
    from tcow_amd import ops
    return ops.skinny_plan


def test_plan_leaves_the_clip_and_training_shapes_alone():
    plan = _plan()
    for N, K in WEIGHTS:
        assert plan(27090, N, K) == 0
    for K in (96, 100, 767, 32, 1):
        assert plan(301, 768, K) == 0
    for M, N in [(2048, 2048), (128 * 256, 128), (128, 128 * 256), (4000, 1024), (2408, 2304), (2408, 3072)]:
        assert -(-M // 128) * -(-N // 128) >= 256 and plan(M, N, 768) == 0


def test_plan_routes_the_stream_shapes_within_the_kernels_limits():
    plan = _plan()
    routed = 0
    for M in STREAM_M:
        for N, K in WEIGHTS:
            S = plan(M, N, K)
            if -(-M // 128) * -(-N // 128) >= 256:
                assert S == 0
                continue
            if S:
                routed += 1
                assert 1 <= S <= min(K // 64, 16), (M, N, K, S)
    assert routed >= 1
    assert plan(1, 4, 64) in (0, 1)                                                       # one k-slice cannot be split


def test_plan_is_monotone():
    """More rows (more tiles) never raise the split; a longer K never lowers it."""
    plan = _plan()
    for N, K in WEIGHTS:
        prev = None
        for M in range(1, 4200, 37):
            S = plan(M, N, K)
            if S == 0:
                continue
            assert prev is None or S <= prev, (M, N, K, S, prev)
            prev = S
    for M in STREAM_M:
        for N in (768, 2304, 3072):
            seq = [plan(M, N, K) for K in range(64, 4097, 64)]
            routed = [s for s in seq if s]
            assert routed == sorted(routed), (M, N, seq)


def test_plan_reproduces_the_measured_table():
    """profiles/gemm_skinny.json (tools/dev_gemm_skinny.py) states per shape what the measurement asks of the rule: 'route' false = today's kernel
    holds the shape; true = the skinny entry point with one of 'accept', the splits within the best one's spread."""
    path = os.path.join(ROOT, 'profiles', 'gemm_skinny.json')
    rows = json.load(open(path))['shapes']
    assert len(rows) == 12
    plan = _plan()
    for r in rows:
        S = plan(r['M'], r['N'], r['K'])
        if r['route']:
            assert S in r['accept'], (r['M'], r['N'], r['K'], S, r['accept'])
        else:
            assert S == 0, (r['M'], r['N'], r['K'], S)


def test_abi_14_declares_the_two_entry_points():
    from tcow_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'tcow_hip.h')).read()
    assert int(re.search(r'#define\s+TCOW_ABI_VERSION\s+(\d+)', hdr).group(1)) == 16 and _lib.ABI_VERSION == 16
    assert re.search(r'long\s+tcow_gemm_nt_skinny_workspace_bytes\(int M, int N, int split\);', hdr)
    assert re.search(r'int\s+tcow_gemm_nt_skinny\(void\* stream, const tcow_gemm_args\* args, int split, void\* workspace, long workspace_bytes\);', hdr)
    i, l, vp = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    assert _lib.SIGNATURES['tcow_gemm_nt_skinny_workspace_bytes'] == (l, [i, i, i])
    assert _lib.SIGNATURES['tcow_gemm_nt_skinny'] == (i, [vp, ctypes.POINTER(_lib.GemmArgs), i, vp, l])
    for fmt in ('bf16', 'fp16'):
        lib = _lib.lib(fmt)
        assert lib.tcow_version() == 16
        assert lib.tcow_gemm_nt_skinny_workspace_bytes(301, 768, 1) == 0 and lib.tcow_gemm_nt_skinny_workspace_bytes(301, 768, 4) == 4 * 301 * 768 * 4


def test_public_keyword_and_default():
    """net.stream / net.stream_pool take skinny_gemm; its default is the measured constant of tcow_amd/stream.py."""
    from tcow_amd import ops, seeker, stream
    for cls in (seeker.QueryMaskTracker, seeker.Seeker):
        for name in ('stream', 'stream_pool'):
            assert inspect.signature(getattr(cls, name)).parameters['skinny_gemm'].default is None
    assert isinstance(stream.SKINNY_GEMM_DEFAULT, bool)
    assert inspect.signature(ops.gemm_nt).parameters['skinny'].default is False


def test_abi_14_declares_the_x3_entry_point():
    from tcow_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'tcow_hip.h')).read()
    assert int(re.search(r'#define\s+TCOW_ABI_VERSION\s+(\d+)', hdr).group(1)) == 16 and _lib.ABI_VERSION == 16
    assert re.search(r'int\s+tcow_gemm_nt_skinny_x3\(void\* stream, const tcow_gemm_args\* args, int split, void\* workspace, long workspace_bytes\);', hdr)
    i, l, vp = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    assert _lib.SIGNATURES['tcow_gemm_nt_skinny_x3'] == (i, [vp, ctypes.POINTER(_lib.GemmArgs), i, vp, l])
    assert _lib.SIGNATURES['tcow_gemm_nt_skinny'] == (i, [vp, ctypes.POINTER(_lib.GemmArgs), i, vp, l])       # (unchanged)
    for fmt in ('bf16', 'fp16'):
        lib = _lib.lib(fmt)
        assert lib.tcow_version() == 16
        assert hasattr(lib, 'tcow_gemm_nt_skinny_x3')


def test_plan_x3_properties():
    from tcow_amd import ops
    plan = ops.skinny_plan_x3
    for N, K in WEIGHTS:
        assert plan(27090, N, K) == 0                                  # the clip and training shapes stay on tcow_gemm_nt
    for K in (96, 100, 767, 32, 1):
        assert plan(301, 768, K) == 0                                  # K the entry point refuses
    for M, N in [(2048, 2048), (128 * 256, 128), (4000, 1024)]:
        assert -(-M // 128) * -(-N // 128) >= 256 and plan(M, N, 768) == 0
    for M in list(range(1, 4200, 37)) + STREAM_M + [14, 28, 30]:
        for N, K in WEIGHTS + [(128, 128), (512, 128), (128, 512), (4, 64), (768, 64)]:
            S = plan(M, N, K)
            assert S == 0 or S in ops.SKINNY_SPLITS, (M, N, K, S)
            assert S <= K // 64, (M, N, K, S)
    assert plan(1, 4, 64) in (0, 1)                                    # one k-slice cannot be split
    for N in (766, 770, 3 * 15 * 15):
        assert plan(301, N, 768) == 0                                  # N the entry point refuses (an odd patch size: a head of 3 P^2 columns)
    for M in (14, 28, 30):
        for N, K in [(128, 128), (384, 128), (512, 128), (128, 512)]:
            assert plan(M, N, K) in (0, 1)                             # K <= 512 never splits (tests/test_gpu_stream_skinny.py, the d128 net)


def test_plan_x3_reproduces_the_measured_table():
    """profiles/gemm_skinny_x3.json (tools/dev_gemm_skinny.py --x3) states per shape what the measurement asks of the rule: 'route' false =
    tcow_gemm_nt holds the shape; true = the skinny entry point with one of 'accept', the splits within the best one's spread."""
    from tcow_amd import ops
    rows = json.load(open(os.path.join(ROOT, 'profiles', 'gemm_skinny_x3.json')))['shapes']
    assert len(rows) == 12 and {(r['M'], r['N'], r['K']) for r in rows} == {(M, N, K) for M in STREAM_M for N, K in WEIGHTS}
    for r in rows:
        S = ops.skinny_plan_x3(r['M'], r['N'], r['K'])
        if r['route']:
            assert S in r['accept'], (r['M'], r['N'], r['K'], S, r['accept'])
        else:
            assert S == 0, (r['M'], r['N'], r['K'], S)


def test_plan_x3_reproduces_the_small_net_table():
    """profiles/gemm_skinny_x3_small.json (the same tool with --rows 14,30): the four weight shapes at the row counts of a 32 x 48-pixel net's steps."""
    from tcow_amd import ops
    rows = json.load(open(os.path.join(ROOT, 'profiles', 'gemm_skinny_x3_small.json')))['shapes']
    assert {(r['M'], r['N'], r['K']) for r in rows} == {(M, N, K) for M in (14, 30) for N, K in WEIGHTS}
    for r in rows:
        S = ops.skinny_plan_x3(r['M'], r['N'], r['K'])
        assert (S in r['accept']) if r['route'] else S == 0, (r['M'], r['N'], r['K'], S, r['accept'])


def test_the_16_bit_entry_point_and_gemm_nt_are_unchanged(monkeypatch):
    import torch
    from tcow_amd import _lib, ops
    x = torch.zeros(64, 64)
    monkeypatch.setattr(ops, '_need_cuda', lambda *ts: None)           # (the mode is refused before anything touches the device)
    for mode in (ops.F32X3, ops.F32):
        with pytest.raises(_lib.TcowError, match='16-bit modes only'):
            ops.gemm_nt_skinny(mode, x, x, x, split=1)
    assert str(inspect.signature(ops.gemm_nt)) == ('(mode, A, W, out, bias=None, row_scale=None, resid=None, act=0, aux=None, tile=0, bias2=None, '
                                                   'row_scale2=None, skinny=False)')
    assert list(inspect.signature(ops.gemm_nt_skinny_x3).parameters) == ['A', 'W', 'out', 'bias', 'row_scale', 'resid', 'act', 'aux', 'bias2', 'row_scale2', 'split']
    assert inspect.signature(ops.gemm_nt_skinny_x3).parameters['split'].default == 1


def test_default_constant():
    from tcow_amd import stream
    assert isinstance(stream.SKINNY_GEMM_X3_DEFAULT, bool) and isinstance(stream.SKINNY_GEMM_DEFAULT, bool)

"""CPU: the host-side refusals of tcow_gemm_nt (csrc/api.cpp gemm_nt_dispatch, csrc/gemm_bf16.hip tcow_gemm_nt_bf16), against both builds.

Each case breaks exactly one thing of an otherwise valid tcow_gemm_args and expects TCOW_ERR_INVALID_ARG (-1) with the check's own message.  No case
reaches a launch (the pointers are never dereferenced), so no GPU is needed.  Where two checks could both fire, the ORDER cases pin which one is
reported: the dispatcher's checks run in source order, before the dtype is looked at, and the 16-bit launcher's run in source order behind them.

tcow_gemm_nt_f32 (gemm_f32.hip) and tcow_gemm_nt_x3 (gemm_x3.hip) have no check of their own in front of their launch: the f32-storage kernels
take any K, any pitch and any alignment (scalar loaders and scalar stores).  What refuses a TCOW_F32 / TCOW_F32X3 call before a launch is the
dispatcher alone, so its cases run with all three dtypes and the 16-bit launcher's with TCOW_BF16 (the 16-bit dtype of either build)."""
import ctypes

import pytest

BUILDS = ('bf16', 'fp16')
PTR = 4096                        # any non-null, 16-byte-aligned address: a refused call does not touch it
M, N, K = 330, 264, 128


def gemm_args(_lib, dtype, **kw):
    f = dict(M=M, N=N, K=K, dtype=dtype, A=PTR, lda=K, W=PTR, ldw=K, C=PTR, ldc=N, out_f32=0, bias=None, row_scale=None, resid=None, ldr=0,
             act=_lib.ACT_NONE, aux=None, ldaux=0, tile=0, bias2=None, row_scale2=None)
    assert set(kw) <= set(f), kw
    f.update(kw)
    return _lib.GemmArgs(**f)


def refused(lib, a):
    status = lib.tcow_gemm_nt(None, ctypes.byref(a))
    return status, lib.tcow_last_error().decode()


# ---- api.cpp: gemm_nt_dispatch (every dtype)
DISPATCH = [
    (dict(M=0), 'tcow_gemm_nt: bad shape M=0 N=264 K=128'),
    (dict(M=-5), 'tcow_gemm_nt: bad shape M=-5 N=264 K=128'),
    (dict(N=0), 'tcow_gemm_nt: bad shape M=330 N=0 K=128'),
    (dict(K=0), 'tcow_gemm_nt: bad shape M=330 N=264 K=0'),
    (dict(K=-64), 'tcow_gemm_nt: bad shape M=330 N=264 K=-64'),
    (dict(A=None), 'tcow_gemm_nt: null operand'),
    (dict(W=None), 'tcow_gemm_nt: null operand'),
    (dict(C=None), 'tcow_gemm_nt: null operand'),
    (dict(act=2), 'tcow_gemm_nt: this activation needs aux'),                 # TCOW_ACT_DGELU
    (dict(act=3), 'tcow_gemm_nt: this activation needs aux'),                 # TCOW_ACT_GELU_DSAVE
    (dict(act=4), 'tcow_gemm_nt: this activation needs aux'),                 # TCOW_ACT_MUL_AUX
    (dict(act=5), 'tcow_gemm_nt: unknown activation 5'),
    (dict(act=-1), 'tcow_gemm_nt: unknown activation -1'),
    (dict(act=5, aux=PTR, ldaux=N), 'tcow_gemm_nt: unknown activation 5'),
    (dict(row_scale2=PTR), 'tcow_gemm_nt: row_scale2 without bias2'),
    # ORDER: shape before operands before aux before the activation's range before row_scale2 -- and all of them before the dtype
    (dict(M=0, A=None), 'tcow_gemm_nt: bad shape M=0 N=264 K=128'),
    (dict(W=None, act=2), 'tcow_gemm_nt: null operand'),
    (dict(act=4, row_scale2=PTR), 'tcow_gemm_nt: this activation needs aux'),
    (dict(act=9, row_scale2=PTR), 'tcow_gemm_nt: unknown activation 9'),
    (dict(row_scale2=PTR, dtype=7), 'tcow_gemm_nt: row_scale2 without bias2'),
    (dict(C=None, K=100, lda=3, tile=7), 'tcow_gemm_nt: null operand'),       # ... and before anything the 16-bit launcher would say
]


@pytest.mark.parametrize('fmt', BUILDS)
def test_dispatcher_refusals(fmt):
    from tcow_amd import _lib
    lib = _lib.lib(fmt)
    assert acts_match(_lib)
    for dtype in (_lib.TCOW_BF16, _lib.TCOW_F32, _lib.TCOW_F32X3):
        for kw, message in DISPATCH:
            kw = dict(kw)
            kw.setdefault('dtype', dtype)
            assert refused(lib, gemm_args(_lib, **kw)) == (-1, message), (dtype, kw)


def acts_match(_lib):
    """The literal activation numbers of the tables above are the ABI's."""
    return (_lib.ACT_NONE, _lib.ACT_GELU, _lib.ACT_DGELU, _lib.ACT_GELU_DSAVE, _lib.ACT_MUL_AUX) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize('fmt', BUILDS)
def test_null_args_and_unknown_dtype(fmt):
    from tcow_amd import _lib
    lib = _lib.lib(fmt)
    assert (lib.tcow_gemm_nt(None, None), lib.tcow_last_error().decode()) == (-1, 'tcow_gemm_nt: null args')
    for dtype in (3, 7, -1, 16):                 # (16 is ops.FP16, a Python-side mode: the binary16 build's ABI dtype is TCOW_BF16)
        assert refused(lib, gemm_args(_lib, dtype)) == (-1, f'tcow_gemm_nt: unknown dtype {dtype}'), dtype


# ---- gemm_bf16.hip: tcow_gemm_nt_bf16 (the 16-bit dtype)
C2 = 'tcow_gemm_nt(bf16): tile 160 needs K % 128 == 0 and operands below 2 GiB'
LDAB = 'tcow_gemm_nt(bf16): lda/ldw must be multiples of 8 elements'
NLDC = 'tcow_gemm_nt(bf16): N and ldc must be multiples of 4'
LDRAUX = 'tcow_gemm_nt(bf16): ldr / ldaux must be multiples of 4'
LAUNCHER = [
    (dict(K=96, lda=96, ldw=96), 'tcow_gemm_nt(bf16): K=96 must be a multiple of 64'),
    (dict(K=32, lda=32, ldw=32), 'tcow_gemm_nt(bf16): K=32 must be a multiple of 64'),
    (dict(K=136, lda=136, ldw=136), 'tcow_gemm_nt(bf16): K=136 must be a multiple of 64'),
    (dict(lda=K + 4), LDAB),
    (dict(lda=K + 1), LDAB),
    (dict(ldw=K + 4), LDAB),
    (dict(ldw=K + 7), LDAB),
    (dict(ldc=N + 2), NLDC),
    (dict(ldc=N + 1), NLDC),
    (dict(N=262, ldc=264), NLDC),
    (dict(N=263, ldc=264), NLDC),
    (dict(resid=PTR, ldr=N + 2, out_f32=1), LDRAUX),
    (dict(resid=PTR, ldr=N + 1, out_f32=1), LDRAUX),
    (dict(aux=PTR, ldaux=N + 2, act=1), LDRAUX),                               # ACT_GELU writes aux
    (dict(aux=PTR, ldaux=N + 3, act=4), LDRAUX),                               # ACT_MUL_AUX reads it
    (dict(aux=PTR, ldaux=N + 2), LDRAUX),                                      # an aux that the activation ignores is still checked
    (dict(tile=1), 'tcow_gemm_nt(bf16): tile must be 0, 128, 160, 256 or 320 (got 1)'),
    (dict(tile=64), 'tcow_gemm_nt(bf16): tile must be 0, 128, 160, 256 or 320 (got 64)'),
    (dict(tile=192), 'tcow_gemm_nt(bf16): tile must be 0, 128, 160, 256 or 320 (got 192)'),
    (dict(tile=-128), 'tcow_gemm_nt(bf16): tile must be 0, 128, 160, 256 or 320 (got -128)'),
    (dict(tile=160, K=64, lda=64, ldw=64), C2),
    (dict(tile=160, K=192, lda=192, ldw=192), C2),
    (dict(tile=160, M=1 << 20, lda=1024), C2),                                # M * lda = 2^30 exactly
    (dict(tile=160, M=(1 << 20) - 1, lda=1032), C2),                          # above it (1 082 129 400)
    (dict(tile=160, N=1 << 20, ldc=1 << 20, ldw=1024), C2),                   # N * ldw = 2^30 exactly
    # ORDER: K, then lda / ldw, then N / ldc, then ldr / ldaux, then the tile's value, then what tile 160 asks
    (dict(K=96, lda=100), 'tcow_gemm_nt(bf16): K=96 must be a multiple of 64'),
    (dict(lda=K + 4, ldc=N + 2), LDAB),
    (dict(ldc=N + 2, resid=PTR, ldr=N + 2), NLDC),
    (dict(resid=PTR, ldr=N + 2, tile=7), LDRAUX),
    (dict(tile=7, K=64, lda=64, ldw=64), 'tcow_gemm_nt(bf16): tile must be 0, 128, 160, 256 or 320 (got 7)'),
    (dict(tile=160, K=96, lda=96, ldw=96), 'tcow_gemm_nt(bf16): K=96 must be a multiple of 64'),
    (dict(tile=160, K=64, lda=68, ldw=64), LDAB),
]


@pytest.mark.parametrize('fmt', BUILDS)
def test_16bit_launcher_refusals(fmt):
    from tcow_amd import _lib
    lib = _lib.lib(fmt)
    for kw, message in LAUNCHER:
        assert refused(lib, gemm_args(_lib, _lib.TCOW_BF16, **kw)) == (-1, message), kw


@pytest.mark.parametrize('fmt', BUILDS)
def test_pitch_of_an_absent_tensor_is_not_looked_at(fmt):
    """resid = NULL / aux = NULL: ldr / ldaux are not looked at (callers pass 0 or anything); the call is then refused by the NEXT check that
    fails, here the tile's value, so these cases do not reach a launch either."""
    from tcow_amd import _lib
    lib = _lib.lib(fmt)
    tile = 'tcow_gemm_nt(bf16): tile must be 0, 128, 160, 256 or 320 (got 7)'
    for kw in (dict(resid=None, ldr=3), dict(aux=None, ldaux=5), dict(resid=None, ldr=1, aux=None, ldaux=2),
               dict(resid=PTR, ldr=N + 4, out_f32=1, aux=None, ldaux=3), dict(aux=PTR, ldaux=N + 4, resid=None, ldr=3)):
        assert refused(lib, gemm_args(_lib, _lib.TCOW_BF16, tile=7, **kw)) == (-1, tile), kw

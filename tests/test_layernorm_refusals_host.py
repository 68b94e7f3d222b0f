"""CPU: the row-stride checks of tcow_layernorm_bwd (csrc/layernorm.hip), against both builds of the library.

The backward reads dy, x and dres and writes dx and dx_cast four elements at a time (16-byte f32, 8-byte 16-bit accesses), so every row stride has to
be a multiple of 4 like the forward's.  Each case breaks exactly one stride of an otherwise valid call and expects TCOW_ERR_INVALID_ARG (-1) with the
check's own message.  No case reaches a launch (the pointers are never dereferenced), so no GPU is needed."""
import pytest

BUILDS = ('bf16', 'fp16')
PTR = 4096                        # any non-null, 16-byte-aligned address: a refused call does not touch it
ROWS, D = 8, 64


def bwd_args(dtype, lddy=D, ldx=D, dres=PTR, lddres=D, lddx=D, dx_cast=None, lddx_cast=0):
    """tcow_layernorm_bwd(stream, dtype, rows, D, dy, lddy, x, ldx, mean, rstd, gamma, dres, lddres, dx, lddx, dgamma, dbeta, accumulate, workspace,
    workspace_bytes, dx_cast, lddx_cast, cast_row_scale, colsum_row_scale, colsum_out) without parameter gradients."""
    return [None, dtype, ROWS, D, PTR, lddy, PTR, ldx, PTR, PTR, PTR, dres, lddres, PTR, lddx, None, None, 0, None, 0, dx_cast, lddx_cast, None, None, None]


CASES = [
    (dict(lddy=D + 2), 'tcow_layernorm_bwd: dy stride 66 must be a multiple of 4'),
    (dict(lddy=D + 1), 'tcow_layernorm_bwd: dy stride 65 must be a multiple of 4'),
    (dict(ldx=D + 3), 'tcow_layernorm_bwd: x stride 67 must be a multiple of 4'),
    (dict(lddres=D + 6), 'tcow_layernorm_bwd: dres stride 70 must be a multiple of 4'),
    (dict(lddx=D + 5), 'tcow_layernorm_bwd: dx stride 69 must be a multiple of 4'),
    (dict(dx_cast=PTR, lddx_cast=D + 2), 'tcow_layernorm_bwd: dx_cast stride must be a multiple of 4'),
    # the first broken stride in argument order is the one reported
    (dict(ldx=D + 1, lddx=D + 1), 'tcow_layernorm_bwd: x stride 65 must be a multiple of 4'),
]


@pytest.mark.parametrize('fmt', BUILDS)
def test_layernorm_bwd_refuses_strides_off_the_vector_width(fmt):
    from tcow_amd import _lib
    lib = _lib.lib(fmt)
    for dtype in (_lib.TCOW_F32, _lib.TCOW_BF16):
        for kw, message in CASES:
            status = lib.tcow_layernorm_bwd(*bwd_args(dtype, **kw))
            assert (status, lib.tcow_last_error().decode()) == (-1, message), kw


@pytest.mark.parametrize('fmt', BUILDS)
def test_layernorm_bwd_ignores_the_stride_of_an_absent_dres(fmt):
    """dres = NULL: its stride is not looked at (callers pass 0 or anything); the call is then refused by the NEXT check that fails, here the
    dx stride, so this case does not reach a launch either."""
    from tcow_amd import _lib
    lib = _lib.lib(fmt)
    status = lib.tcow_layernorm_bwd(*bwd_args(_lib.TCOW_F32, dres=None, lddres=3, lddx=D + 2))
    assert (status, lib.tcow_last_error().decode()) == (-1, 'tcow_layernorm_bwd: dx stride 66 must be a multiple of 4')

"""GPU: tcow_col2im / tcow_col2im_channels (csrc/tokens.hip) alone, exact.

The kernel is a permutation with a scale, so a matrix of distinct integers below 2^24 must come back bit for bit at the pixel the formula of
include/tcow_hip.h names: dst[b, c, t, hp P + py, wp P + px] = dA[(b T + t) S + 1 + hp Wp + wp, c P^2 + py P + px].  The slot-0 rows and the padding
columns of dA hold NaN (never read), the outputs sit in the middle of NaN-filled buffers (every element written, nothing outside), and the adjoint
identity <im2col(x), y> = <x, col2im(y)> ties the kernel to the forward's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GEOMETRIES = [(1, 1, 1, 1, 4), (2, 3, 2, 3, 16), (1, 2, 1, 5, 8), (3, 1, 4, 1, 16)]      # (B, T, Hp, Wp, P)
MARGIN = 64                                                                              # floats on either side of an output (keeps its 16-byte alignment)


@pytest.fixture(scope='module')
def ops(cuda):
    from tcow_amd import ops
    return ops


def matrix(B, T, Hp, Wp, P, C, pad, dev):
    """-> (dA [B T S, C P^2 + pad] on the device, the same on the CPU).  Distinct integers below 2^24 in the patch rows' first C P^2 columns, NaN
    in the slot-0 rows and the padding columns."""
    S, K = Hp * Wp + 1, C * P * P
    rows = B * T * S
    assert rows * K < 2 ** 24
    vals = torch.from_numpy(np.random.default_rng(rows * 31 + K).permutation(rows * K).astype(np.float32) + 1.0).reshape(rows, K)
    dA = torch.full((rows, K + pad), float('nan'))
    dA[:, :K] = vals
    dA.view(B * T, S, K + pad)[:, 0] = float('nan')
    return dA.to(dev), dA


def images(dA, B, T, Hp, Wp, P, C):
    """The CPU restatement: (B, C, T, H, W) by indexing dA with the header's formula."""
    S = Hp * Wp + 1
    a = dA[:, :C * P * P].reshape(B, T, S, C, P, P)[:, :, 1:].reshape(B, T, Hp, Wp, C, P, P)
    return a.permute(0, 4, 1, 2, 5, 3, 6).reshape(B, C, T, Hp * P, Wp * P).contiguous()


def framed(shape, dev):
    """-> (the whole NaN-filled buffer, its middle as a contiguous tensor of `shape`)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * MARGIN,), float('nan'), device=dev)
    return whole, whole[MARGIN:MARGIN + n].view(shape)


def margins_untouched(whole):
    return bool(torch.isnan(whole[:MARGIN]).all()) and bool(torch.isnan(whole[-MARGIN:]).all())


def check_norm(got, ref):
    """1 / 0.225 as an f32 division: within 1 ulp of ref / float32(0.225) (relative 2^-23)."""
    want = ref.double() / float(np.float32(0.225))
    assert bool(((got.double() - want).abs() <= 2.0 ** -23 * want.abs()).all())


@pytest.mark.parametrize('pad', [0, 8])
@pytest.mark.parametrize('geom', GEOMETRIES)
def test_col2im_is_the_index_map(ops, cuda, geom, pad):
    B, T, Hp, Wp, P = geom
    H, W = Hp * P, Wp * P
    dA, dA_cpu = matrix(B, T, Hp, Wp, P, 4, pad, cuda)
    ref = images(dA_cpu, B, T, Hp, Wp, P, 4)
    inv = torch.tensor(2.0 ** -7, device=cuda)
    for norm in (0, 1):
        for scale, k in ((None, 1.0), (inv, 2.0 ** -7)):
            wr, d_rgb = framed((B, 3, T, H, W), cuda); wq, d_qm = framed((B, 1, T, H, W), cuda)
            ops.col2im(dA, B, T, H, W, P, norm, d_rgb, d_qm, inv_scale=scale)
            assert bool(torch.isfinite(d_rgb).all()) and bool(torch.isfinite(d_qm).all())          # every element written, no slot-0 row or padding read
            assert margins_untouched(wr) and margins_untouched(wq)                                # nothing outside
            assert torch.equal(d_qm.cpu(), ref[:, 3:] * k)                                        # the query channel is never normalised
            if norm:
                check_norm(d_rgb.cpu(), ref[:, :3] * k)
            else:
                assert torch.equal(d_rgb.cpu(), ref[:, :3] * k)
    # one output not wanted: its buffer keeps the sentinel, the other is as before
    wr, d_rgb = framed((B, 3, T, H, W), cuda); wq, d_qm = framed((B, 1, T, H, W), cuda)
    ops.col2im(dA, B, T, H, W, P, 0, None, d_qm)
    assert bool(torch.isnan(wr).all()) and margins_untouched(wq) and torch.equal(d_qm.cpu(), ref[:, 3:])
    wr, d_rgb = framed((B, 3, T, H, W), cuda); wq, d_qm = framed((B, 1, T, H, W), cuda)
    ops.col2im(dA, B, T, H, W, P, 0, d_rgb, None)
    assert bool(torch.isnan(wq).all()) and margins_untouched(wr) and torch.equal(d_rgb.cpu(), ref[:, :3])


def test_col2im_skips_the_columns_of_an_unwanted_output(ops, cuda):
    """A null output's columns of dA are not read: the engine leaves them unwritten."""
    B, T, Hp, Wp, P = 2, 3, 2, 3, 16
    dA, dA_cpu = matrix(B, T, Hp, Wp, P, 4, 0, cuda)
    ref = images(dA_cpu, B, T, Hp, Wp, P, 4)
    only_q = dA.clone(); only_q[:, :3 * P * P] = float('nan')
    _, d_qm = framed((B, 1, T, Hp * P, Wp * P), cuda)
    ops.col2im(only_q, B, T, Hp * P, Wp * P, P, 1, None, d_qm)
    assert torch.equal(d_qm.cpu(), ref[:, 3:])
    only_rgb = dA.clone(); only_rgb[:, 3 * P * P:] = float('nan')
    _, d_rgb = framed((B, 3, T, Hp * P, Wp * P), cuda)
    ops.col2im(only_rgb, B, T, Hp * P, Wp * P, P, 0, d_rgb, None)
    assert torch.equal(d_rgb.cpu(), ref[:, :3])


@pytest.mark.parametrize('C', [3, 1])
@pytest.mark.parametrize('pad', [0, 8])
@pytest.mark.parametrize('geom', GEOMETRIES)
def test_col2im_channels_is_the_index_map(ops, cuda, geom, pad, C):
    B, T, Hp, Wp, P = geom
    dA, dA_cpu = matrix(B, T, Hp, Wp, P, C, pad, cuda)
    ref = images(dA_cpu, B, T, Hp, Wp, P, C)
    inv = torch.tensor(2.0 ** -7, device=cuda)
    for norm in (0, 1):
        for scale, k in ((None, 1.0), (inv, 2.0 ** -7)):
            whole, dst = framed((B, C, T, Hp * P, Wp * P), cuda)
            ops.col2im_channels(dA, P, norm, dst, inv_scale=scale)
            assert bool(torch.isfinite(dst).all()) and margins_untouched(whole)
            if norm:
                check_norm(dst.cpu(), ref * k)
            else:
                assert torch.equal(dst.cpu(), ref * k)


def test_col2im_second_trip_of_the_grid_stride_loop(ops, cuda):
    """P = 4, T = 2, 728 x 728: 2 * 182 * 182 patch rows x 16 float4 = 1 059 968 = 1 048 576 (4096 workgroups of 256) + 11 392, so 11 392 threads take a second
    trip and the rest do not."""
    B, T, Hp, Wp, P = 1, 2, 182, 182, 4
    S = Hp * Wp + 1
    dA_cpu = torch.arange(B * T * S * 64, dtype=torch.float32).reshape(B * T * S, 64)           # (below 2^24: 66 250 * 64 = 4 240 000)
    ref = images(dA_cpu, B, T, Hp, Wp, P, 4)
    wr, d_rgb = framed((B, 3, T, Hp * P, Wp * P), cuda); wq, d_qm = framed((B, 1, T, Hp * P, Wp * P), cuda)
    ops.col2im(dA_cpu.to(cuda), B, T, Hp * P, Wp * P, P, 0, d_rgb, d_qm)
    assert margins_untouched(wr) and margins_untouched(wq)
    assert torch.equal(d_rgb.cpu(), ref[:, :3]) and torch.equal(d_qm.cpu(), ref[:, 3:])


@pytest.mark.parametrize('geom', GEOMETRIES)
def test_adjoint_identity_with_im2col(ops, cuda, geom):
    """<im2col(x), y> = <x, col2im(y)> in the f32 storage mode without normalisation.  Both kernels only move values, so the two sides sum the same
    n products of f32 pairs (exact in f64) in different orders: they agree to n * 2^-24 * sum |terms|, computed here."""
    B, T, Hp, Wp, P = geom
    H, W, S = Hp * P, Wp * P, Hp * Wp + 1
    gen = torch.Generator().manual_seed(B * 1000 + T * 100 + Hp * 10 + Wp)
    rgb = torch.randn(B, 3, T, H, W, generator=gen).to(cuda); qm = torch.randn(B, 1, T, H, W, generator=gen).to(cuda)
    y = torch.randn(B * T * S, 4 * P * P, generator=gen).to(cuda)
    A = torch.empty(B * T * S, 4 * P * P, device=cuda)
    ops.im2col(ops.F32, rgb, qm, P, False, A)
    d_rgb = torch.empty_like(rgb); d_qm = torch.empty_like(qm)
    ops.col2im(y, B, T, H, W, P, 0, d_rgb, d_qm)
    left = A.double() * y.double()
    right = torch.cat([rgb.double() * d_rgb.double(), qm.double() * d_qm.double()], 1)
    n = right.numel()
    bound = n * 2.0 ** -24 * float(right.abs().sum())
    assert abs(float(left.sum()) - float(right.sum())) <= bound
    assert float(left.abs().sum()) > 0 and abs(float(left.abs().sum()) - float(right.abs().sum())) <= bound     # the same terms on both sides

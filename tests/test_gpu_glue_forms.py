"""GPU: the glue kernels of csrc/tokens.hip, casts.hip and mask_head.hip at the shapes where their other code runs: the second trip of every grid-stride
loop (gs_blocks() caps a launch at 4096 workgroups x 256 threads = 1 048 576 work items; every shape below is just above that with a ragged last trip:
the remainder is neither 0 nor a multiple of 256), the kernels behind the dispatch conditions test_gpu_kernels.py never meets (generic un-patchify,
16-bit backward, scalar-store upsample, both sides of the upsample backward's fast-path gate), second and ragged rounds of the eight-frame loops,
channel blocks that are not full, idle threads and second trips of the flags head.

Every case compares with a float64 torch restatement of the operation under the bound test_gpu_kernels.py uses for the same quantity; copies, casts and
index maps are compared bit for bit.  Dense outputs are views of NaN-filled buffers with spare elements behind them, strided ones have pad columns and
a spare row (kernel_forms.py): they must keep the sentinel, and every element inside must be finite."""
import pytest
import torch
import torch.nn.functional as F

from kernel_forms import NAN, assert_guarded, assert_guarded_flat, assert_untouched, bits, guarded, guarded_flat
from test_gpu_kernels import MODES, _mode, rel

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CAP = 4096 * 256
STORAGES = [m for m, _ in MODES]
# one rounding to the storage type on top of an f32 result: half an ulp = 2^-24 / 2^-9 / 2^-12 of the element; bound = twice that (f32: the 1e-5 of today)
ROUND = {'f32': 1e-5, 'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11}


@pytest.fixture(scope='module')
def ops(cuda):
    from tcow_amd import ops as o
    return o


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, device=DEV, generator=g) * 2 + 0.5


def second_trip(total):
    """total work items force a second grid-stride trip whose last workgroup is partly idle."""
    return total > CAP and total % CAP != 0 and total % 256 != 0


def out_flat(shape, dt):
    n = 1
    for s in shape:
        n *= s
    buf, v = guarded_flat(n, dt, DEV)
    return buf, v.view(*shape), n


# ------------------------------------------------------------------------------------------------ references
def patches(x, P):
    """(B, C, T, H, W) -> (B, T, N, C P P): the Conv2d flattening of im2col (test_gpu_kernels.py)."""
    B, C, T, H, W = x.shape
    return x.reshape(B, C, T, H // P, P, W // P, P).permute(0, 2, 3, 5, 1, 4, 6).reshape(B, T, (H // P) * (W // P), -1)


def unpatch(pm, BT, Hp, Wp, P, C):
    """[BT S, C P P] token rows -> (BT, C, Hp P, Wp P) image (slot 0 dropped)."""
    return pm.reshape(BT, Hp * Wp + 1, C, P, P)[:, 1:].reshape(BT, Hp, Wp, C, P, P).permute(0, 3, 1, 4, 2, 5).reshape(BT, C, Hp * P, Wp * P)


def repatch(img, BT, Hp, Wp, P, C):
    """(BT, C, Hp P, Wp P) -> [BT, S, C P P] with a zero slot 0: the adjoint of unpatch."""
    body = img.reshape(BT, C, Hp, P, Wp, P).permute(0, 2, 4, 1, 3, 5).reshape(BT, Hp * Wp, C * P * P)
    return torch.cat([torch.zeros_like(body[:, :1]), body], 1)


def pool_ref(pm, BT, Hp, Wp, P, C, st):
    img = unpatch(pm.double(), BT, Hp, Wp, P, C)
    return F.avg_pool2d(img, st, st) if st > 1 else img


def pool_bwd_ref(dpooled, BT, Hp, Wp, P, C, st):
    d = dpooled.double()
    if st > 1:
        d = d.repeat_interleave(st, 2).repeat_interleave(st, 3) / (st * st)
    return repatch(d, BT, Hp, Wp, P, C)


def up_ref(p, st, bilinear):
    """(BT, C, h, w) float64 -> (BT, C, h st, w st): mask_tracker.py:124-130 (nearest at an integer scale factor repeats every pixel st x st times)."""
    if st == 1:
        return p
    return F.interpolate(p, scale_factor=st, mode='bilinear', align_corners=True) if bilinear else p.repeat_interleave(st, 2).repeat_interleave(st, 3)


def up_bwd_ref(dout, B, T, C, h, w, st, bilinear):
    """autograd of up_ref for dout (B, C, T, H, W) -> (BT, C, h, w) float64."""
    p = torch.zeros(B * T, C, h, w, device=dout.device, dtype=torch.float64, requires_grad=True)
    up = up_ref(p, st, bilinear)
    return torch.autograd.grad((up * dout.double().permute(0, 2, 1, 3, 4).reshape_as(up)).sum(), p)[0]


# ------------------------------------------------------------------------------------------------ casts.hip
@pytest.mark.parametrize('mname', STORAGES)
def test_scale_cast_second_trip_and_strides(ops, cuda, mname):
    """4100 x 1028: 4100 * 257 = 1 053 700 float4 items = 1 048 576 + 5124, 5124 = 20 * 256 + 4.  Dense and strided source / destination (pitch D + 4 and
    D + 8), with and without row_scale: dtype(src * scale) bit for bit (torch rounds to nearest even as well)."""
    mode, dt = _mode(ops, mname)
    g = gen(1)
    for rows, D in ((4100, 1028), (5, 12)):
        if rows > 5:
            assert second_trip(rows * D // 4)
        rs = torch.rand(rows, device=cuda, generator=g) + 0.5
        sbuf, src = guarded(rows, D, D + 4, torch.float32, cuda)
        src.copy_(randn(g, rows, D))
        before = sbuf.clone()
        for scale in (rs, None):
            want = (src * scale[:, None] if scale is not None else src).to(dt)
            for s in (src, src.contiguous()):
                dbuf, dst = guarded(rows, D, D + 8, dt, cuda)
                ops.scale_cast(mode, s, scale, dst)
                assert_guarded(dbuf, rows, D, 'dst'); assert torch.equal(dst, want)
                fbuf, dense, _ = out_flat((rows, D), dt)
                ops.scale_cast(mode, s, scale, dense)
                assert_guarded_flat(fbuf, rows * D, 'dense dst'); assert torch.equal(dense, want)
        assert torch.equal(bits(sbuf), bits(before))


@pytest.mark.parametrize('mname', STORAGES)
@pytest.mark.parametrize('N,K', [(n, k) for n in (1, 31, 33) for k in (1, 31, 33)])
def test_cast_transpose_one_output(ops, cuda, mname, N, K):
    """Wc only, Wt only and both, in every storage (f32 included), edges below, at and one past the 32 x 32 tile.  Wc and Wt lie back to back in one
    NaN buffer, so the absent output is where an overrun of the present one would land: it keeps its sentinel."""
    mode, dt = _mode(ops, mname)
    W = randn(gen(N * 64 + K), N, K)
    for want_c, want_t in ((True, False), (False, True), (True, True)):
        buf, v = guarded_flat(2 * N * K, dt, cuda)
        Wc, Wt = v[:N * K].view(N, K), v[N * K:].view(K, N)
        ops.cast_transpose(mode, W, Wc if want_c else None, Wt if want_t else None)
        if want_c:
            assert torch.equal(Wc, W.to(dt))
        else:
            assert_untouched(buf[:N * K], 'Wc')
        if want_t:
            assert torch.equal(Wt, W.t().contiguous().to(dt))
        else:
            assert_untouched(buf[N * K:], 'Wt')
        assert_untouched(buf[2 * N * K:], 'behind Wt')


def test_scale_unless_one_second_trip(ops, cuda):
    """n = 4 * 1 048 576 + 4099: 1 049 600 float4 items + 3 tail elements (second trip of 1024 items); n = 4 * 1 048 576 + 4403: 1 049 676 items + 3
    (second trip of 1100 = 4 * 256 + 76).  x * s bit for bit, s == 1 touches nothing, nothing behind x[n - 1] changes."""
    g = gen(2)
    for n in (4 * 1048576 + 4099, 4 * 1048576 + 4403):
        assert n // 4 > CAP and n % 4 == 3
        buf, x = guarded_flat(n, torch.float32, cuda)
        x.copy_(randn(g, n)); ref = x.clone()
        ops.scale_unless_one(x, torch.ones((), device=cuda))
        assert torch.equal(x, ref)
        s = torch.full((), 0.37, device=cuda)
        ops.scale_unless_one(x, s)
        assert_guarded_flat(buf, n, 'x'); assert torch.equal(x, ref * s)
    assert second_trip((4 * 1048576 + 4403) // 4)


def test_droppath_rows_second_trip(ops, cuda):
    """depth 2 x (B 3, T 5, S 34967): 2 * 524 505 = 1 049 010 rows = 1 048 576 + 434.  Bit for bit against the broadcast expressions of
    test_droppath_rows_kernel (floor(u + keep_p) / keep_p in f32, as vit_utils.py:139-154 computes it)."""
    depth, B, T, S = 2, 3, 5, 34967
    N, M = S - 1, B * T * S
    assert second_trip(depth * M)
    g = gen(3)
    keep_p = torch.tensor([0.9, 0.7], device=cuda)
    u = torch.rand(depth, B * N + B * T + B, device=cuda, generator=g)
    mask0 = (torch.rand(M, device=cuda, generator=g) > 0.2).float()
    sc = (u + keep_p[:, None]).floor() / keep_p[:, None]
    kt = sc[:, :B * N].reshape(depth, B, 1, N); ks = sc[:, B * N:B * N + B * T].reshape(depth, B, T, 1); km = sc[:, B * N + B * T:].reshape(depth, B, 1)
    rt = torch.ones(depth, B, T, S, device=cuda); rt[:, :, :, 1:] = kt; rt = rt.reshape(depth, -1)
    want = torch.stack([rt, ks.expand(depth, B, T, S).reshape(depth, -1), km.expand(depth, B, T * S).reshape(depth, -1), rt * mask0[None]])
    got = ops.droppath_rows(u, keep_p, mask0, B, T, S)
    assert torch.equal(got, want) and 0 < int((got == 0).sum()) < got.numel()


# ------------------------------------------------------------------------------------------------ tokens.hip
def check_im2col(ops, mname, src, P, norm, channels):
    """im2col (3 rgb + 1 query channel) or im2col_channels (C channels, all normalised) against the reshape / permute reference: slot 0 of every frame is
    zero; without normalisation the rest is a copy + cast (bit for bit), with it float64 under today's bounds (1e-6 in f32, 8e-3 in 16 bits)."""
    mode, dt = _mode(ops, mname)
    B, C, T, H, W = src.shape
    S = (H // P) * (W // P) + 1
    buf, out, n = out_flat((B * T * S, C * P * P), dt)
    if channels:
        ops.im2col_channels(mode, src, P, norm, out)
        ref = (src.double() - 0.45) / 0.225 if norm else src
    else:
        rgb, qm = src[:, :3].contiguous(), src[:, 3:].contiguous()
        ops.im2col(mode, rgb, qm, P, norm, out)
        ref = torch.cat([(rgb.double() - 0.45) / 0.225, qm.double()], 1) if norm else src
    assert_guarded_flat(buf, n, 'out')
    got = out.reshape(B, T, S, -1)
    assert not bool(got[:, :, 0].any()), 'slot 0 is not zero'
    if norm:
        assert rel(got[:, :, 1:], patches(ref, P)) < (1e-6 if mname == 'f32' else 8e-3)
    else:
        assert torch.equal(got[:, :, 1:], patches(ref, P).to(dt))


@pytest.mark.parametrize('mname', STORAGES)
def test_im2col_second_trip(ops, cuda, mname):
    """im2col at P = 4, T = 2, 728 x 728: 2 * (182 * 182 + 1) = 66 250 rows x 16 float4 = 1 060 000 = 1 048 576 + 11 424 (44 * 256 + 160);
    im2col_channels at C = 5, P = 4, T = 2, 652 x 652: 2 * (163 * 163 + 1) = 53 140 rows x 20 = 1 062 800 = 1 048 576 + 14 224 (55 * 256 + 144)."""
    assert second_trip(2 * (182 * 182 + 1) * 16) and second_trip(2 * (163 * 163 + 1) * 20)
    g = gen(4)
    src = torch.rand(1, 4, 2, 728, 728, device=cuda, generator=g)
    check_im2col(ops, mname, src, 4, False, False); check_im2col(ops, mname, src, 4, True, False)
    src = torch.rand(1, 5, 2, 652, 652, device=cuda, generator=g)
    check_im2col(ops, mname, src, 4, False, True); check_im2col(ops, mname, src, 4, True, True)


@pytest.mark.parametrize('mname', STORAGES)
@pytest.mark.parametrize('P', [4, 8, 16])
@pytest.mark.parametrize('C', [1, 3, 5])
def test_im2col_channels(ops, cuda, mname, P, C):
    """The entry point the engine calls, with and without normalisation: B = 2, T = 3, 2 x 3 patches."""
    src = torch.rand(2, C, 3, 2 * P, 3 * P, device=cuda, generator=gen(P * 8 + C))
    for norm in (False, True):
        check_im2col(ops, mname, src, P, norm, True)


def test_embed_fwd_second_trip(ops, cuda):
    """D = 12, B = 2, T = 3, S = 58 259: 349 554 rows x 3 float4 = 1 048 662 = 1 048 576 + 86."""
    B, T, S, D = 2, 3, 58259, 12
    assert second_trip(B * T * S * D // 4)
    g = gen(5)
    buf, tok, n = out_flat((B * T * S, D), torch.float32)
    tok.copy_(randn(g, B * T * S, D))
    cls, pos, te = randn(g, D), randn(g, S, D), randn(g, T, D)
    want = tok.double().reshape(B, T, S, D) + pos.double()[None, None] + te.double()[None, :, None]
    want[:, :, 0] = cls.double() + pos.double()[0]
    ops.embed_fwd(tok, B, T, S, cls, pos, te)
    assert_guarded_flat(buf, n, 'x'); assert rel(tok.reshape(B, T, S, D), want) < 1e-6


@pytest.mark.parametrize('D', [8, 72, 264])
@pytest.mark.parametrize('S', [2, 17, 18, 40])
def test_embed_bwd_rounds_and_blocks(ops, cuda, S, D):
    """embed_bwd_time strides the S - 1 patch slots by 16 thread rows (S = 2: one slot; 17: exactly 16; 18: one thread row makes a second trip; 40) over
    16-quad channel blocks (D = 8: 2 of 16 quads; 72: a full block + 2; 264: 66 quads = the position kernel's 64-quad block + 2); embed_bwd_pos splits
    the B T frames over four thread rows in rounds of 24 (B T = 1, 3: idle rows; 23, 24: the tail loop only; 25: one full round, three rows idle in it
    ... ; 50).  dpos, dtime against float64 sums under today's 1e-5, plain and accumulating into random tables; pad elements keep their sentinel."""
    g = gen(S * 512 + D)
    for B, T in ((1, 1), (1, 3), (1, 23), (2, 12), (5, 5), (2, 25)):
        grad = randn(g, B * T * S, D)
        g4 = grad.double().reshape(B, T, S, D)
        want_pos, want_time = g4.sum((0, 1)), g4[:, :, 1:].sum((0, 2))
        for acc in (False, True):
            pbuf, dpos, npos = out_flat((S, D), torch.float32); tbuf, dtime, ntime = out_flat((T, D), torch.float32)
            p0, t0 = randn(g, S, D), randn(g, T, D)
            if acc:
                dpos.copy_(p0); dtime.copy_(t0)
            ops.embed_bwd(grad, B, T, S, dpos, dtime, accumulate=acc)
            assert_guarded_flat(pbuf, npos, 'dpos'); assert_guarded_flat(tbuf, ntime, 'dtime')
            e = rel(dpos, want_pos + p0.double() if acc else want_pos), rel(dtime, want_time + t0.double() if acc else want_time)
            assert e[0] < 1e-5 and e[1] < 1e-5, f'B={B} T={T} acc={acc}: dpos {e[0]:.3e} dtime {e[1]:.3e}'


@pytest.mark.parametrize('T', [1, 8, 9, 13, 17])
def test_cls_merge_rounds(ops, cuda, T):
    """sum_frames and the cast refresh work in rounds of eight frames: T = 1 (a ragged only round), 8 (one exact), 9, 13 (a ragged second), 17 (a third).
    B = 3, D = 200: 150 threads = two full waves + 22 lanes.  Both modes, forward and adjoint against float64 (1e-6, as today); rows of the other slots keep
    their bits.  bwd_cast in the three storages, with and without cast_scale, into a cast_out of pitch D + 4: slot-0 rows = dtype(x * scale) bit for bit,
    every other row and the pads keep the sentinel."""
    B, S, D = 3, 3, 200
    R = B * T * S
    g = gen(T)
    x = randn(g, R, D); gy = randn(g, R, D); sc = torch.rand(R, device=cuda, generator=g) + 0.5
    slot0 = torch.arange(0, R, S, device=cuda)
    for mode in (1, 0):
        buf, y, n = out_flat((R, D), torch.float32)
        y.copy_(x); ops.cls_merge(y, B, T, S, mode)
        assert_guarded_flat(buf, n, 'x')
        x4, y4 = x.double().reshape(B, T, S, D), y.reshape(B, T, S, D)
        want = x4[:, 0:1, 0] if mode == 1 else x4[:, :, 0].mean(1, keepdim=True)
        assert rel(y4[:, :, 0], want.expand(B, T, D)) < 1e-6 and torch.equal(y4[:, :, 1:], x.reshape(B, T, S, D)[:, :, 1:])
        buf, gx, n = out_flat((R, D), torch.float32)
        gx.copy_(gy); ops.cls_merge(gx, B, T, S, mode, backward=True)
        assert_guarded_flat(buf, n, 'x (adjoint)')
        g4, gx4 = gy.double().reshape(B, T, S, D), gx.reshape(B, T, S, D)
        tot = g4[:, :, 0].sum(1, keepdim=True)
        want = torch.cat([tot, torch.zeros(B, T - 1, D, device=cuda, dtype=torch.float64)], 1) if mode == 1 else (tot / T).expand(B, T, D)
        assert rel(gx4[:, :, 0], want) < 1e-6 and torch.equal(gx4[:, :, 1:], gy.reshape(B, T, S, D)[:, :, 1:])
        if mode == 1 and T > 1:
            assert not bool(gx4[:, 1:, 0].any())
        for mname in STORAGES:
            cmode, dt = _mode(ops, mname)
            for scale in (sc, None):
                g2 = gy.clone()
                cbuf, cast = guarded(R, D, D + 4, dt, cuda)
                ops.cls_merge(g2, B, T, S, mode, backward=True, cast_mode=cmode, cast_out=cast, cast_scale=scale)
                assert torch.equal(g2, gx)
                want_buf = torch.full_like(cbuf, NAN)
                want_buf[slot0, :D] = (gx[slot0] * scale[slot0, None] if scale is not None else gx[slot0]).to(dt)
                assert torch.equal(bits(cbuf), bits(want_buf)), f'mode {mode} {mname} scale {scale is not None}'
                assert bool(torch.isfinite(cbuf[slot0, :D].float()).all())


# ------------------------------------------------------------------------------------------------ mask_head.hip
# (P, st) -> forward kernel, backward kernel (tcow_unpatchify_pool_fwd / _bwd): pool4 needs st == 4 and P % 8 == 0, bwd8 needs P % 8 == 0
POOL_FORMS = [(4, 1), (4, 4), (12, 4),          # generic, generic
              (8, 8), (16, 8), (16, 2), (16, 1),  # generic, bwd8
              (24, 3),                          # generic, bwd8 with a stride that does not divide 8
              (16, 4), (8, 4)]                  # pool4, bwd8


@pytest.mark.parametrize('mname', STORAGES)
@pytest.mark.parametrize('P,st', POOL_FORMS)
def test_unpatchify_pool_forms(ops, cuda, mname, P, st):
    """Forward (16-bit / f32 token rows -> f32 pooled, 1e-6 as today) and backward (f32 pooled gradient -> token rows in the storage type, slot 0 zero)
    against avg_pool2d and its adjoint in float64.  The backward's result is dpooled / st^2 rounded once to the storage type.  A token buffer that is
    not 16-byte aligned takes the generic backward even at P % 8 == 0: the same result."""
    mode, dt = _mode(ops, mname)
    BT, Hp, Wp, C = 2, 2, 3, 3
    S, K = Hp * Wp + 1, C * P * P
    g = gen(P * 16 + st)
    pm = randn(g, BT * S, K).to(dt)
    buf, pooled, n = out_flat((BT, C, Hp * P // st, Wp * P // st), torch.float32)
    ops.unpatchify_pool_fwd(mode, pm, BT, Hp, Wp, P, C, st, pooled)
    assert_guarded_flat(buf, n, 'pooled'); assert rel(pooled, pool_ref(pm, BT, Hp, Wp, P, C, st)) < 1e-6
    dpooled = randn(g, *pooled.shape)
    want = pool_bwd_ref(dpooled, BT, Hp, Wp, P, C, st)
    for offset in (0, 1):                                  # 1: dpm starts one element into the buffer (4 or 2 bytes off the 16-byte boundary)
        buf, v = guarded_flat(offset + BT * S * K, dt, cuda)
        dpm = v[offset:].view(BT * S, K)
        ops.unpatchify_pool_bwd(mode, dpooled, BT, Hp, Wp, P, C, st, dpm)
        assert_guarded_flat(buf[offset:], BT * S * K, 'dpm')
        if offset:
            assert_untouched(buf[:offset], 'in front of dpm')
        got = dpm.reshape(BT, S, K)
        assert not bool(got[:, 0].any()) and rel(got, want) < ROUND[mname]


@pytest.mark.parametrize('mname', STORAGES)
def test_unpatchify_pool_second_trip(ops, cuda, mname):
    """pool4 (st 4, P 16, C 1, BT 2, 259 x 254 patches): 131 572 tokens x 8 threads = 1 052 576 = 1 048 576 + 4000 (15 * 256 + 160) -- every thread reads 32
    elements, so the f32 token rows are 134 MB: the smallest tensor that reaches this trip;
    generic forward (st 1, P 4, C 3, BT 2, 105 x 105): 2 * 3 * 420 * 420 = 1 058 400 outputs = 1 048 576 + 9824 (38 * 256 + 96);
    bwd8 (P 8, C 1, st 2, BT 2, 256 x 257): 131 586 rows x 8 = 1 052 688 = 1 048 576 + 4112 (16 * 256 + 16);
    generic backward (P 4, C 1, st 2, BT 2, 182 x 181): 65 886 rows x 16 = 1 054 176 = 1 048 576 + 5600 (21 * 256 + 224)."""
    mode, dt = _mode(ops, mname)
    g = gen(6)
    for BT, Hp, Wp, P, C, st, items in ((2, 259, 254, 16, 1, 4, 2 * 259 * 254 * 8), (2, 105, 105, 4, 3, 1, 2 * 3 * 420 * 420)):
        assert second_trip(items)
        pm = torch.randn(BT * (Hp * Wp + 1), C * P * P, device=cuda, generator=g).to(dt)
        buf, pooled, n = out_flat((BT, C, Hp * P // st, Wp * P // st), torch.float32)
        ops.unpatchify_pool_fwd(mode, pm, BT, Hp, Wp, P, C, st, pooled)
        assert_guarded_flat(buf, n, 'pooled'); assert rel(pooled, pool_ref(pm, BT, Hp, Wp, P, C, st)) < 1e-6
        del pm
    for BT, Hp, Wp, P, C, st, items in ((2, 256, 257, 8, 1, 2, 2 * (256 * 257 + 1) * 8), (2, 182, 181, 4, 1, 2, 2 * (182 * 181 + 1) * 16)):
        assert second_trip(items)
        S, K = Hp * Wp + 1, C * P * P
        dpooled = randn(g, BT, C, Hp * P // st, Wp * P // st)
        buf, dpm, n = out_flat((BT * S, K), dt)
        ops.unpatchify_pool_bwd(mode, dpooled, BT, Hp, Wp, P, C, st, dpm)
        assert_guarded_flat(buf, n, 'dpm')
        got = dpm.reshape(BT, S, K)
        assert not bool(got[:, 0].any()) and rel(got, pool_bwd_ref(dpooled, BT, Hp, Wp, P, C, st)) < ROUND[mname]


def run_upsample_fwd(ops, g, B, T, C, h, w, st, bilinear, tol=1e-5):
    pooled = randn(g, B * T, C, h, w)
    buf, out, n = out_flat((B, C, T, h * st, w * st), torch.float32)
    ops.upsample_fwd(pooled, B, T, C, h, w, st, bilinear, out)
    assert_guarded_flat(buf, n, 'out')
    want = up_ref(pooled.double(), st, bilinear).reshape(B, T, C, h * st, w * st).permute(0, 2, 1, 3, 4)
    e = rel(out, want)
    assert e < tol, f'h={h} w={w} st={st} bilinear={bilinear}: {e:.3e}'


@pytest.mark.parametrize('bilinear', [True, False])
def test_upsample_fwd_forms(ops, cuda, bilinear):
    """W % 4 != 0 takes the scalar stores with a partly dead last quad (st 2, w 3: W = 6; st 1, w 5: W = 5; st 2, w 1: W = 2; st 3, w 3: W = 9); h = 1 and
    w = 1 give the bilinear source rule a zero scale; one frame with H * ceil(W / 4) > 64 * 256 = 16 384 makes the frame's 64 workgroups loop
    (st 2, 130 x 130: 260 * 65 = 16 900; 130 x 131: W = 262, 260 * 66 = 17 160 with scalar stores).
    Bound 1e-5 as today, except for the two 260-row frames: the bilinear source coordinate scale * x is an f32 product, good to ~x * 2^-24, and the same
    interpolation in plain float32 torch ops (F.interpolate on the f32 tensor) is 9.1e-6 and 1.08e-5 away from float64 at these two shapes with these
    inputs (5.5e-8 at 3 x 3); four times the larger = 4.4e-5 there.  Nearest is a copy: bit-exact in effect (error 0)."""
    g = gen(7)
    for h, w, st in ((3, 3, 2), (3, 5, 1), (4, 1, 2), (3, 3, 3), (1, 5, 4), (5, 1, 4), (1, 1, 4), (1, 7, 2), (7, 1, 1)):
        run_upsample_fwd(ops, g, 2, 3, 2, h, w, st, bilinear)
    for h, w in ((130, 130), (130, 131)):
        assert 2 * h * ((2 * w + 3) // 4) > 64 * 256 and (2 * h * ((2 * w + 3) // 4)) % 256 != 0
        run_upsample_fwd(ops, g, 1, 2, 1, h, w, 2, bilinear, tol=4.4e-5 if bilinear else 1e-5)


@pytest.mark.parametrize('h,w', [(5, 5), (4, 6), (6, 4), (1, 7), (7, 1), (12, 16)])
def test_upsample_bwd_gate_and_degenerate_axes(ops, cuda, h, w):
    """The stride-4 bilinear fast path runs for h > 4 and w > 4 only: (5, 5) is its smallest shape, (4, 6) and (6, 4) fall back to the generic gather on one
    side of the gate each, h = 1 / w = 1 have a zero source scale.  Bilinear at strides 4 and 2 and nearest at 3, against the autograd of F.interpolate in
    float64 (1e-5).  Where the fast path runs, also against the gradient written out from the reference's own interpolation matrices
    (dpooled = Uy^T dout Ux, U = F.interpolate of the identity), and the amax variant returns the same bits."""
    g = gen(h * 32 + w)
    B, T, C = 2, 2, 3
    for st, bilinear in ((4, True), (2, True), (3, False), (1, False)):
        dout = randn(g, B, C, T, h * st, w * st)
        buf, dp, n = out_flat((B * T, C, h, w), torch.float32)
        ops.upsample_bwd(dout, B, T, C, h, w, st, bilinear, dp)
        assert_guarded_flat(buf, n, 'dpooled')
        e = rel(dp, up_bwd_ref(dout, B, T, C, h, w, st, bilinear))
        assert e < 1e-5, f'st={st} bilinear={bilinear}: {e:.3e}'
        if st == 4 and h > 4 and w > 4:
            eye = lambda k: torch.eye(k, device=cuda, dtype=torch.float64)
            Uy = F.interpolate(eye(h)[None], scale_factor=4, mode='linear', align_corners=True)[0].t()        # [H, h]
            Ux = F.interpolate(eye(w)[None], scale_factor=4, mode='linear', align_corners=True)[0].t()        # [W, w]
            want = Uy.t() @ dout.double().permute(0, 2, 1, 3, 4).reshape(B * T, C, 4 * h, 4 * w) @ Ux
            assert rel(dp, want) < 1e-5
            dp2, amax = ops.upsample_bwd_amax(dout, B, T, C, h, w, 4, torch.empty_like(dp))
            assert torch.equal(dp2, dp) and float(amax) == float(dout.abs().max())


def test_upsample_bwd_amax_planted_maximum(ops, cuda):
    """max |dout| must see every pixel: an all-zero dout with one negative value planted at each corner, at one inner pixel of each edge, and at the last
    pixel of the last frame -- exact every time; all zeros give 0."""
    B, T, C, h, w = 1, 2, 2, 5, 6
    H, W = 4 * h, 4 * w
    spots = [(0, 0, 0, 0, 0), (0, 0, 0, 0, W - 1), (0, 0, 0, H - 1, 0), (0, 0, 0, H - 1, W - 1),                 # corners of the first frame
             (0, 1, 0, 0, 9), (0, 1, 0, H - 1, 13), (0, 0, 1, 7, 0), (0, 0, 1, 10, W - 1),                       # one pixel of each edge
             (B - 1, C - 1, T - 1, H - 1, W - 1)]                                                                 # the very last pixel
    dp = torch.empty(B * T, C, h, w, device=cuda)
    _, amax = ops.upsample_bwd_amax(torch.zeros(B, C, T, H, W, device=cuda), B, T, C, h, w, 4, dp)
    assert float(amax) == 0.0 and not bool(dp.any())
    for spot in spots:
        dout = torch.zeros(B, C, T, H, W, device=cuda)
        dout[spot] = -3.5
        _, amax = ops.upsample_bwd_amax(dout, B, T, C, h, w, 4, dp)
        assert float(amax) == 3.5, spot
        assert rel(dp, up_bwd_ref(dout, B, T, C, h, w, 4, True)) < 1e-5


def test_upsample_bwd_second_trip(ops, cuda):
    """B 2, T 5, C 2497 frames of 6 x 7 at stride 2: 24 970 * 42 = 1 048 740 pooled pixels = 1 048 576 + 164.  Many small frames, not two large ones: the
    source coordinate scale * x is an f32 product, so its weights are only good to ~x * 2^-24 -- at 1448 columns ATen's own float32 bilinear backward is
    already 1e-5 away from float64, at 14 columns it is not."""
    B, T, C, h, w, st = 2, 5, 2497, 6, 7, 2
    assert second_trip(B * T * C * h * w)
    dout = randn(gen(8), B, C, T, h * st, w * st)
    for bilinear in (True, False):
        buf, dp, n = out_flat((B * T, C, h, w), torch.float32)
        ops.upsample_bwd(dout, B, T, C, h, w, st, bilinear, dp)
        assert_guarded_flat(buf, n, 'dpooled'); assert rel(dp, up_bwd_ref(dout, B, T, C, h, w, st, bilinear)) < 1e-5


@pytest.mark.parametrize('S', [2, 3, 300])
@pytest.mark.parametrize('Fc', [1, 16, 17, 40])
@pytest.mark.parametrize('D', [4, 128, 768, 2048])
def test_flags_fwd_forms(ops, cuda, D, Fc, S):
    """G = 1024 / (D / 4) row groups: D = 4 -> 1024 groups of one quad, D = 128 -> 32, D = 768 -> 5 (G * D4 = 960 < 1024: 64 idle threads),
    D = 2048 -> 2; S - 1 = 1, 2 < G leaves groups without a row; F = 17, 40 send the 16 waves round the flag loop again.  1e-5 as today."""
    BT = 2
    g = gen(D + Fc * 7 + S)
    x = torch.randn(BT * S, D, device=cuda, generator=g); Wf = torch.randn(Fc, D, device=cuda, generator=g); bf = torch.randn(Fc, device=cuda, generator=g)
    buf, fl, n = out_flat((BT, Fc), torch.float32)
    ops.flags_fwd(x, BT, S, Wf, bf, fl)
    assert_guarded_flat(buf, n, 'flags')
    assert rel(fl, x.double().reshape(BT, S, D)[:, 1:].mean(1) @ Wf.double().t() + bf.double()) < 1e-5

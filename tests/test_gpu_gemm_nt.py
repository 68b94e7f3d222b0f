"""GPU: the forward GEMM family (tcow_gemm_nt) checked bit-exactly on every tile kernel, epilogue, pitch form and K-loop trip count.

The oracle.  A and W are uniform integers in {-3 ... 3} stored in the mode's dtype, bias / bias2 integers in {-4 ... 4}, resid integers in
{-8 ... 8}, row_scale in {0, 1, 2} (0 = DropPath's dropped row), row_scale2 in {0, 1}, the MUL_AUX tile integers in {-2 ... 2}.  With K <= 384:
    |A W^T| <= 9 K = 3456,   |(A W^T + bias) row_scale| <= 2 (3456 + 4) = 6920,   |... x aux| <= 13 840,   |... + row_scale2 bias2 + resid| <= 13 852 < 2^14
so every product, partial sum and linear epilogue is an integer far below 2^24: exact in f32 in any order and in every mode (bf16, fp16, f32, and
f32x3, whose `lo` split of such a value is 0).  The reference is the f64 expression.  An f32 output must equal it (torch.equal(got.double(), want)),
a 16-bit output must equal want.float().to(dtype): the kernel's conversion is the compiler's round-to-nearest-even (common.h pack_bf2) of an exact
value, as torch's is.  No tolerance.  A failure reports the number of differing entries and the (row tile, column tile) pairs that hold them.

The GELU family (GELU, GELU_DSAVE, DGELU) is not exact.  Its A operand is scaled by 2^-4 (still exact in both 16-bit formats; the pre-activations
then spread over roughly [-8, 8]: standard deviation 4 sqrt(K) / 16 = 2.8 at K = 128).  Exact parts are checked bit for bit: the pre-activation that
ACT_GELU writes to aux, and the DGELU / MUL_AUX aux operand, which must come back unchanged.  The rest is checked element by element:
    want = mult x act + added     act = gelu(v) or gelu'(x) in f64 of the exact argument;  mult = 1 (GELU, GELU_DSAVE, the saved GELU') or the exact
                                  (A W^T + bias) row_scale that DGELU multiplies by;  added = row_scale2 bias2 + resid (exact integers)
    |got - want| <= ABS x |mult|                        the activation's own error (below)
                  + 2^-22 (|mult act| + |added|)        four f32 roundings of 2^-24 (the product x Phi(x) or cdf + x pdf, x mult, + bias2, + resid)
                  + HALF_ULP (|want| + the two above)   the output format: 2^-8 bf16, 2^-11 fp16, 0 for f32
                  + 2^-25 for fp16                      half the spacing of its subnormals (below 2^-14 the format's ulp no longer shrinks)
ABS was measured against this f64 reference on an MI355X at the commit that introduced this module (max over every f32-output case below of
|got - want| / |mult|, no `added` term), then doubled for the 1-ulp spread of the hardware rcp / exp2 between equivalent roundings; the figures
stand next to the constants.  test_report_measured_activation_error prints them again on every run.  The whole bound stays under what
test_gpu_kernels.py grants (2e-5 / 4e-3 / 5e-4 of the maximum for f32 / bf16 / fp16 outputs): 2^-8 = 3.906e-3 and 2^-11 = 4.88e-4 leave 9.4e-5 and
1.2e-5 of the maximum, the other terms are below 1.1e-6 |mult| + 2.4e-7 |want|; _check_act asserts it per case.

The guards.  Every output, the aux tile and resid are [:M, :N] views of [M + 1, N + pad] buffers: outputs and a written aux NaN-filled
(assert_guarded), an aux that the activation does not write keeps its sentinel (assert_untouched), resid's pad columns and spare row hold NaN so an
over-read poisons the result.  A and W are [:, :K] views of [rows + 1, K + 8] NaN buffers (lda = ldw = K + 8), bias / bias2 heads of N + 8 and
row_scale / row_scale2 heads of M + 8 NaN buffers.  Pitch forms: pad8 (ldc = ldr = ldaux = N + 8: `vec8` of nt_pick_epilogue stays true at
N % 8 == 0), pad4 (N + 4: not a multiple of 8, EpiAny on the 320 / 160 tiles at any N) and dense (everything contiguous, A and W too; the spare
rows stay).  Every base pointer is 16-byte aligned in the 16-bit modes.

Tile kernels (forced through tile=, both 16-bit builds) and the cases that reach them -- (tile, epilogue form, pitch form, k-slices) -> test:
    epilogue form                                   pitch   tile 128          tile 256          tile 320 / 160 (N = 264 -> table entry, 260 -> EpiAny)
    the 8 static table entries + EpiAny (TABLE)     pad8    test_epilogues (130, 132, 128) / (258, 260, 128) / (330, 264, 128): 2 k-slices, 1 trip of the 160 loop
    the same with vec8 false                        pad4    test_epilogues, same shapes; and N = 260 with pad8 on 320 / 160
    the same, contiguous                            dense   test_epilogues, same shapes
    EpiAny-only combinations (ANY_ONLY)             all 3   test_epilogues (on 128 / 256 the one run-time epilogue epi_rows serves everything)
    NONE rows 0 / 3 / 5, GELU_DSAVE                 pad8    test_shapes: K = 64, 128, 192 (1, 2, 3 k-slices; 64 = no prefetch, 192 = odd tail);
                                                    dense   tile 160: K = 128, 256, 384 (1, 2, 3 trips of the two-tiles-per-trip loop)
    the same                                                test_shapes: (1, 4, 64) / (1, 8, 64) / (1, 8, 128) one row; (389, 260) 4 x 3, (515, 516) 3 x 3,
                                                            (650, 776) 3 x 4 / 5 x 4 tiles: more tiles than one, not a multiple of the 8 XCDs of xcd_remap
    column bands (nt_tile_of, band 6 / 4 and 0)     pad8    test_column_bands (330, 3072, 128) and (330, 3080, 128) on 320 / 160
    the dispatcher's own choice (tile = 0)          pad8    test_auto_route, one case per kernel
Shapes added from reading the kernels (test_shapes):
    (300, 264) on 320: gemm_bf16.hip `a_last` -- waves 0-3 load the third 16-row A block group (rows 256 ... 319), here 44 of its 64 rows exist;
                       and wave row 1's last 32-row epilogue band (rows 288 ... 319) is partly filled (12 rows), the other bands full.
    (300, 264) on 160: the second row tile holds 140 rows: buffer loads past M return zeros in the middle of a 32-row A subtile group.
    (330, 264) itself: the last row tile holds 10 rows, so every 32-row epilogue band but the first is wholly empty (gemm_nt_common.h `apply` / rows8).

Auto route: 128 at (130, 132, 64); 256 from 700 tiles of 256 while the 320 tile does not fill 80 % of its rounds: (89 345, 260, 64) = 350 x 2 tiles
(320 tile: 280 x 2 = 560 of 768); 320 from 200 tiles that fill 80 % of a round = 205: (32 641, 264, 128) = 103 x 2 = 206; 160 at the same shape with
an f32 residual (c2_pick).  All run well under a second.

The f32-storage modes (NT direction only): gemm_f32.hip has 64 x 64 tiles and k-slices of 16, gemm_x3.hip 128 x 128 tiles and k-slices of 32.
Shapes are one full tile plus a sliver, (66, 68) and (65, 67) for f32, (130, 132) and (129, 131) for f32x3 (the odd N takes the scalar stores),
K = 4, 31, 32, 33, 65.  Operand forms: ld8 (pitch K + 8, aligned: the vector loader whenever K % 4 == 0), ld3 (pitch K + 3: scalar) and off1 (pitch
K + 8, base one float further: scalar).  Output forms: pad8, pad3 (ldc = ldr = ldaux = N + 3: the scalar stores of gemm_x3.hip) and dense.  Both
modes must equal the integer reference bit for bit.  Neither launcher refuses anything by itself (tests/test_gemm_nt_refusals_host.py).

Measured on an MI355X: 61 cases, 1.1 s of test time inside the whole suite (test_gpu_gemm_tn.py: 52 cases, 0.5 s), 4.5 s wall for the module run alone
with interpreter and library start-up.

What the module found when it was written: DGELU and MUL_AUX with a residual multiplied by the RESIDUAL instead of the aux tile in every 16-bit kernel
(epi_row_fetch keeps both in one register slot, gemm_nt_common.h); 'dgelu_rs_res' and 'mulaux_res_f32' of ANY_ONLY are those cases."""
import math

import pytest
import torch

from kernel_forms import NAN, assert_guarded, assert_untouched, bits, guarded

pytestmark = pytest.mark.gpu

MODES16 = ['bf16', 'fp16']
MODES32 = ['f32', 'f32x3']
TILES = [128, 256, 320, 160]
TILE_DIMS = {128: (128, 128), 256: (256, 256), 320: (320, 256), 160: (160, 256), 'f32': (64, 64), 'f32x3': (128, 128)}
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUBNORMAL = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
CAP = {torch.float32: 2e-5, torch.bfloat16: 4e-3, torch.float16: 5e-4}          # of the tensor's maximum: what test_gpu_kernels.py grants
# ABS: (kernel family, quantity) -> absolute error of the activation itself.  Measured / chosen (= 2 x measured, rounded up):
ABS = {('h16', 'gelu'): 8e-7,        # Abramowitz-Stegun erf with rcp / __expf (gemm_nt_common.h gelu_parts2): measured 3.831e-7 (|x| up to 13: the f32 rounding of x Phi(x) is part of it)
       ('h16', 'dgelu'): 4e-7,       # the same code's cdf + x pdf: measured 1.919e-7
       ('f32', 'gelu'): 8e-7,        # erff (common.h gelu_erf): measured 3.831e-7
       ('f32', 'dgelu'): 2.5e-7}     # erff + __expf (gelu_erf_grad): measured 1.158e-7
MEASURED = {}


@pytest.fixture(scope='module')
def ops(cuda):
    from tcow_amd import ops as o
    return o


@pytest.fixture(scope='module')
def cache():
    """(M, N, K) -> integer masters and their f64 reference; (mode, M, N, K, form, scaled) -> operand views.  Computed once, shared, never written."""
    c = {}
    yield c
    c.clear()


def _mode(ops, name):
    return {'f32': (ops.F32, torch.float32), 'f32x3': (ops.F32X3, torch.float32), 'bf16': (ops.BF16, torch.bfloat16), 'fp16': (ops.FP16, torch.float16)}[name]


# ---- operands
class Ref:
    """The integer masters of one (M, N, K) and the exact f64 product."""

    def __init__(self, dev, M, N, K):
        g = torch.Generator(device=dev).manual_seed(((M * 1009 + N) * 1009 + K) * 7 + 3)

        def ints(shape, lo, hi):
            return torch.randint(lo, hi + 1, shape, device=dev, generator=g, dtype=torch.int32).double()
        self.M, self.N, self.K = M, N, K
        self.A, self.W = ints((M, K), -3, 3), ints((N, K), -3, 3)
        self.bias, self.bias2 = ints((N,), -4, 4), ints((N,), -4, 4)
        self.rs, self.rs2 = ints((M,), 0, 2), ints((M,), 0, 1)
        self.resid, self.auxm = ints((M, N), -8, 8), ints((M, N), -2, 2)
        self.dpre = ints((M, N), -32, 32) / 4.0                      # the DGELU operand: multiples of 1/4 in [-8, 8], exact in bf16 and fp16
        self.acc = self.A @ self.W.t()


def _padded(dev, dt, val, pitch, off=0):
    """val [rows, cols] (f64 integers) as the [rows, cols] view, `off` elements into a NaN buffer of rows + 1 rows of `pitch`."""
    rows, cols = val.shape
    flat = torch.full(((rows + 1) * pitch + 8,), NAN, device=dev, dtype=dt)
    view = torch.as_strided(flat, (rows, cols), (pitch, 1), off)
    view.copy_(val.to(dt))
    return flat, view


def _head(dev, val):
    """val [n] as the head of an n + 8 NaN buffer of f32."""
    buf = torch.full((val.numel() + 8,), NAN, device=dev)
    buf[:val.numel()] = val.float()
    return buf[:val.numel()]


AFORMS = {'pad8': (8, 0), 'dense': (0, 0), 'ld8': (8, 0), 'ld3': (3, 0), 'off1': (8, 1)}     # operand form -> (pad columns of A and W, offset of the base in elements)


class Prob:
    """One GEMM's operands in a mode and operand form: A, W (x 2^-4 on A when `scaled`), the vectors, and the reference masters (ref)."""

    def __init__(self, dev, ref, dt, aform, scaled):
        pad, off = AFORMS[aform]
        self.ref, self.dev, self.dt = ref, dev, dt
        self.scale = 2.0 ** -4 if scaled else 1.0
        self._a, self.A = _padded(dev, dt, ref.A * self.scale, ref.K + pad, off)
        self._w, self.W = _padded(dev, dt, ref.W, ref.K + pad, off)
        self.bias, self.bias2, self.rs, self.rs2 = _head(dev, ref.bias), _head(dev, ref.bias2), _head(dev, ref.rs), _head(dev, ref.rs2)


def _prob(cache, dev, mname, dt, M, N, K, aform, scaled, keep=True):
    if not keep:
        return Prob(dev, Ref(dev, M, N, K), dt, aform, scaled)
    if (M, N, K) not in cache:
        cache[(M, N, K)] = Ref(dev, M, N, K)
    key = (mname, M, N, K, aform, scaled)
    if key not in cache:
        cache[key] = Prob(dev, cache[(M, N, K)], dt, aform, scaled)
    return cache[key]


# ---- epilogues: name -> (activation, bias, row_scale, resid, bias2, row_scale2, output 'h' = the mode's dtype / 'f' = f32, resid aliases the output)
def _e(act='NONE', bias=True, rs=False, res=False, b2=False, rs2=False, out='h', inplace=False):
    return dict(act=act, bias=bias, rs=rs, res=res, b2=b2, rs2=rs2, out=out, inplace=inplace)


TABLE = {        # the entries of nt_pick_epilogue (taken on the 320 / 160 tiles while vec8 holds), each also with the other output type where the engine has it
    'none0': _e(),                                                              # EpiCfg<NONE, 0>
    'none0_nobias_f32': _e(bias=False, out='f'),
    'none1': _e(rs=True),                                                       # <NONE, 1>
    'none2': _e(res=True, out='f'),                                             # <NONE, 2>
    'none2_h16': _e(res=True),                                                  # 16-bit output with a residual
    'none2_inplace': _e(res=True, out='f', inplace=True),                       # the residual aliases the f32 output
    'none3': _e(rs=True, res=True, out='f'),                                    # <NONE, 3>
    'none3_inplace': _e(rs=True, res=True, out='f', inplace=True),
    'none7': _e(rs=True, res=True, b2=True, rs2=True, out='f'),                 # <NONE, 7>
    'none7_inplace_plain_b2': _e(rs=True, res=True, b2=True, out='f', inplace=True),   # row_scale2 = NULL: the plain second bias
    'dsave0': _e(act='GELU_DSAVE'),                                             # <GELU_DSAVE, 0>
    'mulaux0': _e(act='MUL_AUX', bias=False),                                   # <MUL_AUX, 0> (kAuxOnly: the aux tile fetched three bands ahead)
    'mulaux0_bias_f32': _e(act='MUL_AUX', out='f'),
    'gelu0': _e(act='GELU'),                                                    # <GELU, 0>, with aux and with aux = NULL
    'gelu0_f32': _e(act='GELU', out='f'),
}
ANY_ONLY = {     # combinations outside the table: EpiAny on the 320 / 160 tiles at any pitch
    'dgelu': _e(act='DGELU', bias=False),
    'dgelu_bias_f32': _e(act='DGELU', out='f'),
    'gelu_rs': _e(act='GELU', rs=True),
    'gelu_rs_b2_res_f32': _e(act='GELU', rs=True, res=True, b2=True, rs2=True, out='f'),
    'dsave_res': _e(act='GELU_DSAVE', res=True, out='f'),
    'dgelu_rs_res': _e(act='DGELU', rs=True, res=True, out='f'),
    'mulaux_rs': _e(act='MUL_AUX', rs=True),
    'mulaux_res_f32': _e(act='MUL_AUX', res=True, out='f'),
    'rows4': _e(b2=True, rs2=True),                                             # rows = 4: bias2 x row_scale2, no row_scale, no resid
    'rows4_plain_b2': _e(b2=True),                                              # rows = 4, row_scale2 = NULL
    'rows5': _e(rs=True, b2=True, rs2=True, out='f'),                           # rows = 5
    'rows5_plain_b2': _e(rs=True, b2=True),
    'rows6': _e(res=True, b2=True, rs2=True, out='f'),                          # rows = 6 (bit 1 of rows is the residual)
}
EPILOGUES = dict(TABLE, **ANY_ONLY)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def _dgelu(x):
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _diff(got, want, tile):
    """'' when got == want, else the number of differing entries and the (row tile, column tile) pairs that hold them."""
    if torch.equal(got, want):
        return ''
    bad = got.double() != want.double()                        # (NaN != x: an over-read or an unwritten element counts)
    tm, tn = TILE_DIMS[tile]
    idx = bad.nonzero()
    tiles = sorted({(int(a), int(b)) for a, b in torch.unique(torch.stack((idx[:, 0] // tm, idx[:, 1] // tn), 1), dim=0).tolist()})
    r, c = idx[0].tolist()
    return (f'{int(bad.sum())} of {bad.numel()} entries differ, {int(got.double().isnan().sum())} NaN; first at ({r}, {c}): got {float(got[r, c])}, want {float(want[r, c])}; '
            f'(row tile, column tile) of {tm} x {tn}: {tiles[:24]}{" ..." if len(tiles) > 24 else ""}')


def _check_act(got, act, mult, added, family, quantity, tile, clean):
    """The elementwise bound of the module docstring; '' or a description of the worst entry."""
    want = mult * act + added
    dt = got.dtype
    tol = ABS[(family, quantity)] * mult.abs() + 2.0 ** -22 * ((mult * act).abs() + added.abs())
    tol = tol + HALF_ULP[dt] * (want.abs() + tol) + SUBNORMAL[dt]
    assert float(tol.max()) <= CAP[dt] * float(want.abs().max()), 'the bound of this case exceeds what test_gpu_kernels.py grants'
    err = (got.double() - want).abs()
    if dt == torch.float32 and clean:
        fig = float((err / mult.abs().clamp_min(1e-30)).nan_to_num(nan=float('inf')).max())
        MEASURED[(family, quantity)] = max(MEASURED.get((family, quantity), 0.0), fig)
    bad = ~(err <= tol)                                        # (NaN fails)
    if not bool(bad.any()):
        return ''
    tm, tn = TILE_DIMS[tile]
    idx = bad.nonzero()
    tiles = sorted({(int(a), int(b)) for a, b in torch.unique(torch.stack((idx[:, 0] // tm, idx[:, 1] // tn), 1), dim=0).tolist()})
    r, c = divmod(int((err / tol).nan_to_num(nan=float('inf')).flatten().argmax()), got.shape[1])
    return (f'{int(bad.sum())} of {bad.numel()} entries off the bound; worst at ({r}, {c}): got {float(got[r, c])}, want {float(want[r, c])}, bound {float(tol[r, c]):.3e}; '
            f'(row tile, column tile) of {tm} x {tn}: {tiles[:24]}')


def _run(ops, P, mname, tile, name, pad, fails, kernel=None):
    """One call of tcow_gemm_nt with the epilogue `name`, outputs at the pitch N + pad; every finding is appended to `fails`.
    kernel: the tile kernel that tile = 0 is expected to pick (for the tile pairs of a report)."""
    e, ref, dev = EPILOGUES[name], P.ref, P.dev
    mode, dt = _mode(ops, mname)
    M, N = ref.M, ref.N
    family = 'h16' if mname in MODES16 else 'f32'
    key = mname if family == 'f32' else (tile or kernel)
    odt = torch.float32 if (e['out'] == 'f' or family == 'f32') else dt
    adt = dt                                                   # the aux tile has the mode's storage type
    act = getattr(ops, 'ACT_' + e['act'])
    what = f'{mname} tile={tile} ({M}, {N}, {ref.K}) {name} pad={pad}'
    # the exact f64 epilogue
    v = ref.acc * P.scale
    if e['bias']:
        v = v + ref.bias
    if e['rs']:
        v = v * ref.rs[:, None]
    added = torch.zeros_like(v)
    if e['b2']:
        added = added + (ref.rs2[:, None] * ref.bias2 if e['rs2'] else ref.bias2.expand(M, N))
    if e['res']:
        added = added + ref.resid
    # outputs and operands with their guards
    cbuf, C = guarded(M, N, N + pad, odt, dev)
    kw = dict(act=act, tile=tile)
    if e['bias']:
        kw['bias'] = P.bias
    if e['rs']:
        kw['row_scale'] = P.rs
    if e['b2']:
        kw['bias2'] = P.bias2
        if e['rs2']:
            kw['row_scale2'] = P.rs2
    if e['res']:
        if e['inplace']:
            C.copy_(ref.resid)
            kw['resid'] = C
        else:
            rbuf, R = guarded(M, N, N + pad, torch.float32, dev)
            R.copy_(ref.resid)
            kw['resid'] = R
    abuf, AUX = guarded(M, N, N + pad, adt, dev)
    if e['act'] == 'MUL_AUX':
        AUX.copy_(ref.auxm)
    elif e['act'] == 'DGELU':
        AUX.copy_(ref.dpre)
    aux_before = abuf.clone()
    ops.gemm_nt(mode, P.A, P.W, C, aux=AUX, **kw)
    # the checks
    try:
        assert_guarded(cbuf, M, N, what + ': C')
        if e['act'] in ('GELU', 'GELU_DSAVE'):
            assert_guarded(abuf, M, N, what + ': aux')
        elif e['act'] == 'NONE':
            assert_untouched(abuf, what + ': aux')
        else:
            assert torch.equal(bits(abuf), bits(aux_before)), what + ': the aux operand was written'
    except AssertionError as err:
        fails.append(str(err))
    clean = not (e['b2'] or e['res'])
    if e['act'] in ('NONE', 'MUL_AUX'):
        want = (v * ref.auxm if e['act'] == 'MUL_AUX' else v) + added
        assert float(want.abs().max()) < 2 ** 24
        d = _diff(C, want.float().to(odt), key)
    elif e['act'] == 'DGELU':
        d = _check_act(C, _dgelu(ref.dpre), v, added, family, 'dgelu', key, clean)
    else:
        d = _check_act(C, _gelu(v), torch.ones_like(v), added, family, 'gelu', key, clean)
        if e['act'] == 'GELU':
            da = _diff(AUX, v.float().to(adt), key)
            if da:
                fails.append(f'{what}: the pre-activation in aux: {da}')
            # aux = NULL must run and give the same output
            c2buf, C2 = guarded(M, N, N + pad, odt, dev)
            if e['inplace']:
                C2.copy_(ref.resid)
                kw['resid'] = C2
            ops.gemm_nt(mode, P.A, P.W, C2, **kw)
            if not torch.equal(bits(c2buf), bits(cbuf)):
                fails.append(f'{what}: aux = NULL gives another output: {_diff(C2, C, key)}')
        else:
            da = _check_act(AUX, _dgelu(v), torch.ones_like(v), torch.zeros_like(v), family, 'dgelu', key, True)
            if da:
                fails.append(f"{what}: the saved GELU' in aux: {da}")
    if d:
        fails.append(f'{what}: C: {d}')


def _report(fails):
    assert not fails, f'{len(fails)} findings:\n' + '\n'.join(fails[:40])


# ---- 1: every epilogue on every tile kernel, in the three pitch forms
EPI_SHAPES = {128: [(130, 132, 128)], 256: [(258, 260, 128)], 320: [(330, 264, 128), (330, 260, 128)], 160: [(330, 264, 128), (330, 260, 128)]}


@pytest.mark.parametrize('form', ['pad8', 'pad4', 'dense'])
@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('mname', MODES16)
def test_epilogues(ops, cuda, cache, mname, tile, form):
    """TABLE and ANY_ONLY on one full tile plus a sliver each way.  On the 320 / 160 tiles: N = 264 with pad8 / dense takes the table's static epilogues
    (and EpiAny for ANY_ONLY), N = 264 with pad4 takes EpiAny at N % 8 == 0 because of the pitch, N = 260 takes EpiAny because of N."""
    _, dt = _mode(ops, mname)
    pad = {'pad8': 8, 'pad4': 4, 'dense': 0}[form]
    fails = []
    for M, N, K in EPI_SHAPES[tile]:
        for name, e in EPILOGUES.items():
            P = _prob(cache, cuda, mname, dt, M, N, K, 'dense' if form == 'dense' else 'pad8', e['act'] in ('GELU', 'GELU_DSAVE', 'DGELU'))
            _run(ops, P, mname, tile, name, pad, fails)
    _report(fails)


# ---- 2: K-loop trip counts, one row, several tiles, the boundaries read out of the loaders
SHAPE_EPILOGUES = ['none0', 'none3', 'rows5', 'dsave0']
KS = {128: (64, 128, 192), 256: (64, 128, 192), 320: (64, 128, 192), 160: (128, 256, 384)}
SHAPES = {128: [(130, 132, k) for k in KS[128]] + [(1, 4, 64), (389, 260, 128)],
          256: [(258, 260, k) for k in KS[256]] + [(1, 4, 64), (515, 516, 128)],
          320: [(330, n, k) for n in (264, 260) for k in KS[320]] + [(1, 8, 64), (650, 776, 128), (300, 264, 128)],
          160: [(330, n, k) for n in (264, 260) for k in KS[160]] + [(1, 8, 128), (650, 776, 128), (300, 264, 128)]}


@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('mname', MODES16)
def test_shapes(ops, cuda, cache, mname, tile):
    _, dt = _mode(ops, mname)
    fails = []
    for M, N, K in SHAPES[tile]:
        for name in SHAPE_EPILOGUES:
            scaled = EPILOGUES[name]['act'] != 'NONE'
            _run(ops, _prob(cache, cuda, mname, dt, M, N, K, 'pad8', scaled), mname, tile, name, 8, fails)
            _run(ops, _prob(cache, cuda, mname, dt, M, N, K, 'dense', scaled), mname, tile, name, 0, fails)
    _report(fails)


# ---- 3: the column-band tile order
@pytest.mark.parametrize('N', [3072, 3080])
@pytest.mark.parametrize('tile', [320, 160])
@pytest.mark.parametrize('mname', MODES16)
def test_column_bands(ops, cuda, mname, tile, N):
    """N = 3072: 12 column tiles, tcow_nt_band_for gives bands of 6 (320) and 4 (160); N = 3080: 13 column tiles, no band.  Exact equality: every tile is
    produced once and in its place (each column of W holds other integers)."""
    _, dt = _mode(ops, mname)
    fails = []
    P = _prob(None, cuda, mname, dt, 330, N, 128, 'pad8', False, keep=False)
    for name in ('none0', 'none3', 'mulaux0'):
        _run(ops, P, mname, tile, name, 8, fails)
    _report(fails)


# ---- 4: the dispatcher's own choice
AUTO = {128: (130, 132, 64, 'none0'),          # fewer than 700 tiles of 256, fewer than 200 of 320: the 128 x 128 kernel
        256: (89345, 260, 64, 'none0'),        # 350 x 2 = 700 tiles of 256; 280 x 2 = 560 tiles of 320 are 73 % of three rounds (< 80 %): the 256 x 256 kernel
        320: (32641, 264, 128, 'none1'),       # 103 x 2 = 206 tiles of 320 >= 200 and 80.5 % of a round, no c2_pick (16-bit output, row scale): the 320 x 256 kernel
        160: (32641, 264, 128, 'none2')}       # the same tiles with an f32 residual at K <= 1024 (c2_pick): the 160 x 256 kernel


@pytest.mark.parametrize('kernel', TILES)
@pytest.mark.parametrize('mname', MODES16)
def test_auto_route(ops, cuda, mname, kernel):
    """tile = 0 at the smallest M at which each threshold of tcow_gemm_nt_bf16 holds at this commit (one row less and the 128 x 128 kernel runs)."""
    _, dt = _mode(ops, mname)
    M, N, K, name = AUTO[kernel]
    fails = []
    _run(ops, _prob(None, cuda, mname, dt, M, N, K, 'pad8', False, keep=False), mname, 0, name, 8, fails, kernel=kernel)
    _report(fails)


# ---- 5: the f32-storage modes
F32_SHAPES = {'f32': [(66, 68), (65, 67)], 'f32x3': [(130, 132), (129, 131)]}
F32_KS = (4, 31, 32, 33, 65)


@pytest.mark.parametrize('aform', ['ld8', 'ld3', 'off1'])
@pytest.mark.parametrize('mname', MODES32)
def test_f32_modes_k_sweep_and_loaders(ops, cuda, cache, mname, aform):
    """K below, at and just above the k-slice (16 for f32, 32 for f32x3), with the vector loader (ld8 at K = 4, 32) and the scalar one (everything else)."""
    fails = []
    for M, N in F32_SHAPES[mname]:
        for K in F32_KS:
            for name, pad in (('none0', 8), ('none7', 3), ('dsave0', 0), ('mulaux0_bias_f32', 8)):
                scaled = EPILOGUES[name]['act'] not in ('NONE', 'MUL_AUX')
                _run(ops, _prob(cache, cuda, mname, torch.float32, M, N, K, aform, scaled), mname, 0, name, pad, fails)
    _report(fails)


@pytest.mark.parametrize('pad', [8, 3, 0])
@pytest.mark.parametrize('mname', MODES32)
def test_f32_modes_epilogues(ops, cuda, cache, mname, pad):
    """Every epilogue operand and activation at K = 33 (scalar loader) and K = 32 (vector loader), outputs at N + 8, N + 3 and dense."""
    fails = []
    for M, N in F32_SHAPES[mname]:
        for K, aform in ((33, 'ld8'), (32, 'ld8')):
            for name, e in EPILOGUES.items():
                if e['out'] == 'h' and name + '_f32' in EPILOGUES:
                    continue                                   # (the output is f32 in these modes: the _f32 twin is the same call)
                _run(ops, _prob(cache, cuda, mname, torch.float32, M, N, K, aform, e['act'] in ('GELU', 'GELU_DSAVE', 'DGELU')), mname, 0, name, pad, fails)
    _report(fails)


# ---- 6: the figures behind ABS
def test_report_measured_activation_error():
    """Runs last: prints max |got - want| / |mult| over the f32-output GELU-family cases of this run, next to the bound in use."""
    for k in sorted(ABS):
        print(f'activation error {k}: measured {MEASURED.get(k, float("nan")):.3e}, bound {ABS[k]:.3e}')
        assert k not in MEASURED or MEASURED[k] <= ABS[k]
    assert ABS[('h16', 'gelu')] <= 2e-5 and ABS[('f32', 'gelu')] <= 2e-5

"""GPU: the weight-gradient GEMM family (tcow_gemm_tn, tcow_gemm_tn_grouped) checked bit-exactly in every kernel form.

The oracle.  dY and X are uniform integers in {-3 ... 3} stored in the mode's dtype.  Every product and every partial sum is then an
integer of magnitude <= 9 M < 2^24 (M < 1.8 M rows), exact in f32 whatever the slice, stage or fold order and in every mode (bf16, fp16,
f32, and f32x3 whose `lo` split of such a value is 0); the bias gradient is a column sum of magnitude <= 3 M.  The reference is
dY.double().t() @ X.double() and dY.double().sum(0), exact in f64, and every assertion is torch.equal(got.double(), want): no tolerance.
A dropped, duplicated or mis-paired token row, a wrong column, a stale slab slice, a lost accumulate or a wrong fold all change integers.

The guards.  Operands are the [:M, :N] / [:M, :K] views of buffers with >= 64 rows of NaN behind row M and, in the strided forms
(ld = N + 8, K + 8), NaN pad columns: any over-read turns an accumulator into NaN.  dW is a view of an [N + 1, K + pad] buffer and
bias_grad the head of an N + 8 buffer, both filled with the sentinel 7.0, which everything outside the view must keep.

The shape comments give (kernel, splits requested, mps = token rows per slice, nz = slices, rows of the last slice) of the host plan
(tcow_amd/csrc/gemm_tn_plan.h: tcow_tn_plan, tcow_tn_group_plan).  They are asserted, shape by shape, on the CPU: tests/test_gemm_tn_plan_host.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = 7.0
MODES16 = ['bf16', 'fp16']
MODES = MODES16 + ['f32', 'f32x3']
# output forms: name -> (pad columns, offset of the data pointer in floats)
FORMS = {'dense': (0, 0),        # contiguous: the folds' dense fast path
         'ld8': (8, 0),          # lddw = K + 8: the vector fold with strided rows
         'ld3': (3, 0),          # lddw = K + 3: the scalar fold, and the row-reduce fold of the bias table
         'off1': (8, 1)}         # lddw = K + 8, data pointer one float further: unaligned, the scalar fold


@pytest.fixture(scope='module')
def ops(cuda):
    from tcow_amd import ops as o
    return o


@pytest.fixture(scope='module')
def refs():
    """(M, N, K, operand pair) -> (dY^T X, column sums of dY) in f64: computed once per operand pair, shared by the tests of the module, never written."""
    cache = {}
    yield cache
    cache.clear()


def _mode(ops, name):
    return {'f32': (ops.F32, torch.float32), 'f32x3': (ops.F32X3, torch.float32), 'bf16': (ops.BF16, torch.bfloat16), 'fp16': (ops.FP16, torch.float16)}[name]


def _seed(M, N, K, pair=0):
    return ((M * 1009 + N) * 1009 + K) * 7 + pair


def _operands(dev, dt, M, N, K, strided=False, pair=0, tail=64):
    """dY [M, N] and X [M, K], integers in {-3 ... 3} (the same ones for every dtype and pitch), as views of NaN-poisoned buffers."""
    g = torch.Generator(device=dev).manual_seed(_seed(M, N, K, pair))
    views = []
    for C in (N, K):
        buf = torch.full((M + tail, C + 8 if strided else C), float('nan'), device=dev, dtype=dt)
        buf[:M, :C] = torch.randint(-3, 4, (M, C), device=dev, generator=g, dtype=torch.int32).to(dt)
        views.append(buf[:M, :C])
    return views


def _reference(refs, dY, X, pair=0):
    key = (dY.shape[0], dY.shape[1], X.shape[1], pair)
    if key not in refs:
        refs[key] = (dY.double().t() @ X.double(), dY.double().sum(0))
    return refs[key]


def _diff(got, want):
    """'' when got == want bit for bit as f64, else the number of differing entries and the (n // 256, k // 256) tiles that hold them."""
    got = got.double()
    if torch.equal(got, want):
        return ''
    bad = got != want                         # (NaN != x: an over-read counts)
    if got.dim() == 1:
        bad = bad[:, None]
    tiles = sorted({(int(a), int(b)) for a, b in torch.unique(bad.nonzero() // 256, dim=0).tolist()})
    return f'{int(bad.sum())} of {bad.numel()} entries differ, {int(got.isnan().sum())} NaN; (n // 256, k // 256) tiles {tiles[:24]}{" ..." if len(tiles) > 24 else ""}'


class Out:
    """Guarded outputs of one weight gradient: dW [N, K] in the given form and bias_grad [N] (or None); accumulate -> pre-filled with small integers."""

    def __init__(self, dev, N, K, form='dense', bias=True, accumulate=False):
        pad, off = FORMS[form]
        self.N, self.K, self.ld, self.off, self.accumulate = N, K, K + pad, off, accumulate
        self.buf = torch.full((N + 1, K + pad), SENT, device=dev)
        self.dW = self._view(self.buf)
        self.bbuf = torch.full((N + 8,), SENT, device=dev) if bias else None
        self.db = self.bbuf[:N] if bias else None
        self.pre_w = self.pre_b = None
        if accumulate:
            g = torch.Generator(device=dev).manual_seed(N * 4099 + K)
            self.pre_w = torch.randint(-3, 4, (N, K), device=dev, generator=g, dtype=torch.int32).double()
            self.pre_b = torch.randint(-3, 4, (N,), device=dev, generator=g, dtype=torch.int32).double()
            self.dW.copy_(self.pre_w)
            if bias:
                self.db.copy_(self.pre_b)

    def _view(self, buf):
        return torch.as_strided(buf, (self.N, self.K), (self.ld, 1), self.off)

    def untouched(self):
        """Nothing has been written: the sentinel (or, with accumulate, the pre-filled integers) everywhere."""
        w = torch.equal(self.dW.double(), self.pre_w) if self.accumulate else bool((self.dW == SENT).all())
        b = True
        if self.bbuf is not None:
            b = torch.equal(self.db.double(), self.pre_b) if self.accumulate else bool((self.db == SENT).all())
            b = b and bool((self.bbuf[self.N:] == SENT).all())
        return w and b and self.guards_ok()

    def guards_ok(self):
        g = self.buf.clone()
        self._view(g).fill_(SENT)
        return bool((g == SENT).all())

    def check(self, ref, what):
        want_w, want_b = ref
        if self.accumulate:
            want_w, want_b = want_w + self.pre_w, want_b + self.pre_b
        d = _diff(self.dW, want_w)
        assert not d, f'{what}: dW: {d}'
        assert self.guards_ok(), f'{what}: wrote outside dW (guard row / pad columns / tail lost the sentinel)'
        if self.bbuf is not None:
            d = _diff(self.db, want_b)
            assert not d, f'{what}: bias_grad: {d}'
            assert bool((self.bbuf[self.N:] == SENT).all()), f'{what}: wrote behind bias_grad'

    def same_bits(self, other):
        return torch.equal(self.buf, other.buf) and (self.bbuf is None or torch.equal(self.bbuf, other.bbuf))


# ---- 1-3: row sweeps (every M a prefix view of one master buffer: the rows behind M hold real data, an over-read changes integers)
def _sweep(ops, dev, mname, N, K, Ms):
    mode, dt = _mode(ops, mname)
    Ms = sorted(Ms)
    dY, X = _operands(dev, dt, Ms[-1], N, K)
    dYd, Xd = dY.double(), X.double()
    # the f64 reference of the first M by a product, of every later one by an exact update with the rows that M adds
    cur, w, b = Ms[0], dYd[:Ms[0]].t() @ Xd[:Ms[0]], dYd[:Ms[0]].sum(0)
    for M in Ms:
        if M > cur:
            w += dYd[cur:M].t() @ Xd[cur:M]
            b += dYd[cur:M].sum(0)
            cur = M
        out = Out(dev, N, K)
        ops.gemm_tn(mode, dY[:M], X[:M], out.dW, bias_grad=out.db)
        out.check((w, b), f'{mname} M={M} N={N} K={K}')


@pytest.mark.parametrize('mname', MODES16)
def test_row_sweep_256_whole_tiles(ops, cuda, mname):
    """N = K = 768 (9 whole tiles, SCHED = 2: every load a buffer load whose descriptor ends at (M - 1) ld + N).
    M = 4800:        (256-tile, 18, 320, 15, 320)   every slice full, 5 stages (odd)
    M = 4801 - 4863: (256-tile, 18, 320, 16, 1 ... 63)   nz 16 < 18 requested; one-stage last slice
    M = 4864:        (256-tile, 19, 256, 19, 256)   M / 256 = 19: one more slice requested, all full, 4 stages (even)
    M = 4865 - 4930: (256-tile, 19, 320, 16, 65 ... 130)   last slice of 2 and 3 stages (128 -> 2, 129 -> 3)"""
    _sweep(ops, cuda, mname, 768, 768, range(4800, 4931))


@pytest.mark.parametrize('mname', MODES16)
@pytest.mark.parametrize('M', [4096, 4224])
def test_256_whole_tiles_full_and_64_row_last_slice(ops, cuda, mname, M):
    """N = K = 768.  M = 4096: (256-tile, 16, 256, 16, 256), every slice full.  M = 4224: (256-tile, 16, 320, 14, 64): the last slice is exactly
    one stage -- the sweep above steps from 63 to 65 rows, because M = 4864 asks for 19 slices of 256."""
    _sweep(ops, cuda, mname, 768, 768, [M])


@pytest.mark.parametrize('mname', MODES16)
def test_row_sweep_256_ragged_tiles(ops, cuda, mname):
    """N = 776, K = 520 (4 x 3 tiles, the last of each ragged: SCHED = 1, interior tiles by buffer loads, edge tiles by guarded global loads).
    M = 4096:        (256-tile, 16, 256, 16, 256)
    M = 4097 - 4160: (256-tile, 16, 320, 13, 257 ... 320)
    M = 4161 - 4230: (256-tile, 16, 320, 14, 1 ... 70)   incl. 63, 64 and 65 rows"""
    _sweep(ops, cuda, mname, 776, 520, range(4096, 4231))


@pytest.mark.parametrize('mname,N,K', [(m, 136, 72) for m in MODES] + [('f32', 70, 50), ('f32x3', 70, 50)])
def test_row_sweep_128_tile(ops, cuda, mname, N, K):
    """N = 136, K = 72 (2 x 1 tiles of 128, both ragged): (128-tile, 1, ceil64(M), 1, M) for every M here, 1 ... 11 stages of 32 rows with every
    remainder.  f32 / f32x3 also at N = 70, K = 50 (not multiples of 4: scalar loaders, the scalar fold and the row-reduce bias fold)."""
    _sweep(ops, cuda, mname, N, K, list(range(1, 141)) + list(range(250, 331)))


# ---- 4: strided and poisoned operands, guarded outputs
STRIDED_SHAPES = [(4133, 768, 768),      # (256-tile SCHED 2, 16, 320, 13, 293)
                  (4133, 776, 520),      # (256-tile SCHED 1, 16, 320, 13, 293)
                  (513, 264, 136),       # (128-tile, 2, 320, 2, 193)
                  (4160, 768, 256)]      # (128-tile, 16, 320, 13, 320): 3 tiles of 256 are too few for the 256-tile kernel


@pytest.mark.parametrize('mname,M,N,K', [(m,) + s for s in STRIDED_SHAPES for m in MODES16] + [('f32', 513, 264, 136), ('f32x3', 513, 264, 136)])
def test_strided_poisoned_operands_guarded_outputs(ops, cuda, refs, mname, M, N, K):
    mode, dt = _mode(ops, mname)
    dY, X = _operands(cuda, dt, M, N, K, strided=True)
    assert dY.stride(0) == N + 8 and X.stride(0) == K + 8
    ref = _reference(refs, dY, X)
    for form in FORMS:
        for accumulate in (False, True):
            for bias in (True, False):
                outs = []
                for _ in range(3):
                    o = Out(cuda, N, K, form, bias, accumulate)
                    ops.gemm_tn(mode, dY, X, o.dW, bias_grad=o.db, accumulate=accumulate)
                    outs.append(o)
                outs[0].check(ref, f'{mname} ({M}, {N}, {K}) {form} accumulate={accumulate} bias={bias}')
                assert outs[1].same_bits(outs[0]) and outs[2].same_bits(outs[0]), f'{mname} ({M}, {N}, {K}) {form}: three calls, different bits'


@pytest.mark.parametrize('mname', MODES16)
def test_engine_form_two_halves_of_one_buffer(ops, cuda, refs, mname):
    """The shared-rgb patch embedding's weight gradient: K = 768 into [:, :768] and K = 256 into [:, 768:] of one [768, 1024] buffer, lddw = 1024.
    (4133, 768, 768): (256-tile SCHED 2, 16, 320, 13, 293); (4133, 768, 256): (128-tile, 16, 320, 13, 293)."""
    mode, dt = _mode(ops, mname)
    M, N = 4133, 768
    dY, Xa = _operands(cuda, dt, M, N, 768, strided=True)
    dYb, Xb = _operands(cuda, dt, M, N, 256, strided=True, pair=1)
    buf = torch.full((N + 1, 1024), SENT, device=cuda)
    dW = buf[:N]
    ops.gemm_tn(mode, dY, Xa, dW[:, :768])
    d = _diff(dW[:, :768], _reference(refs, dY, Xa)[0])
    assert not d, f'first half: {d}'
    assert bool((dW[:, 768:] == SENT).all()) and bool((buf[N] == SENT).all()), 'the first call touched the other half or the guard row'
    ops.gemm_tn(mode, dYb, Xb, dW[:, 768:])
    for half, X_, dY_, pair in ((dW[:, :768], Xa, dY, 0), (dW[:, 768:], Xb, dYb, 1)):
        d = _diff(half, _reference(refs, dY_, X_, pair)[0])
        assert not d, f'after the second call, half of K = {X_.shape[1]}: {d}'
    assert bool((buf[N] == SENT).all())


# ---- 5: bias-table edges
@pytest.mark.parametrize('mname', MODES16)
@pytest.mark.parametrize('M,N,K', [(4096, 8, 4224),        # (128-tile, 16, 256, 16, 256): 33 k-tiles > 32 stage rows -> rows_per_pk = 1, the last k-tile sums no bias row; fused bias
                                   (4096, 256, 16640),     # (256-tile SCHED 2, 3, 1408, 3, 1280): 65 k-tiles of 256 > 64 stage rows; fused bias (3 x 65 x 2 = 390 table rows)
                                   (2048, 8, 24704)])      # (128-tile, 8, 256, 8, 256): 8 x 193 x 2 = 3088 > 3072 table rows -> un-fused bias (tcow_launch_colsum)
def test_bias_table_edges(ops, cuda, refs, mname, M, N, K):
    mode, dt = _mode(ops, mname)
    dY, X = _operands(cuda, dt, M, N, K)
    ref = _reference(refs, dY, X)
    for accumulate in (False, True):
        o = Out(cuda, N, K, 'dense', True, accumulate)
        ops.gemm_tn(mode, dY, X, o.dW, bias_grad=o.db, accumulate=accumulate)
        o.check(ref, f'{mname} ({M}, {N}, {K}) accumulate={accumulate}')


# ---- 6: exact workspace
PATTERN = 4096


def _exact_workspace(dev, nbytes):
    """A workspace of exactly nbytes (every bit set: NaN to a kernel that reads what it has not written) with a byte pattern in the 4 KiB behind it."""
    raw = torch.full((nbytes + PATTERN,), 0xFF, dtype=torch.uint8, device=dev)
    pattern = (torch.arange(PATTERN, device=dev) % 251).to(torch.uint8)
    raw[nbytes:] = pattern
    return raw, pattern


def _tn_direct(ops, mode, dY, X, o, accumulate, ws_ptr, ws_bytes):
    from tcow_amd import _lib as L
    lib, dm = ops._sel(mode)
    M, N = dY.shape
    L.check(lib.tcow_gemm_tn(ops._stream(), dm, M, N, X.shape[1], dY.data_ptr(), dY.stride(0), X.data_ptr(), X.stride(0), o.dW.data_ptr(), o.dW.stride(0),
                             ops._p(o.db), int(accumulate), ws_ptr, ws_bytes), 'tcow_gemm_tn', lib)


@pytest.mark.parametrize('mname,M,N,K', [(m, 4133, 768, 768) for m in MODES16] + [(m, 513, 264, 136) for m in MODES])
def test_exact_workspace_single(ops, cuda, refs, mname, M, N, K):
    from tcow_amd._lib import TcowError
    mode, dt = _mode(ops, mname)
    dY, X = _operands(cuda, dt, M, N, K, strided=True)
    ref = _reference(refs, dY, X)
    nbytes = int(ops._sel(mode)[0].tcow_gemm_tn_workspace_bytes(M, N, K))
    for form in ('dense', 'ld3'):
        raw, pattern = _exact_workspace(cuda, nbytes)
        o = Out(cuda, N, K, form, True, False)
        _tn_direct(ops, mode, dY, X, o, False, raw.data_ptr(), nbytes)
        o.check(ref, f'{mname} ({M}, {N}, {K}) {form}, workspace of exactly {nbytes} bytes')
        assert torch.equal(raw[nbytes:], pattern), 'wrote behind the workspace'
    o = Out(cuda, N, K, 'dense', True, False)
    with pytest.raises(TcowError):
        _tn_direct(ops, mode, dY, X, o, False, raw.data_ptr(), nbytes - 1)
    torch.cuda.synchronize()
    assert o.untouched(), 'a refused call wrote to its outputs'


# ---- 7: grouped launches
def _problems(ops, dev, refs, dt, specs):
    """specs: (M, N, K, bias, accumulate, form, pair) -> (the tuples of ops.gemm_tn_grouped, the guarded outputs, the references)."""
    operands, probs, outs, want = {}, [], [], []
    for M, N, K, bias, accumulate, form, pair in specs:
        if (M, N, K, pair) not in operands:
            operands[(M, N, K, pair)] = _operands(dev, dt, M, N, K, strided=True, pair=pair)
        dY, X = operands[(M, N, K, pair)]
        o = Out(dev, N, K, form, bias, accumulate)
        probs.append((dY, X, o.dW, o.db, int(accumulate)))
        outs.append(o)
        want.append(_reference(refs, dY, X, pair))
    return probs, outs, want


def _run_group(ops, dev, refs, mname, specs, what):
    mode, dt = _mode(ops, mname)
    probs, outs, want = _problems(ops, dev, refs, dt, specs)
    ops.gemm_tn_grouped(mode, probs)
    for i, (o, w, s) in enumerate(zip(outs, want, specs)):
        o.check(w, f'{what} {mname} problem {i} {s}')


GM = 4133
# 30 tiles -> the group plan asks for 8 slices: (256-tile group SCHED 1 -- one problem is ragged --, 8, 576, 8, 101); all folds by the one group fold launch
GROUP_MIXED = [(GM, 768, 768, True, False, 'dense', 0), (GM, 776, 520, False, True, 'ld8', 0), (GM, 256, 2304, True, True, 'ld8', 0)]


@pytest.mark.parametrize('mname', MODES16)
def test_group_mixed_whole_and_ragged(ops, cuda, refs, mname):
    """7a: whole and ragged problems in one grid, bias_grad present / None, accumulate 0 / 1, contiguous / lddw = K + 8 (the group fold's strided branch)."""
    _run_group(ops, cuda, refs, mname, GROUP_MIXED, '7a')
    _run_group(ops, cuda, refs, mname, [(GM, 768, 768, True, True, 'ld8', 0), (GM, 776, 520, True, False, 'dense', 0), (GM, 256, 2304, False, False, 'dense', 0)], '7a, flipped')


@pytest.mark.parametrize('mname', MODES16)
def test_group_with_scalar_fold_member(ops, cuda, refs, mname):
    """7b: one member at lddw = K + 3 (and, second run, at an unaligned pointer): tcow_fold_vec_ok fails for the group, every problem is folded by its own launch."""
    for form in ('ld3', 'off1'):
        specs = [GROUP_MIXED[0], GROUP_MIXED[1], (GM, 256, 2304, True, True, form, 0)]
        _run_group(ops, cuda, refs, mname, specs, f'7b {form}')


@pytest.mark.parametrize('mname', MODES16)
def test_group_one_slice_direct_write(ops, cuda, refs, mname):
    """7c: 64 + 64 + 64 + 64 = 256 tiles -> the group plan asks for 1 slice (cost 1.044 against 1.088 for two slices): (256-tile group SCHED 2, 1, 4160, 1, 4133).
    The plain problem and the one without bias_grad are written straight into dW (slab = dW, no fold blocks); accumulate = 1 and lddw = K + 8 go through a slab."""
    specs = [(GM, 2048, 2048, True, False, 'dense', 0), (GM, 1024, 4096, True, True, 'dense', 0), (GM, 4096, 1024, True, False, 'ld8', 0), (GM, 2048, 2048, False, False, 'dense', 1)]
    _run_group(ops, cuda, refs, mname, specs, '7c')


def _many(n):
    """n problems of (768, 768) on two operand pairs, every one with outputs of its own; forms, bias and accumulate vary with the index."""
    return [(GM, 768, 768, i % 3 != 1, i % 4 == 2, ('dense', 'ld8')[i % 2], i % 2) for i in range(n)]


@pytest.mark.parametrize('mname', MODES16)
def test_group_of_exactly_group_max(ops, cuda, refs, mname):
    """7d: tcow_gemm_tn_group_max() problems, the last entry of first[]: 360 tiles -> 2 slices: (256-tile group SCHED 2, 2, 2112, 2, 2021)."""
    _run_group(ops, cuda, refs, mname, _many(ops.tn_group_max()), '7d')


@pytest.mark.parametrize('mname', MODES16)
def test_group_one_problem_too_many(ops, cuda, refs, mname):
    """7e: group_max + 1 problems: the library-side loop, each (256-tile SCHED 2, 16, 320, 13, 293)."""
    _run_group(ops, cuda, refs, mname, _many(ops.tn_group_max() + 1), '7e')


@pytest.mark.parametrize('mname', MODES16)
def test_group_with_different_M(ops, cuda, refs, mname):
    """7f: problems that do not share M go one by one: (4133, 768, 768) -> (256-tile SCHED 2, 16, 320, 13, 293), (4200, 768, 768) -> (256-tile SCHED 2, 16, 320, 14, 40),
    (513, 264, 136) -> (128-tile, 2, 320, 2, 193)."""
    specs = [(4133, 768, 768, True, False, 'dense', 0), (4200, 768, 768, True, True, 'ld8', 0), (513, 264, 136, False, False, 'ld3', 0)]
    _run_group(ops, cuda, refs, mname, specs, '7f')


@pytest.mark.parametrize('mname', MODES16)
def test_exact_workspace_grouped(ops, cuda, refs, mname):
    """The group of 7a through the C ABI with a workspace of exactly tcow_gemm_tn_grouped_workspace_bytes; one byte less is refused on the host."""
    from tcow_amd import _lib as L
    mode, dt = _mode(ops, mname)
    lib, dm = ops._sel(mode)

    def table(probs):
        arr = (L.TnProblem * len(probs))()
        for i, (dY, X, dW, db, acc) in enumerate(probs):
            arr[i] = L.TnProblem(dY.shape[0], dY.shape[1], X.shape[1], dY.data_ptr(), dY.stride(0), X.data_ptr(), X.stride(0), dW.data_ptr(), dW.stride(0), ops._p(db), acc)
        return arr

    probs, outs, want = _problems(ops, cuda, refs, dt, GROUP_MIXED)
    arr = table(probs)
    nbytes = int(lib.tcow_gemm_tn_grouped_workspace_bytes(dm, len(probs), arr))
    raw, pattern = _exact_workspace(cuda, nbytes)
    L.check(lib.tcow_gemm_tn_grouped(ops._stream(), dm, len(probs), arr, raw.data_ptr(), nbytes), 'tcow_gemm_tn_grouped', lib)
    for i, (o, w) in enumerate(zip(outs, want)):
        o.check(w, f'{mname} problem {i}, workspace of exactly {nbytes} bytes')
    assert torch.equal(raw[nbytes:], pattern), 'wrote behind the workspace'
    probs, outs, _ = _problems(ops, cuda, refs, dt, GROUP_MIXED)
    arr = table(probs)
    with pytest.raises(L.TcowError):
        L.check(lib.tcow_gemm_tn_grouped(ops._stream(), dm, len(probs), arr, raw.data_ptr(), nbytes - 1), 'tcow_gemm_tn_grouped', lib)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs), 'a refused call wrote to its outputs'

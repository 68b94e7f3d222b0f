"""GPU: the 128 x 128 bf16 x 3 kernel (csrc/gemm_x3.hip) checked bit-exactly on operands with a non-zero `lo` plane, in its three entry points:
tcow_gemm_nt_x3 (ops.gemm_nt(F32X3)), tcow_gemm_tn_x3 (ops.gemm_tn(F32X3), slabs folded by reduce.hip) and tcow_sgemm_x3_batched (ops.sgemm_batched).

The oracle (kernel_forms.hi_lo_operand / want_hi_lo, proved on the CPU by test_x3_planes_host.py).  Every operand element is x = h + l with h in
{+-2, +-3} and l in {-3 .. 3} 2^-10, so bf16(x) = h and bf16(x - h) = l exactly.  Every kept term (hi hi, hi lo, lo hi) is a multiple of 2^-10 and
every partial sum stays below 2^24 of those units while the contraction length is at most 1800 (9.02 x 1024 x 1800 < 2^24): the f32 result is
    want = hi_A hi_B^T + hi_A lo_B^T + lo_A hi_B^T        (f64, planes taken with torch's bf16 cast)
exactly, whatever the slice, split-K or fold order.  want_hi_lo asserts per case that hi + lo is the operand, that both lo planes are non-zero and
that want differs from the full product.  Epilogue operands keep the result a multiple of 2^-10 (integer bias / bias2 / residual / pre-fill, row
scales in {0, 1, 2} and {0, 1}, the MUL_AUX tile in {-2 .. 2}); _exact asserts that every expected output stays below 2^24 units.  Every
comparison is torch.equal(got.double(), want): the module holds no tolerance.  The integer suites (test_gpu_gemm_nt.py, test_gpu_gemm_tn.py) run
the same kernel with lo = 0, where two of the three MFMAs add zero; the GELU family is theirs.

The guards.  Outputs, residuals and the aux tile are views of NaN-filled flat buffers with a spare row, pad columns and 8 spare floats (Out): a
stray write destroys a NaN, a missing one leaves it.  Operands are views of NaN buffers with spare rows behind the last row and pad columns in the
strided forms (_stored): an over-read becomes a NaN in an accumulator.  Vectors are heads of NaN buffers.  No output is a torch.empty.

Which code each case runs is not left to the docstrings alone: _nt_loader, _tn_loader and x3_loader below mirror the host selection of
tcow_gemm_nt_x3, tcow_gemm_tn_x3 and x3_loader / the launch branches of tcow_sgemm_x3_batched, and every test asserts the loader (and, batched, the
branch) its table names before it calls the library.  _v16 mirrors the store-path choice of gemm_x3_body's epilogue.

NT form, (M, N) = (130, 132), (129, 131) and (257, 259) -- 2 x 2 and 3 x 3 tiles; 9 tiles run the XCD remap of gemm_x3_body with q = 1, rr = 1:
    operands  ld8 (pitch K + 8): LD_KVEC at K = 4, 28, 32, 36, 64, 96, 100 (28, 36, 100: the last slice holds 7, 1, 1 float4 groups; 32, 96: an odd
              slice count, the extra all-zero slice runs; 64: one loop trip; 4: K below a slice), LD_ANY at K = 31, 33, 65 (scalar tails)
              ld3 (pitch K + 3) and off1 (pitch K + 8, base one float further): LD_ANY at every K
    outputs   v16 (ldc = N rounded up to 4, + 8): the 16-byte stores; at the odd N the last group of a row takes the scalar tail
              pad3 (ldc = N + 3) and off1 (the v16 pitch, base one float further): the scalar stores; dense: v16 at N = 132, scalar at 131 / 259
    epilogues plain, bias, bias + row_scale + resid, resid aliasing the output, bias2 + row_scale2, MUL_AUX at K = 100 (LD_KVEC) and K = 65 (LD_ANY)
TN form, dW [N, K] = dY [M, N]^T X [M, K]: the token count M is the contraction.  (N, K) = (264, 136) dense or pitch + 8: LD_RVEC; pitch + 3, base
+ 1 float, and (70, 50): LD_ANY.  (splits, mps, nz, rows of the last slice) by tcow_tn_plan, the same for both shapes, asserted on the CPU in
test_gemm_tn_plan_host.py (X3_PLANE_SWEEP):
    M = 1: (1, 32, 1, 1)    31: (1, 32, 1, 31)    32: (1, 32, 1, 32)    33: (1, 64, 1, 33)    64: (1, 64, 1, 64)    65: (1, 96, 1, 65)
    255: (1, 256, 1, 255)   513: (2, 288, 2, 225) -- 9 k-slices per z-slice, an odd count       1793: (7, 288, 7, 65) -- a short last slice
Batched form: BATCH_CASES names, case by case, the (A loader, B loader) that x3_loader gives and the kernel that is launched.

Arithmetic-only mutants of gemm_x3.hip, each run once against this module when it was written (cases that failed / of 50):
    first MFMA line takes ah for al (2 hi hi + lo hi)                    50: every case
    second MFMA line takes al for ah (lo lo for lo hi; 0 on integers)    50: every case
    mask_tail<LD_RVEC> leaves v[2 ps + 1] unmasked                       8: the LD_RVEC cases with a ragged last slice -- test_tn_token_sweep dense / ld8, the three
                                                                         test_tn_output_forms ld8 cases, test_tn_grouped, batched rvec_rvec and the (RVEC, RVEC) mixed sizes
    store_split<LD_ANY> stores h, or 0, into the lo plane                40: every case whose table names LD_ANY; the 10 all-vector cases pass
Measured on an MI355X: 50 cases, 3.1 s wall for the module run alone with interpreter and library start-up."""
import pytest
import torch

from kernel_forms import NAN, X3_MAX_CONTRACTION, bits, hi_lo_operand, planes, want_hi_lo

pytestmark = pytest.mark.gpu

KVEC, RVEC, ANY = 'LD_KVEC', 'LD_RVEC', 'LD_ANY'


@pytest.fixture(scope='module')
def ops(cuda):
    from tcow_amd import ops as o
    return o


@pytest.fixture(scope='module')
def pairs():
    """(rows of A, rows of B, contraction, tag) -> (A, B, want): dense operand values and their f64 reference on the device, computed once per
    operand pair, shared by the tests of the module, never written."""
    cache = {}
    yield cache
    cache.clear()


# ---- operands and references
def _pair(pairs, dev, ra, rb, K, tag=0):
    """A [ra, K] and B [rb, K] of hi_lo_operand and want_hi_lo(A, B) [ra, rb].  Drawn on the CPU (the same numbers on every device); a draw whose
    lo plane, or whose lo lo product, is all zero -- possible only for the one-row, one-column operands -- is drawn again."""
    key = (ra, rb, K, tag)
    if key not in pairs:
        assert K <= X3_MAX_CONTRACTION
        g = torch.Generator().manual_seed(((ra * 1009 + rb) * 1009 + K) * 7 + tag)
        for _ in range(256):
            A, B = hi_lo_operand(g, (ra, K), 'cpu'), hi_lo_operand(g, (rb, K), 'cpu')
            if bool((planes(A)[1] @ planes(B)[1].t() != 0).any()):
                break
        else:
            raise AssertionError(f'no operand pair with a visible lo lo term for {key}')
        A, B = A.to(dev), B.to(dev)
        pairs[key] = (A, B, want_hi_lo(A, B))
    return pairs[key]


def _ints(dev, seed, shape, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double().to(dev)


def _stored(val, form, pad=0, off=0, spare=1):
    """val [rows, K] as a [rows, K] view of a NaN-filled flat buffer.  form 'k': the contraction index contiguous, rows at a pitch of K + pad;
    form 'r': the row index contiguous, k-rows at a pitch of rows + pad.  `off` floats before the first element, `spare` whole pitches of NaN
    behind the last one."""
    inner_first = val if form == 'k' else val.t()
    outer, inner = inner_first.shape
    ld = inner + pad
    flat = torch.full((off + (outer + spare) * ld + 8,), NAN, device=val.device)
    st = torch.as_strided(flat, (outer, inner), (ld, 1), off)
    st.copy_(inner_first)
    return st if form == 'k' else st.t()


def _head(val, spare=8):
    buf = torch.full((val.numel() + spare,), NAN, device=val.device)
    buf[:val.numel()] = val.float()
    return buf[:val.numel()]


class Out:
    """A [rows, cols] output at pitch ld, `off` floats into a NaN-filled flat buffer of rows + 1 pitches and 8 spare floats; pre: what the view
    holds before the call (a residual that aliases the output, the pre-fill of accumulate)."""

    def __init__(self, dev, rows, cols, ld, off=0, pre=None):
        assert ld >= cols
        self.geom = ((rows, cols), (ld, 1), off)
        self.flat = torch.full((off + (rows + 1) * ld + 8,), NAN, device=dev)
        self.v = torch.as_strided(self.flat, *self.geom)
        if pre is not None:
            self.v.copy_(pre)

    def guards_ok(self):
        g = self.flat.clone()
        torch.as_strided(g, *self.geom).fill_(NAN)
        return torch.equal(bits(g), bits(torch.full_like(g, NAN)))

    def untouched(self, pre=None):
        inside = bool(self.v.isnan().all()) if pre is None else torch.equal(self.v.double(), pre)
        return inside and self.guards_ok()


def _exact(want):
    assert float(want.abs().max()) * 1024 < 2 ** 24 and torch.equal((want * 1024).round(), want * 1024), 'the case leaves the exact range of the oracle'
    return want


def _diff(got, want):
    """'' when got == want bit for bit as f64, else the number of differing entries, the first of them and the 128 x 128 tiles that hold them."""
    got = got.double()
    if torch.equal(got, want):
        return ''
    bad = got != want                         # (NaN != x: an over-read or an unwritten element counts)
    if bad.dim() == 1:
        bad, got, want = bad[:, None], got[:, None], want[:, None]
    idx = bad.nonzero()
    tiles = sorted({(int(a), int(b)) for a, b in torch.unique(idx // 128, dim=0).tolist()})
    r, c = idx[0].tolist()
    return (f'{int(bad.sum())} of {bad.numel()} entries differ, {int(got.isnan().sum())} NaN; first at ({r}, {c}): got {float(got[r, c])!r}, want {float(want[r, c])!r}; '
            f'(row tile, column tile) of 128 x 128: {tiles[:16]}{" ..." if len(tiles) > 16 else ""}')


def _check(out, want, what, fails):
    d = _diff(out.v, _exact(want))
    if d:
        fails.append(f'{what}: {d}')
    if not out.guards_ok():
        fails.append(f'{what}: wrote outside the output (spare row, pad columns or the floats around the view lost their NaN)')


def _report(fails):
    assert not fails, f'{len(fails)} findings:\n' + '\n'.join(fails[:40])


def _al16(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


# ---- mirrors of the host selection in gemm_x3.hip
def _nt_loader(A, W):
    """tcow_gemm_nt_x3: float4 along k when both bases are 16-byte aligned and lda, ldw and K are multiples of 4."""
    return KVEC if _al16(A, W) and (A.stride(0) | W.stride(0) | A.shape[1]) % 4 == 0 else ANY


def _tn_loader(dY, X):
    """tcow_gemm_tn_x3: float4 along the rows when both bases are aligned and ldy, ldx, N and K are multiples of 4."""
    return RVEC if _al16(dY, X) and (dY.stride(0) | X.stride(0) | dY.shape[1] | X.shape[1]) % 4 == 0 else ANY


def x3_loader(t):
    """x3_loader of tcow_sgemm_x3_batched for an operand given as its [rows, K] view."""
    (rows, K), (s_row, s_k) = t.shape, t.stride()
    if s_k == 1 and _al16(t) and s_row % 4 == 0 and K % 4 == 0 and K >= 4:
        return KVEC
    if s_row == 1 and _al16(t) and s_k % 4 == 0 and rows % 4 == 0 and rows >= 4:
        return RVEC
    return ANY


BRANCHES = [(KVEC, KVEC), (KVEC, RVEC), (RVEC, RVEC), (RVEC, ANY)]          # the instantiations besides <LD_ANY, LD_ANY>, which takes everything else


def _batch_loaders(probs):
    """((A loader, B loader) after the demotion over the problems of a call, the pair of the kernel that is launched)."""
    la = lb = None
    for A, B, _ in probs:
        a, b = x3_loader(A), x3_loader(B.t())
        la, lb = (a if la in (None, a) else ANY), (b if lb in (None, b) else ANY)
    return (la, lb), ((la, lb) if (la, lb) in BRANCHES else (ANY, ANY))


def _v16(*ts):
    """The 16-byte store path of the epilogue: C, resid, aux and bias2 aligned and the pitches of the 2-D ones multiples of 4."""
    return _al16(*ts) and all(t is None or t.dim() < 2 or t.stride(0) % 4 == 0 for t in ts)


# ---- NT form
NT_SHAPES = [(130, 132), (129, 131), (257, 259)]
NT_KS = (4, 28, 31, 32, 33, 36, 64, 65, 96, 100)
AFORMS = {'ld8': (8, 0), 'ld3': (3, 0), 'off1': (8, 1)}          # operand form -> (pad columns of A and W, offset of the base in floats)
OFORMS = {'v16': (lambda N: (N + 3) // 4 * 4 + 8, 0), 'pad3': (lambda N: N + 3, 0), 'off1': (lambda N: (N + 3) // 4 * 4 + 8, 1), 'dense': (lambda N: N, 0)}


def _nt_operands(pairs, dev, M, N, K, aform):
    A, W, want = _pair(pairs, dev, M, N, K)
    pad, off = AFORMS[aform]
    return _stored(A, 'k', pad, off), _stored(W, 'k', pad, off), want


def _out(dev, M, N, oform, pre=None):
    ld, off = OFORMS[oform]
    return Out(dev, M, N, ld(N), off, pre)


@pytest.mark.parametrize('aform', list(AFORMS))
@pytest.mark.parametrize('M,N', NT_SHAPES)
def test_nt_k_sweep_loaders_and_store_paths(ops, cuda, pairs, M, N, aform):
    """Every K of NT_KS in one operand form, into every output form; no epilogue operands.  ld8: LD_KVEC when K % 4 == 0, else LD_ANY; ld3 and
    off1: LD_ANY.  v16 and, at N = 132, dense: the 16-byte stores; everything else the scalar ones."""
    fails = []
    for K in NT_KS:
        A, W, want = _nt_operands(pairs, cuda, M, N, K, aform)
        assert _nt_loader(A, W) == (KVEC if aform == 'ld8' and K % 4 == 0 else ANY)
        for oform in OFORMS:
            out = _out(cuda, M, N, oform)
            assert _v16(out.v) == (oform == 'v16' or (oform == 'dense' and N % 4 == 0))
            ops.gemm_nt(ops.F32X3, A, W, out.v)
            _check(out, want, f'({M}, {N}, {K}) {aform} -> {oform}', fails)
    _report(fails)


NT_EPILOGUES = ['plain', 'bias', 'bias_rs_res', 'res_alias', 'b2_rs2', 'mul_aux']


@pytest.mark.parametrize('oform', ['v16', 'pad3', 'dense'])
@pytest.mark.parametrize('M,N', NT_SHAPES)
def test_nt_epilogues(ops, cuda, pairs, M, N, oform):
    """The linear epilogues at K = 100 (ld8: LD_KVEC) and K = 65 (ld8: LD_ANY).  The residual and the MUL_AUX tile have the output's form; bias and
    bias2 are integers in {-4 .. 4}, row_scale in {0, 1, 2}, row_scale2 in {0, 1}, resid in {-8 .. 8}, the aux tile in {-2 .. 2}."""
    seed = M * 1009 + N
    bias, bias2 = _ints(cuda, seed, (N,), -4, 4), _ints(cuda, seed + 1, (N,), -4, 4)
    rs, rs2 = _ints(cuda, seed + 2, (M,), 0, 2), _ints(cuda, seed + 3, (M,), 0, 1)
    resid, auxm = _ints(cuda, seed + 4, (M, N), -8, 8), _ints(cuda, seed + 5, (M, N), -2, 2)
    hb, hb2, hrs, hrs2 = _head(bias), _head(bias2), _head(rs), _head(rs2)
    fails = []
    for K, loader in ((100, KVEC), (65, ANY)):
        A, W, acc = _nt_operands(pairs, cuda, M, N, K, 'ld8')
        assert _nt_loader(A, W) == loader
        for name in NT_EPILOGUES:
            what = f'({M}, {N}, {K}) {name} -> {oform}'
            kw, want, pre, aux = {}, acc, None, None
            if name in ('bias', 'bias_rs_res'):
                kw['bias'] = hb; want = want + bias
            if name == 'bias_rs_res':
                kw['row_scale'] = hrs; want = want * rs[:, None]
            if name == 'mul_aux':
                aux = _out(cuda, M, N, oform, auxm)
                kw.update(act=ops.ACT_MUL_AUX, aux=aux.v); want = want * auxm
                before = aux.flat.clone()
            if name == 'b2_rs2':
                kw.update(bias2=hb2, row_scale2=hrs2); want = want + rs2[:, None] * bias2
            if name == 'bias_rs_res':
                r = _out(cuda, M, N, oform, resid)
                kw['resid'] = r.v; want = want + resid
            if name == 'res_alias':
                pre = resid; want = want + resid
            out = _out(cuda, M, N, oform, pre)
            if name == 'res_alias':
                kw['resid'] = out.v
            assert _v16(out.v, kw.get('resid'), kw.get('aux'), kw.get('bias2')) == (oform == 'v16' or (oform == 'dense' and N % 4 == 0))
            ops.gemm_nt(ops.F32X3, A, W, out.v, **kw)
            _check(out, want, what, fails)
            if aux is not None and not torch.equal(bits(aux.flat), bits(before)):
                fails.append(f'{what}: the aux operand was written')
    _report(fails)


# ---- TN form
TN_MS = (1, 31, 32, 33, 64, 65, 255, 513, 1793)
TN_OPERANDS = [(264, 136, 'dense', RVEC), (264, 136, 'ld8', RVEC), (264, 136, 'ld3', ANY), (264, 136, 'off1', ANY), (70, 50, 'dense', ANY)]
TN_FORMS = {'dense': (0, 0), 'ld8': (8, 0), 'ld3': (3, 0), 'off1': (8, 1)}      # of the operands (pitch N / K + pad) and of dW (lddw = K + pad): (pad, base offset)


def _tn_operands(pairs, dev, M, N, K, form):
    """dY [M, N] and X [M, K] token-major with 4 spare rows of NaN; (dW, bias gradient) in f64."""
    dYt, Xt, want = _pair(pairs, dev, N, K, M)
    pad, off = TN_FORMS[form]
    dY, X = _stored(dYt.t(), 'k', pad, off, spare=4), _stored(Xt.t(), 'k', pad, off, spare=4)
    key = ('colsum', N, K, M)
    if key not in pairs:
        pairs[key] = dYt.double().sum(1)
    return dY, X, want, pairs[key]


class TnOut:
    """dW [N, K] in one of TN_FORMS and bias_grad as the head of an N + 8 buffer (or None); accumulate: both pre-filled with integers in {-3 .. 3}."""

    def __init__(self, dev, N, K, form, bias, accumulate):
        pad, off = TN_FORMS[form]
        self.pre_w = _ints(dev, N * 4099 + K, (N, K), -3, 3) if accumulate else None
        self.pre_b = _ints(dev, N * 4099 + K + 1, (N,), -3, 3) if accumulate else None
        self.w = Out(dev, N, K, K + pad, off, self.pre_w)
        self.bbuf = torch.full((N + 8,), NAN, device=dev) if bias else None
        self.db = self.bbuf[:N] if bias else None
        if bias and accumulate:
            self.db.copy_(self.pre_b)

    def check(self, want_w, want_b, what, fails):
        if self.pre_w is not None:
            want_w, want_b = want_w + self.pre_w, want_b + self.pre_b
        _check(self.w, want_w, what + ': dW', fails)
        if self.bbuf is not None:
            d = _diff(self.db, _exact(want_b))
            if d:
                fails.append(f'{what}: bias_grad: {d}')
            if not bool(self.bbuf[self.db.numel():].isnan().all()):
                fails.append(f'{what}: wrote behind bias_grad')

    def same_bits(self, other):
        return torch.equal(bits(self.w.flat), bits(other.w.flat)) and (self.bbuf is None or torch.equal(bits(self.bbuf), bits(other.bbuf)))


@pytest.mark.parametrize('N,K,form,loader', TN_OPERANDS)
def test_tn_token_sweep(ops, cuda, pairs, N, K, form, loader):
    """Every M of TN_MS (the plans: module docstring) in one operand form, dense dW, with the bias gradient = the exact column sums of dY."""
    fails = []
    for M in TN_MS:
        dY, X, want_w, want_b = _tn_operands(pairs, cuda, M, N, K, form)
        assert _tn_loader(dY, X) == loader
        o = TnOut(cuda, N, K, 'dense', True, False)
        ops.gemm_tn(ops.F32X3, dY, X, o.w.v, bias_grad=o.db)
        o.check(want_w, want_b, f'M={M} ({N}, {K}) operands {form}', fails)
    _report(fails)


@pytest.mark.parametrize('N,K,form,loader', [(264, 136, 'ld8', RVEC), (264, 136, 'ld3', ANY), (70, 50, 'dense', ANY)])
@pytest.mark.parametrize('M', [65, 513, 1793])
def test_tn_output_forms_accumulate_bias_three_calls(ops, cuda, pairs, M, N, K, form, loader):
    """One slice of 3 k-slices (65), two slices of 9 k-slices (513) and seven with a short last one (1793), into every output form, accumulate off / on,
    bias_grad on / off; three calls give the same bits."""
    dY, X, want_w, want_b = _tn_operands(pairs, cuda, M, N, K, form)
    assert _tn_loader(dY, X) == loader
    fails = []
    for oform in TN_FORMS:
        for accumulate in (False, True):
            for bias in (True, False):
                outs = []
                for _ in range(3):
                    o = TnOut(cuda, N, K, oform, bias, accumulate)
                    ops.gemm_tn(ops.F32X3, dY, X, o.w.v, bias_grad=o.db, accumulate=accumulate)
                    outs.append(o)
                what = f'M={M} ({N}, {K}) operands {form} -> {oform} accumulate={accumulate} bias={bias}'
                outs[0].check(want_w, want_b, what, fails)
                if not (outs[1].same_bits(outs[0]) and outs[2].same_bits(outs[0])):
                    fails.append(f'{what}: three calls, different bits')
    _report(fails)


def test_tn_grouped_is_the_loop_of_single_calls(ops, cuda, pairs):
    """ops.gemm_tn_grouped(F32X3) runs as a library-side loop: two problems (LD_RVEC, two slices; LD_ANY, one slice, accumulate, no bias_grad) give the
    bits of the one-by-one calls, and the exact result."""
    specs = [(513, 264, 136, 'ld8', RVEC, 'ld8', True, False), (65, 70, 50, 'dense', ANY, 'ld3', False, True)]
    fails, group, single, wants = [], [], [], []
    for M, N, K, form, loader, oform, bias, accumulate in specs:
        dY, X, want_w, want_b = _tn_operands(pairs, cuda, M, N, K, form)
        assert _tn_loader(dY, X) == loader
        g, s = TnOut(cuda, N, K, oform, bias, accumulate), TnOut(cuda, N, K, oform, bias, accumulate)
        group.append((dY, X, g.w.v, g.db, int(accumulate)))
        ops.gemm_tn(ops.F32X3, dY, X, s.w.v, bias_grad=s.db, accumulate=accumulate)
        single.append(s); wants.append((g, want_w, want_b))
    ops.gemm_tn_grouped(ops.F32X3, group)
    for i, ((g, want_w, want_b), s) in enumerate(zip(wants, single)):
        g.check(want_w, want_b, f'grouped problem {i}', fails)
        if not g.same_bits(s):
            fails.append(f'grouped problem {i}: not the bits of the single call')
    _report(fails)


# ---- batched form.  An operand form is (storage, pad, base offset) of _stored: 'k' = contraction index contiguous, 'r' = row index contiguous.
K8, R8, R0, K0, K3, KOFF, ROFF = ('k', 8, 0), ('r', 8, 0), ('r', 0, 0), ('k', 0, 0), ('k', 3, 0), ('k', 8, 1), ('r', 8, 1)
# name -> (A form, B form, (A loader, B loader) of x3_loader, kernel launched, [(M, N, K)]).  A is [M, K]; B's form is that of its [N, K] view, so 'k' is
# "B passed as W.t()" and 'r' the plain row-major B [K, N].
BATCH_CASES = {
    # A row-major, B = W.t(): dWfc = dW' Wproj^T
    'kvec_kvec': (K8, K8, (KVEC, KVEC), (KVEC, KVEC), [(129, 132, 32), (257, 129, 64), (4, 1, 4), (132, 257, 96), (1, 4, 64)]),
    # the plain product A B with N % 4 == 0: the fold's W' = Wfc Wproj
    'kvec_rvec': (K8, R8, (KVEC, RVEC), (KVEC, RVEC), [(129, 132, 32), (257, 4, 96), (1, 132, 4), (132, 132, 64)]),
    # A.t() with M % 4 == 0 times a plain B: dWproj = Wfc^T dW'.  Any K: K = 1, 31, 33, 65 mask a ragged last slice in LD_RVEC
    'rvec_rvec': (R8, R8, (RVEC, RVEC), (RVEC, RVEC), [(132, 132, 1), (132, 132, 31), (132, 132, 33), (132, 132, 65), (4, 132, 32), (132, 4, 96), (4, 4, 4)]),
    # A.t() times a column vector: the GEMV db_proj = Wfc^T db' (B [K, 1] with strides (1, 1): no loader's condition holds)
    'rvec_any_gemv': (R8, R0, (RVEC, ANY), (RVEC, ANY), [(132, 1, 4), (132, 1, 31), (132, 1, 32), (132, 1, 33), (132, 1, 65), (132, 1, 96), (4, 1, 64)]),
    # b' = Wfc b_proj: A row-major times a column vector
    'kvec_any_gemv': (K8, R0, (KVEC, ANY), (ANY, ANY), [(129, 1, 32), (132, 1, 96)]),
    # the flags head (engine.py run_backward): dWf = df^T mean(features), df.t() [3, BT] with k stride 3; dmean = df Wf with K = 3
    'flags_dw': (R0, R0, (ANY, RVEC), (ANY, ANY), [(3, 132, 33), (3, 132, 64)]),
    'flags_dmean': (K0, R0, (ANY, RVEC), (ANY, ANY), [(65, 132, 3), (129, 4, 3)]),
    # K = 1 rank-1 updates u v^T (run with accumulate only: dWfc's bias term); v [1, N] is LD_RVEC-shaped at N % 4 == 0
    'rank1': (K0, R0, (ANY, RVEC), (ANY, ANY), [(129, 132, 1), (257, 4, 1), (1, 132, 1)]),
    'rank1_odd': (K0, R0, (ANY, ANY), (ANY, ANY), [(132, 129, 1), (4, 257, 1), (1, 1, 1)]),
    # pairs that have no kernel of their own
    'kvec_any': (K8, K3, (KVEC, ANY), (ANY, ANY), [(129, 129, 32), (4, 257, 64)]),
    'any_kvec': (K3, K8, (ANY, KVEC), (ANY, ANY), [(129, 132, 64), (257, 1, 4)]),
    'rvec_kvec': (R8, K8, (RVEC, KVEC), (ANY, ANY), [(132, 129, 32), (4, 257, 96)]),
    # unaligned bases
    'unaligned': (KOFF, ROFF, (ANY, ANY), (ANY, ANY), [(129, 132, 33), (257, 257, 65), (1, 4, 31), (132, 132, 32)]),
}
CFORMS = {'dense': (lambda N: N, 0), 'ld3': (lambda N: N + 3, 0), 'off1': (lambda N: (N + 3) // 4 * 4 + 8, 1)}


def _batch_problem(pairs, dev, M, N, K, af, bf, cform, accumulate, tag=0):
    """((A, B, C) of ops.sgemm_batched, the guarded output, the f64 reference)."""
    A, Bt, want = _pair(pairs, dev, M, N, K, tag)
    pre = _ints(dev, M * 4099 + N + tag, (M, N), -3, 3) if accumulate else None
    ld, off = CFORMS[cform]
    out = Out(dev, M, N, ld(N), off, pre)
    return (_stored(A, *af), _stored(Bt, *bf).t(), out.v), out, (want + pre if accumulate else want)


@pytest.mark.parametrize('name', list(BATCH_CASES))
def test_batched_every_branch_one_problem_per_call(ops, cuda, pairs, name):
    """BATCH_CASES: each shape into C dense, at ldc = N + 3 and one float off alignment, overwriting and accumulating onto small integers."""
    af, bf, loaders, launched, shapes = BATCH_CASES[name]
    fails = []
    for M, N, K in shapes:
        for cform in CFORMS:
            for accumulate in ((True,) if name.startswith('rank1') else (False, True)):
                prob, out, want = _batch_problem(pairs, cuda, M, N, K, af, bf, cform, accumulate)
                assert _batch_loaders([prob]) == (loaders, launched), (name, M, N, K, _batch_loaders([prob]))
                ops.sgemm_batched([prob], accumulate=accumulate)
                _check(out, want, f'{name} ({M}, {N}, {K}) -> {cform} accumulate={accumulate}', fails)
    _report(fails)


def _run_batch(ops, dev, pairs, specs, loaders, launched, accumulate=False):
    """One call of several problems: specs = [(M, N, K, A form, B form, C form)]; every output is checked and guarded."""
    built = [_batch_problem(pairs, dev, M, N, K, af, bf, cform, accumulate, tag=i) for i, (M, N, K, af, bf, cform) in enumerate(specs)]
    probs = [b[0] for b in built]
    assert _batch_loaders(probs) == (loaders, launched), _batch_loaders(probs)
    ops.sgemm_batched(probs, accumulate=accumulate)
    fails = []
    for i, ((_, out, want), spec) in enumerate(zip(built, specs)):
        _check(out, want, f'problem {i} {spec[:3]} accumulate={accumulate}', fails)
    return probs, fails


def test_batched_loader_demotion_across_problems(ops, cuda, pairs):
    """Problems that disagree on a loader: the operand goes to LD_ANY for all of them.
    1. B is LD_RVEC in problem 0 (N = 132) and LD_ANY in problem 1 (N = 129): (RVEC, RVEC) alone becomes the (RVEC, ANY) kernel, which loads problem
       0's B with 4-byte loads.  2. the same the other way round (the demotion does not depend on the order).
    3. A is LD_KVEC and LD_ANY (pitch K + 3): (ANY, KVEC) has no kernel, everything falls through to (ANY, ANY)."""
    fails = []
    two = [(132, 132, 33, R8, R8, 'dense'), (132, 129, 33, R8, R0, 'ld3')]
    probs, f = _run_batch(ops, cuda, pairs, two, (RVEC, ANY), (RVEC, ANY))
    assert _batch_loaders(probs[:1]) == ((RVEC, RVEC), (RVEC, RVEC))
    fails += f
    fails += _run_batch(ops, cuda, pairs, two[::-1], (RVEC, ANY), (RVEC, ANY), accumulate=True)[1]
    fails += _run_batch(ops, cuda, pairs, [(129, 132, 32, K8, K8, 'dense'), (129, 132, 32, K3, K8, 'off1'), (4, 4, 64, K8, K8, 'dense')], (ANY, KVEC), (ANY, ANY))[1]
    _report(fails)


def test_batched_mixed_sizes_idle_workgroups_return(ops, cuda, pairs):
    """(4, 4, 32) next to (257, 130, 65): the grid has 3 x 2 = 6 tiles per problem, five workgroups of the small problem return at once and write
    nothing (its output is guarded like every other).  Both orders; the pair of vector-loader problems (4, 4, 32) / (132, 260, 65) stays on
    (RVEC, RVEC) with 2 x 3 tiles against one."""
    fails = []
    mixed = [(4, 4, 32, K8, K8, 'ld3'), (257, 130, 65, K8, K8, 'ld3')]
    for specs in (mixed, mixed[::-1]):
        for accumulate in (False, True):
            fails += _run_batch(ops, cuda, pairs, specs, (ANY, ANY), (ANY, ANY), accumulate)[1]
    fails += _run_batch(ops, cuda, pairs, [(4, 4, 32, R8, R8, 'dense'), (132, 260, 65, R8, R8, 'ld3'), (4, 4, 32, R8, R8, 'off1')], (RVEC, RVEC), (RVEC, RVEC))[1]
    _report(fails)


def test_batched_24_problems(ops, cuda, pairs):
    """The most one call takes, all (KVEC, KVEC), sizes from one tile of one element to 2 x 2 tiles, K = 4, 32, 64, 96, the three C forms in turn."""
    sizes = [(1, 4), (4, 4), (129, 1), (4, 132), (132, 129), (129, 132)]
    specs = [sizes[i % 6] + ((4, 32, 64, 96)[i % 4], K8, K8, list(CFORMS)[i % 3]) for i in range(24)]
    fails = _run_batch(ops, cuda, pairs, specs, (KVEC, KVEC), (KVEC, KVEC))[1]
    fails += _run_batch(ops, cuda, pairs, specs, (KVEC, KVEC), (KVEC, KVEC), accumulate=True)[1]
    _report(fails)


def test_batched_refusals_launch_nothing(ops, cuda, pairs):
    """n = 0, n = 25, a null table or operand, M, N or K = 0 and ldc < N return before any launch: TcowError, and every output of the call keeps its NaN."""
    from tcow_amd import _lib as L
    lib = L.lib()

    def call(n, rows, table=True):
        arr = (L.SGemm * max(len(rows), 1))()
        for i, r in enumerate(rows):
            arr[i] = L.SGemm(*r)
        L.check(lib.tcow_sgemm_x3_batched(ops._stream(), n, arr if table else None), 'tcow_sgemm_x3_batched')

    M, N, K = 4, 132, 32
    built = [_batch_problem(pairs, cuda, M, N, K, K8, K8, 'ld3', False, tag=i % 2) for i in range(25)]
    outs = [b[1] for b in built]

    def row(i, **kw):
        A, B, C = built[i][0]
        f = dict(M=M, N=N, K=K, A=A.data_ptr(), sai=A.stride(0), sak=A.stride(1), B=B.data_ptr(), sbj=B.stride(1), sbk=B.stride(0), C=C.data_ptr(), ldc=C.stride(0), accumulate=0)
        f.update(kw)
        return tuple(f[k] for k in ('M', 'N', 'K', 'A', 'sai', 'sak', 'B', 'sbj', 'sbk', 'C', 'ldc', 'accumulate'))

    refused = [('n = 0', 0, [row(0)], True), ('n = 25', 25, [row(i) for i in range(25)], True), ('null table', 1, [row(0)], False),
               ('A = NULL', 2, [row(0), row(1, A=None)], True), ('B = NULL', 1, [row(0, B=None)], True), ('C = NULL', 2, [row(0), row(1, C=None)], True),
               ('M = 0', 2, [row(0), row(1, M=0)], True), ('N = 0', 1, [row(0, N=0)], True), ('K = 0', 3, [row(0), row(1), row(2, K=0)], True),
               ('ldc < N', 2, [row(0), row(1, ldc=N - 1)], True)]
    for what, n, rows, table in refused:
        with pytest.raises(L.TcowError, match='tcow_sgemm_x3_batched'):
            call(n, rows, table)
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs), f'{what}: a refused call wrote to an output'
    call(24, [row(i) for i in range(24)])                                  # the accepted call these are variations of
    fails = []
    for i in range(24):
        _check(outs[i], built[i][2], f'accepted problem {i}', fails)
    _report(fails)
    assert outs[24].untouched()

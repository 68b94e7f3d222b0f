"""Attention (tcow_attn_{temporal,spatial}_{fwd,bwd}) in the four modes against a float64 reference, at the shapes, masks and score scales
where a flash-attention kernel goes wrong: the lazy running maximum's rescale (ramp, shift, planted), the saved log-sum-exp (an ABI output the
backward consumes), mask / padding / half last tile (uniform), sequence / head / slot-0 addressing (addressing), and every kernel instantiation
the dispatch in attention_api.hip, tcow_attn_mfma_fwd/_bwd, tcow_attn_x3_* and tcow_attn_f32_* can launch (the shape matrix below).

Storage rounding points of the modes: f32 / f32x3 store f32 (u = 2^-24); bf16 stores 8 significand bits (u = 2^-8), fp16 11 (u = 2^-11).
Arithmetic: f32 = exact-f32 products; f32x3 = bf16 x 3 split products (~2^-16 per product); 16-bit = bf16 / fp16 operands with f32
accumulation, P rounded to 16 bits before P V, and (streaming forward without a mask) Q pre-scaled by 0.125 log2(e) and rounded to 16 bits once."""
import math

import pytest
import torch

BIG = 1 << 28
MODES = ['f32', 'f32x3', 'bf16', 'fp16']
U_STORE = {'f32': 2.0 ** -24, 'f32x3': 2.0 ** -24, 'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11}
# test_attention_fwd_bwd's tolerances (max |d| relative to max |ref|; backward 1.5 x)
TOL = {'f32': 2e-5, 'f32x3': 6e-5, 'bf16': 1.5e-2, 'fp16': 2e-3}
# relative rounding of an operand of the P V / dS products: f32 none beyond accumulation, f32x3 the dropped lo x lo (2^-16, twice), 16-bit u
U_OP = {'f32': 2.0 ** -22, 'f32x3': 2.0 ** -15, 'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11}


def _dtype(mname):
    return {'f32': torch.float32, 'f32x3': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}[mname]


def seq_rows(B, T, S, spatial, ca):
    """The header's sequences: rows[i, p] = token row of position p of sequence i, and the mask diagonal (key allowed iff key <= query + diag)."""
    if spatial:
        s0 = 0 if ca in (0, 1) else 1                                           # cls takes part iff causal in {0, 1}
        rows = torch.arange(B * T)[:, None] * S + s0 + torch.arange(S - s0)[None]
        return rows, BIG
    b, s, t = torch.arange(B)[:, None, None], torch.arange(1, S)[None, :, None], torch.arange(T)[None, None, :]
    rows = (b * T * S + t * S + s).reshape(B * (S - 1), T)
    return rows, (BIG if ca <= 0 else (0 if ca <= 2 else ca - 2))


SC32 = torch.tensor(0.125, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)   # the kernels' kScale * kLog2e (f32)


def _scores(q, k, model):
    """float64 scores (nats) of q [G, Lq, 64] against k [G, L, 64] under a model of the kernel's score arithmetic:
      'exact': q.k / 8;
      'x3'   : the split-bf16 products of attention_x3.hip -- x = hi + lo, hi = bf16(x), lo = bf16(x - hi) (both round to nearest), and
               q.k ~ qh.kh + qh.kl + ql.kh (the lo x lo product and the residuals x - hi - lo are dropped);
      a torch 16-bit dtype: the 16-bit streaming forward without a mask -- q multiplied by 0.125 log2(e) in f32 and rounded to that dtype once,
               exp2 of k.q', i.e. ln(2) k.q' nats."""
    if model == 'exact':
        return (q @ k.transpose(1, 2)) * 0.125
    if model == 'x3':
        def split(x):
            x = x.float(); h = x.bfloat16().float()
            return h.double(), (x - h).bfloat16().double()
        qh, ql = split(q); kh, kl = split(k)
        return (qh @ kh.transpose(1, 2) + qh @ kl.transpose(1, 2) + ql @ kh.transpose(1, 2)) * 0.125
    qp = (q.float() * SC32.to(q.device)).to(model).double()
    return (qp @ k.transpose(1, 2)) * math.log(2.0)


def attn_ref64(qkv, B, T, S, heads, ca, spatial, dout=None, fwd_model='exact', bwd_model='exact'):
    """float64 reference on the values the kernel received (qkv / dout as stored), with the scores of fwd_model / bwd_model (_scores: 'exact'
    by default).  The forward's softmax uses fwd_model; the backward recomputes P = exp(s_bwd - lse) from bwd_model's scores and the forward's
    lse, as the kernels do (when the two models differ, P's rows do not sum to 1 -- the kernels' arithmetic, reproduced).  Returns out [M, D], lse [M, heads] (NaN on rows of no
    sequence), valid [M] and, given dout, dqkv [M, 3D] by the closed-form backward dV = P^T dO, dS = P o (dO V^T - rowsum(dO o O)),
    dQ = dS K / 8, dK = dS^T Q / 8, and magnitudes: dqkv_abs = (|dS| |K| / 8, |dS|^T |Q| / 8, P^T |dO|) -- a relative error e of the
    probabilities moves dq, dk, dv by at most 2e times these; dqkv_mag = the same with G = P o (|dO| |V|^T + |delta|) for |dS| -- what a
    relative error of the products in dP - delta can move; dqkv_delta = 4 (c |P K| / 8, sqrt((P o c)^2^T Q^2) / 8, 0), c = |dO o O|_2 --
    four standard deviations of what independent relative roundings of the stored O move dq by (delta = rowsum(dO o O) is formed from it: one
    error per query, shared by its keys) and dk by (independent across queries); dqkv_rms = the products of the squares (|dS|, P), square-rooted -- independent
    relative roundings of size e of the terms move each sum by about e times these.  Queries go in chunks: no intermediate holds more than 2^24 elements (128 MiB)."""
    M, D, dev = qkv.shape[0], heads * 64, qkv.device
    rows, diag = seq_rows(B, T, S, spatial, ca)
    rows = rows.to(dev)
    N, L = rows.shape
    G = N * heads
    x = qkv.double().view(M, 3, heads, 64)[rows]                                # [N, L, 3, H, 64]
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3).reshape(G, L, 64) for i in range(3))
    del x
    pos = torch.arange(L, device=dev)
    keep = pos[None, :] <= pos[:, None] + diag
    out = torch.empty(G, L, 64, dtype=torch.float64, device=dev); lse = torch.empty(G, L, dtype=torch.float64, device=dev)
    prms = torch.empty(G, L, dtype=torch.float64, device=dev)
    if dout is not None:
        do = dout.double().view(M, heads, 64)[rows].permute(0, 2, 1, 3).reshape(G, L, 64)
        dq = torch.empty_like(out); dk = torch.zeros_like(out); dv = torch.zeros_like(out)
        mq = torch.empty_like(out); mk = torch.zeros_like(out); mv = torch.zeros_like(out)
        rq = torch.empty_like(out); rk = torch.zeros_like(out); rv = torch.zeros_like(out)
        aq = torch.empty_like(out); ak = torch.zeros_like(out); eq = torch.empty_like(out); ek = torch.zeros_like(out)
    budget = 1 << 24
    gc = max(1, min(G, budget // (L * L)))
    qc = L if gc > 1 else max(1, min(L, budget // L))
    for g0 in range(0, G, gc):
        g = slice(g0, g0 + gc)
        for q0 in range(0, L, qc):
            r = slice(q0, q0 + qc)
            s = _scores(q[g, r], k[g], fwd_model).masked_fill(~keep[r], float('-inf'))
            ls = torch.logsumexp(s, -1)
            p = torch.exp(s - ls[..., None])
            del s
            o = p @ v[g]
            out[g, r] = o; lse[g, r] = ls; prms[g, r] = p.square().sum(-1).sqrt()
            if dout is not None:
                if bwd_model != fwd_model:
                    p = torch.exp(_scores(q[g, r], k[g], bwd_model).masked_fill(~keep[r], float('-inf')) - ls[..., None])
                dO = do[g, r]
                dv[g] += p.transpose(1, 2) @ dO
                delta = (dO * o).sum(-1, keepdim=True)
                ds = p * (dO @ v[g].transpose(1, 2) - delta)
                mv[g] += p.transpose(1, 2) @ dO.abs()
                rv[g] += p.square().transpose(1, 2) @ dO.square()
                dq[g, r] = (ds @ k[g]) * 0.125
                dk[g] += (ds.transpose(1, 2) @ q[g, r]) * 0.125
                aq[g, r] = (ds.abs() @ k[g].abs()) * 0.125
                cd = (dO * o).square().sum(-1, keepdim=True).sqrt()                     # relative roundings <= e of O move delta by ~e times this
                eq[g, r] = 4 * cd * (p @ k[g]).abs() * 0.125                                 # (one error per query, shared by its keys)
                ek[g] += ((p * cd).square().transpose(1, 2) @ q[g, r].square()) / 64      # (independent errors across queries: squares)
                del cd
                ak[g] += (ds.abs().transpose(1, 2) @ q[g, r].abs()) * 0.125
                rq[g, r] = (ds.square() @ k[g].square()) / 64
                rk[g] += (ds.square().transpose(1, 2) @ q[g, r].square()) / 64
                ds = p * (dO.abs() @ v[g].abs().transpose(1, 2) + delta.abs())          # G >= |dS|: bounds the rounding of dP - delta
                del p
                mq[g, r] = (ds @ k[g].abs()) * 0.125
                mk[g] += (ds.transpose(1, 2) @ q[g, r].abs()) * 0.125
    res = {'valid': torch.zeros(M, dtype=torch.bool, device=dev)}
    res['valid'][rows.reshape(-1)] = True
    o_full = torch.zeros(M, heads, 64, dtype=torch.float64, device=dev)
    o_full[rows] = out.view(N, heads, L, 64).permute(0, 2, 1, 3)
    l_full = torch.full((M, heads), float('nan'), dtype=torch.float64, device=dev)
    l_full[rows] = lse.view(N, heads, L).permute(0, 2, 1)
    res['out'], res['lse'] = o_full.reshape(M, D), l_full
    r_full = torch.zeros(M, heads, dtype=torch.float64, device=dev)
    r_full[rows] = prms.view(N, heads, L).permute(0, 2, 1)
    res['prms'] = r_full                                                         # sqrt(sum_j p_j^2) per (row, head)
    if dout is not None:
        d_full = torch.zeros(M, 3, heads, 64, dtype=torch.float64, device=dev)
        for i, t in enumerate((dq, dk, dv)):
            d_full[rows, i] = t.view(N, heads, L, 64).permute(0, 2, 1, 3)
        res['dqkv'] = d_full.reshape(M, 3 * D)
        m_full = torch.zeros(M, 3, heads, 64, dtype=torch.float64, device=dev)
        for i, t in enumerate((mq, mk, mv)):
            m_full[rows, i] = t.view(N, heads, L, 64).permute(0, 2, 1, 3)
        res['dqkv_mag'] = m_full.reshape(M, 3 * D)
        m_full = torch.zeros(M, 3, heads, 64, dtype=torch.float64, device=dev)
        for i, t in enumerate((eq, 4 * ek.sqrt(), torch.zeros_like(mv))):
            m_full[rows, i] = t.view(N, heads, L, 64).permute(0, 2, 1, 3)
        res['dqkv_delta'] = m_full.reshape(M, 3 * D)
        m_full = torch.zeros(M, 3, heads, 64, dtype=torch.float64, device=dev)
        for i, t in enumerate((aq, ak, mv)):
            m_full[rows, i] = t.view(N, heads, L, 64).permute(0, 2, 1, 3)
        res['dqkv_abs'] = m_full.reshape(M, 3 * D)
        m_full = torch.zeros(M, 3, heads, 64, dtype=torch.float64, device=dev)
        for i, t in enumerate((rq, rk, rv)):
            m_full[rows, i] = t.sqrt().view(N, heads, L, 64).permute(0, 2, 1, 3)
        res['dqkv_rms'] = m_full.reshape(M, 3 * D)
    return res


# ---------------------------------------------------------------------------------------------------- the reference itself (CPU)
@pytest.mark.parametrize('spatial,B,T,S,heads,ca', [
    (False, 2, 5, 4, 2, 1), (False, 1, 6, 3, 2, 2), (False, 1, 6, 3, 1, 3), (False, 1, 7, 3, 2, 5), (False, 2, 4, 3, 1, 0), (False, 1, 5, 3, 2, -1),
    (True, 2, 2, 6, 2, 1), (True, 1, 2, 7, 2, 0), (True, 1, 3, 5, 2, 2), (True, 1, 2, 6, 1, -1)])
def test_attn_ref64_against_autograd(spatial, B, T, S, heads, ca):
    """attn_ref64 (chunked, closed-form backward) == test_gpu_kernels._ref_attn's formulation through torch.autograd, every mask kind; lse == the
    log-sum-exp of that formulation's masked scores.  Runs on the CPU: the reference is tested where the GPU tests are written."""
    from test_gpu_kernels import _ref_attn
    g = torch.Generator().manual_seed(B * 100 + T * 10 + S + ca)
    D = heads * 64; M = B * T * S
    qkv = torch.randn(M, 3 * D, generator=g) * 2
    dout = torch.randn(M, D, generator=g)
    x = qkv.clone().requires_grad_(True)
    ref = _ref_attn(x, B, T, S, D, heads, ca, spatial)
    (ref * dout).sum().backward()
    got = attn_ref64(qkv, B, T, S, heads, ca, spatial, dout)
    assert float((got['out'] - ref.detach().double()).abs().max()) < 1e-5
    assert float((got['dqkv'] - x.grad.double()).abs().max()) < 1e-4
    xs = qkv.double().reshape(B, T, S, 3, heads, 64)
    if spatial:
        s0 = 0 if ca in (0, 1) else 1
        qq, kk = xs[:, :, s0:, 0].permute(0, 1, 3, 2, 4), xs[:, :, s0:, 1].permute(0, 1, 3, 2, 4)
        want = torch.logsumexp(qq @ kk.transpose(-1, -2) / 8, -1).permute(0, 1, 3, 2)                   # [B, T, S - s0, H]
        got_l = got['lse'].reshape(B, T, S, heads)[:, :, s0:]
        assert torch.isnan(got['lse'].reshape(B, T, S, heads)[:, :, :s0]).all()
    else:
        qq, kk = xs[:, :, 1:, 0].permute(0, 2, 3, 1, 4), xs[:, :, 1:, 1].permute(0, 2, 3, 1, 4)
        a = qq @ kk.transpose(-1, -2) / 8
        if ca > 0:
            a = a.masked_fill(~torch.ones(T, T, dtype=torch.bool).tril(0 if ca <= 2 else ca - 2), float('-inf'))
        want = torch.logsumexp(a, -1).permute(0, 3, 1, 2)                                                # [B, T, S - 1, H]
        got_l = got['lse'].reshape(B, T, S, heads)[:, :, 1:]
        assert torch.isnan(got['lse'].reshape(B, T, S, heads)[:, :, 0]).all()
    assert float((got_l - want).abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------------------- shape matrix (GPU)
# (id, spatial, B, T, S, heads, causal).  Kernels: 16-bit (bf16 / fp16 builds) forward / backward | f32x3 | f32.  nt = 32-position tiles.
MATRIX = [
    # temporal, nt = 1: attn_fwd_mfma (zeroes slot 0 itself) / attn_bwd_one_tile | attn_x3_fwd<1,true> / attn_x3_bwd_dq,dkv<1,true> | attn_f32_fwd_solo / attn_f32_bwd_solo
    ('t30_bench', False, 3, 30, 301, 12, 1),
    # temporal, nt = 2 (wave-private): attn_fwd_mfma / attn_bwd_prep_kernel + attn_bwd_dkv_mfma + attn_bwd_dq_mfma + zero_rows_kernel
    #   | attn_x3_fwd<2> / attn_x3_bwd_dq,dkv<4> | attn_f32_fwd / attn_f32_bwd_dq,dkv;  no mask (ca <= 0) included
    ('t60_c1', False, 1, 60, 5, 2, 1), ('t60_c0', False, 1, 60, 5, 2, 0), ('t60_cm1', False, 1, 60, 5, 2, -1),
    ('t33_c3', False, 1, 33, 4, 3, 3),                     # look-ahead 1: one valid key in tile 2
    # temporal, nt = 3 streaming: masked -> attn_fwd_stream<4>, unmasked -> attn_fwd_stream_nc<4,false> on strided sequences; attn_bwd_dq,dkv_stream<4>
    ('t70_c1', False, 2, 70, 3, 2, 1), ('t70_c4', False, 2, 70, 3, 2, 4), ('t70_c0', False, 2, 70, 3, 2, 0),
    ('t150_c1', False, 1, 150, 3, 2, 1),                   # nt = 5: attn_bwd_dq,dkv_stream<5> (stream_ch5)
    # nt = 6, no mask: attn_fwd_stream_nc<4,true> (mixed workgroups) on strided sequences, 3 / 9 / 17 (sequence, head) pairs
    ('t180_p3', False, 3, 180, 2, 1, 0), ('t180_p9', False, 3, 180, 2, 3, 0), ('t180_p17', False, 17, 180, 2, 1, 0),
    # spatial S = 301 (nt = 10): attn_fwd_stream_nc<4,true> / attn_bwd_one_kernel | attn_x3_fwd<2> / attn_x3_bwd<4> | attn_f32_fwd / attn_f32_bwd
    ('s301_bench', True, 3, 30, 301, 12, 1), ('s301_c2', True, 1, 3, 301, 2, 2), ('s301_cm1', True, 1, 3, 301, 2, -1),
    ('s33_c1', True, 2, 3, 33, 3, 1),                      # L = 33, nt = 2: attn_fwd_stream_nc<4,true> / attn_bwd_dq,dkv_stream<4>
    ('s33_c2', True, 2, 3, 33, 3, 2),                      # L = 32, nt = 1 shared: attn_fwd_stream<4> / stream<4> | x3 SOLO | f32 solo; zero_rows_kernel
    ('s321_c2', True, 1, 2, 321, 2, 2),                    # L = 320: the one-kernel backward's last length
    ('s322_c2', True, 1, 2, 322, 2, 2),                    # L = 321, nt = 11: attn_fwd_stream_nc<4,false> / attn_bwd_dq,dkv_stream<4>
    ('s1201_c1', True, 1, 1, 1201, 12, 1),                 # L = 1201: last tile of 17 keys; nt = 38 -> nc<4,true>, stream<5>
    ('s1201_c2', True, 1, 1, 1201, 12, 2),                 # L = 1200: half last tile of exactly 16
    # joint space-time (T = 1, causal 0): 1 + 30 * 48 and 9001 tokens: nc<4,true> / stream<5> | x3 two-tile chunks | f32 tiled
    ('j1441', True, 1, 1, 1441, 12, 0), ('j9001', True, 1, 1, 9001, 1, 0),
]
BY_ID = {m[0]: m[1:] for m in MATRIX}
# one row per dispatch branch for the float64-reference families
BRANCHES = ['t30_bench', 't60_c0', 't33_c3', 't70_c4', 't70_c0', 't150_c1', 't180_p9', 's301_c2', 's33_c1', 's33_c2', 's322_c2', 's1201_c2', 'j9001']


@pytest.fixture(scope='module')
def ops(cuda):
    from tcow_amd import ops as o
    return o


class Case:
    """One (mode, shape): layout, launches, and the failure report that names the worst (row, head, channel) and its sequence."""

    def __init__(self, ops, cuda, mname, sid):
        self.ops, self.dev, self.mname, self.sid = ops, cuda, mname, sid
        self.spatial, self.B, self.T, self.S, self.H, self.ca = BY_ID[sid]
        self.dt = _dtype(mname)
        mode = {'f32': ops.F32, 'f32x3': ops.F32X3, 'bf16': ops.BF16, 'fp16': ops.FP16}[mname]
        self.M, self.D = self.B * self.T * self.S, self.H * 64
        self.shape = ops.attn_shape(mode, self.B, self.T, self.S, self.D, self.H, self.ca)
        rows, self.diag = seq_rows(self.B, self.T, self.S, self.spatial, self.ca)
        self.rows = rows.to(cuda)
        self.N, self.L = rows.shape
        self.nt = (self.L + 31) // 32
        self.seq_of = torch.full((self.M,), -1, dtype=torch.long, device=cuda); self.seq_of[self.rows] = torch.arange(self.N, device=cuda)[:, None]
        self.pos_of = torch.full((self.M,), -1, dtype=torch.long, device=cuda); self.pos_of[self.rows] = torch.arange(self.L, device=cuda)[None]
        self.valid = self.seq_of >= 0
        self.nvis = (torch.clamp(self.pos_of + self.diag + 1, max=self.L)).clamp(min=1).double()   # keys a row's query sees

    def fwd(self, qkv, with_lse=True):
        out = torch.full((self.M, self.D), float('nan'), device=self.dev, dtype=self.dt)
        lse = torch.full((self.M, self.H), float('nan'), device=self.dev) if with_lse else None
        self.ops.attn_fwd(self.shape, self.spatial, qkv, out, lse)
        return out, lse

    def bwd(self, qkv, out, dout, lse):
        dqkv = torch.full((self.M, 3 * self.D), float('nan'), device=self.dev, dtype=self.dt)
        self.ops.attn_bwd(self.shape, self.spatial, qkv, out, dout, lse, dqkv)
        return dqkv

    def check(self, what, got, want, tol):
        """Asserts |got - want| <= tol elementwise (a NaN in got fails) on [M, ...] tensors laid out as the ABI's rows: [M, 3D] (dqkv), [M, D]
        (out) or [M, heads] (lse).  The failure names the worst (row, head, channel) and the sequence and position of that row."""
        g = got.double().reshape(self.M, -1); w = want.double().reshape(self.M, -1)
        t = torch.as_tensor(tol, dtype=torch.float64, device=self.dev)
        t = t.reshape(self.M, -1) if t.dim() else t
        d = (g - w).abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, float('inf')), d)
        excess = d - t
        worst = int(excess.argmax())
        if float(excess.view(-1)[worst]) <= 0:
            return float(d.max())
        X = g.shape[1]
        r, col = divmod(worst, X)
        if X == 3 * self.D:
            sec, rem = divmod(col, self.D); h, ch = divmod(rem, 64); part = ' ' + 'qkv'[sec]
        elif X == self.D:
            (h, ch), part = divmod(col, 64), ''
        else:
            h, ch, part = col, '-', ''
        seq, p = int(self.seq_of[r]), int(self.pos_of[r])
        where = f'sequence {seq} position {p}' if seq >= 0 else 'a row of no sequence'
        tv = float(t.reshape(-1)[worst]) if t.dim() else float(t)
        pytest.fail(f'{self.mname} {self.sid}: {what}{part}: worst at row {r} head {h} channel {ch} ({where}; L={self.L}, causal={self.ca}): '
                    f'got {float(g[r, col])!r}, want {float(w[r, col])!r}, |d| {float(d.view(-1)[worst]):.3e} > tol {tv:.3e}')


def rel_max(got, want, mask):
    g, w = got.double()[mask], want.double()[mask]
    return float((g - w).abs().max() / (w.abs().max() + 1e-300))


def _per_head(c, x):
    return x.view(c.M, c.H, 64)


# ---------------------------------------------------------------------------------------------------- uniform and addressing (closed form)
@pytest.mark.gpu
@pytest.mark.parametrize('sid', [m[0] for m in MATRIX])
@pytest.mark.parametrize('mname', MODES)
def test_attn_uniform_masks_and_lse(ops, cuda, mname, sid):
    """q = 0: every visible probability is exp2(0) = 1 exactly, so lse = ln(n_visible) to f32 rounding (0 exactly for a query that sees only key 0)
    in every mode, and with v = one-hot of the key position (L <= 64) or key tile mod 64 (longer) out is (#visible keys per channel) / n_visible:
    the counts are exact in any accumulator, so the only roundings are 1/l (f32) and the store (one storage ulp), and every channel without a
    visible key is exactly 0.0.  Pins causal / look-ahead masks, last-tile padding (padding rows load key L-1's data), the half last tile, and slot-0
    rows (zero).  The inference call (lse = None) must give a bit-identical output."""
    c = Case(ops, cuda, mname, sid)
    g = torch.Generator(device=cuda).manual_seed(7)
    qkv = torch.randn(c.M, 3, c.H, 64, device=cuda, generator=g)
    qkv[:, 0] = 0.0
    key_code = torch.where(c.pos_of < 0, torch.zeros_like(c.pos_of), c.pos_of if c.L <= 64 else (c.pos_of // 32) % 64)
    onehot = torch.nn.functional.one_hot(key_code, 64).float()
    qkv[:, 2] = onehot[:, None, :]
    qkv[~c.valid, 2] = 1.0                                                   # rows outside every sequence: ones in every channel (a read shows)
    qkv = qkv.reshape(c.M, 3 * c.D).to(c.dt)
    out, lse = c.fwd(qkv)
    out2, _ = c.fwd(qkv, with_lse=False)
    assert torch.equal(out.view(torch.int16 if c.dt != torch.float32 else torch.int32), out2.view(torch.int16 if c.dt != torch.float32 else torch.int32)), \
        f'{mname} {sid}: the lse = None forward differs from the training forward'
    # expected: prefix sums of the one-hots over each sequence, up to the last visible key
    oh = onehot.double()[c.rows]                                             # [N, L, 64]
    cs = oh.cumsum(1)
    last = torch.clamp(torch.arange(c.L, device=cuda) + c.diag, max=c.L - 1)
    want_seq = cs[:, last] / (last + 1).double()[None, :, None]
    want = torch.zeros(c.M, 64, dtype=torch.float64, device=cuda)
    want[c.rows] = want_seq
    want = want[:, None, :].expand(c.M, c.H, 64)
    ulp = 2 * U_STORE[mname] if mname in ('bf16', 'fp16') else 4 * U_STORE[mname]
    got = _per_head(c, out)
    zero = want == 0
    c.check('out of a masked / padding / slot-0 channel (exactly 0)', torch.where(zero, got.double(), want), want, 0.0)
    c.check('out', got, want, ulp * want)
    want_l = torch.log(c.nvis)[:, None].expand(c.M, c.H)
    got_l = torch.where(c.valid[:, None], lse.double(), want_l)
    c.check('lse (uniform scores: ln n_visible)', got_l, want_l, 1e-6 * torch.clamp(want_l, min=1.0))
    if not c.spatial and c.diag == 0:
        first = c.valid & (c.pos_of == 0)
        assert bool((lse[first] == 0).all()), f'{mname} {sid}: a causal query that sees only key 0 must have lse 0 exactly'


@pytest.mark.gpu
@pytest.mark.parametrize('sid', [m[0] for m in MATRIX])
@pytest.mark.parametrize('mname', MODES)
def test_attn_addressing(ops, cuda, mname, sid):
    """q = 0 and v = a code of (sequence i, head h): value c = 1 + ((i // 64 + 5h) mod 64) / 64 in channel (i + 7h) mod 64, zeros elsewhere --
    a read from another sequence or head changes the channel or the value unless both agree (sequences 4096 apart within a head).  Rows outside
    every sequence (slot 0 of temporal attention, and of spatial attention with causal not in {0, 1}) carry channel (i + 7h + 32) mod 64, which
    no row's own output may contain.  out must be c in the row's own code channel -- n c summed exactly, times 1/n in f32, stored: c is exact in
    every storage format, so 2^-22 relative -- and exactly 0 elsewhere: any cross-sequence, cross-head, cls or wrong-stride read shows.
    Backward with dout = the one-hot of the code channel: dP = c and delta = O[code] = c up to the storage ulp, so dQ = dK = 0 up to that ulp
    times max|k| / 8 and dV[key] = sum over the queries that see the key of 1 / n_visible(query), in the code channel only.  Outputs are prefilled with NaN: every row the header promises is written; rows of no sequence are exactly 0."""
    c = Case(ops, cuda, mname, sid)
    g = torch.Generator(device=cuda).manual_seed(11)
    qkv = torch.randn(c.M, 3, c.H, 64, device=cuda, generator=g)
    qkv[:, 0] = 0.0
    heads = torch.arange(c.H, device=cuda)
    if c.spatial:
        seq_any = torch.arange(c.M, device=cuda) // c.S                     # the (clip, frame) of a row, also for an excluded slot 0
    else:
        r = torch.arange(c.M, device=cuda)
        seq_any = (r // (c.T * c.S)) * (c.S - 1) + torch.clamp(r % c.S - 1, min=0)
    code = (seq_any[:, None] + 7 * heads[None]) % 64                         # [M, H]
    code = torch.where(c.valid[:, None], code, (code + 32) % 64)
    oh = torch.nn.functional.one_hot(code, 64).float()
    val = 1.0 + ((seq_any[:, None] // 64 + 5 * heads[None]) % 64).float() / 64
    qkv[:, 2] = oh * val[..., None]
    qkv = qkv.reshape(c.M, 3 * c.D).to(c.dt)
    out, lse = c.fwd(qkv)
    ulp = 2 * U_STORE[mname] if mname in ('bf16', 'fp16') else 4 * U_STORE[mname]
    want = torch.where(c.valid[:, None, None], (oh * val[..., None]).double(), torch.zeros_like(oh, dtype=torch.float64))
    got = _per_head(c, out).double()
    c.check('out (addressing: exactly 0 off the code channel)', torch.where(want == 0, got, want), want, 0.0)
    c.check('out (addressing: code channel)', got, want, 2.0 ** -22 * want)
    dout = oh.reshape(c.M, c.D).to(c.dt)
    dqkv = c.bwd(qkv, out, dout, lse)
    d = dqkv.view(c.M, 3, c.H, 64).double()
    c.check('dqkv of rows of no sequence (exactly 0)', torch.where(c.valid[:, None, None, None], torch.zeros_like(d), d), torch.zeros_like(d), 0.0)
    kmax = float(qkv.view(c.M, 3, c.H, 64)[:, 1].double().abs().max())
    tqk = 8 * ulp * kmax / 8 + 1e-6                                          # (|dP - delta| <= ulp c, c < 2)
    c.check('dq (addressing: 0)', torch.where(c.valid[:, None, None], d[:, 0], torch.zeros_like(d[:, 0])), torch.zeros_like(d[:, 0]), tqk)
    c.check('dk (addressing: 0)', torch.where(c.valid[:, None, None], d[:, 1], torch.zeros_like(d[:, 1])), torch.zeros_like(d[:, 1]), tqk)
    # dV[key] = sum_{q >= key - diag} 1 / n_visible(q)  (suffix sums over each sequence)
    inv = (1.0 / c.nvis)[c.rows]                                             # [N, L]
    suf = inv.flip(1).cumsum(1).flip(1)
    first_q = torch.clamp(torch.arange(c.L, device=cuda) - c.diag, min=0)
    wv = torch.zeros(c.M, dtype=torch.float64, device=cuda)
    wv[c.rows] = suf[:, first_q]
    want_dv = wv[:, None, None] * torch.where(c.valid[:, None, None], oh.double(), torch.zeros_like(oh, dtype=torch.float64))
    tdv = {'f32': 2e-5, 'f32x3': 2e-5, 'bf16': 2.0 ** -6, 'fp16': 2.0 ** -9}[mname] + c.L * 2.0 ** -24     # (+ f32 accumulation of up to L terms)
    c.check('dv (addressing)', torch.where(c.valid[:, None, None], d[:, 2], torch.zeros_like(d[:, 2])), want_dv, tdv * want_dv.abs() + 1e-7)


# ---------------------------------------------------------------------------------------------------- float64-reference families
def _score_bound(c, qkv):
    """Per (row, head) bound A = max over keys of sum_i |q_i k_i| / 8 <= |q| max|k| / 8 (Cauchy-Schwarz): the f32 accumulation of a score rounds
    relative to this magnitude."""
    x = qkv.double().view(c.M, 3, c.H, 64)
    kmax = x[:, 1].norm(dim=-1)[c.rows].amax(1)                              # [N, H]
    kk = torch.zeros(c.M, c.H, dtype=torch.float64, device=c.dev)
    kk[c.rows] = kmax[:, None, :].expand(c.N, c.L, c.H)
    return x[:, 0].norm(dim=-1) * kk / 8


def _models(c):
    """(forward, backward) score models (_scores) of the kernels this mode and shape dispatch to: f32 exact; f32x3 the split products both ways;
    16-bit: the streaming forward without a mask (attn_fwd_stream_nc: spatial / joint sequences, unmasked temporal ones past 64 frames) pre-rounds
    q, every other 16-bit forward and every 16-bit backward uses exact bf16 / fp16 products."""
    if c.mname == 'f32':
        return 'exact', 'exact'
    if c.mname == 'f32x3':
        return 'x3', 'x3'
    nc = c.diag >= BIG and c.nt >= 2 and (c.spatial or c.nt > 2)
    return (c.dt if nc else 'exact'), 'exact'


def _compare(c, qkv, out, lse, dqkv, ref, label, ref_plain=None):
    """The kernel against attn_ref64 under the kernel's own score models (_models): what is left is the f32 accumulation of the scores
    (absolute error <= E = 2^-20 A per score, A = _score_bound: sixteen ulps of the magnitude) and the storage / operand roundings of the mode.
      lse : |d| <= E + 2e-6 max(1, |lse|);
      out : |d| <= TOL max|ref| + (4 U_OP sqrt(sum_j P_j^2) + 4 E) max|v|   (P is rounded to the operand format before P V, term by
            term: four standard deviations of the sum; a systematic score error moves P by 2E relatively);
      dqkv: |d| <= 1.5 TOL max|ref of the column| + 4 max E dqkv_abs + U_DP dqkv_mag + U_STORE dqkv_delta + 4 U_OP dqkv_rms
            (a systematic score error moves every term alike; dP = dO V^T accumulates in f32 -- of split products in f32x3, U_DP = 2^-15,
            else 2^-20; delta comes from the stored O, rounded to the storage format -- one error per row, shared by all its keys; P and dS
            are rounded to the operand format term by term -- independent roundings, four standard deviations of their sum).
    TOL = test_attention_fwd_bwd's tolerance.  The out bound stays below max|ref| / 4 and the dq / dk / dv bounds below |ref| (dv: |ref| / 4)
    on >= 50 % of each section's elements above max|ref| / 4: a zero output fails.  ref_plain (N(0, 1)
    scores): out and dqkv against that exact-score reference with test_attention_fwd_bwd's bounds alone.  Returns the errors
    (max |d| / max |ref| for out and dqkv, max |d| for lse)."""
    v = c.valid
    tol, uop = TOL[c.mname], U_OP[c.mname]
    E = 2.0 ** -20 * _score_bound(c, qkv)                                    # [M, H]
    vmax = float(qkv.double().view(c.M, 3, c.H, 64)[:, 2].abs().max())
    omax = float(ref['out'].abs().max())
    t_out = tol * omax + (4 * uop * ref['prms'] + 4 * E) * vmax
    if ref_plain is not None:
        ref = dict(ref, out=ref_plain['out'], dqkv=ref_plain['dqkv'])
        t_out = torch.full_like(E, tol * omax)
    assert float(t_out[v].max()) < 0.25 * omax, f'{c.mname} {c.sid} {label}: the out bound {float(t_out[v].max()):.3e} is not below max|ref| {omax:.3e} / 4'
    c.check(f'{label}: out', torch.where(v[:, None], out.double(), ref['out']), ref['out'], t_out[..., None].expand(c.M, c.H, 64))
    want_l = torch.where(v[:, None], ref['lse'], torch.zeros_like(ref['lse']))
    got_l = torch.where(v[:, None], lse.double(), torch.zeros_like(want_l))
    c.check(f'{label}: lse', got_l, want_l, E + 2e-6 * torch.clamp(want_l.abs(), min=1.0))
    e_d = None
    if dqkv is not None:
        dmax = float(ref['dqkv'].abs().max())
        cmax = ref['dqkv'].abs().amax(0, keepdim=True).clamp(min=1e-3 * dmax)                    # per column (section, head, channel): channel 0 of q / k is the large one
        t_d = 1.5 * tol * cmax + 4 * float(E[v].max()) * ref['dqkv_abs'] + (2.0 ** -15 if c.mname == 'f32x3' else 2.0 ** -20) * ref['dqkv_mag'] \
            + U_STORE[c.mname] * ref['dqkv_delta'] + 4 * uop * ref['dqkv_rms'] if ref_plain is None \
            else torch.full_like(ref['dqkv'], 1.5 * tol * dmax)
        # dq, dk, dv: the bound is below |ref| (a zero output fails) on >= 50 % of the elements above max|ref| / 4 of that section, and below
        # |ref| / 4 on >= 50 % in dv -- leaving out elements that are cancelling sums (|ref| < dqkv_mag / 10: dP - delta ~ 0 where one key
        # takes the weight, and the rounding of the stored O then sets the error of dk at that key), channel 0
        # of each head, which carries the families' large score component: there dq / dk are cancelling sums of terms 8-30x larger, and the
        # 16-bit rounding of dS bounds them at the level of their value -- and sections that vanish (dS ~ 0 when one key takes all the weight)
        rd = ref['dqkv'].view(c.M, 3, c.H, 64)[..., 1:].abs().reshape(c.M, 3, -1)
        td = (t_d if torch.is_tensor(t_d) else torch.full_like(ref['dqkv'], t_d)).view(c.M, 3, c.H, 64)[..., 1:].reshape(c.M, 3, -1)
        ra = ref['dqkv_mag'].view(c.M, 3, c.H, 64)[..., 1:].reshape(c.M, 3, -1)
        for sec in range(3):
            if float(rd[:, sec].max()) < 1e-3 * dmax:
                continue
            big = (rd[:, sec] >= 0.25 * float(rd[:, sec].max())) & (rd[:, sec] >= 0.1 * ra[:, sec])
            if not bool(big.any()):
                continue
            lim = 0.25 if sec == 2 else 1.0
            frac = float((td[:, sec][big] < lim * rd[:, sec][big]).double().mean())
            assert frac >= 0.5, f'{c.mname} {c.sid} {label}: the d{"qkv"[sec]} bound is below |ref| * {lim} on only {frac:.0%} of its large elements'
        c.check(f'{label}: dqkv', dqkv, ref['dqkv'], t_d)
        e_d = rel_max(dqkv, ref['dqkv'], torch.ones(c.M, dtype=torch.bool, device=c.dev))
    return rel_max(out, ref['out'], v), float((got_l - want_l).abs().max()), e_d


def _run_ref_family(c, qkv32, dout32, label, plain=False):
    """Forward + backward of the kernel against attn_ref64 under the kernel's score models (_compare).  Also returns the errors against the
    exact-score reference -- what the pre-rounded q / split products cost at these scores (printed with -s)."""
    qkv = qkv32.reshape(c.M, 3 * c.D).to(c.dt)
    dout = dout32.reshape(c.M, c.D).to(c.dt)
    out, lse = c.fwd(qkv)
    dqkv = c.bwd(qkv, out, dout, lse)
    fm, bm = _models(c)
    ref = attn_ref64(qkv, c.B, c.T, c.S, c.H, c.ca, c.spatial, dout, fwd_model=fm, bwd_model=bm)
    ref_x = attn_ref64(qkv, c.B, c.T, c.S, c.H, c.ca, c.spatial, dout) if (fm, bm) != ('exact', 'exact') else ref
    errs = _compare(c, qkv, out, lse, dqkv, ref, label, ref_x if plain else None)
    ref = ref_x
    v = c.valid
    exact = (rel_max(out, ref['out'], v), float((lse.double() - ref['lse'])[v].abs().max()), rel_max(dqkv, ref['dqkv'], torch.ones_like(v)))
    print(f'\nattn {label:22s} {c.mname:6s} {c.sid:11s} vs model: out {errs[0]:.2e} lse {errs[1]:.2e} dqkv {errs[2]:.2e} | '
          f'vs exact scores: out {exact[0]:.2e} lse {exact[1]:.2e} dqkv {exact[2]:.2e}')
    return out, lse, ref, errs


def _key_tile(c):
    t = torch.where(c.valid, c.pos_of // 32, torch.zeros_like(c.pos_of))
    return t


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['rise', 'fall', 'rise_last'])
@pytest.mark.parametrize('sid', BRANCHES)
@pytest.mark.parametrize('mname', MODES)
def test_attn_ramp_rescale(ops, cuda, mname, sid, kind):
    """q[:, 0] = 8 and k[key, 0] = 8 level(tile of key), level in 0..31 (integers <= 248: exact in bf16 and fp16), plus N(0, 0.35^2)
    components elsewhere (score noise ~0.12 nats).  rise: level = tile (sawtooth mod 32 on longer sequences) -- the row maximum grows by 8 nats
    = 11.5 log2 units per key tile, more than the lazy maximum's 8, so the alpha rescale of o0, o1, l (and negm, m) runs on every tile;
    fall: level = 31 - tile (max in tile 0, later tiles underflow); rise_last: level = 31 - (nt - 1 - tile), clamped at 0, peaking inside the
    last (ragged / half) tile.  out, lse and dq, dk, dv against attn_ref64 (bounds: _compare)."""
    c = Case(ops, cuda, mname, sid)
    g = torch.Generator(device=cuda).manual_seed(21)
    x = torch.randn(c.M, 3, c.H, 64, device=cuda, generator=g) * 0.35
    x[:, 2] = torch.randn(c.M, c.H, 64, device=cuda, generator=g)
    t = _key_tile(c)
    if kind == 'rise':
        lev = t % 32
    elif kind == 'fall':
        lev = torch.clamp(31 - t, min=0)
    else:
        lev = torch.clamp(31 - (c.nt - 1 - t), min=0)
    x[:, 0, :, 0] = 8.0
    x[:, 1, :, 0] = (8 * lev).float()[:, None]
    dout = torch.randn(c.M, c.H, 64, device=cuda, generator=g)
    _run_ref_family(c, x, dout, f'ramp {kind}')


@pytest.mark.gpu
@pytest.mark.parametrize('sid', BRANCHES)
@pytest.mark.parametrize('mname', MODES)
def test_attn_shift_invariance(ops, cuda, mname, sid):
    """k[:, 0] = 16 for every key and q[:, 0] = +-100 by row: every score of a row moves by the same +-200 nats.  Softmax is invariant, so out
    must match the unshifted run (q[:, 0] = 0) within both runs' tolerances plus the f32 accumulation of the shifted scores (2^-20 A, about 2e-4
    nats here), and lse must move by +-200 plus what the kernels' score model moves it by: nothing in f32 and f32x3 (+-100 and 16 split exactly),
    and in the 16-bit streaming forward without a mask the pre-scaled q[:, 0] = +-100 * 0.125 log2(e) rounded to 16 bits (0.37 nats for bf16,
    0.03 for fp16) -- within the two runs' f32 accumulation bounds (2^-20 A each: 4e-4 nats, about 25 f32 ulps of 205).  Both runs also against
    attn_ref64, backward included (_compare)."""
    c = Case(ops, cuda, mname, sid)
    g = torch.Generator(device=cuda).manual_seed(31)
    x = torch.randn(c.M, 3, c.H, 64, device=cuda, generator=g)
    x[:, 1, :, 0] = 16.0
    sign = torch.where(torch.arange(c.M, device=cuda) % 2 == 0, 1.0, -1.0)
    dout = torch.randn(c.M, c.H, 64, device=cuda, generator=g)
    x0 = x.clone(); x0[:, 0, :, 0] = 0.0
    out0, lse0, ref0, _ = _run_ref_family(c, x0, dout, 'shift (unshifted run)')
    x[:, 0, :, 0] = 100.0 * sign[:, None]
    out1, lse1, _, _ = _run_ref_family(c, x, dout, 'shift +-200 nats')
    # out: the shift moves every score of a row alike, so softmax cancels it -- also the model's rounding of q[:, 0] (one error times the constant
    # k[:, 0] = 16, the same for every key).  What is left: both runs' tolerances and the f32 accumulation of the shifted scores (2^-20 A)
    q1 = x.reshape(c.M, 3 * c.D).to(c.dt)
    vmax = float(q1.double().view(c.M, 3, c.H, 64)[:, 2].abs().max())
    omax = float(out0.double().abs().max())
    t = 2 * TOL[mname] * omax + (8 * U_OP[mname] * ref0['prms'] + 8 * 2.0 ** -20 * _score_bound(c, q1)) * vmax
    assert float(t[c.valid].max()) < 0.25 * omax
    c.check('shifted out vs unshifted out', torch.where(c.valid[:, None], out1.double(), out0.double()), out0, t[..., None].expand(c.M, c.H, 64))
    # lse: moves by +-200 nats plus what the score model moves it by (f32: nothing; f32x3: the split of +-100 and 16 is exact; 16-bit streaming
    # forward without a mask: the pre-scaled q[:, 0]'s rounding times 16), within both runs' f32 accumulation bounds
    fm, _ = _models(c)
    qq = q1.double().view(c.M, 3, c.H, 64)[:, 0, :, :1].reshape(-1, 1, 1)
    kk = torch.full_like(qq, 16.0)
    dmodel = (_scores(qq, kk, fm) - _scores(qq, kk, 'exact')).view(c.M, c.H)
    shift = (200.0 * sign)[:, None].expand(c.M, c.H) + dmodel
    want = torch.where(c.valid[:, None], lse0.double() + shift, torch.zeros_like(shift))
    got = torch.where(c.valid[:, None], lse1.double(), torch.zeros_like(shift))
    tl = 2.0 ** -20 * (_score_bound(c, q1) + _score_bound(c, x0.reshape(c.M, 3 * c.D).to(c.dt))) + 4e-6 * 200
    c.check('lse shift', got, want, tl)


def _planted_keys(c):
    nt, L, lr = c.nt, c.L, c.L - 32 * (c.nt - 1)
    cand = [0, L - 1, 15, 16, 31, 32, 32 * (nt - 1) + min(15, lr - 1), 32 * (nt - 1) + min(16, lr - 1)]
    return sorted({p for p in cand if 0 <= p < L})


@pytest.mark.gpu
@pytest.mark.parametrize('sid', BRANCHES)
@pytest.mark.parametrize('mname', MODES)
def test_attn_planted_key(ops, cuda, mname, sid):
    """One key per (sequence, head) scores 30 nats above the rest (q[:, 0] = 8, k[planted, 0] = 30, other components N(0, 0.3^2): the rest
    of a row is ~0.1 nats wide): at key 0, the last valid key, keys 15 / 16 of a half tile, the 31 / 32 tile boundary, cycling over (sequence,
    head) so that neighbouring sequences -- the two of a mixed workgroup -- plant at different keys.  A query that sees its planted key must get
    out = v[planted] to one storage ulp (f32x3: the split P V product's 2^-16; the others weigh e^-30 L <= 1e-9) and lse = its score under the kernels' score model (_compare); everything, backward
    included, against attn_ref64."""
    c = Case(ops, cuda, mname, sid)
    g = torch.Generator(device=cuda).manual_seed(41)
    x = torch.randn(c.M, 3, c.H, 64, device=cuda, generator=g) * 0.3
    x[:, 2] = torch.randn(c.M, c.H, 64, device=cuda, generator=g)
    cand = torch.tensor(_planted_keys(c), device=cuda)
    seq = torch.arange(c.N, device=cuda)[:, None]; hh = torch.arange(c.H, device=cuda)[None]
    plant = cand[(seq + hh) % len(cand)]                                     # [N, H]
    x[:, 0, :, 0] = 8.0
    k0 = torch.zeros(c.M, c.H, device=cuda)
    prow = c.rows.gather(1, plant)                                           # [N, H] token row of the planted key
    k0[prow, hh.expand_as(prow)] = 30.0
    x[:, 1, :, 0] = k0
    dout = torch.randn(c.M, c.H, 64, device=cuda, generator=g)
    out, lse, ref, _ = _run_ref_family(c, x, dout, 'planted')
    # direct: out == v[planted] where the planted key is visible
    xs = x.reshape(c.M, 3 * c.D).to(c.dt).view(c.M, 3, c.H, 64)
    vp = torch.zeros(c.M, c.H, 64, dtype=torch.float64, device=cuda)
    vp[c.rows] = xs[prow, 2, hh.expand_as(prow)].double()[:, None].expand(c.N, c.L, c.H, 64)
    pp = torch.full((c.M, c.H), BIG, dtype=torch.long, device=cuda)
    pp[c.rows] = plant[:, None, :].expand(c.N, c.L, c.H)
    sees = c.valid[:, None] & (pp <= c.pos_of[:, None] + c.diag)
    ulp = {'f32': 4 * U_STORE[mname], 'f32x3': 2.0 ** -15, 'bf16': 2 * U_STORE[mname], 'fp16': 2 * U_STORE[mname]}[mname]   # f32x3: P V drops lo x lo (2^-16)
    got = _per_head(c, out).double()
    c.check('out == v[planted key]', torch.where(sees[..., None], got, vp), vp, ulp * vp.abs() + 1e-9 * c.L)


@pytest.mark.gpu
@pytest.mark.parametrize('sigma', [1, 4, 8])
@pytest.mark.parametrize('sid', ['t30_bench', 's301_bench', 'j1441'])
@pytest.mark.parametrize('mname', MODES)
def test_attn_random_score_scale(ops, cuda, mname, sid, sigma):
    """randn q, k scaled by sqrt(sigma): scores q.k/8 ~ N(0, sigma^2) nats, at the production shapes (configs[1]'s temporal and spatial calls, the
    joint sequence).  Bounds (_compare): at sigma = 1 out and dqkv against the exact-score reference with test_attention_fwd_bwd's tolerances;
    at sigma = 4 and 8 against the kernels' score models, where what the pre-rounded q / split products cost is no longer small (the errors
    against exact scores print next to them with -s)."""
    c = Case(ops, cuda, mname, sid)
    g = torch.Generator(device=cuda).manual_seed(51 + sigma)
    x = torch.randn(c.M, 3, c.H, 64, device=cuda, generator=g)
    x[:, :2] *= math.sqrt(sigma)
    dout = torch.randn(c.M, c.H, 64, device=cuda, generator=g)
    out, lse, ref, (eo, el, ed) = _run_ref_family(c, x, dout, f'random sigma={sigma}', plain=sigma == 1)
    out2, _ = c.fwd(x.reshape(c.M, 3 * c.D).to(c.dt), with_lse=False)
    assert torch.equal(out.view(torch.int16 if c.dt != torch.float32 else torch.int32), out2.view(torch.int16 if c.dt != torch.float32 else torch.int32)), \
        f'{mname} {sid}: the lse = None forward differs from the training forward'
    print(f'\nattn-score-scale {mname:6s} {sid:11s} sigma={sigma}: out {eo:.3e}  lse {el:.3e}  dqkv {ed:.3e}  (rel tol {TOL[mname]:.1e})')

"""GPU: tcow_attn_temporal_step_probs (csrc/attention_stream_probs.hip), the softmax rows of a stream step against its K cache.

The contract (include/tcow_hip.h): probs[f, s-1, h, k] = softmax_{k' <= t}(q_t . K_k' / 8)[k] for k <= t and +0.0 for t < k < T_total, K_k the
cached line (decoded when the cache is compact) for k < t0 and the step's own row (rounded through the cache type) for k >= t0, q unrounded.
(1) against the float64 softmax of the same stored values within attn_probs_kit.prob_bound (derived, not measured), (2) the exact properties,
(3) bit for bit across forms, layouts and splits, and before / after the step, (4) P @ V against the step's own output, (5) bad rows.
rnd_C and the decoding are those of test_gpu_stream_cache_dtype.py (_enc / _dec: torch on the CPU)."""
import numpy as np
import pytest
import torch

from attn_probs_kit import U32, prob_bound, worst
from stream_kit import CHUNK_LISTS, _i32, _tables, _to_pages
from test_gpu_stream_cache_dtype import PAIRS as COMPACT, _b, _dec, _enc
from tcow_amd import ops

pytestmark = pytest.mark.gpu

NAN = float('nan')
# (storage mode, cache_dtype of ops, torch dtype of the cache): the storage type, the 16-bit type under f32, fp8 under both
PAIRS = dict({'f32': (ops.F32, None, torch.float32), 'bf16': (ops.BF16, None, torch.bfloat16), 'fp16': (ops.FP16, None, torch.float16)}, **COMPACT)


def _sessions(pair, cs, t0s, slots, n_slots, S, heads, T_total, seed):
    """n sessions, session r with cs[r] new frames at t0s[r] on slot slots[r]: the flat qkv [F*S, 3D] in the storage type and K / V caches
    [n_slots, S-1, heads, T_total, 64] that are NaN everywhere but at positions < t0 of a session's slot (encoded randn): whatever a launch may
    not read is poison."""
    mode, _, cdt = PAIRS[pair]
    D = heads * 64
    g = torch.Generator(device='cuda').manual_seed(seed)
    shape = (n_slots, S - 1, heads, T_total, 64)
    kc, vc = torch.full(shape, NAN, device='cuda').to(cdt), torch.full(shape, NAN, device='cuda').to(cdt)
    qkvs = []
    for c, t0, sl in zip(cs, t0s, slots):
        for cache in (kc, vc):
            if t0:
                _b(cache)[sl, ..., :t0, :] = _b(_enc(torch.randn(S - 1, heads, t0, 64, device='cuda', generator=g), cdt))
        qkvs.append(torch.randn(c * S, 3 * D, device='cuda', generator=g).to(ops.tdtype(mode)))
    return torch.cat(qkvs, 0).contiguous(), kc, vc


def _ref64(pair, qkv, k_slot, c, t0, S, heads, T_total):
    """One session: qkv [c*S, 3D] of its frames, k_slot [S-1, heads, T_total, 64] its cache block before the step -> dict(P [c, S-1, heads,
    T_total] f64 with zeros past t, delta = 66 u max sum_c |q_c K_c| / 8 over the products the kernel forms, n_keys [c, 1, 1, 1] = t + 1)."""
    cdt, D = PAIRS[pair][2], heads * 64
    per = lambda x: x.view(c, S, heads, 64)[:, 1:].permute(1, 2, 0, 3).contiguous()            # [S-1, heads, c, 64]
    q = per(qkv[:, :D]).double()
    K = torch.cat([_dec(k_slot[..., :t0, :].contiguous()), _dec(_enc(per(qkv[:, D:2 * D]), cdt))], 2)     # [S-1, heads, t0 + c, 64]
    keep = torch.arange(t0 + c, device='cuda')[None, :] <= (t0 + torch.arange(c, device='cuda'))[:, None]
    s = (q @ K.transpose(-1, -2) / 8.0).masked_fill(~keep, float('-inf'))
    mag = float((q.abs() @ K.abs().transpose(-1, -2)).masked_fill(~keep, 0.0).max()) / 8
    P = torch.nn.functional.pad(torch.softmax(s, -1), (0, T_total - t0 - c)).permute(2, 0, 1, 3).contiguous()
    n_keys = (t0 + 1 + torch.arange(c, device='cuda')).view(c, 1, 1, 1).double()
    return dict(P=P, delta=66 * U32 * mag, n_keys=n_keys)


def _launch(form, pair, cs, t0s, slots, n_slots, S, heads, T_total, qkv, kc, vc, causal=1, P=None, page_of=None, n_pages=None, tables=None):
    """One launch of `form` into a NaN-filled probs [F, S-1, heads, T_total].  stream: one row per session, equal c and t0, slot = row;
    paged: kc / vc are the page arrays."""
    mode, cq, _ = PAIRS[pair]
    D, F, n = heads * 64, sum(cs), len(cs)
    probs = torch.full((F, S - 1, heads, T_total), NAN, device='cuda')
    if form == 'stream':
        ops.attn_temporal_step_probs('stream', mode, n, cs[0], S, D, heads, causal, T_total, _i32(t0s[:1]), qkv, kc, vc, probs, cache_dtype=cq)
    elif form == 'pool':
        ops.attn_temporal_step_probs('pool', mode, n, cs[0], S, D, heads, causal, T_total, n_slots, _i32(t0s), _i32(slots), qkv, kc, vc, probs, cache_dtype=cq)
    else:
        tb = tables if tables is not None else _tables(t0s, slots, cs)[0]
        if form == 'ragged':
            ops.attn_temporal_step_probs('ragged', mode, n, F, S, D, heads, causal, T_total, n_slots, tb['t0'], tb['slot'], tb['first'], tb['c'],
                                         tb['row_of_frame'], qkv, kc, vc, probs, cache_dtype=cq)
        else:
            ops.attn_temporal_step_probs('paged', mode, n, F, S, D, heads, causal, T_total, n_pages, P, tb['t0'], _i32(sum(page_of, [])).view(n, -1),
                                         tb['first'], tb['c'], tb['row_of_frame'], qkv, kc, vc, probs, cache_dtype=cq)
    return probs


def _page_table(n, T_total, P, rng, extra=2):
    """A permuted page table: pps = ceil(T_total / P) pages per session out of n * pps + extra."""
    pps = -(-T_total // P)
    n_pages = n * pps + extra
    ids = [int(v) for v in rng.permutation(n_pages)[:n * pps]]
    return [ids[r * pps:(r + 1) * pps] for r in range(n)], n_pages


def _paged(kc, vc, slots, T_total, P, rng):
    """The sessions' cache blocks as page arrays under a permuted table; pages of no session are NaN."""
    page_of, n_pages = _page_table(len(slots), T_total, P, rng)
    idx = torch.tensor(slots, device='cuda')
    take = lambda cache: _b(cache)[idx].view(cache.dtype)                                     # (gathered as bytes: any cache type)
    return _to_pages(take(kc), page_of, n_pages, P, NAN), _to_pages(take(vc), page_of, n_pages, P, NAN), page_of, n_pages


def _check(pair, probs, qkv, kc0, cs, t0s, slots, S, heads, T_total, tag):
    """Properties 1 and 2 of every session's rows of one launch."""
    f = 0
    for c, t0, sl in zip(cs, t0s, slots):
        got = probs[f:f + c]
        ref = _ref64(pair, qkv[f * S:(f + c) * S], kc0[sl], c, t0, S, heads, T_total)
        assert not torch.isnan(got).any(), tag                  # every element overwritten, and no poisoned byte read
        idx, g, w, d, b = worst(got, ref['P'], prob_bound(ref))
        assert d <= b, (tag, idx, g, w, d, b)
        past = torch.arange(T_total, device='cuda')[None, :] > (t0 + torch.arange(c, device='cuda'))[:, None]          # [c, T_total]
        assert bool((got.view(torch.int32).permute(0, 3, 1, 2)[past] == 0).all()), tag                                # +0.0, bitwise
        rel = (got.double().sum(-1) - 1).abs()
        assert bool((rel <= (ref['n_keys'][..., 0] + 8) * U32).all()), (tag, float(rel.max()))
        f += c


# ---------------------------------------------------------------------------------------------- (1, 2) against float64, exact properties

@pytest.mark.parametrize('pair', list(PAIRS))
def test_probs_rows_and_stream_vs_f64(cuda, pair):
    """A batch is 32 keys in 16-bit storage and 16 in f32; rows of 30 and 33 floats are no 16-byte multiples."""
    seed = 0
    for T_total in (4, 30, 33, 70):
        for c in (1, 3, 9):
            for t0 in sorted({0, 1, T_total - c}):
                if t0 < 0 or t0 + c > T_total:
                    continue
                for S, heads in ((2, 1), (17, 3), (2, 3), (17, 1)):
                    seed += 1
                    form = ('stream', 'pool')[seed % 2]
                    t0s, slots = ([t0, t0], [0, 1]) if form == 'stream' else ([t0, max(T_total - c - t0, 0)], [2, 0])
                    qkv, kc, vc = _sessions(pair, [c, c], t0s, slots, 3 if form == 'pool' else 2, S, heads, T_total, seed)
                    kc0, vc0 = kc.clone(), vc.clone()
                    probs = _launch(form, pair, [c, c], t0s, slots, kc.shape[0], S, heads, T_total, qkv, kc, vc, causal=1 + seed % 2)
                    tag = (pair, form, T_total, c, t0s, S, heads)
                    _check(pair, probs, qkv, kc0, [c, c], t0s, slots, S, heads, T_total, tag)
                    assert torch.equal(_b(kc), _b(kc0)) and torch.equal(_b(vc), _b(vc0)), tag       # the caches are only read


@pytest.mark.parametrize('pair', list(PAIRS))
def test_probs_ragged_and_paged_vs_f64(cuda, pair):
    rng = np.random.default_rng(3)
    for k, (cs, T_total) in enumerate(CHUNK_LISTS):
        n = len(cs)
        t0s = [0, T_total - cs[1], 7][:n] if n > 1 else [T_total - cs[0]]
        t0s = [min(t0, T_total - c) for t0, c in zip(t0s, cs)]
        slots = [3, 0, 4][:n]
        S, heads = ((5, 2), (2, 3), (17, 1))[k % 3]
        qkv, kc, vc = _sessions(pair, cs, t0s, slots, 5, S, heads, T_total, 50 + k)
        kc0, vc0 = kc.clone(), vc.clone()
        ragged = _launch('ragged', pair, cs, t0s, slots, 5, S, heads, T_total, qkv, kc, vc)
        _check(pair, ragged, qkv, kc0, cs, t0s, slots, S, heads, T_total, (pair, 'ragged', cs, T_total, t0s))
        assert torch.equal(_b(kc), _b(kc0)) and torch.equal(_b(vc), _b(vc0))
        for P in (1, 4, 8):
            kp, vp, page_of, n_pages = _paged(kc, vc, slots, T_total, P, rng)
            kp0, vp0 = kp.clone(), vp.clone()
            paged = _launch('paged', pair, cs, t0s, slots, 5, S, heads, T_total, qkv, kp, vp, P=P, page_of=page_of, n_pages=n_pages)
            assert torch.equal(paged, ragged), (pair, 'paged', cs, T_total, P)              # (bitwise: so properties 1 and 2 hold for it too)
            assert torch.equal(_b(kp), _b(kp0)) and torch.equal(_b(vp), _b(vp0))


# ---------------------------------------------------------------------------------------------- (3) bit for bit

def _step(pair, c, t0, S, heads, T_total, qkv, k1, v1):
    """The real step of one session on its own cache block [1, ...]: appends the chunk; returns out."""
    mode, cq, _ = PAIRS[pair]
    out = torch.full((c * S, heads * 64), NAN, device='cuda').to(qkv.dtype)
    ops.attn_temporal_cached(mode, 1, c, S, heads * 64, heads, 1, T_total, _i32([t0]), qkv, k1, v1, out, cache_dtype=cq)
    return out


@pytest.mark.parametrize('pair', list(PAIRS))
def test_probs_bits_do_not_depend_on_form_layout_split_or_order(cuda, pair):
    """Nine frames from t0 = 28 of 70 (the walk crosses a batch boundary in both storage types), as one chunk, 3 + 3 + 3 and nine of 1, the
    cache advanced by the real step; every chunk through all four forms, and once more after the step has appended."""
    S, heads, T_total, t0, sl, n_slots = 3, 2, 70, 28, 2, 3
    D = heads * 64
    rng = np.random.default_rng(9)
    qkv9, kc_init, vc_init = _sessions(pair, [9], [t0], [sl], n_slots, S, heads, T_total, 17)
    rows = {}
    for split in ([9], [3, 3, 3], [1] * 9):
        kc, vc, got, j0 = kc_init.clone(), vc_init.clone(), [], 0
        for c in split:
            qkv, t = qkv9[j0 * S:(j0 + c) * S].contiguous(), t0 + j0
            k1, v1 = kc[sl:sl + 1], vc[sl:sl + 1]
            args = (pair, [c], [t], [sl], n_slots, S, heads, T_total, qkv)
            want = _launch('ragged', *args, kc, vc)
            assert torch.equal(_launch('pool', *args, kc, vc), want), (pair, split, 'pool')
            assert torch.equal(_launch('stream', pair, [c], [t], [0], 1, S, heads, T_total, qkv, k1, v1), want), (pair, split, 'stream')
            for P in (4, 8):
                kp, vp, page_of, n_pages = _paged(kc, vc, [sl], T_total, P, rng)
                assert torch.equal(_launch('paged', *args, kp, vp, P=P, page_of=page_of, n_pages=n_pages), want), (pair, split, 'paged', P)
            _step(pair, c, t, S, heads, T_total, qkv, k1, v1)                                  # (views: kc / vc now hold the chunk)
            assert torch.equal(_launch('ragged', *args, kc, vc), want), (pair, split, 'after the step')
            got.append(want); j0 += c
        rows[len(split)] = torch.cat(got, 0)
        assert not torch.isnan(rows[len(split)]).any()
    assert torch.equal(rows[1], rows[3]) and torch.equal(rows[1], rows[9]), pair


# ---------------------------------------------------------------------------------------------- (4) consistency with the step

@pytest.mark.parametrize('pair', list(PAIRS))
def test_probs_times_v_is_the_steps_output(cuda, pair):
    """P @ V against tcow_attn_temporal_step's own out, V in float64 from the cache after the step (decoded if compact), at the tolerance
    test_cached_temporal_attention_vs_f64 uses for that kernel."""
    mode, cq, cdt = PAIRS[pair]
    B, c, S, heads, T_total, t0 = 2, 3, 5, 2, 40, 33
    D, dt = heads * 64, ops.tdtype(mode)
    qkv, kc, vc = _sessions(pair, [c] * B, [t0] * B, [0, 1], B, S, heads, T_total, 23)
    probs = _launch('stream', pair, [c] * B, [t0] * B, [0, 1], B, S, heads, T_total, qkv, kc, vc)
    out = torch.full((B * c * S, D), NAN, device='cuda').to(dt)
    ops.attn_temporal_cached(mode, B, c, S, D, heads, 1, T_total, _i32([t0]), qkv, kc, vc, out, cache_dtype=cq)
    V = _dec(vc[..., :t0 + c, :].contiguous())                                                 # [B, S-1, heads, t0 + c, 64]
    Pm = probs.view(B, c, S - 1, heads, T_total)[..., :t0 + c].permute(0, 2, 3, 1, 4).double()  # [B, S-1, heads, c, t0 + c]
    ref = Pm @ V
    got = out.view(B, c, S, heads, 64)[:, :, 1:].permute(0, 2, 3, 1, 4).double()
    err = float((got - ref).abs().max())
    print(f'{pair}: max |P @ V - out| = {err:.3e}, max |ref| = {float(ref.abs().max()):.3e}, max |V| = {float(V.abs().max()):.3e}')
    if dt == torch.float32:
        assert err <= 2e-6 * float(ref.abs().max()), (pair, err)
    else:
        assert err <= ((2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11) + 1e-5) * float(V.abs().max()), (pair, err)


# ---------------------------------------------------------------------------------------------- (5) bad rows

@pytest.mark.parametrize('pair', ['f32', 'bf16', 'fp16_fp8'])
def test_probs_bad_row_among_good_rows(cuda, pair):
    """Session 1 of three made bad through the device tables (the host cannot see them): its rows are NaN, the others' rows the bits of the
    launch without the fault, the caches untouched.  The documented, bounds-checked path of the step's own bad rows."""
    cs, t0s, slots, n_slots, S, heads, T_total, P = [2, 1, 3], [5, 28, 0], [3, 0, 4], 5, 3, 2, 30, 4
    qkv, kc, vc = _sessions(pair, cs, t0s, slots, n_slots, S, heads, T_total, 31)
    kc0, vc0 = kc.clone(), vc.clone()
    kp, vp, page_of, n_pages = _paged(kc, vc, slots, T_total, P, np.random.default_rng(31))
    kp0, vp0 = kp.clone(), vp.clone()
    args = (pair, cs, t0s, slots, n_slots, S, heads, T_total, qkv)
    clean = _launch('ragged', *args, kc, vc)
    assert torch.equal(_launch('paged', *args, kp, vp, P=P, page_of=page_of, n_pages=n_pages), clean) and not torch.isnan(clean).any()

    def check(probs, tag):
        assert bool(torch.isnan(probs[2:3]).all()), tag                                        # flat frame 2 is session 1
        assert torch.equal(probs[:2], clean[:2]) and torch.equal(probs[3:], clean[3:]), tag
        assert torch.equal(_b(kc), _b(kc0)) and torch.equal(_b(vc), _b(vc0)) and torch.equal(_b(kp), _b(kp0)) and torch.equal(_b(vp), _b(vp0)), tag

    for table, value in (('t0', -1), ('t0', T_total - cs[1] + 1), ('slot', n_slots)):
        tb = _tables(t0s, slots, cs)[0]
        tb[table][1] = value
        check(_launch('ragged', *args, kc, vc, tables=tb), (pair, table, value))
        if table == 't0':
            check(_launch('paged', *args, kp, vp, P=P, page_of=page_of, n_pages=n_pages, tables=tb), (pair, 'paged', table, value))
    for q in (0, 3, 7):                                         # an entry the frame at t = 28 needs: pages 0 .. 7
        bad = [list(p) for p in page_of]
        bad[1][q] = n_pages
        check(_launch('paged', *args, kp, vp, P=P, page_of=bad, n_pages=n_pages), (pair, 'page', q))

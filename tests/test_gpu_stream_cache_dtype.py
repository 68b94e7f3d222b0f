"""GPU: the compact K / V cache of a stream (net.stream(cache_dtype='bf16' | 'fp8'), the cache_dtype field of tcow_attn_temporal_step).

The contract (include/tcow_hip.h): with a cache of element type C a step computes softmax_{t' <= t}(q_t . rnd_C(k_t') / 8) rnd_C(v_t') with EVERY
key and value at its rounded value, the step's own frames included, and appends the rounded bits once.  rnd_C is defined by torch on the CPU:
x.clamp(-448, 448).to(torch.float8_e4m3fn) for fp8, x.to(torch.bfloat16) for the 16-bit cache of the f32-storage modes (_enc below).  So the
kernel tests compare against an f64 restatement on inputs rounded that way with the tolerances of test_gpu_stream._attn_case (they cover the
output rounding only), the cache bytes against _enc bit for bit, and the four step forms and every chunking against each other bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import build_hip_seeker, golden_inputs, load_golden
from stream_kit import _i32, _to_pages as _pages_filled, f64_cached_attention, synth_clips, synth_net
from tcow_amd import _lib, ops, stream
from tcow_amd._lib import TcowError

pytestmark = pytest.mark.gpu

FP8T = torch.float8_e4m3fn
# (storage mode, cache_dtype of ops, torch dtype of the cache): storage 16-bit -> fp8 in both builds, storage f32 -> the 16-bit type and -> fp8
PAIRS = {'bf16_fp8': (ops.BF16, ops.FP8, FP8T), 'fp16_fp8': (ops.FP16, ops.FP8, FP8T), 'f32_bf16': (ops.F32, ops.BF16, torch.bfloat16),
         'f32_fp8': (ops.F32, ops.FP8, FP8T)}


def _G(mode):
    """Key rows per load of a wave (attention_stream.hip: 64 lanes / (64 channels / channels per lane)); a key-loop trip takes KB = 4 G keys."""
    return 8 if ops.is16(mode) else 4


def _enc(x, cdt):
    """THE defining conversion of a tensor of storage values to the cache type, on the CPU; returned on the GPU."""
    x = x.detach().float().cpu()
    return (x.clamp(-448, 448).to(cdt) if cdt == FP8T else x.to(cdt)).cuda()


def _dec(c):
    """Cache elements -> f64 (exact), converted on the CPU."""
    return c.cpu().float().double().cuda()


def _b(t):
    """The bytes of a contiguous tensor: [..., 64] elements -> [..., 64 * element size] uint8 (a view)."""
    return t.view(torch.uint8)


def _pattern(shape, cdt, seed):
    """A cache of random bytes (any byte, NaN codes included: what a launch may not read, and may not change)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    es = torch.empty(0, dtype=cdt).element_size()
    return torch.randint(0, 256, (*shape[:-1], shape[-1] * es), dtype=torch.uint8, device='cuda', generator=g).view(cdt)


def _per(x, B, c, S, heads):
    """Rows (b*c + j)*S + s of a [B*c*S, heads*64] block -> (B, S-1, heads, c, 64), slot 0 dropped: the layout of a cache."""
    return x.view(B, c, S, heads, 64)[:, :, 1:].permute(0, 2, 3, 1, 4)


def _inputs(mode, cdt, B, c, S, heads, T_total, t0, seed):
    """qkv of a chunk (storage type) and K / V caches [B, S-1, heads, T_total, 64] of random bytes whose positions < t0 hold encoded randn."""
    D = heads * 64
    g = torch.Generator(device='cuda').manual_seed(seed)
    qkv = torch.randn(B * c * S, 3 * D, device='cuda', generator=g).to(ops.tdtype(mode))
    shape = (B, S - 1, heads, T_total, 64)
    kc, vc = _pattern(shape, cdt, seed + 1), _pattern(shape, cdt, seed + 2)
    if t0:
        for cache in (kc, vc):
            _b(cache)[..., :t0, :] = _b(_enc(torch.randn(B, S - 1, heads, t0, 64, device='cuda', generator=g), cdt))
    return qkv, kc, vc


def _f64_reference(qkv, kc0, vc0, cdt, B, c, S, heads, t0):
    """(B, S-1, heads, c, 64) f64: q unrounded, keys / values < t0 decoded from the cache, the chunk's own through _enc; and max |V|."""
    ref, V = f64_cached_attention(qkv, kc0, vc0, B, c, S, heads, t0, own=lambda x: _dec(_enc(x.contiguous(), cdt)), cached=_dec)
    return ref, float(V.abs().max())


def _check_appended(qkv, kc, vc, kc0, vc0, cdt, B, c, S, heads, t0, tag):
    D = heads * 64
    for cache, cache0, o in ((kc, kc0, D), (vc, vc0, 2 * D)):
        want = _enc(_per(qkv[:, o:o + D], B, c, S, heads).contiguous(), cdt)
        assert torch.equal(_b(cache)[..., t0:t0 + c, :], _b(want)), tag                               # appended: the defining conversion, bit for bit
        assert torch.equal(_b(cache)[..., :t0, :], _b(cache0)[..., :t0, :]), tag                      # every other byte as it was
        assert torch.equal(_b(cache)[..., t0 + c:, :], _b(cache0)[..., t0 + c:, :]), tag


def _attn_case(pair, B, c, S, heads, T_total, t0, causal, seed):
    mode, cq, cdt = PAIRS[pair]
    D, dt = heads * 64, ops.tdtype(mode)
    qkv, kc, vc = _inputs(mode, cdt, B, c, S, heads, T_total, t0, seed)
    kc0, vc0 = kc.clone(), vc.clone()
    out = torch.full((B * c * S, D), float('nan'), device='cuda').to(dt)
    ops.attn_temporal_cached(mode, B, c, S, D, heads, causal, T_total, _i32([t0]), qkv, kc, vc, out, cache_dtype=cq)
    ref, vmax = _f64_reference(qkv, kc0, vc0, cdt, B, c, S, heads, t0)
    tag = (pair, B, c, S, heads, T_total, t0, causal)
    err = float((_per(out, B, c, S, heads).double() - ref).abs().max())
    if dt == torch.float32:
        assert err <= 2e-6 * float(ref.abs().max()), (tag, err)
    else:
        assert err <= ((2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11) + 1e-5) * vmax, (tag, err)
    assert bool((out.view(B, c, S, D)[:, :, 0] == 0).all()), tag                                       # slot-0 rows: exactly zero
    _check_appended(qkv, kc, vc, kc0, vc0, cdt, B, c, S, heads, t0, tag)


# ---------------------------------------------------------------------------------------------- (a) against the f64 restatement

@pytest.mark.parametrize('pair', list(PAIRS))
def test_compact_cached_attention_vs_f64(cuda, pair):
    G = _G(PAIRS[pair][0])
    seed = 0
    for T_total in (4, 30, 3 * 4 * G + 6):                      # the last: three full trips of the key loop and a partial one
        for c in (1, 3, G + 1):                                 # G + 1: the append loop of the stream kernel takes two trips
            for t0 in sorted({0, 1, 5, T_total - c}):
                if t0 < 0 or t0 + c > T_total:
                    continue
                for B in (1, 2):
                    for S in (2, 5):
                        for heads in (1, 2):
                            for causal in (1, 2):
                                seed += 1
                                _attn_case(pair, B, c, S, heads, T_total, t0, causal, seed)


# ---------------------------------------------------------------------------------------------- (b) rounding classes

SPECIALS = [1.0625, 1.1875, -1.0625, 2.0 ** -9, 1.5 * 2.0 ** -9, 2.0 ** -10, -2.0 ** -10, 2.5 * 2.0 ** -9, 448.0, -448.0, 449.0, 464.0, 1e4, -1e4,
            -0.0, 0.0]                                          # ties, subnormals (and half of the smallest), the clamp, signed zero


@pytest.mark.parametrize('pair', ['f32_fp8', 'bf16_fp8', 'fp16_fp8'])
def test_compact_cache_rounding_classes(cuda, pair):
    """Chunk K / V lines holding every rounding class of e4m3fn: the cache bytes are torch's; the one NaN, alone in a K line, makes NaN of
    exactly the frames that see the line."""
    mode, cq, cdt = PAIRS[pair]
    B, c, S, heads, T_total, t0 = 1, 3, 3, 2, 12, 2
    D, dt = heads * 64, ops.tdtype(mode)
    qkv, kc, vc = _inputs(mode, cdt, B, c, S, heads, T_total, t0, 77)
    row = lambda j, s: (0 * c + j) * S + s
    sp = torch.tensor(SPECIALS, device='cuda').to(dt)
    for o in (D, 2 * D):                                        # K and V of chunk frame 0, token slot 1: both heads, every channel a special
        qkv[row(0, 1), o:o + D] = sp.repeat(D // len(SPECIALS))
    qkv[row(1, 2), 2 * D:2 * D + 64] = sp.flip(0).repeat(4)     # V of frame 1, slot 2, head 0
    qkv[row(1, 2), D + 64:D + 128] = torch.randn(64, device='cuda').to(dt)
    qkv[row(1, 2), D + 64 + 37] = float('nan')                  # K of frame 1, slot 2, head 1: one NaN, the rest of the line finite
    kc0, vc0 = kc.clone(), vc.clone()
    out = torch.zeros(B * c * S, D, device='cuda').to(dt)
    ops.attn_temporal_cached(mode, B, c, S, D, heads, 1, T_total, _i32([t0]), qkv, kc, vc, out, cache_dtype=cq)
    _check_appended(qkv, kc, vc, kc0, vc0, cdt, B, c, S, heads, t0, pair)
    want_k = _enc(_per(qkv[:, D:2 * D], B, c, S, heads).contiguous(), cdt)
    assert int((_b(want_k) == 0x7f).sum()) == 1 and int((_b(kc)[0, 1, 1, t0 + 1] == 0x7f).sum()) == 1      # the NaN byte, where it belongs
    o = out.view(c, S, heads, 64).float()
    nan = torch.isnan(o)
    for j in range(c):
        for s in range(1, S):
            for h in range(heads):
                sees = (s, h) == (2, 1) and j >= 1              # frames 1 and 2 of (slot 2, head 1) attend to the NaN line
                assert bool(nan[j, s, h].all()) if sees else bool(torch.isfinite(o[j, s, h]).all()), (pair, j, s, h)


# ---------------------------------------------------------------------------------------------- (c) split invariance

def _run_split(pair, split, qkv_all, B, S, heads, T_total, causal, seed):
    """The stream form over all T_total frames in chunks `split`, on caches of random bytes -> (outputs [B, T_total, S, D], K, V)."""
    mode, cq, cdt = PAIRS[pair]
    D = heads * 64
    shape = (B, S - 1, heads, T_total, 64)
    kc, vc = _pattern(shape, cdt, seed), _pattern(shape, cdt, seed + 1)
    outs, t0 = [], 0
    for c in split:
        qkv = qkv_all[:, t0:t0 + c].reshape(B * c * S, 3 * D).contiguous()
        out = torch.full((B * c * S, D), float('nan'), device='cuda').to(qkv.dtype)
        ops.attn_temporal_cached(mode, B, c, S, D, heads, causal, T_total, _i32([t0]), qkv, kc, vc, out, cache_dtype=cq)
        outs.append(out.view(B, c, S, D)); t0 += c
    assert t0 == T_total
    return torch.cat(outs, 1), kc, vc


def _chunks(T, G):
    out, n = [], 0
    for c in [5, 3, G + 1, 1] * T:
        if n + c > T:
            break
        out.append(c); n += c
    return out + [1] * (T - n)


@pytest.mark.parametrize('pair', list(PAIRS))
def test_compact_cache_outputs_do_not_depend_on_the_chunking(cuda, pair):
    """Single frames, chunks (5, 3, G + 1, 1, ...) and one chunk: the same bits, outputs and caches.  (A kernel that used the chunk's own keys
    unrounded would differ between the three.)"""
    mode = PAIRS[pair][0]
    G = _G(mode)
    B, S, heads, T = 2, 3, 2, 3 * 4 * G + 6
    g = torch.Generator(device='cuda').manual_seed(5)
    qkv_all = torch.randn(B, T, S, 3 * heads * 64, device='cuda', generator=g).to(ops.tdtype(mode))
    for causal in (1, 2):
        want = _run_split(pair, [1] * T, qkv_all, B, S, heads, T, causal, 40)
        assert not torch.isnan(want[0].float()).any()
        for split in (_chunks(T, G), [T]):
            got = _run_split(pair, split, qkv_all, B, S, heads, T, causal, 40)
            assert torch.equal(got[0], want[0]), (pair, causal, split)
            assert torch.equal(_b(got[1]), _b(want[1])) and torch.equal(_b(got[2]), _b(want[2])), (pair, causal, split)


# ---------------------------------------------------------------------------------------------- (d) forms

def _sessions(pair, cs, t0s, slots, n_slots, S, heads, T_total, causal, seed):
    """n sessions, session r with cs[r] new frames at t0s[r] on slot slots[r] of caches [n_slots, ...] of random bytes (positions < t0 encoded
    randn).  Returns the flat qkv [F*S, 3D], the caches before the step, and per session the stream form's (out, K slot after, V slot after)."""
    mode, cq, cdt = PAIRS[pair]
    D = heads * 64
    g = torch.Generator(device='cuda').manual_seed(seed)
    shape = (n_slots, S - 1, heads, T_total, 64)
    kc0, vc0 = _pattern(shape, cdt, seed + 1), _pattern(shape, cdt, seed + 2)
    qkvs, refs = [], []
    for c, t0, sl in zip(cs, t0s, slots):
        for cache in (kc0, vc0):
            if t0:
                _b(cache)[sl, ..., :t0, :] = _b(_enc(torch.randn(S - 1, heads, t0, 64, device='cuda', generator=g), cdt))
        qkvs.append(torch.randn(c * S, 3 * D, device='cuda', generator=g).to(ops.tdtype(mode)))
    for c, t0, sl, qkv in zip(cs, t0s, slots, qkvs):
        k1, v1 = kc0[sl:sl + 1].clone(), vc0[sl:sl + 1].clone()
        out = torch.full((c * S, D), float('nan'), device='cuda').to(qkv.dtype)
        ops.attn_temporal_cached(mode, 1, c, S, D, heads, causal, T_total, _i32([t0]), qkv, k1, v1, out, cache_dtype=cq)
        assert not torch.isnan(out.float()).any()
        refs.append((out, k1[0], v1[0]))
    return torch.cat(qkvs, 0).contiguous(), kc0, vc0, refs


def _check_forms(out, kc, vc, kc0, vc0, cs, slots, S, refs, tag):
    f = 0
    for c, sl, (ro, rk, rv) in zip(cs, slots, refs):
        assert torch.equal(out[f * S:(f + c) * S], ro), tag
        assert torch.equal(_b(kc[sl]), _b(rk)) and torch.equal(_b(vc[sl]), _b(rv)), tag
        f += c
    for sl in set(range(kc.shape[0])) - set(slots):             # slots of no session: untouched
        assert torch.equal(_b(kc[sl]), _b(kc0[sl])) and torch.equal(_b(vc[sl]), _b(vc0[sl])), tag


@pytest.mark.parametrize('pair', list(PAIRS))
def test_compact_pool_and_ragged_forms_equal_the_stream_form(cuda, pair):
    mode, cq, cdt = PAIRS[pair]
    G = _G(mode)
    S, heads, T_total, n_slots = 5, 2, 3 * 4 * G + 6, 5
    D, dt = heads * 64, ops.tdtype(mode)
    slots = [3, 0, 4]                                           # shuffled, two slots unused
    for causal in (1, 2):
        for c in (1, 3, G + 1):                                 # pool rows: one chunk length, a t0 per row
            cs, t0s = [c] * 3, [T_total - c, 0, 4 * G + 1]
            qkv, kc0, vc0, refs = _sessions(pair, cs, t0s, slots, n_slots, S, heads, T_total, causal, 100 + c)
            kc, vc = kc0.clone(), vc0.clone()
            out = torch.full((3 * c * S, D), float('nan'), device='cuda').to(dt)
            ops.attn_temporal_pool(mode, 3, c, S, D, heads, causal, T_total, n_slots, _i32(t0s), _i32(slots), qkv, kc, vc, out, cache_dtype=cq)
            _check_forms(out, kc, vc, kc0, vc0, cs, slots, S, refs, (pair, 'pool', causal, c))
        cs, t0s = [3, G + 1, 1], [0, T_total - G - 1, 7]        # a ragged step
        qkv, kc0, vc0, refs = _sessions(pair, cs, t0s, slots, n_slots, S, heads, T_total, causal, 200)
        kc, vc = kc0.clone(), vc0.clone()
        tab = stream.ragged_tables(t0s, slots, cs)
        F = sum(cs)
        out = torch.full((F * S, D), float('nan'), device='cuda').to(dt)
        ops.attn_temporal_ragged(mode, 3, F, S, D, heads, causal, T_total, n_slots, *(_i32(tab[k]) for k in ('t0', 'slot', 'first', 'c', 'row_of_frame')),
                                 qkv, kc, vc, out, cache_dtype=cq)
        _check_forms(out, kc, vc, kc0, vc0, cs, slots, S, refs, (pair, 'ragged', causal))


def _to_pages(cache, page_of, n_pages, P, seed):
    """Contiguous caches [n, S-1, heads, T_total, 64] -> page arrays [n_pages, S-1, heads, P, 64] under page_of[r][q]; everything else random bytes."""
    return _pages_filled(cache, page_of, n_pages, P, _pattern((n_pages, *cache.shape[1:3], P, 64), cache.dtype, seed))


@pytest.mark.parametrize('P,T_total', [(1, 70), (4, 30)])
@pytest.mark.parametrize('pair', list(PAIRS))
def test_compact_paged_ragged_form_equals_the_stream_form(cuda, pair, P, T_total):
    """Non-monotone page ids; T_total = 70 at P = 1: a page table of more than 64 entries, sessions on both sides of entry 64."""
    mode, cq, cdt = PAIRS[pair]
    G = _G(mode)
    S, heads, n = 3, 2, 3
    D, dt = heads * 64, ops.tdtype(mode)
    cs, t0s = [3, G + 1, 1], [T_total - 8, 0, T_total - 1]      # (P = 1, T = 70: frames 62 .. 64 cross entry 64; frame 69 is wide)
    pps = -(-T_total // P)
    n_pages = n * pps + 3
    ids = [int(v) for v in np.random.default_rng(3).permutation(n_pages)[:n * pps]]
    page_of = [ids[r * pps:(r + 1) * pps] for r in range(n)]
    assert any(a > b for a, b in zip(page_of[0], page_of[0][1:]))
    for causal in (1, 2):
        qkv, kc0, vc0, refs = _sessions(pair, cs, t0s, [0, 1, 2], n, S, heads, T_total, causal, 300 + P)
        kp, vp = _to_pages(kc0, page_of, n_pages, P, 11), _to_pages(vc0, page_of, n_pages, P, 12)
        tab = stream.ragged_tables(t0s, [0, 1, 2], cs)
        F = sum(cs)
        out = torch.full((F * S, D), float('nan'), device='cuda').to(dt)
        ops.attn_temporal_ragged_paged(mode, n, F, S, D, heads, causal, T_total, n_pages, P, _i32(tab['t0']), _i32(sum(page_of, [])).view(n, pps),
                                       _i32(tab['first']), _i32(tab['c']), _i32(tab['row_of_frame']), qkv, kp, vp, out, cache_dtype=cq)
        f = 0
        for c, (ro, _, _) in zip(cs, refs):
            assert torch.equal(out[f * S:(f + c) * S], ro), (pair, P, causal)
            f += c
        k_after = torch.stack([_b(r[1]) for r in refs]).view(cdt); v_after = torch.stack([_b(r[2]) for r in refs]).view(cdt)
        # the pages gathered back equal the contiguous caches of the stream form; unowned pages and page tails in the same comparison
        assert torch.equal(_b(kp), _b(_to_pages(k_after, page_of, n_pages, P, 11))), (pair, P, causal)
        assert torch.equal(_b(vp), _b(_to_pages(v_after, page_of, n_pages, P, 12))), (pair, P, causal)


@pytest.mark.parametrize('mode', [ops.F32, ops.BF16, ops.FP16], ids=['f32', 'bf16', 'fp16'])
def test_storage_typed_cache_dtype_is_the_none_path(cuda, mode):
    """A cache_dtype that names the storage type goes through the *_cq entry points to the instantiation that None reaches: each of the four
    wrappers, called with None and with the storage type on clones of the same inputs, leaves the same bytes in the output and in both caches.
    Two sessions at t0 = 0 and 4 G + 1 (one whole cached trip of the key loop, one that crosses into the step's own keys, masked tail keys)."""
    cq, dt, G = (ops.F32 if mode == ops.F32 else ops.BF16), ops.tdtype(mode), _G(mode)
    S, heads, D, n_slots, P = 3, 1, 64, 3, 4
    T_total, t0s, slots = 8 * G + 8, [0, 4 * G + 1], [2, 0]
    g = torch.Generator(device='cuda').manual_seed(17)
    shape = (n_slots, S - 1, heads, T_total, 64)
    kc0, vc0 = _pattern(shape, dt, 18), _pattern(shape, dt, 19)              # random bytes; a session's positions < t0: encoded randn
    for cache in (kc0, vc0):
        _b(cache)[slots[1], ..., :t0s[1], :] = _b(_enc(torch.randn(S - 1, heads, t0s[1], 64, device='cuda', generator=g), dt))
    qkv_all = torch.randn(2 * 3 * S, 3 * D, device='cuda', generator=g).to(dt)

    def both(tag, rows, k0, v0, call):
        got = []
        for cache_dtype in (None, cq):
            k, v, out = k0.clone(), v0.clone(), torch.full((rows, D), float('nan'), device='cuda').to(dt)
            call(k, v, out, cache_dtype)
            assert not torch.isnan(out.float()).any(), (tag, cache_dtype)
            got.append((out, k, v))
        for a, b in zip(*got):
            assert torch.equal(_b(a), _b(b)), tag
        assert not torch.equal(_b(got[0][1]), _b(k0)) and not torch.equal(_b(got[0][2]), _b(v0)), tag         # (the step appended)

    for r, (t0, sl) in enumerate(zip(t0s, slots)):                              # stream form: one session a call, chunk length 3
        qkv = qkv_all[r * 3 * S:(r + 1) * 3 * S].clone()
        both(('stream', r), 3 * S, kc0[sl:sl + 1], vc0[sl:sl + 1], lambda k, v, out, cd: ops.attn_temporal_cached(
            mode, 1, 3, S, D, heads, 1, T_total, _i32([t0]), qkv, k, v, out, cache_dtype=cd))
    both('pool', 2 * 3 * S, kc0, vc0, lambda k, v, out, cd: ops.attn_temporal_pool(
        mode, 2, 3, S, D, heads, 1, T_total, n_slots, _i32(t0s), _i32(slots), qkv_all.clone(), k, v, out, cache_dtype=cd))
    cs = [3, 2]                                                                 # the ragged forms: chunk lengths (3, 2)
    F = sum(cs)
    qkv_r = qkv_all[:F * S]
    tab = {k: _i32(v) for k, v in stream.ragged_tables(t0s, slots, cs).items()}
    both('ragged', F * S, kc0, vc0, lambda k, v, out, cd: ops.attn_temporal_ragged(
        mode, 2, F, S, D, heads, 1, T_total, n_slots, tab['t0'], tab['slot'], tab['first'], tab['c'], tab['row_of_frame'], qkv_r.clone(), k, v, out,
        cache_dtype=cd))
    pps = -(-T_total // P)
    n_pages = 2 * pps + 3                                                       # spare pages, a shuffled table
    ids = [int(i) for i in np.random.default_rng(5).permutation(n_pages)[:2 * pps]]
    page_of = [ids[:pps], ids[pps:]]
    assert any(a > b for a, b in zip(page_of[1], page_of[1][1:]))
    kp0, vp0 = _to_pages(kc0[slots], page_of, n_pages, P, 20), _to_pages(vc0[slots], page_of, n_pages, P, 21)
    both('paged', F * S, kp0, vp0, lambda k, v, out, cd: ops.attn_temporal_ragged_paged(
        mode, 2, F, S, D, heads, 1, T_total, n_pages, P, tab['t0'], _i32(sum(page_of, [])).view(2, pps), tab['first'], tab['c'], tab['row_of_frame'],
        qkv_r.clone(), k, v, out, cache_dtype=cd))


# ---------------------------------------------------------------------------------------------- (e) refusals

def test_compact_entry_points_refuse_bad_arguments(cuda):
    """Each refusal names its argument and launches nothing: the output and the patterned caches stay as they were."""
    B, c, S, heads, T = 1, 1, 5, 1, 8
    t0 = _i32([0])
    for mode, dt in ((ops.F32, torch.float32), (ops.BF16, torch.bfloat16), (ops.FP16, torch.float16)):
        qkv = torch.zeros(B * c * S, 192, device='cuda', dtype=dt)
        out = torch.full((B * c * S, 64), 5.0, device='cuda', dtype=dt)
        kc = _pattern((B, S - 1, heads, T, 64), FP8T, 1); vc = _pattern((B, S - 1, heads, T, 64), FP8T, 2)
        kc0, vc0 = kc.clone(), vc.clone()
        run = lambda cq=ops.FP8, causal=1, T_total=T, D=64, k=kc, v=vc: ops.attn_temporal_cached(mode, B, c, S, D, heads, causal, T_total, t0, qkv, k, v, out,
                                                                                               cache_dtype=cq)
        refusals = [('cache_dtype must be', dict(cq=7)), ('cache_dtype must be', dict(cq=-1)), ('cache_dtype must be', dict(cq=ops.F32X3)),
                    ('causal', dict(causal=0)), ('causal', dict(causal=3)), ('T_total', dict(T_total=4096)), ('head_dim', dict(D=96)),
                    ('needs torch.float8_e4m3fn caches', dict(k=kc.view(torch.uint8))), ('needs torch.float8_e4m3fn caches', dict(v=vc.view(torch.int8)))]
        if mode == ops.F32:
            refusals += [('needs torch.bfloat16 caches', dict(cq=ops.BF16)), ('needs torch.float32 caches', dict(cq=ops.F32))]
        else:
            refusals += [('wider than the 16-bit storage', dict(cq=ops.F32)), (f'needs {dt} caches', dict(cq=ops.BF16))]
        for match, kw in refusals:
            with pytest.raises(TcowError, match=match):
                run(**kw)
            assert bool((out == 5.0).all()) and torch.equal(_b(kc), _b(kc0)) and torch.equal(_b(vc), _b(vc0)), (mode, match, kw)
        run()
        assert not bool((out == 5.0).any())
    # the other three wrappers reach the same refusal of the one entry point
    qkv = torch.zeros(S, 192, device='cuda'); out = torch.full((S, 64), 5.0, device='cuda')
    kc = _pattern((1, S - 1, 1, T, 64), FP8T, 3)
    one = _i32([0])
    with pytest.raises(TcowError, match='tcow_attn_temporal_step: cache_dtype must be'):
        ops.attn_temporal_pool(ops.F32, 1, 1, S, 64, 1, 1, T, 1, one, one, qkv, kc, kc.clone(), out, cache_dtype=9)
    with pytest.raises(TcowError, match='tcow_attn_temporal_step: cache_dtype must be'):
        ops.attn_temporal_ragged(ops.F32, 1, 1, S, 64, 1, 1, T, 1, one, one, one, _i32([1]), one, qkv, kc, kc.clone(), out, cache_dtype=9)
    with pytest.raises(TcowError, match='tcow_attn_temporal_step: cache_dtype must be'):
        ops.attn_temporal_ragged_paged(ops.F32, 1, 1, S, 64, 1, 1, T, 1, 8, one, one.view(1, 1), one, _i32([1]), one, qkv, kc, kc.clone(), out, cache_dtype=9)
    lib = _lib.lib()
    rec = _lib.StreamAttnArgs(shape=_lib.AttnShape(1, 1, S, 64, 1, 1, _lib.TCOW_BF16), cache_dtype=_lib.TCOW_F32, T_total=T, n_slots=1, t0_rows=one.data_ptr(),
                              slot_rows=one.data_ptr(), qkv=qkv.data_ptr(), k_cache=kc.data_ptr(), v_cache=kc.data_ptr(), out=out.data_ptr())      # the pool form
    assert lib.tcow_attn_temporal_step(None, ctypes.byref(rec)) != 0 and b'wider than the 16-bit storage' in lib.tcow_last_error()
    assert bool((out == 5.0).all())


@pytest.mark.parametrize('pair', list(PAIRS))
def test_compact_cache_bad_t0_slot_or_page_touches_no_cache_byte(cuda, pair):
    """NaN to the frame's own output rows, the other rows as without it, and every byte of the patterned caches as it was."""
    mode, cq, cdt = PAIRS[pair]
    S, heads, T_total, c = 3, 1, 12, 2
    D, dt = 64, ops.tdtype(mode)
    nan_rows = lambda o: bool(torch.isnan(o.float()).all())
    qkv, kc, vc = _inputs(mode, cdt, 2, c, S, heads, T_total, 3, 61)
    kc0, vc0 = kc.clone(), vc.clone()
    same = lambda: torch.equal(_b(kc), _b(kc0)) and torch.equal(_b(vc), _b(vc0))
    for t0 in (-1, T_total - c + 1, T_total):                   # the stream form: one t0 for all rows
        out = torch.zeros(2 * c * S, D, device='cuda').to(dt)
        ops.attn_temporal_cached(mode, 2, c, S, D, heads, 1, T_total, _i32([t0]), qkv, kc, vc, out, cache_dtype=cq)
        assert nan_rows(out) and same(), (pair, t0)
    clean_k, clean_v = kc0.clone(), vc0.clone()                 # the pool form: row 0 bad, row 1 good
    clean = torch.zeros(2 * c * S, D, device='cuda').to(dt)
    ops.attn_temporal_pool(mode, 2, c, S, D, heads, 1, T_total, 2, _i32([3, 3]), _i32([0, 1]), qkv, clean_k, clean_v, clean, cache_dtype=cq)
    for t0s, slots in (([T_total - 1, 3], [0, 1]), ([3, 3], [2, 1]), ([3, 3], [-1, 1])):
        out = torch.zeros(2 * c * S, D, device='cuda').to(dt)
        ops.attn_temporal_pool(mode, 2, c, S, D, heads, 1, T_total, 2, _i32(t0s), _i32(slots), qkv, kc, vc, out, cache_dtype=cq)
        assert nan_rows(out[:c * S]) and torch.equal(out[c * S:], clean[c * S:]), (pair, t0s, slots)
        assert torch.equal(_b(kc[0]), _b(kc0[0])) and torch.equal(_b(vc[0]), _b(vc0[0])), (pair, t0s, slots)
        assert torch.equal(_b(kc[1]), _b(clean_k[1])) and torch.equal(_b(vc[1]), _b(clean_v[1]))
        kc.copy_(kc0); vc.copy_(vc0)
    tab = stream.ragged_tables([3, 3], [0, 1], [c, c])          # the ragged and the paged form: session 0 bad
    tb = {k: _i32(v) for k, v in tab.items()}
    for t0s, slots in (([T_total - 1, 3], [0, 1]), ([3, 3], [5, 1])):
        out = torch.zeros(2 * c * S, D, device='cuda').to(dt)
        ops.attn_temporal_ragged(mode, 2, 2 * c, S, D, heads, 1, T_total, 2, _i32(t0s), _i32(slots), tb['first'], tb['c'], tb['row_of_frame'], qkv, kc, vc, out,
                                 cache_dtype=cq)
        assert nan_rows(out[:c * S]) and torch.equal(out[c * S:], clean[c * S:]), (pair, t0s, slots)
        assert torch.equal(_b(kc[0]), _b(kc0[0])) and torch.equal(_b(vc[0]), _b(vc0[0])), (pair, t0s, slots)
        kc.copy_(kc0); vc.copy_(vc0)
    P, pps = 4, 3
    page_of = [[4, 1, 5], [0, 3, 2]]
    kp0, vp0 = _to_pages(kc0, page_of, 6, P, 21), _to_pages(vc0, page_of, 6, P, 22)
    for bad_pages, t0s in (([[6, 1, 5], [0, 3, 2]], [3, 3]), ([[-1, 1, 5], [0, 3, 2]], [3, 3]), (page_of, [T_total - 1, 3])):
        kp, vp = kp0.clone(), vp0.clone()
        out = torch.zeros(2 * c * S, D, device='cuda').to(dt)
        ops.attn_temporal_ragged_paged(mode, 2, 2 * c, S, D, heads, 1, T_total, 6, P, _i32(t0s), _i32(sum(bad_pages, [])).view(2, pps), tb['first'], tb['c'],
                                       tb['row_of_frame'], qkv, kp, vp, out, cache_dtype=cq)
        assert nan_rows(out[:c * S]) and torch.equal(out[c * S:], clean[c * S:]), (pair, bad_pages, t0s)
        for pg in page_of[0] + [p for p in range(6) if p not in page_of[1]]:       # session 0's pages and the unowned ones: untouched
            assert torch.equal(_b(kp[pg]), _b(kp0[pg])) and torch.equal(_b(vp[pg]), _b(vp0[pg])), (pair, bad_pages, t0s, pg)


# ---------------------------------------------------------------------------------------------- module level

# every (precision, keyword) pair with a compact cache ('bf16' with precision 'bf16' is None; with 'fp16' it is refused: the host tests)
KEYWORDS = [('fp32', 'bf16'), ('fp32', 'fp8'), ('bf16x3', 'bf16'), ('bf16x3', 'fp8'), ('bf16', 'fp8'), ('fp16', 'fp8')]
TINY_T = 8


@functools.lru_cache(maxsize=None)
def _tiny_net(precision, ca):
    return synth_net(precision, TINY_T, 32, 48, embed_dim=128, depth=2, num_heads=2, ca=ca, seed=9)


@functools.lru_cache(maxsize=None)
def _tiny_clips():
    return synth_clips(2, TINY_T, 32, 48, seed=4)


def _stream_split(net, rgb, qm, split, **kw):
    st = net.stream(batch_size=rgb.shape[0], **kw)
    ms, fs, t = [], [], 0
    for c in split:
        m, f = st.step(rgb[:, :, t:t + c], qm[:, :, t:t + c])
        ms.append(m); fs.append(f); t += c
    return torch.cat(ms, 2), torch.cat(fs, 1), st


def _pool_run(pool, rgb, qm, ragged):
    """Two sessions, the second opened two frames late, every session to the last frame: step (one frame each) or step_ragged (chunks 3, 1, 2
    cycling) -> per session (mask, flags) over all frames."""
    T, n = TINY_T, rgb.shape[0]
    ids, got, tick = {}, {b: [] for b in range(n)}, 0
    while len(ids) < n or any(pool.frames_done(i) < T for i in ids.values()):
        if tick == 0:
            ids[0] = pool.open()
        if tick == 2:
            ids[1] = pool.open()
        rows = [b for b in ids if pool.frames_done(ids[b]) < T]
        t0s = [pool.frames_done(ids[b]) for b in rows]
        if ragged:
            cs = [min((3, 1, 2)[(tick + b) % 3], T - t0) for b, t0 in zip(rows, t0s)]
            ms, fls = pool.step_ragged([ids[b] for b in rows], [rgb[b:b + 1, :, t0:t0 + c] for b, t0, c in zip(rows, t0s, cs)],
                                       [qm[b:b + 1, :, t0:t0 + c] for b, t0, c in zip(rows, t0s, cs)])
            for k, b in enumerate(rows):
                got[b].append((ms[k], fls[k]))
        else:
            m, fl = pool.step([ids[b] for b in rows], torch.cat([rgb[b:b + 1, :, t0:t0 + 1] for b, t0 in zip(rows, t0s)], 0),
                              torch.cat([qm[b:b + 1, :, t0:t0 + 1] for b, t0 in zip(rows, t0s)], 0))
            for k, b in enumerate(rows):
                got[b].append((m[k:k + 1], fl[k:k + 1]))
        tick += 1
    for i in ids.values():
        pool.close(i)
    return (torch.cat([torch.cat([m for m, _ in got[b]], 2) for b in range(n)], 0), torch.cat([torch.cat([f for _, f in got[b]], 1) for b in range(n)], 0))


@pytest.mark.parametrize('ca', [1, 2])
@pytest.mark.parametrize('precision,keyword', KEYWORDS)
def test_compact_stream_forms_agree_bit_for_bit(cuda, precision, keyword, ca):
    """(f) frame by frame, in chunks, graph mode, a pool with step and with step_ragged, a paged pool: one result."""
    net = _tiny_net(precision, ca)
    rgb, qm = _tiny_clips()
    wm, wf, _ = _stream_split(net, rgb, qm, [1] * TINY_T, cache_dtype=keyword)
    assert torch.isfinite(wm).all() and torch.isfinite(wf).all()
    runs = {'chunks': _stream_split(net, rgb, qm, [3, 1, 2, 2], cache_dtype=keyword)[:2],
            'one chunk': _stream_split(net, rgb, qm, [TINY_T], cache_dtype=keyword)[:2],
            'graph': _stream_split(net, rgb, qm, [1] * TINY_T, cache_dtype=keyword, graph=True)[:2],
            'pool.step': _pool_run(net.stream_pool(2, cache_dtype=keyword), rgb, qm, False),
            'pool.step_ragged': _pool_run(net.stream_pool(3, cache_dtype=keyword), rgb, qm, True)}
    for P in (1, 4):
        pool = net.stream_pool(2, page_frames=P, cache_dtype=keyword)
        runs[f'paged P={P} step'] = _pool_run(pool, rgb, qm, False)
        assert pool.pages_free == pool.pages_total                # every page came back with close()
        runs[f'paged P={P} step_ragged'] = _pool_run(pool, rgb, qm, True)
        assert pool.pages_free == pool.pages_total
    for name, (m, f) in runs.items():
        assert torch.equal(m, wm) and torch.equal(f, wf), (precision, keyword, ca, name)


@pytest.mark.parametrize('precision,keyword', KEYWORDS)
def test_compact_stream_block0_cache_and_cache_bytes(cuda, precision, keyword):
    """(g) block 0's K / V depend on no cache, so its compact cache is the defining conversion of the None stream's, bit for bit: element type,
    layout and plumbing end to end.  cache_bytes follows from the shapes."""
    net = _tiny_net(precision, 1)
    rgb, qm = _tiny_clips()
    _, _, plain = _stream_split(net, rgb, qm, [3, 1, 4])
    _, _, comp = _stream_split(net, rgb, qm, [3, 1, 4], cache_dtype=keyword)
    cdt = FP8T if keyword == 'fp8' else torch.bfloat16
    st = comp._st
    assert st.k_cache.dtype == cdt == st.v_cache.dtype and st.k_cache.shape == plain._st.k_cache.shape == (2, 2, 6, 2, TINY_T, 64)
    assert plain._st.k_cache.dtype == ops.tdtype(net.seeker.mode) and plain._st.cq is None and st.cq == (ops.FP8 if keyword == 'fp8' else ops.BF16)
    for got, src in ((st.k_cache, plain._st.k_cache), (st.v_cache, plain._st.v_cache)):
        assert torch.equal(_b(got[0].contiguous()), _b(_enc(src[0], cdt)))
    es = 1 if keyword == 'fp8' else 2
    assert comp.cache_bytes == 2 * (2 * 2 * 6 * 2 * TINY_T * 64) * es + 2 * 2 * 128 * 4          # K and V [depth, rows, S-1, heads, T, 64] + f32 cls rows
    assert plain.cache_bytes == 2 * (2 * 2 * 6 * 2 * TINY_T * 64) * plain._st.k_cache.element_size() + 2 * 2 * 128 * 4
    pool = net.stream_pool(3, page_frames=4, pages=5, cache_dtype=keyword)
    assert pool._st.k_cache.dtype == cdt and pool.cache_bytes == 2 * (2 * 5 * 6 * 2 * 4 * 64) * es + 2 * 3 * 128 * 4


# (h) max |d| of the mask logits / flags of a frame-by-frame compact stream against the REFERENCE golden (not against the None stream), measured on
# an MI355X: profiles/stream_cache_dtype.json, the accuracy table of DESIGN.md section 9 ("Compact cache").  The bound asserted is twice the
# measured value: the result is a fixed function of the inputs, the factor only covers a compiler's reassociation.
#   (golden, precision, keyword): (mask logits, flags) as measured
MEASURED = {
    ('g1_cfg1_d256', 'fp32', 'bf16'): (1.8019e-05, 1.1213e-05),      # accuracy row g1 / fp32 / bf16
    ('g1_cfg1_d256', 'fp32', 'fp8'): (3.0341e-04, 1.8393e-04),      # accuracy row g1 / fp32 / fp8
    ('g1_cfg1_d256', 'bf16x3', 'bf16'): (1.7971e-05, 1.0651e-05),      # accuracy row g1 / bf16x3 / bf16
    ('g1_cfg1_d256', 'bf16x3', 'fp8'): (3.0339e-04, 1.9138e-04),      # accuracy row g1 / bf16x3 / fp8
    ('g1_cfg1_d256', 'bf16', 'fp8'): (5.5619e-04, 3.9053e-04),      # accuracy row g1 / bf16 / fp8
    ('g1_cfg1_d256', 'fp16', 'fp8'): (3.0718e-04, 1.8790e-04),      # accuracy row g1 / fp16 / fp8
    ('g2_ca2', 'fp32', 'bf16'): (1.7713e-05, 4.5747e-06),      # accuracy row g2 / fp32 / bf16
    ('g2_ca2', 'fp32', 'fp8'): (2.5287e-04, 2.8325e-04),      # accuracy row g2 / fp32 / fp8
    ('g2_ca2', 'bf16x3', 'bf16'): (1.7683e-05, 4.9621e-06),      # accuracy row g2 / bf16x3 / bf16
    ('g2_ca2', 'bf16x3', 'fp8'): (2.5294e-04, 2.8192e-04),      # accuracy row g2 / bf16x3 / fp8
    ('g2_ca2', 'bf16', 'fp8'): (4.8689e-04, 5.7383e-04),      # accuracy row g2 / bf16 / fp8
    ('g2_ca2', 'fp16', 'fp8'): (2.7418e-04, 2.6242e-04),      # accuracy row g2 / fp16 / fp8
}


@pytest.mark.parametrize('name', ['g1_cfg1_d256', 'g2_ca2'])
@pytest.mark.parametrize('precision,keyword', KEYWORDS)
def test_compact_stream_accuracy_vs_reference_golden(cuda, name, precision, keyword):
    meta, g = load_golden(name)
    cfg, sd, rgb, qm = golden_inputs(meta)
    net = build_hip_seeker(cfg, sd, precision).cuda().eval()
    rgb, qm = rgb.cuda(), qm.cuda()
    T = cfg['num_total_frames']
    om, fl, _ = _stream_split(net, rgb, qm, [1] * T, cache_dtype=keyword)
    pm, pf, _ = _stream_split(net, rgb, qm, [1] * T)
    d = float((om - torch.from_numpy(g['output_mask']).cuda()).abs().max())
    df = float((fl - torch.from_numpy(g['output_flags']).cuda()).abs().max())
    print(f'ACCURACY {name} {precision} {keyword} mask {d:.6e} flags {df:.6e}')
    assert not torch.equal(om, pm) and not torch.equal(fl, pf)                                   # the keyword does something
    md, mf = MEASURED[(name, precision, keyword)]
    assert d <= 2 * md and df <= 2 * mf, (d, df, md, mf)

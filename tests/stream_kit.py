"""Stream test kit: what the streaming tests (test_gpu_stream*.py, test_stream_*_host.py) share -- the nets and clips they run, the drivers of a
stream / pool / ragged step that also check shapes and counters, the table builders and launches of the kernel tests, the f64 restatement of
cached temporal attention and the comparison against a reference at the precision's tolerance.  Imports without a GPU; everything that
touches one does so when called.  The tolerance constants stay in test_gpu_seeker.py, which other suites share."""
import torch

from conftest import build_hip_seeker
from test_gpu_seeker import EXACT, bf16_flags_tol, bf16_tol, h16, h16f
from tcow_amd import ops, stream, synth

PRECISIONS = ['fp32', 'bf16', 'bf16x3', 'fp16']
MODES = {'f32': ops.F32, 'bf16': ops.BF16, 'fp16': ops.FP16, 'x3': ops.F32X3}


# ---------------------------------------------------------------------------------------------- nets and clips

def _net(ca=1, attention_type='divided_space_time'):
    """The CPU net of the host tests: the smallest at which every branch is taken."""
    from tcow_amd.seeker import Seeker
    return Seeker(None, num_total_frames=4, frame_height=32, frame_width=48, network_depth=1, embed_dim=64, num_heads=1, causal_attention=ca,
                  attention_type=attention_type, drop_path_rate=0.0, precision='fp32')


def synth_net(precision, T, H, W, embed_dim, depth, num_heads, ca=1, seed=11):
    """A Seeker of synthetic weights on the GPU, in eval mode."""
    cfg = synth.seeker_config(num_total_frames=T, frame_height=H, frame_width=W, embed_dim=embed_dim, depth=depth, num_heads=num_heads, causal_attention=ca)
    return build_hip_seeker(cfg, synth.make_state_dict(cfg, seed), precision).cuda().eval()


def synth_clips(n, T, H, W, seed=5):
    """n synthetic clips and their query masks on the GPU: rgb (n, 3, T, H, W), qm (n, 1, T, H, W)."""
    clip = synth.make_clip(n, T, H, W, seed=seed)
    rgb = torch.from_numpy(clip['rgb']).cuda()
    qm = torch.from_numpy(synth.make_query_mask(clip, 0, 0)).cuda()
    if qm.shape[0] != n:
        qm = qm.expand(n, -1, -1, -1, -1).contiguous()
    return rgb, qm


def _small_net(precision, ca=1, seed=11):
    """The config of test_stream_shared_rgb_and_batched_clips (its tolerances carry over): fp32 2e-5, bf16 1.5e-2."""
    return synth_net(precision, 4, 64, 96, 256, 2, 4, ca, seed)


def _small_clips(n, seed=5):
    rgb, qm = synth_clips(n, 4, 64, 96, seed)
    return [(rgb[b:b + 1], qm[b:b + 1]) for b in range(n)]


# ---------------------------------------------------------------------------------------------- streams and pools

def _splits(T, chunks):
    """Chunk lengths: `chunks` first, then single frames up to T."""
    out, n = [], 0
    for c in chunks:
        if n + c <= T:
            out.append(c); n += c
    return out + [1] * (T - n)


def _stream(net, rgb, qm, split, graph=False, Qs=1):
    """Stream the clip through a fresh stream in chunks `split`; the concatenated outputs."""
    st = net.stream(batch_size=rgb.shape[0], queries_per_clip=Qs, graph=graph)
    ms, fs, t = [], [], 0
    for c in split:
        m, f = st.step(rgb[:, :, t:t + c], qm[:, :, t:t + c])
        assert tuple(m.shape[2:3]) == (c,) and st.frames_done == t + c
        ms.append(m); fs.append(f); t += c
    return torch.cat(ms, 2), (torch.cat(fs, 1) if fs[0] is not None else None)


def _check_vs(om, fl, ref_mask, ref_flags, precision, gold_mask, gold_flags):
    d = float((om - ref_mask).abs().max())
    df = float((fl - ref_flags).abs().max())
    if precision in EXACT:
        assert d < EXACT[precision] and df < EXACT[precision], (d, df)
    else:
        assert d < h16(precision) * bf16_tol(gold_mask) and df < h16f(precision) * bf16_flags_tol(gold_flags), (d, df)


def _cat(parts):
    ms = torch.cat([m for m, _ in parts], 2)
    return ms, (torch.cat([f for _, f in parts], 1) if parts[0][1] is not None else None)


def _pool_step(pool, feeds, c=1):
    """feeds: [(session id, rgb (1,3,T,H,W), qm (1,1,T,H,W))] -> {id: (mask, flags)} of the next c frames of each, taken at its own counter."""
    ids = [f[0] for f in feeds]
    t = [pool.frames_done(i) for i in ids]
    rgb = torch.cat([f[1][:, :, t0:t0 + c] for f, t0 in zip(feeds, t)], 0)
    qm = torch.cat([f[2][:, :, t0:t0 + c] for f, t0 in zip(feeds, t)], 0)
    m, fl = pool.step(ids, rgb, qm)
    assert tuple(m.shape[:1]) == (len(ids),) and m.shape[2] == c and m.dtype == torch.float32
    for i, t0 in zip(ids, t):
        assert pool.frames_done(i) == t0 + c
    return {i: (m[k:k + 1], None if fl is None else fl[k:k + 1]) for k, i in enumerate(ids)}


def _ragged_step(pool, feeds, cs):
    """feeds: [(session id, rgb (1,3,T,H,W), qm (1,1,T,H,W))], cs: a chunk length per feed -> {id: (mask, flags)} of the next cs[k] frames of each,
    taken at its own counter."""
    ids = [f[0] for f in feeds]
    t = [pool.frames_done(i) for i in ids]
    rgbs = [f[1][:, :, t0:t0 + c] for f, t0, c in zip(feeds, t, cs)]
    qms = [f[2][:, :, t0:t0 + c] for f, t0, c in zip(feeds, t, cs)]
    ms, fls = pool.step_ragged(ids, rgbs, qms)
    assert len(ms) == len(ids) and (fls is None or len(fls) == len(ids))
    for k, (i, t0, c) in enumerate(zip(ids, t, cs)):
        assert ms[k].shape[0] == 1 and ms[k].shape[2] == c and ms[k].dtype == torch.float32 and tuple(ms[k].shape[3:]) == tuple(feeds[k][1].shape[3:])
        assert fls is None or tuple(fls[k].shape[:2]) == (1, c)
        assert pool.frames_done(i) == t0 + c
    return {i: (ms[k], None if fls is None else fls[k]) for k, i in enumerate(ids)}


def _run_ragged(pool, clips, T, opens, cycle=(1, 2, 3)):
    """Session b opens at step opens[b] and advances by chunk lengths cycling through `cycle`, offset per session and truncated at T."""
    ids, got, step = {}, {b: [] for b in range(len(clips))}, 0
    while len(ids) < len(clips) or any(pool.frames_done(i) < T for i in ids.values()):
        for b in range(len(clips)):
            if opens[b] == step:
                ids[b] = pool.open()
        rows = [b for b in ids if pool.frames_done(ids[b]) < T]
        if rows:
            cs = [min(cycle[(step + b) % len(cycle)], T - pool.frames_done(ids[b])) for b in rows]
            out = _ragged_step(pool, [(ids[b], *clips[b]) for b in rows], cs)
            for b in rows:
                got[b].append(out[ids[b]])
        step += 1
    return [_cat(got[b]) for b in range(len(clips))]


# ---------------------------------------------------------------------------------------------- kernels

def _i32(v, dev='cuda'):
    return torch.tensor(list(v), dtype=torch.int32, device=dev)


def _tables(t0s, slots, cs):
    tab = stream.ragged_tables(t0s, slots, cs)
    return {k: _i32(tab[k]) for k in ('t0', 'slot', 'first', 'c', 'row_of_frame')}, tab['first']


def _ragged_launch(mode, cs, S, heads, causal, T_total, n_slots, t0s, slots, qkv, kc, vc, fill=float('nan')):
    """One ragged launch into a NaN-poisoned (or `fill`ed) output; returns it."""
    F, D = sum(cs), heads * 64
    tb, _ = _tables(t0s, slots, cs)
    out = torch.full((F * S, D), fill, device=qkv.device).to(qkv.dtype)
    ops.attn_temporal_ragged(mode, len(cs), F, S, D, heads, causal, T_total, n_slots, tb['t0'], tb['slot'], tb['first'], tb['c'], tb['row_of_frame'],
                             qkv, kc, vc, out)
    return out


def _t0_sets(cs, T_total, rng):
    """The t0 lists of a chunk-length list: one session at 0 and one at T_total - c_r in each (a single session: one list per end)."""
    n = len(cs)
    if n == 1:
        return [[0], [T_total - cs[0]]]
    t0s = [int(rng.integers(0, T_total - c + 1)) for c in cs]
    a, b = (int(v) for v in rng.permutation(n)[:2])
    t0s[a], t0s[b] = 0, T_total - cs[b]
    return [t0s]


CHUNK_LISTS = [([1], 4), ([1], 30), ([3], 4), ([3], 30), ([1, 3, 2], 30), ([4, 1, 1], 30), ([9, 1], 30)]


def _to_pages(cache, page_of, n_pages, P, fill):
    """Contiguous caches [n, S-1, heads, T_total, 64] -> page arrays [n_pages, S-1, heads, P, 64] under page_of[r][q], copied byte for byte.
    Everything else holds `fill`: a number, or a tensor of the page arrays' shape and the cache's type (taken as it is: any bytes)."""
    n, Sm, heads, T_total, _ = cache.shape
    pages = fill.clone() if torch.is_tensor(fill) else torch.full((n_pages, Sm, heads, P, 64), fill, device=cache.device).to(cache.dtype)
    assert tuple(pages.shape) == (n_pages, Sm, heads, P, 64) and pages.dtype == cache.dtype
    for r in range(n):
        for q, pg in enumerate(page_of[r]):
            lo, hi = q * P, min(T_total, q * P + P)
            pages.view(torch.uint8)[pg, :, :, :hi - lo] = cache.view(torch.uint8)[r, :, :, lo:hi]
    return pages


def f64_cached_attention(qkv, kc0, vc0, B, c, S, heads, t0, own=torch.Tensor.double, cached=torch.Tensor.double):
    """The f64 restatement of cached temporal attention for B rows at frame t0: qkv [B*c*S, 3D] of the step, kc0 / vc0 [B, S-1, heads, T_total, 64]
    before the launch -> (ref (B, S-1, heads, c, 64), V (B, S-1, heads, t0 + c, 64)), both f64.  q enters as it is; `own` takes the chunk's own keys /
    values (B, S-1, heads, c, 64) to f64 and `cached` the cached ones of frames < t0 -- a compact cache rounds the former and decodes the latter."""
    D = heads * 64
    per = lambda x: x.view(B, c, S, heads, 64)[:, :, 1:].permute(0, 2, 3, 1, 4)            # slot 0 dropped: the layout of a cache
    Q = per(qkv[:, :D]).double()
    K = torch.cat([cached(kc0[..., :t0, :]), own(per(qkv[:, D:2 * D]))], 3); V = torch.cat([cached(vc0[..., :t0, :]), own(per(qkv[:, 2 * D:]))], 3)
    sc = Q @ K.transpose(-1, -2) / 8.0
    allowed = torch.arange(t0 + c, device=qkv.device)[None, :] <= (t0 + torch.arange(c, device=qkv.device))[:, None]
    return torch.softmax(sc.masked_fill(~allowed, float('-inf')), -1) @ V, V

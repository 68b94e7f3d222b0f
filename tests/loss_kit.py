"""Oracles and input generators of the once-per-step loss-side kernels (mask_loss.hip, snitch_weights.hip, query_masks.hip, metrics.hip), shared by
test_loss_kit_host.py (which proves them on the CPU) and test_gpu_loss_kernels.py (which holds the kernels to them).

The mask objective's oracle is a float64 closed form with an exact top-k: values that agree to 1e-12 relative are one tie group, and the group at the
k-th value shares the remaining r = k - above equally (the sub-gradient the kernel documents).  The generators make inputs whose distinct loss values are
far apart in f32 (test_loss_kit_host.py measures the gap), so the top-k set does not depend on how the device rounds expf / log1pf and the GPU tests can
demand every pixel, the ones at the cut included."""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

TIE_RTOL = 1e-12
Selection = namedtuple('Selection', 'valid n_sel n k tau_value above cnt_eq r')


# ------------------------------------------------------------------------------------------------ mask objective (tcow_hip.h: mask objective; loss.py:13-32, 164-225)
def pixel_values(x, t, focal):
    """float64 per-pixel loss value, d(value)/d(logit) and sigmoid: BCE with logits, or the sigmoid focal loss (alpha 0.25, gamma 2)."""
    p = torch.sigmoid(x)
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    if not focal:
        return bce, p - t, p
    q = 1.0 - (p * t + (1.0 - p) * (1.0 - t))
    at = 0.25 * t + 0.75 * (1.0 - t)
    dq = -p * (1.0 - p) * (2.0 * t - 1.0)
    return at * bce * q * q, at * (q * q * (p - t) + bce * 2.0 * q * dq), p


def topk_share(v, k):
    """Exact top-k of the 1-D float64 values v with ties shared: (share per element, tau_value, above, cnt_eq, r)."""
    assert 0 < k <= v.numel()
    tau = torch.sort(v, descending=True)[0][k - 1]
    tol = TIE_RTOL * abs(float(tau))
    tie = (v - tau).abs() <= tol
    gt = (v > tau) & ~tie
    above, cnt_eq = int(gt.sum()), int(tie.sum())
    r = k - above
    assert 0 < r <= cnt_eq
    return gt.double() + tie.double() * (r / cnt_eq), float(tau), above, cnt_eq, r


def mask_objective_ref(x, t, pixel_w, frame_w, T, weighted, aot, topk_frac, focal, loss_weight):
    """One channel of the mask objective on float64 CPU tensors x, t [n_frames, frame_len], pixel_w the same shape or None, frame_w [n_frames] or None
    (T = frames per sequence: only the frame count's divisibility depends on it).  Returns (loss, loss_weight * dloss/dx [n_frames, frame_len], Selection)."""
    assert x.dtype == torch.float64 and t.dtype == torch.float64 and x.shape == t.shape and x.dim() == 2 and x.shape[0] % T == 0
    nf, L = x.shape
    w = torch.ones_like(x)
    if pixel_w is not None:
        w = w * pixel_w.double()
    if frame_w is not None:
        w = w * frame_w.double()[:, None]
    fsel = (w != 0).any(dim=1)
    n_sel, n = int(fsel.sum()) * L, nf * L
    grad = torch.zeros_like(x)
    if n_sel == 0 or float(w.mean()) < 1e-4:
        return 0.0, grad, Selection(False, n_sel, n, 0, None, 0, 0, 0)
    xs, ts, ws = x[fsel].reshape(-1), t[fsel].reshape(-1), w[fsel].reshape(-1)
    val, dval, p = pixel_values(xs, ts, focal)
    custom = (val * ws).sum() / n_sel
    g = ws * dval / n_sel
    k = int(topk_frac * n_sel)
    rec = Selection(True, n_sel, n, k, None, 0, 0, 0)
    if aot > 0.0:
        v = val * ws if weighted else val
        dv = ws * dval if weighted else dval
        if k == n_sel:
            share = torch.ones_like(v)
        else:
            share, tau, above, cnt_eq, r = topk_share(v, k)
            rec = Selection(True, n_sel, n, k, tau, above, cnt_eq, r)
        boot = (share * v).sum() / k
        gboot = share * dv / k
        if weighted:
            jac, gjac = boot, gboot
        elif float(ts.mean()) >= 1e-6:
            num = (p * ts).sum()
            D = p.sum() + ts.sum() - num + 0.1
            jac = 1.0 - num / D
            gjac = -(ts * D - num * (1.0 - ts)) / (D * D) * p * (1.0 - p)
        else:
            jac, gjac = 0.0, torch.zeros_like(v)
        loss = (boot + jac) / 2.0 * aot + custom * (1.0 - aot)
        g = (gboot + gjac) / 2.0 * aot + g * (1.0 - aot)
    else:
        loss = custom
    sf = math.sqrt(n_sel / n)
    grad[fsel] = (g * (sf * loss_weight)).reshape(-1, L)
    return float(loss) * sf, grad, rec


def value_keys(x, t, w, weighted):
    """What decides a pixel's top-k value: (x, t), and the weight when the values are weighted.  [n, 2 or 3] float64."""
    cols = [x.reshape(-1).double(), t.reshape(-1).double()] + ([w.reshape(-1).double()] if weighted else [])
    return torch.stack(cols, dim=1)


def f32_ulps_apart(v):
    """Smallest distance, in f32 units in the last place, between two different positive float64 values of v once rounded to f32
    (positive floats order like their bit patterns); values inside one tie group count as one."""
    s = torch.sort(v.reshape(-1))[0]
    first = torch.ones_like(s, dtype=torch.bool)
    first[1:] = (s[1:] - s[:-1]) > TIE_RTOL * s[1:].abs()
    b = s[first].float().view(torch.int32).long()
    return int((b[1:] - b[:-1]).min()) if b.numel() > 1 else None


LEVELS_T0 = [-4.75 + 0.5 * i for i in range(20)]       # odd multiples of 0.25: bce(x, 0) = bce(-x, 1), and no -x of these is among LEVELS_T1
LEVELS_T1 = [-4.5 + 0.5 * i for i in range(19)]


def _pick(g, choices, shape):
    c = torch.tensor(choices, dtype=torch.float32)
    return c[torch.randint(0, len(choices), shape, generator=g)]


def levels(n_frames, frame_len, seed, weights=None, soft=False):
    """x, t, pixel_w f32 [n_frames, frame_len]: logits from two interleaved level sets in [-5, 5), one per target value, weights from a small set
    (None: ones).  Every (x, t, w) has many exact copies, so the k-th value always sits inside a tie group.  soft: targets 0.25 / 0.75."""
    g = torch.Generator().manual_seed(seed)
    shape = (n_frames, frame_len)
    hi = torch.randint(0, 2, shape, generator=g).bool()
    x = torch.where(hi, _pick(g, LEVELS_T1, shape), _pick(g, LEVELS_T0, shape))
    t = torch.where(hi, torch.tensor(0.75 if soft else 1.0), torch.tensor(0.25 if soft else 0.0))
    w = _pick(g, list(weights), shape) if weights is not None else torch.ones(shape)
    return x, t, w


CLUSTER_X = [2.0 + j * 2.0 ** -15 for j in range(16)]
CLUSTER_ABOVE = [3.25, 3.75, 4.25, 4.75]


def cluster(n_frames, frame_len, seed):
    """x, t, pixel_w (ones): 30 % of the pixels well above a cluster (t = 0, x >= 3.25), 30 % well below it (t = 0 at x <= -0.25, t = 1 at x >= 0.5), the
    other 40 % at t = 0, x = 2 + j 2^-15, j = 0 .. 15: sixteen loss values inside one level-1 bin of the radix select, a few per level-3 bin."""
    g = torch.Generator().manual_seed(seed)
    n = n_frames * frame_len
    n_above, n_below = int(0.3 * n), int(0.3 * n)
    n_cl = n - n_above - n_below
    x = torch.cat([_pick(g, CLUSTER_ABOVE, (n_above,)), _pick(g, CLUSTER_X, (n_cl,)), _pick(g, LEVELS_T0[:10], (n_below - n_below // 2,)),
                   _pick(g, LEVELS_T1[10:], (n_below // 2,))])
    t = torch.zeros(n); t[n - n_below // 2:] = 1.0
    perm = torch.randperm(n, generator=g)
    return x[perm].reshape(n_frames, frame_len), t[perm].reshape(n_frames, frame_len), torch.ones(n_frames, frame_len)


def all_tied(n_frames, frame_len, x=1.5, t=0.0, w=1.5):
    shape = (n_frames, frame_len)
    return torch.full(shape, x), torch.full(shape, t), torch.full(shape, w)


def zero_frame_weights(n_seq, T, seed, choices=(0.5, 1.0, 2.0)):
    """frame_w f32 [n_seq * T] from `choices` with two whole frames and the tail of the last sequence at zero (fewer where the geometry has no room)."""
    g = torch.Generator().manual_seed(seed)
    fw = _pick(g, list(choices), (n_seq, T))
    if n_seq * T >= 4:
        fw.view(-1)[1] = 0.0
        fw.view(-1)[n_seq * T // 2] = 0.0
        fw[-1, (T + 1) // 2:] = 0.0
    return fw.reshape(-1)


def frac_for_k(k, n_sel):
    """A topk_frac whose int(topk_frac * n_sel) is k."""
    f = (k + 0.5) / n_sel
    assert int(f * n_sel) == k
    return f


def frac_at_group_end(x, t, w, frame_w, weighted, focal, lo=0.2):
    """topk_frac for which the k-th value is the LAST of its tie group (r == cnt_eq): k = the number of values in the largest groups that together first
    exceed the fraction `lo` of the selected pixels."""
    wv = w.double() * (frame_w.double()[:, None] if frame_w is not None else 1.0)
    sel = (wv != 0).any(dim=1)
    v = pixel_values(x.double()[sel].reshape(-1), t.double()[sel].reshape(-1), focal)[0]
    if weighted:
        v = v * wv[sel].reshape(-1)
    s = torch.sort(v, descending=True)[0]
    n_sel = s.numel()
    k = int(lo * n_sel)
    while k < n_sel and (s[k - 1] - s[k]).abs() <= TIE_RTOL * s[k - 1].abs():
        k += 1
    assert 0 < k < n_sel
    return frac_for_k(k, n_sel)


# ------------------------------------------------------------------------------------------------ snitch pixel weights (loss.py:85-148 x loss.py:55-83)
def snitch_window(H, W):
    """(k, r, bit path) of tcow_snitch_weights: k = odd(int(sqrt(HW) / 12)), r = k // 2; the 64-bit row-mask path needs whole words per row, the 2r + 1
    rows of a window inside one wave and whole waves inside the frame."""
    k = int(math.sqrt(H * W) / 12.0)
    if k % 2 == 0:
        k += 1
    r = k // 2
    return k, r, (W % 64 == 0 and r <= 31 and (H * W) % 256 == 0)


def box_dilate(m, r):
    """(2r + 1)^2 box dilation of the bool maps m [F, H, W], zero padded."""
    if r == 0:
        return m.clone()
    x = m.float()[:, None]
    x = F.max_pool2d(x, kernel_size=(2 * r + 1, 1), stride=1, padding=(r, 0))
    return F.max_pool2d(x, kernel_size=(1, 2 * r + 1), stride=1, padding=(0, r))[:, 0] > 0


def class_factors(pos_count, n_pixels):
    """(neg factor, pos factor) as f32 values held in float64: fractions in f32 with the 5 % floor, powers 0.7 / -0.3 of their ratio in float64."""
    f32 = np.float32
    pf = max(f32(pos_count) / f32(n_pixels), f32(0.05)); nf = max(f32(n_pixels - pos_count) / f32(n_pixels), f32(0.05))
    p, n = float(pf), float(nf)
    if p > n:
        pc, nc = (n / p) ** 0.7, (n / p) ** -0.3
    else:
        pc, nc = (p / n) ** -0.3, (p / n) ** 0.7
    return float(f32(nc)), float(f32(pc))


def snitch_band(t0, r):
    return box_dilate(t0 > 0, r) & ~(t0 >= 0.5)


SNITCH_SHAPES = [(8, 8, 3), (3, 64, 3), (48, 80, 3), (64, 128, 3), (37, 256, 3), (240, 320, 1), (704, 832, 1), (768, 768, 1)]      # (H, W, frames)


def snitch_weights_ref(t0, ptr, frame_w, pos_count, class_balancing, factor, band=None):
    """t0 [F, H, W] f32 (channel 0 of the target), ptr [F, H, W] u8, frame_w [F] f32 -> float64 [F, H, W] (products not rounded), and the band
    (band: snitch_band(t0, r) when the caller has it already)."""
    Fn, H, W = t0.shape
    _, r, _ = snitch_window(H, W)
    w = torch.ones(t0.shape, dtype=torch.float64)
    if class_balancing:
        nc, pc = class_factors(pos_count, Fn * H * W)
        w = torch.where(t0 == 0, w * nc, w)
        w = torch.where(t0 == 1, w * pc, w)
    w = torch.where(ptr != 0, w * 2.0, w)
    if factor <= 1.0:
        band = torch.zeros_like(t0, dtype=torch.bool)
    elif band is None:
        band = snitch_band(t0, r)
    w = torch.where(band, w * float(np.float32(factor)), w)
    return w * frame_w.double()[:, None, None], band


def snitch_inputs(H, W, frames, seed):
    """Planted targets [frames, H, W] f32 and a ptr map u8 (about 10 % non-zero).  Frame 0: single pixels at the four corners and at columns 63, 64, 127, 128
    where W allows, sparse random pixels (about a quarter of the frame inside some window), a few pixels of value 0.25.  With three frames: frame 1 empty,
    frame 2 full."""
    g = torch.Generator().manual_seed(seed)
    _, r, _ = snitch_window(H, W)
    t = torch.zeros(frames, H, W)
    f0 = t[0]
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        f0[y, x] = 1.0
    for i, c in enumerate((63, 64, 127, 128)):
        if c < W:
            f0[(H // 3 + i * (2 * r + 2)) % H, c] = 1.0
    m = max(2, int(0.22 * H * W / (2 * r + 1) ** 2)) if r > 0 else max(2, H * W // 8)
    idx = torch.randint(0, H * W, (m,), generator=g)
    f0.view(-1)[idx] = 1.0
    soft = torch.randint(0, H * W, (3,), generator=g)
    f0.view(-1)[soft] = 0.25
    if frames >= 3:
        t[2] = 1.0
    ptr = (torch.rand(frames, H, W, generator=g) < 0.1).to(torch.uint8) * 3
    return t, ptr


# ------------------------------------------------------------------------------------------------ query / target masks (tcow_hip.h: query / target masks)
def build_masks_ref(segm, div, qidx, front, cont, qt):
    """segm (B,1,T,H,W) u8, div (B,M,T,H,W) u8, qidx (B,Q), front / cont (B,Q,T) (-1 = none) ->
    query_mask (B,Q,1,T,H,W) f32, target (B,Q,3,T,H,W) f32, snitch_occl_by_ptr (B,Q,1,T,H,W) u8, counts int [1 + 2Q] (flags as 0 / 1)."""
    B, _, T, H, W = segm.shape
    Q = qidx.shape[1]
    qm = torch.zeros(B, Q, 1, T, H, W); tg = torch.zeros(B, Q, 3, T, H, W); pt = torch.zeros(B, Q, 1, T, H, W, dtype=torch.uint8)
    for b in range(B):
        for q in range(Q):
            qi = int(qidx[b, q])
            for t in range(T):
                seg = segm[b, 0, t]
                isq = seg == qi + 1
                amodal = div[b, qi, t] == 1
                if t == qt:
                    qm[b, q, 0, t] = isq.float()
                tg[b, q, 0, t] = amodal.float()
                for ch, idx in ((1, int(front[b, q, t])), (2, int(cont[b, q, t]))):
                    if idx >= 0:
                        tg[b, q, ch, t] = (div[b, idx, t] == 1).float()
                pt[b, q, 0, t] = torch.where(amodal & ~isq, seg, torch.zeros_like(seg))
    counts = torch.zeros(1 + 2 * Q, dtype=torch.int64)
    counts[0] = int(tg[:, :, 0].sum())
    for q in range(Q):
        counts[1 + 2 * q] = int(bool(qm[:, q].any())); counts[2 + 2 * q] = int(bool(tg[:, q].any()))
    return qm, tg, pt, counts


def mask_inputs(B, M, T, HW, seed):
    """segm (B,1,T,1,HW) u8 in 0 .. M and div (B,M,T,1,HW) u8 bits; instance M - 1 has no pixels in frame T - 1."""
    g = torch.Generator().manual_seed(seed)
    segm = torch.randint(0, M + 1, (B, 1, T, 1, HW), generator=g, dtype=torch.uint8)
    div = (torch.rand(B, M, T, 1, HW, generator=g) > 0.5).to(torch.uint8)
    div[:, M - 1, T - 1] = 0
    return segm, div


def decision_inputs(B, K, T, Q, seed):
    """occl_fracs (B,K,T,3), dag (B,T,K,K,3), sel (B,Q) int64 with frames of every kind: above the occlusion threshold for everyone (t = 1), without a
    container candidate (t = 0), with exactly one (t = 2, where T allows), with occluded-by maxima below half the threshold (t = 3, where T allows)."""
    g = torch.Generator().manual_seed(seed)
    occl = torch.rand(B, K, T, 3, generator=g)
    occl[:, :, 1 % T, 0] = 0.99
    dag = torch.rand(B, T, K, K, 3, generator=g)
    dag[:, 0, :, :, 0] *= 0.5
    if T > 2:
        dag[:, 2, :, 3, 0] = 0.9; dag[:, 2, :, :3, 0] *= 0.5; dag[:, 2, :, 4:, 0] *= 0.5
    if T > 3:
        dag[:, 3, :, :, 2] *= 0.3
    sel = torch.stack([torch.randperm(K, generator=g)[:Q] for _ in range(B)])
    return occl, dag, sel


# ------------------------------------------------------------------------------------------------ IoU areas and means (eval/metrics.py:19-20, 55-113)
def iou_counts_ref(logits, target):
    """[F, L] f32 -> int64 [F, 3]: |target|, |output & target|, |output | target| with output = logit > 0, target = value > 0.5."""
    o, g = logits > 0, target > 0.5
    return torch.stack([g.sum(1), (o & g).sum(1), (o | g).sum(1)], dim=1)


def iou_inputs(n_frames, frame_len, seed):
    """Logits with exact +0.0 / -0.0 and targets with exact 0.5 among them: both comparisons are strict."""
    g = torch.Generator().manual_seed(seed)
    x = _pick(g, [-1.5, -0.0, 0.0, 2.0 ** -100, 0.75], (n_frames, frame_len))
    t = _pick(g, [0.0, 0.5, 0.5 + 2.0 ** -24, 1.0], (n_frames, frame_len))
    return x, t


def iou_means_ref(counts):
    """counts (n_seq, C, T, 3) int -> (mean float64 [6] with -1 where nothing is selected, count int64 [6]) in the order snitch_iou, occl_mask_iou,
    cont_mask_iou, snitch_during_vis_iou, snitch_during_occl_iou, snitch_during_cont_iou; channels beyond C count as absent."""
    n_seq, C, T, _ = counts.shape
    c = counts.double()
    iou = c[..., 1] / (c[..., 2] + 1e-7)
    has = counts[..., 0] > 0
    no = torch.zeros(n_seq, T, dtype=torch.bool)
    h = [has[:, i] if i < C else no for i in range(3)]
    sels = [h[0], h[1], h[2], (h[0] & ~h[1]) if C >= 2 else no, h[0] & h[1], h[0] & h[2]]
    vals = [iou[:, 0], iou[:, 1] if C >= 2 else None, iou[:, 2] if C >= 3 else None, iou[:, 0], iou[:, 0], iou[:, 0]]
    mean = torch.full((6,), -1.0, dtype=torch.float64); cnt = torch.zeros(6, dtype=torch.int64)
    for i, (s, v) in enumerate(zip(sels, vals)):
        cnt[i] = int(s.sum())
        if cnt[i] > 0:
            mean[i] = float(v[s].sum()) / int(cnt[i])
    return mean, cnt


def iou_tables(n_seq, C, T, seed):
    """Random area tables int32 (n_seq, C, T, 3) with planted cases: about a quarter of the frames with an empty target per channel, zero unions, and (for
    C >= 3, seed odd) a container channel with no target at all -- its selectors must come out as mean -1, count 0."""
    g = torch.Generator().manual_seed(seed)
    shape = (n_seq, C, T)
    area = torch.randint(1, 5000, shape, generator=g)
    area = torch.where(torch.rand(shape, generator=g) < 0.25, torch.zeros_like(area), area)
    union = area + torch.randint(0, 3000, shape, generator=g)
    inter = (torch.rand(shape, generator=g) * (area + 1)).long().clamp(max=area)
    zero_u = torch.rand(shape, generator=g) < 0.1
    union = torch.where(zero_u, torch.zeros_like(union), union); inter = torch.where(zero_u, torch.zeros_like(inter), inter)
    if C >= 3 and seed % 2 == 1:
        area[:, 2] = 0
    return torch.stack([area, inter, union], dim=-1).to(torch.int32)


# ------------------------------------------------------------------------------------------------ the mask-objective cases of test_gpu_loss_kernels.py
GEOMS = {'1x1x4': (1, 1, 4),                        # the smallest possible call
         '2x3x240': (2, 3, 240),                    # a partly filled first trip
         '2x2x9228': (2, 2, 4 * (2 * 1024 + 259)),  # three workgroups per frame, the last with one full and one ragged trip
         '52x5x8': (52, 5, 8)}                      # 260 frames and 260 partial blocks: the second trips of the control, scan and final folds
MaskCase = namedtuple('MaskCase', 'geom gen wmode weighted focal aot frac zero')
# gen: levels75 / levels2 (pixel weights from {0.75, 1, 1.5} / {0.5, 1, 2}), soft (levels75 with targets 0.25 / 0.75), cluster, all_tied
# wmode: pw / fw / both / none, or the two invalid jobs: tiny (mean weight below 1e-4), nofw (no frame selected)
# frac: topk_frac, or 'edge' = the k-th value is the last of its tie group (r == cnt_eq)
_FORMS = [('levels75', 'pw', 0, 0, 0.8, 0.5, False), ('levels75', 'both', 1, 0, 0.8, 0.15, True), ('levels2', 'fw', 1, 1, 0.8, 0.5, True),
          ('levels2', 'pw', 1, 1, 0.8, 0.15, False), ('levels75', 'none', 0, 1, 0.8, 0.5, False), ('levels75', 'pw', 0, 0, 0.8, 1.0, False),
          ('levels2', 'both', 1, 0, 0.0, 0.5, True), ('cluster', 'none', 0, 0, 0.8, 0.5, False), ('cluster', 'none', 0, 1, 0.8, 0.5, False),
          ('cluster', 'fw', 1, 0, 0.8, 0.5, True), ('all_tied', 'pw', 0, 0, 0.8, 0.5, False), ('soft', 'pw', 1, 0, 0.8, 0.5, False),
          ('soft', 'none', 0, 1, 0.8, 0.15, False), ('levels75', 'pw', 0, 0, 0.8, 'edge', False), ('levels2', 'both', 1, 1, 0.8, 'edge', True)]
MASK_CASES = ([MaskCase(g, *f) for g in ('2x3x240', '2x2x9228') for f in _FORMS]
              + [MaskCase('1x1x4', 'all_tied', 'pw', 0, 0, 0.8, 0.5, False), MaskCase('1x1x4', 'levels75', 'pw', 0, 0, 0.8, 1.0, False),
                 MaskCase('1x1x4', 'levels2', 'both', 1, 1, 0.8, 0.5, False)]
              + [MaskCase('52x5x8', *f) for f in (_FORMS[0], _FORMS[1], _FORMS[2], _FORMS[5], _FORMS[6], _FORMS[13])]
              + [MaskCase('2x3x240', 'levels75', 'tiny', 1, 0, 0.8, 0.5, False), MaskCase('2x3x240', 'levels75', 'nofw', 0, 0, 0.8, 0.5, False)])


def batch_cases(geom):
    """Three jobs of one geometry for tcow_mask_loss_batch: the first and the last run the radix select, the middle one (topk_frac = 1) does not."""
    last = MaskCase(geom, 'cluster', 'fw', 1, 0, 0.8, 0.5, True) if geom != '52x5x8' else MaskCase(geom, 'levels2', 'both', 1, 1, 0.8, 0.15, True)
    return [MaskCase(geom, 'levels75', 'pw', 0, 0, 0.8, 0.5, False), MaskCase(geom, 'levels2', 'fw', 1, 1, 0.8, 1.0, True), last]


BATCH_GEOMS = ['2x3x240', '2x2x9228', '52x5x8']
ALL_MASK_CASES = MASK_CASES + [c for g in BATCH_GEOMS for c in batch_cases(g) if c not in MASK_CASES]      # everything the GPU tests hand to the kernel


def case_id(c):
    return '-'.join(str(v) for v in c)


def mask_case_inputs(c, seed=0):
    """The f32 inputs of a MaskCase: dict(n_seq, T, L, x, t [n_frames, L], pw [n_frames, L] | None, fw [n_frames] | None, frac)."""
    n_seq, T, L = GEOMS[c.geom]
    nf = n_seq * T
    seed = seed + sum(ord(ch) for ch in case_id(c))
    if c.gen == 'cluster':
        x, t, w = cluster(nf, L, seed)
    elif c.gen == 'all_tied':
        x, t, w = all_tied(nf, L)
    else:
        x, t, w = levels(nf, L, seed, weights=(0.5, 1.0, 2.0) if c.gen == 'levels2' else (0.75, 1.0, 1.5), soft=c.gen == 'soft')
    pw = w if c.wmode in ('pw', 'both') else None
    fw = None
    if c.wmode in ('fw', 'both'):
        choices = (1.0,) if c.gen == 'cluster' else (0.5, 1.0, 2.0) if c.gen == 'levels2' else (1.0, 2.0)
        fw = zero_frame_weights(n_seq, T, seed + 1, choices) if c.zero else _pick(torch.Generator().manual_seed(seed + 1), list(choices), (nf,))
    if c.wmode == 'tiny':
        pw = torch.full((nf, L), 5e-5)
    if c.wmode == 'nofw':
        fw = torch.zeros(nf)
    frac = c.frac
    if frac == 'edge':
        frac = frac_at_group_end(x, t, pw if pw is not None else torch.ones(nf, L), fw, c.weighted, c.focal)
    return dict(n_seq=n_seq, T=T, L=L, x=x, t=t, pw=pw, fw=fw, frac=frac)


def mask_case_ref(c, d, loss_weight=1.0):
    f64 = lambda v: None if v is None else v.double()
    return mask_objective_ref(d['x'].double(), d['t'].double(), f64(d['pw']), f64(d['fw']), d['T'], c.weighted, c.aot, d['frac'], c.focal, loss_weight)

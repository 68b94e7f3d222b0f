"""CPU proofs of tests/loss_kit.py, the oracles and generators that test_gpu_loss_kernels.py holds the loss-side kernels to: the float64 mask objective
against float64 autograd of TcowLosses.mask_loss, the separation of the generators' loss values (which is what lets the GPU tests demand every pixel at the
top-k cut), and the snitch-weight / mask-builder / IoU restatements against the package's tensor paths."""
import math

import numpy as np
import pytest
import torch

import loss_kit as K
from conftest import load_golden
from tcow_amd.tcow_loss import TcowLosses, default_args

MIN_ULPS = 64
RADIX_CASES = [c for c in K.ALL_MASK_CASES if c.aot > 0 and c.frac != 1.0 and c.wmode not in ('tiny', 'nofw')]


def _selected(c, d):
    """(values float64 that the top-k orders, their keys, the oracle's record) over the selected frames of a case."""
    x, t = d['x'].double(), d['t'].double()
    w = (d['pw'].double() if d['pw'] is not None else torch.ones_like(x)) * (d['fw'].double()[:, None] if d['fw'] is not None else 1.0)
    sel = (w != 0).any(dim=1)
    v = K.pixel_values(x[sel].reshape(-1), t[sel].reshape(-1), c.focal)[0]
    if c.weighted:
        v = v * w[sel].reshape(-1)
    return v, K.value_keys(x[sel], t[sel], w[sel], c.weighted), K.mask_case_ref(c, d)[2]


@pytest.mark.parametrize('c', RADIX_CASES, ids=K.case_id)
def test_distinct_values_are_far_apart_in_f32(c):
    """Equal float64 value iff equal (x, t[, w]); different values, rounded to f32, at least 64 ulps apart; 0 < k < n_sel."""
    v, keys, rec = _selected(c, K.mask_case_inputs(c))
    s = torch.sort(v)[0]
    n_values = 1 + int(((s[1:] - s[:-1]) > K.TIE_RTOL * s[1:].abs()).sum())
    assert n_values == torch.unique(keys, dim=0).shape[0]
    gap = K.f32_ulps_apart(v)
    assert gap is None or gap >= MIN_ULPS, gap
    assert gap is not None or c.gen == 'all_tied'
    assert 0 < rec.k < rec.n_sel and 0 < rec.r <= rec.cnt_eq
    assert rec.cnt_eq == int(((v - rec.tau_value).abs() <= K.TIE_RTOL * rec.tau_value).sum()) and rec.above == int((v > rec.tau_value * (1 + 2 * K.TIE_RTOL)).sum())
    if c.gen != 'all_tied' and GEOM_PIXELS[c.geom] >= 1000:
        assert rec.cnt_eq > 1                                               # the k-th value sits inside a tie group


GEOM_PIXELS = {g: n * T * L for g, (n, T, L) in K.GEOMS.items()}


def test_measured_gaps_of_the_generators():
    """The smallest gaps of the generators, pinned: levels BCE / focal unweighted, levels x {0.75, 1, 1.5}, cluster BCE / focal."""
    x, t, w = K.levels(4, 4096, 1, weights=(0.75, 1.0, 1.5))
    xd, td, wd = x.double().reshape(-1), t.double().reshape(-1), w.double().reshape(-1)
    assert K.f32_ulps_apart(K.pixel_values(xd, td, False)[0]) == 515928 and K.f32_ulps_apart(K.pixel_values(xd, td, True)[0]) == 184155
    assert K.f32_ulps_apart(K.pixel_values(xd, td, False)[0] * wd) == 18625 and K.f32_ulps_apart(K.pixel_values(xd, td, True)[0] * wd) == 14885
    x, t, _ = K.cluster(4, 4096, 1)
    cl = (x >= 2.0) & (x < 2.001) & (t == 0)
    xc, tc = x[cl].double(), t[cl].double()
    assert float(tc.max()) == 0.0 and torch.unique(xc).numel() == 16
    assert K.f32_ulps_apart(K.pixel_values(xc, tc, False)[0]) == 112 and K.f32_ulps_apart(K.pixel_values(xc, tc, True)[0]) == 206


@pytest.mark.parametrize('c', [c for c in RADIX_CASES if c.gen == 'cluster'], ids=K.case_id)
def test_cluster_threshold_is_decided_by_the_third_radix_level(c):
    """The sixteen cluster values share their top 11 bits, spread over several second-level bins, and at least two DIFFERENT values share the threshold's
    top 22 bits: only the last 9 bits tell the k-th value from its neighbour."""
    v, _, rec = _selected(c, K.mask_case_inputs(c))
    tau_bits = int(torch.tensor(rec.tau_value, dtype=torch.float64).float().view(torch.int32))
    b = torch.unique(v.float()).view(torch.int32).long()
    cl = b[(b >> 20) == (tau_bits >> 20)]
    in_cluster = torch.unique(v[(v > 2.0 * (0.3 if c.focal else 1.0)) & (v < 2.2)].float()).numel()
    assert in_cluster == 16 and cl.numel() == 16
    assert torch.unique(cl >> 9).numel() >= 4
    assert int(((cl >> 9) == (tau_bits >> 9)).sum()) >= 2


def test_selection_coverage():
    """Across the cases: the k-th value strictly inside its tie group (0 < r < cnt_eq) and at its end (r == cnt_eq), in both loss forms."""
    recs = [(c, K.mask_case_ref(c, K.mask_case_inputs(c))[2]) for c in RADIX_CASES]
    for focal in (0, 1):
        assert any(0 < r.r < r.cnt_eq for c, r in recs if c.focal == focal) and any(r.r == r.cnt_eq and r.cnt_eq > 1 for c, r in recs if c.focal == focal)
    assert {c.wmode for c in K.MASK_CASES} >= {'pw', 'fw', 'both', 'none', 'tiny', 'nofw'}
    assert {c.frac for c in K.MASK_CASES} >= {1.0, 0.5, 0.15} and {c.aot for c in K.MASK_CASES} == {0.8, 0.0}
    assert {(c.weighted, c.focal) for c in K.MASK_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c.gen for c in K.MASK_CASES} == {'levels75', 'levels2', 'soft', 'cluster', 'all_tied'} and {c.geom for c in K.MASK_CASES} == set(K.GEOMS)
    for c in K.MASK_CASES:
        if c.zero and c.geom != '1x1x4':
            fw = K.mask_case_inputs(c)['fw'].reshape(K.GEOMS[c.geom][0], K.GEOMS[c.geom][1])
            assert int((fw == 0).sum()) >= 3 and float(fw[-1, -1]) == 0.0 and float(fw[0, 0]) != 0.0          # two whole frames and the tail of the last sequence


def _autograd(x, t, w, progress, weighted, focal, aot):
    """float64 autograd of the tensor restatement of loss.py:164-225 on [n_frames, L] inputs."""
    xs = x.clone().requires_grad_(True)
    lo = TcowLosses(default_args(focal_loss=bool(focal), aot_loss=aot), fused=False)
    shape = (1, 1, x.shape[0], 1, x.shape[1])
    loss = lo.mask_loss(xs.reshape(shape), t.reshape(shape), w.reshape(shape), progress, bool(weighted))
    if loss.requires_grad:
        loss.backward()
    return float(loss.detach()), xs.grad if xs.grad is not None else torch.zeros_like(x)


def _frac(progress):
    return min(max(1.0 - progress * 8.5, 0.15), 1.0)


@pytest.mark.parametrize('weighted', [0, 1])
@pytest.mark.parametrize('focal', [0, 1])
@pytest.mark.parametrize('aot', [0.8, 0.0])
def test_oracle_equals_autograd_on_untied_inputs(weighted, focal, aot):
    g = torch.Generator().manual_seed(7 + weighted + 2 * focal)
    nf, L, T = 6, 40, 3
    x = torch.randn(nf, L, generator=g, dtype=torch.float64) * 2.5
    t = (torch.rand(nf, L, generator=g) > 0.6).double()
    pw = torch.rand(nf, L, generator=g, dtype=torch.float64) + 0.5
    for zero in (False, True):
        fw = torch.rand(nf, generator=g, dtype=torch.float64) + 0.5
        if zero:
            fw[1] = 0.0; fw[4:] = 0.0
        for progress in (0.0, 1.0 / 17.0, 1.0):
            frac = _frac(progress)
            assert abs(frac - (1.0, 0.5, 0.15)[(0.0, 1.0 / 17.0, 1.0).index(progress)]) < 1e-12
            want_l, want_g = _autograd(x, t, pw * fw[:, None], progress, weighted, focal, aot)
            got_l, got_g, rec = K.mask_objective_ref(x, t, pw, fw, T, weighted, aot, frac, focal, 1.0)
            assert abs(got_l - want_l) <= 1e-12 * abs(want_l)
            assert float((got_g - want_g).abs().max()) <= 1e-12 * float(want_g.abs().max())
            assert rec.n_sel == (3 if zero else 6) * L and rec.k == int(frac * rec.n_sel)
            assert aot == 0.0 or frac == 1.0 or (rec.cnt_eq == 1 and rec.r == 1)
    l2, g2, _ = K.mask_objective_ref(x, t, pw, None, T, weighted, aot, 0.5, focal, 0.25)          # loss_weight scales the gradient only
    l1, g1, _ = K.mask_objective_ref(x, t, pw, None, T, weighted, aot, 0.5, focal, 1.0)
    assert l1 == l2 and torch.equal(g2, g1 * 0.25)
    assert K.mask_objective_ref(x, t, pw * 5e-5, None, T, weighted, aot, 0.5, focal, 1.0)[0] == 0.0
    assert K.mask_objective_ref(x, t, pw, fw * 0, T, weighted, aot, 0.5, focal, 1.0)[0] == 0.0
    le, ge, _ = K.mask_objective_ref(x, torch.zeros_like(t), pw, None, T, weighted, aot, 0.5, focal, 1.0)      # empty target: no Tversky term
    we, wg = _autograd(x, torch.zeros_like(t), pw, 1.0 / 17.0, weighted, focal, aot)
    assert abs(le - we) <= 1e-12 * abs(we) and float((ge - wg).abs().max()) <= 1e-12 * float(wg.abs().max())


@pytest.mark.parametrize('c', [c for c in RADIX_CASES if c.geom in ('2x3x240', '1x1x4', '52x5x8') and c.frac in (0.5, 0.15)], ids=K.case_id)
def test_oracle_equals_autograd_outside_the_tie_group(c):
    """Tied inputs: torch.topk gives r arbitrary members of the threshold group the whole weight, the oracle gives every member r / cnt_eq.  Same loss, same
    gradient outside the group, same gradient sum inside it."""
    d = K.mask_case_inputs(c)
    x, t = d['x'].double(), d['t'].double()
    w = (d['pw'].double() if d['pw'] is not None else torch.ones_like(x)) * (d['fw'].double()[:, None] if d['fw'] is not None else 1.0)
    progress = {0.5: 1.0 / 17.0, 0.15: 1.0}[c.frac]
    want_l, want_g = _autograd(x, t, w, progress, c.weighted, c.focal, c.aot)
    got_l, got_g, rec = K.mask_case_ref(c, d)
    assert abs(got_l - want_l) <= 1e-12 * abs(want_l)
    v = K.pixel_values(x, t, c.focal)[0] * (w if c.weighted else 1.0)
    group = ((v - rec.tau_value).abs() <= K.TIE_RTOL * rec.tau_value) & (w != 0).any(dim=1, keepdim=True)
    assert int(group.sum()) == rec.cnt_eq
    scale = float(want_g.abs().max())
    assert float(((got_g - want_g).abs() * ~group).max()) <= 1e-12 * scale
    assert abs(float(got_g[group].sum() - want_g[group].sum())) <= 1e-12 * scale * rec.cnt_eq
    if 0 < rec.r < rec.cnt_eq:
        assert float((got_g - want_g).abs().max()) > 1e-6 * scale            # (and inside the group the two do differ)


# ------------------------------------------------------------------------------------------------ snitch weights
def test_snitch_window_arithmetic():
    want = {(8, 8): (1, 0, False), (3, 64): (1, 0, False), (48, 80): (5, 2, False), (64, 128): (7, 3, True), (37, 256): (9, 4, True), (240, 320): (23, 11, True),
            (704, 832): (63, 31, True), (768, 768): (65, 32, False), (64, 64): (5, 2, True)}
    for (H, W), w in want.items():
        assert K.snitch_window(H, W) == w, (H, W)


@pytest.mark.parametrize('H,W', [(48, 80), (64, 64)])
@pytest.mark.parametrize('class_balancing,factor', [(True, 3.0), (False, 3.0), (True, 1.0)])
def test_snitch_reference_equals_pixel_weights(H, W, class_balancing, factor):
    """Binary targets (the tensor path counts target == 0 as the negatives, the kernel and this reference n - positives: the same on binary targets)."""
    t, ptr = K.snitch_inputs(H, W, 3, 4)
    t = (t >= 0.5).float()
    g = torch.Generator().manual_seed(1)
    fw = torch.rand(3, generator=g) + 0.5
    L = TcowLosses(default_args(class_balancing=class_balancing, hard_negative_factor=factor))
    want = fw[None, None, :, None, None] * L.pixel_weights(t[None, None], ptr[None, None])
    got, band = K.snitch_weights_ref(t, ptr, fw, int((t == 1).sum()), class_balancing, factor)
    assert float((got.float() - want[0, 0]).abs().max()) <= 4e-7 * float(want.max())
    assert factor == 1.0 or 0 < int(band.sum()) < band.numel()


@pytest.mark.parametrize('H,W', [(48, 80), (64, 128), (37, 256)])
def test_snitch_band_is_the_full_box_dilation(H, W):
    """The separable dilation of the kit against one (2r + 1) x (2r + 1) max-pool; pixels of value 0.25 dilate and stay inside the band."""
    t, _ = K.snitch_inputs(H, W, 3, 4)
    _, r, _ = K.snitch_window(H, W)
    full = torch.nn.functional.max_pool2d((t > 0).float()[:, None], kernel_size=2 * r + 1, stride=1, padding=r)[:, 0] > 0
    band = K.snitch_band(t, r)
    assert torch.equal(band, full & ~(t >= 0.5))
    assert bool(band[t == 0.25].all()) and int((t == 0.25).sum()) > 0 and not bool(band[2].any()) and not bool(band[1].any())


@pytest.mark.parametrize('H,W,frames', K.SNITCH_SHAPES)
def test_snitch_inputs_cover_their_band(H, W, frames):
    t, ptr = K.snitch_inputs(H, W, frames, 4)
    _, r, _ = K.snitch_window(H, W)
    band = K.snitch_band(t[:1], r)
    if r == 0:
        assert torch.equal(band, t[:1] == 0.25)                             # no window: only the soft pixels are "dilated but not target"
    else:
        assert 0.05 <= float(band.float().mean()) <= 0.5, float(band.float().mean())
    assert all(float(t[0, y, x]) > 0 for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)))
    assert all(float(t[0, :, c].max()) == 1.0 for c in (63, 64, 127, 128) if c < W)
    assert 0.05 < float((ptr != 0).float().mean()) < 0.15
    assert frames == 1 or (float(t[1].max()) == 0.0 and float(t[2].min()) == 1.0)


def test_class_factors_reach_every_branch():
    n = 10000
    (n1, p1), (n2, p2), (n3, p3), (n4, p4) = (K.class_factors(p, n) for p in (7000, 2000, 100, 9900))
    assert p1 < 1 < n1 and n2 < 1 < p2
    f32 = np.float32
    floor = float(f32(0.05))
    assert p3 == float(f32((floor / float(f32(0.99))) ** -0.3)) and p3 != float(f32((float(f32(0.01)) / float(f32(0.99))) ** -0.3))      # the 5 % floor, positive side
    assert n4 == float(f32((floor / float(f32(0.99))) ** -0.3)) and p4 == float(f32((floor / float(f32(0.99))) ** 0.7))                   # ... and negative side
    assert abs(p2 - float(np.float32((0.2 / 0.8) ** -0.3))) < 1e-6 and abs(n2 - float(np.float32((0.2 / 0.8) ** 0.7))) < 1e-6


# ------------------------------------------------------------------------------------------------ masks and tables
def test_mask_reference_equals_the_tensor_path_on_the_golden_inputs():
    from tcow_amd import synth
    from tcow_amd.pipeline import fill_kubric_query_target_mask_flags, frame_decisions
    _, g = load_golden('g5_pipeline_cfg1')
    data = synth.to_torch_tree(synth.make_kubric_batch(2, 4, 64, 64, seed=900), None)
    kr = data['kubric_retval']; tr = kr['traject_retval_tf']
    segm, div, occl, dag = kr['pv_segm_tf'], kr['pv_div_segm_tf'], tr['occl_fracs_tf'], tr['occl_cont_dag_tf']
    qt = int(tr['query_time'][0].item())
    sel = torch.from_numpy(g['train::sel_query_inds'])
    args = default_args()
    fi, ci, ids, flags = frame_decisions(occl, dag, sel, args)
    qm, tg, pt, counts = K.build_masks_ref(segm, div, sel, fi, ci, qt)
    for q in range(sel.shape[1]):
        wq, wp, wi, wt, wf = fill_kubric_query_target_mask_flags(segm, div, sel[:, q], qt, occl, dag, args)
        assert torch.equal(qm[:, q], wq) and torch.equal(pt[:, q], wp) and torch.equal(tg[:, q], wt) and torch.equal(ids[:, q], wi) and torch.equal(flags[:, q], wf)
        assert int(counts[1 + 2 * q]) == int(bool(wq.any())) and int(counts[2 + 2 * q]) == int(bool(wt.any()))
    assert np.array_equal(tg.numpy(), g['train::target_mask']) and np.array_equal(qm.numpy(), g['train::seeker_query_mask'])
    assert int(counts[0]) == int((tg[:, :, 0] == 1).sum()) > 0


def test_mask_and_decision_inputs_reach_every_kind_of_frame():
    from tcow_amd.pipeline import frame_decisions
    occl, dag, sel = K.decision_inputs(2, 4, 3, 2, 0)
    fi, ci, _, _ = frame_decisions(occl, dag, sel, default_args())
    assert int((fi >= 0).sum()) > 0 and int((fi < 0).sum()) > 0 and int((ci >= 0).sum()) > 0 and int((ci < 0).sum()) > 0
    occl, dag, sel = K.decision_inputs(3, 6, 23, 4, 0)
    fi, ci, _, _ = frame_decisions(occl, dag, sel, default_args())
    assert int((fi >= 0).sum()) > 0 and int((fi < 0).sum()) > 0 and int((ci >= 0).sum()) > 0 and int((ci < 0).sum()) > 0
    segm, div = K.mask_inputs(2, 4, 3, 16, 0)
    assert int(div[:, 3, 2].sum()) == 0 and int(segm.max()) == 4 and int(segm.min()) == 0


# ------------------------------------------------------------------------------------------------ IoU
def test_iou_references_equal_the_tensor_path():
    """calculate_metrics_mask_track on images whose areas are a count table gives the kit's means; the inputs hold the values both strict comparisons turn on."""
    from tcow_amd.metrics import calculate_metrics_mask_track
    x, t = K.iou_inputs(7, 1036, 0)
    assert int((x == 0).sum()) > 0 and int((t == 0.5).sum()) > 0 and bool((torch.signbit(x) & (x == 0)).any())
    c = K.iou_counts_ref(x, t)
    assert torch.equal(c[:, 0], (t > 0.5).sum(1)) and int(c[:, 0].sum()) < int((t >= 0.5).sum()) and int(c[:, 2].sum()) < int(((x >= 0) | (t > 0.5)).sum())
    g = torch.Generator().manual_seed(0)
    for C in (1, 2, 3):
        out = torch.randn(2, 3, C, 5, 6, 8, generator=g); tgt = (torch.rand(2, 3, C, 5, 6, 8, generator=g) > 0.6).float()
        tgt[0, 1] = 0; tgt[1, :, C - 1, 2:] = 0
        cnt = K.iou_counts_ref(out.reshape(-1, 48), tgt.reshape(-1, 48)).reshape(6, C, 5, 3)
        mean, n = K.iou_means_ref(cnt)
        m = calculate_metrics_mask_track(out, tgt)
        for i, k in enumerate(('snitch_iou', 'occl_mask_iou', 'cont_mask_iou', 'snitch_during_vis_iou', 'snitch_during_occl_iou', 'snitch_during_cont_iou')):
            assert int(m['count_' + k]) == int(n[i]) and abs(float(m['mean_' + k]) - float(mean[i])) <= 2.0 ** -23 * abs(float(mean[i])), (C, k)


@pytest.mark.parametrize('C', [1, 2, 3])
def test_iou_tables_hold_the_planted_cases(C):
    tab = K.iou_tables(24, C, 25, 1)
    assert int((tab[:, 0, :, 0] == 0).sum()) > 0 and int(((tab[..., 2] == 0) & (tab[..., 0] > 0)).sum()) > 0
    mean, n = K.iou_means_ref(tab)
    if C == 3:
        assert float(mean[2]) == -1.0 and int(n[2]) == 0 and float(mean[5]) == -1.0 and int(n[5]) == 0
    if C == 1:
        assert [int(v) for v in n[1:]] == [0] * 5 and int(n[0]) > 0
    assert math.isfinite(float(mean[0])) and 0 < float(mean[0]) < 1

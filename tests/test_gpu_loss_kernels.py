"""The once-per-step loss-side kernels against the float64 oracles of tests/loss_kit.py (proved on the CPU by test_loss_kit_host.py), through the C ABI,
with every output inside a sentinel-filled buffer:

  tcow_mask_loss / tcow_mask_loss_batch   every pixel of the logit gradient, the ones at the top-k cut included (the inputs' loss values are >= 64 f32 ulps
                                          apart or bit-identical, so the selected set cannot depend on the device's rounding); one workgroup per frame, three
                                          with a ragged last trip, 260 frames / partial blocks; pixel and frame weights, zero-weight frames, the two invalid
                                          jobs, three different sequence strides, dlogits / total absent; the same call twice bit for bit
  tcow_snitch_weights                     byte path and 64-bit row-mask path across word boundaries (nw = 2 .. 13, r = 0 .. 32), exact with power-of-two factors
  tcow_build_masks / tcow_build_query_masks   one, two and eight workgroups per frame with a ragged second grid-stride trip; 276 table rows
  tcow_iou_counts / tcow_iou_means        one to four loop trips, ragged; 1 .. 600 frames

Bounds: the loss within 2e-6 max(1, |ref|), every gradient pixel within 2e-5 (BCE) / 3e-5 (focal) of the largest reference gradient -- the project's
existing bounds, here without exception pixels (measured on the MI355X: at most 5.4e-7 and 2.6e-7 of the scale); snitch weights 1e-6 relative (four f32 products and a one-ulp pow factor); IoU means 2^-23 relative
(a float64 sum rounded once; snitch weights measured at most 7.4e-8).  No bound had to be re-measured or widened."""
import ctypes

import numpy as np
import pytest
import torch

import loss_kit as K
from kernel_forms import assert_guarded_flat, bits, guarded_flat

pytestmark = pytest.mark.gpu
NAN = float('nan')


def _api():
    from tcow_amd import _lib, ops
    return _lib, _lib.lib(), ops._stream()


def _tail_intact(buf, n, what):
    """The float32 sentinel buffer `buf` past its first n elements (n may count 4-byte units of an integer view) is untouched."""
    assert torch.equal(bits(buf)[n:], bits(torch.full_like(buf, NAN))[n:]), f'{what}: wrote past the end'


def _guarded_words(n_words, dev):
    """A guarded buffer for integer / byte outputs: n_words 4-byte units + spare, all holding the NaN sentinel's bits."""
    return guarded_flat(n_words, torch.float32, dev)[0]


def _scratch(nbytes, dev):
    return torch.full((max(int(nbytes), 1),), 0xA5, dtype=torch.uint8, device=dev)          # (a workspace is never assumed to be zeroed)


# ------------------------------------------------------------------------------------------------ tcow_mask_loss / tcow_mask_loss_batch
LOGIT_CH, TARGET_CH, GRAD_CH = 4, 5, 3          # three images with three different sequence strides; job c uses channel c + 1, c + 2, c


def _run_mask(dev, jobs, n_seq, T, L, total0=0.375, with_dl=True, with_total=True):
    """jobs: dicts (x, t, pw, fw f32 CPU tensors or None; weighted, focal, aot, frac, lw).  One tcow_mask_loss call for one job, tcow_mask_loss_batch for more.
    Returns (losses f32 CPU [n jobs], gradient image f32 CPU (n_seq, 3, T, L) or None, total f32 CPU scalar or None); the guards are checked here."""
    _lib, lib, st = _api()
    nf = n_seq * T
    lo = torch.full((n_seq, LOGIT_CH, T, L), NAN, device=dev); tg = torch.full((n_seq, TARGET_CH, T, L), NAN, device=dev)
    n_dl = n_seq * GRAD_CH * T * L
    dl_buf, dl = guarded_flat(n_dl, torch.float32, dev)
    loss_buf, loss = guarded_flat(len(jobs), torch.float32, dev)
    tot_buf, tot = guarded_flat(1, torch.float32, dev)
    tot[0] = total0
    keep = []
    arr = (_lib.MaskLossArgs * len(jobs))()
    for c, j in enumerate(jobs):
        lo[:, c + 1] = j['x'].reshape(n_seq, T, L).to(dev); tg[:, c + 2] = j['t'].reshape(n_seq, T, L).to(dev)
        pw = j['pw'].contiguous().to(dev) if j['pw'] is not None else None
        fw = j['fw'].contiguous().to(dev) if j['fw'] is not None else None
        nbytes = lib.tcow_mask_loss_workspace_bytes_for(nf, L, float(j['frac']), float(j['aot']))
        assert nbytes <= lib.tcow_mask_loss_workspace_bytes(nf, L)
        ws = _scratch(nbytes, dev)
        keep += [pw, fw, ws]
        arr[c] = _lib.MaskLossArgs(nf, L, T, lo.data_ptr() + 4 * (c + 1) * T * L, LOGIT_CH * T * L, tg.data_ptr() + 4 * (c + 2) * T * L, TARGET_CH * T * L,
                                   pw.data_ptr() if pw is not None else None, fw.data_ptr() if fw is not None else None, int(j['weighted']), float(j['aot']),
                                   float(j['frac']), float(j['lw']), loss.data_ptr() + 4 * c, tot.data_ptr() if with_total else None,
                                   (dl.data_ptr() + 4 * c * T * L) if with_dl else None, GRAD_CH * T * L, ws.data_ptr(), ws.numel(), int(j['focal']))
    if len(jobs) == 1:
        _lib.check(lib.tcow_mask_loss(st, ctypes.byref(arr[0])), 'tcow_mask_loss', lib)
    else:
        _lib.check(lib.tcow_mask_loss_batch(st, arr, len(jobs)), 'tcow_mask_loss_batch', lib)
    torch.cuda.synchronize()
    assert_guarded_flat(loss_buf, len(jobs), 'loss')
    img = dl.view(n_seq, GRAD_CH, T, L)
    _tail_intact(dl_buf, n_dl, 'dlogits')
    sentinel = bits(torch.full_like(img[:, 0], NAN))
    for c in range(GRAD_CH):
        if c >= len(jobs) or not with_dl:
            assert torch.equal(bits(img[:, c]), sentinel), f'dlogits: channel {c} of the image is not this call\'s'
        else:
            assert bool(torch.isfinite(img[:, c]).all()), f'dlogits: channel {c} has unwritten (or non-finite) pixels'
    if with_total:
        assert_guarded_flat(tot_buf, 1, 'total')
    else:
        _tail_intact(tot_buf, 1, 'total'); assert float(tot[0]) == total0
    del keep
    return loss.cpu(), (img.cpu() if with_dl else None), (tot.cpu()[0] if with_total else None)


def _job(c, d, lw):
    return dict(x=d['x'], t=d['t'], pw=d['pw'], fw=d['fw'], weighted=c.weighted, focal=c.focal, aot=c.aot, frac=d['frac'], lw=lw)


def _check_job(name, c, d, lw, got_loss, got_grad):
    """One job's loss and gradient [n_frames, L] against the oracle; figures printed before they are asserted."""
    ref_loss, ref_grad, rec = K.mask_case_ref(c, d, loss_weight=float(np.float32(lw)))
    err_l = abs(float(got_loss) - ref_loss)
    print(f'{name}: loss {float(got_loss):.9g} ref {ref_loss:.9g} |d| {err_l:.3g} (bound {2e-6 * max(1.0, abs(ref_loss)):.3g}); k {rec.k} of {rec.n_sel}, '
          f'cnt_eq {rec.cnt_eq}, r {rec.r}', end='')
    scale = float(ref_grad.abs().max())
    if got_grad is not None:
        err_g = float((got_grad.double() - ref_grad).abs().max())
        print(f'; grad max|d| {err_g:.3g} = {err_g / scale if scale else 0.0:.3g} of max|ref| {scale:.3g}')
    assert err_l < 2e-6 * max(1.0, abs(ref_loss))
    if got_grad is None:
        return rec
    w = (d['pw'].double() if d['pw'] is not None else torch.ones_like(ref_grad)) * (d['fw'].double()[:, None] if d['fw'] is not None else 1.0)
    dead = ~(w != 0).any(dim=1) if rec.valid else torch.ones(w.shape[0], dtype=torch.bool)
    assert torch.equal(got_grad[dead], torch.zeros_like(got_grad[dead])), 'frames without weight / an invalid job get exactly 0'
    if rec.valid:
        assert scale > 0 and err_g <= (3e-5 if c.focal else 2e-5) * scale
    else:
        assert float(got_loss) == 0.0
    return rec


@pytest.mark.parametrize('c', K.MASK_CASES, ids=K.case_id)
def test_mask_objective_matches_the_oracle(cuda, c):
    """tcow_mask_loss, one channel: loss, total (+= loss_weight * loss in f32), every gradient pixel, exact zeros on dead frames, the guards."""
    d = K.mask_case_inputs(c)
    lw = 0.5 if c.weighted else 1.25
    loss, img, tot = _run_mask(cuda, [_job(c, d, lw)], d['n_seq'], d['T'], d['L'])
    _check_job(K.case_id(c), c, d, lw, loss[0], img[:, 0].reshape(-1, d['L']))
    assert float(tot) == float(np.float32(0.375) + np.float32(lw) * np.float32(float(loss[0])))


@pytest.mark.parametrize('geom', K.BATCH_GEOMS)
def test_mask_objective_batch_matches_the_oracle(cuda, geom):
    """tcow_mask_loss_batch: three jobs in one set of launches, each against the oracle (not only against single calls, which must agree bit for bit);
    total accumulates in job order."""
    cases = K.batch_cases(geom)
    ds = [K.mask_case_inputs(c) for c in cases]
    lws = [1.0, 0.3, 0.2]
    n_seq, T, L = K.GEOMS[geom]
    loss, img, tot = _run_mask(cuda, [_job(c, d, lw) for c, d, lw in zip(cases, ds, lws)], n_seq, T, L)
    want_tot = np.float32(0.375)
    for i, (c, d, lw) in enumerate(zip(cases, ds, lws)):
        _check_job(f'{geom} job {i}', c, d, lw, loss[i], img[:, i].reshape(-1, L))
        want_tot = np.float32(want_tot + np.float32(lw) * np.float32(float(loss[i])))
        one_loss, one_img, _ = _run_mask(cuda, [_job(c, d, lw)], n_seq, T, L)
        assert torch.equal(bits(one_loss[0]), bits(loss[i])) and torch.equal(bits(one_img[:, 0]), bits(img[:, i])), f'job {i}: batch and single call differ'
    assert float(tot) == float(want_tot)


@pytest.mark.parametrize('geom', ['2x2x9228', '52x5x8'])
def test_mask_objective_is_deterministic_and_takes_absent_outputs(cuda, geom):
    """The same call twice: bit-identical loss and gradient (fixed-order sums).  dlogits = NULL and total = NULL: the same loss bits, nothing else written."""
    c = K.MaskCase(geom, 'levels75', 'both', 1, 0, 0.8, 0.15, True)
    d = K.mask_case_inputs(c)
    n_seq, T, L = K.GEOMS[geom]
    first = _run_mask(cuda, [_job(c, d, 0.5)], n_seq, T, L)
    again = _run_mask(cuda, [_job(c, d, 0.5)], n_seq, T, L)
    assert torch.equal(bits(first[0]), bits(again[0])) and torch.equal(bits(first[1]), bits(again[1])) and torch.equal(bits(first[2]), bits(again[2]))
    no_dl = _run_mask(cuda, [_job(c, d, 0.5)], n_seq, T, L, with_dl=False)
    no_tot = _run_mask(cuda, [_job(c, d, 0.5)], n_seq, T, L, with_total=False)
    assert torch.equal(bits(no_dl[0]), bits(first[0])) and torch.equal(bits(no_dl[2]), bits(first[2]))
    assert torch.equal(bits(no_tot[0]), bits(first[0])) and torch.equal(bits(no_tot[1]), bits(first[1]))
    _check_job(f'{geom} no dlogits', c, d, 0.5, no_dl[0][0], None)


# ------------------------------------------------------------------------------------------------ tcow_snitch_weights
SNITCH_PATHS = {(8, 8): (0, False), (3, 64): (0, False), (48, 80): (2, False), (64, 128): (3, True), (37, 256): (4, True), (240, 320): (11, True),
                (704, 832): (31, True), (768, 768): (32, False)}
_snitch_cache = {}


def _snitch_case(H, W, frames):
    """Inputs and the dilation band of a shape, made once and shared by the exact and the rounded test."""
    if (H, W) not in _snitch_cache:
        k, r, bit = K.snitch_window(H, W)
        assert (r, bit) == SNITCH_PATHS[(H, W)] and k == 2 * r + 1
        assert bit == (W % 64 == 0 and 2 * r + 1 <= 63 and (H * W) % 256 == 0)      # one word per 64 pixels, the window's rows inside one wave, whole waves per frame
        t, ptr = K.snitch_inputs(H, W, frames, 4)
        band = K.snitch_band(t, r)
        cover = float(band[0].float().mean())
        assert (0.05 <= cover <= 0.5) if r > 0 else torch.equal(band, t == 0.25), cover
        _snitch_cache[(H, W)] = (t, ptr, band)
    return _snitch_cache[(H, W)]


def _run_snitch(dev, t, ptr, fw, pos_count, class_balancing, factor, seq_major):
    """t [F, H, W] as channel 0 of a (n_seq, 3, T, H, W) image whose other channels are NaN; F = n_seq x T split either way.  Returns f32 CPU [F, H, W]."""
    _lib, lib, st = _api()
    Fn, H, W = t.shape
    n_seq, T = (Fn, 1) if seq_major else (1, Fn)
    img = torch.full((n_seq, 3, T, H, W), NAN, device=dev)
    img[:, 0] = t.reshape(n_seq, T, H, W).to(dev)
    p = ptr.contiguous().to(dev); f = fw.contiguous().to(dev); pc = torch.tensor([pos_count, -1], dtype=torch.int32, device=dev)
    out_buf, out = guarded_flat(Fn * H * W, torch.float32, dev)
    ws = _scratch(lib.tcow_snitch_weights_workspace_bytes(Fn, H, W), dev)
    _lib.check(lib.tcow_snitch_weights(st, n_seq, T, H, W, img.data_ptr(), 3 * T * H * W, p.data_ptr(), f.data_ptr(), pc.data_ptr(), int(class_balancing), float(factor),
                                       out.data_ptr(), ws.data_ptr(), ws.numel()), 'tcow_snitch_weights', lib)
    torch.cuda.synchronize()
    assert_guarded_flat(out_buf, Fn * H * W, 'snitch weights')
    return out.cpu().reshape(Fn, H, W)


@pytest.mark.parametrize('H,W,frames', K.SNITCH_SHAPES)
def test_snitch_weights_exact(cuda, H, W, frames):
    """No class balancing, factor 4, frame weights from {0.5, 1, 2}: every product is a power-of-two scaling, the result is the reference bit for bit."""
    t, ptr, band = _snitch_case(H, W, frames)
    fw = torch.tensor([0.5, 2.0, 1.0])[:frames]
    want, _ = K.snitch_weights_ref(t, ptr, fw, 0, False, 4.0, band=band)
    got = _run_snitch(cuda, t, ptr, fw, 0, False, 4.0, seq_major=(H % 2 == 1))
    wrong = got.double() != want
    assert not bool(wrong.any()), (int(wrong.sum()), wrong.nonzero()[:8].tolist())
    assert torch.equal(_run_snitch(cuda, t, ptr, fw, 0, False, 1.0, seq_major=(H % 2 == 0)).double(), K.snitch_weights_ref(t, ptr, fw, 0, False, 1.0, band=band)[0])


@pytest.mark.parametrize('H,W,frames', K.SNITCH_SHAPES)
def test_snitch_weights_rounded(cuda, H, W, frames):
    """Class balancing on, factor 3, random frame weights; positives the majority, the minority, under the 5 % floor, and the negatives under it."""
    t, ptr, band = _snitch_case(H, W, frames)
    fw = torch.rand(frames, generator=torch.Generator().manual_seed(H)) + 0.5
    n = frames * H * W
    for pos in (int(0.7 * n), int(0.2 * n), int(0.01 * n), int(0.99 * n)):
        want, _ = K.snitch_weights_ref(t, ptr, fw, pos, True, 3.0, band=band)
        got = _run_snitch(cuda, t, ptr, fw, pos, True, 3.0, seq_major=(H % 2 == 1)).double()
        rel = float(((got - want).abs() / want).max())
        print(f'{H}x{W} pos {pos}/{n}: max rel |d| {rel:.3g}')
        assert rel <= 1e-6


# ------------------------------------------------------------------------------------------------ tcow_build_masks / tcow_build_query_masks
def _run_query_masks(dev, B, Q, K_, M, T, HW, qt, seed):
    """tcow_build_query_masks through the C ABI on loss_kit's inputs, every output guarded.  Returns the inputs and the outputs on the CPU."""
    from tcow_amd.tcow_loss import default_args
    _lib, lib, st = _api()
    a = default_args()
    occl, dag, sel = K.decision_inputs(B, K_, T, Q, seed)
    segm, div = K.mask_inputs(B, M, T, HW, seed)
    n = B * Q * T
    f32 = np.float32
    z = f32(a.occl_cont_zero_weight); has_w = f32(f32(1.0 - a.occl_cont_zero_weight) + z)
    words = dict(idx=B * Q + 2 * n, ids=n * 2 // 4, flags=n * 3, sel_occl=n * 3, frame_w=3 * n, qmask=n * HW, target=3 * n * HW, ptr=n * HW // 4, counts=1 + 2 * Q)
    assert (n * 2) % 4 == 0
    buf = {k: _guarded_words(v, dev) for k, v in words.items()}
    ins = [segm.to(dev), div.to(dev), occl.to(dev), dag.to(dev), sel.to(dev)]
    _lib.check(lib.tcow_build_query_masks(st, B, Q, K_, M, T, HW, qt, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), ins[4].data_ptr(),
                                          float(f32(a.front_occl_thres)), float(f32(a.front_occl_thres / 2.0)), float(f32(a.outer_cont_thres)),
                                          float(f32(float(a.occluded_weight))), float(z), float(has_w), buf['idx'].data_ptr(), buf['ids'].data_ptr(),
                                          buf['flags'].data_ptr(), buf['sel_occl'].data_ptr(), buf['frame_w'].data_ptr(), buf['qmask'].data_ptr(),
                                          buf['target'].data_ptr(), buf['ptr'].data_ptr(), buf['counts'].data_ptr()), 'tcow_build_query_masks', lib)
    torch.cuda.synchronize()
    for k, v in words.items():
        _tail_intact(buf[k], v, k)
    idx = buf['idx'].view(torch.int32)[:words['idx']].cpu()
    out = dict(query_idx=idx[:B * Q].view(B, Q), front=idx[B * Q:B * Q + n].view(B, Q, T), cont=idx[B * Q + n:].view(B, Q, T),
               ids=buf['ids'].view(torch.uint8)[:n * 2].cpu().view(B, Q, T, 2), flags=buf['flags'][:n * 3].cpu().view(B, Q, T, 3),
               sel_occl=buf['sel_occl'][:n * 3].cpu().view(B, Q, T, 3), frame_w=buf['frame_w'][:3 * n].cpu().view(3, B, Q, T),
               qmask=buf['qmask'][:n * HW].cpu().view(B, Q, 1, T, 1, HW), target=buf['target'][:3 * n * HW].cpu().view(B, Q, 3, T, 1, HW),
               ptr=buf['ptr'].view(torch.uint8)[:n * HW].cpu().view(B, Q, 1, T, 1, HW), counts=buf['counts'].view(torch.int32)[:1 + 2 * Q].cpu())
    return dict(occl=occl, dag=dag, sel=sel, segm=segm, div=div, args=a), out


def _check_tables(ins, out, qt):
    """The table pass against frame_decisions and TcowLosses.frame_weights: indices, ids, flags bit-exact, weights equal to the tensor expressions' f32 results."""
    from tcow_amd.pipeline import frame_decisions
    from tcow_amd.tcow_loss import TcowLosses
    a = ins['args']
    fi, ci, ids, flags = frame_decisions(ins['occl'], ins['dag'], ins['sel'], a)
    assert torch.equal(out['query_idx'].long(), ins['sel']) and torch.equal(out['front'].long(), fi) and torch.equal(out['cont'].long(), ci)
    assert torch.equal(out['ids'], ids) and torch.equal(out['flags'], flags)
    assert int((fi >= 0).sum()) > 0 and int((fi < 0).sum()) > 0 and int((ci >= 0).sum()) > 0 and int((ci < 0).sum()) > 0
    B, Q = ins['sel'].shape
    sel_of = ins['occl'][torch.arange(B)[:, None].expand(B, Q), ins['sel']]
    assert torch.equal(out['sel_occl'], sel_of)
    want_fw = TcowLosses(a).frame_weights(sel_of, qt)
    assert torch.equal(out['frame_w'][0], want_fw)
    plain = (sel_of[..., 0] * float(a.occluded_weight)).clip(min=1.0)
    assert torch.equal(want_fw[:-1], plain[:-1]) and torch.equal(want_fw[-1, :, qt], plain[-1, :, qt] * 0.2)      # (the x 0.2 at (B - 1, :, query_time) is in there)
    for ch in (1, 2):
        has = out['target'][:, :, ch].flatten(-2).any(dim=-1).to(torch.float32)
        assert torch.equal(out['frame_w'][ch], has * (1.0 - a.occl_cont_zero_weight) + a.occl_cont_zero_weight), ch
        assert 0 < int(has.sum()) < has.numel()
    return fi, ci


@pytest.mark.parametrize('HW', [16, 16 * 255, 16 * 257, 16 * (2048 + 256 + 5)])
def test_mask_builders_match_the_reference(cuda, HW):
    """One workgroup, one nearly full, two, and eight with a ragged second grid-stride trip: query mask, the three target channels, the occluder tags, the
    amodal count and both flags per query bit-exact; tcow_build_masks on the same decisions writes the same bits."""
    B, Q, M, T, qt = 2, 2, 4, 3, 1
    ins, out = _run_query_masks(cuda, B, Q, M, M, T, HW, qt, seed=HW)
    fi, ci = _check_tables(ins, out, qt)
    qm, tg, pt, counts = K.build_masks_ref(ins['segm'], ins['div'], ins['sel'], fi, ci, qt)
    assert int((tg[:, :, 1:].flatten(-2).any(-1) == 0).sum()) > 0 and int(counts[0]) > 0
    assert torch.equal(out['qmask'], qm) and torch.equal(out['target'], tg) and torch.equal(out['ptr'], pt)
    assert int(out['counts'][0]) == int(counts[0]) and torch.equal((out['counts'][1:] != 0).long(), counts[1:])
    # the other entry point, handed the decisions
    _lib, lib, st = _api()
    n = B * Q * T
    words = dict(qmask=n * HW, target=3 * n * HW, ptr=n * HW // 4, counts=1 + 2 * Q)
    buf = {k: _guarded_words(v, cuda) for k, v in words.items()}
    ins_d = [ins['segm'].to(cuda), ins['div'].to(cuda), ins['sel'].to(torch.int32).to(cuda), fi.to(torch.int32).to(cuda), ci.to(torch.int32).to(cuda)]
    _lib.check(lib.tcow_build_masks(st, B, Q, M, T, HW, qt, ins_d[0].data_ptr(), ins_d[1].data_ptr(), ins_d[2].data_ptr(), ins_d[3].data_ptr(), ins_d[4].data_ptr(),
                                    buf['qmask'].data_ptr(), buf['target'].data_ptr(), buf['ptr'].data_ptr(), buf['counts'].data_ptr()), 'tcow_build_masks', lib)
    torch.cuda.synchronize()
    for k, v in words.items():
        _tail_intact(buf[k], v, k)
    assert torch.equal(buf['qmask'][:n * HW].cpu(), out['qmask'].reshape(-1)) and torch.equal(buf['target'][:3 * n * HW].cpu(), out['target'].reshape(-1))
    assert torch.equal(buf['ptr'].view(torch.uint8)[:n * HW].cpu(), out['ptr'].reshape(-1))
    assert torch.equal(buf['counts'].view(torch.int32)[:1 + 2 * Q].cpu(), out['counts'])


def test_query_tables_second_workgroup(cuda):
    """276 (b, q, t) rows: the table kernel's second workgroup.  Decisions, ids, flags, the queried occlusion fractions and the three frame-weight channels."""
    B, Q, T, KM, qt = 3, 4, 23, 6, 5
    ins, out = _run_query_masks(cuda, B, Q, KM, KM, T, 16, qt, seed=3)
    fi, ci = _check_tables(ins, out, qt)
    qm, tg, pt, counts = K.build_masks_ref(ins['segm'], ins['div'], ins['sel'], fi, ci, qt)
    assert torch.equal(out['qmask'], qm) and torch.equal(out['target'], tg) and torch.equal(out['ptr'], pt) and int(out['counts'][0]) == int(counts[0])


# ------------------------------------------------------------------------------------------------ tcow_iou_counts / tcow_iou_means
@pytest.mark.parametrize('frame_len', [4, 4 * 255, 4 * 256, 4 * 259, 4 * 769])
def test_iou_counts_are_exact(cuda, frame_len):
    _lib, lib, st = _api()
    x, t = K.iou_inputs(7, frame_len, frame_len)
    want = K.iou_counts_ref(x, t)
    assert frame_len == 4 or (int((x == 0).sum()) > 0 and int((t == 0.5).sum()) > 0)
    xd, td = x.to(cuda), t.to(cuda)
    buf = _guarded_words(21, cuda)
    _lib.check(lib.tcow_iou_counts(st, xd.data_ptr(), td.data_ptr(), 7, frame_len, buf.data_ptr()), 'tcow_iou_counts', lib)
    torch.cuda.synchronize()
    _tail_intact(buf, 21, 'iou counts')
    assert torch.equal(buf.view(torch.int32)[:21].cpu().view(7, 3).long(), want)


@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('n_seq,T', [(1, 1), (16, 16), (257, 1), (24, 25)])
def test_iou_means_match_the_float64_reference(cuda, n_seq, T, C):
    _lib, lib, st = _api()
    tab = K.iou_tables(n_seq, C, T, seed=n_seq + C)
    want_mean, want_n = K.iou_means_ref(tab)
    if C == 3 and (n_seq + C) % 2 == 1:
        assert int(want_n[2]) == 0 and int(want_n[5]) == 0 and int(want_n[0]) > 0          # a selector with no frame at all
    td = tab.contiguous().to(cuda)
    mean_buf, mean = guarded_flat(6, torch.float32, cuda)
    cnt_buf = _guarded_words(6, cuda)
    _lib.check(lib.tcow_iou_means(st, td.data_ptr(), n_seq, C, T, mean.data_ptr(), cnt_buf.data_ptr()), 'tcow_iou_means', lib)
    torch.cuda.synchronize()
    assert_guarded_flat(mean_buf, 6, 'iou means'); _tail_intact(cnt_buf, 6, 'iou frame counts')
    assert torch.equal(cnt_buf.view(torch.int32)[:6].cpu().long(), want_n)
    got = mean.cpu().double()
    for i in range(6):
        if int(want_n[i]) == 0:
            assert float(got[i]) == -1.0
        else:
            assert abs(float(got[i]) - float(want_mean[i])) <= 2.0 ** -23 * abs(float(want_mean[i])), (i, float(got[i]), float(want_mean[i]))

"""Writes tests/golden/glue_refusals.json: what the glue and loss-head entry points of the library answer to arguments their checks refuse, and the
values of their four size functions, in both builds.  Everything runs on the CPU: the stream is null, the pointers are null or a dummy address, and
no case may get past the argument checks.  The fixture is recorded from the commit BEFORE a change of these sources and must not be regenerated to
make a changed status or message pass.

    python tools/make_glue_refusals.py [output path]
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_glue_refusals_host as kit  # noqa: E402

# the sources whose entry points are recorded: the two bags of the parent, or the eight family files that replace them
SOURCES = ('elementwise', 'tokens', 'clip_input', 'mask_head', 'casts', 'mask_loss', 'metrics', 'query_masks', 'snitch_weights')
P, Z = 4096, None                                    # a dummy (16-byte aligned) address, a null pointer
F32X3 = 2                                            # TCOW_F32X3: a dtype none of these entry points stores


def _job(**over):
    j = dict(n_frames=2, frame_len=16, frames_per_seq=2, logits=P, logits_seq_stride=32, target=P, target_seq_stride=32, pixel_w=Z, frame_w=Z,
             weighted_aot=0, aot_loss=0.8, topk_frac=0.5, loss_weight=1.0, loss=P, total=Z, dlogits=Z, dlogits_seq_stride=32, ws=P, ws_bytes=1 << 20, focal=0)
    j.update(over)
    return j


def _ml(*jobs):
    return {'mask_loss_args': list(jobs)}


_QM = [P, P, P, P, P, 0.5, 0.25, 0.5, 2.0, 0.1, 1.0, P, P, P, P, P, P, P, P, P]      # tcow_build_query_masks from segm on

CASES = [
    # ---- tokens
    ('tcow_im2col', [Z, 1, 0, 1, 16, 16, 4, P, P, 0, P]),
    ('tcow_im2col', [Z, 1, 1, 1, 16, 18, 4, P, P, 0, P]),
    ('tcow_im2col', [Z, 1, 1, 1, 16, 16, 4, Z, P, 0, P]),
    ('tcow_im2col', [Z, F32X3, 1, 1, 16, 16, 4, P, P, 0, P]),
    ('tcow_im2col_channels', [Z, 0, 1, 1, 16, 16, 4, 0, P, 0, P]),
    ('tcow_im2col_channels', [Z, 0, 1, 1, 16, 16, 4, 3, P, 0, Z]),
    ('tcow_im2col_channels', [Z, F32X3, 1, 1, 16, 16, 4, 3, P, 0, P]),
    ('tcow_embed_fwd', [Z, 1, 2, 1, 64, P, P, P, P]),
    ('tcow_embed_bwd', [Z, 1, 2, 5, 6, P, P, P, 0]),
    ('tcow_cls_merge', [Z, 1, 2, 5, 64, P, 2, 0]),
    ('tcow_cls_merge_bwd_cast', [Z, 1, 1, 2, 5, 64, P, 1, P, 6, Z]),
    ('tcow_cls_merge_bwd_cast', [Z, 0, 1, 2, 5, 64, P, 1, Z, 64, Z]),
    ('tcow_cls_merge_bwd_cast', [Z, F32X3, 1, 2, 5, 64, P, 1, P, 64, Z]),
    # ---- clip_input
    ('tcow_gather_frames', [Z, 1, 0, 2, 8, 8, 2, 4, 4, P, P, P, P, P]),
    ('tcow_gather_frames', [Z, 2, 3, 2, 8, 8, 2, 4, 4, P, P, P, P, P]),
    ('tcow_resize_aa', [Z, 3, 2, 8, 8, 2, 8, 8, 4, 4, P, P, P, P, P, P, P, 0, P, P, P, 3, P]),
    ('tcow_resize_aa', [Z, 3, 2, 8, 8, 2, 8, 8, 4, 4, Z, P, P, P, P, P, P, 3, P, P, P, 3, P]),
    # ---- mask_head
    ('tcow_unpatchify_pool_fwd', [Z, 1, 2, 2, 2, 16, 3, 3, P, P]),
    ('tcow_unpatchify_pool_fwd', [Z, F32X3, 2, 2, 2, 16, 3, 4, P, P]),
    ('tcow_unpatchify_pool_fwd', [Z, F32X3, 2, 2, 2, 6, 3, 2, P, P]),
    ('tcow_unpatchify_pool_bwd', [Z, 1, 2, 2, 2, 16, 3, 4, P, Z]),
    ('tcow_unpatchify_pool_bwd', [Z, F32X3, 2, 2, 2, 16, 3, 4, P, P]),
    ('tcow_unpatchify_pool_bwd', [Z, F32X3, 2, 2, 2, 6, 3, 2, P, P]),
    ('tcow_upsample_fwd', [Z, 1, 2, 3, 4, 4, 0, 1, P, P]),
    ('tcow_upsample_fwd', [Z, 65536, 1, 1, 4, 4, 4, 1, P, P]),
    ('tcow_upsample_bwd', [Z, 1, 2, 3, 0, 4, 4, 1, P, P]),
    ('tcow_upsample_bwd_amax', [Z, 1, 2, 3, 4, 8, 4, P, P, P, 64]),
    ('tcow_upsample_bwd_amax', [Z, 1, 2, 3, 8, 8, 4, P, P, P, 1]),
    ('tcow_flags_fwd', [Z, 2, 1, 64, 3, P, P, P, P]),
    ('tcow_flags_fwd', [Z, 2, 5, 6, 3, P, P, P, P]),
    # ---- casts
    ('tcow_droppath_rows', [Z, 0, 1, 2, 5, P, P, P, P]),
    ('tcow_scale_unless_one', [Z, P + 4, 8, P]),
    ('tcow_scale_cast', [Z, 1, 4, 6, P, 8, Z, P, 8]),
    ('tcow_scale_cast', [Z, F32X3, 4, 8, P, 8, Z, P, 8]),
    ('tcow_cast_transpose', [Z, 1, 8, 8, P, Z, Z]),
    ('tcow_cast_transpose', [Z, F32X3, 8, 8, P, P, P]),
    ('tcow_cast_transpose_batched', [Z, 1, P, 0, 4]),
    ('tcow_cast_transpose_batched', [Z, F32X3, P, 2, 4]),
    # ---- mask_loss
    ('tcow_mask_loss', [Z, _ml()]),
    ('tcow_mask_loss', [Z, _ml(_job(logits=Z))]),
    ('tcow_mask_loss', [Z, _ml(_job(frames_per_seq=3))]),
    ('tcow_mask_loss', [Z, _ml(_job(frame_len=6))]),
    ('tcow_mask_loss', [Z, _ml(_job(logits_seq_stride=6))]),
    ('tcow_mask_loss', [Z, _ml(_job(n_frames=65536, frames_per_seq=1))]),
    ('tcow_mask_loss', [Z, _ml(_job(topk_frac=0.0))]),
    ('tcow_mask_loss', [Z, _ml(_job(topk_frac=1.5))]),
    ('tcow_mask_loss', [Z, _ml(_job(ws_bytes=1024))]),
    ('tcow_mask_loss', [Z, _ml(_job(ws_bytes=19712))]),         # enough without the bit-pattern image, not with it
    ('tcow_mask_loss_batch', [Z, _ml(_job()), 0]),
    ('tcow_mask_loss_batch', [Z, _ml(_job()), 5]),
    ('tcow_mask_loss_batch', [Z, _ml(_job(), _job(ws=2 * P, dlogits_seq_stride=2)), 2]),
    ('tcow_mask_loss_batch', [Z, _ml(_job(), _job(ws=2 * P, frame_len=32)), 2]),
    ('tcow_mask_loss_batch', [Z, _ml(_job(), _job(ws=2 * P, total=P)), 2]),
    ('tcow_mask_loss_batch', [Z, _ml(_job(), _job(ws=2 * P), _job()), 3]),
    # ---- metrics
    ('tcow_iou_counts', [Z, P, Z, 2, 16, P]),
    ('tcow_iou_counts', [Z, P, P, 2, 6, P]),
    ('tcow_iou_means', [Z, P, 2, 0, 4, P, P]),
    # ---- query_masks
    ('tcow_build_masks', [Z, 1, 1, 2, 2, 8, 0, P, P, P, P, P, P, P, P, P]),
    ('tcow_build_masks', [Z, 1, 1, 2, 2, 16, 0, P, P, P, P, P, P, P, P, Z]),
    ('tcow_build_masks', [Z, 65536, 1, 2, 1, 16, 0, P, P, P, P, P, P, P, P, P]),
    ('tcow_build_query_masks', [Z, 1, 1, 0, 2, 4, 16, 0] + _QM),
    ('tcow_build_query_masks', [Z, 1, 1, 2, 2, 4, 16, 0] + _QM[:-1] + [Z]),
    ('tcow_build_query_masks', [Z, 1, 1, 2, 2, 2, 16, 0] + _QM),                # 1 + 2 Q > B Q T
    ('tcow_build_query_masks', [Z, 1, 1, 2, 256, 4, 16, 0] + _QM),
    ('tcow_build_query_masks', [Z, 1, 1, 2, 2, 4, 16, 4] + _QM),
    # ---- snitch_weights
    ('tcow_snitch_weights', [Z, 2, 2, 0, 64, P, 3 * 2 * 64 * 64, P, P, P, 1, 3.0, P, P, 1 << 20]),
    ('tcow_snitch_weights', [Z, 2, 2, 64, 64, P, 3 * 2 * 64 * 64, P, P, Z, 1, 3.0, P, P, 1 << 20]),
    ('tcow_snitch_weights', [Z, 65536, 1, 64, 64, P, 3 * 64 * 64, P, P, P, 1, 3.0, P, P, 1 << 20]),
    ('tcow_snitch_weights', [Z, 2, 2, 64, 64, P, 3 * 2 * 64 * 64, P, P, P, 1, 3.0, P, Z, 0]),
    ('tcow_snitch_weights', [Z, 2, 2, 64, 64, P, 3 * 2 * 64 * 64, P, P, P, 0, 3.0, P, P, 4 * 64 * 64]),
]

_SHAPES = [(0, 16), (1, 4), (2, 16), (3, 4096), (6, 4100), (64, 240 * 320)]
SIZES = ([('tcow_mask_loss_workspace_bytes', list(s)) for s in _SHAPES] +
         [('tcow_mask_loss_workspace_bytes_for', list(s) + list(ta)) for s in _SHAPES for ta in ((0.5, 0.8), (1.0, 0.8), (0.5, 0.0))] +
         [('tcow_snitch_weights_workspace_bytes', list(s)) for s in ((1, 7, 9), (6, 64, 64), (90, 240, 320))] +
         [('tcow_cast_desc_bytes', [])])

DISPATCHED = ('tcow_im2col', 'tcow_im2col_channels', 'tcow_cls_merge_bwd_cast', 'tcow_unpatchify_pool_fwd', 'tcow_unpatchify_pool_bwd', 'tcow_scale_cast',
              'tcow_cast_transpose', 'tcow_cast_transpose_batched')


def _source_facts():
    """(entry points the sources define, one regular expression per TCOW_CHECK_ARG line matching the message it sets)."""
    entries, checks = set(), []
    for name in SOURCES:
        path = os.path.join(ROOT, 'tcow_amd', 'csrc', name + '.hip')
        if not os.path.exists(path):
            continue
        text = open(path).read()
        entries |= set(re.findall(r'^(?:extern "C" )?(?:int|long|size_t) (tcow_\w+)\(', text, re.M))
        for fmt in re.findall(r'TCOW_CHECK_ARG\([^"]*"((?:[^"\\]|\\.)*)"', text):
            checks.append((fmt, re.compile(re.sub(r'%l?[dg]', r'\\S+', re.escape(fmt)) + '$')))
    return entries, checks


def main():
    from tcow_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else kit.FIXTURE
    entries, checks = _source_facts()
    size_fns = {e for e, _ in SIZES}
    assert {e for e, _ in CASES} | size_fns == entries, sorted(entries ^ ({e for e, _ in CASES} | size_fns))
    doc = {'abi': _lib.ABI_VERSION, 'refusals': {}, 'sizes': {}}
    for fmt in kit.BUILDS:
        lib = _lib.lib(fmt)
        rows = []
        for entry, args in CASES:
            status, message = kit.call(lib, entry, args)
            assert status == -1, (entry, args, status, message)                       # TCOW_ERR_INVALID_ARG: refused, nothing launched
            rows.append({'entry': entry, 'args': args, 'status': status, 'message': message})
        for text, rx in checks:
            assert any(rx.match(r['message']) for r in rows), f'no case fires the check "{text}"'
        for entry in DISPATCHED:
            assert any(r['entry'] == entry and r['args'][1] == F32X3 and r['message'] == f'{entry}: unknown dtype 2' for r in rows), entry
        doc['refusals'][fmt] = rows
        doc['sizes'][fmt] = [{'entry': e, 'args': a, 'value': getattr(lib, e)(*a)} for e, a in SIZES]
        print(f'{fmt}: {len(rows)} refusals over {len({r["entry"] for r in rows})} entry points, {len(checks)} check lines, {len(SIZES)} sizes')
    with open(out, 'w') as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write('\n')
    print(f'{out}: {os.path.getsize(out)} bytes, libraries from {os.path.dirname(_lib.LIB_PATH)}')


if __name__ == '__main__':
    main()

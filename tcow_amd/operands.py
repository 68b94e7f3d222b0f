"""Everything the Seeker hot path derives from the f32 master parameters and keeps across steps, with ONE owner: QueryMaskTracker._operands.

An OperandCache holds the 16-bit W / W^T copies of every GEMM weight, the folded temporal projection W' = Wfc Wproj (see engine.py), the one-launch
re-cast table, the small per-geometry constants (mask0, joint rows, DropPath keep probabilities) and the persistent gradient buckets.  It takes
the module's mode as an argument and keeps no reference to the module.  The rules that keep this state correct:

  current        a copy is served iff its stamp (parameter._version(s), epoch), its mode and "has W^T if training asked for it" all match; anything else re-casts it.
  epoch          invalidate() bumps it (the parameters were written through raw pointers or .data, which no version counter sees) and re-casts what is registered.
  generation     moves on every training registration of a plain weight and on every drop(): FusedAdamWClip's tile table and SeekerStream's graphs point into the buffers.
  consumed once  optimizer_wrote(keys): the fused optimizer wrote these copies itself; the next refresh() skips exactly those (stamps them all the same) and forgets the set.
  keep-alive     a captured graph holds raw pointers into tensors only this cache owns: keep_alive() returns references that outlive any replacement of entries, or a drop.
"""
import struct

import torch

from . import _lib, ops


def fold_on(module):
    return ops.is16(module.mode) and module.attention_type == 'divided_space_time'


def _fold_products(ents):
    """W' = Wfc Wproj and b' = Wfc b_proj for a list of fold entries: two batched launches (per 24 entries)."""
    for c0 in range(0, len(ents), 24):
        ops.sgemm_batched([(e['fc'].detach(), e['proj'].detach(), e['W32']) for e in ents[c0:c0 + 24]])
        ops.sgemm_batched([(e['fc'].detach(), e['bproj'].detach().view(1, -1).t(), e['b32'].view(-1, 1)) for e in ents[c0:c0 + 24]])


class OperandCache:
    def __init__(self, generation=0, epoch=0):
        self.generation, self.epoch = generation, epoch      # see the module docstring; FusedAdamWClip and SeekerStream read them
        self.copies = {}                  # id(parameter) -> (stamp, mode, Wc, Wt); ('fold', block) -> fold entry; constant key -> tensor
        self.registry = {}                # key -> (f32 source, Wc or None, Wt, N, K): what refresh() re-casts
        self.folds = {}                   # ('fold', block) -> fold entry: what refresh() recomputes first
        self.table = None                 # (pointer signature, device records, record count, tile total) of the batched re-cast
        self.buckets = {}                 # persistent gradient buckets and the folded projection's dW' / db' pairs
        self._optimizer_wrote = ()

    def fresh(self):
        """An empty cache one generation on, for a DataParallel replica: its __dict__ is a shallow copy of the original's, so it must never mutate the shared instance."""
        return OperandCache(self.generation + 1, self.epoch)

    def drop(self, buckets=True):
        """Forget everything derived from the parameters' storage: 16-bit W / W^T copies, their registries and pointer table, the folded products, the constants
        and (buckets=True) the persistent gradient buffers; the generation moves.  They are keyed by id(parameter), which survives a `.data` swap.  set_precision()
        passes buckets=False: the gradient buffers do not depend on the mode (f32, keyed by what they hold) and survive; .to() / .cuda() leave none behind."""
        self.copies, self.registry, self.folds, self.table, self._optimizer_wrote = {}, {}, {}, None, ()
        self.generation += 1
        if buckets:
            self.buckets = {}

    def keep_alive(self):
        """References to every tensor a graph captured now may point into (operand copies, folded W' / b', mask0), alive as long as the caller holds them."""
        return dict(self.copies)

    def constant(self, key, build):
        """Small per-geometry constant (mask0, joint rows, DropPath keep probabilities): built once per key."""
        if key not in self.copies:
            self.copies[key] = build()
        return self.copies[key]

    def longest(self, key, n, build):
        """A constant whose shorter forms are prefixes of its longer ones (mask0 of one row of frames): ONE entry per key, rebuilt only when a longer
        one is asked for; returns the first n elements."""
        t = self.copies.get(key)
        if t is None or t.numel() < n:
            t = self.copies[key] = build(n)
        return t[:n]

    def buffer(self, key, alloc):
        """Persistent gradient storage: allocated once per key, the same pointers every step."""
        if key not in self.buckets:
            self.buckets[key] = alloc()
        return self.buckets[key]

    def weight(self, mode, p, train):
        """Operand copies of a weight: (Wc [N,K] in the mode's dtype, Wt [K,N] or None), cached per parameter version."""
        key = id(p)
        ent = self.copies.get(key)
        ver = (p._version, self.epoch)
        if ent is not None and ent[0] == ver and ent[1] == mode and (ent[3] is not None or not train):
            return ent[2], ent[3]
        w = p.detach().reshape(p.shape[0], -1)
        N, K = w.shape
        dt = ops.tdtype(mode)
        if ops.is16(mode):
            Wc = torch.empty(N, K, dtype=dt, device=w.device)
            Wt = torch.empty(K, N, dtype=dt, device=w.device) if train else None
            ops.cast_transpose(mode, w.contiguous(), Wc, Wt)
        else:
            Wc = w.contiguous()
            Wt = torch.empty(K, N, dtype=dt, device=w.device) if train else None
            if train:
                ops.cast_transpose(mode, Wc, None, Wt)
        self.copies[key] = (ver, mode, Wc, Wt)
        if train:
            # remember the buffers: after an optimizer step refresh() re-casts ALL registered weights in one launch
            self.registry[key] = (p, Wc if ops.is16(mode) else None, Wt, N, K)
            self.generation += 1      # (FusedAdamWClip's tile table points into these buffers: it rebuilds when this moves)
        return Wc, Wt

    def folded(self, mode, i, q, ix, train):
        """Operands of block i's folded temporal projection: (Wc' [D,D], Wt' [D,D] or None, b' [D] f32), cached per parameter version."""
        pfc, pproj, bproj = q[ix['tfc']], q[ix['tproj']], q[ix['tproj'] + 1]
        key = ('fold', i)
        ver = (pfc._version, pproj._version, bproj._version, self.epoch)
        ent = self.copies.get(key)
        if ent is not None and ent['ver'] == ver and ent['mode'] == mode and (ent['Wt'] is not None or not train):
            return ent['Wc'], ent['Wt'], ent['b32']
        D = pfc.shape[0]
        dev = pfc.device
        dt = ops.tdtype(mode)
        if ent is None or ent['mode'] != mode:
            ent = dict(fc=pfc, proj=pproj, bproj=bproj, W32=torch.empty(D, D, dtype=torch.float32, device=dev), b32=torch.empty(D, dtype=torch.float32, device=dev),
                       Wc=torch.empty(D, D, dtype=dt, device=dev), Wt=None, mode=mode)
        if train and ent['Wt'] is None:
            ent['Wt'] = torch.empty(D, D, dtype=dt, device=dev)
        _fold_products([ent])
        ops.cast_transpose(mode, ent['W32'], ent['Wc'], ent['Wt'])
        ent['ver'] = ver
        self.copies[key] = ent
        if train:
            # registered like any GEMM weight: refresh() recomputes W' (all blocks, one launch) and re-casts it with the others
            self.registry[key] = (ent['W32'], ent['Wc'], ent['Wt'], D, D)
            self.folds[key] = ent
        return ent['Wc'], ent['Wt'], ent['b32']

    def castable(self):
        """{id(parameter): (Wc, Wt, N, K)} of the registered GEMM weights whose 16-bit operand copies the fused optimizer may write itself
        (64 x 64 tiles of a whole Parameter; the fold entries are cast here)."""
        return {k: (Wc, Wt, N, K) for k, (p, Wc, Wt, N, K) in self.registry.items()
                if isinstance(k, int) and isinstance(p, torch.nn.Parameter) and Wc is not None and Wt is not None and N % 64 == 0 and K % 64 == 0 and p.numel() == N * K}

    def optimizer_wrote(self, keys):
        """The fused optimizer has just written the copies of these castable() keys: the next refresh() skips them, once."""
        self._optimizer_wrote = keys

    def invalidate(self, mode):
        """The parameters were updated through raw pointers: bump the epoch, then refresh if anything is registered."""
        self.epoch += 1
        self.refresh(mode)       # all operand copies of the next step in one launch

    def refresh(self, mode):
        """Re-cast every registered GEMM weight (bf16 copy + transposed copy) with ONE kernel launch instead of one per weight;
        called right after the optimizer has written the f32 master weights."""
        reg = self.registry
        live = [ent for k, ent in self.folds.items() if k in reg]         # (a fold whose operand copies are no longer registered is stale: skip it)
        if live:
            _fold_products(live)
        # weights whose copies the optimizer has just written itself (FusedAdamWClip's tile kernel, 16-bit modes): only their version stamps are refreshed below
        done, self._optimizer_wrote = self._optimizer_wrote, ()
        ents = [(k, v) for k, v in reg.items() if k not in done]
        if ents:
            sig = tuple((k, p.data_ptr(), 0 if Wc is None else Wc.data_ptr(), 0 if Wt is None else Wt.data_ptr()) for k, (p, Wc, Wt, N, K) in ents) + (mode,)
            tab = self.table
            if tab is None or tab[0] != sig:
                rec, tiles = [], 0
                edge = 64 if all(N % 64 == 0 and K % 64 == 0 for _, (_, _, _, N, K) in ents) else 32     # tile edge of tcow_cast_transpose_batched (all records alike)
                for k, (p, Wc, Wt, N, K) in ents:
                    rec.append(struct.pack('<QQQiiii', p.data_ptr(), 0 if Wc is None else Wc.data_ptr(), 0 if Wt is None else Wt.data_ptr(), N, K, tiles, edge))
                    tiles += ((N + edge - 1) // edge) * ((K + edge - 1) // edge)
                assert len(rec[0]) == int(_lib.lib().tcow_cast_desc_bytes())
                buf = torch.frombuffer(bytearray(b''.join(rec)), dtype=torch.uint8).to(ents[0][1][0].device)
                tab = self.table = (sig, buf, len(rec), tiles)
            ops.cast_transpose_batched(mode, tab[1], tab[2], tab[3])
        # every registered copy is now current for its parameters' present versions (and this weight epoch): the next lookup is a hit
        for k, (p, Wc, Wt, N, K) in reg.items():
            e = self.folds.get(k)
            if e is not None:
                e['ver'] = (e['fc']._version, e['proj']._version, e['bproj']._version, self.epoch)
            else:
                self.copies[k] = ((p._version, self.epoch), mode, Wc if Wc is not None else p.detach().reshape(p.shape[0], -1).contiguous(), Wt)

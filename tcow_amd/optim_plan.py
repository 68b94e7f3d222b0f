"""Host arithmetic of FusedAdamWClip (optim.py): the tables tcow_adamw_clip_step reads, when they are current, and the step number a table goes on
from.  Plain ints and numpy only -- no device tensor, no library call, no module.  Addresses are byte addresses; p / g / m / v are f32 arrays."""
import numpy as np

CHUNK = 65536                           # elements per chunk record: one workgroup of the norm and of the flat update kernel
CHUNK_BYTES, TILE_BYTES, TILE = 40, 56, 64        # sizeof(Chunk), sizeof(CastTile) of csrc/optim.hip (FusedAdamWClip holds them against the library's answers once); a tile's edge


def chunk_rows(tensors):
    """tensors: [(p, g, m, v addresses, numel)] in table order (the gradient norm folds its partial sums in it) -> (rows int64 [n, 5] = Chunk {p, g, m, v, n},
    every tensor cut into pieces of at most CHUNK elements; owner [n]: each row's index into `tensors`)."""
    rows = [(p + 4 * off, g + 4 * off, m + 4 * off, v + 4 * off, min(CHUNK, n - off), i) for i, (p, g, m, v, n) in enumerate(tensors) for off in range(0, n, CHUNK)]
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
    return np.ascontiguousarray(rows[:, :5]), rows[:, 5]


def flat_rows(rows, owner, tiled):
    """The rows the flat kernel updates: those of tensors not in `tiled` (indices into chunk_rows' list).  Nothing tiled: `rows` itself."""
    return rows[~np.isin(owner, sorted(tiled))] if tiled else rows


def tile_records(p, g, m, v, wc, wt, N, K):
    """The 64 x 64 tiles of a weight [N, K] (multiples of 64), row by row: int64 [N / 64 * K / 64, 7] = CastTile {float* p; const float* g; float* m; float* v;
    bf16_t* wc; bf16_t* wt; int K, N;} of csrc/optim.hip.  Every pointer names the tile's origin in its array: p / g / m / v and wc (16-bit) are [N, K] with row
    stride K, wt (16-bit) is the transpose [K, N] with row stride N.  The two ints share the seventh word, K in its low half (little endian)."""
    n0, k0 = np.meshgrid(np.arange(0, N, TILE, dtype=np.int64), np.arange(0, K, TILE, dtype=np.int64), indexing='ij')
    o, ot = (n0 * K + k0).reshape(-1), (k0 * N + n0).reshape(-1)
    return np.stack([p + 4 * o, g + 4 * o, m + 4 * o, v + 4 * o, wc + 2 * o, wt + 2 * ot, np.full_like(o, K | (N << 32))], axis=1)


def table_key(ids, grads, moments):
    """What the tables point at, per live parameter: (id(parameter), gradient address, first-moment address -- 0 before it exists)."""
    return tuple(zip(ids, grads, moments))


def tables_current(key, generation, built_key, built_generation, fuse_cast):
    """Current iff built for the same parameters with the same gradient and moment addresses (they move on the first step, with re-allocated gradients and
    with load_state_dict) and, when the update writes the module's operand copies (fuse_cast), for the same operand generation (they were re-allocated)."""
    return key == built_key and (not fuse_cast or generation == built_generation)


def step_base(counts):
    """The live parameters' own counts -> the one step number the whole table goes on from: the largest.  A parameter thawed after others have stepped starts
    its moments at zero and takes the others' bias correction: its first updates are smaller than torch.optim.AdamW's per-parameter count would make them,
    never larger; the max keeps a thawed parameter that happens to come first from resetting everybody's count."""
    return max(counts)

"""The strip plan of the stream sampler (k3::strip_plan) in a few lines of numpy, for the tests that compare the library's
plan with it, and the maps that follow from a plan: block -> (gene tile, strip), and the run words class by class."""
import numpy as np

from run_rule import run_words


def strip_plan(N, G, resident, strip_cells=0, taper=0):
    """(classes, tiles_g, blocks): classes = int32 rows {first cell, strip length, first block}."""
    tiles = -(-G // 256)
    L = 64
    while L > 8 and -(-N // L) * tiles < 4 * 5 * 1024:
        L //= 2
    L = 64 if strip_cells == 128 else strip_cells or L
    R, sizes, uniform = taper or resident, [], L
    if taper or (resident and -(-(-(-N // L)) // 4) * tiles >= 4 * resident):
        L = 128 if L == 64 and strip_cells != 64 else L          # the bulk of a graded plan
        for k in (1, 2, 3):
            s = max(64, (R * 4 * (L >> k) // max(tiles, 1) + 32) // 64 * 64)
            if (L >> k) < 8 or N - (sum(sizes) + s) < max(L, 64):
                break
            sizes.append(s)
    L = L if sizes else uniform
    sizes = ([(N - sum(sizes)) // max(L, 64) * max(L, 64)] + sizes) if sizes else [N]
    first = np.r_[0, np.cumsum(sizes)[:-1]].astype(np.int64)
    cells = np.r_[first[1:], N] - first                     # the last class takes the remainder
    lens = L >> np.arange(first.size)
    blocks = -(-(-(-cells // lens)) // 4) * tiles
    classes = np.c_[first, lens, np.r_[0, np.cumsum(blocks)[:-1]]].astype(np.int32)
    return classes, tiles, int(blocks.sum())


def strips_of_blocks(classes, tiles, blocks, N):
    """int64[blocks * 4, 3]: {gene tile, first cell, cells} of every region = 4 * block + wave (cells 0: no strip)."""
    out = np.zeros((blocks * 4, 3), np.int64)
    ends = np.r_[classes[1:, 0], N]
    next_block = np.r_[classes[1:, 2], blocks]
    for (first, length, fb), end, nb in zip(classes.tolist(), ends.tolist(), next_block.tolist()):
        strips = -(-(end - first) // length)
        groups = max(1, -(-strips // 4))
        tile, group = np.divmod(np.arange(nb - fb), groups)
        strip = group[:, None] * 4 + np.arange(4)
        n0 = first + strip * length
        cells = np.where(strip < strips, np.clip(end - n0, 0, length), 0)
        out[fb * 4:nb * 4] = np.stack([np.repeat(tile, 4).reshape(-1, 4), n0, cells], axis=-1).reshape(-1, 3)
    return out


def plan_run_words(row_of_cell, rows, classes):
    """run_rule.run_words applied class by class: uint32[N + 4]."""
    roc = np.asarray(row_of_cell)
    ends = np.r_[classes[1:, 0], roc.size]
    parts = [run_words(roc[first:end], rows, length)[:end - first] for (first, length, _), end in zip(classes.tolist(), ends.tolist())]
    return np.r_[np.concatenate(parts) if parts else np.zeros(0, np.uint32), np.ones(4, np.uint32)].astype(np.uint32)


def plan_loops(words, classes, N):
    """One letter per strip, in cell order: 'R' the run loop, 'T' the loop that loads per cell (run_rule.loops)."""
    from run_rule import loops
    ends = np.r_[classes[1:, 0], N]
    return "".join(loops(words[first:], end - first, length) for (first, length, _), end in zip(classes.tolist(), ends.tolist()))

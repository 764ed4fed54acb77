"""The run rule of the stream sampler's cell records (k3::run_word) in a few lines of numpy, for the tests that compare
the library's words with it, and which loop of the stream kernel each strip takes by it."""
import numpy as np

RUN_MIN_CELLS = 8      # k3::kRunMinCells


def run_words(row_of_cell, rows, strip_cells):
    """uint32[N + 4]: run length at a run's first cell (low 16 bits), runs of the strip at a strip's first cell (high
    16 bits), 0 elsewhere, 1 in the four entries behind the last cell.  Rows are clamped to [0, rows)."""
    row = np.clip(np.asarray(row_of_cell, np.int64), 0, rows - 1)
    N = row.size
    words = np.zeros(N + 4, np.uint32)
    words[N:] = 1
    for first in range(0, N, strip_cells):
        strip = row[first:first + strip_cells]
        starts = np.flatnonzero(np.r_[True, strip[1:] != strip[:-1]])
        words[first + starts] = np.diff(np.r_[starts, strip.size])
        words[first] |= starts.size << 16
    return words


def loops(words, N, strip_cells):
    """One letter per strip: 'R' the run loop (runs * RUN_MIN_CELLS <= cells), 'T' the loop that loads per cell."""
    out = []
    for first in range(0, N, strip_cells):
        cells = min(strip_cells, N - first)
        out.append("R" if (int(words[first]) >> 16) * RUN_MIN_CELLS <= cells else "T")
    return "".join(out)

"""The numpy model of THIN-1 (include/prosstt_amd_thin.h holds the definition; prosstt_amd/thin.py and libprosstt_amd_thin.so
evaluate it on the device).  A helper: nothing here is collected.

    mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31      (mod 2^64)
    Kc = mix(seed ^ mix(c + 0xE7037ED1A0B428DB));  Kg = mix(g + 0xA0761D6478BD642F);  K = mix(Kc ^ Kg)
    W(seed, c, g, w, b) = mix(K + 0x9E3779B97F4A7C15 (16 w + b + 1))
    bit 15 - b of U_t = bit (t mod 64) of W(seed, c, g, floor(t / 64), b);    y = #{t < x : lo <= U_t < hi}

``parts`` is the plain definition: all 16 planes of every trial are generated, the 16-bit uniforms are formed as numbers and
compared as numbers, with no shortcut.  ``parts_sliced`` restates what the kernel does, 64 trials per word with the planes
below the lowest set bit of lo | hi left out; tests/test_thin_model.py holds the two equal."""
import numpy as np

GRID = 65536
MAX_COUNT = 1 << 24
CELL_SALT = np.uint64(0xE7037ED1A0B428DB)
GENE_SALT = np.uint64(0xA0761D6478BD642F)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
CHUNK_WORDS = 1 << 14              # words of 64 trials whose uniforms are held at once


def _u64(v):
    return np.asarray(v).astype(np.uint64)


def mix(z):
    """The splitmix64 finaliser on uint64 arrays."""
    z = _u64(z)
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * M1
        z = z ^ (z >> np.uint64(27))
        z = z * M2
        return z ^ (z >> np.uint64(31))


def keys(seed, cells, genes):
    """K of the entries of ``cells`` and ``genes`` (arrays that broadcast), uint64."""
    with np.errstate(over="ignore"):
        kc = mix(np.uint64(seed) ^ mix(_u64(cells) + CELL_SALT))
        kg = mix(_u64(genes) + GENE_SALT)
        return mix(kc ^ kg)


def words(K, w, b):
    """W for the keys ``K``, the words ``w`` and the planes ``b`` (arrays that broadcast), uint64."""
    with np.errstate(over="ignore"):
        return mix(_u64(K) + GOLDEN * (np.uint64(16) * _u64(w) + _u64(b) + np.uint64(1)))


def _word_list(x):
    """(entry, word) of every word of 64 trials of the entries with the counts ``x``."""
    n_words = (x + 63) // 64
    entry = np.repeat(np.arange(x.size), n_words)
    first = np.cumsum(n_words) - n_words
    return entry, np.arange(entry.size) - first[entry]


def uniforms(K, w):
    """(len(w), 64) uint16: U_t of the trials t = 64 w .. 64 w + 63 of the keys ``K``: every plane, bit by bit."""
    W = words(K[:, None], w[:, None], np.arange(16)[None, :])                     # (words, 16)
    bits = np.unpackbits(np.ascontiguousarray(W).view(np.uint8).reshape(-1, 16, 8), axis=2, bitorder="little")   # (words, 16, 64)
    weight = (1 << (15 - np.arange(16))).astype(np.uint16)
    return (bits.astype(np.uint16) * weight[None, :, None]).sum(axis=1, dtype=np.uint16)


def uniform_matrix(K, x):
    """(len(K), x) uint16: U_t of the trials t < x of entries that all have the count ``x``."""
    K = _u64(K).ravel()
    n_words = (int(x) + 63) // 64
    out = np.empty((K.size, 64 * n_words), dtype=np.uint16)
    step = max(1, CHUNK_WORDS // n_words)
    for at in range(0, K.size, step):
        k = K[at:at + step]
        U = uniforms(np.repeat(k, n_words), np.tile(np.arange(n_words), k.size))
        out[at:at + step] = U.reshape(k.size, 64 * n_words)
    return out[:, :int(x)]


def parts(K, x, lo, hi):
    """y of flat entries with the keys ``K``, the counts ``x`` (0 .. 2^24) and the bounds ``lo``, ``hi`` (one per entry): the
    plain definition."""
    K, x = _u64(K).ravel(), np.asarray(x, dtype=np.int64).ravel()
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.int64), x.shape) for v in (lo, hi))
    assert x.size == 0 or (0 <= x.min() and x.max() <= MAX_COUNT)
    assert np.all((0 <= lo) & (lo <= hi) & (hi <= GRID))
    entry, w = _word_list(x)
    y = np.zeros(x.size, dtype=np.int64)
    for at in range(0, entry.size, CHUNK_WORDS):
        e, ww = entry[at:at + CHUNK_WORDS], w[at:at + CHUNK_WORDS]
        U = uniforms(K[e], ww).astype(np.int64)
        t = 64 * ww[:, None] + np.arange(64)[None, :]
        inside = (t < x[e][:, None]) & (lo[e][:, None] <= U) & (U < hi[e][:, None])
        np.add.at(y, e, inside.sum(axis=1))
    return y


def planes_needed(lo, hi):
    """16 - the trailing zeros of (lo | hi) mod 65536; 0 when that is 0."""
    m = (int(lo) | int(hi)) & (GRID - 1)
    return 16 - ((m & -m).bit_length() - 1) if m else 0


def _below(W, k, planes):
    """The word of the trials with U < k from the planes' words ``W`` (words, planes): the kernel's comparator."""
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    if k >> 16:
        return np.full(W.shape[0], ones)
    lt, eq = np.zeros(W.shape[0], dtype=np.uint64), np.full(W.shape[0], ones)
    for b in range(planes):
        if (k >> (15 - b)) & 1:
            lt |= eq & ~W[:, b]
            eq &= W[:, b]
        else:
            eq &= ~W[:, b]
    return lt


def parts_sliced(K, x, lo, hi):
    """The same y for ONE pair of bounds, as the kernel evaluates it: the needed planes only, 64 trials per word, the last
    word masked, a population count."""
    K, x = _u64(K).ravel(), np.asarray(x, dtype=np.int64).ravel()
    planes = planes_needed(lo, hi)
    if planes == 0:
        return x.copy() if (lo == 0 and hi == GRID) else np.zeros_like(x)
    entry, w = _word_list(x)
    W = words(K[entry][:, None], w[:, None], np.arange(planes)[None, :])
    inside = _below(W, int(hi), planes) & ~_below(W, int(lo), planes)
    last = (w + 1) * 64 > x[entry]
    keep = np.where(last, (np.uint64(1) << _u64(x[entry] % 64)) - np.uint64(1), np.uint64(0xFFFFFFFFFFFFFFFF))
    inside &= keep
    count = np.unpackbits(inside.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)
    y = np.zeros(x.size, dtype=np.int64)
    np.add.at(y, entry, count)
    return y


def interval(X, lo, hi, seed=0, cell_ids=None, gene_ids=None, sliced=False):
    """(N, G) int64: the part [lo, hi) of every entry of the integer matrix ``X``; ``lo``, ``hi`` one value or one per row;
    ``cell_ids`` (N,) and ``gene_ids`` (G,) default to 0 .. N - 1 and 0 .. G - 1.  An entry outside 0 .. 2^24 gives 0, as the
    device writes it."""
    X = np.asarray(X, dtype=np.int64)
    N, G = X.shape
    cells = np.arange(N) if cell_ids is None else np.asarray(cell_ids)
    genes = np.arange(G) if gene_ids is None else np.asarray(gene_ids)
    K = keys(seed, cells[:, None], genes[None, :])
    x = np.where((X < 0) | (X > MAX_COUNT), 0, X)
    if sliced:
        return parts_sliced(K, x, lo, hi).reshape(N, G)
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.int64).reshape(-1, 1), (N, G)) for v in (lo, hi))
    return parts(K, x, lo.ravel(), hi.ravel()).reshape(N, G)

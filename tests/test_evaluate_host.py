"""prosstt_amd/evaluate.py without a device: every refusal (all of them come before any device use), the statistics from
hand-made integer tables, and a Python mirror of the library's two block tables (tests/evaluate_model.py's ``plan``) that
shows which kinds of block and tile the cases of tests/test_gpu_evaluate.py reach.  No GPU."""
import numpy as np
import pytest

import evaluate_model as em
import test_gpu_evaluate as cases

from prosstt_amd import evaluate
from prosstt_amd.tree import Tree


def _fork():
    return Tree(topology=[["A", "B"], ["A", "C"]], time={"A": 20, "B": 20, "C": 20}, num_branches=3, branch_points=1, modules=0,
                G=4)


# ------------------------------------------------------------------------------------------------------- refusals

def test_pair_counts_refuses_before_any_device_use():
    a = np.arange(10)
    c = np.zeros(10, dtype=np.int64)
    bad = [
        dict(a=a.astype(float)), dict(a=a.reshape(2, 5)), dict(a=a[:9]), dict(a=a[:1], b=a[:1], classes=c[:1]),
        dict(a=a + (1 << 30)), dict(b=-a - (1 << 30)), dict(classes=c - 1), dict(classes=c + 64), dict(classes=c + 2, K=2),
        dict(classes=c.astype(float)), dict(K=0), dict(K=65), dict(K=2.0), dict(K=True), dict(tiles_per_block=-1),
        dict(tiles_per_block=4097), dict(tiles_per_block=1.0), dict(out="cupy"), dict(a="abc"),
        dict(a=np.full(10, 1 << 63, dtype=np.uint64)), dict(a=np.full(10, 1 << 30, dtype=np.uint32)),
        dict(classes=np.full(10, 64, dtype=np.uint8)),
    ]
    for change in bad:
        args = dict(a=a, b=a, classes=c, K=None, tiles_per_block=0, out="numpy")
        args.update(change)
        with pytest.raises(ValueError):
            evaluate.pair_counts(args["a"], args["b"], args["classes"], args["K"], tiles_per_block=args["tiles_per_block"],
                                 out=args["out"])
    # host integers of any kind travel as int64 with their values
    for dtype in (np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32):
        arr, on_device = evaluate._vector("a", np.array([0, 5, 100], dtype=dtype))
        assert arr.dtype == np.int64 and arr.tolist() == [0, 5, 100] and not on_device


def test_tree_moments_refuses_before_any_device_use():
    h = np.arange(10)
    c = np.zeros(10, dtype=np.int64)
    J = np.full((1, 1), em.MAX_DEPTH)
    bad = [
        dict(h=h - 1), dict(h=h + em.MAX_DEPTH), dict(h2=h + em.MAX_DEPTH), dict(h=h.astype(float)), dict(h=h[:9]),
        dict(classes=c + 1), dict(c2=c + 1), dict(c2=c - 1), dict(J=np.zeros((2, 3), dtype=int)), dict(J=np.zeros((65, 65), dtype=int)),
        dict(J2=np.array([[0, 1], [2, 0]])), dict(J=J.astype(float)), dict(J2=np.zeros((0, 0), dtype=int)), dict(ticks=0),
        dict(ticks=1.5), dict(tiles_per_block=4097), dict(out="list"),
        dict(h=h[:1], classes=c[:1], h2=h[:1], c2=c[:1]),
    ]
    for change in bad:
        args = dict(h=h, classes=c, J=J, h2=h, c2=c, J2=J, ticks=1, tiles_per_block=0, out="numpy")
        args.update(change)
        with pytest.raises(ValueError):
            evaluate.tree_moments(args["h"], args["classes"], args["J"], args["h2"], args["c2"], args["J2"], ticks=args["ticks"],
                                  tiles_per_block=args["tiles_per_block"], out=args["out"])


def test_the_tree_entry_points_refuse_before_any_device_use():
    t = _fork()
    pt = np.array([0, 5, 25, 30])
    br = np.array(["A", "A", "B", "C"])
    for call in (
            lambda: evaluate.pair_moments(t, pt, np.array(["A", "A", "B", "D"]), t, pt, br),          # no branch of the tree
            lambda: evaluate.pair_moments(t, pt, br, t, pt[:3], br[:3]),                               # other cells
            lambda: evaluate.pair_moments(t, pt, br, t, pt.astype(float) * np.nan, br),
            lambda: evaluate.pair_moments(t, pt, br, t, pt, br, ticks=2200),                           # 30 x 2200 > 65 535
            lambda: evaluate.pair_moments(t, pt, br, t, pt - 1.0, br),                                 # a negative depth
            lambda: evaluate.pair_moments(t, pt, br, t, pt, br, ticks=0),
            lambda: evaluate.pair_moments(t, pt, br, t, pt, br, out="x"),
            lambda: evaluate.pair_moments(t, pt.reshape(2, 2), br, t, pt, br),
            lambda: evaluate.ordering(t, pt, br, np.array([1.0, np.inf, 2.0, 3.0])),
            lambda: evaluate.ordering(t, pt, br, np.arange(3)),
            lambda: evaluate.ordering(t, pt, br, np.array(["a", "b", "c", "d"])),
            lambda: evaluate.ordering(t, pt[:1], br[:1], np.arange(1)),
            lambda: evaluate.ordering(t, pt, np.array(["A", "A", "B", "Z"]), pt),
            lambda: evaluate.labels(np.arange(4), np.arange(3)),
            lambda: evaluate.labels(np.arange(4.0), np.arange(4)),
            lambda: evaluate.labels(np.arange(4), np.full(4, -1)),
            lambda: evaluate.labels(np.arange(4).reshape(2, 2), np.arange(4)),
            lambda: evaluate.trajectory(t, pt, br, "a fit"),
            lambda: evaluate.trajectory(t, pt, br, (br,)),
    ):
        with pytest.raises(ValueError):
            call()
    # (three branches, 60 time steps: the depths and the junctions that the checks above guard)
    h, codes, J = evaluate._depths(evaluate._Nodes(t), pt, br, 16, "the tree")
    assert h.tolist() == [0, 80, 400, 480] and codes.tolist() == [0, 0, 1, 2]
    assert J.tolist() == [[65535, 65535, 65535], [65535, 65535, 19 * 16], [65535, 19 * 16, 65535]]


def test_a_tree_of_more_than_64_branches_is_refused():
    names = ["b%d" % i for i in range(65)]
    t = Tree(topology=[[names[i], names[i + 1]] for i in range(64)], time={n: 2 for n in names}, num_branches=65, branch_points=0,
             modules=0, G=4)
    with pytest.raises(ValueError, match="more than 64"):
        evaluate.ordering(t, np.array([0, 1]), np.array(["b0", "b0"]), np.array([0.0, 1.0]))


def test_check_status_names_the_bits():
    evaluate.check_status(0)
    for bit, name, _ in evaluate.STATUS_MESSAGES:
        with pytest.raises(ValueError, match=name):
            evaluate.check_status(bit)
    with pytest.raises(ValueError, match="OFFSETS_RANGE.*BRANCH_RANGE"):
        evaluate.check_status(evaluate.OFFSETS_RANGE | evaluate.BRANCH_RANGE)
    with pytest.raises(RuntimeError):
        evaluate.check_status(8)


# ------------------------------------------------------------------------------------------------------ statistics

def _hand_made():
    """Three classes, the second one empty."""
    s = np.array([[4, 0, -3], [0, 0, 0], [0, 0, 0]])
    p = np.array([[6, 0, 5], [0, 0, 0], [0, 0, 0]])
    a2 = np.array([[8, 0, 9], [0, 0, 0], [0, 0, 0]])
    b2 = np.array([[8, 0, 4], [0, 0, 0], [0, 0, 1]])
    return evaluate.PairCounts(s, p, a2, b2, evaluate.class_pairs([5, 0, 3]))


def test_the_statistics_of_hand_made_tables():
    pc = _hand_made()
    assert pc.pairs.tolist() == [[10, 0, 15], [0, 0, 0], [0, 0, 3]]
    assert pc.concordant().tolist() == [[5, 0, 1], [0, 0, 0], [0, 0, 0]] and pc.discordant().tolist() == [[1, 0, 4], [0, 0, 0], [0, 0, 0]]
    assert pc.gamma() == 1 / 11 and pc.tau_a() == 1 / 28 and pc.tau_b() == 1 / np.sqrt(17 * 13)
    diagonal = np.eye(3, dtype=bool)
    assert pc.gamma(diagonal) == 4 / 6 and pc.tau_a(diagonal) == 4 / 13 and pc.tau_b(diagonal) == 4 / np.sqrt(72)
    one = np.zeros((3, 3), dtype=bool)
    one[2, 0] = True                                    # a pair in either order
    assert pc.gamma(one) == -3 / 5 and pc.tau_a(one) == -3 / 15 and pc.tau_b(one) == -3 / 6
    # a class pair with no untied pair, an empty class and an empty selection: NaN, not an exception
    one[:] = False
    one[2, 2] = True
    assert np.isnan(pc.gamma(one)) and pc.tau_a(one) == 0.0 and np.isnan(pc.tau_b(one))
    one[:] = False
    one[1, 1] = True
    assert all(np.isnan(v) for v in pc.scores(one))
    assert all(np.isnan(v) for v in pc.scores(np.zeros((3, 3), dtype=bool)))
    per = pc.per_pair()
    assert per.gamma[0, 0] == 4 / 6 and per.gamma[0, 2] == -3 / 5 and np.isnan(per.gamma[1, 2]) and np.isnan(per.gamma[2, 0])
    assert per.tau_a[2, 2] == 0.0 and np.isnan(per.tau_a[1, 1])
    for mask in (np.ones((2, 2), dtype=bool), np.ones((3, 3)), "all"):
        with pytest.raises(ValueError):
            pc.gamma(mask)


def test_the_moments_of_hand_made_words():
    # one class pair holding the pairs (d, d2) = (1, 2), (2, 4), (4, 7); another with a sum above 2^64
    sums = np.zeros((2, 2, 5), dtype=object)
    sums[0, 0] = (7, 13, 21, 69, 38)
    big = (1 << 70) + 5
    sums[0, 1] = (3, 3, big, big, big)
    pm = evaluate.moments_from_words(em.words(sums), [[3, 4], [0, 0]], 2)
    assert pm.dd[0, 1] == big and pm.d[0, 0] == 7 and pm.dd2[1, 1] == 0
    one = np.array([[True, False], [False, False]])
    want = np.corrcoef([1, 2, 4], [2, 4, 7])[0, 1]
    assert abs(pm.pearson(one) - want) <= 1e-15
    assert pm.mean_distances(one) == (7 / 6, 13 / 6)
    assert np.isnan(pm.pearson(np.array([[False, False], [False, True]])))         # no pairs
    flat = evaluate.moments_from_words(em.words(np.array([[[6, 3, 12, 5, 6]]], dtype=object)), [[3]], 1)
    assert np.isnan(flat.pearson())                                                 # d = 2, 2, 2: no variance


def test_label_scores_of_hand_made_tables():
    ls = evaluate.label_scores([[5, 0], [0, 7]], ["x", "y"], [3, 9])
    assert (ls.ari, ls.accuracy, ls.n) == (1.0, 1.0, 12) and ls.matching == {"x": 3, "y": 9}
    assert abs(ls.nmi - 1.0) <= 1e-15                   # (logarithms in binary64: a few roundings of 2^-53)
    ls = evaluate.label_scores([[4, 1, 0], [0, 2, 3]])
    assert ls.accuracy == 7 / 10 and ls.jaccard.tolist() == [4 / 5, 3 / 5] and ls.f1.tolist() == [8 / 9, 6 / 8]
    assert evaluate.label_scores([[9]]).ari == 1.0 and evaluate.label_scores([[9]]).nmi == 1.0
    split = evaluate.label_scores([[3, 3]])                                         # one true class cut in two
    assert split.ari == 0.0 and split.nmi == 0.0 and split.accuracy == 0.5
    for bad in ([[0, 0]], [[-1, 2]], [1, 2], [[1.0]]):
        with pytest.raises(ValueError):
            evaluate.label_scores(bad)


# ---------------------------------------------------------------------------------------- the paths of the GPU cases

def _offsets(case):
    return np.concatenate([[0], np.cumsum(cases.SIZE_CASES[case])]).astype(np.int64)


def test_the_mirror_of_the_tables():
    rows, chunks = em.tables(np.array([0, 513, 513, 770]), 1)
    assert rows == [(0, 0, 512), (512, 0, 1), (513, 2, 257)]
    assert chunks == [(0, 0, 256), (256, 0, 256), (512, 0, 1), (513, 2, 256), (769, 2, 1)]
    # the bounds the workspace is sized by
    for case in cases.SIZE_CASES:
        offsets = _offsets(case)
        N, K = int(offsets[-1]), len(offsets) - 1
        for tiles in (1, 2, 3, em.MAX_TILES, em.default_tiles(N, K)):
            rows, chunks = em.tables(offsets, tiles)
            assert len(rows) <= -(-N // em.BLOCK_ROWS) + K and len(chunks) <= -(-N // (em.TILE * tiles)) + K
            assert sum(r[2] for r in rows) == N == sum(c[2] for c in chunks)
    assert em.default_tiles(50000, 8) == 4 and em.default_tiles(3000, 3) == 1 and em.default_tiles((1 << 31) - 1, 64) == em.MAX_TILES
    assert em.default_tiles(1 << 24, 64) >= 1


def test_the_gpu_cases_reach_every_kind_of_block():
    """Both GPU tests, of the counts and of the moments, run every case of SIZE_CASES at every entry of TILES: what is shown
    here holds for either pass."""
    import inspect
    for test in (cases.test_pair_counts_are_the_models_on_every_tiles_per_block,
                 cases.test_pair_moments_are_the_models_on_every_tiles_per_block):
        marks = [m for m in test.pytestmark if m.name == "parametrize" and m.args[0] == "case"]
        assert marks and list(marks[0].args[1]) == list(cases.SIZE_CASES) and "for tiles in TILES" in inspect.getsource(test)
    seen = {}
    for case in cases.SIZE_CASES:
        offsets = _offsets(case)
        for tiles in cases.TILES:
            tiles = tiles or em.default_tiles(int(offsets[-1]), len(offsets) - 1)
            for key, value in em.plan(offsets, tiles).items():
                seen.setdefault(key, {})[(case, tiles)] = value
    reached = lambda key: any(v > 0 for v in seen[key].values())          # noqa: E731
    for key in ("below", "skipped", "off_diagonal", "diagonal", "tiles_fast", "tiles_masked", "tiles_before", "ragged_tiles",
                "ragged_rows", "split_classes", "empty_classes"):
        assert reached(key), key
    # the particular ones the issue names
    p = em.plan(_offsets("tiles"), 1)                   # 1025, 256, 255, 512 at one tile per chunk
    assert p["skipped"] > 0 and p["tiles_masked"] > 0 and p["tiles_fast"] > p["tiles_masked"] and p["split_classes"] == 2
    p = em.plan(_offsets("tiles"), 3)                   # a chunk boundary inside the class of 1025, and tiles passed over
    assert p["split_classes"] == 1 and p["tiles_before"] > 0 and p["ragged_tiles"] > 0
    p = em.plan(_offsets("tiles"), em.MAX_TILES)        # one chunk per class: no block is skipped, tiles are passed over
    assert p["skipped"] == 0 and p["tiles_before"] > 0 and p["split_classes"] == 0
    p = em.plan(_offsets("K = 64"), 1)
    assert p["empty_classes"] > 20 and p["blocks"] == (64 - p["empty_classes"]) ** 2
    p = em.plan(_offsets("N = 2, one class"), 0 or 1)
    assert (p["blocks"], p["diagonal"], p["tiles_masked"]) == (1, 1, 1)
    # a diagonal block's fast tiles: columns wholly after its rows, in the same class
    p = em.plan(np.array([0, 1025]), 2)
    # rows (0, 512), (512, 512), (1024, 1) x chunks of the same spans: three blocks below the diagonal of the class are
    # skipped; (0, 0), (1, 1), (2, 2) meet their rows (2 + 2 + 1 tiles); (0, 1), (0, 2), (1, 2) lie after them (2 + 1 + 1)
    assert (p["diagonal"], p["skipped"], p["tiles_fast"], p["tiles_masked"], p["tiles_before"]) == (6, 3, 4, 5, 0)

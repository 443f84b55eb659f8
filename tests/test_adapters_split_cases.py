"""The batches of tests/_adapters_split_cases.py are what tests/test_adapters_split_geometry_gpu.py takes them for — checked on the
model and the mirrored formulas alone, without a GPU.  A batch exists to reach one edge of how csrc/adapters_split.hip cuts the work
(kPieceBases, kMaxPieces, kItemsPerGroup, kSplitWaves; adapters::kWarmup).  If one of them is retuned, a test here fails, on a CPU,
instead of the coverage vanishing silently."""
import numpy as np
import pytest

import _adapters_model as model
import _adapters_split_cases as cases
import _adapters_split_model as split


def test_mirrored_constants_are_the_sources():
    assert cases.source_constants() == cases.MIRRORED
    assert cases.WARMUP >= model.MAX_BASES + model.MAX_BASES * 40 // 100 and cases.WARMUP % 4 == 0
    assert cases.STEP_BASES == 2048


def test_pieces_per_group_classes():
    assert [cases.pieces_per_group(2 * n) for n in cases.PIECE_SETS] == [28, 16, 4]
    assert cases.pieces_per_group(2) == cases.MAX_PIECES < cases.ITEMS_PER_GROUP // 2                 # bound by the texts' room
    assert cases.pieces_per_group(64) == cases.ITEMS_PER_GROUP // 64 < cases.MAX_PIECES               # bound by the items
    assert cases.pieces_per_group(2 * model.MAX_SEQS) == 4                                            # the smallest


@pytest.mark.parametrize("kind", cases.PIECE_KINDS)
@pytest.mark.parametrize("n_seqs", cases.PIECE_SETS)
def test_piece_batches(n_seqs, kind):
    seqs, reads, counts, ppb = cases.piece_batch(n_seqs, kind)
    S = cases.PIECE_BASES
    assert [(len(r) + S - 1) // S for r in reads] == counts and ppb == cases.pieces_per_group(2 * len(seqs))
    total = sum(counts)
    groups = (total + ppb - 1) // ppb
    if kind == "below":
        assert total == ppb - 1 and groups == 1
    elif kind == "exact":
        assert total == ppb and groups == 1
    elif kind == "above":
        assert total == ppb + 1 and groups == 2
    else:
        assert groups >= 3 and total % ppb != 0
    start = np.concatenate(([0], np.cumsum(counts)))
    if kind == "partial":
        assert any(start[i] // ppb != (start[i + 1] - 1) // ppb for i in range(len(counts)))  # a read with pieces in two workgroups
    pats = model.patterns(seqs[:1])  # (the planted occurrences are exact: the first sequence alone finds them)
    marks = [split.marks(r, pats, 0) for r in reads]

    def hit_in(piece):
        r = int(np.searchsorted(start, piece, side="right")) - 1
        lo = (piece - int(start[r])) * S
        return bool(marks[r][lo:lo + S].any())

    for b in range(ppb, total, ppb):  # a hit on both sides of every workgroup boundary
        assert hit_in(b - 1) and hit_in(b), (n_seqs, kind, b)
    assert hit_in(0) and hit_in(total - 1)


@pytest.mark.parametrize("nc", cases.CHILD_COUNTS)
def test_child_count_batches(nc):
    pats = model.patterns([cases.GEOMETRY_ADAPTER])
    got = [split.split_of(r, 1, pats, 0, 0) for r in cases.child_count_batch(nc)]
    assert [len(g[3]) for g in got] == [0, nc, 0, 0] and all(g[0] == 0 and g[1] == 0 for g in got)
    assert nc < 1023 or len(cases.child_count_batch(nc)[1]) > 7 * cases.STEP_BASES  # several steps of the child walk


@pytest.mark.parametrize("n", cases.READ_COUNTS)
def test_read_count_batches(n):
    reads = cases.read_count_batch(n)
    pats = model.patterns([cases.GEOMETRY_ADAPTER])
    got = [split.split_of(r, 1, pats, 0, 0) for r in reads]
    assert len(reads) == n and len(got[-1][3]) == 2 and sum(len(g[3]) == 2 for g in got) >= n // 3
    assert {n % 256 for n in cases.READ_COUNTS} == {255, 0, 1} and (n + 1) % cases.SPLIT_WAVES in (0, 1, 2)

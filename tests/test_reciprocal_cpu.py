"""The numpy models of tests/reciprocal_model.py against brute force and against each other, and the argument checks of
seekr_amd.reciprocal and its users that need no device."""
import numpy as np
import pytest

import neighbors_cases as nc
import reciprocal_model as rm


def tied_r(rng, n1, n2, nan=0.05):
    """A dense r of few distinct values (ties decide almost every rank), some cells NaN."""
    r = np.array([-0.5, -0.0, 0.0, 0.25, 0.5], np.float32)[rng.integers(0, 5, (n1, n2))]
    r[rng.random((n1, n2)) < nan] = np.nan
    return r


def lists_of(r, k, self_form):
    a = nc.merge_block(r, k, exclude_diag=self_form)
    return a if self_form else a + rm.merge_cols_block(r, k, exclude_diag=False)


@pytest.mark.parametrize("mode", ["mutual", "union"])
@pytest.mark.parametrize("positive_only", [False, True])
def test_pairing_model_against_brute_force(mode, positive_only):
    rng = np.random.default_rng(31)
    for n1, n2, k in ((1, 1, 1), (7, 5, 2), (13, 17, 4), (9, 30, 40), (25, 6, 3)):
        r = tied_r(rng, n1, n2)
        got = rm.knn_pairs_model(*lists_of(r, k, False), mode=mode, positive_only=positive_only)
        assert rm.same_pairs(got, rm.brute_force_pairs(r, k, mode, positive_only)), (n1, n2, k)
    for n, k in ((1, 1), (2, 1), (12, 3), (21, 30)):
        r = tied_r(rng, n, n)
        got = rm.knn_pairs_model(*lists_of(r, k, True), mode=mode, positive_only=positive_only)
        assert rm.same_pairs(got, rm.brute_force_pairs(r, k, mode, positive_only, self_form=True)), (n, k)
        assert (got[0] < got[1]).all()


def test_mutual_is_a_subset_of_union_with_the_same_fields():
    rng = np.random.default_rng(32)
    for self_form in (False, True):
        n1, n2 = (15, 15) if self_form else (15, 11)
        idx_a, val_a = rm.random_lists(rng, n1, n2, 4, self_form)
        rest = (None, None) if self_form else rm.random_lists(rng, n2, n1, 4)
        mutual = rm.knn_pairs_model(idx_a, val_a, *rest, mode="mutual")
        union = rm.knn_pairs_model(idx_a, val_a, *rest, mode="union")
        fields = lambda p: zip(p[0].tolist(), p[1].tolist(), nc.bits(p[2]).tolist(), p[3].tolist(), p[4].tolist())  # noqa: E731
        by_pair = {(i, j): (v, a, b) for i, j, v, a, b in fields(union)}
        assert 0 < len(mutual[0]) < len(union[0])
        for i, j, v, a, b in fields(mutual):
            assert by_pair[(i, j)] == (v, a, b)
            assert a != rm.NO_RANK and b != rm.NO_RANK
        assert all((a == rm.NO_RANK) != (b == rm.NO_RANK) for p, (_, a, b) in by_pair.items()
                   if p not in set(zip(mutual[0].tolist(), mutual[1].tolist())))


@pytest.mark.parametrize("mode", ["mutual", "union"])
def test_self_form_is_the_two_set_form_on_the_same_lists(mode):
    """Fed idx as both sides, the two-set form holds (u, v) with rank_row from row u and rank_col from row v: the self
    form's pair (u, v), u < v, is that pair, with the value of the entry read from row u when there is one."""
    rng = np.random.default_rng(33)
    for n, k in ((9, 2), (20, 5), (6, 8)):
        idx, val = rm.random_lists(rng, n, n, k, self_form=True)
        two = rm.knn_pairs_model(idx, val, idx, val, mode=mode)
        keep = two[0] < two[1]
        assert rm.same_pairs(rm.knn_pairs_model(idx, val, mode=mode), tuple(x[keep] for x in two)), (n, k)


def test_merging_model_does_not_depend_on_the_row_split():
    rng = np.random.default_rng(34)
    for pattern in ("five_values", "specials", "equal"):
        for rows, width, k in ((9, 5, 3), (40, 7, 8), (23, 3, 30)):
            r = nc.fill(pattern, rows, width, 35)
            whole = rm.merge_cols_block(r, k, row0=100, col0=110)
            for parts in nc.MERGE_SPLITS:
                cuts = [0] + nc.split_points(rows, parts, 36) + [rows]
                running = None
                for p in range(len(cuts) - 1):
                    running = rm.merge_cols_block(r[cuts[p]:cuts[p + 1]], k, row0=100 + cuts[p], col0=110, running=running)
                assert np.array_equal(running[0], whole[0]) and np.array_equal(nc.bits(running[1]), nc.bits(whole[1])), (pattern, rows, parts)
    del rng


def test_a_nan_entry_never_pairs():
    idx_a = np.array([[0, 1], [1, nc.NO_CELL]], np.uint32)
    val_a = np.array([[np.nan, 0.5], [0.25, np.nan]], np.float32)
    idx_b = np.array([[0, 1], [0, 1]], np.uint32)
    val_b = np.array([[0.75, 0.5], [np.nan, 0.25]], np.float32)
    union = rm.knn_pairs_model(idx_a, val_a, idx_b, val_b, mode="union")
    # (0, 0): only b's entry counts; (0, 1): only a's; (1, 0): only b's; (1, 1): both
    assert list(zip(union[0], union[1])) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert list(union[3]) == [rm.NO_RANK, 1, rm.NO_RANK, 0] and list(union[4]) == [0, rm.NO_RANK, 1, 1]
    assert list(union[2]) == [0.75, 0.5, 0.5, 0.25]
    mutual = rm.knn_pairs_model(idx_a, val_a, idx_b, val_b, mode="mutual")
    assert list(zip(mutual[0], mutual[1])) == [(1, 1)]
    # self form: a NaN on one side leaves the pair to the other side alone
    idx = np.array([[1], [0]], np.uint32)
    val = np.array([[np.nan], [0.5]], np.float32)
    assert len(rm.knn_pairs_model(idx, val, mode="mutual")[0]) == 0
    got = rm.knn_pairs_model(idx, val, mode="union")
    assert (list(got[0]), list(got[1]), list(got[2]), list(got[3]), list(got[4])) == ([0], [1], [0.5], [rm.NO_RANK], [0])


def test_positive_only_filters_on_the_output_value():
    # pair (0, 1): the row side says -0.5, the column side 0.5: the output value is the row side's, so the pair goes
    idx_a, val_a = np.array([[1], [0]], np.uint32), np.array([[-0.5], [0.0]], np.float32)
    idx_b, val_b = np.array([[1], [0]], np.uint32), np.array([[0.75], [0.5]], np.float32)
    everything = rm.knn_pairs_model(idx_a, val_a, idx_b, val_b, mode="union")
    assert list(zip(everything[0], everything[1])) == [(0, 1), (1, 0)] and list(everything[2]) == [-0.5, 0.0]
    assert len(rm.knn_pairs_model(idx_a, val_a, idx_b, val_b, mode="union", positive_only=True)[0]) == 0
    # without the row side's entry the column side's value decides
    idx_a[0, 0] = nc.NO_CELL
    got = rm.knn_pairs_model(idx_a, val_a, idx_b, val_b, mode="union", positive_only=True)
    assert list(zip(got[0], got[1])) == [(0, 1)] and list(got[2]) == [0.5]


def test_model_refuses_an_index_out_of_range():
    with pytest.raises(ValueError):
        rm.knn_pairs_model(np.array([[2]], np.uint32), np.array([[1.0]], np.float32), np.array([[0], [0]], np.uint32),
                           np.array([[1.0], [1.0]], np.float32))
    with pytest.raises(ValueError):
        rm.knn_pairs_model(np.array([[1]], np.uint32), np.array([[1.0]], np.float32))


def test_value_errors_before_any_device_work(tmp_path):
    from seekr_amd import _lib, consumers, kmer_leiden, leiden, reciprocal
    assert _lib.TOPK_COLS_KMAX >= 32
    x = np.zeros((3, 16), np.float32)
    y = np.ones((4, 16), np.float32)
    for bad in (0, _lib.TOPK_COLS_KMAX + 1, 2.5):
        with pytest.raises(ValueError):
            reciprocal.reciprocal_hits(x, y, k=bad)
    for bad in (0, _lib.TOPK_MERGE_KMAX + 1):
        with pytest.raises(ValueError):
            reciprocal.reciprocal_hits(x, k=bad)
    assert reciprocal.check_k(_lib.TOPK_COLS_KMAX + 1, two_sets=False) == _lib.TOPK_COLS_KMAX + 1  # one set: the row kernel's limit
    with pytest.raises(ValueError):
        reciprocal.reciprocal_hits(x, y, k=3, mode="both")
    with pytest.raises(ValueError):
        consumers.knn_mode("either")
    with pytest.raises(ValueError):
        consumers.pearson_topk_both(None, None, k=_lib.TOPK_COLS_KMAX + 1)
    with pytest.raises(ValueError):
        leiden.pearson_communities(None, 0.1, knn=5)
    fasta = tmp_path / "s.fa"
    fasta.write_text(">a\nACGTACGTAC\n>b\nACGTTTGTAC\n")
    mean, std = np.zeros(16, np.float32), np.ones(16, np.float32)
    with pytest.raises(ValueError):
        kmer_leiden.kmer_leiden(str(fasta), mean, std, 2, knn=5, density=0.5)
    with pytest.raises(ValueError):
        kmer_leiden.kmer_leiden(str(fasta), mean, std, 2, knn=5, pearsoncutoff=0.1)
    with pytest.raises(ValueError):
        kmer_leiden.kmer_leiden(str(fasta), mean, std, 2, knn=0)
    with pytest.raises(ValueError):
        kmer_leiden.kmer_leiden(str(fasta), mean, std, 2, knn=5, knn_mode="both")

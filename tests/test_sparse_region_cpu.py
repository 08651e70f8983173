"""Sparse region edits, host side (chronoedit_amd/sparse_region.py): the active token set of a mask, the compute / refresh / sparse plan,
and the C ABI of the four gather / scatter passes (csrc/ce_sparse.hip).  No GPU."""
import pytest
import torch

from chronoedit_amd import hiplib, sparse_region as sr

ENTRY_POINTS = ("ce_sparse_patchify_bf16", "ce_sparse_scatter_rows_bf16", "ce_sparse_scatter_vt_bf16", "ce_sparse_unpatchify_bf16")


def ids_of(patches, T, Hp, Wp):
    """The token ids of a set of (i, j) patches in all T frames - the definition, spelled out."""
    return sorted((t * Hp + i) * Wp + j for t in range(T) for (i, j) in patches)


def check_list(ids, n_active, N):
    assert ids.dtype == torch.int64 and ids.dim() == 1
    assert ids.numel() % 8 == 0 or ids.numel() == N
    assert n_active <= ids.numel() < n_active + 8
    assert bool((ids[1:] > ids[:-1]).all()) and int(ids[0]) >= 0 and int(ids[-1]) < N  # sorted, unique, in range


def test_one_cell_marks_its_patch_and_the_margin_dilates_it():
    w = torch.zeros(12, 16)  # 6 x 8 patches
    w[5, 7] = 0.25           # patch (2, 3), through one of its four cells
    Hp, Wp, T = 6, 8, 2
    ids, n = sr.active_tokens(w, T, margin=0)
    assert n == 2
    check_list(ids, n, T * Hp * Wp)
    want = ids_of([(2, 3)], T, Hp, Wp)
    assert set(want) <= set(ids.tolist())
    # the padding: the lowest-index tokens that are not active
    assert ids.tolist() == sorted(want + [0, 1, 2, 3, 4, 5])
    ids1, n1 = sr.active_tokens(w, T, margin=1)
    assert n1 == 2 * 9
    check_list(ids1, n1, T * Hp * Wp)
    want1 = ids_of([(i, j) for i in (1, 2, 3) for j in (2, 3, 4)], T, Hp, Wp)
    assert set(want1) <= set(ids1.tolist()) and ids1.numel() == 24
    assert sorted(set(ids1.tolist()) - set(want1)) == [0, 1, 2, 3, 4, 5]


def test_a_feathered_edge_counts_wherever_the_weight_is_positive():
    w = torch.zeros(8, 12)  # 4 x 6 patches
    w[:, 4:] = torch.tensor([1e-6, 0.1, 0.5, 0.9, 1.0, 1.0, 1.0, 1.0])  # a ramp: the smallest positive weight already counts
    ids, n = sr.active_tokens(w, 1, margin=0)
    assert n == 4 * 4 and ids.tolist() == ids_of([(i, j) for i in range(4) for j in range(2, 6)], 1, 4, 6)
    w[:, 4] = 0.0  # column 4 leaves, column 5 keeps patch column 2 active
    assert sr.active_tokens(w, 1, margin=0)[1] == 16
    w[:, 5] = 0.0
    assert sr.active_tokens(w, 1, margin=0)[1] == 12


def test_two_islands_and_margins_at_the_border():
    w = torch.zeros(16, 20)  # 8 x 10 patches
    w[0, 0] = 1.0            # patch (0, 0): a corner
    w[15, 19] = 1.0          # patch (7, 9): the other corner
    T, Hp, Wp = 2, 8, 10
    ids0, n0 = sr.active_tokens(w, T, margin=0)
    assert n0 == 4 and set(ids_of([(0, 0), (7, 9)], T, Hp, Wp)) <= set(ids0.tolist())
    check_list(ids0, n0, T * Hp * Wp)
    ids2, n2 = sr.active_tokens(w, T, margin=2)  # clipped at the border: two 3 x 3 corners
    corners = [(i, j) for i in range(3) for j in range(3)] + [(i, j) for i in range(5, 8) for j in range(7, 10)]
    assert n2 == 2 * 18 and set(ids_of(corners, T, Hp, Wp)) <= set(ids2.tolist())
    check_list(ids2, n2, T * Hp * Wp)
    assert ids2.numel() == 40
    # the islands merge once the margin bridges them
    assert sr.active_tokens(w, T, margin=7)[1] == T * Hp * Wp


def test_a_full_grid_returns_all_tokens_and_an_empty_mask_only_padding():
    w = torch.ones(6, 10)  # 3 x 5 patches, 3 frames: 45 tokens, no multiple of 8 - and nothing left to pad with
    ids, n = sr.active_tokens(w, 3, margin=1)
    assert n == 45 and ids.tolist() == list(range(45))
    ids, n = sr.active_tokens(torch.zeros(6, 10), 3, margin=3)
    assert n == 0 and ids.numel() == 0
    with pytest.raises(ValueError):
        sr.active_tokens(torch.ones(5, 10), 1)
    with pytest.raises(ValueError):
        sr.active_tokens(torch.ones(6, 10), 1, margin=-1)


def test_validate_ids():
    good = torch.tensor([0, 3, 4, 159])
    assert sr.validate_ids(good, 160).tolist() == [0, 3, 4, 159]
    assert sr.validate_ids(good.to(torch.int32), 160).dtype == torch.int64
    for bad in (torch.tensor([0, 3, 3]), torch.tensor([4, 3]), torch.tensor([0, 160]), torch.tensor([-1, 2]), torch.tensor([], dtype=torch.int64),
                torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]])):
        with pytest.raises(ValueError):
            sr.validate_ids(bad, 160)


def dense_before_sparse(plan):
    """Every sparse step has a refresh behind the last compute step in front of it."""
    last = None
    for k in plan:
        if k == "sparse":
            assert last == "refresh", plan
        else:
            last = k
    return True


def test_plan_refresh_every_and_the_refresh_compute_distinction():
    C = sr.SparseRegionConfig
    assert sr.plan(6, C(3), ()) == ["refresh", "sparse", "sparse", "refresh", "sparse", "sparse"]
    assert sr.plan(7, C(3), ()) == ["refresh", "sparse", "sparse", "refresh", "sparse", "sparse", "compute"]  # nobody reads a last refresh
    assert sr.plan(5, C(2), ()) == ["refresh", "sparse", "refresh", "sparse", "compute"]
    assert sr.plan(4, C(1), ()) == ["compute"] * 4
    assert sr.plan(4, C(100), ()) == ["refresh", "sparse", "sparse", "sparse"]
    assert sr.plan(4, C(2), (), full=True) == ["compute"] * 4
    assert sr.plan(0, C(2), ()) == []
    for n in range(1, 12):
        for every in range(1, 6):
            for start in (0.0, 0.3, 1.0):
                p = sr.plan(n, C(every, start=start), ())
                assert len(p) == n and dense_before_sparse(p) and set(p) <= set(sr.KINDS)
                if every == 1 or start == 1.0:
                    assert p == ["compute"] * n
                elif start == 0.0 and n > 1:
                    assert p[:2] == ["refresh", "sparse"]
                assert p[-1] != "refresh"


def test_plan_start_and_forced_steps():
    C = sr.SparseRegionConfig
    # first = ceil(0.5 * 8) = 4: steps 0..3 dense, step 4 is the first of the count
    assert sr.plan(8, C(2, start=0.5), ()) == ["compute"] * 4 + ["refresh", "sparse", "refresh", "sparse"]
    assert sr.plan(8, C(3, start=0.3), ()) == ["compute"] * 3 + ["refresh", "sparse", "sparse", "refresh", "sparse"]
    # the truncation at step 2 forces steps 0, 1, 2; the count restarts behind them
    assert sr.plan(8, C(3), (0, 1, 2)) == ["compute"] * 3 + ["refresh", "sparse", "sparse", "refresh", "sparse"]
    assert sr.plan(6, C(2), (0, 1, 2)) == ["compute"] * 3 + ["refresh", "sparse", "compute"]
    # a step forced later (a callback replaced the latents behind step 3): dense, and the count restarts behind it
    p = sr.plan(8, C(3), (4,))
    assert p == ["refresh", "sparse", "sparse", "compute", "compute", "refresh", "sparse", "sparse"] and dense_before_sparse(p)
    for forced in ((1,), (2, 3), (0, 5), (7,)):
        p = sr.plan(8, C(3), forced)
        assert all(p[f] != "sparse" for f in forced) and dense_before_sparse(p)


def test_config_validation_and_report():
    C = sr.SparseRegionConfig
    assert C(2).start == 0.0 and C(2).margin == 1
    for kw in (dict(refresh_every=0), dict(refresh_every=1.5), dict(refresh_every=True), dict(refresh_every=2, start=-0.1),
               dict(refresh_every=2, start=1.5), dict(refresh_every=2, start=float("nan")), dict(refresh_every=2, margin=-1),
               dict(refresh_every=2, margin=0.5)):
        with pytest.raises(ValueError):
            C(**kw)
    p = sr.plan(7, C(3), ())
    assert sr.report(p, 64, 160) == {"plan": p, "compute": 1, "refresh": 2, "sparse": 4, "active": 64, "tokens": 160}


def test_the_c_abi_declares_the_four_entry_points():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_sparse_")] == list(ENTRY_POINTS)
    assert "ce_sparse.hip" in hiplib.SOURCES
    from chronoedit_amd import ops
    for fn in ("sparse_patchify", "sparse_scatter_rows_", "sparse_scatter_vt_", "sparse_unpatchify_"):
        assert callable(getattr(ops, fn))

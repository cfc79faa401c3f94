"""CPU side of the exact nearest-neighbour tests: the probe helper (tests/_knn_probe.py) is held to itself and to the oracle
before a GPU is touched -- the set-mode decode under the blend's fp32 fmaf chain, the brute-force reference against
oracle.field_set_forward_knn, the near-tie screen's counts on every layout test_gpu_knn_exact.py uses, and the gap that file
closes: the blend at distance_factor = 10 accepts a wrong K-th neighbour, the set-mode check rejects it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_probe as Q  # noqa: E402
from oracle import ngm_oracle as O  # noqa: E402

FS = O.FieldSpec(**Q.NERF16)


def test_probe_fields_output_their_code_everywhere():
    NF = 5
    codes = Q.int_codes(NF, 1)
    params = Q.probe_params(FS, NF, codes)
    assert sum(v[0].numel() for v in params.values()) == 276
    x = torch.randn(NF, 33, 3, generator=torch.Generator().manual_seed(0)) * 3
    out = O.field_forward_local(x, params, FS)
    assert torch.equal(out, codes.float()[:, None, :].expand(NF, 33, 4))


@pytest.mark.parametrize("K", list(range(1, 17)))
def test_set_mode_decode_survives_the_fp32_fmaf_chain(K):
    """round(K out) is the exact sum of the K codes: worst distance of K out from the integer over random code sets and the
    extreme ones (all 4095, all 0, alternating), against the rounding margin 0.5"""
    g = np.random.default_rng(K)
    sets = g.integers(0, Q.CODE_RANGE, (20000, K, 4))
    sets[0], sets[1] = Q.CODE_RANGE - 1, 0
    sets[2] = np.where(np.arange(K)[:, None] % 2 == 0, Q.CODE_RANGE - 1, 0)
    sets[3] = np.where(np.arange(K)[:, None] % 2 == 0, 0, Q.CODE_RANGE - 1)
    out = Q.emulate_set_blend(K, sets)
    worst = float(np.abs(K * out.astype(np.float64) - sets.sum(1)).max())
    print(f"K={K}: worst |K out - sum| = {worst:.4f}")
    assert worst < 0.05                                                   # a tenth of the margin
    assert torch.equal(Q.decode_sums(torch.from_numpy(out), K), torch.from_numpy(sets.sum(1)))


def test_brute_force_orders_ties_by_field_index():
    pos = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [-1.0, 0, 0], [0, 0, 2.0], [0, -1.0, 0], [0, 0, 0.5]])
    idx, d2 = Q.brute_force(torch.zeros(1, 3), pos, kmax=3)
    assert idx.tolist() == [[5, 0, 1, 2]] and d2.tolist() == [[0.25, 1.0, 1.0, 1.0]]
    idx, d2 = Q.brute_force(torch.zeros(3, 3), pos, kmax=16, chunk=2)     # fewer centres than kmax + 1: all of them, ordered
    assert idx.tolist() == [[5, 0, 1, 2, 4, 3]] * 3


@pytest.mark.parametrize("K", [1, 3, 8, 14])
def test_reference_agrees_with_the_oracle_on_tie_free_inputs(K):
    """the oracle's own forward (topk on its own distances) against the softmax blend over the brute-force sets, in fp64, with
    probe fields of real codes at distance_factor 0.5 (every weight of order 1 / K: a wrong member shows) and 10"""
    NF, P = 300, 1500
    pos = Q.cover_lattice(NF, seed=21, noise=1e-3)
    pts = Q.points_in_box(pos, P, 21)
    codes = Q.real_codes(NF, 21)
    params = {k: v.double() for k, v in Q.probe_params(FS, NF, codes).items()}
    exp = Q.expect(Q.brute_force(pts, pos), K)
    assert int(exp.undecided.sum()) == 0 and 0.25 < exp.share() < 0.9
    for df in (0.5, 10.0):
        ref = O.field_set_forward_knn(pts.double(), pos.double(), Q.unit_quats(NF).double(), params, FS, num_knn=K,
                                      distance_factor=df, outside_value=Q.OUTSIDE)
        assert torch.equal((ref == Q.OUTSIDE).all(-1), ~exp.inside)
        mine = Q.softmax_blend64(exp, codes, df)
        torch.testing.assert_close(ref[exp.inside], mine[exp.inside], rtol=0, atol=1e-13)


@pytest.mark.parametrize("name", list(Q.LAYOUTS))
def test_screen_leaves_out_at_most_one_percent_on_every_gpu_layout(name):
    """the condition of the GPU file, known to hold before a GPU is touched: per layout and K, undecided points <= 1 %"""
    pos, pts, ref = Q.layout_case(name)
    for K in (1, 2, 8, 11, 16):
        exp = Q.expect(ref, K, exact_ties=name in Q.EXACT_TIES)
        n = Q.check_screen(f"{name} K={K}", exp)
        print(f"{name}: NF={pos.shape[0]} K={exp.K} points={exp.P} inside={exp.share():.3f} undecided={n}")
        assert exp.share() > 0.1


def test_thresholds_of_the_assignment_paths():
    """the smallest maps past each run-time threshold of ngm_knn.hip, from its own formulas"""
    assert Q.nf_grid_not_in_lds() == 1261              # 52 NF + 4 bytes of histogram, centres and 8 NF + 1 cell offsets > 64 KB
    assert Q.grid_in_lds_bytes(1260) == 65524 and Q.grid_in_lds_bytes(1261) > 65536
    assert Q.nf_global_histograms() == 38401           # 4 NF > 150 KB
    # the grid's exclusive scan works in rounds of 1024 cells: one cell in the second round
    assert Q.grid_cells(Q.LAYOUTS["scan_round_1025"]()[0]) == 1025


@pytest.mark.parametrize("spacing", [0.5, 1.0, 1.5])
def test_dyadic_cases_are_exact_and_full_of_ties(spacing):
    """every coordinate a multiple of 1/8: fp32 squared distances equal the fp64 ones bit for bit, so no point is undecided; a
    large share of the points has an exact tie at the K-th place, and the row order changes which geometric centres win"""
    pts = Q.dyadic_points(spacing)
    assert pts.shape[0] <= 4096
    geo = []
    for seed in (0, 1):
        pos, perm = Q.dyadic_lattice(spacing, seed=seed)
        ref = Q.brute_force(pts, pos)
        d32 = ((pts[:, None, :] - pos[ref[0]]) ** 2).sum(-1)
        assert torch.equal(d32.double(), ref[1])
        for K in (1, 2, 4, 8, 9, 16):
            exp = Q.expect(ref, K, exact_ties=True, exact_radius=True)
            assert Q.check_screen("dyadic", exp, cap=0.0) == 0
            assert int(exp.tied.sum()) > 0.05 * exp.P, (K, int(exp.tied.sum()))
        exp = Q.expect(ref, 4, exact_ties=True, exact_radius=True)
        geo.append(torch.sort(perm[exp.idx], dim=1).values)
    assert int((geo[0] != geo[1]).any(-1).sum()) > 0.05 * pts.shape[0]
    if spacing == 1.5:                                 # an edge midpoint: two centres at 0.75, then four tied at sqrt(0.75^2 + 1.5^2)
        i = int((pts == torch.tensor([0.75, 1.5, 1.5])).all(-1).nonzero()[0])
        assert ref[1][i, :6].tolist() == [0.5625, 0.5625] + [0.5625 + 2.25] * 4


def test_the_blend_at_factor_ten_accepts_a_wrong_kth_neighbour_and_set_mode_rejects_it():
    """The gap, shown on the host (no kernel is broken): with the oracle's blend at distance_factor = 10 and K = 14, replacing
    every point's K-th neighbour by its (K+1)-th stays within the existing tests' rtol 3e-4 / atol 3e-5 on at least 99 % of the
    inside points; the set-mode check rejects the same swap on every decided inside point."""
    NF, P, K = 300, 3000, 14
    pos = Q.cover_lattice(NF, seed=31, noise=1e-3)
    quat = Q.unit_quats(NF, 31)
    pts = Q.points_in_box(pos, P, 31)
    ref = Q.brute_force(pts, pos)
    exp = Q.expect(ref, K)
    swapped_idx = torch.cat([ref[0][:, :K - 1], ref[0][:, K:K + 1]], 1)
    swapped_d2 = torch.cat([ref[1][:, :K - 1], ref[1][:, K:K + 1]], 1)
    params = O.init_params(FS, NF, seed=31, sigma=3.0)
    p64 = {k: v.double() for k, v in params.items()}
    args = (pts.double(), pos.double(), quat.double(), p64, FS)
    good = Q.oracle_blend_on_sets(*args, exp.idx, exp.d2, exp.inside)
    torch.testing.assert_close(good, O.field_set_forward_knn(*args, num_knn=K, distance_factor=10.0, outside_value=1.0), rtol=0, atol=1e-13)
    bad = Q.oracle_blend_on_sets(*args, swapped_idx, swapped_d2, exp.inside)
    within = ((bad - good).abs() <= 3e-5 + 3e-4 * good.abs()).all(-1)
    n_in = int(exp.inside.sum())
    beyond = int((~within & exp.inside).sum())
    print(f"K={K}: {n_in} inside points, {beyond} beyond the blend tests' tolerance after the swap")
    assert n_in > 1000 and beyond <= 0.01 * n_in
    # set mode on the same swap: the blend the kernels would return for the swapped sets, through the fp32 chain
    codes = Q.int_codes(NF, 31)
    out_good = torch.from_numpy(Q.emulate_set_blend(K, codes[exp.idx].numpy()))
    out_bad = torch.from_numpy(Q.emulate_set_blend(K, codes[swapped_idx].numpy()))
    out_good[~exp.inside] = Q.OUTSIDE
    out_bad[~exp.inside] = Q.OUTSIDE
    dec_in = exp.inside & ~exp.undecided
    assert int(exp.undecided.sum()) <= 0.01 * P
    assert bool(Q.set_mode_accepts(out_good, exp, codes).all())
    assert not bool(Q.set_mode_accepts(out_bad, exp, codes)[dec_in].any())
    with pytest.raises(AssertionError, match="neighbour set wrong"):
        Q.check_set("swapped", out_bad, exp, codes, pts)
    Q.RECORDS.pop()
    Q.check_set("unswapped", out_good, exp, codes, pts)
    Q.RECORDS.pop()

"""-m gpu: the nearest-neighbour assignment of ngm_knn.hip held to brute force -- exact neighbour SETS, the tie rule, the
strict inside test and the boundary shapes of its bookkeeping stages -- through the public ops.field_eval_knn /
ops.grid_eval_knn and probe fields (tests/_knn_probe.py: a field that outputs a 4-vector code everywhere, so the blend is
sum_k w_k code[f_k]).

Set mode (distance_factor 0, integer codes): round(K out) is the exact sum of the K codes, compared with torch.equal against
the sums over the brute-force set (fp64, all centres, ordered by (squared distance, field index)).  Points on which two correct
fp32 implementations may disagree (the near-tie screen of the helper) are left out; no case leaves out more than 1 % of its
points, the dyadic cases -- exact arithmetic, ties everywhere -- leave out none.  tests/test_knn_probe_cpu.py checks the
helper, the screen's counts on these very layouts and, on the host, that the blend tests accept a wrong K-th neighbour which
this check rejects.

What is pinned: which fields every point blends, which points are outside, that every pair reaches its own field's weights,
and (weights mode) the softmax weights.  Not observable and not claimed: the order of the neighbours inside a point's list.
With NGM_KNN_EXACT_REPORT=<file> the figures of every case are written there at the end of the module
(profiles/r16_knn_exact.txt is such a file)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_probe as Q  # noqa: E402
from gpu_common import DEV, cu  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from oracle import ngm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

FS = O.FieldSpec(**Q.NERF16)
ALL_K = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16]
_DEVICE = {}


@pytest.fixture(scope="module", autouse=True)
def figures():
    n0 = len(Q.RECORDS)
    yield
    report = os.environ.get("NGM_KNN_EXACT_REPORT")
    if report:
        os.makedirs(os.path.dirname(os.path.abspath(report)), exist_ok=True)
        with open(report, "w") as fh:
            fh.write(Q.format_records(Q.RECORDS[n0:]))


def fcfg(mode="auto", **kw):
    return K.field_cfg(**Q.NERF16, matmul_mode=mode, **kw)


def probe(NF, codes, key=None):
    """probe fields of `codes` on the device (cached by `key`: the 38 401-field map is 43 MB)"""
    if key is None:
        return cu(Q.probe_params(FS, NF, codes))
    if key not in _DEVICE:
        _DEVICE[key] = cu(Q.probe_params(FS, NF, codes))
    return _DEVICE[key]


def evaluate(pos, pts, codes, K_, distance_factor=0.0, mode="auto", key=None, **kw):
    NF = pos.shape[0]
    out = ops.field_eval_knn(fcfg(mode), probe(NF, codes, key), pts.to(DEV), pos.to(DEV), Q.unit_quats(NF).to(DEV), K_, distance_factor,
                             Q.OUTSIDE, **kw)
    return out.cpu()


def set_case(name, K_, **kw):
    """a named layout of the helper in set mode at K_"""
    pos, pts, ref = Q.layout_case(name)
    codes = Q.int_codes(pos.shape[0], len(name))
    exp = Q.expect(ref, K_, exact_ties=name in Q.EXACT_TIES)
    out = evaluate(pos, pts, codes, K_, key=name, **kw)
    return Q.check_set(f"{name}", out, exp, codes, pts), exp


# ------------------------------------------------------------------------------------------------ premise
@pytest.mark.parametrize("mode", ["auto", "f32"])
def test_premise_one_neighbour_returns_the_nearest_fields_code_bit_for_bit(mode):
    """K = 1: out == code[nearest] under torch.equal, integer and real codes.  Everything else in this file leans on it: the
    evaluation adds nothing to a probe field's code, and the blend's single fmaf(1, v, 0) returns it."""
    pos, pts, ref = Q.layout_case("cover300")
    exp = Q.expect(ref, 1)
    Q.check_screen("premise", exp)
    m = exp.inside & ~exp.undecided
    assert int(m.sum()) > 1000
    for codes in (Q.int_codes(300, 0).float(), Q.real_codes(300, 0)):
        out = evaluate(pos, pts, codes, 1, mode=mode)
        assert torch.equal(out[m], codes[exp.idx[:, 0]][m]), int((out[m] != codes[exp.idx[:, 0]][m]).any(-1).sum())
        assert bool((out[~exp.inside & ~exp.undecided] == Q.OUTSIDE).all())


# ------------------------------------------------------------------------------------------------ A: every K instance
@pytest.mark.parametrize("K_", ALL_K)
def test_a_every_k_instance_on_the_exact_cover_lattice(K_):
    """300 nodes of the exact cover lattice (no noise, shuffled rows), random points up to two radii beyond the map"""
    rec, exp = set_case("cover300", K_)
    assert 0.25 <= exp.share() <= 0.9, exp.share()


# ------------------------------------------------------------------------------------------------ B: every assignment path
B_CASES = ["lds_edge_below", "grid_not_in_lds", "near_inline_2048", "near_kernels_2049", "global_histograms_38401", "scan_round_1025",
           "clusters20", "sparse50", "single_field", "identical5", "collinear40", "coplanar40"]


@pytest.mark.parametrize("K_", [2, 11])
@pytest.mark.parametrize("name", B_CASES)
def test_b_every_assignment_path(name, K_):
    """grid_not_in_lds: 1 261 fields, the smallest map whose grid (52 NF + 4 bytes) no longer fits the 64 KB the assignment keeps
    it in (lds_edge_below: 1 260, the last that does); near_kernels_2049: candidate lists by the three device-wide kernels
    (near_inline_2048: the last map one workgroup lists); global_histograms_38401: 4 NF > 150 KB, per-pair global atomics;
    scan_round_1025: a 5 x 5 x 41 lattice, 1 025 cells, one past a round of the one-workgroup scan of the cell counts (the other
    maps' grids have 1 331, 2 197 and 39 304 cells, 149 to 392 past a round; the candidate lists' lengths are multiples of 8);
    clusters20 / sparse50: the coarsened grid, phase B over several rings; one field, five identical centres (every distance
    ties: the lowest indices win), 40 collinear and 40 coplanar centres: grids of one cell, one row, one plane"""
    assert Q.nf_grid_not_in_lds() == 1261 and Q.nf_global_histograms() == 38401
    rec, exp = set_case(name, K_)
    assert exp.share() > 0.1
    if name == "identical5":
        assert exp.K == min(K_, 5) and (exp.K == 5 or bool(exp.tied[exp.inside].all()))
        assert bool((exp.idx == torch.arange(exp.K)).all())


def test_b_sparse_map_eight_neighbours():
    """50 centres in a 60^3 box, K = 8: the eighth neighbour is several rings of coarsened cells away, phase B iterates"""
    rec, exp = set_case("sparse50", 8)
    assert float(torch.sqrt(exp.d2[:, 7]).median()) > 10.0


# ------------------------------------------------------------------------------------------------ C: ties, dyadic
@pytest.mark.parametrize("K_", [1, 2, 4, 8, 9, 16])
@pytest.mark.parametrize("spacing", [0.5, 1.0, 1.5])
def test_c_exact_ties_follow_the_index_rule(spacing, K_):
    """Centres on a lattice of spacing 0.5 / 1.0 / 1.5, radius 1.0, every coordinate a multiple of 1/8: all fp32 arithmetic is
    exact (contraction cannot matter), ties are everywhere (cell vertices, edge midpoints, face and body centres, a 1/8-step
    lattice).  Spacing 1.0 keeps >= K centres within the radius for small K (phase A, 64-bit keys) and spacing 0.5 -- several
    centres per grid cell -- for every K, the 16-slot instance included; spacing 1.5 at K = 4 has two centres inside the
    radius and then four tied across cells the scan visits in different orders (phase B).  No point is left out.
    Twice, with two row orders of the same centres: the geometric centres chosen must follow the index rule each time."""
    pts = Q.dyadic_points(spacing)
    for seed in (0, 1):
        pos, perm = Q.dyadic_lattice(spacing, seed=seed)
        codes = Q.int_codes(64, 50 + seed)
        exp = Q.expect(Q.brute_force(pts, pos), K_, exact_ties=True, exact_radius=True)
        assert int(exp.tied.sum()) > 0.05 * exp.P
        out = evaluate(pos, pts, codes, K_)
        rec = Q.check_set(f"dyadic spacing {spacing} rows {seed}", out, exp, codes, pts, cap=0.0)
        assert rec["undecided"] == 0


# ------------------------------------------------------------------------------------------------ D: the inside boundary
@pytest.mark.parametrize("K_", [1, 2])
@pytest.mark.parametrize("mask_radius", [None, 1.25, 0.5])
def test_d_the_inside_test_is_strict(mask_radius, K_):
    """Points at exactly the radius from their only near centre are outside, points at radius - 2^-10 inside (dyadic: exact).
    mask_radius 1.25 > 1.1547 field_radius sets the cell size; 0.5 is below it."""
    r = mask_radius or 1.0
    pos, pts, own, inside = Q.boundary_case(r)
    codes = Q.int_codes(8, 60)
    exp = Q.expect(Q.brute_force(pts, pos), K_, radius=r, exact_ties=True, exact_radius=True)
    assert torch.equal(exp.inside, inside) and torch.equal(exp.idx[:, 0], own)
    assert bool((torch.sqrt(exp.d2[~inside, 0]) == r).all())
    out = evaluate(pos, pts, codes, K_, mask_radius=mask_radius)
    Q.check_set(f"boundary radius {r}", out, exp, codes, pts, cap=0.0)
    assert bool((out[~inside] == Q.OUTSIDE).all()) and bool((out[inside] != Q.OUTSIDE).any(-1).all())


# ------------------------------------------------------------------------------------------------ E: weights
@pytest.mark.parametrize("K_", [4, 12])
@pytest.mark.parametrize("distance_factor", [0.5, 10.0])
def test_e_softmax_weights(distance_factor, K_):
    """Real codes in [-1, 1] on the case-A map against the fp64 softmax over the reference's own set.  The bar is 4 x the worst
    error of a plain fp32 restatement (torch sqrt, softmax, the fmaf-order sum) against that fp64 reference on the same points:
    the kernels' expf is another one.  At distance_factor 0.5 every weight is of order 1 / K: a weight on the wrong pair shows."""
    pos, pts, ref = Q.layout_case("cover300")
    codes = Q.real_codes(300, 70)
    exp = Q.expect(ref, K_)
    m = exp.inside & ~exp.undecided
    restated = float((Q.softmax_blend32(exp, pts, pos, codes, distance_factor).double() - Q.softmax_blend64(exp, codes, distance_factor))[m].abs().max())
    assert 0 < restated < 1e-5
    out = evaluate(pos, pts, codes, K_, distance_factor=distance_factor)
    Q.check_weights(f"weights factor {distance_factor}", out, exp, codes, distance_factor, 4 * restated, restated)


# ------------------------------------------------------------------------------------------------ F: bookkeeping edges
def _around(centre, n, seed):
    """n points within 0.5 of `centre`"""
    g = torch.Generator().manual_seed(seed)
    v = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 0.5 * torch.rand(n, 1, generator=g)
    return centre + v


def _counted_case(case, pos, loads, seed):
    """K = 1: exactly loads[f] points inside field f (centres far apart), some points outside every field, shuffled"""
    g = torch.Generator().manual_seed(seed)
    pts = torch.cat([_around(pos[f], n, seed + f) for f, n in loads.items()] + [pos[list(loads)[0]] + torch.tensor([3.0, 3.0, 3.0]) + torch.rand(37, 3, generator=g)])
    pts = pts[torch.randperm(pts.shape[0], generator=g)].contiguous()
    codes = Q.int_codes(pos.shape[0], seed)
    exp = Q.expect(Q.brute_force(pts, pos), 1)
    got = torch.bincount(exp.idx[exp.inside, 0], minlength=pos.shape[0])
    want = torch.zeros(pos.shape[0], dtype=torch.int64)
    for f, n in loads.items():
        want[f] = n
    assert torch.equal(got, want) and int((~exp.inside).sum()) == 37
    out = evaluate(pos, pts, codes, 1)
    rec = Q.check_set(case, out, exp, codes, pts, cap=0.0)
    assert rec["undecided"] == 0


def test_f_tiles_of_512_513_and_1_pairs():
    """three far-apart fields that receive exactly 512, 513 and 1 pairs: a full tile, a tile and one pair, one pair"""
    pos = torch.tensor([[0.0, 0.0, 0.0], [40.0, 3.0, -2.0], [-7.0, 55.0, 9.0]])
    _counted_case("tiles 512 / 513 / 1", pos, {0: 512, 1: 513, 2: 1}, 80)


def test_f_empty_fields_across_the_rounds_of_the_offsets_scan():
    """130 fields of which only 63, 64 and 129 receive points (the other 127 centres are far from every point): empty fields
    either side of the 64-lane rounds of the segment / tile scans"""
    pos = torch.zeros(130, 3)
    pos[:, 0] = torch.arange(130, dtype=torch.float32) * 10.0
    pos[:, 1] = (torch.arange(130) % 7).float() * 4.0
    _counted_case("fields 63 / 64 / 129 of 130", pos, {63: 300, 64: 17, 129: 130}, 81)


@pytest.mark.parametrize("P", [8191, 8192, 8193, 1])
def test_f_scatter_workgroup_edges_and_one_point(P):
    """P K = 8 191, 8 192, 8 193 pairs at K = 1 (a scatter workgroup ranks 32 x 256 pairs) and a single point"""
    pos = Q.layout_case("cover300")[0]
    pts = Q.points_in_box(pos, P, 90 + P) if P > 1 else (pos[17] + torch.tensor([0.25, -0.125, 0.3])).reshape(1, 3)
    codes = Q.int_codes(300, 90)
    exp = Q.expect(Q.brute_force(pts, pos), 1)
    if P == 1:
        assert bool(exp.inside.all()) and not bool(exp.undecided.any())
    out = evaluate(pos, pts, codes, 1)
    assert out.shape == (P, 4)
    Q.check_set(f"P K = {P}", out, exp, codes, pts, cap=0.0 if P == 1 else 0.01)


@pytest.mark.parametrize("K_", [1, 3])
def test_f_field_index_a_shuffled_proper_subset_of_the_rows(K_):
    """seven fields whose weights are rows (9, 0, 4, 11, 2, 7, 5) of twelve: field f must answer with code[rows[f]]"""
    rows = torch.tensor([9, 0, 4, 11, 2, 7, 5])
    pos = Q.cover_lattice(7, seed=95, dims=(2, 2, 2))
    pts = Q.points_in_box(pos, 1000, 95, reach=1.0)
    codes = Q.int_codes(12, 95)
    exp = Q.expect(Q.brute_force(pts, pos), K_)
    out = ops.field_eval_knn(fcfg(), probe(12, codes), pts.to(DEV), pos.to(DEV), Q.unit_quats(7).to(DEV), K_, 0.0, Q.OUTSIDE,
                             rows.to(DEV)).cpu()
    Q.check_set("field_index subset", out, exp, codes[rows], pts, NF=7)
    assert not bool(Q.set_mode_accepts(out, exp, codes[:7])[exp.inside].all())          # (the identity map would be another answer)


@pytest.mark.parametrize("K_", [1, 3])
def test_f_lattice_entry_against_the_reference(K_):
    """one 17 x 13 x 11 lattice call of ops.grid_eval_knn per channel on the 2 049-field map: the volume's channel c holds
    channel c of the sums over the brute-force sets"""
    pos = Q.layout_case("near_kernels_2049")[0]
    NF = pos.shape[0]
    codes = Q.int_codes(NF, len("near_kernels_2049"))
    axes = [torch.linspace(-1.3, 9.1, 17), torch.linspace(-0.7, 6.3, 13) + 0.013, torch.linspace(2.2, 16.4, 11) - 0.007]
    pts = torch.cartesian_prod(*axes).contiguous()
    exp = Q.expect(Q.brute_force(pts, pos), K_)
    assert 0.25 < exp.share() < 0.95
    params = probe(NF, codes, "near_kernels_2049")
    quat = Q.unit_quats(NF).to(DEV)
    vols = [ops.grid_eval_knn(fcfg(), params, *(a.to(DEV) for a in axes), pos.to(DEV), quat, K_, 0.0, Q.OUTSIDE, channel=c).cpu()
            for c in range(4)]
    assert all(v.shape == (17, 13, 11) for v in vols)
    out = torch.stack([v.reshape(-1) for v in vols], -1)
    Q.check_set("lattice entry 17x13x11", out, exp, codes, pts)
    assert torch.equal(out, evaluate(pos, pts, codes, K_, key="near_kernels_2049"))      # and the point entry's bits, as documented


# ------------------------------------------------------------------------------------------------ G: points documented as outside
@pytest.mark.parametrize("K_", [1, 4, 16])
def test_g_non_finite_and_huge_points_are_outside_and_disturb_nothing(K_):
    """NaN, +-inf and +-1e30 coordinates (one coordinate or all three) mixed into a normal batch: those points return
    outside_value, every other point returns what it returns without them.  (Only the points: centres are finite.)"""
    pos, pts, ref = Q.layout_case("cover300")
    pts = pts[:2000].clone()
    codes = Q.int_codes(300, 99)
    clean = evaluate(pos, pts, codes, K_)
    exp = Q.expect((ref[0][:2000], ref[1][:2000]), K_)
    Q.check_set("batch without bad points", clean, exp, codes, pts)
    bad_vals = [float("nan"), float("inf"), float("-inf"), 1e30, -1e30]
    g = torch.Generator().manual_seed(99)
    rows = torch.randperm(2000, generator=g)[:20 * len(bad_vals)]
    assert int(exp.inside[rows].sum()) > 20                  # points that were inside a field become bad ones, too
    dirty = pts.clone()
    for i, r in enumerate(rows.tolist()):
        v = bad_vals[i % len(bad_vals)]
        which = (i // len(bad_vals)) % 4
        if which == 3:
            dirty[r] = v
        else:
            dirty[r, which] = v
    out = evaluate(pos, dirty, codes, K_)
    is_bad = torch.zeros(2000, dtype=torch.bool)
    is_bad[rows] = True
    assert bool((out[is_bad] == Q.OUTSIDE).all())
    assert torch.equal(out[~is_bad], clean[~is_bad])

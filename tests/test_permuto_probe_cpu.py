"""The conditions tests/test_gpu_permuto_exact.py rests on, shown for the reference alone (no GPU, no library): the float32
simplex search gives proper barycentric weights on every probe input, the tie set holds exact ties, the run-head groups have
the run heads they claim, `uniform` has no run, and the expected table gradient equals a brute-force loop."""
import numpy as np
import pytest
import torch

import _permuto_probe as PP

T = 4096
FS = PP.spec()
SHIFT = PP.shifts(16, seed=11)


def _builders():
    return {
        "uniform": PP.uniform(513, SHIFT, FS, T, seed=1),
        "ties": PP.ties(SHIFT, FS, seed=2),
        "runs": PP.runs(PP.run_lengths(1024), seed=3),
        "one_run": PP.runs([1024], seed=4),
        "heads40": PP.heads(40, 2, SHIFT, FS, T, seed=5),
        "alternating": PP.alternating(256, SHIFT, FS, T, seed=6),
        "ray_like": PP.ray_like(8, 64, seed=7),
    }


BUILT = _builders()


@pytest.mark.parametrize("name", sorted(BUILT))
def test_reference_weights_are_barycentric_and_indices_in_range(name):
    x = BUILT[name]
    assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 3
    idx, w = PP.simplex32(x, SHIFT, FS, T)
    assert w.dtype == np.float32 and idx.shape == (x.shape[0], 16, 4)
    assert (w >= 0).all(), float(w.min())
    assert float(np.abs(w.astype(np.float64).sum(-1) - 1.0).max()) <= 4 * PP.EPS
    assert idx.min() >= 0 and idx.max() < T


def test_tie_set_holds_exact_ties_at_every_level():
    x = BUILT["ties"]
    el, diff = PP.residuals(x, SHIFT, FS)
    for l in range(16):
        d = np.sort(diff[:, l, :], -1)
        two_equal = (d[:, 1:] == d[:, :-1]).any(-1)
        assert int(two_equal.sum()) > 0, l
        # -shift_l itself: every elevated coordinate exactly zero, all four residuals equal
        assert (el[l, l, :] == 0).all() and (diff[l, l, :] == 0).all()
    # ties of the nearest remainder-0 point (el / 4 exactly halfway, round-to-nearest-even goes up): built level by level
    hx, hl = PP.half_ties(SHIFT, FS, seed=3)
    elh, _ = PP.residuals(hx, SHIFT, FS)
    v = elh[np.arange(len(hl)), hl, 3] * np.float32(0.25)
    assert len(hl) > 0 and ((np.rint(v) - v) == 0.5).all()
    assert len(set(hl.tolist())) >= 12, sorted(set(hl.tolist()))        # (the search is not guaranteed to hit at every level)
    # lattice coordinates of several 1e5 are in the set
    assert float(np.abs(el).max()) > 3e5


@pytest.mark.parametrize("h", [1, 39, 40, 41, 64])
def test_head_groups_have_exactly_h_run_heads(h):
    x = PP.heads(h, 3, SHIFT, FS, T, seed=20 + h)
    assert x.shape == (192, 3)
    idx, _ = PP.simplex32(x, SHIFT, FS, T)
    assert (PP.run_heads(idx[:, 0, :]) == h).all()
    for l in range(16):                       # identical points stay together, different ones stay apart, at every level
        assert (PP.run_heads(idx[:, l, :]) == h).all(), l


def test_uniform_and_its_permutation_have_no_run_at_any_level():
    x = PP.uniform(4096, SHIFT, FS, T, seed=8)
    assert not PP.same_as_previous(PP.simplex32(x, SHIFT, FS, T)[0]).any()
    perm = PP.permutation_without_runs(x, SHIFT, FS, T, seed=9)
    assert sorted(perm.tolist()) == list(range(4096)) and not torch.equal(perm, torch.arange(4096))
    assert not PP.same_as_previous(PP.simplex32(x[perm], SHIFT, FS, T)[0]).any()
    # and with the smallest table, where every entry collides
    x16 = PP.uniform(513, SHIFT, FS, 16, seed=8)
    assert not PP.same_as_previous(PP.simplex32(x16, SHIFT, FS, 16)[0]).any()


def test_run_inputs_have_the_runs_they_claim():
    ls = PP.run_lengths(1024)
    ends = np.cumsum(ls)
    starts = ends - np.asarray(ls)
    assert ls[:10] == list(range(1, 11))
    assert any(s <= 63 and e > 64 for s, e in zip(starts, ends))            # a block over lanes 63|64
    assert any(s <= 511 and e > 512 for s, e in zip(starts, ends))          # a block over threads 511|512
    assert max(ls) > 64                                                      # a block longer than a wave
    idx, _ = PP.simplex32(BUILT["runs"], SHIFT, FS, T)
    same = PP.same_as_previous(idx)
    inside = np.ones(1024, dtype=bool)
    inside[starts] = False
    assert same[inside].all()                                                # identical points: merged at every level
    assert PP.same_as_previous(PP.simplex32(BUILT["one_run"], SHIFT, FS, T)[0])[1:].all()
    # alternating: no run, eight entries per level
    ia, _ = PP.simplex32(BUILT["alternating"], SHIFT, FS, T)
    assert not PP.same_as_previous(ia).any()
    assert all(len(np.unique(ia[:, l, :])) <= 8 for l in range(16))
    # ray-like: runs at the coarsest level, none at the finest
    ir, _ = PP.simplex32(BUILT["ray_like"], SHIFT, FS, T)
    sr = PP.same_as_previous(ir)
    assert sr[:, 0].mean() > 0.5 and not sr[:, 15].any()


def test_expected_table_grad_equals_brute_force():
    P, L, Ts = 50, 16, 16                       # 16 entries: every entry collects many terms
    x = PP.uniform(P, SHIFT, FS, Ts, seed=12)
    idx, w = PP.simplex32(x, SHIFT, FS, Ts)
    d = torch.randn(P, 2 * L, generator=torch.Generator().manual_seed(13)).numpy()
    G, A, n = PP.expected_table_grad(idx, w, d, Ts)
    G2, A2, n2 = np.zeros((L, Ts, 2)), np.zeros((L, Ts, 2)), np.zeros((L, Ts), dtype=np.int64)
    for p in range(P):
        for l in range(L):
            for r in range(4):
                i = idx[p, l, r]
                n2[l, i] += 1
                for c in range(2):
                    v = np.float32(d[p, 2 * l + c]) * np.float32(w[p, l, r])
                    assert type(v) is np.float32
                    G2[l, i, c] += float(v)
                    A2[l, i, c] += abs(float(v))
    assert (n == n2).all() and n.sum() == P * L * 4
    np.testing.assert_allclose(G, G2, rtol=0, atol=1e-13)
    np.testing.assert_allclose(A, A2, rtol=1e-14, atol=0)


def test_expected_encoding_equals_brute_force():
    P, L = 20, 16
    x = PP.uniform(P, SHIFT, FS, T, seed=14)
    idx, w = PP.simplex32(x, SHIFT, FS, T)
    tab = (0.5 + 0.5 * torch.rand(L, T, 2, generator=torch.Generator().manual_seed(15))).numpy()
    E, M = PP.expected_encoding(idx, w, tab)
    for p in range(P):
        for l in range(L):
            for c in range(2):
                e = sum(float(w[p, l, r]) * float(tab[l, idx[p, l, r], c]) for r in range(4))
                assert abs(E[p, 2 * l + c] - e) < 1e-15
            assert M[p, l] == max(abs(float(tab[l, idx[p, l, r], c])) for r in range(4) for c in range(2))

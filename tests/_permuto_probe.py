"""Host-side probe of the permutohedral hash encoding: exact-arithmetic expectations and input builders.

The reference of tests/test_gpu_permuto_exact.py is `oracle.ngm_oracle.permuto_simplex` run in FLOAT32 on the very float32
field-frame points handed to the kernels: same inputs, same roundings, so the hashed indices are equal and the barycentric
weights agree to an ulp (`bw[0]` is associated differently in the kernel).  What remains between a kernel and the
expectations below is the kernel's own accumulation, which the derived bars of that file bound.  Everything here is numpy /
CPU torch: no library, no GPU.  One field at a time: x (P,3), shift (L,3), table (L,T,2), d_enc (P,2L).
"""
import numpy as np
import torch

from oracle import ngm_oracle as O

EPS = 2.0 ** -24          # unit roundoff of float32


def spec(nr_levels=16, log2_hashmap_size=12):
    return O.FieldSpec(encoding="permuto", num_layers=1, nr_levels=nr_levels, log2_hashmap_size=log2_hashmap_size,
                       coarsest_scale=1.0, finest_scale=1e-4)


def shifts(L, seed):
    """(L,3) float32 per-level shifts, drawn like the encoding's own (N(0, 10^2))"""
    return (10.0 * torch.randn(L, 3, generator=torch.Generator().manual_seed(seed))).float()


def simplex32(x, shift, fs, T):
    """the reference: float32 simplex search of one field -> idx (P,L,4) int64, w32 (P,L,4) float32, numpy"""
    assert x.dtype == torch.float32 and shift.dtype == torch.float32
    idx, w = O.permuto_simplex(x[None], shift[None], fs, T)
    assert w.dtype == torch.float32
    return idx[0].numpy(), w[0].numpy()


def residuals(x, shift, fs):
    """float32 elevated coordinates and residuals of the reference's first steps -> el (P,L,4), diff (P,L,4), numpy"""
    scale = O.permuto_scale_factors(fs, torch.float32)
    cf = (x[:, None, :] + shift[None]) * scale[None]
    el = x.new_zeros(x.shape[0], shift.shape[0], 4)
    sm = x.new_zeros(x.shape[0], shift.shape[0])
    for i in range(3, 0, -1):
        el[..., i] = sm - i * cf[..., i - 1]
        sm = sm + cf[..., i - 1]
    el[..., 0] = sm
    v = el * 0.25
    up, down = torch.ceil(v) * 4, torch.floor(v) * 4
    rem0 = torch.where(up - el < el - down, up, down)
    return el.numpy(), (el - rem0).numpy()


# ------------------------------------------------------------------------------------------------ expectations
def expected_encoding(idx, w32, table):
    """E_ref[p, 2l+c] = sum_r w32[p,l,r] table[l, idx[p,l,r], c] in float64 (P,2L); M[p,l] = max_r |table[l, idx_r, :]| (P,L)"""
    P, L, _ = idx.shape
    tab = np.asarray(table, dtype=np.float64)
    g = tab[np.arange(L)[None, :, None], idx]                          # (P,L,4,2)
    E = (g * w32.astype(np.float64)[..., None]).sum(2)
    return E.reshape(P, 2 * L), np.abs(g).max((2, 3))


def expected_table_grad(idx, w32, d_enc, T):
    """The table gradient of d_enc (P,2L) float32 with the kernel's single float32 rounding of every term,
    v = float32(d * w32), summed in float64: G_ref (L,T,2) = sum v over the terms whose entry is i, A (L,T,2) = sum |v|,
    n (L,T) = number of terms."""
    P, L, _ = idx.shape
    d = np.asarray(d_enc, dtype=np.float32).reshape(P, L, 1, 2)
    v = (d * w32.astype(np.float32)[..., None]).astype(np.float32)     # (P,L,4,2): one fp32 product each
    assert v.dtype == np.float32
    G, A, n = np.zeros((L, T, 2)), np.zeros((L, T, 2)), np.zeros((L, T), dtype=np.int64)
    for l in range(L):
        i = idx[:, l, :].reshape(-1)
        n[l] = np.bincount(i, minlength=T)
        for c in range(2):
            vv = v[:, l, :, c].reshape(-1).astype(np.float64)
            G[l, :, c] = np.bincount(i, weights=vv, minlength=T)
            A[l, :, c] = np.bincount(i, weights=np.abs(vv), minlength=T)
    return G, A, n


# ------------------------------------------------------------------------------------------------ run structure
def same_as_previous(idx):
    """(P,L) bool: all four vertices of point p at level l equal those of point p - 1 (False for p = 0)"""
    s = np.zeros(idx.shape[:2], dtype=bool)
    s[1:] = (idx[1:] == idx[:-1]).all(-1)
    return s


def run_heads(idx_level, group=64):
    """run heads per group of 64 consecutive points by the kernel's rule: lane 0 always starts a run, any other lane starts
    one unless all four vertices equal the previous lane's.  idx_level (P,4), P a multiple of `group` -> (P / group,) int"""
    P = idx_level.shape[0]
    assert P % group == 0
    head = np.ones(P, dtype=bool)
    head[1:] = ~(idx_level[1:] == idx_level[:-1]).all(-1)
    head[::group] = True
    return head.reshape(-1, group).sum(-1)


# ------------------------------------------------------------------------------------------------ input builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def uniform(P, shift, fs, T, seed=0, lo=-1.0, hi=1.0):
    """P points uniform on [lo, hi]^3, none with the four vertices of its predecessor at any level: no run anywhere"""
    g = _gen(seed)
    x = lo + (hi - lo) * torch.rand(P, 3, generator=g)
    for _ in range(200):
        bad = same_as_previous(simplex32(x, shift, fs, T)[0]).any(-1)
        if not bad.any():
            return x
        x[torch.from_numpy(bad)] = lo + (hi - lo) * torch.rand(int(bad.sum()), 3, generator=g)
    raise AssertionError("uniform: could not separate consecutive points")


def permutation_without_runs(x, shift, fs, T, seed=0):
    """a fixed permutation of the points of `uniform` that has no run either -> int64 (P,)"""
    g = _gen(seed)
    P = x.shape[0]
    perm = torch.randperm(P, generator=g)
    for _ in range(200):
        s = same_as_previous(simplex32(x[perm], shift, fs, T)[0]).any(-1)
        if not s.any():
            return perm
        for p in np.nonzero(s)[0]:
            q = int(torch.randint(0, P, (1,), generator=g))
            perm[[int(p), q]] = perm[[q, int(p)]]
    raise AssertionError("permutation_without_runs: did not converge")


def half_ties(shift, fs, seed=0, per_level=4):
    """Points whose elevated coordinate el_3 / 4 is exactly k + 1/2 with round-to-nearest-even going UP (k odd): the nearest
    remainder-0 point is a tie that the restatement gives to the lower candidate.  Found by scanning consecutive float32 z
    around the solutions of -3 (z + shift_z) scale_z = 4 k + 2, |z| <= 64.  -> (n,3) float32 and the level each was built for"""
    scale = O.permuto_scale_factors(fs, torch.float32).numpy()
    sh = shift.numpy()
    g = _gen(seed)
    pts, lv = [], []
    for l in range(sh.shape[0]):
        s, sc = np.float32(sh[l, 2]), np.float32(scale[l, 2])
        kmax = max(1.0, (3.0 * 60.0 * float(sc) - 2.0) / 4.0)
        ks = np.unique(np.round(np.geomspace(1.0, kmax, 48)).astype(np.int64) | 1)
        ks = np.concatenate([ks, -ks])
        zc = ((-(4.0 * ks + 2.0) / 3.0) / float(sc) - float(s)).astype(np.float32)
        z = (zc.view(np.int32)[:, None] + np.arange(-1024, 1025, dtype=np.int32)[None]).view(np.float32).reshape(-1)
        z = z[np.isfinite(z) & (np.abs(z) <= 64.0)]
        v = (np.float32(0.0) - np.float32(3.0) * ((z + s) * sc)) * np.float32(0.25)
        assert v.dtype == np.float32
        hit = z[(np.rint(v) - v) == np.float32(0.5)]
        if hit.size > per_level:
            hit = hit[np.linspace(0, hit.size - 1, per_level).astype(np.int64)]
        for zz in hit:
            xy = 2.0 * torch.rand(2, generator=g) - 1.0
            pts.append([float(xy[0]), float(xy[1]), float(zz)])
            lv.append(l)
    return torch.tensor(pts, dtype=torch.float32).reshape(-1, 3), np.asarray(lv, dtype=np.int64)


def ties(shift, fs, seed=0):
    """The edges of the simplex search, float32 (P,3):
      * -shift_l for every level: every elevated coordinate is exactly 0 there, a four-way rank tie;
      * one axis at -shift_l (x: el_0 == el_1, a two-way tie), the others random;
      * half_ties: exact ties of the nearest remainder-0 point;
      * dyadic points (i, j, k) / 64;
      * |x| up to 64 (lattice coordinates up to ~6e5 at the finest level);
      * the negative octant."""
    g = _gen(seed)
    L = shift.shape[0]
    parts = [-shift]
    for a in range(3):
        p = 2.0 * torch.rand(L, 3, generator=g) - 1.0
        p[:, a] = -shift[:, a]
        parts.append(p)
    parts.append(half_ties(shift, fs, seed + 1)[0])
    k = torch.arange(-6, 6, dtype=torch.float32) / 64.0
    parts.append(torch.stack(torch.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3))
    parts.append(128.0 * torch.rand(512, 3, generator=g) - 64.0)
    parts.append(-torch.rand(256, 3, generator=g))
    return torch.cat(parts).float().contiguous()


def runs(lengths, seed=0):
    """blocks of identical points, block b of lengths[b] points -> (sum(lengths), 3) float32"""
    g = _gen(seed)
    base = 2.0 * torch.rand(len(lengths), 3, generator=g) - 1.0
    return base.repeat_interleave(torch.tensor(list(lengths)), 0).contiguous()


def run_lengths(P=1024):
    """Block lengths for `runs`, sum P: 1, 2, 3, ..., 10 (points 0..54), a block over lanes 63|64 (55..74), blocks of growing
    length up to point 499, a block over threads 511|512 (500..529), a block longer than a wave (530..649), then 1, 2, 3, ...
    to the end"""
    ls = list(range(1, 11)) + [20]
    n, k = 75, 11
    while n + k <= 500:
        ls.append(k); n += k; k += 3
    ls.append(500 - n)
    ls += [30, 120]
    n, k = 650, 1
    while n + k <= P:
        ls.append(k); n += k; k += 1
    if n < P:
        ls.append(P - n)
    ls = [v for v in ls if v > 0]
    assert sum(ls) == P
    return ls


def heads(h, groups, shift, fs, T, seed=0):
    """`groups` groups of 64 points with exactly h run heads each, at every level: h points of `uniform` (consecutive ones in
    different simplices at every level), the first 64 % h of them repeated 64 // h + 1 times, the others 64 // h times"""
    base = uniform(groups * h, shift, fs, T, seed)
    rep = torch.tensor(([64 // h + 1] * (64 % h) + [64 // h] * (h - 64 % h)) * groups)
    return base.repeat_interleave(rep, 0).contiguous()


def alternating(P, shift, fs, T, seed=0):
    """A, B, A, B, ...: no two consecutive points share a simplex, every point falls on the same eight entries per level"""
    ab = uniform(2, shift, fs, T, seed)
    return ab.repeat((P + 1) // 2, 1)[:P].contiguous()


def ray_like(R, S, seed=0, length=0.5):
    """R rays o + t d of S samples, t in [0, length]: consecutive samples share a simplex at the coarse levels and not at
    the fine ones -> (R * S, 3)"""
    g = _gen(seed)
    o = 1.6 * torch.rand(R, 1, 3, generator=g) - 0.8
    d = torch.nn.functional.normalize(torch.randn(R, 1, 3, generator=g), dim=-1)
    t = torch.linspace(0.0, length, S)[None, :, None]
    return (o + t * d).reshape(R * S, 3).float().contiguous()

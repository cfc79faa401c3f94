"""Generate g29_mesh_cull.npz from the REAL reference (build container only).

    python tests/golden/make_golden_mesh_cull.py

mesh_culling._cull_from_one_pose and _cull_by_bounds (mesh_culling.py:123-190), called as _apply_culling_strategy calls them
(float32 points and pose, float64 depth map, eps 0.03), on a small scene.  The function sends its projection matrix `.to("cuda")`:
there is no GPU in the build container, so Tensor.to is asked for the CPU instead during the calls (as _ref_import.build_map
redirects torch.empty).  pyrender is mocked, so the depth maps the reference is handed come from the host mirror
(tests/_mesh_cull_host.py), rounded to multiples of 2^-9 m and stored as uint16 counts so that eight 160 x 120 maps fit the
fixture's size limit -- a step fifteen times finer than eps; the reference is given exactly the stored values.

Scene: a room of 4 x 3 x 2.4 m in triangles of 10 cm, an inner box as an occluder, a patch outside the room (the annex the
bounds rule removes), a 160 x 120 camera, eight poses: four inside looking around, one 5 cm above the floor (its near plane cuts
the floor), one outside looking away, and two more that play virtual cameras (num_frustum_poses = 6).
Stored: vertices, faces, poses, intrinsics (cx, cy in the 0.5-pixel-centre convention), bounds, the depth maps, the reference's
two masks per pose and its bounds mask (bit-packed).  Data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_import import import_reference  # noqa: E402
import _mesh_cull_host as CH  # noqa: E402

_, _, ref_camera, _, _, _ = import_reference()
from neural_graph_mapping import mesh_culling as mc  # noqa: E402

ROOM = (4.0, 3.0, 2.4)
BOX = ((1.6, 1.2, 0.3), (2.4, 1.8, 1.3))
STEP = 0.1
W, H, FX, FY, CX, CY = 160, 120, 140.0, 138.0, 80.3, 60.2            # cx, cy: 0.5-pixel-centre convention
EPS, NUM_FRUSTUM_POSES, DEPTH_STEP = 0.03, 6, 2.0 ** -9
PAIR_CAP, PIXEL_CAP = 0.01, 0.02
# A face hangs on 3 vertices x 8 poses = 24 pairs: at the pair cap of 1 % up to a quarter of the faces touch a doubtful pair.
# Such a pair decides the face only when no sure pair keeps it; with about half of the in-frustum vertices hidden from a pose
# and several poses per face that is well below one face in five of those: 5 %.  The test that matters is the other one --
# outside the doubtful faces the two meshes are identical; this cap only keeps that comparison from becoming empty.
FACE_CAP = 0.05


def grid_patch(origin, du, dv, nu, nv):
    """(nu x nv) squares spanned by du, dv from origin, two triangles each"""
    o, du, dv = (np.asarray(a, np.float64) for a in (origin, du, dv))
    i, j = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing="ij")
    v = o + i[..., None] * du + j[..., None] * dv
    idx = (i * (nv + 1) + j)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v.reshape(-1, 3), f


def box_patches(lo, hi):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    n = np.rint((hi - lo) / STEP).astype(int)
    e = np.eye(3) * STEP
    out = []
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for side in (lo, hi):
            o = lo.copy()
            o[axis] = side[axis]
            out.append(grid_patch(o, e[a], e[b], n[a], n[b]))
    return out


def scene():
    patches = box_patches((0, 0, 0), ROOM) + box_patches(*BOX)
    patches.append(grid_patch((4.6, 1.0, 1.0), (STEP, 0, 0), (0, STEP, 0), 8, 10))          # the annex, outside the room
    verts, faces, off = [], [], 0
    for v, f in patches:
        verts.append(v); faces.append(f + off); off += len(v)
    return np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int64)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """OpenGL camera-to-world: x right, y up, z back"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, up); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, u, -f, eye
    return m


POSES = [((0.5, 0.5, 1.2), (2.0, 1.5, 0.8)), ((3.5, 2.5, 1.4), (2.0, 1.5, 0.8)), ((0.6, 2.4, 1.0), (3.5, 0.5, 1.05)),
         ((2.0, 0.3, 1.6), (2.05, 2.9, 0.2)), ((1.0, 1.45, 0.05), (3.0, 1.5, 0.06)), ((-1.0, 1.5, 1.2), (-5.0, 1.4, 1.25)),
         ((2.0, 2.7, 2.2), (2.0, 1.5, 0.8)), ((3.6, 0.4, 0.4), (2.0, 1.5, 0.8))]
LOOKS_AT_ROOM = [0, 1, 2, 3, 4, 6, 7]


def reference_masks(verts, c2ws, depth):
    cam = ref_camera.Camera(W, H, FX, FY, CX, CY, pixel_center=0.5)
    assert cam.get_pinhole_camera_parameters(0.5)[2:4] == (CX, CY)
    real_to = torch.Tensor.to

    def cpu_to(self, *a, **k):
        a = tuple("cpu" if isinstance(x, str) and x == "cuda" else x for x in a)
        if k.get("device") == "cuda":
            k["device"] = "cpu"
        return real_to(self, *a, **k)
    torch.Tensor.to = cpu_to
    try:
        points = torch.from_numpy(verts.astype(np.float64)).to(device="cuda", dtype=torch.float)      # mesh_culling.py:205
        ins, obs = [], []
        for pose, d in zip(c2ws, depth):
            i, o = mc._cull_from_one_pose(points, torch.from_numpy(pose.astype(np.float64)).to(device="cuda", dtype=torch.float),
                                          cam=cam, rendered_depth=torch.from_numpy(d.astype(np.float64)).to("cuda"),
                                          remove_occlusion=True, eps=EPS)
            assert i.dtype == torch.int32 and o.dtype == torch.int32
            ins.append(i.numpy().astype(bool)); obs.append(o.numpy().astype(bool))
    finally:
        torch.Tensor.to = real_to
    return np.stack(ins), np.stack(obs)


def main():
    verts, faces = scene()
    c2ws = np.stack([look_at(e, t) for e, t in POSES]).astype(np.float32)
    cam = CH.make_cam(W, H, FX, FY, CX, CY)
    bounds = np.array([(0, 0, 0), ROOM], np.float32)
    stats = {}
    depth64, pdoubt = CH.render_depth(verts, faces, c2ws, cam, stats=stats)
    counts = np.rint(depth64 / DEPTH_STEP)
    assert counts.max() < 65536
    counts = counts.astype(np.uint16)
    depth = (counts.astype(np.float64) * DEPTH_STEP).astype(np.float32)                      # exact in float32
    covered = depth64 > 0
    print(f"covered pixels {covered.sum()}, doubtful among them {(pdoubt & covered).sum()} ({(pdoubt & covered).sum() / covered.sum():.4%})")
    assert (pdoubt & covered).sum() <= PIXEL_CAP * covered.sum()
    assert not covered[5].any() and all(covered[p].any() for p in LOOKS_AT_ROOM)

    ref_in, ref_obs = reference_masks(verts, c2ws, depth)
    ins, seen, db = CH.visibility(verts, c2ws, cam, depth, EPS, pdoubt)
    sure = ~db
    print(f"pairs {db.size}, doubtful {db.sum()} ({db.mean():.4%}); disagreements outside them: "
          f"in_frustum {(ins != ref_in)[sure].sum()}, observed {(seen != ref_obs)[sure].sum()}")
    assert ((ins == ref_in) | db).all() and ((seen == ref_obs) | db).all()
    assert db.mean() <= PAIR_CAP
    for p in LOOKS_AT_ROOM:
        assert 0 < ref_in[p].sum() < ref_in.shape[1] and 0 < ref_obs[p].sum() < ref_obs.shape[1], p
    assert not ref_in[5].any()
    hidden = (ref_in & ~ref_obs)[:4].sum() / ref_in[:4].sum()
    print(f"share of in-frustum vertices hidden (poses 0-3): {hidden:.3f}")
    assert hidden >= 0.03

    ref_bounds = mc._cull_by_bounds(verts.astype(np.float64), bounds)
    assert np.array_equal(CH.cull_by_bounds(verts, bounds), ref_bounds) and 0 < ref_bounds.sum() < len(verts)

    for method in ("frustum", "occlusion", "virt_cams"):
        for b in (None, bounds):
            r = CH.cull(verts, faces, c2ws, cam, method, bounds=b, num_frustum_poses=NUM_FRUSTUM_POSES if method == "virt_cams" else None)
            share = r["face_doubt"].sum() / max(r["start"].sum(), 1)
            print(f"cull {method:9s} bounds={'yes' if b is not None else 'no '}: {r['keep'].sum()} of {len(faces)} faces kept, "
                  f"doubtful {share:.4%}")
            assert share <= FACE_CAP and 0 < r["keep"].sum() < len(faces)

    out = dict(verts=verts, faces=faces.astype(np.int32), c2ws=c2ws, intrinsics=np.array([W, H, FX, FY, CX, CY], np.float64),
               bounds=bounds, depth_counts=counts, depth_step=np.float64(DEPTH_STEP), eps=np.float64(EPS),
               num_frustum_poses=np.int64(NUM_FRUSTUM_POSES), ref_in_frustum=np.packbits(ref_in, axis=1),
               ref_observed=np.packbits(ref_obs, axis=1), ref_bounds=np.packbits(ref_bounds))
    path = os.path.join(HERE, "g29_mesh_cull.npz")
    np.savez_compressed(path, **out)
    print(f"g29_mesh_cull: {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < 200 * 1000


if __name__ == "__main__":
    main()

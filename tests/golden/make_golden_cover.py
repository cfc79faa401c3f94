"""Generate g30_cover_depth.npz from the REAL reference (build container only).

    python tests/golden/make_golden_cover.py

NeuralGraphMap._extend_global_map_dict (rm.py:265-345) on the CPU, twice, on 48 x 64 depth images of a box room
(tests/_cover_host.box_scene): first with active_map_dict=None, then from a nearby second pose with the first call's fields active.
pytorch3d's ball_query is not installed: its K = 1 form is restated here from its public definition (index of a point with
d^2 < r^2, else -1).  The shift of each call is recovered by re-seeding torch before the call and repeating the draw.  The
fp64 mirror must find no ambiguous pixel or centre in either call, and the second call must need the occupied filter;
otherwise the next seed is tried.  Data only.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_import import build_map, import_reference, make_config  # noqa: E402
import _cover_host as CH  # noqa: E402

rm, models, camera, pe, losses, utils = import_reference()
H, W, RADIUS = 48, 64, 1.0


def ball_query(p1, p2, K=1, radius=0.2, return_nn=False, **kw):
    """(1, N, 3) query points, (1, M, 3) points -> idx (1, N, 1): a point of p2 with squared distance < radius^2, else -1"""
    assert K == 1 and not return_nn
    d = p1[0, :, None, :] - p2[0, None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    hit = d2 < radius * radius
    idx = torch.where(hit.any(-1), hit.float().argmax(-1), torch.full((p1.shape[1],), -1))
    return None, idx[None, :, None], None


def run(ngm, depth, frame_id, c2w, cam, active, seed):
    """one call of the reference; its shift is the first draw after the seed, repeated here (rm.py:299-300)"""
    torch.manual_seed(seed)
    shift = torch.empty((3,)).uniform_(0.0, 2 * ngm._field_radius / math.sqrt(3))
    torch.manual_seed(seed)
    ngm._extend_global_map_dict(torch.from_numpy(depth), frame_id, torch.from_numpy(c2w), cam, active)
    return shift.numpy()


def attempt(seed):
    rm.ball_query = ball_query
    ngm = build_map(rm, make_config(field_radius=RADIUS), 0, torch.zeros(0, 3), torch.zeros(0, 4))
    ngm._optim_state = None
    ngm._bb_min, ngm._bb_max = torch.full((3,), torch.inf), torch.full((3,), -torch.inf)
    depth0, c2w0, K = CH.box_scene(seed, H, W)
    depth1, c2w1, _ = CH.box_scene(seed, H, W, nudge=1)
    cam = camera.Camera(width=W, height=H, fx=K[0], fy=K[1], cx=K[2], cy=K[3], pixel_center=0.0)
    shift0 = run(ngm, depth0, 3, c2w0, cam, None, 7 * seed + 1)
    n0 = ngm._global_map_dict["num"]
    pos0 = ngm._global_map_dict["positions"][:n0].clone()
    shift1 = run(ngm, depth1, 8, c2w1, cam, {"positions": pos0}, 7 * seed + 2)
    n1 = ngm._global_map_dict["num"]
    md = ngm._global_map_dict
    c0 = CH.classify(depth0, c2w0, K, shift0, RADIUS)
    c1 = CH.classify(depth1, c2w1, K, shift1, RADIUS, pos0.numpy())
    if c0["ambiguous_pixels"] or c1["ambiguous_pixels"] or c1["ambiguous_centres"]:
        return "an ambiguous pixel"
    assert not c0["optional"] and not c1["optional"]
    # the second call must need the occupied filter: an active centre's cell that still holds uncovered points
    if len(CH.cover_fp32(depth1, c2w1, K, shift1, RADIUS, pos0.numpy(), fault="no_occupied_filter")[0]) == n1 - n0:
        return "the occupied filter drops nothing"
    return dict(depth0=depth0, c2w0=c2w0, depth1=depth1, c2w1=c2w1, intrinsics=np.array(K, np.float64), radius=np.float64(RADIUS),
                shift0=shift0, shift1=shift1, num0=np.int64(n0), num1=np.int64(n1), positions=md["positions"][:n1].numpy(),
                orientations=md["orientations"][:n1].numpy(), kf_ids=md["kf_ids"][:n1].numpy(),
                kf2fields_3=np.array(sorted(ngm._kf2fields[3]), np.int64), kf2fields_8=np.array(sorted(ngm._kf2fields[8]), np.int64),
                seed=np.int64(seed))


def main():
    for seed in range(50):
        out = attempt(seed)
        if isinstance(out, dict):
            break
        print(f"seed {seed}: {out}, next")
    else:
        raise SystemExit("no seed without an ambiguous pixel")
    # the mirror's float32 restatement must reproduce the reference before anything is stored
    p0, k0 = CH.cover_fp32(out["depth0"], out["c2w0"], tuple(out["intrinsics"]), out["shift0"], RADIUS)
    p1, k1 = CH.cover_fp32(out["depth1"], out["c2w1"], tuple(out["intrinsics"]), out["shift1"], RADIUS, out["positions"][:int(out["num0"])])
    n0, n1 = int(out["num0"]), int(out["num1"])
    assert p0.tobytes() == out["positions"][:n0].tobytes(), "first call: restatement and reference differ"
    assert p1.tobytes() == out["positions"][n0:n1].tobytes(), "second call: restatement and reference differ"
    assert n0 > 0 and n1 > n0 and k1[2] < k1[3], "the second call must find covered pixels and new cells"
    path = os.path.join(HERE, "g30_cover_depth.npz")
    np.savez_compressed(path, **out)
    print(f"g30_cover_depth: seed {int(out['seed'])}, {n0} + {n1 - n0} fields, {k0[3]} / {k1[3]} valid pixels, {k1[2]} uncovered in the "
          f"second call, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

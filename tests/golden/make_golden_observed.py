"""Generate g26_observed_fields.npz from the REAL reference (build container only).

    python tests/golden/make_golden_observed.py

NeuralGraphMap._get_observed_fields (rm.py:1642-1670) on the procedural RGB-D frame of tests/golden/scene.py (sv_frame,
regenerated from its seed), with torch.multinomial wrapped to record the 500 points it draws (as g16_target_sampler_sv
records its draws).  Stored: the draws as linear pixel indices (multinomial indexes the torch.nonzero list of the depth
image, camera.py:374; pixel = row * W + col of that entry), the field positions, the pose and the observed ids.  The scene
seed is the first one for which every field clears the margin condition of tests/test_live_iteration_cpu.py in float64, so
float32 rounding cannot flip a field.  Data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_import import build_map, import_reference, make_config  # noqa: E402
import scene  # noqa: E402
import _target_live_host as LH  # noqa: E402

rm, models, camera, pe, losses, utils = import_reference()
NF, RADIUS, FRAME_SEED, NUM_POINTS = 70, 0.35, 261, 500


def make_scene(seed):
    gen = torch.Generator().manual_seed(seed)
    c2w = torch.eye(4)
    ang = 0.2 * torch.rand(1, generator=gen).item()
    c2w[0, 0], c2w[0, 2], c2w[2, 0], c2w[2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
    c2w[:3, 3] = torch.tensor([0.3, -0.2, 0.1])
    # camera-frame positions: most inside the frustum at the depth range of the frame, ten behind the camera, ten far
    # outside the points' bounding box
    pts_c = torch.stack((3.0 * torch.rand(NF, generator=gen) - 1.5, 2.0 * torch.rand(NF, generator=gen) - 1.0,
                         -(1.0 + 3.5 * torch.rand(NF, generator=gen))), -1)
    pts_c[:10, 2] = 0.5 + 2.0 * torch.rand(10, generator=gen)
    pts_c[10:20, 0] += 6.0
    return c2w, (pts_c @ c2w[:3, :3].T + c2w[:3, 3]).contiguous()


def main():
    cam = camera.Camera(width=scene.SV_W, height=scene.SV_H, fx=scene.SV_FX, fy=scene.SV_FY, cx=scene.SV_CX, cy=scene.SV_CY,
                        pixel_center=0.0)
    img = scene.sv_frame(FRAME_SEED)
    for seed in range(260, 360):
        c2w, pos = make_scene(seed)
        cfg = make_config(num_samples_coarse=4, num_samples_depth_guided=4)
        cfg["field_radius"] = RADIUS
        ngm = build_map(rm, cfg, NF, pos, torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(NF, 1), seed=seed)
        ngm._camera = cam
        rec, orig = [], torch.multinomial

        def wrapped(*a, **k):
            out = orig(*a, **k)
            rec.append(out)
            return out
        torch.manual_seed(seed + 1)
        torch.multinomial = wrapped
        try:
            ids = ngm._get_observed_fields(img, c2w)
        finally:
            torch.multinomial = orig
        assert len(rec) == 1 and rec[0].shape == (NUM_POINTS,)
        nz = torch.nonzero(img[..., 3])
        pixels = (nz[rec[0], 0] * scene.SV_W + nz[rec[0], 1]).numpy()
        got, m_box, m_seg = LH.observed_from_pixels(img.numpy(), c2w.numpy(), pos.numpy(), RADIUS, pixels, scene.SV_FX, scene.SV_FY,
                                                    scene.SV_CX, scene.SV_CY, dt=np.float64, margins=True)
        assert np.array_equal(got, ids.numpy()), "the restatement disagrees with the reference"
        if m_box >= 1e-3 and m_seg >= 1e-3 and 5 <= len(got) <= NF - 25:
            path = os.path.join(HERE, "g26_observed_fields.npz")
            np.savez_compressed(path, frame_seed=np.int64(FRAME_SEED), scene_seed=np.int64(seed), positions=pos.numpy(),
                                c2w=c2w.numpy(), field_radius=np.float32(RADIUS), num_points=np.int64(NUM_POINTS),
                                d_pixels=pixels.astype(np.int32), o_field_ids=ids.numpy().astype(np.int64))
            print(f"g26_observed_fields: seed {seed}, {len(got)} observed, margins {m_box:.2e} / {m_seg:.2e}, "
                  f"{os.path.getsize(path) / 1024:.1f} KiB")
            return
    raise SystemExit("no scene seed met the margin condition")


if __name__ == "__main__":
    main()

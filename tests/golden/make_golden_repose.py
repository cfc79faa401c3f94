"""Generate g25_repose.npz from the REAL reference (build container only).

    python tests/golden/make_golden_repose.py

NeuralGraphMap._absolute_map_dict_to_relative with the previous keyframe poses, then _relative_map_dict_to_absolute with the
new ones (rm.py:844-885; neither uses `self`): what _update_field_poses (rm.py:937-952) does to the map at a pose-graph
update.  12 fields over 5 keyframes, float32 as the reference runs it.  Among the keyframe poses: a rotation by pi about
each coordinate axis (where a trace-only matrix_to_quaternion loses all accuracy), one keyframe that does not move; among
the fields: one non-unit quaternion.  Stored: the inputs, the relative map in between and the result.  Data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_import import import_reference  # noqa: E402
import _repose_host as RH  # noqa: E402

rm, models, camera, pe, losses, utils = import_reference()
NF, NK, SEED = 12, 5, 25


def main():
    rng = np.random.default_rng(SEED)
    rand_rot = lambda: RH.rot(rng.normal(size=3), rng.uniform(0.2, 2.8))
    # previous poses: general rotations, metre-scale translations; keyframe 3 stands at a rotation by pi about y
    prev = [RH.pose(rand_rot(), rng.uniform(-3, 3, 3)) for _ in range(NK)]
    prev[3] = RH.pose(RH.rot(1, np.pi), rng.uniform(-3, 3, 3))
    # new poses: keyframe 0 turns by pi about x, keyframe 1 lands ON a rotation by pi about z, keyframe 2 gets a small
    # loop-closure correction, keyframe 3 leaves its rotation by pi, keyframe 4 does not move
    new = [RH.pose(RH.rot(0, np.pi) @ prev[0][:3, :3], prev[0][:3, 3] + rng.uniform(-0.5, 0.5, 3)),
           RH.pose(RH.rot(2, np.pi), prev[1][:3, 3] + rng.uniform(-0.5, 0.5, 3)),
           RH.pose(RH.rot(rng.normal(size=3), 0.03) @ prev[2][:3, :3], prev[2][:3, 3] + rng.uniform(-0.05, 0.05, 3)),
           RH.pose(rand_rot(), prev[3][:3, 3] + rng.uniform(-0.5, 0.5, 3)),
           prev[4].copy()]
    prev, new = np.stack(prev).astype(np.float32), np.stack(new).astype(np.float32)
    kf_ids = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 2, 2], np.int64)
    pos = rng.uniform(-4, 4, (NF, 3)).astype(np.float32)
    quat = rng.normal(size=(NF, 4))
    quat /= np.linalg.norm(quat, axis=-1, keepdims=True)
    quat[5] *= 1.7                                            # a non-unit field quaternion: its norm scales the field's frame
    quat = quat.astype(np.float32)
    md = dict(positions=torch.from_numpy(pos), orientations=torch.from_numpy(quat), kf_ids=torch.from_numpy(kf_ids), num=NF,
              training_iterations=torch.zeros(NF, dtype=torch.int64))
    rel = rm.NeuralGraphMap._absolute_map_dict_to_relative(None, md, torch.from_numpy(prev))
    out = rm.NeuralGraphMap._relative_map_dict_to_absolute(None, rel, torch.from_numpy(new))
    assert out["positions"].dtype == torch.float32 and torch.equal(out["kf_ids"], md["kf_ids"])
    # the restatement in float64 must agree before anything is stored
    p64, q64, touched = RH.repose(pos, quat, kf_ids, prev, new, np.float64)
    ep, eq = RH.errors(out["positions"].numpy(), out["orientations"].numpy(), p64, q64)
    assert ep < 1e-4 and eq < 1e-4, (ep, eq)
    assert touched.tolist() == [k != 4 for k in kf_ids]
    path = os.path.join(HERE, "g25_repose.npz")
    np.savez_compressed(path, positions=pos, orientations=quat, kf_ids=kf_ids, prev_kf2ws=prev, new_kf2ws=new,
                        rel_positions=rel["positions"].numpy(), rel_orientations=rel["orientations"].numpy(),
                        out_positions=out["positions"].numpy(), out_orientations=out["orientations"].numpy())
    print(f"g25_repose: {NF} fields / {NK} keyframes, reference vs float64 restatement {ep:.2e} / {eq:.2e}, "
          f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()

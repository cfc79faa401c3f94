"""Generate g28_train_gnll_nll_branch.npz from the REAL reference (build container only).

    python tests/golden/make_golden_nll_branch.py

A training step with `photometric_loss: gaussian_nll` that TAKES the NLL branch of losses.py:30-36 (mean colour NLL <= 2; the
three G20 fixtures all sit on its L1 side).  make_golden._train_case's set-up (2 fields, 24 rays each, 8 + 8 samples,
gaussian_nll for both losses, termination weight 0.5); the reference renders once, the target colours move to
C + 1.5 sqrt(V) z around that prediction (tests/gpu_common.nll_branch_targets: per-element NLL 0.5 (1.5 z)^2 + 0.5 log V), the
target depths likewise (nll_depth_targets: with synth_target's depths the depth NLL carries 99.9 % of every gradient and the
colour term could be wrong unnoticed), and the reference runs again on the same draws: prediction, losses and parameter
gradients are recorded like G20.  Data only.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as MG  # noqa: E402  (imports the reference through _ref_import)
from gpu_common import nll_branch_targets, nll_depth_targets  # noqa: E402

NAME, F, R, N_C, N_G, SEED, SCALE = "g28_train_gnll_nll_branch", 2, 24, 8, 8, 280, 1.5


def main():
    cam = MG.camera.Camera(**MG.NRGBD_CAMERA)
    gen = torch.Generator().manual_seed(SEED)
    pos = 0.5 * torch.randn(F, 3, generator=gen)
    quat = MG.rand_quats(F, gen)
    cfg = MG.make_config(num_samples_coarse=N_C, num_samples_depth_guided=N_G, termination_weight=0.5,
                         photometric_loss="gaussian_nll", depth_loss="gaussian_nll")
    ngm = MG.build_map(MG.rm, cfg, F, pos, quat, seed=SEED)
    ngm._camera = cam
    model = ngm._model
    for k, v in model.all_fields_params.items():
        if v.dim() > 1:
            v.add_(0.05 * torch.randn(v.shape, generator=gen))
    model.all_fields_params["_linears.2.weight"].mul_(2.0)
    t = MG.synth_target(F, R, cam, pos, gen)
    fids = torch.arange(F)

    def render():
        torch.manual_seed(SEED + 1000)
        return ngm._render_ijs(t["ijs"], t["c2ws"], cam, field_ids=fids, use_vmap=True, near_distances=t["near"],
                               far_distances=t["far"], gt_distances=t["gt"])
    with torch.no_grad():
        p0 = render()
    p0d = dict(rgbds=p0.rgbds, color_vars=p0.color_vars, depth_vars=p0.depth_vars, term_probs=p0.term_probs)
    t = nll_depth_targets(nll_branch_targets(t, p0d, SCALE, gen), p0d, SCALE, gen)
    pred = render()                                        # the same draws: the prediction is the first run's
    assert torch.equal(pred.rgbds.detach(), p0.rgbds)
    u_c, u_g = MG.draw_u(SEED + 1000, F, R, N_C, N_G)
    loss = ngm._compute_losses(MG.make_target(t, fids), pred)
    m = t["depth_mask"] & (pred.term_probs > 0.8)
    e, v = (t["rgbds"][m][:, :3] - pred.rgbds[m][:, :3]).detach(), pred.color_vars[m].detach()
    nll = float((0.5 * e ** 2 / v + torch.log(torch.sqrt(v))).mean())
    assert nll < 1.0 and int(m.sum()) >= 16, (nll, int(m.sum()))
    assert abs(float(loss["photometric_gaussian_nll"].detach()) - nll) < 1e-5       # the NLL value, not the L1 loss
    loss["combined"].backward()
    vp = model.vmap_fields_params
    arrays = {"p::" + k: v for k, v in vp.items()}
    arrays.update({"g::" + k: v.grad for k, v in vp.items() if v.grad is not None})
    arrays.update({"t::" + k: v for k, v in t.items()})
    arrays.update({"loss::" + k: v for k, v in loss.items()})
    MG.save(NAME, pos=pos, quat=quat, u_coarse=u_c, u_guided=u_g, pred_rgbds=pred.rgbds, pred_color_vars=pred.color_vars,
            pred_depth_vars=pred.depth_vars, pred_term_probs=pred.term_probs, pred_freespace=pred.freespace_geometry,
            pred_tsdf=pred.tsdf_residuals, **arrays)
    print(f"{NAME}: {int(m.sum())} selected rays of {F * R}, mean colour NLL {nll:.4f}, "
          f"photometric_gaussian_nll {float(loss['photometric_gaussian_nll'].detach()):.6f}")


if __name__ == "__main__":
    main()

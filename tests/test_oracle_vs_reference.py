"""The oracle against the reference on a seed the other fixtures do not contain (fixture G25, recorded from the real
reference by tests/golden/make_golden.py:g25_oracle_fresh_seed): render, losses and every parameter gradient, held to
the reference at tighter bars than the GPU parity tests hold the kernels to the oracle."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_oracle_matches_the_live_reference_on_a_fresh_seed():
    from oracle import ngm_oracle as O
    z = np.load(os.path.join(GOLD, "g25_oracle_fresh_seed.npz"))
    g = {k: torch.from_numpy(z[k]) for k in z.files}
    t = {k[3:]: v for k, v in g.items() if k.startswith("t::")}
    n_c, n_g = g["u_coarse"].shape[-1], g["u_guided"].shape[-1]
    fs = O.FieldSpec(encoding="fourier", dim_enc=64, num_layers=2)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3)
    camo = O.CameraSpec(640, 480, 554.2562584220408, 554.2562584220408, 319.5, 239.5)
    po = {k[3:]: v.clone().requires_grad_() for k, v in g.items() if k.startswith("p::")}
    op = O.render_ijs(t["ijs"], t["c2ws"], camo, g["pos"], g["quat"], po, fs, rs, t["near"], t["far"], t["gt"],
                      g["u_coarse"], g["u_guided"])
    ol = O.compute_losses(op, t["rgbds"], t["depth_mask"], t["term_mask"], t["term_probs"], rs)
    ol["combined"].backward()
    torch.testing.assert_close(op["rgbds"], g["rgbds"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ol["combined"], g["combined"], rtol=1e-5, atol=1e-7)
    for k, v in po.items():
        ref = g["grad::" + k]
        assert float((v.grad - ref).abs().max() / ref.abs().max().clamp_min(1e-12)) < 1e-4, k

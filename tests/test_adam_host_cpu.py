"""The fp64 Adam reference of tests/_adam_host.py and its bar, checked without a GPU: a plain fp32 evaluation of the update
stays within 1x the bound everywhere, and every one of seven plausible faults breaks the 4x bar the GPU kernels are held to
on a large share of the elements -- the proof that tests/test_gpu_adam.py can fail."""
import numpy as np
import pytest

from _adam_host import BAR, HYPER_CPU, MUTANTS, STEPS, adam_fp32, adam_ref64, draw_inputs, ratios, summarize

N_PER_STEP = 200_000                       # x 5 steps = 10^6 elements per hyper-parameter set
SCALES = (1.0, 1e-4, 1e3, 1e-2, 1e6)       # of |g| and of the moments, one per step (|g| <= 1.5e6: nothing overflows in fp32)


def _chunks(name):
    hp = HYPER_CPU[name]
    for i, (step, scale) in enumerate(zip(STEPS, SCALES)):
        yield hp, step, draw_inputs(N_PER_STEP, seed=1000 * sorted(HYPER_CPU).index(name) + i, scale=scale)


@pytest.mark.parametrize("name", sorted(HYPER_CPU))
def test_fp32_restatement_within_one_bound(name):
    worst = dict(p=0.0, m=0.0, v=0.0)
    for hp, step, (p, g, m, v) in _chunks(name):
        ref, bound = adam_ref64(p, g, m, v, *hp, step)
        got = adam_fp32(p, g, m, v, *hp, step)
        for k, (w, _) in summarize(ratios(got, ref, bound)).items():
            worst[k] = max(worst[k], w)
    print(f"\nadam fp32 restatement [{name}] worst |fp32 - fp64| / bound: " + "  ".join(f"{k}={w:.3f}" for k, w in worst.items()))
    assert all(w <= 1.0 for w in worst.values()), worst


@pytest.mark.parametrize("step", [1, 2, 7, 1000])
def test_reference_is_torch_optim_adam(step):
    """adam_ref64 is one step of torch.optim.Adam (L2-coupled decay) in float64 from the same moments and step count"""
    torch = pytest.importorskip("torch")
    hp = tuple(float(np.float32(x)) for x in HYPER_CPU["far"])
    p, g, m, v = draw_inputs(4096, seed=7 + step)
    q = torch.from_numpy(p.astype(np.float64)).requires_grad_()
    opt = torch.optim.Adam([q], lr=hp[0], betas=(hp[1], hp[2]), eps=hp[3], weight_decay=hp[4])
    opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.astype(np.float64)),
                        exp_avg_sq=torch.from_numpy(v.astype(np.float64)))
    q.grad = torch.from_numpy(g.astype(np.float64))
    opt.step()
    (pn, mn, vn), _ = adam_ref64(p, g, m, v, *hp, step)
    np.testing.assert_allclose(pn, q.detach().numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(mn, opt.state[q]["exp_avg"].numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(vn, opt.state[q]["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_breaks_the_bar(mutant):
    shares = {}
    factor = {}
    for name in sorted(HYPER_CPU):
        bad, n, worst = 0, 0, 0.0
        for hp, step, (p, g, m, v) in _chunks(name):
            ref, bound = adam_ref64(p, g, m, v, *hp, step)
            rs = ratios(adam_fp32(p, g, m, v, *hp, step, mutant=mutant), ref, bound)
            over = np.maximum(np.maximum(rs[0], rs[1]), rs[2])
            bad += int((over > BAR).sum())
            n += over.size
            fin = over[np.isfinite(over)]
            worst = max(worst, float(fin.max()) if fin.size else 0.0)
        shares[name], factor[name] = bad / n, worst
    print(f"\nadam mutant [{mutant}] share of elements beyond {BAR:g}x the bound: "
          + "  ".join(f"{k}={s:.1%} (worst {factor[k]:.1e}x)" for k, s in shares.items()))
    assert max(shares.values()) >= 0.20, shares

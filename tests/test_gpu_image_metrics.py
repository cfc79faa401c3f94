"""-m gpu: scoring rendered frames on the device (include/ngm_hip.h ngm_image_metrics; evaluation.image_metrics / psnr / ssim /
depthl1; NeuralGraphRenderer.evaluate_frame / evaluate_frames) against the fp64 host mirror tests/_image_metrics_host.py.  Raw C
calls run with `out` and the workspace between guard bands, the workspace pre-filled with NaN bytes.  The shapes are the smallest
at which the kernels can go wrong: one window, a ragged crop, at least three ragged tiles each way (a tile is 16 x 32 windows).

Bars against the mirror (derived, not tuned; tests/test_image_metrics_cpu.py holds the mirror's own summation orders to a tenth):
counts exact (integers); ssim 1e-10 absolute (a window sum of <= 22 sequential fp64 operations on values in [0, 1] errs by
<= 2.7e-15, the quotient amplifies by at most about 2 / c2 = 2.2e3: 6e-12); mse and depth_l1 1e-11 relative (<= 31 500 terms at
these sizes: worst case 3.5e-12); psnr 1e-10 absolute (4.34 x the relative error of mse plus one log10)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _image_metrics_host as IH  # noqa: E402
from gpu_common import DEV, make_renderer  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import evaluation as Ev  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from neural_graph_mapping_amd.renderer import Camera  # noqa: E402
from test_image_metrics_cpu import PSNR_BAR, REL_BAR, SSIM_BAR, TEXTURED  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 4096, 0xA5


class Banded:
    """`nbytes` of device memory between two bands of 4096 pattern bytes; fill: the byte the payload starts with"""

    def __init__(self, nbytes, fill):
        self.nbytes = int(nbytes)
        self.raw = torch.full((GUARD + self.nbytes + (-self.nbytes) % 256 + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.raw[GUARD:GUARD + self.nbytes] = fill
        self.ptr = self.raw.data_ptr() + GUARD

    def payload(self, dtype):
        return self.raw[GUARD:GUARD + self.nbytes].view(dtype)

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.raw[:GUARD] == PATTERN).all()) and bool((self.raw[GUARD + self.nbytes:] == PATTERN).all()), self.nbytes


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def c_metrics(pred, target, crop, calls=1):
    """ngm_image_metrics through the C ABI on (B, H, W, 4) arrays: `out` between guard bands, the workspace between guard bands and
    PRE-FILLED with 0xFF bytes (NaN as doubles) -> (B, 8) float64, or the list of `calls` results on the same workspace"""
    p, t = dev(np.asarray(pred, np.float32)), dev(np.asarray(target, np.float32))
    b, h, w = p.shape[:3]
    L = K.lib()
    wsb = L.ngm_image_metrics_workspace(b, h, w, crop)
    assert wsb > 0
    ws = Banded(wsb, 0xFF)
    res = []
    for _ in range(calls):
        out = Banded(64 * b, PATTERN)
        K.check(L.ngm_image_metrics(p.data_ptr(), t.data_ptr(), b, h, w, crop, out.ptr, ws.ptr, wsb, ops._stream()), "ngm_image_metrics")
        out.check()
        ws.check()
        res.append(out.payload(torch.float64).view(b, 8).cpu().numpy().copy())
    return res[0] if calls == 1 else res


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def against_mirror(got, want, what):
    """one row of the device against the mirror's: counts exact, NaN and inf in the same places, the rest within the bars"""
    assert np.array_equal(got[4:], want[4:]), (what, got, want)
    worst = {}
    for i, (name, bar, rel) in enumerate((("psnr", PSNR_BAR, False), ("ssim", SSIM_BAR, False), ("depth_l1", REL_BAR, True), ("mse", REL_BAR, True))):
        g, w = got[i], want[i]
        if np.isnan(w) or np.isinf(w):
            assert (np.isnan(g) and np.isnan(w)) or g == w, (what, name, g, w)
            continue
        err = abs(g - w) / abs(w) if rel and w != 0 else abs(g - w)
        worst[name] = (err, bar)
        assert err <= bar, (what, name, g, w, err, bar)
    print(what + ": " + ", ".join(f"{k} {e:.2e} (bar {b:.0e})" for k, (e, b) in worst.items()))


def check_batch(pred, target, crop, what):
    out = c_metrics(pred, target, crop)
    for b in range(len(pred)):
        want, _ = IH.image_metrics(pred[b], target[b], crop)
        against_mirror(out[b], want, f"{what} frame {b}")
    return out


# ------------------------------------------------------------------------------------------------ the table of cases
@pytest.mark.parametrize("h,w,crop,seed,noise", TEXTURED)
def test_textured_scenes_single_window_and_ragged_tiles(h, w, crop, seed, noise):
    """11 x 11 crop 0 and 31 x 31 crop 10: one window; 75 x 140 crop 1: 63 x 128 windows = 4 x 4 tiles, the last row of tiles 15
    high, and with crop 0 below 65 x 130: 5 x 5 tiles, ragged both ways"""
    pred, target = IH.textured(h, w, seed, noise)
    out = check_batch(pred[None], target[None], crop, f"{h} x {w} crop {crop}")
    assert out[0, 5] == 3 * (h - 2 * crop - 10) * (w - 2 * crop - 10)
    if h == 75:
        out = check_batch(pred[None], target[None], 0, f"{h} x {w} crop 0")
        assert out[0, 5] == 3 * 65 * 130


def test_ragged_crop_batch_of_three_where_the_clamp_acts():
    frames = [IH.beyond_range(33, 45, seed) for seed in (4, 5, 6)]
    pred, target = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    out = check_batch(pred, target, 10, "33 x 45 crop 10")
    assert np.all(out[:, 5] == 3 * 3 * 15) and np.all(out[:, 4] == 3 * 13 * 25) and np.all(out[:, 6] == 33 * 45)


def test_too_small_and_empty_regions():
    pred, target = IH.textured(10, 40, seed=6)
    out = check_batch(pred[None], target[None], 0, "10 x 40 crop 0")[0]
    assert np.isnan(out[1]) and out[5] == 0 and np.isfinite(out[0]) and np.isfinite(out[3]) and out[4] == 3 * 400
    pred, target = IH.textured(20, 20, seed=6)
    for crop in (10, 11):
        out = check_batch(pred[None], target[None], crop, f"20 x 20 crop {crop}")[0]
        assert np.isnan(out[0]) and np.isnan(out[1]) and np.isnan(out[3]) and out[4] == 0 and out[5] == 0
        assert np.isfinite(out[2]) and out[2] > 0 and out[6] == 400


def test_depth_zero_everywhere_and_on_a_lattice():
    pred, target = IH.textured(33, 45, seed=9)
    lattice = IH.textured(33, 45, seed=9, depth_zero_every=4)[1]
    lattice[1, 1, 3] = -0.0                                                  # does not take part either
    zero = target.copy()
    zero[..., 3] = 0.0
    pred[:10, :, 3] += 5.0                                                   # depth errors in the border the crop removes count
    out = check_batch(np.stack([pred, pred, pred]), np.stack([zero, lattice, target]), 10, "depth masks")
    assert np.isnan(out[0, 2]) and out[0, 6] == 0
    assert out[1, 6] == 33 * 45 - 9 * 12 - 1 and out[2, 6] == 33 * 45
    assert out[2, 2] > 1.0
    assert np.array_equal(bits(out[0, [0, 1, 3]]), bits(out[2, [0, 1, 3]]))   # the colour numbers do not see the depth


def test_nan_and_inf_spoil_what_the_mirror_says_and_no_other_frame():
    pred, target = IH.textured(33, 45, seed=5)
    p1 = pred.copy(); p1[16, 20, 1] = np.nan                                 # frame 1: one NaN in the prediction's colour
    t2 = target.copy(); t2[16, 20, 0] = np.inf; t2[3, 3, 3] = np.nan         # frame 2: inf in the target's colour, NaN target depth
    out = check_batch(np.stack([pred, p1, pred, pred]), np.stack([target, target, t2, target]), 2, "nan / inf")
    assert np.isfinite(out[0]).all() and np.array_equal(bits(out[0]), bits(out[3]))
    assert np.isnan(out[1, [0, 1, 3]]).all() and np.array_equal(bits(out[1, 2]), bits(out[0, 2]))
    assert np.isfinite(out[2, [0, 1, 3]]).all() and np.isnan(out[2, 2]) and out[2, 6] == out[0, 6]
    alone = c_metrics(pred[None], target[None], 2)
    assert np.array_equal(bits(alone[0]), bits(out[0]))


@pytest.mark.parametrize("shape,crop", [((11, 11), 0), ((33, 45), 10), ((75, 140), 1)])
def test_identical_frames_score_exactly(shape, crop):
    _, target = IH.textured(*shape, seed=7)
    out = c_metrics(target[None], target[None].copy(), crop)[0]
    assert out[1] == 1.0 and out[0] == np.inf and out[2] == 0.0 and out[3] == 0.0 and out[7] == 0.0
    want, _ = IH.image_metrics(target, target, crop)
    assert np.array_equal(out[4:], want[4:])


def test_no_pixels_gives_nan_rows_with_zero_counts():
    L = K.lib()
    stand_in = torch.zeros(64, device=DEV)                                   # a non-NULL address: no pixel is read
    for h, w in ((0, 17), (17, 0), (0, 0)):
        wsb = L.ngm_image_metrics_workspace(3, h, w, 0)
        out, ws = Banded(64 * 3, PATTERN), Banded(wsb, 0xFF)
        K.check(L.ngm_image_metrics(stand_in.data_ptr(), stand_in.data_ptr(), 3, h, w, 0, out.ptr, ws.ptr, wsb, ops._stream()), "no pixels")
        out.check()
        ws.check()
        rows = out.payload(torch.float64).view(3, 8).cpu().numpy()
        assert np.isnan(rows[:, :4]).all() and np.all(rows[:, 4:] == 0.0)
        got = Ev.image_metrics(torch.zeros(3, h, w, 4, device=DEV), torch.zeros(3, h, w, 4, device=DEV))
        assert bool(got["ssim"].isnan().all()) and bool((got["num_depth_pixels"] == 0).all())
    assert Ev.image_metrics(torch.zeros(0, 12, 12, 4, device=DEV), torch.zeros(0, 12, 12, 4, device=DEV))["psnr"].shape == (0,)


# ------------------------------------------------------------------------------------------------ repeatability
def test_two_calls_and_batch_against_single_frames_are_bitwise_equal():
    frames = [IH.textured(75, 140, seed, 0.01, depth_zero_every=5) for seed in (21, 22, 23)]
    pred, target = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    a, b = c_metrics(pred, target, 1, calls=2)                               # the second call finds the first one's rows in the workspace
    assert np.array_equal(bits(a), bits(b))
    for i in range(3):
        assert np.array_equal(bits(c_metrics(pred[i:i + 1], target[i:i + 1], 1)), bits(a[i:i + 1])), i


def test_op_and_host_layer_give_the_bits_of_the_raw_call():
    frames = [IH.beyond_range(33, 45, seed) for seed in (4, 5, 6)]
    pred, target = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    raw = c_metrics(pred, target, 10)
    p, t = dev(pred), dev(target)
    assert np.array_equal(bits(torch.ops.ngm355.image_metrics(p, t, 10).cpu().numpy()), bits(raw))
    d = Ev.image_metrics(p, t, crop=10)
    assert list(d) == ["psnr", "ssim", "depthl1", "mse", "num_color_terms", "num_ssim_windows", "num_depth_pixels"]
    for i, v in enumerate(d.values()):
        assert v.is_cuda and v.dtype == torch.float64 and v.shape == (3,)
        assert np.array_equal(bits(v.cpu().numpy()), bits(raw[:, i]))
    one = Ev.image_metrics(p[1], t[1], crop=10)
    assert all(v.shape == () for v in one.values()) and float(one["ssim"]) == raw[1, 1]
    # the reference's three functions: (H, W, 3) colour and (H, W) depth
    assert Ev.psnr(p[2, ..., :3], t[2, ..., :3], 10) == raw[2, 0]
    assert Ev.ssim(p[2, ..., :3], t[2, ..., :3], 10) == raw[2, 1]
    assert Ev.depthl1(p[2, ..., 3], t[2, ..., 3], 10) == raw[2, 2]
    with pytest.raises(ValueError, match="differ in size"):
        Ev.image_metrics(p, t[:2])


def test_call_is_capturable_in_a_graph():
    pred, target = IH.textured(33, 45, seed=31)
    p, t = dev(pred[None]), dev(target[None])
    want = torch.ops.ngm355.image_metrics(p, t, 2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = torch.ops.ngm355.image_metrics(p, t, 2)
    t.copy_(dev(IH.textured(33, 45, seed=32)[1][None]))
    g.replay()
    torch.cuda.synchronize()
    again = torch.ops.ngm355.image_metrics(p, t, 2)
    assert torch.equal(out, again) and not torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ the host layer on a renderer
@pytest.fixture(scope="module")
def scene():
    torch.manual_seed(5)
    r = make_renderer(dict(encoding="fourier", dim_enc=32, num_layers=1),
                      dict(num_samples_coarse=8, num_samples_depth_guided=8, eval_num_samples=24, eval_far_distance=4.0, eval_crop=10,
                           eval_metrics=["psnr", "ssim", "depthl1"]), 8)
    g = torch.tensor([-0.6, 0.6])
    pos = torch.stack(torch.meshgrid(g, g, torch.tensor([-2.2, -1.8]), indexing="ij"), -1).reshape(-1, 3)
    quat = torch.nn.functional.normalize(torch.randn(8, 4), dim=-1)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    cam = Camera(40, 32, 35.0, 35.0, 19.5, 15.5, pixel_center=0.0)
    c2ws = []
    for k in range(3):
        c2w = torch.eye(4)
        c2w[0, 3] = 0.1 * (k - 1)
        c2ws.append(c2w.to(DEV))
    targets = [dev(IH.textured(32, 40, seed=40 + k, depth_zero_every=3)[1]) for k in range(3)]
    return r, cam, c2ws, targets


def test_evaluate_frame_is_the_mirror_of_the_rendered_image(scene):
    r, cam, c2ws, targets = scene
    got = r.evaluate_frame(c2ws[0], targets[0], camera=cam, seed=3)
    assert r._mode == "train" and list(got) == ["psnr", "ssim", "depthl1"] and all(isinstance(v, float) for v in got.values())
    r.eval()
    rgbd, _ = r.render_image(c2ws[0], cam, seed=3)
    r.train()
    assert rgbd.shape == (32, 40, 4)
    want, _ = IH.image_metrics(rgbd.cpu().numpy(), targets[0].cpu().numpy(), 10)        # config eval_crop
    assert want[5] == 3 * 2 * 10
    against_mirror(np.array([got["psnr"], got["ssim"], got["depthl1"], want[3], *want[4:]]), want, "evaluate_frame")
    sub = r.evaluate_frame(c2ws[0], targets[0], camera=cam, metrics=["ssim"], crop=0, seed=3)
    want0, _ = IH.image_metrics(rgbd.cpu().numpy(), targets[0].cpu().numpy(), 0)
    assert list(sub) == ["ssim"] and abs(sub["ssim"] - want0[1]) <= SSIM_BAR and r._mode == "train"


def test_evaluate_frames_gives_the_mean_of_the_frames(scene):
    r, cam, c2ws, targets = scene
    singles = [r.evaluate_frame(c2ws[k], targets[k], camera=cam, seed=3) for k in range(3)]
    mean, per_frame = r.evaluate_frames(c2ws, targets, camera=cam, seed=3, batch=2)
    assert r._mode == "train" and isinstance(per_frame, np.ndarray) and per_frame.shape == (3, 8) and per_frame.dtype == np.float64
    for k in range(3):
        assert [per_frame[k, 0], per_frame[k, 1], per_frame[k, 2]] == [singles[k][m] for m in ("psnr", "ssim", "depthl1")]
    for m in ("psnr", "ssim", "depthl1"):
        assert mean[m] == (singles[0][m] + singles[1][m] + singles[2][m]) / 3
    assert r.evaluate_frames([], [], camera=cam)[0] == {}


def test_lpips_unknown_names_and_bad_targets_raise(scene):
    r, cam, c2ws, targets = scene
    with pytest.raises(NotImplementedError, match="weights"):
        r.evaluate_frame(c2ws[0], targets[0], camera=cam, metrics=["psnr", "lpips"])
    with pytest.raises(ValueError, match="Unknown render metric"):
        r.evaluate_frames(c2ws, targets, camera=cam, metrics=["f1"])
    with pytest.raises(ValueError, match="crop"):
        r.evaluate_frame(c2ws[0], targets[0], camera=cam, crop=-1)
    with pytest.raises(ValueError, match="target_rgbd"):
        r.evaluate_frame(c2ws[0], targets[0][:, :, :3], camera=cam)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.evaluate_frame(c2ws[0], targets[0].cpu(), camera=cam)
    assert r._mode == "train"

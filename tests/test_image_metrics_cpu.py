"""CPU-side checks of the per-frame render metrics (include/ngm_hip.h ngm_image_metrics; evaluation.image_metrics / psnr / ssim /
depthl1; NeuralGraphRenderer.evaluate_frame / evaluate_frames): the fp64 host mirror tests/_image_metrics_host.py obeys the rules
of the header, is compared with an independent fp32 restatement of torchmetrics' algorithm, and keeps its own summation orders
within a tenth of the bars the GPU tests hold the kernels to; the C ABI, the op and the host layer refuse what they must without a
device."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _image_metrics_host as IH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bars of tests/test_gpu_image_metrics.py against the mirror (derived in the issue, restated there)
SSIM_BAR, REL_BAR, PSNR_BAR = 1e-10, 1e-11, 1e-10
# the textured scenes the GPU tests use: (height, width, crop, seed, noise)
TEXTURED = [(11, 11, 0, 1, 0.02), (31, 31, 10, 2, 0.02), (75, 140, 1, 3, 0.01)]


def torchmetrics_fp32(pred, target, crop):
    """torchmetrics.functional.structural_similarity_index_measure(data_range=1.0) as evaluation.ssim calls it
    (evaluation.py:20-30), restated from its public algorithm in torch fp32: crop, clamp, the 11 x 11 Gaussian of sigma 1.5,
    reflect padding by 5, ONE grouped conv2d over the five stacked inputs, variances clamped at 0, the padded border cut off
    again, the mean.  Returns (mean, per-pixel map (3, h - 10, w - 10)) as float64 numpy."""
    import torch
    import torch.nn.functional as F
    p, t = torch.from_numpy(pred[..., :3].copy()), torch.from_numpy(target[..., :3].copy())
    if crop > 0:
        p, t = p[crop:-crop, crop:-crop], t[crop:-crop, crop:-crop]
    p = p.permute(2, 0, 1).unsqueeze(0).clamp(0.0, 1.0)
    t = t.permute(2, 0, 1).unsqueeze(0).clamp(0.0, 1.0)
    dist = torch.arange((1 - 11) / 2, (1 + 11) / 2, 1, dtype=torch.float32)
    gauss = torch.exp(-torch.pow(dist / 1.5, 2) / 2)
    g = (gauss / gauss.sum()).unsqueeze(0)
    kernel = torch.matmul(g.t(), g).expand(3, 1, 11, 11)
    c1, c2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
    p, t = F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect")
    out = F.conv2d(torch.cat((p, t, p * p, t * t, p * t)), kernel, groups=3)
    mp, mt, pp, tt, pt = out.split(1)
    vp = torch.clamp(pp - mp * mp, min=0.0)
    vt = torch.clamp(tt - mt * mt, min=0.0)
    vpt = pt - mp * mt
    full = ((2 * mp * mt + c1) * (2 * vpt + c2)) / ((mp * mp + mt * mt + c1) * (vp + vt + c2))
    cut = full[..., 5:-5, 5:-5]
    return float(cut.reshape(1, -1).mean(-1)[0]), cut[0].double().numpy()


# ------------------------------------------------------------------------------------------------ the mirror
def test_weights_sum_to_one_and_are_symmetric():
    g = IH.weights()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(g[4] / g[5] - np.exp(-(1 / 1.5) ** 2 / 2)) < 1e-15


@pytest.mark.parametrize("shape,crop", [((11, 11), 0), ((31, 31), 10), ((33, 45), 10), ((75, 140), 1)])
def test_identical_images_give_exactly_one_inf_and_zero(shape, crop):
    _, target = IH.textured(*shape, seed=7)
    row, smap = IH.image_metrics(target, target.copy(), crop)
    assert np.all(smap == 1.0) and row[1] == 1.0
    assert row[0] == np.inf and row[3] == 0.0 and row[2] == 0.0
    h, w = shape[0] - 2 * crop, shape[1] - 2 * crop
    assert row[4] == 3 * h * w and row[5] == 3 * (h - 10) * (w - 10) and row[6] == shape[0] * shape[1] and row[7] == 0.0


def test_counts_of_the_ragged_crop():
    pred, target = IH.beyond_range(33, 45, seed=4)
    row, smap = IH.image_metrics(pred, target, 10)
    assert smap.shape == (3, 15, 3) and row[4] == 3 * 13 * 25 and row[5] == 3 * 3 * 15
    assert ((pred[..., :3] < 0) | (pred[..., :3] > 1)).mean() > 0.1            # the clamp acts
    assert 0.0 < row[3] < 1.0 and np.isfinite(row[0]) and -1.0 < row[1] < 1.0


def test_nan_is_kept_and_spoils_only_what_it_touches():
    pred, target = IH.textured(33, 45, seed=5)
    clean, _ = IH.image_metrics(pred, target, 2)
    p = pred.copy(); p[16, 20, 1] = np.nan                                   # colour of the prediction, inside the region
    row, smap = IH.image_metrics(p, target, 2)
    assert np.isnan(row[0]) and np.isnan(row[1]) and np.isnan(row[3]) and row[2] == clean[2]
    assert np.isnan(smap[..., 1]).sum() == 121 and not np.isnan(smap[..., 0]).any() and not np.isnan(smap[..., 2]).any()
    t = target.copy(); t[16, 20, 0] = np.inf                                 # inf clamps to 1: everything stays finite
    row, _ = IH.image_metrics(pred, t, 2)
    assert np.isfinite(row[:4]).all() and row[3] > clean[3] and row[2] == clean[2]
    t = target.copy(); t[3, 3, 3] = np.nan                                   # a NaN target depth takes part
    row, _ = IH.image_metrics(pred, t, 2)
    assert np.isnan(row[2]) and row[6] == clean[6] and np.array_equal(row[[0, 1, 3]], clean[[0, 1, 3]])
    p = pred.copy(); p[0, 0, 0] = np.nan                                     # in the cropped border: colour does not see it
    row, _ = IH.image_metrics(p, target, 2)
    assert np.array_equal(row, clean)
    assert np.isnan(IH.clamp01(np.float32("nan"))) and IH.clamp01(np.float32("inf")) == 1.0 and IH.clamp01(np.float32("-inf")) == 0.0


def test_too_small_and_empty_regions():
    pred, target = IH.textured(10, 40, seed=6)
    row, smap = IH.image_metrics(pred, target, 0)                            # fewer than 11 rows: OUR RULE
    assert smap is None and np.isnan(row[1]) and row[5] == 0 and np.isfinite(row[0]) and row[4] == 3 * 10 * 40
    pred, target = IH.textured(20, 20, seed=6)
    for crop in (10, 11, 500):                                               # 2 crop >= size: the region is empty
        row, smap = IH.image_metrics(pred, target, crop)
        assert smap is None and np.isnan(row[0]) and np.isnan(row[1]) and np.isnan(row[3]) and row[4] == 0 and row[5] == 0
        assert np.isfinite(row[2]) and row[6] == 400
    row, _ = IH.image_metrics(pred, target, 5)                               # 10 x 10 left
    assert np.isnan(row[1]) and np.isfinite(row[0]) and row[4] == 300


def test_depth_ignores_the_crop_and_counts_nonzero_targets():
    pred, target = IH.textured(31, 31, seed=8)
    pred[:10, :, 3] += 5.0                                                   # large depth errors in the border the crop removes
    row0, _ = IH.image_metrics(pred, target, 0)
    row10, _ = IH.image_metrics(pred, target, 10)
    want = np.abs(pred[..., 3].astype(np.float64) - target[..., 3].astype(np.float64)).mean()
    assert row0[2] == row10[2] and abs(row10[2] - want) < 1e-12 and row10[2] > 1.5 and row10[6] == 31 * 31
    _, lattice = IH.textured(31, 31, seed=8, depth_zero_every=4)
    row, _ = IH.image_metrics(pred, lattice, 10)
    assert row[6] == 31 * 31 - 8 * 8
    lattice[1, 1, 3] = -0.0                                                  # -0.0 does not take part
    assert IH.image_metrics(pred, lattice, 10)[0][6] == 31 * 31 - 8 * 8 - 1
    lattice[..., 3] = 0.0
    row, _ = IH.image_metrics(pred, lattice, 10)
    assert np.isnan(row[2]) and row[6] == 0


@pytest.mark.parametrize("h,w,crop,seed,noise", TEXTURED + [(37, 53, 0, 11, 0.02), (480, 640, 10, 12, 0.02)])
def test_mirror_against_the_fp32_restatement_of_torchmetrics(h, w, crop, seed, noise):
    pred, target = IH.textured(h, w, seed, noise)
    row, smap = IH.image_metrics(pred, target, crop)
    mean32, map32 = torchmetrics_fp32(pred, target, crop)
    dmean, dpix = abs(row[1] - mean32), np.abs(smap.transpose(2, 0, 1) - map32).max()
    # one window: the restatement's rounding in E[x^2] - mu^2 (a few 2^-24 of values up to 1) is divided by sums that start at
    # c2 = 9e-4, so a single window differs by up to about 2 / c2 x 8 x 2^-24 = 1.1e-3 (3e-4 was seen when the feature was specified)
    window_bar = 2 / IH.C2 * 8 * 2.0 ** -24
    # the mean: these errors average out over the windows.  10 x the largest difference measured on such scenes when the feature
    # was specified (1.4e-7), never above 2e-6.  The two single-window scenes have nothing to average: their mean IS one window
    # and is held to the window bar
    bar = min(10 * 1.4e-7, 2e-6) if smap.size > 3 else window_bar
    print(f"{h} x {w} crop {crop}: ssim {row[1]:.9f}, |mean - fp32 restatement| {dmean:.2e} (bar {bar:.1e}), worst window {dpix:.2e} "
          f"(bar {window_bar:.1e})")
    assert dmean < bar
    assert dpix < window_bar


def test_near_flat_scene_shows_the_bias_of_fp32():
    pred, target = IH.near_flat(37, 53, seed=13)
    row, smap = IH.image_metrics(pred, target, 0)
    mean32, map32 = torchmetrics_fp32(pred, target, 0)
    print(f"near flat: fp64 ssim {row[1]:.6f}, fp32 restatement {mean32:.6f}, difference {abs(row[1] - mean32):.2e} (must exceed 1e-4), "
          f"worst pixel {np.abs(smap.transpose(2, 0, 1) - map32).max():.2e}")
    assert abs(row[1] - mean32) > 1e-4


@pytest.mark.parametrize("h,w,crop,seed,noise", TEXTURED + [(33, 45, 10, 4, None), (37, 53, 0, 13, "flat")])
def test_summation_orders_of_the_mirror_agree_within_a_tenth_of_the_bars(h, w, crop, seed, noise):
    if noise is None:
        pred, target = IH.beyond_range(h, w, seed)
    elif noise == "flat":
        pred, target = IH.near_flat(h, w, seed)
    else:
        pred, target = IH.textured(h, w, seed, noise)
    rows, smap_r = IH.image_metrics(pred, target, crop, order="rows_first")
    cols, smap_c = IH.image_metrics(pred, target, crop, order="columns_first")
    d = abs(rows[1] - cols[1])
    print(f"{h} x {w} crop {crop}: rows first against columns first: ssim {d:.2e} (bar {SSIM_BAR / 10:.0e}), worst window "
          f"{np.abs(smap_r - smap_c).max():.2e}")
    assert d < SSIM_BAR / 10
    # mse and depth L1: the sum taken pixel by pixel in fp64 against numpy's pairwise sum
    x, y = IH.clamp01(pred[crop:h - crop, crop:w - crop, :3]), IH.clamp01(target[crop:h - crop, crop:w - crop, :3])
    seq = 0.0
    for v in ((x - y) ** 2).ravel():
        seq += v
    mse = seq / x.size
    assert abs(mse - rows[3]) <= REL_BAR / 10 * rows[3]
    assert abs(10 * np.log10(1 / mse) - rows[0]) <= PSNR_BAR / 10
    seq = 0.0
    for v in np.abs(pred[..., 3].astype(np.float64) - target[..., 3].astype(np.float64)).ravel():
        seq += v
    assert abs(seq / (h * w) - rows[2]) <= REL_BAR / 10 * rows[2]


# ------------------------------------------------------------------------------------------------ the library without a device
@pytest.fixture(scope="module")
def capi():
    from neural_graph_mapping_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from neural_graph_mapping_amd import build
        build.build(verbose=False)
    return _capi


NAMES = ("ngm_image_metrics_workspace", "ngm_image_metrics")


def test_entry_points_are_declared_exported_and_additive(capi):
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "ngm_hip.h")).read()
    L = capi.lib()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in capi.EXPORTED and hasattr(L, name)
    assert L.ngm_abi_version() == 11 and re.search(r"#define\s+NGM_ABI_VERSION\s+11\b", hdr)
    assert len(L.ngm_image_metrics.argtypes) == 10 and len(L.ngm_image_metrics_workspace.argtypes) == 4
    assert L.ngm_image_metrics_workspace.restype is C.c_int64 and L.ngm_image_metrics_workspace.argtypes[0] is C.c_int32
    assert "PARITY UNPINNED against torchmetrics" in hdr and "OUR RULE: fewer than 11 rows or columns" in hdr


def test_workspace_query_refuses_and_is_monotone(capi):
    L, INV = capi.lib(), capi.NGM_E_INVALID
    ws = L.ngm_image_metrics_workspace
    for bad in ((-1, 10, 10, 0), (1, -1, 10, 0), (1, 10, -1, 0), (1, 10, 10, -1), (2, 2 ** 15, 2 ** 15, 0), (2 ** 11, 2 ** 10, 2 ** 10, 0)):
        assert ws(*bad) == INV, bad
    assert ws(2 ** 11 - 1, 2 ** 10, 2 ** 10, 0) > 0 and ws(0, 480, 640, 10) > 0 and ws(3, 0, 640, 0) > 0 and ws(3, 480, 0, 0) > 0
    base = (4, 480, 640, 10)
    for arg in range(3):                                                     # never smaller for more frames, rows or columns
        sizes = [ws(*[v if i != arg else k for i, v in enumerate(base)]) for k in (0, 1, 2, 11, 30, 31, 100, 481, 1000, 2000)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0], (arg, sizes)
    sizes = [ws(4, 480, 640, crop) for crop in (0, 1, 10, 100, 234, 235, 240, 1000, 2 ** 31 - 1)]
    assert sizes == sorted(sizes, reverse=True) and sizes[0] > sizes[-1]    # never larger for a larger crop


def test_entry_point_refuses_bad_arguments_before_any_launch(capi):
    L, INV = capi.lib(), capi.NGM_E_INVALID
    p = 256                                                                  # a non-NULL address nothing may reach
    wsb = L.ngm_image_metrics_workspace(2, 33, 45, 10)

    def args(**kw):
        a = dict(pred=p, target=p, B=2, H=33, W=45, crop=10, out=p, ws=p, wsb=wsb)
        a.update(kw)
        return tuple(a.values()) + (None,)

    bad = [dict(pred=None), dict(target=None), dict(out=None), dict(ws=None), dict(B=-1), dict(H=-1), dict(W=-1), dict(crop=-1),
           dict(B=2, H=2 ** 15, W=2 ** 15), dict(B=2 ** 11, H=2 ** 10, W=2 ** 10), dict(wsb=wsb - 1), dict(wsb=0), dict(pred=p + 4),
           dict(target=p + 8)]
    for kw in bad:
        assert L.ngm_image_metrics(*args(**kw)) == INV, kw
        assert L.ngm_last_error().startswith(b"ngm_image_metrics")
    # no frame: nothing is launched, nothing is touched
    assert L.ngm_image_metrics(*args(B=0)) == capi.NGM_OK
    assert L.ngm_image_metrics(*args(B=0, H=0, W=0, crop=0)) == capi.NGM_OK


def test_op_exists_with_fake_shapes_and_no_cpu_kernel(capi):
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from neural_graph_mapping_amd import evaluation as Ev  # noqa: F401
    assert hasattr(torch.ops.ngm355, "image_metrics")
    with FakeTensorMode():
        for b in (0, 1, 5):
            x = torch.empty(b, 20, 30, 4, device="cuda")
            out = torch.ops.ngm355.image_metrics(x, x, 3)
            assert out.shape == (b, 8) and out.dtype == torch.float64 and out.device.type == "cuda"
    x = torch.zeros(1, 12, 12, 4)
    with pytest.raises((RuntimeError, NotImplementedError)):                 # the dispatcher itself: no CPU kernel
        torch.ops.ngm355.image_metrics(x, x, 0)


def test_host_layer_refuses_cpu_tensors_and_bad_arguments_before_any_launch(capi, monkeypatch):
    import torch
    from neural_graph_mapping_amd import evaluation as Ev
    x = torch.zeros(12, 12, 4)
    for fn, a in ((Ev.image_metrics, x), (Ev.image_metrics, x[None]), (Ev.psnr, x[..., :3]), (Ev.ssim, x[..., :3]), (Ev.depthl1, x[..., 3])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(a, a)

    def no_launch(*a, **k):
        raise AssertionError("a launch was reached")
    monkeypatch.setattr(Ev.ops, "_require_gpu", lambda *t: None)
    monkeypatch.setattr(Ev.K, "lib", no_launch)
    for crop in (-1, 1.0, 2.5, None, True, "3"):
        for fn, a in ((Ev.image_metrics, x), (Ev.psnr, x[..., :3]), (Ev.ssim, x[..., :3]), (Ev.depthl1, x[..., 3])):
            with pytest.raises(ValueError, match="crop"):
                fn(a, a, crop)
    for bad in (torch.zeros(12, 12, 3), torch.zeros(12, 12), torch.zeros(2, 2, 12, 12, 4), torch.zeros(12, 12, 4, dtype=torch.float64),
                torch.zeros(1, 12, 12, 4, dtype=torch.float16)):
        with pytest.raises(ValueError, match="image_metrics expects"):
            Ev.image_metrics(bad, bad)
    for a, b in ((x, torch.zeros(12, 13, 4)), (x, x[None]), (x[None], torch.zeros(2, 12, 12, 4))):
        with pytest.raises(ValueError, match="differ in size"):
            Ev.image_metrics(a, b)
    for fn, good, bads in ((Ev.psnr, x[..., :3], (x, x[..., 0], x[..., :3].double())), (Ev.ssim, x[..., :3], (x, x[..., 0])),
                           (Ev.depthl1, x[..., 0], (x, x[..., :3], x[..., 0].double()))):
        for bad in bads:
            with pytest.raises(ValueError, match="expects float32"):
                fn(bad, bad)
        with pytest.raises(ValueError, match="differ in size"):
            fn(good, good[:5])
    with pytest.raises(NotImplementedError, match="weights"):
        Ev.check_metrics(["psnr", "lpips"])
    with pytest.raises(ValueError, match="Unknown render metric"):
        Ev.check_metrics(["psnr", "mse"])
    assert Ev.check_metrics(("ssim", "psnr")) == ["ssim", "psnr"] and Ev.check_metrics([]) == []


def test_mean_metric_dict_is_the_references():
    from neural_graph_mapping_amd import evaluation as Ev
    rows = np.array([[20.0, 0.5, 0.1, 0, 0, 0, 0, 0], [30.0, 0.7, 0.3, 0, 0, 0, 0, 0], [np.inf, 0.9, np.nan, 0, 0, 0, 0, 0]])
    mean = Ev.mean_metric_dict(rows[:2], ["ssim", "psnr"])
    assert list(mean) == ["ssim", "psnr"] and mean["psnr"] == 25.0 and mean["ssim"] == (0.5 + 0.7) / 2
    mean = Ev.mean_metric_dict(rows, ["psnr", "depthl1"])
    assert mean["psnr"] == np.inf and np.isnan(mean["depthl1"])


def test_signatures_and_the_statement_that_went():
    from neural_graph_mapping_amd import evaluation as Ev
    from neural_graph_mapping_amd.renderer import NeuralGraphRenderer as Renderer
    for fn in (Ev.psnr, Ev.ssim, Ev.depthl1):                                # evaluation.py:20, 46, 59
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["prediction", "target", "crop"] and sig.parameters["crop"].default == 0
    sig = inspect.signature(Ev.image_metrics)
    assert list(sig.parameters) == ["pred", "target", "crop"] and sig.parameters["crop"].default == 0
    sig = inspect.signature(Renderer.evaluate_frame)
    assert list(sig.parameters) == ["self", "c2w", "target_rgbd", "camera", "metrics", "crop", "seed"]
    assert [sig.parameters[k].default for k in ("camera", "metrics", "crop", "seed")] == [None, None, None, 0]
    sig = inspect.signature(Renderer.evaluate_frames)
    assert list(sig.parameters)[:7] == ["self", "c2ws", "target_rgbds", "camera", "metrics", "crop", "seed"]
    assert list(inspect.signature(Renderer.psnr).parameters) == ["prediction", "target", "crop"]     # stays as it is
    stale = re.compile(r"OUT OF SCOPE[^\n]*SSIM", re.I)
    for rel in ("neural_graph_mapping_amd/mesh.py", "include/ngm_hip.h", "DESIGN.md", "README.md", "INTEGRATION.md"):
        assert not stale.search(open(os.path.join(ROOT, rel)).read()), rel

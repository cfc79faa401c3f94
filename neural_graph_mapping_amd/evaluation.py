"""Per-frame render metrics on the device: PSNR, SSIM and depth L1 in fp64 (the reference's evaluation.psnr / ssim / depthl1,
evaluation.py:20-62, as NeuralGraphMap._evaluate_frame calls them, run_mapping.py:1977-2020).

One C call scores a batch of frames (ngm_image_metrics, csrc/ngm_image_metrics.hip; the definitions are its contract in
include/ngm_hip.h): no transfer, no host synchronisation, bitwise repeatable.  PARITY UNPINNED against torchmetrics (not a
dependency): the algorithm is its public one, evaluated in fp64 instead of fp32; the yardstick is tests/_image_metrics_host.py.
LPIPS is not built: its network weights are not part of this project.  There is no CPU fallback."""
import numbers

import torch

from . import _capi as K
from . import ops

OUT_COLUMNS = ("psnr", "ssim", "depthl1", "mse", "num_color_terms", "num_ssim_windows", "num_depth_pixels")
METRICS = ("psnr", "ssim", "depthl1")                          # what evaluate_frame can be asked for, besides "lpips" (raises)


@ops._op("image_metrics")
def _image_metrics_op(pred: torch.Tensor, target: torch.Tensor, crop: int) -> torch.Tensor:
    """(B, 8) fp64: the row layout of include/ngm_hip.h"""
    L = K.lib()
    b, h, w = pred.shape[0], pred.shape[1], pred.shape[2]
    wsb = L.ngm_image_metrics_workspace(b, h, w, crop)
    if wsb < 0:
        raise K.NgmError(f"image_metrics: {b} frames of {h} x {w} with crop {crop} not supported (batch * height * width < 2^31)", code=int(wsb))
    ws = torch.empty(wsb, device=pred.device, dtype=torch.uint8)
    out = torch.empty(b, 8, device=pred.device, dtype=torch.float64)
    if b == 0:
        return out
    # frames without pixels have no address; the call refuses NULL and reads nothing there, so `out` stands in
    pp, tp = (pred.data_ptr(), target.data_ptr()) if h * w > 0 else (out.data_ptr(), out.data_ptr())
    K.check(L.ngm_image_metrics(pp, tp, b, h, w, int(crop), out.data_ptr(), ws.data_ptr(), wsb, ops._stream()), "ngm_image_metrics")
    return out


@_image_metrics_op.register_fake
def _(pred, target, crop):
    return pred.new_empty(pred.shape[0], 8, dtype=torch.float64)


def _check_crop(crop) -> int:
    if isinstance(crop, bool) or not isinstance(crop, numbers.Integral) or crop < 0:
        raise ValueError(f"crop must be an integer >= 0, got {crop!r}")
    return int(crop)


def image_metrics_raw(pred: torch.Tensor, target: torch.Tensor, crop: int = 0) -> torch.Tensor:
    """pred, target (B, H, W, 4) fp32 r g b depth -> the (B, 8) fp64 rows of ngm_image_metrics on the device."""
    ops._require_gpu(pred, target)
    crop = _check_crop(crop)
    for name, t in (("pred", pred), ("target", target)):
        if t.dim() != 4 or t.shape[3] != 4 or t.dtype != torch.float32:
            raise ValueError(f"image_metrics expects {name} as (B, H, W, 4) float32 r g b depth, got {tuple(t.shape)} {t.dtype}")
    if pred.shape != target.shape:
        raise ValueError(f"image_metrics: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in size")
    if pred.device != target.device:
        raise ValueError("image_metrics: pred and target are on different devices")
    return torch.ops.ngm355.image_metrics(pred.contiguous(), target.contiguous(), crop)


def image_metrics(pred: torch.Tensor, target: torch.Tensor, crop: int = 0) -> dict:
    """Score rendered frames against their targets.  pred, target: (H, W, 4) or (B, H, W, 4) float32 device tensors, r g b depth
    (what render_image returns and a keyframe holds); crop: the reference's eval_crop (PSNR and SSIM leave that border out,
    depth L1 runs over the whole image, as the reference's does).  Returns device tensors, fp64, 0-d for one frame or (B,):
    psnr, ssim, depthl1, mse and the counts num_color_terms, num_ssim_windows, num_depth_pixels.  No transfer is made.
    SSIM is NaN where the cropped image has fewer than 11 rows or columns; PSNR too where it is empty; depth L1 where no target
    depth is non-zero."""
    ops._require_gpu(pred, target)
    _check_crop(crop)
    single = pred.dim() == 3
    if single != (target.dim() == 3):
        raise ValueError(f"image_metrics: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in size")
    out = image_metrics_raw(pred[None] if single else pred, target[None] if single else target, crop)
    return {name: (out[0, i] if single else out[:, i]) for i, name in enumerate(OUT_COLUMNS)}


def _rgbd_pair(fn, prediction, target, channels):
    """the reference passes (H, W, 3) colour or (H, W) depth: place them in the r g b depth layout the kernel reads"""
    ops._require_gpu(prediction, target)
    want = "(H, W, 3) colour" if channels == 3 else "(H, W) depth"
    for t in (prediction, target):
        if t.dtype != torch.float32 or t.dim() != (3 if channels == 3 else 2) or (channels == 3 and t.shape[2] != 3):
            raise ValueError(f"{fn} expects float32 {want}, got {tuple(t.shape)} {t.dtype}")
    if prediction.shape != target.shape:
        raise ValueError(f"{fn}: prediction {tuple(prediction.shape)} and target {tuple(target.shape)} differ in size")
    h, w = prediction.shape[0], prediction.shape[1]
    pair = torch.zeros(2, h, w, 4, device=prediction.device, dtype=torch.float32)
    if channels == 3:
        pair[0, :, :, :3], pair[1, :, :, :3] = prediction, target
    else:
        pair[0, :, :, 3], pair[1, :, :, 3] = prediction, target
    return pair


def psnr(prediction: torch.Tensor, target: torch.Tensor, crop: int = 0) -> float:
    """evaluation.psnr (evaluation.py:46-56): (H, W, 3) colour, clamped to [0, 1], border `crop` left out, data range 1."""
    crop = _check_crop(crop)
    pair = _rgbd_pair("psnr", prediction, target, 3)
    return float(image_metrics_raw(pair[:1], pair[1:], crop)[0, 0])


def ssim(prediction: torch.Tensor, target: torch.Tensor, crop: int = 0) -> float:
    """evaluation.ssim (evaluation.py:20-30): (H, W, 3) colour, torchmetrics' defaults (11 x 11 Gaussian, sigma 1.5) in fp64."""
    crop = _check_crop(crop)
    pair = _rgbd_pair("ssim", prediction, target, 3)
    return float(image_metrics_raw(pair[:1], pair[1:], crop)[0, 1])


def depthl1(prediction: torch.Tensor, target: torch.Tensor, crop: int = 0) -> float:
    """evaluation.depthl1 (evaluation.py:59-62): (H, W) depth, mean |difference| where target != 0; `crop` is accepted and,
    as in the reference, not used."""
    crop = _check_crop(crop)
    pair = _rgbd_pair("depthl1", prediction, target, 1)
    return float(image_metrics_raw(pair[:1], pair[1:], crop)[0, 2])


def check_metrics(metrics) -> list:
    """the names evaluate_frame accepts, in the caller's order"""
    metrics = list(metrics)
    for m in metrics:
        if m == "lpips":
            raise NotImplementedError("lpips is not built: the network weights it needs are not part of this project "
                                      f"(built: {list(METRICS)})")
        if m not in METRICS:
            raise ValueError(f"Unknown render metric {m!r} (built: {list(METRICS)})")
    return metrics


def mean_metric_dict(per_frame, metrics) -> dict:
    """_mean_metric_dict (run_mapping.py:82-92) over the rows of a (N, 8) host array: the values are added frame by frame and
    divided by their number"""
    mean = {}
    for m in metrics:
        col = OUT_COLUMNS.index(m)
        total = 0
        for row in per_frame:
            total += float(row[col])
        mean[m] = total / len(per_frame)
    return mean

"""fp64 host mirror of ngm_image_metrics (include/ngm_hip.h): PSNR, SSIM and depth L1 of one frame, every operation after the
fp32 load in float64, written to the header's rules in numpy.  It is the yardstick of the kernels (parity with torchmetrics
itself is unpinned: it is not a dependency), and it builds the scenes the CPU and GPU tests share."""
import math

import numpy as np

C1, C2 = 1e-4, 9e-4
TAPS = 11


def weights():
    """g_i proportional to exp(-((i - 5) / 1.5)^2 / 2), i = 0..10, normalised to sum 1 in fp64 (the sum taken in index order)"""
    g = [math.exp(-(((i - 5) / 1.5) ** 2) / 2.0) for i in range(TAPS)]
    total = 0.0
    for v in g:
        total += v
    return np.array([v / total for v in g], np.float64)


def clamp01(v):
    """torch.clamp(v, 0, 1): NaN passes through both comparisons"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(v < 0.0, 0.0, np.where(v > 1.0, 1.0, v))


def _taps(a, axis, fused=False):
    """the 11-tap weighted sum along `axis`, valid positions only, taps in index order from 0 (the device adds each tap by one
    fused multiply-add; numpy rounds the product first -- a difference of rounding level, which the bars cover)"""
    g = weights()
    n = a.shape[axis] - (TAPS - 1)
    out = np.zeros(a.shape[:axis] + (n,) + a.shape[axis + 1:], np.float64)
    for k in range(TAPS):
        sl = [slice(None)] * a.ndim
        sl[axis] = slice(k, k + n)
        out = out + g[k] * a[tuple(sl)]
    return out


def ssim_map(x, y, order="rows_first"):
    """x, y: (h, w, 3) float64 clamped colour of the cropped region, h, w >= 11 -> s per window and channel, (h - 10, w - 10, 3).
    order: "rows_first" sums along the row and then down the column, as the device does; "columns_first" the other way."""
    first, second = (1, 0) if order == "rows_first" else (0, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        e = [_taps(_taps(v, first), second) for v in (x, y, x * x, y * y, x * y)]
        mx, my, xx, yy, xy = e
        vx, vy = xx - mx * mx, yy - my * my
        vx = np.where(vx < 0.0, 0.0, vx)                                   # max(., 0) that keeps NaN
        vy = np.where(vy < 0.0, 0.0, vy)
        vxy = xy - mx * my
        return ((2.0 * mx * my + C1) * (2.0 * vxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def image_metrics(pred, target, crop=0, order="rows_first"):
    """pred, target: (H, W, 4) float32 r g b depth.  Returns (row, smap): the eight numbers of ngm_image_metrics' row and the
    per-window SSIM map (h - 10, w - 10, 3), or None where the cropped region has fewer than 11 rows or columns."""
    pred, target = np.asarray(pred), np.asarray(target)
    assert pred.dtype == np.float32 and target.dtype == np.float32 and pred.shape == target.shape and pred.shape[2] == 4
    H, W = pred.shape[:2]
    nan = float("nan")
    row = np.zeros(8, np.float64)
    # depth L1: the whole image, whatever the crop
    pd, td = pred[..., 3].astype(np.float64), target[..., 3].astype(np.float64)
    take = td != 0.0                                                        # NaN != 0 is true, -0.0 != 0 is false
    count = int(take.sum())
    with np.errstate(invalid="ignore"):
        row[2] = np.abs(pd[take] - td[take]).sum() / count if count else nan
    row[6] = count
    # PSNR and SSIM: the cropped region
    h, w = max(H - 2 * crop, 0), max(W - 2 * crop, 0)
    if h == 0 or w == 0:
        h = w = 0
    x = clamp01(pred[crop:crop + h, crop:crop + w, :3])
    y = clamp01(target[crop:crop + h, crop:crop + w, :3])
    terms = 3 * h * w
    row[4] = terms
    if terms:
        with np.errstate(divide="ignore", invalid="ignore"):
            d = x - y
            row[3] = (d * d).sum() / terms
            row[0] = 10.0 * np.log10(np.float64(1.0) / row[3])
    else:
        row[3] = row[0] = nan
    smap = None
    if h >= TAPS and w >= TAPS:
        smap = ssim_map(x, y, order)
        row[5] = smap.size
        row[1] = smap.sum() / smap.size
    else:
        row[1] = nan
    return row, smap


# ------------------------------------------------------------------------------------------------ scenes
def textured(h, w, seed, noise=0.02, depth_zero_every=0):
    """a pair of (h, w, 4) float32 frames: smooth colour patterns plus texture, the prediction = the target plus small noise;
    depth 1..4 m with a prediction off by centimetres; depth_zero_every = n > 0 sets the target depth to 0 on the lattice of
    every n-th row and column"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([0.5 + 0.4 * np.sin(xx / 5.0 + c) * np.cos(yy / 7.0 - c) for c in range(3)], -1)
    tex = rng.uniform(-0.1, 0.1, (h, w, 3))
    target = np.zeros((h, w, 4))
    target[..., :3] = base + tex
    target[..., 3] = 2.5 + 1.5 * np.sin(xx / 11.0) * np.sin(yy / 13.0)
    pred = target.copy()
    pred[..., :3] += rng.normal(0.0, noise, (h, w, 3))
    pred[..., 3] += rng.normal(0.0, 0.03, (h, w))
    if depth_zero_every:
        target[::depth_zero_every, ::depth_zero_every, 3] = 0.0
    return pred.astype(np.float32), target.astype(np.float32)


def beyond_range(h, w, seed):
    """colours drawn from uniform(-0.1, 1.1), independently for both frames: the clamp acts on a sixth of the values"""
    rng = np.random.default_rng(seed)
    pred = rng.uniform(-0.1, 1.1, (h, w, 4)).astype(np.float32)
    target = rng.uniform(-0.1, 1.1, (h, w, 4)).astype(np.float32)
    pred[..., 3] += 2.0
    target[..., 3] += 2.0
    return pred, target


def near_flat(h, w, seed):
    """a flat prediction of 0.7 against a target of 0.7 plus noise of 1e-3: the prediction's variance is 0, and in fp32
    E[x^2] - mu^2 is rounding noise of about 1e-7 around it, which the clamp at 0 turns into a bias"""
    rng = np.random.default_rng(seed)
    pred = np.full((h, w, 4), 0.7)
    target = np.full((h, w, 4), 0.7) + rng.normal(0.0, 1e-3, (h, w, 4))
    return pred.astype(np.float32), target.astype(np.float32)

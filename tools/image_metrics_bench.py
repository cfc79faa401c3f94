"""Scoring rendered frames on the device (evaluation.image_metrics: ngm_image_metrics, PSNR + SSIM + depth L1 in fp64, one call per
batch) against the reference's three functions written in torch on the device: clamp, crop and permute, the fp32 grouped-conv2d
SSIM as torchmetrics defines it, the masked mean for depth, and the three .item() calls the reference makes per frame.

    python tools/image_metrics_bench.py [--out profiles/r17_image_metrics.json] [--reps 5] [--poses 16] [--bench-json FILE]

One process; after one warm-up of every item the items are run in turn, `--reps` times, 20 calls between two device events (host
clock ending in a synchronise for the torch baseline, which synchronises by itself, and for the whole-frame items).  640 x 480,
crop 10, B = 1 and B = 16, on textured synthetic frames; then evaluate_frames over `--poses` poses of the room map of
tools/mesh_bench.py against render_image plus that baseline per frame, and the ssim difference between the two on those frames.
--bench-json merges a file holding bench.py's result lines of the parent commit and of this tree from the same box."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_iteration_bench import DEV, _write  # noqa: E402
from mesh_bench import make  # noqa: E402
from mesh_cull_bench import room_poses  # noqa: E402
from mesh_metrics_bench import device_ms, host_ms, shader_clock_under_load, summary  # noqa: E402
from neural_graph_mapping_amd import evaluation as Ev  # noqa: E402

H, W, CROP, INNER = 480, 640, 10, 20
# per window and channel: the horizontal pass (11 taps x (3 products + 5 fused multiply-adds), shared by the 16 rows of a tile out
# of 26 staged) and the vertical pass (11 x 5), counted as 2 flop per fused multiply-add, plus about 20 for the quotient
FLOP_PER_WINDOW = 11 * (3 + 2 * 5) * 26 / 16 + 11 * 2 * 5 + 20


def _prep(x, crop):
    x = x.clone()
    if crop > 0:
        x = x[crop:-crop, crop:-crop]
    return x.permute(2, 0, 1).unsqueeze(0).clamp_(0.0, 1.0)


_KERNEL = {}


def torch_ssim(prediction, target, crop):
    """evaluation.ssim with torchmetrics' structural_similarity_index_measure(data_range=1.0) written out (fp32, as it runs it)"""
    p, t = _prep(prediction, crop), _prep(target, crop)
    if p.device not in _KERNEL:
        dist = torch.arange((1 - 11) / 2, (1 + 11) / 2, 1, dtype=torch.float32, device=p.device)
        g = torch.exp(-torch.pow(dist / 1.5, 2) / 2)
        g = (g / g.sum()).unsqueeze(0)
        _KERNEL[p.device] = torch.matmul(g.t(), g).expand(3, 1, 11, 11).contiguous()
    p, t = F.pad(p, (5, 5, 5, 5), mode="reflect"), F.pad(t, (5, 5, 5, 5), mode="reflect")
    out = F.conv2d(torch.cat((p, t, p * p, t * t, p * t)), _KERNEL[p.device], groups=3)
    mp, mt, pp, tt, pt = out.split(1)
    vp, vt, vpt = torch.clamp(pp - mp * mp, min=0.0), torch.clamp(tt - mt * mt, min=0.0), pt - mp * mt
    full = ((2 * mp * mt + 1e-4) * (2 * vpt + 9e-4)) / ((mp * mp + mt * mt + 1e-4) * (vp + vt + 9e-4))
    return full[..., 5:-5, 5:-5].reshape(1, -1).mean(-1).mean().item()


def torch_psnr(prediction, target, crop):
    p, t = _prep(prediction, crop), _prep(target, crop)
    return (10.0 * torch.log10(1.0 / ((p - t) ** 2).mean())).item()


def torch_depthl1(prediction, target, crop):
    mask = target != 0
    return (prediction[mask] - target[mask]).abs().mean().item()


def torch_frame(rgbd, target, crop):
    """the three calls of _evaluate_frame (rm.py:1993-2004)"""
    return (torch_psnr(rgbd[:, :, :3], target[:, :, :3], crop), torch_ssim(rgbd[:, :, :3], target[:, :, :3], crop),
            torch_depthl1(rgbd[:, :, 3], target[:, :, 3], crop))


def frames(b, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(xx / 5 + c) * torch.cos(yy / 7 - c) for c in range(3)] + [2.5 + 1.5 * torch.sin(xx / 11) * torch.sin(yy / 13)], -1)
    target = base[None] + torch.cat([0.1 * (2 * torch.rand(b, H, W, 3, device=DEV, generator=g) - 1), torch.zeros(b, H, W, 1, device=DEV)], -1)
    pred = target + 0.02 * torch.randn(b, H, W, 4, device=DEV, generator=g)
    target[:, ::7, ::7, 3] = 0.0
    return pred.contiguous(), target.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--bench-json", default=None, help="bench.py's result lines of the parent commit and this tree, same box")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "image_metrics_bench needs the MI355X: there is no CPU fallback to time"
    p1, t1 = frames(1, 1)
    p16, t16 = frames(16, 2)
    dev_rows = torch.ops.ngm355.image_metrics(p16, t16, CROP).cpu().numpy()
    base_rows = np.array([torch_frame(p16[i], t16[i], CROP) for i in range(16)])
    agreement = dict(worst_psnr_difference=float(np.abs(dev_rows[:, 0] - base_rows[:, 0]).max()),
                     worst_ssim_difference=float(np.abs(dev_rows[:, 1] - base_rows[:, 1]).max()),
                     worst_depthl1_difference=float(np.abs(dev_rows[:, 2] - base_rows[:, 2]).max()))
    print(json.dumps(dict(stage="agreement on the synthetic frames (device fp64 against the fp32 baseline)", **agreement)), flush=True)

    r = make("m1_fourier")
    cam = r._camera
    poses = room_poses(a.poses)
    r.eval()
    targets = [r.render_image(poses[i], seed=1)[0] + 0.02 * torch.randn(cam.height, cam.width, 4, device=DEV) for i in range(a.poses)]
    r.train()

    def baseline_frames():
        out = []
        for i in range(a.poses):
            r.eval()
            rgbd, _ = r.render_image(poses[i], seed=0)
            out.append(torch_frame(rgbd, targets[i], CROP))
            r.train()
        return out

    def render_only():
        r.eval()
        for i in range(a.poses):
            r.render_image(poses[i], seed=0)
        r.train()

    metrics = ["psnr", "ssim", "depthl1"]
    _, per_frame = r.evaluate_frames(poses, targets, metrics=metrics, crop=CROP)
    rendered = dict(ssim_device=[float(v) for v in per_frame[:, 1]], ssim_fp32_baseline=[v[1] for v in baseline_frames()])
    rendered["worst_ssim_difference"] = float(np.abs(np.array(rendered["ssim_device"]) - np.array(rendered["ssim_fp32_baseline"])).max())
    print(json.dumps(dict(stage="ssim on the rendered frames", worst_difference=rendered["worst_ssim_difference"])), flush=True)

    items = {
        "device/B1": lambda: device_ms(lambda: torch.ops.ngm355.image_metrics(p1, t1, CROP), INNER)[0],
        "device/B16": lambda: device_ms(lambda: torch.ops.ngm355.image_metrics(p16, t16, CROP), INNER)[0],
        "torch_baseline/B1": lambda: host_ms(lambda: torch_frame(p1[0], t1[0], CROP), INNER)[0],
        "torch_baseline/B16": lambda: host_ms(lambda: [torch_frame(p16[i], t16[i], CROP) for i in range(16)], INNER)[0],
        "frames/evaluate_frames": lambda: host_ms(lambda: r.evaluate_frames(poses, targets, metrics=metrics, crop=CROP))[0],
        "frames/render_image_plus_torch_baseline": lambda: host_ms(baseline_frames)[0],
        "frames/render_image_alone": lambda: host_ms(render_only)[0],
    }
    times = {k: [] for k in items}
    for k, fn in items.items():
        fn()
        print(json.dumps(dict(stage="warm-up", item=k)), flush=True)
    for rep in range(a.reps):
        for k, fn in items.items():
            times[k].append(fn())
        print(json.dumps(dict(stage="repeat", n=rep, **{k: round(v[-1], 4) for k, v in times.items()})), flush=True)
    sclk = shader_clock_under_load(lambda: torch.ops.ngm355.image_metrics(p16, t16, CROP), n=200)
    out_times = {k: summary(v) for k, v in times.items()}
    med = {k: v["median_ms"] for k, v in out_times.items()}
    windows = 3 * (H - 2 * CROP - 10) * (W - 2 * CROP - 10)
    per_frame_ms = med["device/B16"] / 16
    render = med["frames/render_image_alone"]
    derived = dict(
        device_below_baseline_in_every_repeat=all(d < t for b in ("B1", "B16") for d, t in zip(times["device/" + b], times["torch_baseline/" + b])),
        us_per_frame_B1=round(1e3 * med["device/B1"], 2), us_per_frame_B16=round(1e3 * per_frame_ms, 2),
        gb_per_s_against_the_9_8_mb_it_must_read_B16=round(2 * H * W * 16 / (per_frame_ms * 1e-3) / 1e9, 1),
        fp64_gflop_per_s_B16=round(windows * FLOP_PER_WINDOW / (per_frame_ms * 1e-3) / 1e9, 1),
        flop_per_frame_counted=int(windows * FLOP_PER_WINDOW),
        speedup_B1=round(med["torch_baseline/B1"] / med["device/B1"], 1), speedup_B16=round(med["torch_baseline/B16"] / med["device/B16"], 1),
        frames_below_baseline_in_every_repeat=all(d < t for d, t in zip(times["frames/evaluate_frames"], times["frames/render_image_plus_torch_baseline"])),
        metrics_share_of_frame_time_device=round(max(med["frames/evaluate_frames"] - render, 0.0) / med["frames/evaluate_frames"], 4),
        metrics_share_of_frame_time_baseline=round(max(med["frames/render_image_plus_torch_baseline"] - render, 0.0) / med["frames/render_image_plus_torch_baseline"], 4))
    out = dict(tool="tools/image_metrics_bench.py",
               command=f"python tools/image_metrics_bench.py --out <file> --reps {a.reps} --poses {a.poses}" + (" --bench-json <bench.py lines>" if a.bench_json else ""),
               device=torch.cuda.get_device_name(0), torch=torch.__version__, sclk_mhz=sclk,
               workload=f"{W} x {H} frames, crop {CROP}, B = 1 and B = 16, textured synthetic frames; frames/*: {a.poses} poses inside the room map of "
                        f"tools/mesh_bench.py (m1_fourier, 200 fields) at {cam.width} x {cam.height}, targets = another draw of the same render plus noise",
               procedure=f"one process, one warm-up of every item, then the items in turn, {a.reps} repeats; device/*: ms per CALL between two device events "
                         f"around {INNER} calls of the op (workspace and output allocation included); torch_baseline/*: ms per call by the host clock around "
                         f"{INNER} calls (B16: 16 frames in turn, three .item() each) and a synchronise; frames/*: host clock around the {a.poses} frames, "
                         "one synchronise at the end; the shares subtract render_image alone",
               agreement_synthetic=agreement, rendered_frames=rendered, times=out_times, derived=derived)
    if a.bench_json and os.path.exists(a.bench_json):
        out["bench_py_parent_and_this_tree_same_box"] = json.load(open(a.bench_json))
    _write(a.out, out)
    print(json.dumps(dict(times=med, derived=derived, agreement=agreement, sclk_mhz=sclk)), flush=True)


if __name__ == "__main__":
    main()

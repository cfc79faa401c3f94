"""CPU-side checks of the device training-target sampler's boundary (include/ngm_hip.h ngm_target_sample_mv): symbols
declared and exported, the parameter struct's layout, the custom op's registration and fake shapes, the host-side
validators, and the host restatement's float32 stand-ins for log / sin / cos.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngm_hip.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from neural_graph_mapping_amd import _capi, build
    if not os.path.exists(_capi.LIB_PATH):
        build.build(verbose=False)
    return _capi


def test_symbols_declared_and_exported(capi):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = capi.lib()
    for n in ("ngm_target_sample_mv_workspace", "ngm_target_sample_mv"):
        assert re.search(rf"\b{n}\s*\(", src), n
        assert n in capi.EXPORTED and hasattr(L, n), n
    assert int(re.search(r"#define\s+NGM_TARGET_MAX_DRAW\s+(\d+)", src).group(1)) == capi.NGM_TARGET_MAX_DRAW
    # the planner sizes the workspace without a device; bad sizes give -1
    assert L.ngm_target_sample_mv_workspace(100, 30, 200, 32) > 0
    assert L.ngm_target_sample_mv_workspace(3000, 30, 200, 32) > L.ngm_target_sample_mv_workspace(100, 30, 200, 32)
    assert L.ngm_target_sample_mv_workspace(0, 30, 200, 32) == -1
    assert L.ngm_target_sample_mv_workspace(10, 30, 200, capi.NGM_TARGET_MAX_DRAW + 1) == -1


def test_struct_layout_matches_header(capi, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ngm_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n",'
                   "sizeof(ngm_target_sample),offsetof(ngm_target_sample,seed),offsetof(ngm_target_sample,iteration_dev),"
                   "offsetof(ngm_target_sample,u_xy));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    T = capi.TargetSample
    assert sizes == [C.sizeof(T), T.seed.offset, T.iteration_dev.offset, T.u_xy.offset]


def test_op_registered_with_fake_shapes_and_no_cpu_kernel(capi):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from neural_graph_mapping_amd import ops
    op = torch.ops.ngm355.target_sample_mv
    assert "Tensor(a5!)? iteration_dev" in str(op.default._schema)          # declared as mutating the counter
    args = lambda dev: (torch.zeros(5, dtype=torch.int64, device=dev), torch.zeros(6, 4, 4, device=dev),
                        torch.zeros(8, 48, 64, 4, device=dev), torch.zeros(6, dtype=torch.int64, device=dev),
                        torch.zeros(12, 3, device=dev), None, [1.0, 1.0, 0.0, 0.0], 1.0)
    with pytest.raises(NotImplementedError):                                  # dispatcher: no CPU kernel
        op(*args("cpu"), 12, 8, 16, 0, 0, 1, 0)
    with FakeTensorMode(allow_non_fake_inputs=True):
        out = op(*args("cuda"), 12, 8, 16, 0, 0, 1, 0)
        shapes = {k: tuple(v.shape) for k, v in zip(ops.TARGET_SAMPLE_MV_OUT, out)}
        assert shapes["ijs"] == (8, 16, 2) and shapes["c2ws"] == (8, 16, 4, 4) and shapes["field_ids"] == (8,)
        assert shapes["count"] == (1,) and shapes["subset_observed"] == (4,) and shapes["subset_random"] == (4,)
        assert shapes["offsets"] == (20, 3) and shapes["frame_cids"] == (8, 16) and shapes["u_xy"] == (8, 16, 2)
        assert out[ops.TARGET_SAMPLE_MV_OUT.index("rgb_mask")].dtype == torch.bool
        assert out[ops.TARGET_SAMPLE_MV_OUT.index("count")].dtype == torch.int32
        out = op(*args("cuda"), 12, 8, 16, 0, 0, 3, 1)                        # rank 1 of 3: ids 1, 4, 7, 10 -> 4 rows
        assert tuple(out[0].shape) == (4, 16, 2) and tuple(out[ops.TARGET_SAMPLE_MV_OUT.index("subset_random")].shape) == (4,)


def test_plan(capi):
    P = capi.target_sample_mv_plan
    assert P(5, 12, 8, 16) == (4, 4, 8)
    assert P(12, 12, 32, 8) == (12, 0, 12)                 # n_rand == 0
    assert P(0, 50, 16, 8) == (0, 16, 16)                  # no current fields
    assert P(4, 10, 32, 8) == (4, 6, 10)                   # num_fields < num_train_fields
    assert P(30, 200, 32, 8, world_size=3, rank=2) == (16, 16, 32)
    assert P(30, 40, 32, 8, world_size=3, rank=2) == (16, 16, 13)


def test_validators_raise_before_launch(capi):
    from neural_graph_mapping_amd import ops
    good = dict(current_field_ids=torch.zeros(5, dtype=torch.int64), c2ws=torch.zeros(6, 4, 4), rgbd_store=torch.zeros(8, 48, 64, 4),
                frame_to_store=torch.zeros(6, dtype=torch.int64), field_positions=torch.zeros(12, 3))

    def call(**kw):
        a = dict(good)
        rest = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, radius=1.0, num_fields=12, num_train_fields=8, num_rays_per_field=16, iteration=0)
        for k in list(kw):
            (a if k in a else rest)[k] = kw[k]
        return ops.target_sample_mv(**a, **rest)
    with pytest.raises(ValueError, match="num_rays_per_field"):
        call(num_rays_per_field=0)
    with pytest.raises(TypeError, match="current_field_ids"):
        call(current_field_ids=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(TypeError, match="field_positions"):
        call(field_positions=torch.zeros(12, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="c2ws"):
        call(c2ws=torch.zeros(6, 3, 4))
    with pytest.raises(ValueError, match="frame_to_store"):
        call(frame_to_store=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="field_positions"):
        call(num_fields=13)
    with pytest.raises(ValueError, match="rank"):
        call(world_size=2, rank=2)
    with pytest.raises(ValueError, match="at most"):
        capi.target_sample_mv_plan(5, 100000, 10000, 16)
    with pytest.raises(ValueError, match="iteration_dev"):
        call(iteration=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):               # valid input, but no device tensors
        call()


def test_host_stand_ins_are_accurate():
    """tests/_target_device_host.py restates the kernel's exact-rounding log / sincos: close to the true functions"""
    import _target_device_host as H
    u = ((np.arange(1, 1 << 16, dtype=np.uint64) * np.uint64(255)) * np.uint64(2) + np.uint64(1)).astype(np.float32) / np.float32(1 << 24)
    assert np.abs(H.log_f32(u) - np.log(u.astype(np.float64))).max() < 2e-6
    v = np.arange(1 << 16, dtype=np.float32) / np.float32(1 << 16)
    s, c = H.sincos_2pi_f32(v)
    assert np.abs(s - np.sin(2 * np.pi * v.astype(np.float64))).max() < 1e-6
    assert np.abs(c - np.cos(2 * np.pi * v.astype(np.float64))).max() < 1e-6
    off = H.offsets(0, 0)
    assert off.shape == (20, 3) and np.abs(np.linalg.norm(off.astype(np.float64), axis=1) - 1).max() < 1e-6

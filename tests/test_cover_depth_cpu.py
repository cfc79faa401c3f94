"""ngm_cover_depth without a GPU: the host mirror against the fixture recorded from the real reference, against the reference
itself where it is present, the C struct, the op's registration, the argument refusals, and -- the point of a yardstick --
the checker the GPU test uses rejecting seven faulty restatements (tests/_cover_host.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import _cover_host as CH  # noqa: E402
from _ref_import import reference_available  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "g30_cover_depth.npz")
RADII = (1.0, 0.25)


@pytest.fixture(scope="module")
def g30():
    return dict(np.load(FIXTURE))


@pytest.fixture(scope="module")
def capi():
    from neural_graph_mapping_amd import _capi, build
    if not os.path.exists(_capi.LIB_PATH):
        build.build(verbose=False)
    return _capi


def fixture_calls(g):
    """the two recorded calls as keyword dictionaries for the mirror, and the positions the reference added in each"""
    K, n0, n1 = tuple(g["intrinsics"]), int(g["num0"]), int(g["num1"])
    first = dict(depth=g["depth0"], c2w=g["c2w0"], K=K, shift=g["shift0"], radius=float(g["radius"]))
    second = dict(depth=g["depth1"], c2w=g["c2w1"], K=K, shift=g["shift1"], radius=float(g["radius"]), positions=g["positions"][:n0])
    return (first, g["positions"][:n0]), (second, g["positions"][n0:n1])


def test_the_mirror_reproduces_the_fixture(g30):
    """same cells, same order, positions bit for bit; no pixel of the fixture is ambiguous, so nothing is optional"""
    for call, want in fixture_calls(g30):
        cls = CH.classify(**call)
        assert cls["ambiguous_pixels"] == 0 and cls["ambiguous_centres"] == 0 and not cls["optional"]
        cells = sorted(cls["required"])
        assert CH.emit(cells, call["shift"], cls["cell"]).tobytes() == want.tobytes()
        pos, counts = CH.cover_fp32(**call)
        assert pos.tobytes() == want.tobytes() and counts[:2] == [len(want), 0]
        CH.check(cls, pos, counts)
    n0, n1 = int(g30["num0"]), int(g30["num1"])
    assert n0 > 0 and n1 > n0
    assert g30["kf_ids"].tolist() == [3] * n0 + [8] * (n1 - n0)
    assert g30["kf2fields_3"].tolist() == list(range(n0)) and g30["kf2fields_8"].tolist() == list(range(n0, n1))
    assert np.array_equal(g30["orientations"], np.tile(np.float32([1, 0, 0, 0]), (n1, 1)))
    # the second call exercises both filters: some pixels are covered, and an active centre's cell holds uncovered points
    second, _ = fixture_calls(g30)[1]
    _, counts = CH.cover_fp32(**second)
    assert 0 < counts[2] < counts[3]
    assert len(CH.cover_fp32(**second, fault="no_occupied_filter")[0]) > n1 - n0


@pytest.mark.skipif(not reference_available(), reason="the reference is not present")
def test_the_mirror_agrees_with_the_real_reference():
    """a handful of random scenes without an ambiguous pixel: NeuralGraphMap._extend_global_map_dict itself, on the CPU"""
    import math
    from _ref_import import build_map, import_reference, make_config
    rm, _, camera, _, _, _ = import_reference()

    def ball_query(p1, p2, K=1, radius=0.2, return_nn=False, **kw):     # public definition, K = 1
        d = p1[0, :, None, :] - p2[0, None, :, :]
        hit = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) < radius * radius
        return None, torch.where(hit.any(-1), hit.float().argmax(-1), torch.full((p1.shape[1],), -1))[None, :, None], None
    rm.ball_query = ball_query
    done = 0
    for seed in range(40):
        radius = RADII[seed % 2]
        case = CH.sweep_case(seed, radius, 24, 32)
        cell = 2 * radius / math.sqrt(3)
        torch.manual_seed(seed)
        shift = torch.empty(3).uniform_(0.0, cell).numpy()
        active = case["positions"][case["field_ids"]]
        cls = CH.classify(case["depth"], case["c2w"], case["K"], shift, radius, active)
        if cls["ambiguous_pixels"] or cls["ambiguous_centres"]:
            continue
        ngm = build_map(rm, make_config(field_radius=radius), 0, torch.zeros(0, 3), torch.zeros(0, 4))
        ngm._optim_state = None
        ngm._bb_min, ngm._bb_max = torch.full((3,), torch.inf), torch.full((3,), -torch.inf)
        K = case["K"]
        cam = camera.Camera(width=32, height=24, fx=K[0], fy=K[1], cx=K[2], cy=K[3], pixel_center=0.0)
        torch.manual_seed(seed)
        ngm._extend_global_map_dict(torch.from_numpy(case["depth"]), 5, torch.from_numpy(case["c2w"]), cam,
                                    {"positions": torch.from_numpy(active)})
        n = ngm._global_map_dict["num"]
        got = ngm._global_map_dict["positions"][:n].numpy()
        assert got.tobytes() == CH.emit(sorted(cls["required"]), shift, cls["cell"]).tobytes(), seed
        assert got.tobytes() == CH.cover_fp32(case["depth"], case["c2w"], K, shift, radius, active)[0].tobytes(), seed
        done += 1
        if done == 6:
            break
    assert done >= 4


def test_struct_size_matches_the_header(capi, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ngm_hip.h"\nint main(){printf("%zu %zu %zu %zu %d\\n",'
                   "sizeof(ngm_cover_depth_args),offsetof(ngm_cover_depth_args,pixel_stride),offsetof(ngm_cover_depth_args,fx),"
                   "offsetof(ngm_cover_depth_args,cell),NGM_COVER_MAX_NEW);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_stride, o_fx, o_cell, max_new = (int(x) for x in subprocess.check_output([str(exe)]).split())
    A = capi.CoverDepthArgs
    assert (size, o_stride, o_fx, o_cell) == (C.sizeof(A), A.pixel_stride.offset, A.fx.offset, A.cell.offset)
    assert max_new == capi.NGM_COVER_MAX_NEW
    assert {"ngm_cover_depth", "ngm_cover_depth_workspace"} <= set(capi.EXPORTED)


def test_op_is_registered_without_a_cpu_kernel():
    from neural_graph_mapping_amd import ops
    assert hasattr(torch.ops.ngm355, "cover_depth")
    depth, c2w, shift = torch.ones(4, 5), torch.eye(4), torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cover_depth(depth, c2w, shift, None, 1.0, 5.0, 5.0, 2.0, 1.5, 8)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.ngm355.cover_depth(depth, c2w, shift, None, None, 0, [5.0, 5.0, 2.0, 1.5], 1.0, 1.0, 8)
    # the fake registration gives the shapes
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        pos, counts = torch.ops.ngm355.cover_depth(torch.empty(4, 5), torch.empty(4, 4), torch.empty(3), None, None, 0,
                                                   [5.0, 5.0, 2.0, 1.5], 1.0, 1.0, 8)
    assert tuple(pos.shape) == (8, 3) and pos.dtype == torch.float32 and tuple(counts.shape) == (4,) and counts.dtype == torch.int32
    assert ops.cover_cell(1.0) == CH.cell_of(1.0) and ops.cover_cell(0.25) == CH.cell_of(0.25)


def test_argument_refusals_hold_without_a_device(capi):
    """every refusal comes before the first launch, so fake addresses are never dereferenced"""
    L = capi.lib()
    P = 0x1000

    def args(**kw):
        a = capi.CoverDepthArgs(P, P, P, P, None, P, P, 1, 10, 10, 48, 64, 16, 50.0, 50.0, 31.5, 23.5, 1.0, CH.cell_of(1.0))
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def call(a, ws=P, nbytes=1 << 40):
        return L.ngm_cover_depth(C.byref(a), ws, nbytes, None)
    E = capi
    assert L.ngm_cover_depth(None, P, 1 << 40, None) == E.NGM_E_INVALID
    for name in ("depth", "c2w", "shift", "new_positions", "counts"):
        assert call(args(**{name: None})) == E.NGM_E_INVALID, name
    assert call(args(), ws=None) == E.NGM_E_INVALID
    assert call(args(field_positions=None)) == E.NGM_E_INVALID                # active fields without a table
    assert call(args(num_active=11)) == E.NGM_E_INVALID                        # more than rows, no id list
    assert call(args(height=1 << 16, width=1 << 15)) == E.NGM_E_INVALID        # H W = 2^31
    assert call(args(height=0)) == E.NGM_E_INVALID and call(args(width=-1)) == E.NGM_E_INVALID
    assert call(args(pixel_stride=0)) == E.NGM_E_INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(args(radius=bad)) == E.NGM_E_INVALID, bad
        assert call(args(cell=bad)) == E.NGM_E_INVALID, bad
    assert call(args(max_new=0)) == E.NGM_E_INVALID
    assert call(args(max_new=E.NGM_COVER_MAX_NEW + 1)) == E.NGM_E_UNSUPPORTED
    need = L.ngm_cover_depth_workspace(48, 64, 10, 16)
    assert need > 2 * 48 * 64 * 8
    assert call(args(), nbytes=need - 1) == E.NGM_E_WORKSPACE
    assert L.ngm_cover_depth_workspace(1 << 16, 1 << 15, 0, 16) == E.NGM_E_INVALID
    assert L.ngm_cover_depth_workspace(48, 64, 0, 0) == E.NGM_E_INVALID
    assert L.ngm_cover_depth_workspace(48, 64, 0, E.NGM_COVER_MAX_NEW + 1) == E.NGM_E_UNSUPPORTED
    assert L.ngm_cover_depth_workspace(48, 64, 0, E.NGM_COVER_MAX_NEW) > 0
    assert L.ngm_abi_version() == 11


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick can fail
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    """the scenes of the GPU sweep with their classification (12 per radius are enough here)"""
    out = []
    for radius in RADII:
        for seed in range(12):
            case = CH.sweep_case(seed, radius)
            cls = CH.classify(case["depth"], case["c2w"], case["K"], case["shift"], radius, case["positions"], case["field_ids"])
            out.append((case, cls))
    return out


def _run(case, fault=None):
    return CH.cover_fp32(case["depth"], case["c2w"], case["K"], case["shift"], case["radius"], case["positions"], case["field_ids"],
                         fault=fault)


def test_the_checker_accepts_the_faultless_restatement(sweep, g30):
    for case, cls in sweep:
        CH.check(cls, *_run(case))
    optional = sum(len(c["optional"]) for _, c in sweep)
    total = optional + sum(len(c["required"]) for _, c in sweep)
    assert total > 500 and optional <= 0.01 * total, (optional, total)


@pytest.mark.parametrize("fault", CH.FAULTS)
def test_the_checker_rejects_a_single_fault(sweep, g30, fault):
    """each faulty restatement is rejected on the fixture or on a sweep scene -- and on most of them, not by luck on one"""
    rejected = 0
    calls = [(dict(depth=c["depth"], c2w=c["c2w"], K=c["K"], shift=c["shift"], radius=c["radius"], positions=c.get("positions")), None)
             for c, _ in fixture_calls(g30)]
    for call, _ in calls:
        cls = CH.classify(**call)
        try:
            CH.check(cls, *CH.cover_fp32(**call, fault=fault))
        except AssertionError:
            rejected += 1
    for case, cls in sweep:
        try:
            CH.check(cls, *_run(case, fault))
        except AssertionError:
            rejected += 1
    assert rejected >= (len(sweep) + 2) // 2, f"{fault}: rejected on {rejected} of {len(sweep) + 2} scenes"

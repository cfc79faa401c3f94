"""CPU-side checks of the drop-in boundary: the C-ABI library builds/loads, exports every symbol
include/ngm_hip.h declares, struct layouts agree, and the product path refuses to run without a GPU
(no silent CPU fallback).  No compute calls here."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngm_hip.h")


@pytest.fixture(scope="module")
def capi():
    from neural_graph_mapping_amd import _capi, build
    if not os.path.exists(_capi.LIB_PATH):
        build.build(verbose=False)
    return _capi


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ngm_[a-z_0-9]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(capi):
    L = capi.lib()
    names = declared_functions()
    assert len(names) >= 15
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/ngm_hip.h but not exported"
    assert sorted(capi.EXPORTED) == names
    want = int(re.search(r"#define\s+NGM_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert L.ngm_abi_version() == want == 11
    L.ngm_peer_set_timeout.restype, L.ngm_peer_set_timeout.argtypes = C.c_double, [C.c_double]
    prev = L.ngm_peer_set_timeout(5.0)
    assert prev > 0 and L.ngm_peer_set_timeout(prev) == 5.0 and L.ngm_peer_set_timeout(0.0) == prev     # <= 0 only reads


def test_struct_layouts_match_header(capi, tmp_path):
    """Compile a tiny C program against the header and compare sizeof() with the ctypes mirrors."""
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "ngm_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n",'
                   "sizeof(ngm_field_cfg),sizeof(ngm_params),sizeof(ngm_grads),sizeof(ngm_render_cfg),"
                   "sizeof(ngm_rays),sizeof(ngm_targets),sizeof(ngm_prediction));"
                   "printf(\" %zu %zu %zu\\n\",sizeof(ngm_keyframes),sizeof(ngm_target_out),sizeof(ngm_adam_tensor));return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    mirrors = [capi.FieldCfg, capi.Params, capi.Grads, capi.RenderCfg, capi.Rays, capi.Targets, capi.Prediction,
               capi.Keyframes, capi.TargetOut, capi.AdamTensor]
    assert sizes == [C.sizeof(m) for m in mirrors]


def test_integration_md_level3_snippet_matches_the_library(capi, tmp_path):
    """INTEGRATION.md's Level-3 ctypes stub is what a reference maintainer would paste: EXECUTE its fenced block (the real
    library substituted for the bare file name) and compare the struct definitions printed there with the C structs --
    sizeof from a C program compiled against include/ngm_hip.h, every field offset against the _capi mirrors.  (Round 4's
    page had a FieldCfg 8 bytes short of ngm_field_cfg: the library would have read two ints past the caller's struct.)"""
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", md, flags=re.S)
    snippet = [b for b in blocks if "class FieldCfg(C.Structure)" in b]
    assert len(snippet) == 1
    code = snippet[0].replace('C.CDLL("libngm_hip.so")', f"C.CDLL({capi.LIB_PATH!r})")
    assert code != snippet[0]
    ns = {}
    exec(compile(code, "INTEGRATION.md:Level-3", "exec"), ns)          # defines lib, FieldCfg, Params, field_set_forward
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ngm_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n",'
                   "sizeof(ngm_field_cfg),sizeof(ngm_params),offsetof(ngm_field_cfg,tri_mode),offsetof(ngm_params,neus_sd_stride));"
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sz_fc, sz_p, off_tri, off_neus = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(ns["FieldCfg"]) == sz_fc == 276
    assert C.sizeof(ns["Params"]) == sz_p
    assert ns["FieldCfg"].tri_mode.offset == off_tri and ns["Params"].neus_sd_stride.offset == off_neus
    for doc, mirror in ((ns["FieldCfg"], capi.FieldCfg), (ns["Params"], capi.Params)):
        assert [(n, getattr(doc, n).offset, getattr(doc, n).size) for n, _ in doc._fields_] == \
               [(n, getattr(mirror, n).offset, getattr(mirror, n).size) for n, _ in mirror._fields_]
    assert callable(ns["field_set_forward"]) and ns["lib"].ngm_abi_version() == capi.lib().ngm_abi_version()
    # no stale "not built" statements about the loss modes on the page or in the header
    assert "and are not built" not in md and "are NOT built" not in open(HEADER).read()


def test_workspace_sizing_and_validation_without_gpu(capi):
    L = capi.lib()
    fc = capi.field_cfg(encoding="fourier", dim_enc=64, num_layers=2)
    rc = capi.render_cfg(num_samples_coarse=64, num_samples_guided=64)
    ws = L.ngm_render_workspace(C.byref(fc), C.byref(rc), 8, 512, 1)
    # stash: 24 B / sample + ray table + partial gradient vectors
    assert ws > 8 * 512 * 128 * 24
    assert L.ngm_render_workspace(C.byref(fc), C.byref(rc), 8, 512, 0) < 4096
    bad = capi.field_cfg(encoding="fourier", dim_enc=64, num_layers=2, dim_out=3)
    assert L.ngm_render_workspace(C.byref(bad), C.byref(rc), 8, 512, 1) < 0
    assert b"dim_out" in L.ngm_last_error()
    # argument validation happens before any launch
    assert L.ngm_field_eval_fwd(C.byref(fc), None, 1, 10, None, None, None, None, None) == -1


def test_workspace_boundary_without_a_device(capi):
    """One byte short of what the size query reports is refused as too small; the reported size gets past that check, to a later
    refusal that launches nothing either (no pointer below is ever read)."""
    L, fake = capi.lib(), 0x1000
    WS, INV, UNS = capi.NGM_E_WORKSPACE, capi.NGM_E_INVALID, capi.NGM_E_UNSUPPORTED
    err = lambda: L.ngm_last_error().decode()

    def params(fc):
        ptrs = {n: fake for n in capi.param_shapes(fc)}
        return capi.params_struct(fc, ptrs, {n: 1 for n in ptrs}, None, 0)

    # marching cubes: the count without `counts`, the emit without `verts`
    need = L.ngm_marching_cubes_workspace(5, 4, 3)
    assert need > 0
    assert L.ngm_marching_cubes_count(fake, 5, 4, 3, 0.0, None, fake, need - 1, None) == WS and "too small" in err()
    assert L.ngm_marching_cubes_count(fake, 5, 4, 3, 0.0, None, fake, need, None) == INV
    assert L.ngm_marching_cubes_emit(fake, 5, 4, 3, 0.0, None, 1, fake, 1, fake, need - 1, None) == WS and "too small" in err()
    assert L.ngm_marching_cubes_emit(fake, 5, 4, 3, 0.0, None, 1, fake, 1, fake, need, None) == INV
    # kNN evaluation of points: P * K = 2^31 pairs are refused as unsupported, after the workspace
    fc = capi.field_cfg(encoding="nerf", num_octaves=2, num_layers=1, dim_hidden=16)
    ps = params(fc)
    NF, P, K_ = 7, 2 ** 30, 2
    need = L.ngm_field_eval_knn_workspace(NF, P, K_)
    knn = lambda wsb: L.ngm_field_eval_knn(C.byref(fc), C.byref(ps), NF, P, fake, fake, fake, K_, 10.0, 1.0, 0.0, fake, fake, wsb, None)
    assert need > 0 and knn(need - 1) == WS and err() == "ngm_field_eval_knn: workspace too small"
    assert knn(need) == UNS
    # the standalone encoding backward (Fourier partials, permutohedral scratch) without the gradient tensor
    gr = capi.Grads()
    F, P = 3, 257
    for enc, why in ((dict(encoding="fourier", dim_enc=64, num_layers=2), "enc_w is NULL"), (dict(encoding="permuto", num_layers=1), "lattice is NULL")):
        fc = capi.field_cfg(**enc)
        ps = params(fc)
        need = L.ngm_encode_bwd_workspace(C.byref(fc), F, P)
        enc_bwd = lambda wsb: L.ngm_encode_bwd(C.byref(fc), C.byref(ps), F, P, fake, fake, fake, fake, C.byref(gr), fake, wsb, None)
        assert need > 256 and enc_bwd(need - 1) == WS and err() == "ngm_encode_bwd: workspace too small", enc
        assert enc_bwd(need) == INV and why in err(), (enc, err())
    # the point-mode backward (partials, then the encoding's scratch) without the encoding's gradient tensor
    for enc, why in ((dict(encoding="permuto", num_layers=1), "lattice is NULL"),
                     (dict(encoding="triplane", num_layers=1, resolution=16, num_components=32), "planes missing")):
        fc = capi.field_cfg(**enc)
        ps = params(fc)
        need = L.ngm_field_eval_bwd_workspace(C.byref(fc), F, P)
        bwd = lambda wsb: L.ngm_field_eval_bwd(C.byref(fc), C.byref(ps), F, P, fake, fake, fake, fake, C.byref(gr), fake, wsb, None)
        assert need > 256 and bwd(need - 1) == WS and err() == "workspace too small", enc
        assert bwd(need) == INV and why in err(), (enc, err())
    # its stash: one byte short is the stash's refusal, the reported size reaches the workspace's
    fc = capi.field_cfg(encoding="fourier", dim_enc=64, num_layers=2, matmul_mode="auto")
    ps = params(fc)
    sb, wsb = L.ngm_field_eval_stash_bytes(C.byref(fc), F, P), L.ngm_field_eval_bwd_workspace(C.byref(fc), F, P)
    stash_bwd = lambda s, w: L.ngm_field_eval_bwd_stash(C.byref(fc), C.byref(ps), F, P, fake, fake, fake, fake, C.byref(gr), fake, s, fake, w, None)
    assert sb > 256 and stash_bwd(sb - 1, wsb) == WS and err() == "ngm_field_eval_bwd_stash: stash too small"
    assert stash_bwd(sb, wsb - 1) == WS and err() == "workspace too small"
    # the fused backward, every wrapper of it (loss, counted, Adam, counted Adam, seeded, seeded with variances): a
    # permutohedral network without the table's gradient tensor
    fc, rc = capi.field_cfg(encoding="permuto", num_layers=1), capi.render_cfg(num_samples_coarse=9, num_samples_guided=5)
    ps, fp = params(fc), C.cast(fake, capi.f32p)
    rays = capi.Rays()
    rays.F, rays.R, rays.ijs, rays.c2ws, rays.gt, rays.field_pos, rays.field_quat = 3, 41, fake, fp, fp, fp, fp
    tg, pred = capi.Targets(fp, fake, None, None), capi.Prediction(fp, None, None, fp)
    at = capi.AdamTensor(fp, fp, fp, fp, 1, 1, 1)
    head = (C.byref(fc), C.byref(rc), C.byref(ps), C.byref(rays))
    loss = head + (C.byref(tg), C.byref(pred), None, C.byref(gr))
    adam = loss + (C.byref(at), 1, C.byref(at), None, 1, None, 1e-3, 0.9, 0.999, 1e-15, 0.0)
    need = L.ngm_render_workspace(C.byref(fc), C.byref(rc), rays.F, rays.R, 1)
    wrappers = {
        "ngm_render_bwd": lambda w: L.ngm_render_bwd(*loss, None, fake, w, None),
        "ngm_render_bwd_counted": lambda w: L.ngm_render_bwd_counted(*loss, None, fake, w, None, fake),
        "ngm_render_bwd_adam": lambda w: L.ngm_render_bwd_adam(*adam, None, fake, w, None),
        "ngm_render_bwd_adam_counted": lambda w: L.ngm_render_bwd_adam_counted(*adam, None, fake, w, None, fake),
        "ngm_render_bwd_seeded": lambda w: L.ngm_render_bwd_seeded(*head, fake, None, None, C.byref(gr), fake, w, None),
        "ngm_render_bwd_seeded_vars": lambda w: L.ngm_render_bwd_seeded_vars(*head, C.byref(pred), fake, fake, None, None, None,
                                                                             C.byref(gr), fake, w, None),
    }
    assert need > 4096
    for name, call in wrappers.items():
        assert call(need - 1) == WS and err() == "render_bwd: workspace too small", name
        assert call(need) == INV and err() == "permutohedral: grads.lattice is NULL", (name, err())


def test_param_names_and_shapes_follow_reference(capi):
    fc = capi.field_cfg(encoding="fourier", dim_enc=64, num_layers=2)
    shapes = capi.param_shapes(fc)
    assert shapes == {"_encoding._linear.weight": (61, 3), "_linears.0.weight": (64, 64), "_linears.0.bias": (64,),
                      "_linears.1.weight": (64, 64), "_linears.1.bias": (64,), "_linears.2.weight": (4, 64),
                      "_linears.2.bias": (4,)}          # SURVEY 8b, observed on the reference
    from oracle import ngm_oracle as O
    assert O.FieldSpec(encoding="fourier", dim_enc=64, num_layers=2).param_shapes() == shapes
    fcn = capi.field_cfg(encoding="nerf", num_octaves=8, num_layers=1)
    assert fcn.dim_enc == 48 and capi.param_shapes(fcn)["_linears.0.weight"] == (48, 48)


def test_ops_refuse_cpu_tensors(capi):
    from neural_graph_mapping_amd import ops
    fc = capi.field_cfg()
    params = {n: torch.zeros(1, *s) for n, s in capi.param_shapes(fc).items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.field_eval(fc, params, torch.zeros(1, 8, 3))
    rc = capi.render_cfg()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.quadrature(rc, torch.zeros(2, 4, 3), torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, 4))


def test_missing_library_fails_loudly(capi, monkeypatch):
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", "/nonexistent/libngm_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        capi.lib()


def test_ops_are_registered_with_the_dispatcher(capi):
    """north_star: "a thin C-ABI exposed as PyTorch-ROCm custom ops" -- every op is a torch.library op of namespace
    ngm355 (schema + fake shapes + autograd formula) with a ROCm ("cuda") kernel only: no CPU registration."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from neural_graph_mapping_amd import mesh, ops  # noqa: F401
    names = {"sample_rays", "field_eval", "field_eval_bwd", "field_eval_train", "field_eval_bwd_stash", "field_eval_knn", "quadrature", "quadrature_bwd",
             "composite_packed", "render_ijs", "render_ijs_bwd", "adam_sparse_", "marching_cubes", "render_eval_knn"}
    for n in names:
        assert hasattr(torch.ops.ngm355, n), n
    assert "Tensor(a0!) param" in str(torch.ops.ngm355.adam_sparse_.default._schema)        # declared as mutating
    assert "!) workspace" in str(torch.ops.ngm355.render_ijs_bwd.default._schema)
    fc, rc = capi.field_cfg(), capi.render_cfg(num_samples_coarse=4, num_samples_guided=0)
    params = [torch.zeros(1, *s) for s in capi.param_shapes(fc).values()]
    with pytest.raises(NotImplementedError):                                                # dispatcher: no CPU kernel
        torch.ops.ngm355.field_eval(ops.cfg_blob(fc), torch.zeros(1, 8, 3), None, None, params)
    # shape inference without a device (what torch.compile / export see)
    with FakeTensorMode(allow_non_fake_inputs=True):
        g = torch.empty(6, 4, device="cuda")
        out = torch.ops.ngm355.quadrature(ops.cfg_blob(rc), torch.empty(6, 4, 3, device="cuda"), g, g, g, None, 4)
        assert [tuple(o.shape) for o in out] == [(6, 3), (6,), (6, 3), (6,), (6,), (6, 4)]
        ij = torch.empty(2, 5, 2, dtype=torch.int64, device="cuda")
        out = torch.ops.ngm355.sample_rays(ops.cfg_blob(rc), ij, None, None, None, None, None, None, 0, 0.0, 8.0, 4)
        assert [tuple(o.shape) for o in out] == [(2, 5, 4, 3), (0,), (2, 5, 4), (2, 5, 3)]
        o = torch.ops.ngm355.field_eval(ops.cfg_blob(fc), torch.empty(1, 8, 3, device="cuda"), None, None,
                                        [torch.empty(p.shape, device="cuda") for p in params])
        assert tuple(o.shape) == (1, 8, 4)
        ij1 = torch.empty(7, 2, dtype=torch.int64, device="cuda")
        e4 = torch.empty(4, 4, device="cuda")
        out = torch.ops.ngm355.render_eval_knn(ops.cfg_blob(fc), ops.cfg_blob(rc), ij1, e4, None, None, None, 0, 0.0, 8.0,
                                               torch.empty(3, 3, device="cuda"), torch.empty(3, 4, device="cuda"),
                                               [torch.empty(p.shape, device="cuda") for p in params], 2, 10.0, 1.0, None, 0.0, 8192)
        assert [tuple(o.shape) for o in out] == [(7, 4), (7, 3), (7,), (7,)]


def test_graft_entry_build_passes():
    """the driver's "does it build" check: __graft_entry__.build() compiles (cached here), loads the library and compares
    its ABI version with the header's -- a hard-coded number there once went stale across two ABI bumps unnoticed"""
    import importlib
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    ge = importlib.import_module("__graft_entry__")
    ge.build()

"""Dump what the host-side planning decides, without a GPU: ngm_render_workspace (inference and training) and the
ngm_debug_plan_bwd tuple over every entry of tests/_config_matrix.py x matmul mode x geometry mode x batch shape.

    python tools/plan_dump.py > plan.txt

Run in two checkouts (before / after a change to the planning code) and diff the outputs: a refactor leaves them identical."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _config_matrix as CM                               # noqa: E402
from neural_graph_mapping_amd import _capi as K           # noqa: E402

MODES = ("f32", "auto", "bf16x3")
GEOMETRIES = ("nrgbd", "density", "neus")
FS = (1, 2, 4, 8, 32)
RS = (1, 7, 8, 33, 512)
SAMPLES = ((5, 2), (8, 16), (64, 64), (256, 0))


def main():
    L = K.lib()
    out = (C.c_int32 * 5)()
    for e in CM.ENTRIES:
        for mode in MODES:
            fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
            for geo in GEOMETRIES:
                for n_c, n_g in SAMPLES:
                    rc = K.render_cfg(geometry_mode=geo, num_samples_coarse=n_c, num_samples_guided=n_g)
                    for F in FS:
                        for R in RS:
                            ws = [L.ngm_render_workspace(C.byref(fc), C.byref(rc), F, R, train) for train in (0, 1)]
                            row = []
                            for guided in (0, 1):
                                for i in range(5):
                                    out[i] = -9
                                status = L.ngm_debug_plan_bwd(C.byref(fc), C.byref(rc), F, R, guided, 0, 1, out)
                                row.append((status,) + tuple(out))
                            print(e["name"], mode, geo, n_c, n_g, F, R, *ws, *row)


if __name__ == "__main__":
    main()
